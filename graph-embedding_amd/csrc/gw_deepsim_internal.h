// gw_deepsim handle shared by gw_deepsim_host.cpp (C ABI, table build, init,
// host law, writer) and gw_deepsim.hip (kernels).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/graphwalk.h"

struct gw_deepsim {
  int device = -1;  // -1: host evaluation
  gw_deepsim_params_t p{};
  int64_t V = 0;
  int W = 0;       // 2*window+1
  int ntiles = 0;  // ceil(V / GW_DS_TW)
  // table (host copy, always kept): rows of `topk` entries, the first tab_cnt[v] sorted by id
  int topk = 0;
  bool have_tab = false, have_walks = false;
  std::vector<int32_t> tab_id, tab_cnt;
  std::vector<float> tab_val, tem;
  // corpus
  const int32_t* walks = nullptr;  // caller's matrix (host or device memory)
  int64_t nwalks = 0;
  int walk_len = 0;
  bool has_labels = false;
  std::vector<int64_t> labels;
  std::vector<int64_t> elig;  // eligible walk indices, ascending
  std::vector<int32_t> elig_len;
  // host state (device = -1): par/am/av = {w1, b1, w2, b2}
  std::vector<float> par[4], am[4], av[4];
  struct gw_deepsim_dev* dev = nullptr;  // device state (device >= 0), defined and owned by gw_deepsim.hip
  std::string err;
};

int gw_deepsim_fail(gw_deepsim* m, int code, const char* fmt, ...);
inline auto gw_fail_of(const gw_deepsim*) { return &gw_deepsim_fail; }  // for the shared device plumbing
inline size_t gw_ds_numel(const gw_deepsim* m, int t) {
  return t == 0 || t == 2 ? (size_t)m->V * (size_t)m->p.dim : (t == 1 ? (size_t)m->p.dim : (size_t)m->V);
}

// device entry points (gw_deepsim.hip)
int gw_ds_dev_alloc(gw_deepsim* m, const std::vector<float> init[4]);
void gw_ds_dev_free(gw_deepsim* m);
int gw_ds_dev_fetch_table(gw_deepsim* m, const int32_t* ids_dev, const double* scores_dev, int topk,
                          std::vector<int32_t>* ids, std::vector<double>* scores);
int gw_ds_dev_upload_table(gw_deepsim* m);
// len[w] of every walk (label map applied to check the range); GW_ERR_RANGE on a bad token
int gw_ds_dev_scan_walks(gw_deepsim* m, std::vector<int32_t>* len);
int gw_ds_dev_upload_elig(gw_deepsim* m);
int gw_ds_dev_train(gw_deepsim* m, int64_t step_begin, int64_t step_count, double* loss_out, void* stream);
int gw_ds_dev_gradients(gw_deepsim* m, int64_t step, float* gw1, float* gb1, float* gw2, float* gb2);
int gw_ds_dev_batch(gw_deepsim* m, int64_t step, int32_t* centre, int32_t* tgt_id, float* tgt_val, int32_t* tgt_n,
                    float* ysum);
int gw_ds_dev_export(gw_deepsim* m, float* const par[4], float* const am[4], float* const av[4]);
float* gw_ds_dev_vectors(gw_deepsim* m);  // w1 in device memory, [V][dim]
