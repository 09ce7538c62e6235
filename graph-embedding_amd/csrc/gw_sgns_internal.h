// gw_sgns handle shared by gw_sgns_host.cpp (C ABI, vocabulary, host law)
// and gw_sgns.hip (kernels).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/graphwalk.h"

struct gw_sgns {
  int device = -1;  // -1: host evaluation
  int64_t n = 0;
  gw_sgns_params_t p{};
  int pitch = 0;  // floats per row: 4*ceil(dim/4), pad kept at 0
  bool vocab = false;
  // host side (always filled by build_vocab)
  std::vector<int64_t> counts;
  std::vector<int32_t> J;
  std::vector<uint32_t> thr, keep_thr;
  std::vector<float> expt;
  std::vector<float> syn0, syn1;  // device = -1 only, [n][pitch]
  struct gw_sgns_dev* dev = nullptr;  // device state (device >= 0), defined and owned by gw_sgns.hip
  std::string err;
};

int gw_sgns_fail(gw_sgns* m, int code, const char* fmt, ...);
inline auto gw_fail_of(const gw_sgns*) { return &gw_sgns_fail; }  // for the shared device plumbing

// device entry points (gw_sgns.hip)
int gw_sgns_dev_alloc(gw_sgns* m);
void gw_sgns_dev_free(gw_sgns* m);
int gw_sgns_dev_count(gw_sgns* m, const int32_t* walks_dev, int64_t nwalks, int walk_len);  // -> m->counts
int gw_sgns_dev_upload_vocab(gw_sgns* m);                                                   // tables + init
int gw_sgns_dev_train(gw_sgns* m, const int32_t* walks_dev, int64_t nwalks, int walk_len, int epoch_begin,
                      int epoch_count, int concurrency, int64_t* stats, void* stream);
int gw_sgns_dev_export(gw_sgns* m, float* syn0, float* syn1neg);
float* gw_sgns_dev_vectors(gw_sgns* m);  // syn0 in device memory, [n][pitch]
int gw_sgns_auto_concurrency(const gw_sgns* m, int64_t nwalks);
