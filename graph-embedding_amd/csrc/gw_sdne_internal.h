// gw_sdne handle shared by gw_sdne_host.cpp (C ABI, argument checks, init, host
// law) and gw_sdne.hip (kernels).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/graphwalk.h"

struct gw_sdne {
  int device = -1;  // -1: host evaluation
  gw_sdne_params_t p{};
  int u[5] = {0, 0, 0, 0, 0};
  int B = 0;
  // rows: dense (the caller's matrix, host or device memory) or CSR (host copy, always kept)
  int64_t N = 0;
  bool have_rows = false, sparse = false;
  const float* rows = nullptr;
  int64_t pitch = 0;
  std::vector<int64_t> offs;
  std::vector<int32_t> cols;
  std::vector<float> vals;
  // host state (device = -1): tensor t = 2 * layer + (0 weight | 1 bias)
  std::vector<float> par[8], am[8], av[8];
  std::vector<float> enc;               // [N][u2], host path
  struct gw_sdne_dev* dev = nullptr;    // device state (device >= 0), defined and owned by gw_sdne.hip
  std::string err;
};

int gw_sdne_fail(gw_sdne* m, int code, const char* fmt, ...);
inline auto gw_fail_of(const gw_sdne*) { return &gw_sdne_fail; }  // for the shared device plumbing
inline size_t gw_sdne_numel(const gw_sdne* m, int t) {
  const int l = t >> 1;
  return t & 1 ? (size_t)m->u[l + 1] : (size_t)m->u[l] * (size_t)m->u[l + 1];
}

// device entry points (gw_sdne.hip)
int gw_sdne_dev_alloc(gw_sdne* m, const std::vector<float> init[8]);
void gw_sdne_dev_free(gw_sdne* m);
int gw_sdne_dev_set_rows(gw_sdne* m);  // after the handle's row fields are set: upload the CSR, size the encoding
int gw_sdne_dev_train(gw_sdne* m, int64_t step_begin, int64_t step_count, double* loss_out, void* stream);
int gw_sdne_dev_gradients(gw_sdne* m, int64_t step, float* const grads[8]);
int gw_sdne_dev_batch_rows(gw_sdne* m, int64_t step, int64_t* rows);  // stages step's batch, copies its row ids back
int gw_sdne_dev_encode(gw_sdne* m, int64_t row_begin, int64_t row_count, float* out);
int gw_sdne_dev_export(gw_sdne* m, float* const par[8], float* const am[8], float* const av[8]);
float* gw_sdne_dev_vectors(gw_sdne* m);  // the encoding in device memory, [N][u2]
