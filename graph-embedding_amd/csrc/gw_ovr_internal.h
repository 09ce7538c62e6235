// gw_ovr handle shared by gw_ovr_host.cpp (C ABI, checks, host law) and
// gw_ovr.hip (kernels).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/graphwalk.h"
#include "gw_ovr_law.h"

struct gw_ovr {
  int device = -1;  // -1: host evaluation
  gw_ovr_params_t p{};
  int64_t n = 0;
  int L = 0, D = 0;  // labels, dim + 1
  const float* x = nullptr;  // caller's features (host or device memory)
  int64_t pitch = 0;
  bool have_x = false, have_y = false, fitted = false;
  std::vector<int64_t> row_off;  // [n + 1]
  std::vector<int32_t> ids;      // [nnz]
  // per-label solver state and results (host copies on both paths after a fit)
  std::vector<gw_ovr_label> lab;  // [L]
  std::vector<double> W;          // [L][D]
  struct gw_ovr_dev* dev = nullptr;  // device state (device >= 0), defined and owned by gw_ovr.hip
  std::string err;
};

int gw_ovr_fail(gw_ovr* m, int code, const char* fmt, ...);
inline auto gw_fail_of(const gw_ovr*) { return &gw_ovr_fail; }  // for the shared device plumbing

// device entry points (gw_ovr.hip)
int gw_ovr_dev_alloc(gw_ovr* m);
void gw_ovr_dev_free(gw_ovr* m);
int gw_ovr_dev_upload_labels(gw_ovr* m);
// y: [T][L] 0/1 of the gathered rows; m->lab holds the initial states; fills m->lab and m->W
int gw_ovr_dev_fit(gw_ovr* m, const int64_t* rows, int64_t T, const uint8_t* y, int64_t* passes, void* stream);
int gw_ovr_dev_score(gw_ovr* m, const int64_t* rows, int64_t count, int64_t* counts, void* stream);
int gw_ovr_dev_decision(gw_ovr* m, const int64_t* rows, int64_t count, double* z);
