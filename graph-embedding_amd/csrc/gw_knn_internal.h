// gw_knn handle shared by gw_knn_host.cpp (C ABI, checks, host law) and
// gw_knn.hip (kernels).
#pragma once
#include <stdint.h>

#include "gw_knn_law.h"
#include "gw_pairs_host.h"

struct gw_knn : gw_pairs_handle {
  gw_knn_params_t p{};
  struct gw_knn_dev* dev = nullptr;  // device state (device >= 0), defined and owned by gw_knn.hip
};

int gw_knn_fail(gw_knn* m, int code, const char* fmt, ...);
inline auto gw_fail_of(const gw_knn*) { return &gw_knn_fail; }  // for the shared plumbing (gw_pairs_host.h, gw_pairs_topk.h)

// device entry points (gw_knn.hip)
int gw_knn_dev_alloc(gw_knn* m);
void gw_knn_dev_free(gw_knn* m);
// sources (device memory, or NULL for 0 .. n-1) are range-checked on the device before anything is written
int gw_knn_dev_query(gw_knn* m, const int32_t* sources, int64_t nsrc, int32_t* out_ids, double* out_scores,
                     void* stream);
