// gw_nng handle shared by gw_nng_host.cpp (C ABI, checks, host law) and
// gw_nng.hip (kernels).
#pragma once
#include <stdint.h>

#include "gw_nng_law.h"
#include "gw_pairs_host.h"

struct gw_nng : gw_pairs_handle {
  gw_nng_params_t p{};
  struct gw_nng_dev* dev = nullptr;  // device state (device >= 0), defined and owned by gw_nng.hip
};

int gw_nng_fail(gw_nng* m, int code, const char* fmt, ...);
inline auto gw_fail_of(const gw_nng*) { return &gw_nng_fail; }  // for the shared plumbing (gw_pairs_host.h, gw_pairs_topk.h)

// device entry points (gw_nng.hip)
int gw_nng_dev_alloc(gw_nng* m);
void gw_nng_dev_free(gw_nng* m);
// sources (device memory, or NULL for 0 .. n-1) are range-checked on the device before anything is written;
// out_d2 may be NULL
int gw_nng_dev_query(gw_nng* m, const int32_t* sources, int64_t nsrc, int32_t* out_ids, double* out_weights,
                     double* out_d2, void* stream);
