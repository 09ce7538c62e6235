// Neighbour-graph kernels (gfx950): the law of gw_nng_law.h.
//
//   k_nng_check   every source lies in [0, n): the first offending entry, by integer atomic min
//   k_nng_main    pairs_topk_main (gw_pairs_topk.h: the tiling, the selection and the launch plumbing
//                 shared with gw_knn.hip) under NngLaw: one subtract and one fma per pair and
//                 column, no row double, d2 ascending, topk - include_self others per row; the
//                 epilogue turns d2 into the heat weight and writes the row, the source itself
//                 first under include_self, with the (-1, 0.0) padding.
#include <hip/hip_runtime.h>

#include "gw_nng_internal.h"
#include "gw_pairs_topk.h"

using namespace gw_pairs;

// Device state of a gw_nng handle (device >= 0); the buffer is freed with it.
struct gw_nng_dev {
  gw_dev_buf<unsigned long long> bad;  // first source outside [0, n)
};

namespace {

// gw_nng_law.h for pairs_topk_main: no row double, the best entries are the nearest, the source leads its row
struct NngLaw {
  static constexpr int kRowDoubles = 0, kMaxTopk = GW_NNG_MAX_TOPK;
  int include_self;
  double heat_t;
  int32_t* out_ids;
  double* out_weights;
  double* out_d2;  // may be NULL
  __device__ double row_double(int32_t) const { return 0.0; }
  __device__ static double step(double q, double c, double acc) { return gw_nng_step(q, c, acc); }
  __device__ bool score(double d2, double, int32_t, bool, double* s) const {
    *s = d2;
    return gw_nng_listed(d2);
  }
  __device__ static int before(double da, int32_t ia, double db, int32_t ib) { return gw_nng_before(da, ia, db, ib); }
  // others listed per row; 0 (topk = 1 with the source itself): no candidate is read
  __device__ int keep(int topk) const { return topk - include_self; }
  __device__ void write(int64_t o, int t, int32_t v, int cnt, const double* s, const int32_t* ids) const {
    int32_t id = -1;
    double d2 = 0.0, w = 0.0;
    if (include_self && t == 0) {
      id = v;
      w = 1.0;
    } else if (t - include_self < cnt) {
      id = ids[t - include_self];
      d2 = s[t - include_self];
      w = gw_nng_weight(d2, heat_t);
    }
    out_ids[o + t] = id;
    out_weights[o + t] = w;
    if (out_d2) out_d2[o + t] = d2;
  }
};

__global__ void k_nng_check(const int32_t* __restrict__ sources, int64_t nsrc, int n, unsigned long long* bad) {
  check_sources(sources, nsrc, n, bad);
}

__global__ __launch_bounds__(kThreads) void k_nng_main(const PairsArgs A, const NngLaw L) { pairs_topk_main(A, L); }

}  // namespace

int gw_nng_dev_alloc(gw_nng* m) { return dev_alloc(m, k_nng_main); }

void gw_nng_dev_free(gw_nng* m) { dev_free(m); }

int gw_nng_dev_query(gw_nng* m, const int32_t* sources, int64_t nsrc, int32_t* out_ids, double* out_weights,
                     double* out_d2, void* stream) {
  GW_DEV_GUARD(m);
  hipStream_t st = (hipStream_t)stream;
  PairsArgs A;
  const int rc = dev_begin_query(m, k_nng_check, sources, nsrc, st, &A);
  if (rc != GW_OK) return rc;
  return dev_run_main(m, k_nng_main, A, NngLaw{m->p.include_self, m->p.heat_t, out_ids, out_weights, out_d2}, st);
}

extern "C" int gw_nng_kernel_attrs(gw_nng* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                                   int32_t* lds_bytes, int32_t* count) {
  if (!m) return gw_nng_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (m->device < 0) return gw_nng_fail(m, GW_ERR_STATE, "host evaluation launches no kernel");
  GW_DEV_GUARD(m);
  const gw_kernel_entry ks[] = {{"k_nng_check", (const void*)k_nng_check, 0},
                                {"k_nng_main", (const void*)k_nng_main, main_lds(m->p.topk, NngLaw::kRowDoubles)}};
  return gw_trainer_kernel_attrs(m, ks, cap, names, vgprs, scratch_bytes, lds_bytes, count);
}

extern "C" int gw_nng_tiles(const gw_nng* m, int32_t* tq, int32_t* tc, int32_t* kc, int32_t* buf) {
  return tiles(m, tq, tc, kc, buf);
}
