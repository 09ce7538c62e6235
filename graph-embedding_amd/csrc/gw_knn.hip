// Nearest-neighbour kernels (gfx950): the law of gw_knn_law.h.
//
//   k_knn_check   every source lies in [0, n): the first offending entry, by integer atomic min
//   k_knn_norms   nrm(j) = sqrt(dot(j,j)), one lane per row (GW_KNN_COSINE only)
//   k_knn_main    pairs_topk_main (gw_pairs_topk.h: the tiling, the selection and the launch plumbing
//                 shared with gw_nng.hip) under KnnLaw: fma steps, the source's norm as the row's
//                 double, cosine or dot scores, score descending, topk entries per row, written
//                 with the (-1, 0.0) padding.
//   k_knn_fma_calib  the rate ceiling of the main loop (gw_knn_fma_rate)
#include <hip/hip_runtime.h>

#include "gw_knn_internal.h"
#include "gw_pairs_topk.h"

using namespace gw_pairs;

// Device state of a gw_knn handle (device >= 0); the buffers are freed with it.
struct gw_knn_dev {
  gw_dev_buf<double> nrm;             // [n]
  gw_dev_buf<unsigned long long> bad;  // first source outside [0, n)
};

namespace {

// gw_knn_law.h for pairs_topk_main: the row double is the source's norm (cosine), the best entries are the largest
struct KnnLaw {
  static constexpr int kRowDoubles = 1, kMaxTopk = GW_KNN_MAX_TOPK;
  int metric;
  const double* nrm;  // [n], read under GW_KNN_COSINE only
  int32_t* out_ids;
  double* out_scores;
  __device__ double row_double(int32_t v) const { return (v >= 0 && metric == GW_KNN_COSINE) ? nrm[v] : 0.0; }
  __device__ static double step(double q, double c, double acc) { return GW_KNN_FMA(q, c, acc); }
  __device__ bool score(double dot, double nv, int32_t j, bool in, double* s) const {
    const double nj = (in && metric == GW_KNN_COSINE) ? nrm[j] : 0.0;
    *s = gw_knn_score(metric, dot, nv, nj);
    return gw_knn_listed(metric, *s, nv, nj);
  }
  __device__ static int before(double sa, int32_t ia, double sb, int32_t ib) { return gw_knn_before(sa, ia, sb, ib); }
  __device__ int keep(int topk) const { return topk; }
  __device__ void write(int64_t o, int t, int32_t, int cnt, const double* s, const int32_t* ids) const {
    out_ids[o + t] = t < cnt ? ids[t] : -1;
    out_scores[o + t] = t < cnt ? s[t] : 0.0;
  }
};

__global__ void k_knn_check(const int32_t* __restrict__ sources, int64_t nsrc, int n, unsigned long long* bad) {
  check_sources(sources, nsrc, n, bad);
}

__global__ void k_knn_norms(const float* __restrict__ x, int64_t pitch, int n, int dim, double* __restrict__ nrm) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  nrm[j] = gw_knn_nrm(x + j * pitch, dim);
}

__global__ __launch_bounds__(kThreads) void k_knn_main(const PairsArgs A, const KnnLaw L) { pairs_topk_main(A, L); }

}  // namespace

int gw_knn_dev_alloc(gw_knn* m) { return dev_alloc(m, k_knn_main); }

void gw_knn_dev_free(gw_knn* m) { dev_free(m); }

int gw_knn_dev_query(gw_knn* m, const int32_t* sources, int64_t nsrc, int32_t* out_ids, double* out_scores,
                     void* stream) {
  GW_DEV_GUARD(m);
  hipStream_t st = (hipStream_t)stream;
  PairsArgs A;
  const int rc = dev_begin_query(m, k_knn_check, sources, nsrc, st, &A);
  if (rc != GW_OK) return rc;
  if (m->p.metric == GW_KNN_COSINE) {
    if (m->dev->nrm.grow(m->n) != hipSuccess) return gw_knn_fail(m, GW_ERR_NOMEM, "device allocation failed");
    k_knn_norms<<<(unsigned)((m->n + 255) / 256), 256, 0, st>>>(m->x, m->pitch, A.n, A.dim, m->dev->nrm.get());
    GW_DEV_TRY(m, hipGetLastError());
  }
  return dev_run_main(m, k_knn_main, A, KnnLaw{m->p.metric, m->dev->nrm.get(), out_ids, out_scores}, st);
}

extern "C" int gw_knn_kernel_attrs(gw_knn* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                                   int32_t* lds_bytes, int32_t* count) {
  if (!m) return gw_knn_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (m->device < 0) return gw_knn_fail(m, GW_ERR_STATE, "host evaluation launches no kernel");
  GW_DEV_GUARD(m);
  const gw_kernel_entry ks[] = {{"k_knn_check", (const void*)k_knn_check, 0},
                                {"k_knn_norms", (const void*)k_knn_norms, 0},
                                {"k_knn_main", (const void*)k_knn_main, main_lds(m->p.topk, KnnLaw::kRowDoubles)}};
  return gw_trainer_kernel_attrs(m, ks, cap, names, vgprs, scratch_bytes, lds_bytes, count);
}

namespace {
// the rate ceiling of the main loop: 16 independent fp64 fma chains per lane, nothing else
__global__ __launch_bounds__(kThreads) void k_knn_fma_calib(double* out, int iters, double a, double b) {
  double acc[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) acc[u] = (double)(u + 1) + (double)threadIdx.x * 1e-3;
  for (int i = 0; i < iters; ++i)
#pragma unroll
    for (int u = 0; u < 16; ++u) acc[u] = GW_KNN_FMA(acc[u], a, b);
  double s = 0.0;
#pragma unroll
  for (int u = 0; u < 16; ++u) s = s + acc[u];
  out[(size_t)blockIdx.x * kThreads + threadIdx.x] = s;
}
}  // namespace

extern "C" int gw_knn_fma_rate(gw_knn* m, int blocks, int iters, double* fma_per_second) {
  if (!m || !fma_per_second || blocks < 1 || iters < 1) return gw_knn_fail(m, GW_ERR_INVALID, "bad arguments");
  if (m->device < 0) return gw_knn_fail(m, GW_ERR_STATE, "host evaluation launches no kernel");
  GW_DEV_GUARD(m);
  gw_dev_buf<double> out;
  if (out.alloc((int64_t)blocks * kThreads) != hipSuccess) return gw_knn_fail(m, GW_ERR_NOMEM, "device allocation failed");
  hipEvent_t e0, e1;
  GW_DEV_TRY(m, hipEventCreate(&e0));
  GW_DEV_TRY(m, hipEventCreate(&e1));
  k_knn_fma_calib<<<blocks, kThreads>>>(out.get(), iters, 0.999999, 1e-6);  // warm-up
  hipError_t e = hipEventRecord(e0, nullptr);
  k_knn_fma_calib<<<blocks, kThreads>>>(out.get(), iters, 0.999999, 1e-6);
  if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  if (e == hipSuccess) e = hipGetLastError();
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  GW_DEV_TRY(m, e);
  *fma_per_second = (double)blocks * kThreads * 16.0 * (double)iters / ((double)ms * 1e-3);
  return GW_OK;
}

extern "C" int gw_knn_tiles(const gw_knn* m, int32_t* tq, int32_t* tc, int32_t* kc, int32_t* buf) {
  return tiles(m, tq, tc, kc, buf);
}
