// Spring-layout kernels (gfx950): the law of gw_layout_law.h.
//
//   k_layout_init     t0 and dt from the starting positions' extents; clears the stop flag and the iteration count
//   k_layout_pairs    the all-pairs repulsion.  Workgroup (x, y) owns kRows rows (one per thread) and the law's column
//                     chunk y: the chunk's positions go through LDS once, every thread reads them at the same address
//                     (a broadcast, no bank conflict) and keeps the law's GW_LAYOUT_STRANDS independent accumulators
//                     per coordinate.  Per pair: dim subtracts, the squares, one compare-select, one divide, dim
//                     multiplies and adds.  The chunk's sum goes to part[chunk][row][dim]: nothing of size n x n.
//   k_layout_update   one wave per row.  R_i = the row's chunk sums added ascending; the attraction: lane l takes the
//                     entry e0 + l of a 64-entry trip (gather, root, divide), then every lane adds the trip's terms in
//                     stored order, read lane by lane; then the length, the step, the fixed mask, nxt = pos + step and
//                     s_i, the vertex's share of the stop norm.
//   k_layout_commit   one workgroup: pos = nxt, the stop norm as the law's blocked sum (a thread per block, then one
//                     thread over the blocks), t -= dt, the iteration count, the stop flag.
//   k_layout_rescale  one workgroup: the blocked column sums, the means, max |pos|, the scale and the shift.
//
// The schedule of a run: init, then per iteration pairs, update, commit, back to back on the stream.  Every kernel
// of an iteration reads the stop flag first and exits when it is set, so nothing after the stopping iteration changes
// a byte.  The host reads the control words once at the end.
//
// Every loop runs over a chunk's columns, a row's entries, the chunks or blocks of n, or a strided range of n.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gw_layout_internal.h"
#include "gw_trainer_device.h"

namespace {

constexpr int kRows = 128;      // rows (threads) of a k_layout_pairs workgroup
constexpr int kUpdLanes = 256;  // threads of a k_layout_update workgroup: 4 rows
constexpr int kOneLanes = 1024; // threads of the single-workgroup kernels

struct LayoutCtl {
  double t, dt;
  int32_t stop, done;
};

template <int DIM>
struct Vec {
  double v[DIM];
};

__device__ __forceinline__ double lane_value(double x, int lane) {  // lane is wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
  return __hiloint2double(hi, lo);
}

template <int DIM>
__global__ __launch_bounds__(kOneLanes) void k_layout_init(const double* __restrict__ pos, int64_t n, int32_t iterations,
                                                           LayoutCtl* ctl) {
  __shared__ double s_m[4][kOneLanes / 64];
  double mn0 = pos[0], mx0 = pos[0], mn1 = pos[1], mx1 = pos[1];
  for (int64_t i = threadIdx.x; i < n; i += kOneLanes) {
    const double x = pos[i * DIM], y = pos[i * DIM + 1];
    mn0 = x < mn0 ? x : mn0;
    mx0 = x > mx0 ? x : mx0;
    mn1 = y < mn1 ? y : mn1;
    mx1 = y > mx1 ? y : mx1;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double a = __shfl_xor(mn0, o, 64), b = __shfl_xor(mx0, o, 64), c = __shfl_xor(mn1, o, 64),
                 d = __shfl_xor(mx1, o, 64);
    mn0 = a < mn0 ? a : mn0;
    mx0 = b > mx0 ? b : mx0;
    mn1 = c < mn1 ? c : mn1;
    mx1 = d > mx1 ? d : mx1;
  }
  if ((threadIdx.x & 63) == 0) {
    s_m[0][threadIdx.x >> 6] = mn0;
    s_m[1][threadIdx.x >> 6] = mx0;
    s_m[2][threadIdx.x >> 6] = mn1;
    s_m[3][threadIdx.x >> 6] = mx1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kOneLanes / 64; ++w) {
      mn0 = s_m[0][w] < mn0 ? s_m[0][w] : mn0;
      mx0 = s_m[1][w] > mx0 ? s_m[1][w] : mx0;
      mn1 = s_m[2][w] < mn1 ? s_m[2][w] : mn1;
      mx1 = s_m[3][w] > mx1 ? s_m[3][w] : mx1;
    }
    const double t0 = gw_layout_t0(mn0, mx0, mn1, mx1);
    ctl->t = t0;
    ctl->dt = t0 / (double)(iterations + 1);
    ctl->stop = 0;
    ctl->done = 0;
  }
}

template <int DIM>
__global__ __launch_bounds__(kRows) void k_layout_pairs(const double* __restrict__ pos, int64_t n, double kk,
                                                        double* __restrict__ part, const LayoutCtl* ctl) {
  __shared__ double s_cols[GW_LAYOUT_CHUNK * DIM];
  if (ctl && ctl->stop) return;
  const int64_t c0 = (int64_t)blockIdx.y * GW_LAYOUT_CHUNK;
  const int m = (int)(n - c0 < GW_LAYOUT_CHUNK ? n - c0 : GW_LAYOUT_CHUNK);
  for (int x = threadIdx.x; x < m * DIM; x += kRows) s_cols[x] = pos[c0 * DIM + x];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x;
  if (i >= n) return;
  double pi[DIM], out[DIM];
#pragma unroll
  for (int c = 0; c < DIM; ++c) pi[c] = pos[i * DIM + c];
  gw_layout_chunk<DIM>(pi, s_cols, m, kk, out);
#pragma unroll
  for (int c = 0; c < DIM; ++c) part[((int64_t)blockIdx.y * n + i) * DIM + c] = out[c];
}

template <int DIM>
__global__ __launch_bounds__(kUpdLanes) void k_layout_update(const double* __restrict__ pos, int64_t n, int64_t chunks,
                                                             const double* __restrict__ part,
                                                             const int64_t* __restrict__ off,
                                                             const int32_t* __restrict__ col,
                                                             const double* __restrict__ val,
                                                             const uint8_t* __restrict__ fixed, double k, double t_arg,
                                                             const LayoutCtl* ctl, double* __restrict__ disp_out,
                                                             double* __restrict__ nxt, double* __restrict__ s) {
  if (ctl && ctl->stop) return;
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (kUpdLanes / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (i >= n) return;
  const double t = ctl ? ctl->t : t_arg;
  double pi[DIM], R[DIM], T[DIM], term[DIM], disp[DIM], step[DIM];
#pragma unroll
  for (int c = 0; c < DIM; ++c) {
    pi[c] = pos[i * DIM + c];
    R[c] = T[c] = 0.0;
  }
  for (int64_t ch = 0; ch < chunks; ++ch) {
#pragma unroll
    for (int c = 0; c < DIM; ++c) R[c] = R[c] + part[(ch * n + i) * DIM + c];
  }
  const int64_t e1 = off[i + 1];
  for (int64_t e0 = off[i]; e0 < e1; e0 += 64) {
    const int cnt = (int)(e1 - e0 < 64 ? e1 - e0 : 64);
#pragma unroll
    for (int c = 0; c < DIM; ++c) term[c] = 0.0;
    if (lane < cnt) {
      const int64_t j = col[e0 + lane];
      double pj[DIM];
#pragma unroll
      for (int c = 0; c < DIM; ++c) pj[c] = pos[j * DIM + c];
      gw_layout_pull<DIM>(pi, pj, val[e0 + lane], k, term);
    }
    for (int q = 0; q < cnt; ++q) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) T[c] = T[c] + lane_value(term[c], q);
    }
  }
  const double si = gw_layout_move<DIM>(R, T, t, fixed[i], disp, step);
  if (lane == 0) {
    if (s) s[i] = si;
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      if (disp_out) disp_out[i * DIM + c] = disp[c];
      nxt[i * DIM + c] = pi[c] + step[c];
    }
  }
}

__global__ __launch_bounds__(kOneLanes) void k_layout_commit(double* __restrict__ pos, const double* __restrict__ nxt,
                                                             int64_t n, int dim, const double* __restrict__ s,
                                                             double* __restrict__ bsum, double threshold,
                                                             LayoutCtl* ctl) {
  if (ctl->stop) return;
  const int64_t blocks = (n + GW_LAYOUT_BLOCK - 1) / GW_LAYOUT_BLOCK;
  for (int64_t x = threadIdx.x; x < n * dim; x += kOneLanes) pos[x] = nxt[x];
  for (int64_t b = threadIdx.x; b < blocks; b += kOneLanes) bsum[b] = gw_layout_block_sum(s, 1, b, n);
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int64_t b = 0; b < blocks; ++b) total = total + bsum[b];
    ctl->t = ctl->t - ctl->dt;
    ctl->done = ctl->done + 1;
    if (gw_layout_stops(total, n, threshold)) ctl->stop = 1;
  }
}

template <int DIM>
__global__ __launch_bounds__(kOneLanes) void k_layout_rescale(double* __restrict__ pos, int64_t n,
                                                              double* __restrict__ bsum, double scale, Vec<DIM> center) {
  __shared__ double s_mean[DIM];
  __shared__ double s_lim[kOneLanes / 64];
  const int64_t blocks = (n + GW_LAYOUT_BLOCK - 1) / GW_LAYOUT_BLOCK;
  for (int64_t x = threadIdx.x; x < blocks * DIM; x += kOneLanes) {
    const int64_t b = x / DIM;
    const int c = (int)(x - b * DIM);
    bsum[x] = gw_layout_block_sum(pos + c, DIM, b, n);
  }
  __syncthreads();
  if (threadIdx.x < DIM) {
    double total = 0.0;
    for (int64_t b = 0; b < blocks; ++b) total = total + bsum[b * DIM + threadIdx.x];
    s_mean[threadIdx.x] = total / (double)n;
  }
  __syncthreads();
  double lim = 0.0;
  for (int64_t x = threadIdx.x; x < n * DIM; x += kOneLanes) {
    const double v = pos[x] - s_mean[x % DIM];
    pos[x] = v;
    const double a = v < 0.0 ? -v : v;
    lim = a > lim ? a : lim;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double a = __shfl_xor(lim, o, 64);
    lim = a > lim ? a : lim;
  }
  if ((threadIdx.x & 63) == 0) s_lim[threadIdx.x >> 6] = lim;
  __syncthreads();
  lim = s_lim[0];
  for (int w = 1; w < kOneLanes / 64; ++w) lim = s_lim[w] > lim ? s_lim[w] : lim;
  const double f = lim > 0.0 ? scale / lim : 1.0;
  for (int64_t x = threadIdx.x; x < n * DIM; x += kOneLanes) {  // a thread rereads only what it wrote itself
    const double v = lim > 0.0 ? pos[x] * f : pos[x];
    pos[x] = v + center.v[x % DIM];
  }
}

}  // namespace

// Device state of a gw_layout handle (device >= 0); the buffers are freed with it.
struct gw_layout_dev {
  gw_dev_buf<int64_t> off;
  gw_dev_buf<int32_t> col;
  gw_dev_buf<double> val;
  gw_dev_buf<uint8_t> fixed;
  gw_dev_buf<double> part;  // [chunks][n][dim]: grows as n * n / 1024 (DESIGN.md §20 has the ceiling)
  gw_dev_buf<double> nxt;   // [n][dim]
  gw_dev_buf<double> s;     // [n]
  gw_dev_buf<double> bsum;  // [blocks][dim]
  gw_dev_buf<LayoutCtl> ctl;
};

int gw_layout_dev_alloc(gw_layout* m) {
  const int rc = gw_trainer_open_device(m);
  if (rc != GW_OK) return rc;
  GW_DEV_GUARD(m);
  gw_layout_dev* d = m->dev;
  const int64_t n = m->n;
  GW_DEV_TRY(m, d->ctl.alloc(1));
  GW_DEV_TRY(m, d->fixed.alloc(n));
  GW_DEV_TRY(m, hipMemset(d->fixed.get(), 0, (size_t)n));
  GW_DEV_TRY(m, d->nxt.alloc(n * m->dim));
  GW_DEV_TRY(m, d->s.alloc(n));
  GW_DEV_TRY(m, d->bsum.alloc(gw_layout_blocks(n) * m->dim));
  if (d->part.alloc(gw_layout_chunks(n) * n * m->dim) != hipSuccess) {
    (void)hipGetLastError();
    return gw_layout_fail(m, GW_ERR_NOMEM, "no device memory for %lld chunk sums of %lld rows",
                          (long long)gw_layout_chunks(n), (long long)n);
  }
  return GW_OK;
}

void gw_layout_dev_free(gw_layout* m) {
  if (!m->dev) return;
  gw_device_guard g(m->device);
  delete m->dev;
  m->dev = nullptr;
}

int gw_layout_dev_upload(gw_layout* m) {
  GW_DEV_GUARD(m);
  gw_layout_dev* d = m->dev;
  const int64_t nnz = (int64_t)m->col.size();
  GW_DEV_TRY(m, d->off.grow(m->n + 1));
  GW_DEV_TRY(m, d->col.grow(nnz));
  GW_DEV_TRY(m, d->val.grow(nnz));
  GW_DEV_TRY(m, hipMemcpy(d->off.get(), m->off.data(), sizeof(int64_t) * (size_t)(m->n + 1), hipMemcpyHostToDevice));
  if (nnz) {
    GW_DEV_TRY(m, hipMemcpy(d->col.get(), m->col.data(), sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice));
    GW_DEV_TRY(m, hipMemcpy(d->val.get(), m->val.data(), sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice));
  }
  return GW_OK;
}

int gw_layout_dev_upload_fixed(gw_layout* m) {
  GW_DEV_GUARD(m);
  GW_DEV_TRY(m, hipMemcpy(m->dev->fixed.get(), m->fixed.data(), (size_t)m->n, hipMemcpyHostToDevice));
  return GW_OK;
}

namespace {

// pairs and update of one iteration; ctl NULL: temperature t, no stop flag (gw_layout_step)
template <int DIM>
int launch_iteration(gw_layout* m, const double* pos, double k, double t, const LayoutCtl* ctl, double* disp_out,
                     double* nxt, double* s, hipStream_t st) {
  gw_layout_dev* d = m->dev;
  const int64_t n = m->n, chunks = gw_layout_chunks(n);
  hipLaunchKernelGGL(k_layout_pairs<DIM>, dim3((unsigned)((n + kRows - 1) / kRows), (unsigned)chunks), dim3(kRows), 0,
                     st, pos, n, k * k, d->part.get(), ctl);
  GW_DEV_TRY(m, hipGetLastError());
  const int rows = kUpdLanes / 64;
  hipLaunchKernelGGL(k_layout_update<DIM>, dim3((unsigned)((n + rows - 1) / rows)), dim3(kUpdLanes), 0, st, pos, n,
                     chunks, d->part.get(), d->off.get(), d->col.get(), d->val.get(), d->fixed.get(), k, t, ctl,
                     disp_out, nxt, s);
  GW_DEV_TRY(m, hipGetLastError());
  return GW_OK;
}

template <int DIM>
int dev_run(gw_layout* m, double* pos, double k, int32_t iterations, double threshold, hipStream_t st,
            int32_t* iterations_done) {
  gw_layout_dev* d = m->dev;
  const int64_t n = m->n;
  LayoutCtl ctl;
  hipLaunchKernelGGL(k_layout_init<DIM>, dim3(1), dim3(kOneLanes), 0, st, pos, n, iterations, d->ctl.get());
  GW_DEV_TRY(m, hipGetLastError());
  for (int32_t it = 0; it < iterations; ++it) {
    const int rc = launch_iteration<DIM>(m, pos, k, 0.0, d->ctl.get(), nullptr, d->nxt.get(), d->s.get(), st);
    if (rc != GW_OK) return rc;
    hipLaunchKernelGGL(k_layout_commit, dim3(1), dim3(kOneLanes), 0, st, pos, d->nxt.get(), n, DIM, d->s.get(),
                       d->bsum.get(), threshold, d->ctl.get());
    GW_DEV_TRY(m, hipGetLastError());
  }
  GW_DEV_TRY(m, hipMemcpyAsync(&ctl, d->ctl.get(), sizeof ctl, hipMemcpyDeviceToHost, st));
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  if (iterations_done) *iterations_done = ctl.done;
  return GW_OK;
}

}  // namespace

int gw_layout_dev_run(gw_layout* m, double* pos, double k, int32_t iterations, double threshold, void* stream,
                      int32_t* iterations_done) {
  GW_DEV_GUARD(m);
  return m->dim == 2 ? dev_run<2>(m, pos, k, iterations, threshold, (hipStream_t)stream, iterations_done)
                     : dev_run<3>(m, pos, k, iterations, threshold, (hipStream_t)stream, iterations_done);
}

int gw_layout_dev_step(gw_layout* m, const double* pos_in, double k, double t, double* disp_out, double* pos_out,
                       void* stream) {
  GW_DEV_GUARD(m);
  hipStream_t st = (hipStream_t)stream;
  const int rc = m->dim == 2 ? launch_iteration<2>(m, pos_in, k, t, nullptr, disp_out, pos_out, nullptr, st)
                             : launch_iteration<3>(m, pos_in, k, t, nullptr, disp_out, pos_out, nullptr, st);
  if (rc != GW_OK) return rc;
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  return GW_OK;
}

int gw_layout_dev_rescale(gw_layout* m, double* pos, double scale, const double* center, void* stream) {
  GW_DEV_GUARD(m);
  hipStream_t st = (hipStream_t)stream;
  if (m->dim == 2) {
    Vec<2> c{{center ? center[0] : 0.0, center ? center[1] : 0.0}};
    hipLaunchKernelGGL(k_layout_rescale<2>, dim3(1), dim3(kOneLanes), 0, st, pos, m->n, m->dev->bsum.get(), scale, c);
  } else {
    Vec<3> c{{center ? center[0] : 0.0, center ? center[1] : 0.0, center ? center[2] : 0.0}};
    hipLaunchKernelGGL(k_layout_rescale<3>, dim3(1), dim3(kOneLanes), 0, st, pos, m->n, m->dev->bsum.get(), scale, c);
  }
  GW_DEV_TRY(m, hipGetLastError());
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  return GW_OK;
}

extern "C" int gw_layout_kernel_attrs(gw_layout* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                                      int32_t* lds_bytes, int32_t* count) {
  if (!m) return gw_layout_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (m->device < 0) return gw_layout_fail(m, GW_ERR_STATE, "host evaluation launches no kernel");
  GW_DEV_GUARD(m);
  const gw_kernel_entry ks[] = {{"k_layout_init_2", (const void*)k_layout_init<2>, 0},
                                {"k_layout_init_3", (const void*)k_layout_init<3>, 0},
                                {"k_layout_pairs_2", (const void*)k_layout_pairs<2>, 0},
                                {"k_layout_pairs_3", (const void*)k_layout_pairs<3>, 0},
                                {"k_layout_update_2", (const void*)k_layout_update<2>, 0},
                                {"k_layout_update_3", (const void*)k_layout_update<3>, 0},
                                {"k_layout_commit", (const void*)k_layout_commit, 0},
                                {"k_layout_rescale_2", (const void*)k_layout_rescale<2>, 0},
                                {"k_layout_rescale_3", (const void*)k_layout_rescale<3>, 0}};
  return gw_trainer_kernel_attrs(m, ks, cap, names, vgprs, scratch_bytes, lds_bytes, count);
}

extern "C" int gw_layout_tiles(const gw_layout* m, int32_t* rows, int32_t* chunk, int32_t* strands, int32_t* block) {
  if (!m) return gw_layout_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (rows) *rows = m->device >= 0 ? kRows : 0;
  if (chunk) *chunk = GW_LAYOUT_CHUNK;
  if (strands) *strands = GW_LAYOUT_STRANDS;
  if (block) *block = GW_LAYOUT_BLOCK;
  return GW_OK;
}
