// One-vs-rest scorer kernels (gfx950): the law of gw_ovr_law.h.
//
// A fit is a loop of shared passes on the caller's stream; after each pass the
// per-label states (a few bytes each) come back to the host, which stops when
// no label runs any more:
//   k_ovr_pass     one workgroup per (block of 64 gathered rows, chunk of 32 labels): the
//                  directions of the chunk's running labels tile by tile in LDS (fp64), the
//                  rows tile by tile in LDS (fp32, 16 B reads), t = x~.v in registers,
//                  the coefficient (sigma(t) - y, or D t), then coefficient * x~ summed over
//                  the block's rows into the block's partial
//   k_ovr_reduce   q = the partials added in block order
//   k_ovr_step     one workgroup per running label: its vectors into LDS, the law's own
//                  transition (gw_ovr_label_step) on one lane, the vectors back
// Scoring: k_ovr_decision (z = w.x~, +-inf for a constant label), k_ovr_count (top-k rule
// by rank, tp / fp / fn with integer atomics).
// No float atomics and no MFMA: every sum has the law's order, so two runs give the same
// bits and the host evaluation gives them too.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gw_ovr_internal.h"
#include "gw_trainer_device.h"

// Device state of a gw_ovr handle (device >= 0); the buffers are freed with it.
struct gw_ovr_dev {
  gw_dev_buf<int64_t> row_off;
  gw_dev_buf<int32_t> ids;
  gw_dev_buf<int64_t> rows;  // gathered row list of the running call
  gw_dev_buf<uint8_t> y;     // [T][L]
  gw_dev_buf<double> z;      // [T][L] z, then [T][L] D; decision values when scoring
  gw_dev_buf<double> part;   // [blocks][L][D]
  gw_dev_buf<double> vec;    // 7 x [L][D]: q, w, wt, g, sv, r, p
  gw_dev_buf<gw_ovr_label> lab;
  gw_dev_buf<int64_t> counts;  // [L][3]
};

namespace {

constexpr int kRB = GW_OVR_RB;  // rows per workgroup = the law's partial block
constexpr int kLC = 32;         // labels per workgroup
constexpr int kLT = 8;          // labels per lane (kLC / 4 waves)
constexpr int kJT = 64;         // columns per LDS tile
constexpr int kThreads = 256;
constexpr int kXsPitch = kJT + 1;  // lanes along the rows read a column conflict-free
constexpr int kCsPitch = kLC + 1;
static_assert(kRB == 64 && kLC == 4 * kLT && kThreads == 4 * kRB && kJT == 64, "the lane maps below");

struct OvrArgs {
  const float* x;
  int64_t pitch;
  int vec16;  // rows are 16 B aligned: whole chunks are read as float4
  const int64_t* rows;
  int64_t T;
  int L, D;
  const uint8_t* y;
  double* z;
  double* Dd;
  double* part;
  double* vec;  // 7 x [L][D]: q, w, wt, g, sv, r, p
  gw_ovr_label* lab;
};

// rows [i0, i0 + rn) x columns [j0, j0 + jn) of the gathered features into xs; nothing past dim is read
__device__ __forceinline__ void load_x_tile(const OvrArgs& A, int64_t i0, int rn, int j0, int d, float* xs, int tid) {
  for (int idx = tid; idx < kRB * (kJT / 4); idx += kThreads) {
    const int rr = idx / (kJT / 4), j = j0 + (idx % (kJT / 4)) * 4;
    if (rr >= rn || j >= d) continue;
    const float* src = A.x + A.rows[i0 + rr] * A.pitch + j;
    float* dst = xs + rr * kXsPitch + (j - j0);
    if (A.vec16 && j + 3 < d) {
      const float4 v = *reinterpret_cast<const float4*>(src);
      dst[0] = v.x;
      dst[1] = v.y;
      dst[2] = v.z;
      dst[3] = v.w;
    } else {
      for (int u = 0; u < 4 && j + u < d; ++u) dst[u] = src[u];
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_ovr_pass(const OvrArgs A) {
  __shared__ float xs[kRB * kXsPitch];
  __shared__ double vs[kLC * kJT];
  __shared__ double cs[kRB * kCsPitch];
  __shared__ int modes[kLC];
  const int tid = threadIdx.x, lane = tid & 63, lg = tid >> 6;
  const int L = A.L, D = A.D, d = D - 1;
  const int64_t b = blockIdx.x, i0 = b * kRB;
  const int rn = (int)(A.T - i0 < kRB ? A.T - i0 : kRB);
  const int l0 = blockIdx.y * kLC;
  const int ln = L - l0 < kLC ? L - l0 : kLC;
  if (tid < kLC) modes[tid] = tid < ln ? A.lab[l0 + tid].mode : GW_OVR_MODE_IDLE;
  __syncthreads();
  int any = 0;
  for (int ll = 0; ll < kLC; ++ll) any |= modes[ll];
  if (!any) return;  // uniform: every label of the chunk is frozen
  const size_t LD = (size_t)L * D;
  // t = x~.v of row `lane` for the labels lg * kLT .. + kLT
  double t[kLT];
#pragma unroll
  for (int u = 0; u < kLT; ++u) t[u] = 0.0;
  for (int j0 = 0; j0 < d; j0 += kJT) {
    const int jn = d - j0 < kJT ? d - j0 : kJT;
    __syncthreads();
    load_x_tile(A, i0, rn, j0, d, xs, tid);
    for (int idx = tid; idx < kLC * kJT; idx += kThreads) {
      const int ll = idx / kJT, jj = idx % kJT;
      if (ll < ln && jj < jn && modes[ll])
        vs[idx] = A.vec[(modes[ll] == GW_OVR_MODE_GRAD ? 2 : 6) * LD + (size_t)(l0 + ll) * D + j0 + jj];
    }
    __syncthreads();
    if (lane < rn) {
      for (int jj = 0; jj < jn; ++jj) {
        const double xv = (double)xs[lane * kXsPitch + jj];
#pragma unroll
        for (int u = 0; u < kLT; ++u) t[u] = GW_OVR_FMA(xv, vs[(lg * kLT + u) * kJT + jj], t[u]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kLT; ++u) {
    const int ll = lg * kLT + u;
    if (lane < rn && ll < ln && modes[ll]) {  // ll, modes: wave-uniform
      const int l = l0 + ll;
      const double vd = A.vec[(modes[ll] == GW_OVR_MODE_GRAD ? 2 : 6) * LD + (size_t)l * D + d];
      const size_t at = (size_t)(i0 + lane) * L + l;
      cs[lane * kCsPitch + ll] = gw_ovr_coef(modes[ll], t[u] + vd, (double)A.y[at], &A.z[at], &A.Dd[at]);
    }
  }
  // part[b][l][j] over the block's rows ascending: column `lane` of the tile, labels lg * kLT .. + kLT
  double* part = A.part + (size_t)b * LD;
  for (int j0 = 0; j0 < d; j0 += kJT) {
    const int jn = d - j0 < kJT ? d - j0 : kJT;
    __syncthreads();
    load_x_tile(A, i0, rn, j0, d, xs, tid);
    __syncthreads();
    if (lane < jn) {
      double acc[kLT];
#pragma unroll
      for (int u = 0; u < kLT; ++u) acc[u] = 0.0;
      for (int rr = 0; rr < rn; ++rr) {
        const double xv = (double)xs[rr * kXsPitch + lane];
#pragma unroll
        for (int u = 0; u < kLT; ++u) acc[u] = GW_OVR_FMA(cs[rr * kCsPitch + lg * kLT + u], xv, acc[u]);
      }
#pragma unroll
      for (int u = 0; u < kLT; ++u) {
        const int ll = lg * kLT + u;
        if (ll < ln && modes[ll]) part[(size_t)(l0 + ll) * D + j0 + lane] = acc[u];
      }
    }
  }
  if (tid < ln && modes[tid]) {
    double acc = 0.0;
    for (int rr = 0; rr < rn; ++rr) acc = acc + cs[rr * kCsPitch + tid];
    part[(size_t)(l0 + tid) * D + d] = acc;
  }
}

__global__ void k_ovr_reduce(const OvrArgs A, int64_t nb) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t LD = (int64_t)A.L * A.D;
  if (o >= LD) return;
  if (A.lab[o / A.D].mode == GW_OVR_MODE_IDLE) return;
  double q = 0.0;
#pragma unroll 8
  for (int64_t b = 0; b < nb; ++b) q = q + A.part[b * LD + o];
  A.vec[o] = q;
}

__global__ __launch_bounds__(kThreads) void k_ovr_step(const OvrArgs A, const gw_ovr_consts K) {
  extern __shared__ double lv[];  // 7 x [D]
  const int l = blockIdx.x, D = A.D;
  if (A.lab[l].mode == GW_OVR_MODE_IDLE) return;  // uniform
  const size_t LD = (size_t)A.L * D;
  for (int idx = threadIdx.x; idx < 7 * D; idx += kThreads) lv[idx] = A.vec[(idx / D) * LD + (size_t)l * D + idx % D];
  __syncthreads();
  if (threadIdx.x == 0) {
    gw_ovr_label s = A.lab[l];
    gw_ovr_label_step(&s, K, D, lv, lv + D, lv + 2 * D, lv + 3 * D, lv + 4 * D, lv + 5 * D, lv + 6 * D);
    A.lab[l] = s;
  }
  __syncthreads();
  for (int idx = D + threadIdx.x; idx < 7 * D; idx += kThreads) A.vec[(idx / D) * LD + (size_t)l * D + idx % D] = lv[idx];
}

// z[i][l] of the rows to score; W [L][D]
__global__ void k_ovr_decision(const OvrArgs A, const int64_t* __restrict__ rows, int64_t count,
                               const double* __restrict__ W, double* __restrict__ z) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= count * A.L) return;
  const int64_t i = idx / A.L;
  const int l = (int)(idx % A.L), d = A.D - 1;
  const int st = A.lab[l].state;
  if (st == GW_OVR_CONST_NEG || st == GW_OVR_CONST_POS) {
    z[idx] = st == GW_OVR_CONST_NEG ? -__builtin_inf() : __builtin_inf();
    return;
  }
  const float* xr = A.x + rows[i] * A.pitch;
  const double* w = W + (size_t)l * A.D;
  double t = 0.0;
  for (int j = 0; j < d; ++j) t = GW_OVR_FMA((double)xr[j], w[j], t);
  z[idx] = t + w[d];
}

__global__ void k_ovr_count(int L, const int64_t* __restrict__ rows, int64_t count, const double* __restrict__ z,
                            const int64_t* __restrict__ row_off, const int32_t* __restrict__ ids,
                            unsigned long long* counts) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= count * L) return;
  const int64_t i = idx / L;
  const int l = (int)(idx % L);
  const int64_t b = row_off[rows[i]], e = row_off[rows[i] + 1];
  if (e == b) return;  // k = 0: nothing true, nothing predicted
  const int pred = gw_ovr_predicted(z + i * L, L, l, (int)(e - b));
  int truth = 0;
  for (int64_t q = b; q < e; ++q) truth |= ids[q] == l;
  if (pred && truth) atomicAdd(&counts[l * 3 + 0], 1ull);
  if (pred && !truth) atomicAdd(&counts[l * 3 + 1], 1ull);
  if (!pred && truth) atomicAdd(&counts[l * 3 + 2], 1ull);
}

size_t step_lds(const gw_ovr* m) { return (size_t)7 * m->D * sizeof(double); }

// the gathered row list and the [rows][L] buffers of a call over `count` rows
int stage_rows(gw_ovr* m, const int64_t* rows, int64_t count, hipStream_t st) {
  gw_ovr_dev& dv = *m->dev;
  const int64_t cells = count * m->L;
  if (dv.rows.grow(count) != hipSuccess || dv.y.grow(cells) != hipSuccess || dv.z.grow(2 * cells) != hipSuccess)
    return gw_ovr_fail(m, GW_ERR_NOMEM, "device allocation failed");
  GW_DEV_TRY(m, hipMemcpyAsync(dv.rows.get(), rows, (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice, st));
  return GW_OK;
}

OvrArgs make_args(const gw_ovr* m, int64_t T) {
  const gw_ovr_dev& dv = *m->dev;
  OvrArgs A = {};
  A.x = m->x;
  A.pitch = m->pitch;
  A.vec16 = ((uintptr_t)m->x % 16 == 0 && m->pitch % 4 == 0) ? 1 : 0;
  A.rows = dv.rows.get();
  A.T = T;
  A.L = m->L;
  A.D = m->D;
  A.y = dv.y.get();
  A.z = dv.z.get();
  A.Dd = dv.z.get() + (size_t)T * m->L;
  A.part = dv.part.get();
  A.vec = dv.vec.get();
  A.lab = dv.lab.get();
  return A;
}

}  // namespace

int gw_ovr_dev_alloc(gw_ovr* m) {
  const int rc = gw_trainer_open_device(m);
  if (rc != GW_OK) return rc;
  GW_DEV_GUARD(m);
  gw_ovr_dev& dv = *m->dev;
  hipError_t e = dv.vec.alloc((int64_t)7 * m->L * m->D);
  if (e == hipSuccess) e = dv.lab.alloc(m->L);
  if (e == hipSuccess) e = dv.counts.alloc((int64_t)m->L * 3);
  if (e == hipSuccess) e = dv.row_off.alloc(m->n + 1);
  if (e != hipSuccess) return gw_ovr_fail(m, GW_ERR_NOMEM, "device allocation failed: %s", hipGetErrorString(e));
  return GW_OK;
}

void gw_ovr_dev_free(gw_ovr* m) {
  gw_device_guard dg(m->device);
  delete m->dev;
  m->dev = nullptr;
}

int gw_ovr_dev_upload_labels(gw_ovr* m) {
  GW_DEV_GUARD(m);
  gw_ovr_dev& dv = *m->dev;
  const size_t nnz = m->ids.size(), off_bytes = m->row_off.size() * sizeof(int64_t);
  if (dv.ids.alloc((int64_t)nnz) != hipSuccess) return gw_ovr_fail(m, GW_ERR_NOMEM, "device allocation failed");
  GW_DEV_TRY(m, hipMemcpy(dv.row_off.get(), m->row_off.data(), off_bytes, hipMemcpyHostToDevice));
  if (nnz) GW_DEV_TRY(m, hipMemcpy(dv.ids.get(), m->ids.data(), nnz * sizeof(int32_t), hipMemcpyHostToDevice));
  return GW_OK;
}

int gw_ovr_dev_fit(gw_ovr* m, const int64_t* rows, int64_t T, const uint8_t* y, int64_t* passes, void* stream) {
  GW_DEV_GUARD(m);
  gw_ovr_dev& dv = *m->dev;
  hipStream_t st = (hipStream_t)stream;
  const int L = m->L, D = m->D;
  const size_t LD = (size_t)L * D, lab_bytes = (size_t)L * sizeof(gw_ovr_label);
  const int64_t nb = (T + kRB - 1) / kRB;
  if (nb > 0x7FFFFFFF) return gw_ovr_fail(m, GW_ERR_UNSUPPORTED, "too many rows for one launch");
  int rc = stage_rows(m, rows, T, st);
  if (rc != GW_OK) return rc;
  if (dv.part.grow(nb * (int64_t)LD) != hipSuccess) return gw_ovr_fail(m, GW_ERR_NOMEM, "device allocation failed");
  GW_DEV_TRY(m, hipMemcpyAsync(dv.y.get(), y, (size_t)T * L, hipMemcpyHostToDevice, st));
  GW_DEV_TRY(m, hipMemcpyAsync(dv.lab.get(), m->lab.data(), lab_bytes, hipMemcpyHostToDevice, st));
  GW_DEV_TRY(m, hipMemsetAsync(dv.vec.get(), 0, 7 * LD * sizeof(double), st));
  // the caller's host arrays are read: no early return leaves a copy in flight
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  const OvrArgs A = make_args(m, T);
  const gw_ovr_consts K = {m->p.C, m->p.gtol, m->p.max_newton, m->p.max_cg};
  const dim3 grid((unsigned)nb, (unsigned)((L + kLC - 1) / kLC));
  for (;;) {
    bool any = false;
    for (int l = 0; l < L; ++l) any = any || m->lab[(size_t)l].mode != GW_OVR_MODE_IDLE;
    if (!any) break;
    k_ovr_pass<<<grid, kThreads, 0, st>>>(A);
    k_ovr_reduce<<<(unsigned)((LD + 255) / 256), 256, 0, st>>>(A, nb);
    k_ovr_step<<<L, kThreads, step_lds(m), st>>>(A, K);
    GW_DEV_TRY(m, hipGetLastError());
    GW_DEV_TRY(m, hipMemcpyAsync(m->lab.data(), dv.lab.get(), lab_bytes, hipMemcpyDeviceToHost, st));
    GW_DEV_TRY(m, hipStreamSynchronize(st));
    *passes += 1;
  }
  m->W.resize(LD);
  GW_DEV_TRY(m, hipMemcpyAsync(m->W.data(), dv.vec.get() + LD, LD * sizeof(double), hipMemcpyDeviceToHost, st));
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  return GW_OK;
}

// decision values of `rows` into z; the weights ride in vec's w slot (they are what the fit left there)
static int launch_decision(gw_ovr* m, const int64_t* rows, int64_t count, hipStream_t st) {
  gw_ovr_dev& dv = *m->dev;
  const int rc = stage_rows(m, rows, count, st);
  if (rc != GW_OK) return rc;
  const int64_t cells = count * m->L;
  if ((cells + 255) / 256 > 0x7FFFFFFF) return gw_ovr_fail(m, GW_ERR_UNSUPPORTED, "too many rows for one launch");
  const OvrArgs A = make_args(m, count);
  const double* w = dv.vec.get() + (size_t)m->L * m->D;
  k_ovr_decision<<<(unsigned)((cells + 255) / 256), 256, 0, st>>>(A, dv.rows.get(), count, w, dv.z.get());
  GW_DEV_TRY(m, hipGetLastError());
  return GW_OK;
}

int gw_ovr_dev_decision(gw_ovr* m, const int64_t* rows, int64_t count, double* z) {
  GW_DEV_GUARD(m);
  gw_ovr_dev& dv = *m->dev;
  const int rc = launch_decision(m, rows, count, nullptr);
  if (rc != GW_OK) return rc;
  GW_DEV_TRY(m, hipMemcpy(z, dv.z.get(), (size_t)count * m->L * sizeof(double), hipMemcpyDeviceToHost));
  return GW_OK;
}

int gw_ovr_dev_score(gw_ovr* m, const int64_t* rows, int64_t count, int64_t* counts, void* stream) {
  GW_DEV_GUARD(m);
  gw_ovr_dev& dv = *m->dev;
  hipStream_t st = (hipStream_t)stream;
  const int rc = launch_decision(m, rows, count, st);
  if (rc != GW_OK) return rc;
  const int64_t cells = count * m->L;
  GW_DEV_TRY(m, hipMemsetAsync(dv.counts.get(), 0, (size_t)m->L * 3 * sizeof(int64_t), st));
  k_ovr_count<<<(unsigned)((cells + 255) / 256), 256, 0, st>>>(m->L, dv.rows.get(), count, dv.z.get(), dv.row_off.get(),
                                                               dv.ids.get(), (unsigned long long*)dv.counts.get());
  GW_DEV_TRY(m, hipGetLastError());
  GW_DEV_TRY(m, hipMemcpyAsync(counts, dv.counts.get(), (size_t)m->L * 3 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  return GW_OK;
}

extern "C" int gw_ovr_kernel_attrs(gw_ovr* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                                   int32_t* lds_bytes, int32_t* count) {
  if (!m) return gw_ovr_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (m->device < 0) return gw_ovr_fail(m, GW_ERR_STATE, "host evaluation launches no kernel");
  GW_DEV_GUARD(m);
  const gw_kernel_entry ks[] = {
      {"k_ovr_pass", (const void*)k_ovr_pass, 0},
      {"k_ovr_reduce", (const void*)k_ovr_reduce, 0},
      {"k_ovr_step", (const void*)k_ovr_step, step_lds(m)},
      {"k_ovr_decision", (const void*)k_ovr_decision, 0},
      {"k_ovr_count", (const void*)k_ovr_count, 0}};
  return gw_trainer_kernel_attrs(m, ks, cap, names, vgprs, scratch_bytes, lds_bytes, count);
}
