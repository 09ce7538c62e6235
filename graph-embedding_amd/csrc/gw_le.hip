// Laplacian-eigenmap kernels (gfx950): the law of gw_le_law.h on [n][m] fp64 row-major blocks.
//
//   k_le_init         the Philox start block, 0 on isolated rows
//   k_le_apply        out = combine(S x): a row of S belongs to one wave from its first entry to its last (the
//                     sum order is the law's, so a hub row is never split), lanes across the columns, up to
//                     kPasses columns per lane; every entry gathers m * 8 contiguous bytes of x[j].  The
//                     Chebyshev combine is the epilogue, so one filter step is one pass.
//   k_le_gram         per chunk of GW_LE_CHUNK rows, the 64 x 64 tiles i <= j of A^T B: rows stream through
//                     LDS 32 at a time, every lane keeps a 4 x 4 tile of fp64 accumulators and walks the rows
//                     ascending.  fp64 fma on the VALU, no MFMA and no atomics: the host restates the order.
//   k_le_gram_reduce  adds the chunk partials in ascending chunk order, one lane per entry, and mirrors
//   k_le_rotate       out = X Q: 64 rows x 64 columns per workgroup, X and Q tiled through LDS 32 k at a time
//                     (Q at m = 160 is 204,800 B and would not fit whole), k ascending
//   k_le_residual     per chunk and column the sum of squares of y - theta x, or of s o x with the entry of
//                     largest magnitude; k_le_col_reduce adds the chunks in order
//   k_le_output       scale, sign, and the fp32 copy
// Loops are bounded and no workgroup waits on another.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gw_le_internal.h"
#include "gw_trainer_device.h"

// Device state of a gw_le handle (device >= 0); the buffers are freed with it.
struct gw_le_dev {
  gw_dev_buf<int64_t> off;
  gw_dev_buf<int32_t> col;
  gw_dev_buf<double> val, s;
  gw_dev_buf<double> blk[GW_LE_BLOCKS];  // [n][m]
  gw_dev_buf<double> part;               // [chunks][m][m]
  gw_dev_buf<double> small;              // [m][m]: a product on its way down, Q on its way up
  gw_dev_buf<double> cpart, camax;       // [chunks][m]
  gw_dev_buf<int64_t> carow;             // [chunks][m]
  gw_dev_buf<double> vec;                // [2 m]: theta or norms up, sums down
  gw_dev_buf<int32_t> neg;               // [m]
  gw_dev_buf<double> out64;              // [n][dim]
  gw_dev_buf<float> out32;               // [n][dim]
};

namespace {

constexpr int kThreads = 256;
constexpr int kRowsPerWg = kThreads / 64;  // k_le_apply: one row per wave
constexpr int kPasses = GW_LE_MAX_BLOCK / 64;
constexpr int kGather = 8;  // k_le_apply: entries of a row whose gathers are issued together
constexpr int kTile = 64;   // k_le_gram, k_le_rotate: output tile edge
constexpr int kStage = 32;  // rows (gram) or k (rotate) per LDS stage
static_assert(kRowsPerWg == 4, "gw_le_tiles reports 4 rows per workgroup");
static_assert(kThreads == (kTile / 4) * (kTile / 4), "one 4 x 4 register tile per lane");
static_assert(GW_LE_CHUNK % kStage == 0, "a chunk is whole stages");

__global__ void k_le_init(double* __restrict__ X, const double* __restrict__ s, int64_t n, int m, uint64_t seed) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * m) return;
  const int64_t i = idx / m;
  const int c = (int)(idx - i * m);
  X[idx] = s[i] == 0.0 ? 0.0 : gw_le_start(seed, i, c);
}

__global__ __launch_bounds__(kThreads) void k_le_apply(const int64_t* __restrict__ off, const int32_t* __restrict__ col,
                                                       const double* __restrict__ val, int64_t n,
                                                       const double* __restrict__ x, double* __restrict__ y,
                                                       const double* __restrict__ z, int64_t cols, int mode,
                                                       double alpha, double beta, double gamma) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t i = (int64_t)blockIdx.x * kRowsPerWg + wave;
  if (i >= n) return;  // wave-uniform
  const int64_t c0 = (int64_t)blockIdx.y * GW_LE_MAX_BLOCK;
  double acc[kPasses];
#pragma unroll
  for (int q = 0; q < kPasses; ++q) acc[q] = 0.0;
  bool live[kPasses];  // this lane's column of pass q exists; a dead one computes on zeros and is never written
#pragma unroll
  for (int q = 0; q < kPasses; ++q) live[q] = c0 + lane + 64 * q < cols;
  const int64_t b = off[i], e = off[i + 1];
  int64_t p = b;
  // kGather entries' gathers are in flight together (a hub row is one wave's serial work, so its latency is the
  // kernel's tail); the fma chain still takes the entries in ascending order
  for (; p + kGather <= e; p += kGather) {
    double w[kGather], xv[kGather][kPasses];
#pragma unroll
    for (int u = 0; u < kGather; ++u) {
      w[u] = val[p + u];
      const double* xr = x + (int64_t)col[p + u] * cols + c0;
#pragma unroll
      for (int q = 0; q < kPasses; ++q) xv[u][q] = live[q] ? xr[lane + 64 * q] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kGather; ++u)
#pragma unroll
      for (int q = 0; q < kPasses; ++q) acc[q] = GW_LE_FMA(w[u], xv[u][q], acc[q]);
  }
  for (; p < e; ++p) {  // the row's last entries
    const double w = val[p];
    const double* xr = x + (int64_t)col[p] * cols + c0;
#pragma unroll
    for (int q = 0; q < kPasses; ++q) {
      const int c = lane + 64 * q;
      if (c0 + c < cols) acc[q] = GW_LE_FMA(w, xr[c], acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < kPasses; ++q) {
    const int64_t c = c0 + lane + 64 * q;
    if (c >= cols) continue;
    const int64_t o = i * cols + c;
    y[o] = gw_le_combine(mode, alpha, acc[q], beta, mode == GW_LE_PLAIN ? 0.0 : x[o], gamma,
                         mode == GW_LE_CHEB ? z[o] : 0.0);
  }
}

__global__ __launch_bounds__(kThreads) void k_le_gram(const double* __restrict__ A, const double* __restrict__ B, int64_t n,
                                                      int m, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double As[kStage][kTile];
  __shared__ __attribute__((aligned(16))) double Bs[kStage][kTile];
  const int tid = threadIdx.x, tq = tid >> 4, tc = tid & 15;
  const int tiles = (m + kTile - 1) / kTile;
  int t = blockIdx.x, ti = 0;
  while (t >= tiles - ti) {  // blockIdx.x counts the tiles ti <= tj row by row
    t -= tiles - ti;
    ++ti;
  }
  const int tj = ti + t;
  const int64_t ch = blockIdx.y;
  const int64_t r_begin = ch * GW_LE_CHUNK, r_end = r_begin + GW_LE_CHUNK < n ? r_begin + GW_LE_CHUNK : n;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[a][u] = 0.0;
  for (int64_t r0 = r_begin; r0 < r_end; r0 += kStage) {
    __syncthreads();  // the last stage's reads are done
#pragma unroll
    for (int p = 0; p < kStage * kTile / kThreads; ++p) {
      const int rr = (tid >> 6) + (kThreads / 64) * p, cc = tid & 63;
      const int64_t r = r0 + rr;
      const int ca = ti * kTile + cc, cb = tj * kTile + cc;
      As[rr][cc] = (r < r_end && ca < m) ? A[r * m + ca] : 0.0;
      Bs[rr][cc] = (r < r_end && cb < m) ? B[r * m + cb] : 0.0;
    }
    __syncthreads();
    const int rn = r_end - r0 < kStage ? (int)(r_end - r0) : kStage;
    for (int rr = 0; rr < rn; ++rr) {  // rows ascending; rows past the chunk's end are never added
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = As[rr][tq * 4 + u];
        b[u] = Bs[rr][tc * 4 + u];
      }
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[v][u] = GW_LE_FMA(a[v], b[u], acc[v][u]);
    }
  }
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = ti * kTile + tq * 4 + v, j = tj * kTile + tc * 4 + u;
      if (i < m && j < m) part[((size_t)ch * m + i) * m + j] = acc[v][u];
    }
}

__global__ void k_le_gram_reduce(const double* __restrict__ part, int64_t chunks, int m, double* __restrict__ C) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m * m) return;
  const int i = idx / m, j = idx - i * m;
  if (i > j) return;  // the lane of [j][i] writes both
  double acc = 0.0;
  for (int64_t ch = 0; ch < chunks; ++ch) acc = acc + part[((size_t)ch * m + i) * m + j];
  C[(size_t)i * m + j] = acc;
  C[(size_t)j * m + i] = acc;
}

__global__ __launch_bounds__(kThreads) void k_le_rotate(const double* __restrict__ X, const double* __restrict__ Q,
                                                        double* __restrict__ out, int64_t n, int m) {
  __shared__ double Xs[kTile][kStage + 1];  // one column of padding: the four rows of a lane fall into four banks
  __shared__ __attribute__((aligned(16))) double Qs[kStage][kTile];
  const int tid = threadIdx.x, tq = tid >> 4, tc = tid & 15;
  const int64_t row0 = (int64_t)blockIdx.x * kTile;
  const int col0 = blockIdx.y * kTile;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[a][u] = 0.0;
  for (int k0 = 0; k0 < m; k0 += kStage) {
    __syncthreads();
#pragma unroll
    for (int p = 0; p < kTile * kStage / kThreads; ++p) {
      const int idx = p * kThreads + tid;
      const int rr = idx >> 5, kk = idx & 31;
      Xs[rr][kk] = (row0 + rr < n && k0 + kk < m) ? X[(row0 + rr) * m + k0 + kk] : 0.0;
      const int qk = idx >> 6, qc = idx & 63;
      Qs[qk][qc] = (k0 + qk < m && col0 + qc < m) ? Q[(size_t)(k0 + qk) * m + col0 + qc] : 0.0;
    }
    __syncthreads();
    const int kn = m - k0 < kStage ? m - k0 : kStage;
    for (int kk = 0; kk < kn; ++kk) {  // k ascending; k past m is never added
      double x[4], q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        x[u] = Xs[tq * 4 + u][kk];
        q[u] = Qs[kk][tc * 4 + u];
      }
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[v][u] = GW_LE_FMA(x[v], q[u], acc[v][u]);
    }
  }
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = row0 + tq * 4 + v;
      const int j = col0 + tc * 4 + u;
      if (i < n && j < m) out[i * m + j] = acc[v][u];
    }
}

// theta != NULL: the residual's terms; else s o x with the entry of largest magnitude (lowest row among equals)
__global__ __launch_bounds__(kThreads) void k_le_residual(const double* __restrict__ X, const double* __restrict__ Y,
                                                          const double* __restrict__ theta, const double* __restrict__ s,
                                                          int64_t n, int m, int col0, int dim, double* __restrict__ part,
                                                          double* __restrict__ amax, int64_t* __restrict__ arow) {
  const int c = threadIdx.x;
  if (c >= dim) return;
  const int64_t ch = blockIdx.x;
  const int64_t r_begin = ch * GW_LE_CHUNK, r_end = r_begin + GW_LE_CHUNK < n ? r_begin + GW_LE_CHUNK : n;
  const double th = theta ? theta[c] : 0.0;
  double acc = 0.0, best = 0.0;
  int64_t brow = -1;
  for (int64_t r = r_begin; r < r_end; ++r) {
    const double x = X[r * m + col0 + c];
    const double v = theta ? gw_le_res_term(th, x, Y[r * m + col0 + c]) : s[r] * x;
    acc = GW_LE_FMA(v, v, acc);
    const double av = v < 0.0 ? -v : v;
    if (av > best) {
      best = av;
      brow = r;
    }
  }
  part[ch * dim + c] = acc;
  amax[ch * dim + c] = best;
  arow[ch * dim + c] = brow;
}

__global__ void k_le_col_reduce(const double* __restrict__ part, const double* __restrict__ amax,
                                const int64_t* __restrict__ arow, int64_t chunks, int dim, const double* __restrict__ X,
                                const double* __restrict__ s, int m, int col0, double* __restrict__ sums,
                                int32_t* __restrict__ neg) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= dim) return;
  double acc = 0.0, best = 0.0;
  int64_t brow = -1;
  for (int64_t ch = 0; ch < chunks; ++ch) {
    acc = acc + part[ch * dim + c];
    if (amax[ch * dim + c] > best) {
      best = amax[ch * dim + c];
      brow = arow[ch * dim + c];
    }
  }
  sums[c] = acc;
  neg[c] = brow >= 0 && s[brow] * X[brow * m + col0 + c] < 0.0;
}

__global__ void k_le_output(const double* __restrict__ X, const double* __restrict__ s, int64_t n, int m, int col0, int dim,
                            const double* __restrict__ nrm, const int32_t* __restrict__ neg, double* __restrict__ out64,
                            float* __restrict__ out32) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * dim) return;
  const int64_t i = idx / dim;
  const int c = (int)(idx - i * dim);
  const double f = gw_le_out(s[i], X[i * m + col0 + c], nrm[c], neg[c]);
  out64[idx] = f;
  out32[idx] = (float)f;
}

int64_t chunks_of(const gw_le* m) { return (m->n + GW_LE_CHUNK - 1) / GW_LE_CHUNK; }
unsigned blocks_for(int64_t items) { return (unsigned)((items + kThreads - 1) / kThreads); }

template <typename T>
int upload(gw_le* m, gw_dev_buf<T>& dst, const T* src, size_t count) {
  if (dst.alloc((int64_t)count) != hipSuccess) return gw_le_fail(m, GW_ERR_NOMEM, "device allocation failed");
  if (count) GW_DEV_TRY(m, hipMemcpy(dst.get(), src, sizeof(T) * count, hipMemcpyHostToDevice));
  return GW_OK;
}

int launch_apply(gw_le* m, const double* x, double* y, const double* z, int64_t cols, int mode, double alpha, double beta,
                 double gamma, hipStream_t st) {
  gw_le_dev& dv = *m->dev;
  const dim3 grid((unsigned)((m->n + kRowsPerWg - 1) / kRowsPerWg), (unsigned)((cols + GW_LE_MAX_BLOCK - 1) / GW_LE_MAX_BLOCK));
  k_le_apply<<<grid, kThreads, 0, st>>>(dv.off.get(), dv.col.get(), dv.val.get(), m->n, x, y, z, cols, mode, alpha, beta,
                                        gamma);
  GW_DEV_TRY(m, hipGetLastError());
  return GW_OK;
}

int launch_gram(gw_le* m, const double* A, const double* B, hipStream_t st) {
  gw_le_dev& dv = *m->dev;
  const int mb = m->m, tiles = (mb + kTile - 1) / kTile;
  const dim3 grid((unsigned)(tiles * (tiles + 1) / 2), (unsigned)chunks_of(m));
  k_le_gram<<<grid, kThreads, 0, st>>>(A, B, m->n, mb, dv.part.get());
  GW_DEV_TRY(m, hipGetLastError());
  k_le_gram_reduce<<<blocks_for((int64_t)mb * mb), kThreads, 0, st>>>(dv.part.get(), chunks_of(m), mb, dv.small.get());
  GW_DEV_TRY(m, hipGetLastError());
  return GW_OK;
}

int launch_rotate(gw_le* m, const double* X, double* out, hipStream_t st) {
  const int mb = m->m;
  const dim3 grid((unsigned)((m->n + kTile - 1) / kTile), (unsigned)((mb + kTile - 1) / kTile));
  k_le_rotate<<<grid, kThreads, 0, st>>>(X, m->dev->small.get(), out, m->n, mb);
  GW_DEV_TRY(m, hipGetLastError());
  return GW_OK;
}

}  // namespace

int gw_le_dev_alloc(gw_le* m) { return gw_trainer_open_device(m); }

void gw_le_dev_free(gw_le* m) {
  gw_device_guard dg(m->device);
  delete m->dev;
  m->dev = nullptr;
}

int gw_le_dev_upload(gw_le* m) {
  GW_DEV_GUARD(m);
  gw_le_dev& dv = *m->dev;
  int rc = upload(m, dv.off, m->off.data(), m->off.size());
  if (rc == GW_OK) rc = upload(m, dv.col, m->col.data(), m->col.size());
  if (rc == GW_OK) rc = upload(m, dv.val, m->val.data(), m->val.size());
  if (rc == GW_OK) rc = upload(m, dv.s, m->s.data(), m->s.size());
  return rc;
}

int gw_le_dev_prepare(gw_le* m) {
  GW_DEV_GUARD(m);
  gw_le_dev& dv = *m->dev;
  const int64_t mb = m->m, ch = chunks_of(m);
  hipError_t e = hipSuccess;
  for (auto& b : dv.blk)
    if (e == hipSuccess) e = b.grow(m->n * mb);
  if (e == hipSuccess) e = dv.part.grow(ch * mb * mb);
  if (e == hipSuccess) e = dv.small.grow(mb * mb);
  if (e == hipSuccess) e = dv.cpart.grow(ch * mb);
  if (e == hipSuccess) e = dv.camax.grow(ch * mb);
  if (e == hipSuccess) e = dv.carow.grow(ch * mb);
  if (e == hipSuccess) e = dv.vec.grow(2 * mb);
  if (e == hipSuccess) e = dv.neg.grow(mb);
  if (e == hipSuccess) e = dv.out64.grow(m->n * m->p.dim);
  if (e == hipSuccess) e = dv.out32.grow(m->n * m->p.dim);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return gw_le_fail(m, GW_ERR_NOMEM, "device allocation failed: %s", hipGetErrorString(e));
  }
  return GW_OK;
}

int gw_le_dev_init(gw_le* m, int dst) {
  GW_DEV_GUARD(m);
  gw_le_dev& dv = *m->dev;
  k_le_init<<<blocks_for(m->n * m->m), kThreads, 0, (hipStream_t)m->stream>>>(dv.blk[dst].get(), dv.s.get(), m->n, m->m,
                                                                              m->p.seed);
  GW_DEV_TRY(m, hipGetLastError());
  return GW_OK;
}

int gw_le_dev_apply(gw_le* m, int mode, double alpha, double beta, double gamma, int src, int dst, int z) {
  GW_DEV_GUARD(m);
  gw_le_dev& dv = *m->dev;
  return launch_apply(m, dv.blk[src].get(), dv.blk[dst].get(), z >= 0 ? dv.blk[z].get() : nullptr, m->m, mode, alpha, beta,
                      gamma, (hipStream_t)m->stream);
}

int gw_le_dev_gram(gw_le* m, int a, int b, double* C) {
  GW_DEV_GUARD(m);
  gw_le_dev& dv = *m->dev;
  hipStream_t st = (hipStream_t)m->stream;
  const int rc = launch_gram(m, dv.blk[a].get(), dv.blk[b].get(), st);
  if (rc != GW_OK) return rc;
  GW_DEV_TRY(m, hipMemcpyAsync(C, dv.small.get(), sizeof(double) * m->m * m->m, hipMemcpyDeviceToHost, st));
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  return GW_OK;
}

int gw_le_dev_rotate(gw_le* m, int src, int dst, const double* Q) {
  GW_DEV_GUARD(m);
  gw_le_dev& dv = *m->dev;
  hipStream_t st = (hipStream_t)m->stream;
  GW_DEV_TRY(m, hipMemcpyAsync(dv.small.get(), Q, sizeof(double) * m->m * m->m, hipMemcpyHostToDevice, st));
  GW_DEV_TRY(m, hipStreamSynchronize(st));  // Q is the caller's again
  return launch_rotate(m, dv.blk[src].get(), dv.blk[dst].get(), st);
}

static int col_sums(gw_le* m, int x, int y, const double* theta, int col0, int dim, double* sumsq, int32_t* negate) {
  gw_le_dev& dv = *m->dev;
  hipStream_t st = (hipStream_t)m->stream;
  const int mb = m->m;
  double* d_theta = nullptr;
  if (theta) {
    d_theta = dv.vec.get();
    GW_DEV_TRY(m, hipMemcpyAsync(d_theta, theta, sizeof(double) * dim, hipMemcpyHostToDevice, st));
    GW_DEV_TRY(m, hipStreamSynchronize(st));
  }
  double* d_sums = dv.vec.get() + mb;
  k_le_residual<<<(unsigned)chunks_of(m), kThreads, 0, st>>>(dv.blk[x].get(), y >= 0 ? dv.blk[y].get() : nullptr, d_theta,
                                                            dv.s.get(), m->n, mb, col0, dim, dv.cpart.get(), dv.camax.get(),
                                                            dv.carow.get());
  GW_DEV_TRY(m, hipGetLastError());
  k_le_col_reduce<<<blocks_for(dim), kThreads, 0, st>>>(dv.cpart.get(), dv.camax.get(), dv.carow.get(), chunks_of(m), dim,
                                                       dv.blk[x].get(), dv.s.get(), mb, col0, d_sums, dv.neg.get());
  GW_DEV_TRY(m, hipGetLastError());
  GW_DEV_TRY(m, hipMemcpyAsync(sumsq, d_sums, sizeof(double) * dim, hipMemcpyDeviceToHost, st));
  if (negate) GW_DEV_TRY(m, hipMemcpyAsync(negate, dv.neg.get(), sizeof(int32_t) * dim, hipMemcpyDeviceToHost, st));
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  return GW_OK;
}

int gw_le_dev_resid(gw_le* m, int x, int y, const double* theta, double* sumsq) {
  GW_DEV_GUARD(m);
  return col_sums(m, x, y, theta, 0, m->m, sumsq, nullptr);
}

int gw_le_dev_colstat(gw_le* m, int x, int col0, int dim, double* sumsq, int32_t* negate) {
  GW_DEV_GUARD(m);
  return col_sums(m, x, -1, nullptr, col0, dim, sumsq, negate);
}

int gw_le_dev_output(gw_le* m, int x, int col0, int dim, const double* nrm, const int32_t* negate) {
  GW_DEV_GUARD(m);
  gw_le_dev& dv = *m->dev;
  hipStream_t st = (hipStream_t)m->stream;
  GW_DEV_TRY(m, hipMemcpyAsync(dv.vec.get(), nrm, sizeof(double) * dim, hipMemcpyHostToDevice, st));
  GW_DEV_TRY(m, hipMemcpyAsync(dv.neg.get(), negate, sizeof(int32_t) * dim, hipMemcpyHostToDevice, st));
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  k_le_output<<<blocks_for(m->n * dim), kThreads, 0, st>>>(dv.blk[x].get(), dv.s.get(), m->n, m->m, col0, dim, dv.vec.get(),
                                                          dv.neg.get(), dv.out64.get(), dv.out32.get());
  GW_DEV_TRY(m, hipGetLastError());
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  return GW_OK;
}

int gw_le_dev_export(gw_le* m, double* vectors) {
  GW_DEV_GUARD(m);
  GW_DEV_TRY(m, hipMemcpy(vectors, m->dev->out64.get(), sizeof(double) * m->n * m->p.dim, hipMemcpyDeviceToHost));
  return GW_OK;
}

int gw_le_dev_vectors(gw_le* m, float** ptr) {
  *ptr = m->dev->out32.get();
  return GW_OK;
}

int gw_le_dev_apply_user(gw_le* m, const double* x, double* y, int cols) {
  GW_DEV_GUARD(m);
  const int rc = launch_apply(m, x, y, nullptr, cols, GW_LE_PLAIN, 1.0, 0.0, 0.0, nullptr);
  if (rc != GW_OK) return rc;
  GW_DEV_TRY(m, hipStreamSynchronize(nullptr));
  return GW_OK;
}

extern "C" int gw_le_kernel_attrs(gw_le* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                                  int32_t* lds_bytes, int32_t* count) {
  if (!m) return gw_le_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (m->device < 0) return gw_le_fail(m, GW_ERR_STATE, "host evaluation launches no kernel");
  GW_DEV_GUARD(m);
  const gw_kernel_entry ks[] = {{"k_le_init", (const void*)k_le_init, 0},
                                {"k_le_apply", (const void*)k_le_apply, 0},
                                {"k_le_gram", (const void*)k_le_gram, 0},
                                {"k_le_gram_reduce", (const void*)k_le_gram_reduce, 0},
                                {"k_le_rotate", (const void*)k_le_rotate, 0},
                                {"k_le_residual", (const void*)k_le_residual, 0},
                                {"k_le_col_reduce", (const void*)k_le_col_reduce, 0},
                                {"k_le_output", (const void*)k_le_output, 0}};
  return gw_trainer_kernel_attrs(m, ks, cap, names, vgprs, scratch_bytes, lds_bytes, count);
}

extern "C" int gw_le_time_kernel(gw_le* m, int which, int reps, double* ms) {
  if (!m || !ms || reps < 1 || which < 0 || which > 2) return gw_le_fail(m, GW_ERR_INVALID, "bad arguments");
  if (m->device < 0) return gw_le_fail(m, GW_ERR_STATE, "host evaluation launches no kernel");
  if (!m->solved) return gw_le_fail(m, GW_ERR_STATE, "call gw_le_solve first");
  GW_DEV_GUARD(m);
  gw_le_dev& dv = *m->dev;
  hipEvent_t e0, e1;
  GW_DEV_TRY(m, hipEventCreate(&e0));
  GW_DEV_TRY(m, hipEventCreate(&e1));
  int rc = GW_OK;
  hipError_t e = hipSuccess;
  for (int r = -1; r < reps && rc == GW_OK; ++r) {  // r = -1: the warm-up
    if (r == 0) e = hipEventRecord(e0, nullptr);
    if (which == 0)
      rc = launch_apply(m, dv.blk[0].get(), dv.blk[1].get(), dv.blk[2].get(), m->m, GW_LE_CHEB, 1.0, -0.5, -1.0, nullptr);
    else if (which == 1)
      rc = launch_gram(m, dv.blk[0].get(), dv.blk[1].get(), nullptr);
    else
      rc = launch_rotate(m, dv.blk[0].get(), dv.blk[3].get(), nullptr);
  }
  if (rc == GW_OK && e == hipSuccess) e = hipEventRecord(e1, nullptr);
  if (rc == GW_OK && e == hipSuccess) e = hipEventSynchronize(e1);
  float t = 0.f;
  if (rc == GW_OK && e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc != GW_OK) return rc;
  GW_DEV_TRY(m, e);
  *ms = (double)t / reps;
  return GW_OK;
}
