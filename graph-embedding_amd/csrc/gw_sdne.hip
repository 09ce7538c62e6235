// SDNE trainer kernels (gfx950): the training law of gw_sdne_law.h.
//
// One step is a fixed chain on the caller's stream, no host round trip:
//   k_sdne_batch      the step's B rows (gw_sdne_row: ordered or the epoch's permutation) as a dense x[B][u0]
//                     (dense input: copied; CSR: zeroed and scattered) and their ids
//   k_sdne_gemm       every product of the law on the fp32 MFMA (32x32x2, a k-ordered fmaf chain), operands
//                     staged in LDS, 64x64 output tile per workgroup, general operand strides:
//                       forward        z = in . W + b        (4 times; bias preload, relu, the pre-activation kept)
//                       backward data  dz = (dz' . W^T [+ klg]) masked by the pre-activation   (3 times)
//                       backward wgt   dW = in^T . dz', g = fmaf(wd, W, dW), Adam from the accumulators (4 times)
//                     A product of at most kInKernelChunks chunks walks its chunks inside the kernel; a longer one
//                     (the two that reduce over u0) runs one chunk per workgroup into `part` and
//   k_sdne_reduce     adds the chunk partials in ascending order and applies the same epilogue
//   k_sdne_first      with first_order > 0, after forward layer 2: g1[B][u2], the first-order term's gradient; one
//                     workgroup per batch row, the nonzero S_ij compacted in j order into LDS, threads over c
//   k_sdne_q          q = mean(h2) in the law's order and the KL gradient scalar
//   k_sdne_loss_*     the reported loss in fp64 (only when it is asked for)
//   k_sdne_bias       the four bias gradients and their Adam
// All backward-data products run before the first weight update, so they read the old weights.  No float
// atomics: every sum has the law's order, so two runs give the same bits and the host evaluation gives them too.
// Past a tile's or the reduction's end the staged operands are 0 and fma(0, 0, acc) leaves acc as it is (acc
// starts at +0 or the bias), so a padded MFMA chain equals the law's shorter one.
#include <hip/hip_runtime.h>

#include "gw_sdne_internal.h"
#include "gw_sdne_law.h"
#include "gw_trainer_device.h"

// Device state of a gw_sdne handle (device >= 0); the buffers are freed with it.
struct gw_sdne_dev {
  gw_dev_buf<float> par[8], am[8], av[8];  // {w1, b1, .., w4, b4} and their Adam moments
  gw_dev_buf<float> grad[8];               // diagnostic, allocated by gw_sdne_gradients
  gw_dev_buf<float> x;                     // [B][u0]
  gw_dev_buf<int64_t> rowid;               // [B]: the input row of each staged row
  gw_dev_buf<float> g1;                    // [B][u2]: the first-order term's gradient (first_order > 0)
  gw_dev_buf<float> z[4], h[3];            // pre-activations z1, z2, z3, y; h1, h2, h3
  gw_dev_buf<float> dz[4];                 // dz1 .. dz4
  gw_dev_buf<float> part;                  // [chunks][M][N] of the longest split product
  gw_dev_buf<float> q;                     // q, klg
  gw_dev_buf<double> lpart, loss;          // loss partials; per-step losses of one train call
  gw_dev_buf<int64_t> offs;                // CSR rows
  gw_dev_buf<int32_t> cols;
  gw_dev_buf<float> vals;
  gw_dev_buf<float> enc;  // [N][u2]
};

namespace {

constexpr int kT = 64;             // output tile edge
constexpr int kTK = 64;            // reduction indices per LDS stage; divides GW_SDNE_KC
constexpr int kPitch = kT + 1;
constexpr int kThreads = 256;
constexpr int kStage = kT * kTK / kThreads;  // elements of each operand a thread stages
constexpr int kInKernelChunks = 4; // a launch constant: the bits do not depend on it
constexpr int kLossBlocks = 128;

static_assert(GW_SDNE_KC % kTK == 0, "a stage never straddles a chunk");

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum { EPI_FWD = 0, EPI_BWD = 1, EPI_WGT = 2 };

struct Gemm {
  const float* a;  // A(row, k) = a[row * a_rs + k * a_ks]
  int64_t a_rs, a_ks;
  const float* b;  // B(k, col) = b[k * b_ks + col * b_cs]
  int64_t b_ks, b_cs;
  int M, N, K;
  int tiles_n;
  float* part;  // split launch: [chunk][M][N]
};

struct Epi {
  int kind;
  // EPI_FWD
  const float* bias;  // the chain's start
  float* pre;         // [M][N]
  float* act;         // relu(z), or gw_sdne_dz4(z, xin, bw, Bf) when xin is set; may be NULL
  const float* xin;
  float Bf, bw;
  // EPI_BWD
  const float* mask;  // pre-activation [M][N]
  const float* klg;   // NULL or the scalar added before the mask
  const float* add;   // NULL or [M][N] added after the mask
  float* out;         // dz [M][N]; EPI_WGT with adam off: g [M][N]
  // EPI_WGT
  float *W, *am, *av;
  float wd;
  int adam;
  gw_sdne_adam_c C;
};

__device__ __forceinline__ void apply_epi(const Epi& E, int row, int col, int N, float v) {
  const int64_t at = (int64_t)row * N + col;
  if (E.kind == EPI_FWD) {
    E.pre[at] = v;
    if (E.act) {
      if (E.xin) {
        E.act[at] = gw_sdne_dz4(v, E.xin[at], E.bw, E.Bf);
      } else {
        E.act[at] = v > 0.0f ? v : 0.0f;
      }
    }
  } else if (E.kind == EPI_BWD) {
    if (E.klg) v = v + *E.klg;
    v = E.mask[at] > 0.0f ? v : 0.0f;
    if (E.add) v = v + E.add[at];
    E.out[at] = v;
  } else {
    const float g = fmaf(E.wd, E.W[at], v);
    if (E.adam)
      gw_sdne_adam(&E.W[at], &E.am[at], &E.av[at], g, E.C);
    else
      E.out[at] = g;
  }
}

// which input rows a launch of k_sdne_batch stages: a step's (step = 1: gw_sdne_row of slot blockIdx.x) or
// row0 + blockIdx.x (the encoder)
struct RowSel {
  int step, shuffle;
  uint64_t seed, t;
  int64_t N, B, row0;
};

__global__ __launch_bounds__(kThreads) void k_sdne_batch(float* __restrict__ x, int u0, const float* __restrict__ rows,
                                                         int64_t pitch, const int64_t* __restrict__ offs,
                                                         const int32_t* __restrict__ cols,
                                                         const float* __restrict__ vals, const RowSel R,
                                                         int64_t* __restrict__ rowid) {
  const int64_t r = R.step ? gw_sdne_row(R.seed, R.shuffle, R.N, R.B, R.t, blockIdx.x) : R.row0 + blockIdx.x;
  if (r < 0 || r >= R.N) return;  // cannot happen: the permutation maps [0, N) onto itself
  if (threadIdx.x == 0) rowid[blockIdx.x] = r;
  float* xr = x + (int64_t)blockIdx.x * u0;
  if (rows) {
    for (int i = threadIdx.x; i < u0; i += kThreads) xr[i] = rows[r * pitch + i];
    return;
  }
  for (int i = threadIdx.x; i < u0; i += kThreads) xr[i] = 0.0f;
  __syncthreads();
  // the columns were range-checked and found distinct by gw_sdne_set_rows_csr
  for (int64_t e = offs[r] + threadIdx.x; e < offs[r + 1]; e += kThreads) {
    const int32_t c = cols[e];
    if ((uint32_t)c < (uint32_t)u0) xr[c] = vals[e];
  }
}

// Workgroup (tile, z): the 64x64 output tile `tile` over the chunks [0, nch) (gridDim.y == 1) or over chunk z alone
// (gridDim.y == nch: the partial goes to G.part).  Wave w owns the 32x32 block (w >> 1, w & 1) of the tile.
__global__ __launch_bounds__(kThreads) void k_sdne_gemm(const Gemm G, const Epi E) {
  __shared__ float As[kTK * kPitch];  // [k][row]
  __shared__ float Bs[kTK * kPitch];  // [k][col]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lhi = lane >> 5;
  const int wr = wv >> 1, wc = wv & 1;
  const int r0 = (int)(blockIdx.x / G.tiles_n) * kT, c0 = (int)(blockIdx.x % G.tiles_n) * kT;
  const int M = G.M, N = G.N, K = G.K;
  const int nch = (K + GW_SDNE_KC - 1) / GW_SDNE_KC;
  const bool split = gridDim.y > 1;
  const int ch_begin = split ? (int)blockIdx.y : 0, ch_end = split ? (int)blockIdx.y + 1 : nch;
  const int col = c0 + wc * 32 + l31;
  const float start = (E.kind == EPI_FWD && col < N) ? E.bias[col] : 0.0f;
  const bool a_kfast = G.a_ks == 1, b_cfast = G.b_cs == 1;
  f32x16 tot, acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) tot[r] = 0.0f;
  for (int ch = ch_begin; ch < ch_end; ++ch) {
    const float s0 = ch == 0 ? start : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = s0;
    const int kend = min(K, (ch + 1) * GW_SDNE_KC);
    for (int k0 = ch * GW_SDNE_KC; k0 < kend; k0 += kTK) {
      // every load of the stage is issued before the first LDS store waits for one
      float ra[kStage], rb[kStage];
#pragma unroll
      for (int i = 0; i < kStage; ++i) {
        const int idx = tid + i * kThreads;
        const int kk = a_kfast ? idx % kTK : idx / kT, rr = a_kfast ? idx / kTK : idx % kT;
        const int row = r0 + rr, k = k0 + kk;
        ra[i] = (row < M && k < kend) ? G.a[(int64_t)row * G.a_rs + (int64_t)k * G.a_ks] : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < kStage; ++i) {
        const int idx = tid + i * kThreads;
        const int kk = b_cfast ? idx / kT : idx % kTK, cc = b_cfast ? idx % kT : idx / kTK;
        const int c = c0 + cc, k = k0 + kk;
        rb[i] = (c < N && k < kend) ? G.b[(int64_t)k * G.b_ks + (int64_t)c * G.b_cs] : 0.0f;
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < kStage; ++i) {
        const int idx = tid + i * kThreads;
        As[(a_kfast ? idx % kTK : idx / kT) * kPitch + (a_kfast ? idx / kTK : idx % kT)] = ra[i];
        Bs[(b_cfast ? idx / kT : idx % kTK) * kPitch + (b_cfast ? idx % kT : idx / kTK)] = rb[i];
      }
      __syncthreads();
#pragma unroll 4
      for (int kk = 0; kk < kTK; kk += 2) {
        const float a = As[(kk + lhi) * kPitch + wr * 32 + l31];
        const float b = Bs[(kk + lhi) * kPitch + wc * 32 + l31];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
      }
    }
    if (ch == ch_begin) {
      tot = acc;
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) tot[r] = tot[r] + acc[r];
    }
  }
  if (col >= N) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = r0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
    if (row < M) {
      if (split)
        G.part[((int64_t)blockIdx.y * M + row) * N + col] = tot[r];
      else
        apply_epi(E, row, col, N, tot[r]);
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_sdne_reduce(const float* __restrict__ part, int M, int N, int nch,
                                                          const Epi E) {
  const int64_t n = (int64_t)M * N;
  const int64_t o = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (o >= n) return;
  float acc = part[o];
#pragma unroll 8
  for (int ch = 1; ch < nch; ++ch) acc = acc + part[(int64_t)ch * n + o];
  apply_epi(E, (int)(o / N), (int)(o % N), N, acc);
}

// g1[i][c] = coef * (the chain over j ascending from +0 of fmaf(S_ij, z2[i][c] - z2[j][c], acc)), S_ij = a_ij + a_ji,
// a_ij = x[i][rowid[j]].  Workgroup i: threads [0, B) form S_i., the nonzero ones are compacted in j order into LDS
// (skipping S_ij = 0 keeps the bits, gw_sdne_law.h), then the threads run over c and read z2[j][.] coalesced.
__global__ __launch_bounds__(kThreads) void k_sdne_first(const float* __restrict__ x, int u0,
                                                         const int64_t* __restrict__ rowid,
                                                         const float* __restrict__ z2, int B, int u2, float coef,
                                                         float* __restrict__ g1) {
  static_assert(GW_SDNE_MAX_BATCH <= kThreads && GW_SDNE_MAX_BATCH % 64 == 0, "one thread per batch row, whole waves");
  constexpr int kW = GW_SDNE_MAX_BATCH / 64;
  __shared__ float Sv[GW_SDNE_MAX_BATCH];
  __shared__ int Sj[GW_SDNE_MAX_BATCH];
  __shared__ int cnt[kW];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float s = 0.0f;
  bool nz = false;
  int before = 0;
  if (tid < GW_SDNE_MAX_BATCH) {  // whole waves
    if (tid < B) {
      const int64_t ri = rowid[i], rj = rowid[tid];
      if ((uint64_t)ri < (uint64_t)u0 && (uint64_t)rj < (uint64_t)u0) {  // N = u0 was checked when the rows were set
        const float aij = x[(int64_t)i * u0 + rj];
        const float aji = x[(int64_t)tid * u0 + ri];
        s = aij + aji;
        nz = s != 0.0f;
      }
    }
    const unsigned long long mask = __ballot(nz);
    before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) cnt[wv] = __popcll(mask);
  }
  __syncthreads();
  int n = 0;
#pragma unroll
  for (int w = 0; w < kW; ++w) {
    if (w == wv && nz) {
      Sv[n + before] = s;
      Sj[n + before] = tid;
    }
    n += cnt[w];
  }
  __syncthreads();
  for (int c = tid; c < u2; c += kThreads) {
    const float zi = z2[(int64_t)i * u2 + c];
    float acc = 0.0f;
#pragma unroll 4
    for (int k = 0; k < n; ++k) {
      const float d = zi - z2[(int64_t)Sj[k] * u2 + c];
      acc = fmaf(Sv[k], d, acc);
    }
    g1[(int64_t)i * u2 + c] = coef * acc;
  }
}

// qk[0] = q, qk[1] = klg
__global__ __launch_bounds__(GW_SDNE_MAX_BATCH) void k_sdne_q(const float* __restrict__ h2, int B, int u2, float p,
                                                               float klw, float* __restrict__ qk) {
  __shared__ float rs[GW_SDNE_MAX_BATCH];
  const int b = threadIdx.x;
  if (b < B) {
    float s = 0.0f;
#pragma unroll 4
    for (int j = 0; j < u2; ++j) s = s + h2[b * u2 + j];
    rs[b] = s;
  }
  __syncthreads();
  if (b == 0) {
    float qs = 0.0f;
    for (int i = 0; i < B; ++i) qs = qs + rs[i];
    const float count = (float)(B * u2);
    const float q = qs / count;
    qk[0] = q;
    qk[1] = gw_sdne_kl_grad(q, p, klw, count);
  }
}

struct BiasArgs {
  const float* dz[4];
  float *b[4], *am[4], *av[4], *g[4];
  int width[4];
  int B;
  float wd;
  int adam;
  gw_sdne_adam_c C;
};

__global__ __launch_bounds__(kThreads) void k_sdne_bias(const BiasArgs A) {
  int j = blockIdx.x * kThreads + threadIdx.x;
  int l = 0;
  while (l < 4 && j >= A.width[l]) j -= A.width[l++];
  if (l == 4) return;
  const int J = A.width[l];
  const float* dz = A.dz[l];
  float s = 0.0f;
#pragma unroll 4
  for (int b = 0; b < A.B; ++b) s = s + dz[(int64_t)b * J + j];
  const float g = fmaf(A.wd, A.b[l][j], s);
  if (A.adam)
    gw_sdne_adam(&A.b[l][j], &A.am[l][j], &A.av[l][j], g, A.C);
  else
    A.g[l][j] = g;
}

struct LossArgs {
  const float *y, *x;
  int64_t nyx;
  const float* par[8];
  int64_t n[8];
  double bw;
  // the first-order term (z2 = NULL: none)
  const float* z2;
  const int64_t* rowid;
  int B, u0, u2;
};

// lpart[3 * block + {0, 1, 2}] = the block's share of sum(w * (y - x)^2), of sum(theta^2) and of
// sum(a_ij * |z2_i - z2_j|^2) (fp64)
__global__ __launch_bounds__(kThreads) void k_sdne_loss_part(const LossArgs L, double* __restrict__ lpart) {
  __shared__ double red[3][kThreads];
  const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x, stride = (int64_t)gridDim.x * kThreads;
  double rec = 0.0, reg = 0.0, l1 = 0.0;
  for (int64_t i = gid; i < L.nyx; i += stride) {
    const float xv = L.x[i];
    const double d = (double)L.y[i] - (double)xv;
    rec += (xv != 0.0f ? L.bw : 1.0) * (d * d);
  }
  if (L.z2)
    for (int p = blockIdx.x; p < L.B * L.B; p += gridDim.x) {  // a pair (i, j) per trip, the threads over c
      const int i = p / L.B, j = p % L.B;
      const int64_t rj = L.rowid[j];
      if ((uint64_t)rj >= (uint64_t)L.u0) continue;
      const double a = (double)L.x[(int64_t)i * L.u0 + rj];
      if (a == 0.0) continue;
      double sq = 0.0;
      for (int c = threadIdx.x; c < L.u2; c += kThreads) {
        const double d = (double)L.z2[(int64_t)i * L.u2 + c] - (double)L.z2[(int64_t)j * L.u2 + c];
        sq += d * d;
      }
      l1 += a * sq;
    }
  for (int t = 0; t < 8; ++t)
    for (int64_t i = gid; i < L.n[t]; i += stride) {
      const double v = (double)L.par[t][i];
      reg += v * v;
    }
  red[0][threadIdx.x] = rec;
  red[1][threadIdx.x] = reg;
  red[2][threadIdx.x] = l1;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
      red[2][threadIdx.x] += red[2][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    lpart[3 * blockIdx.x] = red[0][0];
    lpart[3 * blockIdx.x + 1] = red[1][0];
    lpart[3 * blockIdx.x + 2] = red[2][0];
  }
}

__global__ void k_sdne_loss_final(const double* __restrict__ lpart, int nblocks, const float* __restrict__ qk, double p,
                                  double klw, double wd, double B, double alpha, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double rec = 0.0, reg = 0.0, l1 = 0.0;
  for (int i = 0; i < nblocks; ++i) {
    rec += lpart[3 * i];
    reg += lpart[3 * i + 1];
    l1 += lpart[3 * i + 2];
  }
  const double q = (double)qk[0];
  const double kl = p * log(p / (q + 1e-8)) + (1.0 - p) * log((1.0 - p) / (1.0 - q + 1e-8));
  *out = rec / 2.0 / B + wd * reg / 2.0 + klw * kl + alpha / B * l1;
}

bool is_split(int K) { return gw_sdne_chunks(K) > kInKernelChunks; }

// one product and its epilogue; E.kind's fields are the caller's
int launch_gemm(gw_sdne* m, hipStream_t st, Gemm G, const Epi& E) {
  const int64_t tm = (G.M + kT - 1) / kT, tn = (G.N + kT - 1) / kT;
  const int64_t nch = gw_sdne_chunks(G.K);
  const bool split = is_split(G.K);
  if (tm * tn > 0x7FFFFFFF || nch > 65535 || (int64_t)G.M * G.N + kThreads > 0x7FFFFFFFLL * kThreads)
    return gw_sdne_fail(m, GW_ERR_UNSUPPORTED, "a %d x %d x %d product is too large for one launch", G.M, G.N, G.K);
  G.tiles_n = (int)tn;
  G.part = split ? m->dev->part.get() : nullptr;
  k_sdne_gemm<<<dim3((unsigned)(tm * tn), split ? (unsigned)nch : 1u), kThreads, 0, st>>>(G, E);
  if (split) {
    const int64_t n = (int64_t)G.M * G.N;
    k_sdne_reduce<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, st>>>(G.part, G.M, G.N, (int)nch, E);
  }
  return GW_OK;
}

// forward layer l (0..3) of M staged rows; pre / act override the handle's buffers when not NULL
int launch_forward(gw_sdne* m, hipStream_t st, int l, int M, float* pre, bool want_act) {
  gw_sdne_dev& dv = *m->dev;
  const int* u = m->u;
  Gemm G = {};
  G.a = l == 0 ? dv.x.get() : dv.h[l - 1].get();
  G.a_rs = u[l], G.a_ks = 1;
  G.b = dv.par[2 * l].get();
  G.b_ks = u[l + 1], G.b_cs = 1;
  G.M = M, G.N = u[l + 1], G.K = u[l];
  Epi E = {};
  E.kind = EPI_FWD;
  E.bias = dv.par[2 * l + 1].get();
  E.pre = pre ? pre : dv.z[l].get();
  E.act = !want_act ? nullptr : (l == 3 ? dv.dz[3].get() : dv.h[l].get());
  E.xin = l == 3 ? dv.x.get() : nullptr;
  E.Bf = (float)m->B;
  const float bf = (float)m->p.nonzero_weight;
  E.bw = bf * bf;
  return launch_gemm(m, st, G, E);
}

// stage M rows: step t's batch (step = true, M = B) or rows [row0, row0 + M)
int launch_batch(gw_sdne* m, hipStream_t st, bool step, uint64_t t, int64_t row0, int M) {
  gw_sdne_dev& dv = *m->dev;
  RowSel R = {};
  R.step = step, R.shuffle = m->p.shuffle;
  R.seed = m->p.seed, R.t = t;
  R.N = m->N, R.B = m->B, R.row0 = row0;
  k_sdne_batch<<<M, kThreads, 0, st>>>(dv.x.get(), m->u[0], m->sparse ? nullptr : m->rows, m->pitch, dv.offs.get(),
                                       dv.cols.get(), dv.vals.get(), R, dv.rowid.get());
  return GW_OK;
}

// one step's chain; adam = 0: gradients only (into dv.grad, nothing updated)
int launch_step(gw_sdne* m, uint64_t t, int adam, double* loss_dev, hipStream_t st) {
  gw_sdne_dev& dv = *m->dev;
  const int* u = m->u;
  const int B = m->B;
  const double alpha = m->p.first_order;
  const gw_sdne_adam_c C = gw_sdne_adam_consts(m->p.learning_rate, m->p.beta1, m->p.beta2, m->p.epsilon, t);
  const float wd = (float)m->p.weight_decay;
  int rc = launch_batch(m, st, true, t, 0, B);
  for (int l = 0; l < 4 && rc == GW_OK; ++l) {
    rc = launch_forward(m, st, l, B, nullptr, true);
    if (l == 1 && rc == GW_OK && alpha > 0.0)
      k_sdne_first<<<B, kThreads, 0, st>>>(dv.x.get(), u[0], dv.rowid.get(), dv.z[1].get(), B, u[2],
                                           (float)(2.0 * alpha / (double)B), dv.g1.get());
  }
  if (rc != GW_OK) return rc;
  k_sdne_q<<<1, GW_SDNE_MAX_BATCH, 0, st>>>(dv.h[1].get(), B, u[2], (float)m->p.kl_target, (float)m->p.kl_weight,
                                            dv.q.get());
  if (loss_dev) {
    LossArgs L = {};
    L.y = dv.z[3].get();
    L.x = dv.x.get();
    L.nyx = (int64_t)B * u[0];
    for (int t8 = 0; t8 < 8; ++t8) {
      L.par[t8] = dv.par[t8].get();
      L.n[t8] = (int64_t)gw_sdne_numel(m, t8);
    }
    const float bf = (float)m->p.nonzero_weight;
    L.bw = (double)(bf * bf);
    L.z2 = alpha > 0.0 ? dv.z[1].get() : nullptr;
    L.rowid = dv.rowid.get();
    L.B = B, L.u0 = u[0], L.u2 = u[2];
    k_sdne_loss_part<<<kLossBlocks, kThreads, 0, st>>>(L, dv.lpart.get());
    k_sdne_loss_final<<<1, 64, 0, st>>>(dv.lpart.get(), kLossBlocks, dv.q.get(), m->p.kl_target, m->p.kl_weight,
                                        m->p.weight_decay, (double)B, alpha, loss_dev);
  }
  // backward data, layers 4 -> 2: dz_l = (dz_{l+1} . W_{l+1}^T [+ klg]) masked by z_l; all against the old weights
  for (int l = 3; l >= 1 && rc == GW_OK; --l) {
    Gemm G = {};
    G.a = dv.dz[l].get();
    G.a_rs = u[l + 1], G.a_ks = 1;
    G.b = dv.par[2 * l].get();  // W_{l+1} [u_l][u_{l+1}], read transposed
    G.b_ks = 1, G.b_cs = u[l + 1];
    G.M = B, G.N = u[l], G.K = u[l + 1];
    Epi E = {};
    E.kind = EPI_BWD;
    E.mask = dv.z[l - 1].get();
    E.klg = l == 2 ? dv.q.get() + 1 : nullptr;
    E.add = l == 2 && alpha > 0.0 ? dv.g1.get() : nullptr;
    E.out = dv.dz[l - 1].get();
    rc = launch_gemm(m, st, G, E);
  }
  // backward weight: dW_l = in_l^T . dz_l, the decay and Adam from the accumulators
  for (int l = 0; l < 4 && rc == GW_OK; ++l) {
    Gemm G = {};
    G.a = l == 0 ? dv.x.get() : dv.h[l - 1].get();
    G.a_rs = 1, G.a_ks = u[l];
    G.b = dv.dz[l].get();
    G.b_ks = u[l + 1], G.b_cs = 1;
    G.M = u[l], G.N = u[l + 1], G.K = B;
    Epi E = {};
    E.kind = EPI_WGT;
    E.W = dv.par[2 * l].get(), E.am = dv.am[2 * l].get(), E.av = dv.av[2 * l].get();
    E.out = dv.grad[2 * l].get();
    E.wd = wd, E.adam = adam, E.C = C;
    rc = launch_gemm(m, st, G, E);
  }
  if (rc != GW_OK) return rc;
  BiasArgs A = {};
  int total = 0;
  for (int l = 0; l < 4; ++l) {
    A.dz[l] = dv.dz[l].get();
    A.b[l] = dv.par[2 * l + 1].get(), A.am[l] = dv.am[2 * l + 1].get(), A.av[l] = dv.av[2 * l + 1].get();
    A.g[l] = dv.grad[2 * l + 1].get();
    A.width[l] = u[l + 1];
    total += u[l + 1];
  }
  A.B = B, A.wd = wd, A.adam = adam, A.C = C;
  k_sdne_bias<<<(total + kThreads - 1) / kThreads, kThreads, 0, st>>>(A);
  GW_DEV_TRY(m, hipGetLastError());
  return GW_OK;
}

}  // namespace

int gw_sdne_dev_alloc(gw_sdne* m, const std::vector<float> init[8]) {
  const int rc = gw_trainer_open_device(m);
  if (rc != GW_OK) return rc;
  GW_DEV_GUARD(m);
  gw_sdne_dev& dv = *m->dev;
  const int* u = m->u;
  const int64_t B = m->B;
  hipError_t e = hipSuccess;
  for (int t = 0; t < 8 && e == hipSuccess; ++t) {
    const size_t n = gw_sdne_numel(m, t);
    e = dv.par[t].alloc((int64_t)n);
    if (e == hipSuccess) e = dv.am[t].alloc((int64_t)n);
    if (e == hipSuccess) e = dv.av[t].alloc((int64_t)n);
    if (e == hipSuccess) e = hipMemcpy(dv.par[t].get(), init[t].data(), n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dv.am[t].get(), 0, n * sizeof(float));
    if (e == hipSuccess) e = hipMemset(dv.av[t].get(), 0, n * sizeof(float));
  }
  if (e == hipSuccess) e = dv.x.alloc(B * u[0]);
  if (e == hipSuccess) e = dv.rowid.alloc(B);
  if (e == hipSuccess) e = dv.g1.alloc(B * u[2]);
  for (int l = 0; l < 4 && e == hipSuccess; ++l) {
    e = dv.z[l].alloc(B * u[l + 1]);
    if (e == hipSuccess) e = dv.dz[l].alloc(B * u[l + 1]);
    if (e == hipSuccess && l < 3) e = dv.h[l].alloc(B * u[l + 1]);
  }
  // the chunk partials of the longest split product: forward (K = u_l, B x u_{l+1}) and backward data
  // (K = u_{l+1}, B x u_l); a weight gradient reduces over B <= KC and never splits
  int64_t part = 1;
  for (int l = 0; l < 4; ++l) {
    if (is_split(u[l])) part = std::max(part, gw_sdne_chunks(u[l]) * B * u[l + 1]);
    if (is_split(u[l + 1])) part = std::max(part, gw_sdne_chunks(u[l + 1]) * B * u[l]);
  }
  if (e == hipSuccess) e = dv.part.alloc(part);
  if (e == hipSuccess) e = dv.q.alloc(2);
  if (e == hipSuccess) e = dv.lpart.alloc(3 * kLossBlocks);
  if (e != hipSuccess) return gw_sdne_fail(m, GW_ERR_NOMEM, "device allocation failed: %s", hipGetErrorString(e));
  return GW_OK;
}

void gw_sdne_dev_free(gw_sdne* m) {
  gw_device_guard dg(m->device);
  delete m->dev;
  m->dev = nullptr;
}

int gw_sdne_dev_set_rows(gw_sdne* m) {
  GW_DEV_GUARD(m);
  gw_sdne_dev& dv = *m->dev;
  GW_DEV_TRY(m, hipDeviceSynchronize());  // nothing of an earlier call still reads the buffers regrown here
  hipError_t e = dv.enc.grow(m->N * m->u[2]);
  if (e == hipSuccess && m->sparse) {
    const int64_t nnz = (int64_t)m->cols.size();
    e = dv.offs.grow(m->N + 1);
    if (e == hipSuccess) e = dv.cols.grow(nnz);
    if (e == hipSuccess) e = dv.vals.grow(nnz);
    if (e != hipSuccess) return gw_sdne_fail(m, GW_ERR_NOMEM, "device allocation failed: %s", hipGetErrorString(e));
    GW_DEV_TRY(m, hipMemcpy(dv.offs.get(), m->offs.data(), (size_t)(m->N + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (nnz > 0) {
      GW_DEV_TRY(m, hipMemcpy(dv.cols.get(), m->cols.data(), (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
      GW_DEV_TRY(m, hipMemcpy(dv.vals.get(), m->vals.data(), (size_t)nnz * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  if (e != hipSuccess) return gw_sdne_fail(m, GW_ERR_NOMEM, "device allocation failed: %s", hipGetErrorString(e));
  GW_DEV_TRY(m, hipMemset(dv.enc.get(), 0, (size_t)(m->N * m->u[2]) * sizeof(float)));
  return GW_OK;
}

int gw_sdne_dev_train(gw_sdne* m, int64_t step_begin, int64_t step_count, double* loss_out, void* stream) {
  GW_DEV_GUARD(m);
  gw_sdne_dev& dv = *m->dev;
  hipStream_t st = (hipStream_t)stream;
  if (loss_out && dv.loss.grow(step_count) != hipSuccess)
    return gw_sdne_fail(m, GW_ERR_NOMEM, "device allocation failed");
  for (int64_t i = 0; i < step_count; ++i) {
    const int rc = launch_step(m, (uint64_t)(step_begin + i), 1, loss_out ? dv.loss.get() + i : nullptr, st);
    if (rc != GW_OK) return rc;
  }
  const size_t loss_bytes = (size_t)step_count * sizeof(double);
  if (loss_out) GW_DEV_TRY(m, hipMemcpyAsync(loss_out, dv.loss.get(), loss_bytes, hipMemcpyDeviceToHost, st));
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  return GW_OK;
}

int gw_sdne_dev_gradients(gw_sdne* m, int64_t step, float* const grads[8]) {
  GW_DEV_GUARD(m);
  gw_sdne_dev& dv = *m->dev;
  for (int t = 0; t < 8; ++t)
    if (dv.grad[t].grow((int64_t)gw_sdne_numel(m, t)) != hipSuccess)
      return gw_sdne_fail(m, GW_ERR_NOMEM, "device allocation failed");
  GW_DEV_TRY(m, hipDeviceSynchronize());
  const int rc = launch_step(m, (uint64_t)step, 0, nullptr, nullptr);
  if (rc != GW_OK) return rc;
  GW_DEV_TRY(m, hipDeviceSynchronize());
  for (int t = 0; t < 8; ++t)
    if (grads[t])
      GW_DEV_TRY(m, hipMemcpy(grads[t], dv.grad[t].get(), gw_sdne_numel(m, t) * sizeof(float), hipMemcpyDeviceToHost));
  return GW_OK;
}

int gw_sdne_dev_batch_rows(gw_sdne* m, int64_t step, int64_t* rows) {
  GW_DEV_GUARD(m);
  GW_DEV_TRY(m, hipDeviceSynchronize());
  launch_batch(m, nullptr, true, (uint64_t)step, 0, m->B);
  GW_DEV_TRY(m, hipGetLastError());
  GW_DEV_TRY(m, hipDeviceSynchronize());
  GW_DEV_TRY(m, hipMemcpy(rows, m->dev->rowid.get(), (size_t)m->B * sizeof(int64_t), hipMemcpyDeviceToHost));
  return GW_OK;
}

int gw_sdne_dev_encode(gw_sdne* m, int64_t row_begin, int64_t row_count, float* out) {
  GW_DEV_GUARD(m);
  gw_sdne_dev& dv = *m->dev;
  const int64_t u2 = m->u[2], end = row_begin + row_count;
  GW_DEV_TRY(m, hipDeviceSynchronize());  // the rows' producer and any training call are complete
  for (int64_t r0 = row_begin; r0 < end; r0 += m->B) {
    const int M = (int)std::min<int64_t>(m->B, end - r0);
    int rc = launch_batch(m, nullptr, false, 0, r0, M);
    if (rc == GW_OK) rc = launch_forward(m, nullptr, 0, M, nullptr, true);
    if (rc == GW_OK) rc = launch_forward(m, nullptr, 1, M, dv.enc.get() + r0 * u2, false);
    if (rc != GW_OK) return rc;
  }
  GW_DEV_TRY(m, hipGetLastError());
  GW_DEV_TRY(m, hipDeviceSynchronize());
  if (out)
    GW_DEV_TRY(m, hipMemcpy(out, dv.enc.get() + row_begin * u2, (size_t)(row_count * u2) * sizeof(float),
                            hipMemcpyDeviceToHost));
  return GW_OK;
}

int gw_sdne_dev_export(gw_sdne* m, float* const par[8], float* const am[8], float* const av[8]) {
  GW_DEV_GUARD(m);
  gw_sdne_dev& dv = *m->dev;
  GW_DEV_TRY(m, hipDeviceSynchronize());
  for (int t = 0; t < 8; ++t) {
    const size_t bytes = gw_sdne_numel(m, t) * sizeof(float);
    if (par && par[t]) GW_DEV_TRY(m, hipMemcpy(par[t], dv.par[t].get(), bytes, hipMemcpyDeviceToHost));
    if (am && am[t]) GW_DEV_TRY(m, hipMemcpy(am[t], dv.am[t].get(), bytes, hipMemcpyDeviceToHost));
    if (av && av[t]) GW_DEV_TRY(m, hipMemcpy(av[t], dv.av[t].get(), bytes, hipMemcpyDeviceToHost));
  }
  return GW_OK;
}

extern "C" int gw_sdne_kernel_attrs(gw_sdne* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                                    int32_t* lds_bytes, int32_t* count) {
  if (!m) return gw_sdne_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (m->device < 0) return gw_sdne_fail(m, GW_ERR_STATE, "host evaluation launches no kernel");
  GW_DEV_GUARD(m);
  const gw_kernel_entry ks[] = {
      {"k_sdne_batch", (const void*)k_sdne_batch, 0},           {"k_sdne_gemm", (const void*)k_sdne_gemm, 0},
      {"k_sdne_reduce", (const void*)k_sdne_reduce, 0},         {"k_sdne_q", (const void*)k_sdne_q, 0},
      {"k_sdne_loss_part", (const void*)k_sdne_loss_part, 0},   {"k_sdne_loss_final", (const void*)k_sdne_loss_final, 0},
      {"k_sdne_bias", (const void*)k_sdne_bias, 0},             {"k_sdne_first", (const void*)k_sdne_first, 0}};
  return gw_trainer_kernel_attrs(m, ks, cap, names, vgprs, scratch_bytes, lds_bytes, count);
}

float* gw_sdne_dev_vectors(gw_sdne* m) { return m->dev->enc.get(); }
