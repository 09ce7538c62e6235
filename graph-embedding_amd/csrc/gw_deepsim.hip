// DeepSim trainer kernels (gfx950): the training law of gw_deepsim_law.h.
//
// One step is a fixed chain on the caller's stream, no host round trip:
//   k_ds_batch     one wave per slot: draw, label map, window dedup, table lookup
//   k_ds_hidden    hidden = relu(w1[c] + b1) and the pre-activation, [B][d]
//   k_ds_forward   one workgroup per column tile (TW = 64): hidden chunks in LDS,
//                  hidden x w2 on the fp32 MFMA (32x32x2, a k-ordered fmaf chain),
//                  logits stored, per-row tile maximum and exp-sum
//   k_ds_rowstats  M, S per row from the tile partials (tiles ascending); the loss (one workgroup)
//   k_ds_backward  per column tile: dlogits into LDS, the tile's dhidden partial
//                  against the old w2 (LDS copy), dw2 (its reduction over b is
//                  inside the tile), db2, and Adam on the tile's w2 / b2
//   k_ds_reduce_dh dhidden = tile partials ascending, relu mask
//   k_ds_dw1       dw1 rows (slots ascending, the first slot of a centre owns the row), db1
//   k_ds_adam_w1   dense Adam over w1 and b1
//   k_ds_zero_rows the touched rows of the w1 gradient buffer back to 0
// No float atomics: every sum has the law's order, so two runs give the same
// bits and the host evaluation gives them too.
#include <hip/hip_runtime.h>

#include "gw_deepsim_internal.h"
#include "gw_deepsim_law.h"
#include "gw_trainer_device.h"

// Device state of a gw_deepsim handle (device >= 0); the buffers are freed with it.
struct gw_deepsim_dev {
  gw_dev_buf<float> par[4], am[4], av[4];  // {w1, b1, w2, b2} and their Adam moments
  gw_dev_buf<float> gw1;                   // [V][dim] gradient rows of w1, all 0 between steps
  bool gw1_dirty = false;        // a call ended before its rows were zeroed again: the next call clears gw1
  gw_dev_buf<float> gsmall;      // gb1 [dim]
  gw_dev_buf<float> gw2;         // diagnostic [dim][V] + gb2 [V], allocated by gw_deepsim_gradients
  gw_dev_buf<float> logits;      // [B][V]
  gw_dev_buf<float> hidden;      // [B][dim] hidden, then [B][dim] pre-activation
  gw_dev_buf<float> tmax, tsum;  // [ntiles][B] each
  gw_dev_buf<float> rowM;        // [B] M, then [B] S
  gw_dev_buf<float> part;        // [ntiles][B][dim]
  gw_dev_buf<float> dh;          // [B][dim]
  gw_dev_buf<int32_t> centre, tgt_id, tgt_n, tab_id, tab_cnt, elig_len;
  gw_dev_buf<float> tgt_val, ysum, tab_val, tem;
  gw_dev_buf<int64_t> labels, elig;
  gw_dev_buf<double> loss;  // per-step losses of one train call
};

namespace {

constexpr int kTW = GW_DS_TW;
constexpr int kThreads = 256;
constexpr int kKC = 32;            // hidden columns per LDS chunk of the forward
constexpr int kHsPitch = kKC + 1;  // conflict-free column reads
constexpr int kLtPitch = kTW + 1;
constexpr int kMaxW = 2 * GW_DS_MAX_WINDOW + 1;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct DsArgs {
  int64_t V;
  int B, d, k, W, ntiles, topk, fallback;
  uint64_t seed;
  const int32_t* walks;
  int walk_len;
  const int64_t* labels;  // NULL: identity
  int64_t n_labels;
  const int64_t* elig;
  const int32_t* elig_len;
  int64_t n_elig;
  const int32_t* tab_id;
  const int32_t* tab_cnt;
  const float* tab_val;
  const float* tem;
  int32_t* centre;
  int32_t* tgt_id;
  float* tgt_val;
  int32_t* tgt_n;
  float* ysum;
  float *w1, *b1, *w2, *b2;
  float *m1, *mb1, *m2, *mb2;
  float *v1, *vb1, *v2, *vb2;
  float* gw1;
  float* gb1;
  float* gw2;  // gradient-only evaluation: [d][V], then gb2 [V]
  float* logits;
  float* hidden;  // [B][d] hidden, [B][d] pre-activation
  float* tmax;
  float* tsum;
  float* rowM;  // [B] M, [B] S
  float* part;
  float* dh;
};

__global__ void k_ds_scan(const int32_t* __restrict__ walks, int64_t nwalks, int walk_len, const int64_t* labels,
                          int64_t n_labels, int64_t V, int32_t* __restrict__ len, unsigned long long* flag) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nwalks) return;
  const int32_t* row = walks + w * (int64_t)walk_len;
  const int64_t lim = labels ? n_labels : V;
  int i = 0;
  for (; i < walk_len; ++i) {
    const int32_t v = row[i];
    if (v == -1) break;
    const int64_t mv = v < 0 || v >= lim ? -1 : (labels ? labels[v] : (int64_t)v);
    if (mv < 0 || mv >= V) {
      atomicMax(flag, (unsigned long long)(w + 1));
      break;
    }
  }
  len[w] = i;
}

__global__ __launch_bounds__(64) void k_ds_batch(const DsArgs A, uint64_t t) {
  __shared__ int32_t tok[kMaxW];
  __shared__ int32_t uniq[kMaxW];
  __shared__ int32_t first[kMaxW];
  __shared__ float vals[kMaxW];
  __shared__ int nuniq;
  const int s = blockIdx.x, lane = threadIdx.x;
  const int k = A.k, W = A.W;
  uint64_t e = gw_ds_walk_slot(A.seed, t, (uint32_t)s, (uint64_t)A.n_elig);
  if (e >= (uint64_t)A.n_elig) e = 0;  // cannot happen: a permutation of [0, n_elig)
  const int64_t w = A.elig[e];
  const int len = A.elig_len[e];
  const int pos = gw_ds_pos(A.seed, t, (uint32_t)s, len, k);
  const int32_t* row = A.walks + w * (int64_t)A.walk_len;
  const int64_t lim = A.labels ? A.n_labels : A.V;
  for (int i = lane; i < W; i += 64) {
    // tokens were range-checked by gw_deepsim_set_walks; the clamps only keep a
    // matrix changed since then inside the buffers
    int64_t v = row[pos - k + i];
    v = v < 0 ? 0 : (v >= lim ? lim - 1 : v);
    if (A.labels) v = A.labels[v];
    v = v < 0 ? 0 : (v >= A.V ? A.V - 1 : v);
    tok[i] = (int32_t)v;
  }
  __syncthreads();
  for (int i = lane; i < W; i += 64) {
    const int32_t v = tok[i];
    int f = 1;
    for (int q = 0; q < i; ++q) f = tok[q] == v ? 0 : f;
    first[i] = f;
  }
  __syncthreads();
  if (lane == 0) {
    int n = 0;
    for (int i = 0; i < W; ++i)
      if (first[i]) uniq[n++] = tok[i];
    nuniq = n;
  }
  __syncthreads();
  const int n = nuniq;
  const int32_t c = tok[k];
  const float fb = A.fallback == GW_DEEPSIM_FALLBACK_ROW_MIN ? A.tem[c] : A.tem[pos < A.V ? pos : 0];
  for (int q = lane; q < W; q += 64) {
    int32_t id = -1;
    float val = 0.0f;
    if (q < n) {
      id = uniq[q];
      val = gw_ds_lookup(A.tab_id + (int64_t)c * A.topk, A.tab_val + (int64_t)c * A.topk, A.tab_cnt[c], id, fb);
    }
    vals[q] = val;
    A.tgt_id[(int64_t)s * W + q] = id;
    A.tgt_val[(int64_t)s * W + q] = val;
  }
  __syncthreads();
  if (lane == 0) {
    float ys = 0.0f;
    for (int q = 0; q < n; ++q) ys = ys + vals[q];
    A.ysum[s] = ys;
    A.centre[s] = c;
    A.tgt_n[s] = n;
  }
}

__global__ void k_ds_hidden(const DsArgs A) {
  const int b = blockIdx.x, h = threadIdx.x;
  const float x = A.w1[(int64_t)A.centre[b] * A.d + h] + A.b1[h];
  A.hidden[b * A.d + h] = x > 0.0f ? x : 0.0f;
  A.hidden[(A.B + b) * A.d + h] = x;
}

__global__ __launch_bounds__(kThreads) void k_ds_forward(const DsArgs A) {
  extern __shared__ float lds[];
  float* hs = lds;                      // [B][kHsPitch]
  float* lt = lds + A.B * kHsPitch;     // [B][kLtPitch]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int B = A.B, d = A.d;
  const int64_t V = A.V, j0 = (int64_t)blockIdx.x * kTW;
  const float* __restrict__ hid = A.hidden;
  const float* __restrict__ w2 = A.w2;
  // 32x32 output blocks of the [B][64] tile: block q -> rows 32*(q>>1).., columns 32*(q&1)..;
  // wave wv owns blocks wv and wv + 4
  const int nblk = (B / 32) * 2;
  const int l31 = lane & 31, lhi = lane >> 5;
  f32x16 acc[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int q = wv + 4 * u;
    const int64_t col = j0 + (q & 1) * 32 + l31;
    const float bias = (q < nblk && col < V) ? A.b2[col] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[u][r] = bias;
  }
  for (int kc = 0; kc < d; kc += kKC) {
    __syncthreads();
    for (int idx = tid; idx < B * kKC; idx += kThreads) {
      const int b = idx / kKC, hh = idx % kKC;
      hs[b * kHsPitch + hh] = hid[b * d + kc + hh];
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < kKC; kk += 2) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int q = wv + 4 * u;
        if (q < nblk) {  // wave-uniform
          const int64_t col = j0 + (q & 1) * 32 + l31;
          const float a = hs[((q >> 1) * 32 + l31) * kHsPitch + kk + lhi];
          const float bv = col < V ? w2[(int64_t)(kc + kk + lhi) * V + col] : 0.0f;
          acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[u], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int q = wv + 4 * u;
    if (q < nblk) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rowi = (q >> 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        lt[rowi * kLtPitch + (q & 1) * 32 + l31] = acc[u][r];
      }
    }
  }
  __syncthreads();
  for (int idx = tid; idx < B * kTW; idx += kThreads) {
    const int b = idx / kTW, jj = idx % kTW;
    if (j0 + jj < V) A.logits[(int64_t)b * V + j0 + jj] = lt[b * kLtPitch + jj];
  }
  if (tid < B) {
    const int jn = (int)(V - j0 < kTW ? V - j0 : kTW);
    const float* l = lt + tid * kLtPitch;
    float mx = l[0];
    for (int jj = 1; jj < jn; ++jj) mx = l[jj] > mx ? l[jj] : mx;
    float s = 0.0f;
    for (int jj = 0; jj < jn; ++jj) s = s + gw_ds_exp(l[jj] - mx);
    A.tmax[(int64_t)blockIdx.x * B + tid] = mx;
    A.tsum[(int64_t)blockIdx.x * B + tid] = s;
  }
}

// M, S of every row from the tile partials and the step's loss.  kRsSeg threads per row: thread (b, s) loads
// its share of the partials at once; the law's chain S = fmaf(s_T, exp(m_T - M), S) over T ascending is then
// walked in runs of kRsRun tiles, segment after segment, the running S handed on through LDS.
constexpr int kRsSeg = 8;
constexpr int kRsRun = 16;

__global__ __launch_bounds__(1024) void k_ds_rowstats(const DsArgs A, double* loss_out) {
  __shared__ float red[kRsSeg][128];
  __shared__ float Srow[128];
  __shared__ double lpart[kRsSeg][128];
  const int B = A.B, b = threadIdx.x % B, s = threadIdx.x / B, nt = A.ntiles;
  float mx = -INFINITY;
#pragma unroll 4
  for (int T = s; T < nt; T += kRsSeg) {
    const float x = A.tmax[(int64_t)T * B + b];
    mx = x > mx ? x : mx;
  }
  red[s][b] = mx;
  if (s == 0) Srow[b] = 0.0f;
  __syncthreads();
  float M = red[0][b];
#pragma unroll
  for (int i = 1; i < kRsSeg; ++i) M = red[i][b] > M ? red[i][b] : M;
  for (int T0 = 0; T0 < nt; T0 += kRsSeg * kRsRun) {
    const int t0 = T0 + s * kRsRun;
    float e[kRsRun], ts[kRsRun];
#pragma unroll
    for (int i = 0; i < kRsRun; ++i) {
      const bool in = t0 + i < nt;
      ts[i] = in ? A.tsum[(int64_t)(t0 + i) * B + b] : 0.0f;
      e[i] = in ? gw_ds_exp(A.tmax[(int64_t)(t0 + i) * B + b] - M) : 0.0f;
    }
    for (int ph = 0; ph < kRsSeg; ++ph) {
      if (s == ph) {
        float S = Srow[b];
#pragma unroll
        for (int i = 0; i < kRsRun; ++i)
          if (t0 + i < nt) S = fmaf(ts[i], e[i], S);
        Srow[b] = S;
      }
      __syncthreads();
    }
  }
  const float S = Srow[b];
  if (s == 0) {
    A.rowM[b] = M;
    A.rowM[B + b] = S;
  }
  if (!loss_out) return;  // uniform: the loss is computed only when it is asked for
  // loss (fp64, not part of the bit law): the row's targets dealt to its kRsSeg threads
  double lb = 0.0;
  const double logS = log((double)S);
  const int n = A.tgt_n[b];
  for (int q = s; q < n; q += kRsSeg) {
    const int32_t j = A.tgt_id[b * A.W + q];
    lb += (double)A.tgt_val[b * A.W + q] * ((double)A.logits[(int64_t)b * A.V + j] - (double)M - logS);
  }
  lpart[s][b] = lb;
  __syncthreads();
  if (threadIdx.x == 0) {
    double loss = 0.0;
    for (int i = 0; i < B; ++i)
      for (int u = 0; u < kRsSeg; ++u) loss += -lpart[u][i];
    *loss_out = loss / (double)B;
  }
}

// LDS images of the backward tile, both swizzled so that the MFMA operand reads
// (32 lanes along the strided index) and the row-wise fills are conflict-free
__device__ __forceinline__ int w2s_at(int jj, int h, int d) { return jj * d + (h ^ (jj & 31)); }
__device__ __forceinline__ int dl_at(int b, int jj) { return b * kTW + (jj ^ (b & 31)); }

__global__ __launch_bounds__(kThreads) void k_ds_backward(const DsArgs A, const gw_ds_adam_c C, int adam) {
  extern __shared__ float lds[];
  float* dl = lds;                 // [B][kTW]: y, then dlogits; columns past the tile's end hold 0
  float* w2s = lds + A.B * kTW;    // [kTW][d]: the old w2 of the tile; rows past the tile's end hold 0
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lhi = lane >> 5;
  const int B = A.B, d = A.d, W = A.W;
  const int64_t V = A.V, j0 = (int64_t)blockIdx.x * kTW;
  const int jn = (int)(V - j0 < kTW ? V - j0 : kTW);
  const float* __restrict__ hid = A.hidden;
  for (int idx = tid; idx < B * kTW; idx += kThreads) dl[idx] = 0.0f;
  __syncthreads();
  for (int idx = tid; idx < B * W; idx += kThreads) {
    const int b = idx / W, q = idx % W;
    if (q < A.tgt_n[b]) {
      const int64_t j = A.tgt_id[idx];
      if (j >= j0 && j < j0 + jn) dl[dl_at(b, (int)(j - j0))] = A.tgt_val[idx];
    }
  }
  __syncthreads();
  const float Bf = (float)B;
  for (int idx = tid; idx < B * kTW; idx += kThreads) {
    const int b = idx / kTW, jj = idx % kTW;
    const int at = dl_at(b, jj);
    dl[at] = jj < jn ? gw_ds_dlogit(A.logits[(int64_t)b * V + j0 + jj], A.rowM[b], A.rowM[B + b], A.ysum[b], dl[at], Bf)
                     : 0.0f;
  }
  for (int idx = tid; idx < d * kTW; idx += kThreads) {
    const int h = idx / kTW, jj = idx % kTW;
    w2s[w2s_at(jj, h, d)] = jj < jn ? A.w2[(int64_t)h * V + j0 + jj] : 0.0f;
  }
  __syncthreads();
  // The tile's dhidden partial against the old w2: part[b][h] = fmaf chain over the tile's j from +0, on the
  // MFMA (A = dlogits [b][j], B = w2s [j][h]).  Past the tile's end both operands are 0 and fma(0, 0, acc)
  // leaves acc as it is (acc is never -0: it starts at +0), so the chain is the law's jn terms.
  {
    const int nblk = (B / 32) * (d / 32), ncb = d / 32;  // block q: rows 32*(q / ncb).., columns 32*(q % ncb)..
    f32x16 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[u][r] = 0.0f;
#pragma unroll 2
    for (int jj = 0; jj < kTW; jj += 2) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = wv + 4 * u;
        if (q < nblk) {  // wave-uniform
          const float a = dl[dl_at((q / ncb) * 32 + l31, jj + lhi)];
          const float bv = w2s[w2s_at(jj + lhi, (q % ncb) * 32 + l31, d)];
          acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[u], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = wv + 4 * u;
      if (q < nblk) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int b = (q / ncb) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
          A.part[((int64_t)blockIdx.x * B + b) * d + (q % ncb) * 32 + l31] = acc[u][r];
        }
      }
    }
  }
  // dw2[h][j] = fmaf chain over b ascending from +0, on the MFMA (A = hidden^T [h][b], B = dlogits [b][j]);
  // then Adam on the tile's w2 straight from the accumulators
  {
    const int nblk = (d / 32) * 2;  // block q: rows h 32*(q >> 1).., columns 32*(q & 1)..
    f32x16 acc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[u][r] = 0.0f;
#pragma unroll 2
    for (int b = 0; b < B; b += 2) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int q = wv + 4 * u;
        if (q < nblk) {
          const float a = hid[(b + lhi) * d + (q >> 1) * 32 + l31];
          const float bv = dl[dl_at(b + lhi, (q & 1) * 32 + l31)];
          acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[u], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int q = wv + 4 * u;
      const int jj = (q & 1) * 32 + l31;
      if (q < nblk && jj < jn) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int h = (q >> 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
          const int64_t at = (int64_t)h * V + j0 + jj;
          if (adam)
            gw_ds_adam(&A.w2[at], &A.m2[at], &A.v2[at], acc[u][r], C);
          else
            A.gw2[at] = acc[u][r];
        }
      }
    }
  }
  if (tid < jn) {
    float s = 0.0f;
    for (int b = 0; b < B; ++b) s = s + dl[dl_at(b, tid)];
    const int64_t at = j0 + tid;
    if (adam)
      gw_ds_adam(&A.b2[at], &A.mb2[at], &A.vb2[at], s, C);
    else
      A.gw2[(int64_t)d * V + at] = s;
  }
}

__global__ void k_ds_reduce_dh(const DsArgs A) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = A.B * A.d;
  if (o >= n) return;
  float acc = 0.0f;
#pragma unroll 8
  for (int T = 0; T < A.ntiles; ++T) acc = acc + A.part[(int64_t)T * n + o];
  A.dh[o] = A.hidden[n + o] > 0.0f ? acc : 0.0f;
}

__global__ void k_ds_dw1(const DsArgs A) {
  __shared__ int32_t cs[128];
  const int b = blockIdx.x, h = threadIdx.x, B = A.B, d = A.d;
  if (b == B) {
    float s = 0.0f;
#pragma unroll 8
    for (int i = 0; i < B; ++i) s = s + A.dh[i * d + h];
    A.gb1[h] = s;
    return;
  }
  for (int i = h; i < B; i += d) cs[i] = A.centre[i];
  __syncthreads();
  const int32_t c = cs[b];
  for (int i = 0; i < b; ++i)
    if (cs[i] == c) return;  // an earlier slot owns the row
  float acc = 0.0f;
  for (int i = b; i < B; ++i)
    if (cs[i] == c) acc = acc + A.dh[i * d + h];
  A.gw1[(int64_t)c * d + h] = acc;
}

__global__ void k_ds_adam_w1(const DsArgs A, const gw_ds_adam_c C) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < A.V * A.d) gw_ds_adam(&A.w1[i], &A.m1[i], &A.v1[i], A.gw1[i], C);
  if (i < A.d) gw_ds_adam(&A.b1[i], &A.mb1[i], &A.vb1[i], A.gb1[i], C);
}

__global__ void k_ds_zero_rows(const DsArgs A) {
  A.gw1[(int64_t)A.centre[blockIdx.x] * A.d + threadIdx.x] = 0.0f;
}

size_t fwd_lds(const gw_deepsim* m) { return (size_t)m->p.batch * (kHsPitch + kLtPitch) * sizeof(float); }
size_t bwd_lds(const gw_deepsim* m) { return ((size_t)m->p.batch * kTW + (size_t)kTW * m->p.dim) * sizeof(float); }

DsArgs make_args(const gw_deepsim* m) {
  const gw_deepsim_dev& dv = *m->dev;
  DsArgs A = {};
  A.V = m->V;
  A.B = m->p.batch;
  A.d = m->p.dim;
  A.k = m->p.window;
  A.W = m->W;
  A.ntiles = m->ntiles;
  A.topk = m->topk;
  A.fallback = m->p.fallback;
  A.seed = m->p.seed;
  A.walks = m->walks;
  A.walk_len = m->walk_len;
  A.labels = m->has_labels ? dv.labels.get() : nullptr;
  A.n_labels = (int64_t)m->labels.size();
  A.elig = dv.elig.get();
  A.elig_len = dv.elig_len.get();
  A.n_elig = (int64_t)m->elig.size();
  A.tab_id = dv.tab_id.get();
  A.tab_cnt = dv.tab_cnt.get();
  A.tab_val = dv.tab_val.get();
  A.tem = dv.tem.get();
  A.centre = dv.centre.get();
  A.tgt_id = dv.tgt_id.get();
  A.tgt_val = dv.tgt_val.get();
  A.tgt_n = dv.tgt_n.get();
  A.ysum = dv.ysum.get();
  A.w1 = dv.par[0].get(), A.b1 = dv.par[1].get(), A.w2 = dv.par[2].get(), A.b2 = dv.par[3].get();
  A.m1 = dv.am[0].get(), A.mb1 = dv.am[1].get(), A.m2 = dv.am[2].get(), A.mb2 = dv.am[3].get();
  A.v1 = dv.av[0].get(), A.vb1 = dv.av[1].get(), A.v2 = dv.av[2].get(), A.vb2 = dv.av[3].get();
  A.gw1 = dv.gw1.get();
  A.gb1 = dv.gsmall.get();
  A.gw2 = dv.gw2.get();
  A.logits = dv.logits.get();
  A.hidden = dv.hidden.get();
  A.tmax = dv.tmax.get();
  A.tsum = dv.tsum.get();
  A.rowM = dv.rowM.get();
  A.part = dv.part.get();
  A.dh = dv.dh.get();
  return A;
}

// The w1 gradient buffer is all 0 between steps (k_ds_zero_rows ends every step).  A call that ended early
// leaves gw1_dirty set; the next call clears the whole buffer before it launches anything.
int clean_gw1(gw_deepsim* m, hipStream_t st) {
  gw_deepsim_dev& dv = *m->dev;
  if (!dv.gw1_dirty) return GW_OK;
  GW_DEV_TRY(m, hipMemsetAsync(dv.gw1.get(), 0, (size_t)m->V * (size_t)m->p.dim * sizeof(float), st));
  dv.gw1_dirty = false;
  return GW_OK;
}

// one step's chain; adam = 0: gradients only (w2 / b2 gradients into A.gw2, nothing updated)
int launch_step(gw_deepsim* m, const DsArgs& A, uint64_t t, int adam, double* loss_dev, hipStream_t st) {
  const int B = A.B, d = A.d;
  const gw_ds_adam_c C = gw_ds_adam_consts(m->p.learning_rate, m->p.beta1, m->p.beta2, m->p.epsilon, t);
  k_ds_batch<<<B, 64, 0, st>>>(A, t);
  k_ds_hidden<<<B, d, 0, st>>>(A);
  k_ds_forward<<<A.ntiles, kThreads, fwd_lds(m), st>>>(A);
  k_ds_rowstats<<<1, B * kRsSeg, 0, st>>>(A, loss_dev);
  k_ds_backward<<<A.ntiles, kThreads, bwd_lds(m), st>>>(A, C, adam);
  k_ds_reduce_dh<<<(B * d + 255) / 256, 256, 0, st>>>(A);
  k_ds_dw1<<<B + 1, d, 0, st>>>(A);
  if (adam) {
    k_ds_adam_w1<<<(unsigned)((A.V * d + 255) / 256), 256, 0, st>>>(A, C);
    k_ds_zero_rows<<<B, d, 0, st>>>(A);
  }
  GW_DEV_TRY(m, hipGetLastError());
  return GW_OK;
}

}  // namespace

int gw_ds_dev_alloc(gw_deepsim* m, const std::vector<float> init[4]) {
  const int rc = gw_trainer_open_device(m);
  if (rc != GW_OK) return rc;
  GW_DEV_GUARD(m);
  gw_deepsim_dev& dv = *m->dev;
  const int64_t B = m->p.batch, d = m->p.dim, V = m->V, nt = m->ntiles, W = m->W;
  hipError_t e = hipSuccess;
  for (int t = 0; t < 4 && e == hipSuccess; ++t) {
    const size_t n = gw_ds_numel(m, t);
    e = dv.par[t].alloc((int64_t)n);
    if (e == hipSuccess) e = dv.am[t].alloc((int64_t)n);
    if (e == hipSuccess) e = dv.av[t].alloc((int64_t)n);
    if (e == hipSuccess) e = hipMemcpy(dv.par[t].get(), init[t].data(), n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dv.am[t].get(), 0, n * sizeof(float));
    if (e == hipSuccess) e = hipMemset(dv.av[t].get(), 0, n * sizeof(float));
  }
  if (e == hipSuccess) e = dv.gw1.alloc(V * d);
  if (e == hipSuccess) e = hipMemset(dv.gw1.get(), 0, (size_t)(V * d) * sizeof(float));
  if (e == hipSuccess) e = dv.gsmall.alloc(d);
  if (e == hipSuccess) e = dv.logits.alloc(B * V);
  if (e == hipSuccess) e = dv.hidden.alloc(2 * B * d);
  if (e == hipSuccess) e = dv.tmax.alloc(nt * B);
  if (e == hipSuccess) e = dv.tsum.alloc(nt * B);
  if (e == hipSuccess) e = dv.rowM.alloc(2 * B);
  if (e == hipSuccess) e = dv.part.alloc(nt * B * d);
  if (e == hipSuccess) e = dv.dh.alloc(B * d);
  if (e == hipSuccess) e = dv.centre.alloc(B);
  if (e == hipSuccess) e = dv.tgt_id.alloc(B * W);
  if (e == hipSuccess) e = dv.tgt_val.alloc(B * W);
  if (e == hipSuccess) e = dv.tgt_n.alloc(B);
  if (e == hipSuccess) e = dv.ysum.alloc(B);
  if (e == hipSuccess) e = dv.tem.alloc(V);
  if (e == hipSuccess) e = dv.tab_cnt.alloc(V);
  if (e != hipSuccess) return gw_deepsim_fail(m, GW_ERR_NOMEM, "device allocation failed: %s", hipGetErrorString(e));
  return GW_OK;
}

void gw_ds_dev_free(gw_deepsim* m) {
  gw_device_guard dg(m->device);
  delete m->dev;
  m->dev = nullptr;
}

int gw_ds_dev_fetch_table(gw_deepsim* m, const int32_t* ids_dev, const double* scores_dev, int topk,
                          std::vector<int32_t>* ids, std::vector<double>* scores) {
  GW_DEV_GUARD(m);
  const size_t n = (size_t)m->V * (size_t)topk;
  ids->resize(n);
  scores->resize(n);
  GW_DEV_TRY(m, hipDeviceSynchronize());  // the producer (gw_topsim on any stream) is complete
  GW_DEV_TRY(m, hipMemcpy(ids->data(), ids_dev, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  GW_DEV_TRY(m, hipMemcpy(scores->data(), scores_dev, n * sizeof(double), hipMemcpyDeviceToHost));
  return GW_OK;
}

int gw_ds_dev_upload_table(gw_deepsim* m) {
  GW_DEV_GUARD(m);
  gw_deepsim_dev& dv = *m->dev;
  const size_t n = (size_t)m->V * (size_t)m->topk;
  hipError_t e = dv.tab_id.alloc((int64_t)n);
  if (e == hipSuccess) e = dv.tab_val.alloc((int64_t)n);
  if (e != hipSuccess) return gw_deepsim_fail(m, GW_ERR_NOMEM, "device allocation failed: %s", hipGetErrorString(e));
  GW_DEV_TRY(m, hipMemcpy(dv.tab_id.get(), m->tab_id.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
  GW_DEV_TRY(m, hipMemcpy(dv.tab_val.get(), m->tab_val.data(), n * sizeof(float), hipMemcpyHostToDevice));
  GW_DEV_TRY(m, hipMemcpy(dv.tab_cnt.get(), m->tab_cnt.data(), (size_t)m->V * sizeof(int32_t), hipMemcpyHostToDevice));
  GW_DEV_TRY(m, hipMemcpy(dv.tem.get(), m->tem.data(), (size_t)m->V * sizeof(float), hipMemcpyHostToDevice));
  return GW_OK;
}

int gw_ds_dev_scan_walks(gw_deepsim* m, std::vector<int32_t>* len) {
  GW_DEV_GUARD(m);
  gw_deepsim_dev& dv = *m->dev;
  dv.labels.reset();
  if (m->has_labels) {
    const size_t n = m->labels.size();
    if (dv.labels.alloc((int64_t)n) != hipSuccess) return gw_deepsim_fail(m, GW_ERR_NOMEM, "device allocation failed");
    GW_DEV_TRY(m, hipMemcpy(dv.labels.get(), m->labels.data(), n * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  if (m->nwalks == 0) return GW_OK;
  const int64_t blocks = (m->nwalks + 255) / 256;
  if (blocks > 0x7FFFFFFF) return gw_deepsim_fail(m, GW_ERR_UNSUPPORTED, "too many walks for one launch");
  gw_dev_buf<int32_t> d_len;
  gw_dev_buf<unsigned long long> d_flag;
  if (d_len.alloc(m->nwalks) != hipSuccess || d_flag.alloc(1) != hipSuccess)
    return gw_deepsim_fail(m, GW_ERR_NOMEM, "device allocation failed");
  unsigned long long bad = 0;
  hipError_t e = hipDeviceSynchronize();  // the walks' producer is complete
  if (e == hipSuccess) e = hipMemset(d_flag.get(), 0, sizeof bad);
  if (e == hipSuccess) {
    k_ds_scan<<<(unsigned)blocks, 256>>>(m->walks, m->nwalks, m->walk_len, dv.labels.get(), (int64_t)m->labels.size(),
                                         m->V, d_len.get(), d_flag.get());
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(&bad, d_flag.get(), sizeof bad, hipMemcpyDeviceToHost);
  if (e == hipSuccess)
    e = hipMemcpy(len->data(), d_len.get(), (size_t)m->nwalks * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return gw_deepsim_fail(m, GW_ERR_DEVICE, "walk scan: %s", hipGetErrorString(e));
  if (bad)
    return gw_deepsim_fail(m, GW_ERR_RANGE, "walk %lld holds a token that maps outside [0, %lld)", (long long)bad - 1,
                           (long long)m->V);
  return GW_OK;
}

int gw_ds_dev_upload_elig(gw_deepsim* m) {
  GW_DEV_GUARD(m);
  gw_deepsim_dev& dv = *m->dev;
  const size_t n = m->elig.size();
  if (dv.elig.alloc((int64_t)n) != hipSuccess || dv.elig_len.alloc((int64_t)n) != hipSuccess)
    return gw_deepsim_fail(m, GW_ERR_NOMEM, "device allocation failed");
  GW_DEV_TRY(m, hipMemcpy(dv.elig.get(), m->elig.data(), n * sizeof(int64_t), hipMemcpyHostToDevice));
  GW_DEV_TRY(m, hipMemcpy(dv.elig_len.get(), m->elig_len.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
  return GW_OK;
}

int gw_ds_dev_train(gw_deepsim* m, int64_t step_begin, int64_t step_count, double* loss_out, void* stream) {
  GW_DEV_GUARD(m);
  gw_deepsim_dev& dv = *m->dev;
  hipStream_t st = (hipStream_t)stream;
  if (loss_out && dv.loss.grow(step_count) != hipSuccess)
    return gw_deepsim_fail(m, GW_ERR_NOMEM, "device allocation failed");
  const DsArgs A = make_args(m);
  int rc = clean_gw1(m, st);
  if (rc != GW_OK) return rc;
  dv.gw1_dirty = true;
  for (int64_t i = 0; i < step_count; ++i) {
    rc = launch_step(m, A, (uint64_t)(step_begin + i), 1, loss_out ? dv.loss.get() + i : nullptr, st);
    if (rc != GW_OK) return rc;
  }
  const size_t loss_bytes = (size_t)step_count * sizeof(double);
  if (loss_out) GW_DEV_TRY(m, hipMemcpyAsync(loss_out, dv.loss.get(), loss_bytes, hipMemcpyDeviceToHost, st));
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  dv.gw1_dirty = false;
  return GW_OK;
}

int gw_ds_dev_gradients(gw_deepsim* m, int64_t step, float* gw1, float* gb1, float* gw2, float* gb2) {
  GW_DEV_GUARD(m);
  gw_deepsim_dev& dv = *m->dev;
  const size_t V = (size_t)m->V, d = (size_t)m->p.dim;
  if (dv.gw2.grow((int64_t)(d * V + V)) != hipSuccess)
    return gw_deepsim_fail(m, GW_ERR_NOMEM, "device allocation failed");
  const DsArgs A = make_args(m);
  int rc = clean_gw1(m, nullptr);
  if (rc != GW_OK) return rc;
  dv.gw1_dirty = true;  // until the rows this step writes are zero again, whichever way this call ends
  rc = launch_step(m, A, (uint64_t)step, 0, nullptr, nullptr);
  if (rc != GW_OK) return rc;
  GW_DEV_TRY(m, hipDeviceSynchronize());
  if (gw1) GW_DEV_TRY(m, hipMemcpy(gw1, dv.gw1.get(), V * d * sizeof(float), hipMemcpyDeviceToHost));
  if (gb1) GW_DEV_TRY(m, hipMemcpy(gb1, dv.gsmall.get(), d * sizeof(float), hipMemcpyDeviceToHost));
  if (gw2) GW_DEV_TRY(m, hipMemcpy(gw2, dv.gw2.get(), d * V * sizeof(float), hipMemcpyDeviceToHost));
  if (gb2) GW_DEV_TRY(m, hipMemcpy(gb2, dv.gw2.get() + d * V, V * sizeof(float), hipMemcpyDeviceToHost));
  k_ds_zero_rows<<<A.B, A.d>>>(A);
  GW_DEV_TRY(m, hipGetLastError());
  GW_DEV_TRY(m, hipDeviceSynchronize());
  dv.gw1_dirty = false;
  return GW_OK;
}

int gw_ds_dev_batch(gw_deepsim* m, int64_t step, int32_t* centre, int32_t* tgt_id, float* tgt_val, int32_t* tgt_n,
                    float* ysum) {
  GW_DEV_GUARD(m);
  gw_deepsim_dev& dv = *m->dev;
  const DsArgs A = make_args(m);
  const size_t B = (size_t)A.B, W = (size_t)A.W;
  k_ds_batch<<<A.B, 64>>>(A, (uint64_t)step);
  GW_DEV_TRY(m, hipGetLastError());
  GW_DEV_TRY(m, hipDeviceSynchronize());
  if (centre) GW_DEV_TRY(m, hipMemcpy(centre, dv.centre.get(), B * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (tgt_id) GW_DEV_TRY(m, hipMemcpy(tgt_id, dv.tgt_id.get(), B * W * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (tgt_val) GW_DEV_TRY(m, hipMemcpy(tgt_val, dv.tgt_val.get(), B * W * sizeof(float), hipMemcpyDeviceToHost));
  if (tgt_n) GW_DEV_TRY(m, hipMemcpy(tgt_n, dv.tgt_n.get(), B * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (ysum) GW_DEV_TRY(m, hipMemcpy(ysum, dv.ysum.get(), B * sizeof(float), hipMemcpyDeviceToHost));
  return GW_OK;
}

int gw_ds_dev_export(gw_deepsim* m, float* const par[4], float* const am[4], float* const av[4]) {
  GW_DEV_GUARD(m);
  gw_deepsim_dev& dv = *m->dev;
  GW_DEV_TRY(m, hipDeviceSynchronize());
  for (int t = 0; t < 4; ++t) {
    const size_t bytes = gw_ds_numel(m, t) * sizeof(float);
    if (par && par[t]) GW_DEV_TRY(m, hipMemcpy(par[t], dv.par[t].get(), bytes, hipMemcpyDeviceToHost));
    if (am && am[t]) GW_DEV_TRY(m, hipMemcpy(am[t], dv.am[t].get(), bytes, hipMemcpyDeviceToHost));
    if (av && av[t]) GW_DEV_TRY(m, hipMemcpy(av[t], dv.av[t].get(), bytes, hipMemcpyDeviceToHost));
  }
  return GW_OK;
}

extern "C" int gw_deepsim_kernel_attrs(gw_deepsim* m, int cap, const char** names, int32_t* vgprs,
                                       int32_t* scratch_bytes, int32_t* lds_bytes, int32_t* count) {
  if (!m) return gw_deepsim_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (m->device < 0) return gw_deepsim_fail(m, GW_ERR_STATE, "host evaluation launches no kernel");
  GW_DEV_GUARD(m);
  const gw_kernel_entry ks[] = {
      {"k_ds_batch", (const void*)k_ds_batch, 0},
      {"k_ds_hidden", (const void*)k_ds_hidden, 0},
      {"k_ds_forward", (const void*)k_ds_forward, fwd_lds(m)},
      {"k_ds_rowstats", (const void*)k_ds_rowstats, 0},
      {"k_ds_backward", (const void*)k_ds_backward, bwd_lds(m)},
      {"k_ds_reduce_dh", (const void*)k_ds_reduce_dh, 0},
      {"k_ds_dw1", (const void*)k_ds_dw1, 0},
      {"k_ds_adam_w1", (const void*)k_ds_adam_w1, 0},
      {"k_ds_zero_rows", (const void*)k_ds_zero_rows, 0}};
  return gw_trainer_kernel_attrs(m, ks, cap, names, vgprs, scratch_bytes, lds_bytes, count);
}

float* gw_ds_dev_vectors(gw_deepsim* m) { return m->dev->par[0].get(); }
