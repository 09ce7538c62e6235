// Neighbour-graph kernels (gfx950): the law of gw_nng_law.h.
//
//   k_nng_check   every source lies in [0, n): the first offending entry, by integer atomic min
//   k_nng_main    k_knn_main's plan (gw_knn.hip) with a squared distance where that has a dot
//                 product: one workgroup per tile of kTQ source rows streams tiles of kTC
//                 candidate rows through LDS in chunks of kKC columns (fp32, column-major with
//                 an XOR swizzle, so that staging stores and 16 B reads are free of bank
//                 conflicts); every lane keeps a 4 x 4 tile of fp64 accumulators and walks k
//                 strictly ascending, one subtract and one fma per pair and column, so each
//                 d2 has the law's bits whatever the tiling.  Behind each finished candidate
//                 tile the distances pass through LDS to the selection: a row belongs to one
//                 wave, which appends the candidates that beat the row's bound (its current
//                 last kept entry under the law's ascending order) to the row's buffer in LDS
//                 by ballot and prefix count, and compacts a full buffer to its best entries
//                 by rank, which leaves it sorted and lowers the bound.  After the last tile
//                 one more compaction sorts the row; the epilogue turns d2 into the heat
//                 weight and writes the row, the source itself first under include_self, with
//                 the (-1, 0.0) padding.  Nothing n x n reaches HBM.
// The staging and selection code is a copy of gw_knn.hip's, not shared with it: that file keeps
// its kernels and results untouched, and the two orders (descending score there, ascending
// distance here) stay readable where they are used.
// No float atomics and no MFMA: every sum has the law's order and the order of a row is total,
// so two runs give the same bits and the host evaluation gives them too.
#include <hip/hip_runtime.h>

#include "gw_nng_internal.h"
#include "gw_trainer_device.h"

// Device state of a gw_nng handle (device >= 0); the buffer is freed with it.
struct gw_nng_dev {
  gw_dev_buf<unsigned long long> bad;  // first source outside [0, n)
};

namespace {

constexpr int kTQ = 32;    // source rows per workgroup
constexpr int kTC = 128;   // candidate rows per tile
constexpr int kKC = 32;    // columns per LDS chunk
constexpr int kThreads = 256;
constexpr int kUnionBytes = kTQ * kTC * (int)sizeof(double);  // the fp32 tiles, then the distances of the tile
constexpr int kEntriesPerLane = 3;                            // of a row's buffer in a compaction
static_assert(kThreads == (kTQ / 4) * (kTC / 4), "one 4 x 4 register tile per lane");
static_assert(kKC * (kTQ + kTC) * (int)sizeof(float) <= kUnionBytes, "the fp32 tiles fit under the distance tile");
static_assert(kTQ * (kKC / 4) == kThreads && (kTC * (kKC / 4)) % kThreads == 0, "the staging maps below");
static_assert(GW_NNG_MAX_TOPK + 64 <= kEntriesPerLane * 64, "a full buffer is ranked in kEntriesPerLane registers");

__host__ __device__ constexpr int buf_len(int topk) { return topk + 64; }  // a wave appends at most 64 at a time

struct NngArgs {
  const float* x;
  int64_t pitch;
  int vec16;  // rows are 16 B aligned: whole groups of 4 columns are read as float4
  int n, dim, topk, include_self;
  double heat_t;
  const int32_t* sources;  // NULL: 0 .. n-1
  int64_t nsrc;
  int32_t* out_ids;
  double* out_weights;
  double* out_d2;  // may be NULL
};

size_t main_lds(int topk) {
  const size_t B = (size_t)buf_len(topk);
  return (size_t)kUnionBytes + kTQ * B * (sizeof(double) + sizeof(int32_t)) + kTQ * (sizeof(double) + 4 * sizeof(int32_t));
}

__global__ void k_nng_check(const int32_t* __restrict__ sources, int64_t nsrc, int n, unsigned long long* bad) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nsrc) return;
  const int32_t v = sources[r];
  if (v < 0 || v >= n) atomicMin(bad, (unsigned long long)r);
}

// columns [k, k + 4) of row `row` (row < 0: no such row), zeros past dim; nothing past dim is read
__device__ __forceinline__ float4 load_cols(const NngArgs& A, int64_t row, int k) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row < 0 || k >= A.dim) return v;
  const float* src = A.x + row * A.pitch + k;
  if (A.vec16 && k + 3 < A.dim) return *reinterpret_cast<const float4*>(src);
  v.x = src[0];
  if (k + 1 < A.dim) v.y = src[1];
  if (k + 2 < A.dim) v.z = src[2];
  if (k + 3 < A.dim) v.w = src[3];
  return v;
}

// tile[kl][col ^ (group of kl << 2)] = the four columns kq * 4 .. + 3 of row `col`: the 32 lanes of a
// store instruction (4 rows x 8 column groups) fall into 32 banks
__device__ __forceinline__ void store_cols(float* tile, int width, int col, int kq, const float4 v) {
  const int c = col ^ (kq << 2);
  tile[(kq * 4 + 0) * width + c] = v.x;
  tile[(kq * 4 + 1) * width + c] = v.y;
  tile[(kq * 4 + 2) * width + c] = v.z;
  tile[(kq * 4 + 3) * width + c] = v.w;
}

// The lanes of a wave hand LDS values to one another: keep the compiler from moving memory operations across.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct RowState {
  double* buf_d;  // [kTQ][B] squared distances
  double* bd;     // [kTQ] bound distance
  int32_t* buf_i;  // [kTQ][B]
  int32_t* cnt;   // [kTQ]
  int32_t* hasb;  // [kTQ] the bound is set
  int32_t* bi;    // [kTQ] bound id
  int32_t* src;   // [kTQ] source vertex, -1 past nsrc
  int B;
};

// One wave: the buffer of row rr down to its best min(cnt, keep) entries, sorted; the bound is set once `keep` stand.
__device__ __forceinline__ void compact_row(const RowState& R, int rr, int keep, int lane) {
  const int cnt = R.cnt[rr];
  double* bd = R.buf_d + (size_t)rr * R.B;
  int32_t* bi = R.buf_i + (size_t)rr * R.B;
  double ed[kEntriesPerLane];
  int32_t ei[kEntriesPerLane];
  int rank[kEntriesPerLane];
#pragma unroll
  for (int t = 0; t < kEntriesPerLane; ++t) {
    const int e = lane + 64 * t;
    ed[t] = e < cnt ? bd[e] : 0.0;
    ei[t] = e < cnt ? bi[e] : 0;
    rank[t] = 0;
  }
  for (int f = 0; f < cnt; ++f) {
    const double df = bd[f];
    const int32_t jf = bi[f];
#pragma unroll
    for (int t = 0; t < kEntriesPerLane; ++t) rank[t] += gw_nng_before(df, jf, ed[t], ei[t]);
  }
  wave_sync();  // every lane has read the buffer before any lane rewrites it
#pragma unroll
  for (int t = 0; t < kEntriesPerLane; ++t) {
    if (lane + 64 * t < cnt && rank[t] < keep) {
      bd[rank[t]] = ed[t];
      bi[rank[t]] = ei[t];
      if (rank[t] == keep - 1) {
        R.bd[rr] = ed[t];
        R.bi[rr] = ei[t];
        R.hasb[rr] = 1;
      }
    }
  }
  if (lane == 0) R.cnt[rr] = cnt < keep ? cnt : keep;
  wave_sync();
}

__global__ __launch_bounds__(kThreads) void k_nng_main(const NngArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* qs = reinterpret_cast<float*>(smem);  // [kKC][kTQ]
  float* cs = qs + kKC * kTQ;                  // [kKC][kTC]
  double* S = reinterpret_cast<double*>(smem);  // [kTQ][kTC], over the tiles once they are consumed
  RowState R;
  R.B = buf_len(A.topk);
  R.buf_d = reinterpret_cast<double*>(smem + kUnionBytes);
  R.bd = R.buf_d + (size_t)kTQ * R.B;
  R.buf_i = reinterpret_cast<int32_t*>(R.bd + kTQ);
  R.cnt = R.buf_i + (size_t)kTQ * R.B;
  R.hasb = R.cnt + kTQ;
  R.bi = R.hasb + kTQ;
  R.src = R.bi + kTQ;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tq = tid >> 5, tc = tid & 31;  // rows tq * 4 .. + 3, candidates tc * 4 .. + 3 of the tile
  const int64_t r0 = (int64_t)blockIdx.x * kTQ;
  const int n = A.n, dim = A.dim, topk = A.topk, self = A.include_self;
  const int keep = topk - self;  // others listed per row; 0 (topk = 1 with the source itself): no candidate is read
  if (tid < kTQ) {
    const int64_t r = r0 + tid;
    const int32_t v = r < A.nsrc ? (A.sources ? A.sources[r] : (int32_t)r) : -1;
    R.src[tid] = v;
    R.cnt[tid] = 0;
    R.hasb[tid] = 0;
    R.bd[tid] = 0.0;
    R.bi[tid] = 0;
  }
  const int64_t nc = keep > 0 ? n : 0;
  for (int64_t c0 = 0; c0 < nc; c0 += kTC) {
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[a][u] = 0.0;
    for (int k0 = 0; k0 < dim; k0 += kKC) {
      __syncthreads();  // the union is free: the last chunk's reads, or the last tile's selection, are done
      {
        const int rr = tid >> 3, kq = tid & 7;
        store_cols(qs, kTQ, rr, kq, load_cols(A, R.src[rr], k0 + kq * 4));
      }
#pragma unroll
      for (int it = 0; it < kTC * (kKC / 4) / kThreads; ++it) {
        const int idx = it * kThreads + tid, rr = idx >> 3, kq = idx & 7;
        const int64_t j = c0 + rr;
        store_cols(cs, kTC, rr, kq, load_cols(A, j < n ? j : -1, k0 + kq * 4));
      }
      __syncthreads();
      // columns past dim hold zeros on both sides (e = 0 leaves acc as it is): whole groups of 4 run
      const int kn = dim - k0 < kKC ? dim - k0 : kKC;
      for (int kg = 0; kg * 4 < kn; ++kg) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int kl = kg * 4 + kk;
          const float4 qv = *reinterpret_cast<const float4*>(qs + kl * kTQ + ((tq ^ kg) << 2));
          const float4 cv = *reinterpret_cast<const float4*>(cs + kl * kTC + ((tc ^ kg) << 2));
          const double q[4] = {(double)qv.x, (double)qv.y, (double)qv.z, (double)qv.w};
          const double c[4] = {(double)cv.x, (double)cv.y, (double)cv.z, (double)cv.w};
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[a][u] = gw_nng_step(q[a], c[u], acc[a][u]);
        }
      }
    }
    __syncthreads();  // the tiles are consumed: the distances go over them
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int u = 0; u < 4; ++u) S[(tq * 4 + a) * kTC + tc * 4 + u] = acc[a][u];
    __syncthreads();
    // selection: row rr belongs to wave rr % 4 from the first tile to the output
    for (int rr = wave; rr < kTQ; rr += kThreads / 64) {
      const int32_t v = R.src[rr];
      if (v < 0) continue;  // wave-uniform
#pragma unroll
      for (int half = 0; half < kTC / 64; ++half) {
        const int c = lane + 64 * half;
        const int64_t j64 = c0 + c;
        const bool in = j64 < n;
        const int32_t j = (int32_t)j64;
        const double d = S[rr * kTC + c];
        bool ok = in && j != v && gw_nng_listed(d);
        if (ok && R.hasb[rr]) ok = gw_nng_before(d, j, R.bd[rr], R.bi[rr]);
        unsigned long long mask = __ballot(ok);
        if (mask == 0) continue;  // wave-uniform
        if (R.cnt[rr] + __popcll(mask) > R.B) {
          compact_row(R, rr, keep, lane);  // at least `keep` stood: the bound is set now
          ok = ok && gw_nng_before(d, j, R.bd[rr], R.bi[rr]);
          mask = __ballot(ok);
        }
        const int cnt = R.cnt[rr];
        wave_sync();
        if (ok) {
          const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
          R.buf_d[(size_t)rr * R.B + pos] = d;
          R.buf_i[(size_t)rr * R.B + pos] = j;
        }
        if (lane == 0) R.cnt[rr] = cnt + __popcll(mask);
        wave_sync();
      }
    }
  }
  __syncthreads();  // keep = 0 or n = 0 tiles: the row state written above is visible to its wave
  for (int rr = wave; rr < kTQ; rr += kThreads / 64) {
    const int32_t v = R.src[rr];
    if (v < 0) continue;
    compact_row(R, rr, keep, lane);
    const int cnt = R.cnt[rr];
    const int64_t o = (r0 + rr) * (int64_t)topk;
    for (int t = lane; t < topk; t += 64) {
      int32_t id = -1;
      double d2 = 0.0, w = 0.0;
      if (self && t == 0) {
        id = v;
        w = 1.0;
      } else if (t - self < cnt) {
        id = R.buf_i[(size_t)rr * R.B + t - self];
        d2 = R.buf_d[(size_t)rr * R.B + t - self];
        w = gw_nng_weight(d2, A.heat_t);
      }
      A.out_ids[o + t] = id;
      A.out_weights[o + t] = w;
      if (A.out_d2) A.out_d2[o + t] = d2;
    }
  }
}

}  // namespace

int gw_nng_dev_alloc(gw_nng* m) {
  const int rc = gw_trainer_open_device(m);
  if (rc != GW_OK) return rc;
  GW_DEV_GUARD(m);
  if (m->dev->bad.alloc(1) != hipSuccess) return gw_nng_fail(m, GW_ERR_NOMEM, "device allocation failed");
  GW_DEV_TRY(m, hipFuncSetAttribute((const void*)k_nng_main, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)main_lds(GW_NNG_MAX_TOPK)));
  return GW_OK;
}

void gw_nng_dev_free(gw_nng* m) {
  gw_device_guard dg(m->device);
  delete m->dev;
  m->dev = nullptr;
}

int gw_nng_dev_query(gw_nng* m, const int32_t* sources, int64_t nsrc, int32_t* out_ids, double* out_weights,
                     double* out_d2, void* stream) {
  GW_DEV_GUARD(m);
  gw_nng_dev& dv = *m->dev;
  hipStream_t st = (hipStream_t)stream;
  const int64_t blocks = (nsrc + kTQ - 1) / kTQ;
  if (blocks > 0x7FFFFFFF || (nsrc + 255) / 256 > 0x7FFFFFFF)
    return gw_nng_fail(m, GW_ERR_UNSUPPORTED, "too many sources for one launch");
  if (sources) {
    unsigned long long bad = ~0ull;
    GW_DEV_TRY(m, hipMemsetAsync(dv.bad.get(), 0xFF, sizeof bad, st));
    k_nng_check<<<(unsigned)((nsrc + 255) / 256), 256, 0, st>>>(sources, nsrc, (int)m->n, dv.bad.get());
    GW_DEV_TRY(m, hipGetLastError());
    GW_DEV_TRY(m, hipMemcpyAsync(&bad, dv.bad.get(), sizeof bad, hipMemcpyDeviceToHost, st));
    GW_DEV_TRY(m, hipStreamSynchronize(st));
    if (bad != ~0ull)
      return gw_nng_fail(m, GW_ERR_RANGE, "entry %llu: source outside [0, %lld)", bad, (long long)m->n);
  }
  NngArgs A = {};
  A.x = m->x;
  A.pitch = m->pitch;
  A.vec16 = ((uintptr_t)m->x % 16 == 0 && m->pitch % 4 == 0) ? 1 : 0;
  A.n = (int)m->n;
  A.dim = m->p.dim;
  A.topk = m->p.topk;
  A.include_self = m->p.include_self;
  A.heat_t = m->p.heat_t;
  A.sources = sources;
  A.nsrc = nsrc;
  A.out_ids = out_ids;
  A.out_weights = out_weights;
  A.out_d2 = out_d2;
  k_nng_main<<<(unsigned)blocks, kThreads, main_lds(A.topk), st>>>(A);
  GW_DEV_TRY(m, hipGetLastError());
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  return GW_OK;
}

extern "C" int gw_nng_kernel_attrs(gw_nng* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                                   int32_t* lds_bytes, int32_t* count) {
  if (!m) return gw_nng_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (m->device < 0) return gw_nng_fail(m, GW_ERR_STATE, "host evaluation launches no kernel");
  GW_DEV_GUARD(m);
  const gw_kernel_entry ks[] = {{"k_nng_check", (const void*)k_nng_check, 0},
                                {"k_nng_main", (const void*)k_nng_main, main_lds(m->p.topk)}};
  return gw_trainer_kernel_attrs(m, ks, cap, names, vgprs, scratch_bytes, lds_bytes, count);
}

extern "C" int gw_nng_tiles(const gw_nng* m, int32_t* tq, int32_t* tc, int32_t* kc, int32_t* buf) {
  if (!m) return gw_nng_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (m->device < 0) return gw_nng_fail(const_cast<gw_nng*>(m), GW_ERR_STATE, "host evaluation has no launch geometry");
  if (tq) *tq = kTQ;
  if (tc) *tc = kTC;
  if (kc) *kc = kKC;
  if (buf) *buf = buf_len(m->p.topk);
  return GW_OK;
}
