// All-pairs top-k on the device (gfx950): the one plan behind k_knn_main (gw_knn.hip) and
// k_nng_main (gw_nng.hip), and the launch plumbing of their handles.  Included by those two files only.
//
//   pairs_topk_main<Law>  one workgroup per tile of kTQ source rows.  It streams tiles of kTC candidate
//                 rows through LDS in chunks of kKC columns (fp32, stored column-major with an
//                 XOR swizzle so that both the staging stores and the 16 B reads are free of
//                 bank conflicts), every lane keeps a 4 x 4 tile of fp64 accumulators and walks
//                 k strictly ascending, one Law::step per pair and column, so each raw value has
//                 the law's bits whatever the tiling.  Behind each finished candidate tile the raw
//                 values pass through LDS to the selection: a row belongs to one wave, which
//                 appends the candidates that beat the row's bound (its current keep-th entry under
//                 the law's total order) to the row's buffer in LDS by ballot and prefix count, and
//                 compacts a full buffer to its best `keep` by rank (entry e goes to slot
//                 #{f : f before e}), which leaves it sorted and tightens the bound.  After the last
//                 tile one more compaction sorts the row, and the law writes it.  Nothing n x n
//                 reaches HBM.
// A family is a law struct, passed to its kernel by value next to PairsArgs.  It gives what the two
// families differ in and nothing else; every hook is resolved at compile time and inlined:
//   kRowDoubles, row_double(v)       extra per-row doubles in LDS (0 or 1) and the value for source v
//   step(q, c, acc)                  one column of one pair
//   score(raw, xv, j, in, &s)        the finished chain to the value the row is ordered by (xv: the row's
//                                    double; in: j < n, nothing of j may be read otherwise); returns
//                                    whether (s, j) may be listed
//   before(sa, ia, sb, ib)           the law's total order
//   keep(topk)                       entries selected per row; 0: no candidate tile is read
//   write(o, t, v, cnt, s, ids)      entry t of the row of source v to the outputs at o + t, from the
//                                    row's cnt sorted entries
// No float atomics and no MFMA: every sum has the law's order and the order of a row is total,
// so two runs give the same bits and the host evaluation gives them too.
#pragma once
#include <hip/hip_runtime.h>

#include "gw_trainer_device.h"

namespace gw_pairs {

constexpr int kTQ = 32;    // source rows per workgroup
constexpr int kTC = 128;   // candidate rows per tile
constexpr int kKC = 32;    // columns per LDS chunk
constexpr int kThreads = 256;
constexpr int kUnionBytes = kTQ * kTC * (int)sizeof(double);  // the fp32 tiles, then the raw values of the tile
constexpr int kEntriesPerLane = 3;                            // of a row's buffer in a compaction
constexpr int kMaxTopk = kEntriesPerLane * 64 - 64;           // a full buffer is ranked in kEntriesPerLane registers
static_assert(kThreads == (kTQ / 4) * (kTC / 4), "one 4 x 4 register tile per lane");
static_assert(kKC * (kTQ + kTC) * (int)sizeof(float) <= kUnionBytes, "the fp32 tiles fit under the tile of raw values");
static_assert(kTQ * (kKC / 4) == kThreads && (kTC * (kKC / 4)) % kThreads == 0, "the staging maps below");

__host__ __device__ constexpr int buf_len(int topk) { return topk + 64; }  // a wave appends at most 64 at a time

// The matrix and the request; the rest of a kernel's arguments is its law.
struct PairsArgs {
  const float* x;
  int64_t pitch;
  int vec16;  // rows are 16 B aligned: whole groups of 4 columns are read as float4
  int n, dim, topk;
  const int32_t* sources;  // NULL: 0 .. n-1
  int64_t nsrc;
};

inline size_t main_lds(int topk, int row_doubles) {
  const size_t B = (size_t)buf_len(topk);
  return (size_t)kUnionBytes + kTQ * B * (sizeof(double) + sizeof(int32_t)) +
         kTQ * ((1 + row_doubles) * sizeof(double) + 4 * sizeof(int32_t));
}

// every source lies in [0, n): the first offending entry, by integer atomic min
__device__ __forceinline__ void check_sources(const int32_t* __restrict__ sources, int64_t nsrc, int n,
                                              unsigned long long* bad) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nsrc) return;
  const int32_t v = sources[r];
  if (v < 0 || v >= n) atomicMin(bad, (unsigned long long)r);
}

// columns [k, k + 4) of row `row` (row < 0: no such row), zeros past dim; nothing past dim is read
__device__ __forceinline__ float4 load_cols(const PairsArgs& A, int64_t row, int k) {
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

// The selection's LDS behind the union, in this order (xd is empty where the law has no row double).
struct RowState {
  double* buf_s;  // [kTQ][B] the values the row is ordered by
  double* bs;     // [kTQ] bound value
  double* xd;     // [kTQ][kRowDoubles] the law's row double
  int32_t* buf_i;  // [kTQ][B]
  int32_t* cnt;   // [kTQ]
  int32_t* hasb;  // [kTQ] the bound is set
  int32_t* bi;    // [kTQ] bound id
  int32_t* src;   // [kTQ] source vertex, -1 past nsrc
  int B;
};

// One wave: the buffer of row rr down to its best min(cnt, keep) entries, sorted; the bound is set once `keep` stand.
template <class Law>
__device__ __forceinline__ void compact_row(const RowState& R, int rr, int keep, int lane) {
  const int cnt = R.cnt[rr];
  double* bs = R.buf_s + (size_t)rr * R.B;
  int32_t* bi = R.buf_i + (size_t)rr * R.B;
  double es[kEntriesPerLane];
  int32_t ei[kEntriesPerLane];
  int rank[kEntriesPerLane];
#pragma unroll
  for (int t = 0; t < kEntriesPerLane; ++t) {
    const int e = lane + 64 * t;
    es[t] = e < cnt ? bs[e] : 0.0;
    ei[t] = e < cnt ? bi[e] : 0;
    rank[t] = 0;
  }
  for (int f = 0; f < cnt; ++f) {
    const double sf = bs[f];
    const int32_t jf = bi[f];
#pragma unroll
    for (int t = 0; t < kEntriesPerLane; ++t) rank[t] += Law::before(sf, jf, es[t], ei[t]);
  }
  wave_sync();  // every lane has read the buffer before any lane rewrites it
#pragma unroll
  for (int t = 0; t < kEntriesPerLane; ++t) {
    if (lane + 64 * t < cnt && rank[t] < keep) {
      bs[rank[t]] = es[t];
      bi[rank[t]] = ei[t];
      if (rank[t] == keep - 1) {
        R.bs[rr] = es[t];
        R.bi[rr] = ei[t];
        R.hasb[rr] = 1;
      }
    }
  }
  if (lane == 0) R.cnt[rr] = cnt < keep ? cnt : keep;
  wave_sync();
}

// The body of a family's main kernel: kThreads lanes, main_lds(topk, Law::kRowDoubles) bytes of dynamic LDS.
template <class Law>
__device__ __forceinline__ void pairs_topk_main(const PairsArgs& A, const Law& L) {
  static_assert(Law::kRowDoubles == 0 || Law::kRowDoubles == 1, "RowState::xd holds at most one double per row");
  static_assert(Law::kMaxTopk <= kMaxTopk, "a full buffer is ranked in kEntriesPerLane registers");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* qs = reinterpret_cast<float*>(smem);  // [kKC][kTQ]
  float* cs = qs + kKC * kTQ;                  // [kKC][kTC]
  double* S = reinterpret_cast<double*>(smem);  // [kTQ][kTC], over the tiles once they are consumed
  RowState R;
  R.B = buf_len(A.topk);
  R.buf_s = reinterpret_cast<double*>(smem + kUnionBytes);
  R.bs = R.buf_s + (size_t)kTQ * R.B;
  R.xd = R.bs + kTQ;
  R.buf_i = reinterpret_cast<int32_t*>(R.xd + kTQ * Law::kRowDoubles);
  R.cnt = R.buf_i + (size_t)kTQ * R.B;
  R.hasb = R.cnt + kTQ;
  R.bi = R.hasb + kTQ;
  R.src = R.bi + kTQ;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tq = tid >> 5, tc = tid & 31;  // rows tq * 4 .. + 3, candidates tc * 4 .. + 3 of the tile
  const int64_t r0 = (int64_t)blockIdx.x * kTQ;
  const int n = A.n, dim = A.dim, topk = A.topk;
  const int keep = L.keep(topk);
  if (tid < kTQ) {
    const int64_t r = r0 + tid;
    const int32_t v = r < A.nsrc ? (A.sources ? A.sources[r] : (int32_t)r) : -1;
    R.src[tid] = v;
    R.cnt[tid] = 0;
    R.hasb[tid] = 0;
    R.bs[tid] = 0.0;
    R.bi[tid] = 0;
    if (Law::kRowDoubles) R.xd[tid] = L.row_double(v);
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
      // columns past dim hold zeros on both sides, which leave acc as it is under either step: whole groups of 4 run
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
            for (int u = 0; u < 4; ++u) acc[a][u] = Law::step(q[a], c[u], acc[a][u]);
        }
      }
    }
    __syncthreads();  // the tiles are consumed: the raw values go over them
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int u = 0; u < 4; ++u) S[(tq * 4 + a) * kTC + tc * 4 + u] = acc[a][u];
    __syncthreads();
    // selection: row rr belongs to wave rr % 4 from the first tile to the output
    for (int rr = wave; rr < kTQ; rr += kThreads / 64) {
      const int32_t v = R.src[rr];
      if (v < 0) continue;  // wave-uniform
      const double xv = Law::kRowDoubles ? R.xd[rr] : 0.0;
#pragma unroll
      for (int half = 0; half < kTC / 64; ++half) {
        const int c = lane + 64 * half;
        const int64_t j64 = c0 + c;
        const bool in = j64 < n;
        const int32_t j = (int32_t)j64;
        double s;
        const bool listed = L.score(S[rr * kTC + c], xv, j, in, &s);
        bool ok = in && j != v && listed;
        if (ok && R.hasb[rr]) ok = Law::before(s, j, R.bs[rr], R.bi[rr]);
        unsigned long long mask = __ballot(ok);
        if (mask == 0) continue;  // wave-uniform
        if (R.cnt[rr] + __popcll(mask) > R.B) {
          compact_row<Law>(R, rr, keep, lane);  // at least `keep` stood: the bound is set now
          ok = ok && Law::before(s, j, R.bs[rr], R.bi[rr]);
          mask = __ballot(ok);
        }
        const int cnt = R.cnt[rr];
        wave_sync();
        if (ok) {
          const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
          R.buf_s[(size_t)rr * R.B + pos] = s;
          R.buf_i[(size_t)rr * R.B + pos] = j;
        }
        if (lane == 0) R.cnt[rr] = cnt + __popcll(mask);
        wave_sync();
      }
    }
  }
  __syncthreads();  // no tile ran (keep = 0): the row state written above is visible to its wave
  for (int rr = wave; rr < kTQ; rr += kThreads / 64) {
    const int32_t v = R.src[rr];
    if (v < 0) continue;
    compact_row<Law>(R, rr, keep, lane);
    const int cnt = R.cnt[rr];
    const int64_t o = (r0 + rr) * (int64_t)topk;
    for (int t = lane; t < topk; t += 64) L.write(o, t, v, cnt, R.buf_s + (size_t)rr * R.B, R.buf_i + (size_t)rr * R.B);
  }
}

// ---- the host side of a handle H: device, n, x, pitch, p.dim, p.topk, dev->bad, gw_fail_of(H*) --------------
using check_kernel = void (*)(const int32_t*, int64_t, int, unsigned long long*);

// *_dev_alloc: the device state, and the main kernel may ask for the LDS of Law::kMaxTopk
template <class H, class Law>
int dev_alloc(H* m, void (*kernel)(PairsArgs, Law)) {
  const int rc = gw_trainer_open_device(m);
  if (rc != GW_OK) return rc;
  GW_DEV_GUARD(m);
  if (m->dev->bad.alloc(1) != hipSuccess) return gw_fail_of(m)(m, GW_ERR_NOMEM, "device allocation failed");
  GW_DEV_TRY(m, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)main_lds(Law::kMaxTopk, Law::kRowDoubles)));
  return GW_OK;
}

template <class H>
void dev_free(H* m) {
  gw_device_guard dg(m->device);
  delete m->dev;
  m->dev = nullptr;
}

// What a query does before its launches, under the caller's GW_DEV_GUARD: the launch fits a grid, the
// sources (device memory) are range-checked before anything is written, *A describes the request.
template <class H>
int dev_begin_query(H* m, check_kernel check, const int32_t* sources, int64_t nsrc, hipStream_t st, PairsArgs* A) {
  if ((nsrc + kTQ - 1) / kTQ > 0x7FFFFFFF || (nsrc + 255) / 256 > 0x7FFFFFFF)
    return gw_fail_of(m)(m, GW_ERR_UNSUPPORTED, "too many sources for one launch");
  if (sources) {
    unsigned long long bad = ~0ull;
    GW_DEV_TRY(m, hipMemsetAsync(m->dev->bad.get(), 0xFF, sizeof bad, st));
    check<<<(unsigned)((nsrc + 255) / 256), 256, 0, st>>>(sources, nsrc, (int)m->n, m->dev->bad.get());
    GW_DEV_TRY(m, hipGetLastError());
    GW_DEV_TRY(m, hipMemcpyAsync(&bad, m->dev->bad.get(), sizeof bad, hipMemcpyDeviceToHost, st));
    GW_DEV_TRY(m, hipStreamSynchronize(st));
    if (bad != ~0ull)
      return gw_fail_of(m)(m, GW_ERR_RANGE, "entry %llu: source outside [0, %lld)", bad, (long long)m->n);
  }
  *A = {};
  A->x = m->x;
  A->pitch = m->pitch;
  A->vec16 = ((uintptr_t)m->x % 16 == 0 && m->pitch % 4 == 0) ? 1 : 0;
  A->n = (int)m->n;
  A->dim = m->p.dim;
  A->topk = m->p.topk;
  A->sources = sources;
  A->nsrc = nsrc;
  return GW_OK;
}

// the main kernel over every source tile, to the end
template <class H, class Law>
int dev_run_main(H* m, void (*kernel)(PairsArgs, Law), const PairsArgs& A, const Law& L, hipStream_t st) {
  kernel<<<(unsigned)((A.nsrc + kTQ - 1) / kTQ), kThreads, main_lds(A.topk, Law::kRowDoubles), st>>>(A, L);
  GW_DEV_TRY(m, hipGetLastError());
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  return GW_OK;
}

// *_tiles
template <class H>
int tiles(const H* m, int32_t* tq, int32_t* tc, int32_t* kc, int32_t* buf) {
  if (!m) return gw_fail_of(m)(nullptr, GW_ERR_INVALID, "NULL handle");
  if (m->device < 0) return gw_fail_of(m)(const_cast<H*>(m), GW_ERR_STATE, "host evaluation has no launch geometry");
  if (tq) *tq = kTQ;
  if (tc) *tc = kTC;
  if (kc) *kc = kKC;
  if (buf) *buf = buf_len(m->p.topk);
  return GW_OK;
}

}  // namespace gw_pairs
