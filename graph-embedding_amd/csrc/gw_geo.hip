// Geodesic kernels (gfx950): the law of gw_geo_law.h.
//
//   k_geo_check   every source lies in [0, n): the first offending entry, by integer atomic min
//   k_geo_main    one workgroup per source (further sources by grid stride): near-far rounds over a bitmap.
//
// The schedule of k_geo_main.  dist[] holds bit patterns of upper bounds (+inf at the start, +0 at the source), flag[]
// one bit per vertex whose bound improved since it last relaxed its row, act[] the bits a round has taken.  A round:
//   scan    lane t reads the flag words t, t + lanes, ...; a flagged vertex with dist <= threshold is taken (its flag
//           cleared, its act bit set), the others give the workgroup's minimum flagged distance.  Nothing taken:
//           threshold = that minimum + delta and one more scan, which then takes at least the minimum's vertex.
//   relax   every taken vertex reads its CSR row: nd = dist[u] + l; where nd < dist[v], an unsigned 64-bit atomic min
//           on the bit patterns, and v is flagged where the minimum improved it.
// A source is finished when a scan finds no flag, or when a round improved nothing and left nothing flagged behind.
// A bitmap, not a worklist: nothing can overflow.  The work is the rows of the taken vertices; a vertex is taken again
// only after an improvement, and with a bucket of a few edge lengths that is a small multiple of once (the stats'
// relaxations / (sources * entries) reports it), not sweeps * entries.
//
// Why no ordering discipline is needed: gw_geo_law.h shows the fixed point is unique.  All an order of arrival decides
// is how many rounds are spent.  The same holds for reads: every read of dist[], flag[] and act[] is an atomic load
// (LDS mode: LDS has no cache; global mode: agent scope, which goes past the CU's L1 to the L2 the atomics work in).
// A stale value would be a larger bound: an extra atomic or an extra round, never a wrong result.  What is needed is
// that no improvement is lost: flags are set after the minimum, scanned only after the round's barrier, and a taken
// vertex whose bound improves during its own relax phase is flagged again by the improver.
//
// Where the state lies: while 8 n bytes of distances and the two bitmaps fit kLdsBudget (n <= lds_rows of
// gw_geo_tiles), in LDS, and the row leaves in whole coalesced segments; above it, the distances are the source's own
// output row (8 n bytes: L2-resident for the n of landmark Isomap) and the bitmaps lie in per-workgroup device scratch.
//
// The bound on every loop (this runs on shared machines: nothing here can spin).  The round loop is
// for (round = 0; round < cap + n; ++round).  cap = 2 n + 64: with delta -> 0 the schedule is Dijkstra's, one vertex
// settled per round, n rounds; a bucket that holds a chain of short edges spends one more round per hop inside it, and
// over all buckets those hops are again at most n; 64 is slack for tiny graphs.  At round == cap the threshold becomes
// +inf: plain Bellman-Ford over the flagged set, which from any state of upper bounds is final after n - 1 rounds and
// sees that in the n-th.  Such a source is counted in the stats' fallbacks; one still unfinished when the loop ends
// sets the status word (GW_ERR_INTERNAL on the host; by the argument above it cannot happen).  Every inner loop runs
// over a word's bits, a row's entries or a strided range of n.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gw_geo_internal.h"
#include "gw_trainer_device.h"

namespace {

typedef unsigned long long u64;

constexpr int kLanes = 256;         // threads of a workgroup; a lane scans one 64-vertex word per trip
constexpr int kGridMax = 1024;      // workgroups of a launch: 256 CUs x 4
constexpr int kLdsBudget = 65472;   // dynamic LDS of the LDS mode: 64 KiB less the 64 B of s_hdr, two workgroups per CU
constexpr u64 kInf = GW_GEO_INF_BITS;

// ctl words
enum { kBad = 0, kStatus = 1, kRounds = 2, kRelaxed = 3, kFallbacks = 4, kCtlWords = 8 };

int64_t words_of(int64_t n) { return (n + 63) / 64; }
int64_t lds_bytes_of(int64_t n) { return 8 * n + 16 * words_of(n); }
int64_t lds_rows() {
  int64_t n = kLdsBudget / 8;
  while (n > 0 && lds_bytes_of(n) > kLdsBudget) --n;
  return n;
}

struct GeoArgs {
  const int64_t* off;
  const int32_t* col;
  const double* len;
  const int32_t* sources;  // NULL: 0 .. nsrc-1
  int64_t nsrc;
  int n;
  int64_t words;   // of a bitmap
  u64* out;        // [nsrc][pitch], bit patterns of doubles
  int64_t pitch;
  u64* scratch;    // global mode: [grid][2][words]
  double delta;
  int64_t cap;
  u64* ctl;
};

template <bool LDS>
__device__ __forceinline__ u64 ld(const u64* p) {
  if constexpr (LDS) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ void st(u64* p, u64 v) {
  if constexpr (LDS) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ u64 amin(u64* p, u64 v) {
  if constexpr (LDS) return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ void aor(u64* p, u64 v) {
  if constexpr (LDS) __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void k_geo_check(const int32_t* __restrict__ sources, int64_t nsrc, int n, u64* ctl) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nsrc; r += (int64_t)gridDim.x * blockDim.x)
    if (sources[r] < 0 || sources[r] >= n) atomicMin(ctl + kBad, (u64)r);
}

template <bool LDS>
__global__ __launch_bounds__(kLanes) void k_geo_main(const GeoArgs A) {
  extern __shared__ u64 s_dyn[];  // LDS mode: dist[n], flag[words], act[words]
  __shared__ u64 s_hdr[8];        // four slots of (taken, minimum flagged distance), used in turn, reset a pass ahead
  const int tid = threadIdx.x, n = A.n;
  const int64_t W = A.words;
  u64* const flag = LDS ? s_dyn + n : A.scratch + (int64_t)blockIdx.x * 2 * W;
  u64* const act = flag + W;
  u64 relaxed = 0;
  for (int64_t r = blockIdx.x; r < A.nsrc; r += gridDim.x) {
    const int32_t s = A.sources ? A.sources[r] : (int32_t)r;
    u64* const dist = LDS ? s_dyn : A.out + r * A.pitch;
    for (int64_t v = tid; v < n; v += kLanes) st<LDS>(dist + v, kInf);
    for (int64_t w = tid; w < W; w += kLanes) st<LDS>(flag + w, 0);
    if (tid < 8) s_hdr[tid] = (tid & 1) ? kInf : 0;
    __syncthreads();
    if (tid == 0) {
      st<LDS>(dist + s, 0);
      st<LDS>(flag + (s >> 6), 1ull << (s & 63));
    }
    __syncthreads();
    u64 thr = 0;
    bool done = false, fell = false;
    int64_t rounds = 0;
    unsigned k = 0;
    const int64_t bound = A.cap + n;
    for (int64_t round = 0; round < bound; ++round) {
      if (round == A.cap) {  // the fallback: Bellman-Ford over whatever is flagged
        thr = kInf;
        fell = true;
      }
      ++rounds;
      bool taken = false;
      u64 minfar = kInf;
      for (int pass = 0; pass < 2; ++pass) {
        u64* const h = s_hdr + 2 * (k & 3);
        ++k;
        if (tid == 0) {  // the next pass's slot: last read two barriers ago
          s_hdr[2 * (k & 3)] = 0;
          s_hdr[2 * (k & 3) + 1] = kInf;
        }
        u64 any = 0, mn = kInf;
        for (int64_t w = tid; w < W; w += kLanes) {
          const u64 f = ld<LDS>(flag + w);
          u64 take = 0;
          for (u64 g = f; g; g &= g - 1) {
            const int b = __builtin_ctzll(g);
            const u64 d = ld<LDS>(dist + (w << 6) + b);
            if (d <= thr) take |= 1ull << b;
            else if (d < mn) mn = d;
          }
          if (take) st<LDS>(flag + w, f & ~take);  // this lane alone writes the word during a scan
          st<LDS>(act + w, take);
          any |= take;
        }
        if (any) __hip_atomic_fetch_or(h, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (mn != kInf) __hip_atomic_fetch_min(h + 1, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        taken = __hip_atomic_load(h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0;
        minfar = __hip_atomic_load(h + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (taken || minfar == kInf) break;
        thr = gw_geo_bits(gw_geo_double(minfar) + A.delta);  // >= minfar: the next scan takes its vertex
      }
      if (!taken && minfar == kInf) {  // no flag anywhere
        done = true;
        break;
      }
      int improved = 0;
      if (taken)
        for (int64_t w = tid; w < W; w += kLanes)
          for (u64 a = ld<LDS>(act + w); a; a &= a - 1) {
            const int64_t u = (w << 6) + __builtin_ctzll(a);
            const u64 du = ld<LDS>(dist + u);
            const int64_t e1 = A.off[u + 1];
            for (int64_t e = A.off[u]; e < e1; ++e) {
              const int32_t v = A.col[e];
              const u64 nd = gw_geo_relax(du, A.len[e]);
              ++relaxed;
              if (nd < ld<LDS>(dist + v) && nd < amin<LDS>(dist + v, nd)) {
                aor<LDS>(flag + (v >> 6), 1ull << (v & 63));
                improved = 1;
              }
            }
          }
      if (!__syncthreads_or(improved) && minfar == kInf) {  // nothing flagged behind, nothing flagged now
        done = true;
        break;
      }
    }
    if (LDS)
      for (int64_t v = tid; v < n; v += kLanes) A.out[r * A.pitch + v] = s_dyn[v];
    if (tid == 0) {
      atomicMax(A.ctl + kRounds, (u64)rounds);
      if (fell) atomicAdd(A.ctl + kFallbacks, 1ull);
      if (!done) atomicOr(A.ctl + kStatus, 1ull);
    }
    __syncthreads();  // the next source's initialisation writes what this one still reads
  }
  if (relaxed) atomicAdd(A.ctl + kRelaxed, relaxed);
}

}  // namespace

// Device state of a gw_geo handle (device >= 0); the buffers are freed with it.
struct gw_geo_dev {
  gw_dev_buf<int64_t> off;
  gw_dev_buf<int32_t> col;
  gw_dev_buf<double> len;
  gw_dev_buf<u64> ctl;
  gw_dev_buf<u64> scratch;  // global mode: the workgroups' bitmaps
};

int gw_geo_dev_alloc(gw_geo* m) {
  const int rc = gw_trainer_open_device(m);
  if (rc != GW_OK) return rc;
  GW_DEV_GUARD(m);
  GW_DEV_TRY(m, m->dev->ctl.alloc(kCtlWords));
  GW_DEV_TRY(m, hipFuncSetAttribute((const void*)k_geo_main<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    kLdsBudget));
  return GW_OK;
}

void gw_geo_dev_free(gw_geo* m) {
  if (!m->dev) return;
  gw_device_guard g(m->device);
  delete m->dev;
  m->dev = nullptr;
}

int gw_geo_dev_upload(gw_geo* m) {
  GW_DEV_GUARD(m);
  gw_geo_dev* d = m->dev;
  const int64_t nnz = (int64_t)m->col.size();
  GW_DEV_TRY(m, d->off.grow(m->n + 1));
  GW_DEV_TRY(m, d->col.grow(nnz));
  GW_DEV_TRY(m, d->len.grow(nnz));
  GW_DEV_TRY(m, hipMemcpy(d->off.get(), m->off.data(), sizeof(int64_t) * (size_t)(m->n + 1), hipMemcpyHostToDevice));
  if (nnz) {
    GW_DEV_TRY(m, hipMemcpy(d->col.get(), m->col.data(), sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice));
    GW_DEV_TRY(m, hipMemcpy(d->len.get(), m->len.data(), sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice));
  }
  return GW_OK;
}

int gw_geo_dev_query(gw_geo* m, const int32_t* sources, int64_t nsrc, double* out, int64_t pitch, void* stream) {
  GW_DEV_GUARD(m);
  gw_geo_dev* d = m->dev;
  hipStream_t st = (hipStream_t)stream;
  u64 ctl[kCtlWords];
  GW_DEV_TRY(m, hipMemsetAsync(d->ctl.get(), 0, sizeof ctl, st));
  GW_DEV_TRY(m, hipMemsetAsync(d->ctl.get() + kBad, 0xFF, sizeof(u64), st));
  if (sources) {
    const int grid = (int)std::min<int64_t>((nsrc + 255) / 256, kGridMax);
    hipLaunchKernelGGL(k_geo_check, dim3(grid), dim3(256), 0, st, sources, nsrc, (int)m->n, d->ctl.get());
    GW_DEV_TRY(m, hipGetLastError());
    GW_DEV_TRY(m, hipMemcpyAsync(ctl, d->ctl.get(), sizeof ctl, hipMemcpyDeviceToHost, st));
    GW_DEV_TRY(m, hipStreamSynchronize(st));
    if (ctl[kBad] != ~0ull)
      return gw_geo_fail(m, GW_ERR_RANGE, "entry %lld: source outside [0, %lld)", (long long)ctl[kBad], (long long)m->n);
  }
  GeoArgs A;
  A.off = d->off.get();
  A.col = d->col.get();
  A.len = d->len.get();
  A.sources = sources;
  A.nsrc = nsrc;
  A.n = (int)m->n;
  A.words = words_of(m->n);
  A.out = reinterpret_cast<u64*>(out);
  A.pitch = pitch;
  A.scratch = nullptr;
  A.delta = m->delta;
  A.cap = m->cap >= 0 ? m->cap : 2 * m->n + 64;
  A.ctl = d->ctl.get();
  const int grid = (int)std::min<int64_t>(nsrc, kGridMax);
  if (m->n <= lds_rows()) {
    hipLaunchKernelGGL(k_geo_main<true>, dim3(grid), dim3(kLanes), (size_t)lds_bytes_of(m->n), st, A);
  } else {
    if (d->scratch.grow((int64_t)grid * 2 * A.words) != hipSuccess) {
      (void)hipGetLastError();
      return gw_geo_fail(m, GW_ERR_NOMEM, "no device memory for %d workgroups' bitmaps of %lld vertices", grid,
                         (long long)m->n);
    }
    A.scratch = d->scratch.get();
    hipLaunchKernelGGL(k_geo_main<false>, dim3(grid), dim3(kLanes), 0, st, A);
  }
  GW_DEV_TRY(m, hipGetLastError());
  GW_DEV_TRY(m, hipMemcpyAsync(ctl, d->ctl.get(), sizeof ctl, hipMemcpyDeviceToHost, st));
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  m->st.rounds_max = (int64_t)ctl[kRounds];
  m->st.relaxations = (int64_t)ctl[kRelaxed];
  m->st.fallbacks = (int32_t)ctl[kFallbacks];
  if (ctl[kStatus])
    return gw_geo_fail(m, GW_ERR_INTERNAL, "a source was still flagged after cap + n rounds (cap %lld)", (long long)A.cap);
  return GW_OK;
}

extern "C" int gw_geo_kernel_attrs(gw_geo* m, int cap, const char** names, int32_t* vgprs, int32_t* scratch_bytes,
                                   int32_t* lds_bytes, int32_t* count) {
  if (!m) return gw_geo_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (m->device < 0) return gw_geo_fail(m, GW_ERR_STATE, "host evaluation launches no kernel");
  GW_DEV_GUARD(m);
  const bool lds = m->n <= lds_rows();
  const gw_kernel_entry ks[] = {{"k_geo_check", (const void*)k_geo_check, 0},
                                {"k_geo_main_lds", (const void*)k_geo_main<true>, lds ? (size_t)lds_bytes_of(m->n) : 0},
                                {"k_geo_main_global", (const void*)k_geo_main<false>, 0}};
  return gw_trainer_kernel_attrs(m, ks, cap, names, vgprs, scratch_bytes, lds_bytes, count);
}

extern "C" int gw_geo_tiles(const gw_geo* m, int32_t* lanes, int32_t* rows, int32_t* sources_per_launch) {
  if (!m) return gw_geo_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (m->device < 0) return gw_geo_fail(const_cast<gw_geo*>(m), GW_ERR_STATE, "host evaluation launches no kernel");
  if (lanes) *lanes = kLanes;
  if (rows) *rows = (int32_t)lds_rows();
  if (sources_per_launch) *sources_per_launch = kGridMax;
  return GW_OK;
}
