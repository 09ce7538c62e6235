// SGNS trainer kernels (gfx950): the training law of gw_sgns_law.h, one wave
// per walk.
//
// Shape.  A wave owns one walk at a time and runs its pairs in the law's
// order; wave c of `concurrency` takes walks c, c + concurrency, ... of the
// epoch (one launch per epoch, so epochs are ordered), Hogwild between waves.
// With concurrency = 1 the launch IS the sequential law.  A row (pitch =
// 4*ceil(dim/4) floats) is dealt to the 64 lanes in 16 B chunks, NCH chunks per
// lane (dim <= 256: 1, ... <= 1024: 4), through a per-row buffer resource:
// lanes past the row read 0 and their stores are dropped by the bounds check,
// so no lane ever touches another row.
//
// Visibility.  Every load and store of a syn0 / syn1neg row is a 16 B
// buffer access with sc1 (agent scope): loads bypass the CU's L1 and stores
// write through the XCD's L2, so a wave on any XCD trains against what the
// last completed store left, never against a private stale copy (DESIGN).
//
// Prefetch.  The targets of a pair do not depend on data, so the next
// target's row is loaded before the current one is updated - unless it is
// the same row, in which case the updated registers carry over.
#include <hip/hip_runtime.h>

#include "gw_sgns_internal.h"
#include "gw_sgns_law.h"
#include "gw_trainer_device.h"

namespace {

constexpr int kWaves = 4;            // independent waves per workgroup (no barriers)
constexpr int kMaxWalkLen = 2048;    // kept sequence in LDS: 8 B * walk_len * kWaves <= 64 KB
constexpr int kSc1 = 16;             // buffer aux bit: sc1
constexpr int kRsrcFlags = 0x00020000;  // raw 32-bit dword buffer (gfx9)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct SgnsArgs {
  const int32_t* walks;
  int64_t nwalks;
  int walk_len;
  int64_t n;
  int pitch, window, K;
  int epoch, epochs, conc;
  double alpha0, min_alpha;
  uint64_t seed;
  const int32_t* J;
  const uint32_t* thr;
  const uint32_t* keep;
  const float* expt;
  float* syn0;
  float* syn1;
  unsigned long long* stats;  // [5] + error flag
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(float* base, int32_t id, int pitch) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)(base + (size_t)id * (size_t)pitch), 0, pitch * 4, kRsrcFlags);
}

template <int NCH>
struct Row {
  float v[NCH * 4];
};

template <int NCH>
__device__ __forceinline__ Row<NCH> row_load(__amdgpu_buffer_rsrc_t r, int lane) {
  Row<NCH> x;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(r, (c * GW_SGNS_LANES + lane) * 16, 0, kSc1);
    x.v[4 * c] = __uint_as_float(q.x);
    x.v[4 * c + 1] = __uint_as_float(q.y);
    x.v[4 * c + 2] = __uint_as_float(q.z);
    x.v[4 * c + 3] = __uint_as_float(q.w);
  }
  return x;
}

template <int NCH>
__device__ __forceinline__ void row_store(__amdgpu_buffer_rsrc_t r, int lane, const Row<NCH>& x) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    u32x4 q;
    q.x = __float_as_uint(x.v[4 * c]);
    q.y = __float_as_uint(x.v[4 * c + 1]);
    q.z = __float_as_uint(x.v[4 * c + 2]);
    q.w = __float_as_uint(x.v[4 * c + 3]);
    __builtin_amdgcn_raw_buffer_store_b128(q, r, (c * GW_SGNS_LANES + lane) * 16, 0, kSc1);
  }
}

template <int NCH>
__global__ __launch_bounds__(kWaves* GW_SGNS_LANES) void k_sgns_train(const SgnsArgs A) {
  extern __shared__ int32_t lds[];
  const int lane = threadIdx.x & (GW_SGNS_LANES - 1);
  const int wv = threadIdx.x / GW_SGNS_LANES;
  const int c = blockIdx.x * kWaves + wv;
  if (c >= A.conc) return;
  const int L = A.walk_len;
  int32_t* s = lds + wv * 2 * L;  // kept ids
  int32_t* pb = s + L;            // their walk position << 11 | window draw b
  const uint32_t e = (uint32_t)A.epoch;
  unsigned long long st0 = 0, st1 = 0, st2 = 0, st3 = 0, st4 = 0;
  for (int64_t w = c; w < A.nwalks; w += A.conc) {
    const float alpha = gw_sgns_alpha(A.alpha0, A.min_alpha, A.epoch, w, A.epochs, A.nwalks);
    // ---- kept sequence of the walk (subsampling), 64 positions at a time
    int cnt = 0;
    for (int base = 0; base < L; base += GW_SGNS_LANES) {
      const int i = base + lane;
      const int32_t v = i < L ? A.walks[w * (int64_t)L + i] : -1;
      const bool bad = v < -1 || (int64_t)v >= A.n;
      const unsigned long long endm = __ballot(v == -1 || bad);
      const int first_end = endm ? __ffsll((long long)endm) - 1 : GW_SGNS_LANES;
      if (bad && lane == first_end) atomicExch(&A.stats[5], 1ull);  // id outside [0, n): the call fails
      bool keep = false;
      uint32_t b = 0;
      if (lane < first_end) {
        const gw_u4 u = gw_sgns_tok_draw(A.seed, e, (uint64_t)w, (uint32_t)i);
        keep = gw_sgns_keep(u.x, A.keep[v]);
        b = u.y % (uint32_t)A.window;
      }
      const unsigned long long km = __ballot(keep);
      if (keep) {
        const int idx = cnt + __popcll(km & ((1ull << lane) - 1ull));
        s[idx] = v;
        pb[idx] = (int32_t)(((uint32_t)i << 11) | b);
      }
      cnt += __popcll(km);
      if (endm) break;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    st0 += (unsigned long long)cnt;
    // ---- pairs in the law's order
    for (int i = 0; i < cnt; ++i) {
      const int32_t centre = __builtin_amdgcn_readfirstlane(s[i]);
      const uint32_t pbi = (uint32_t)__builtin_amdgcn_readfirstlane(pb[i]);
      const int b = (int)(pbi & 2047u);
      const uint32_t pos = pbi >> 11;
      const int jlo = max(i - A.window + b, 0), jhi = min(i + A.window - b, cnt - 1);
      for (int j = jlo; j <= jhi; ++j) {
        if (j == i) continue;
        const int32_t sj = __builtin_amdgcn_readfirstlane(s[j]);
        const uint32_t slot = (uint32_t)(j - (i - A.window));
        const __amdgpu_buffer_rsrc_t r0 = row_rsrc(A.syn0, sj, A.pitch);
        Row<NCH> l1 = row_load<NCH>(r0, lane);
        Row<NCH> neu;
#pragma unroll
        for (int d = 0; d < NCH * 4; ++d) neu.v[d] = 0.0f;
        ++st1;
        st2 += (unsigned long long)A.K;
        int k = 0;           // target index: 0 = the centre word, 1..K = negatives
        int32_t t = centre;  // its row
        int32_t negv = 0;    // lane l: negative (chunk * 64 + l) of this pair
        Row<NCH> cur = row_load<NCH>(row_rsrc(A.syn1, t, A.pitch), lane);
        for (;;) {
          // the next target that is trained (negatives equal to the centre are skipped)
          int kn = k + 1;
          int32_t tn = -1;
          while (kn <= A.K) {
            const int q = kn - 1;
            if ((q & (GW_SGNS_LANES - 1)) == 0) {
              negv = q + lane < A.K ? gw_sgns_neg_draw(A.seed, e, (uint64_t)w, pos, slot, (uint32_t)(q + lane),
                                                       (uint32_t)A.n, A.J, A.thr)
                                    : -1;
            }
            tn = __builtin_amdgcn_readlane(negv, q & (GW_SGNS_LANES - 1));
            if (tn != centre) break;
            ++st3;
            ++kn;
          }
          const bool has_next = kn <= A.K;
          const bool same = has_next && tn == t;
          Row<NCH> nxt;
          if (has_next && !same) nxt = row_load<NCH>(row_rsrc(A.syn1, tn, A.pitch), lane);
          // f = dot(l1, cur): lane partial over its chunks, then the butterfly
          float p = 0.0f;
#pragma unroll
          for (int d = 0; d < NCH * 4; ++d) p = gw_sgns_fma2(p, l1.v[d], cur.v[d]);
#pragma unroll
          for (int o = GW_SGNS_LANES / 2; o >= 1; o >>= 1) p = p + __shfl_xor(p, o, GW_SGNS_LANES);
          const float f = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p)));
          float g;
          if (gw_sgns_grad(f, k == 0 ? 1.0f : 0.0f, alpha, A.expt, &g)) {
#pragma unroll
            for (int d = 0; d < NCH * 4; ++d) {
              neu.v[d] = gw_sgns_fma2(neu.v[d], g, cur.v[d]);
              cur.v[d] = gw_sgns_fma2(cur.v[d], g, l1.v[d]);
            }
            row_store<NCH>(row_rsrc(A.syn1, t, A.pitch), lane, cur);
          } else {
            ++st4;
          }
          if (!has_next) break;
          if (!same) cur = nxt;
          k = kn;
          t = tn;
        }
#pragma unroll
        for (int d = 0; d < NCH * 4; ++d) l1.v[d] = l1.v[d] + neu.v[d];
        row_store<NCH>(r0, lane, l1);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0) {
    atomicAdd(&A.stats[0], st0);
    atomicAdd(&A.stats[1], st1);
    atomicAdd(&A.stats[2], st2);
    atomicAdd(&A.stats[3], st3);
    atomicAdd(&A.stats[4], st4);
  }
}

// occurrences of every vertex; one thread per walk (a walk ends at its first -1)
__global__ void k_sgns_count(const int32_t* __restrict__ walks, int64_t nwalks, int walk_len, int64_t n,
                             unsigned long long* __restrict__ counts, unsigned long long* __restrict__ flag) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nwalks) return;
  const int32_t* row = walks + w * (int64_t)walk_len;
  for (int i = 0; i < walk_len; ++i) {
    const int32_t v = row[i];
    if (v == -1) break;
    if (v < 0 || (int64_t)v >= n) {
      atomicMax(flag, (unsigned long long)(w + 1));
      break;
    }
    atomicAdd(&counts[v], 1ull);
  }
}

__global__ void k_sgns_init(float* __restrict__ syn0, int64_t n, int pitch, int dim, uint64_t seed) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * pitch) return;
  const int64_t v = i / pitch;
  const int d = (int)(i - v * pitch);
  syn0[i] = d < dim ? gw_sgns_init(seed, (uint32_t)v, (uint32_t)d, dim) : 0.0f;
}

const void* train_kernel(int pitch) {
  const int nch = (pitch / 4 + GW_SGNS_LANES - 1) / GW_SGNS_LANES;
  switch (nch) {
    case 1: return (const void*)k_sgns_train<1>;
    case 2: return (const void*)k_sgns_train<2>;
    case 3: return (const void*)k_sgns_train<3>;
    default: return (const void*)k_sgns_train<4>;
  }
}

}  // namespace

// Device state of a gw_sgns handle (device >= 0); the buffers are freed with it.
struct gw_sgns_dev {
  gw_dev_buf<unsigned long long> counts;
  gw_dev_buf<int32_t> J;
  gw_dev_buf<uint32_t> thr, keep;
  gw_dev_buf<float> expt, syn0, syn1;
  gw_dev_buf<long long> stats;  // 5 stats + 1 error flag (8 allocated)
  int cus = 0;
};

int gw_sgns_dev_alloc(gw_sgns* m) {
  const int rc = gw_trainer_open_device(m);
  if (rc != GW_OK) return rc;
  GW_DEV_GUARD(m);
  gw_sgns_dev& dv = *m->dev;
  hipDeviceProp_t prop;
  GW_DEV_TRY(m, hipGetDeviceProperties(&prop, m->device));
  dv.cus = prop.multiProcessorCount;
  const int64_t n = m->n, rows = n * m->pitch;
  hipError_t e = dv.counts.alloc(n);
  if (e == hipSuccess) e = dv.J.alloc(n);
  if (e == hipSuccess) e = dv.thr.alloc(n);
  if (e == hipSuccess) e = dv.keep.alloc(n);
  if (e == hipSuccess) e = dv.expt.alloc(GW_SGNS_EXP_SIZE);
  if (e == hipSuccess) e = dv.syn0.alloc(rows);
  if (e == hipSuccess) e = dv.syn1.alloc(rows);
  if (e == hipSuccess) e = dv.stats.alloc(8);
  if (e != hipSuccess) return gw_sgns_fail(m, GW_ERR_NOMEM, "device allocation failed: %s", hipGetErrorString(e));
  return GW_OK;
}

void gw_sgns_dev_free(gw_sgns* m) {
  gw_device_guard dg(m->device);
  delete m->dev;
  m->dev = nullptr;
}

int gw_sgns_dev_count(gw_sgns* m, const int32_t* walks_dev, int64_t nwalks, int walk_len) {
  GW_DEV_GUARD(m);
  gw_sgns_dev& dv = *m->dev;
  unsigned long long* flag = (unsigned long long*)dv.stats.get();
  GW_DEV_TRY(m, hipMemset(dv.counts.get(), 0, (size_t)m->n * sizeof(unsigned long long)));
  GW_DEV_TRY(m, hipMemset(flag, 0, sizeof(unsigned long long)));
  if (nwalks > 0) {
    const int64_t blocks = (nwalks + 255) / 256;
    if (blocks > 0x7FFFFFFF) return gw_sgns_fail(m, GW_ERR_UNSUPPORTED, "too many walks for one launch");
    k_sgns_count<<<(unsigned)blocks, 256>>>(walks_dev, nwalks, walk_len, m->n, dv.counts.get(), flag);
    GW_DEV_TRY(m, hipGetLastError());
  }
  unsigned long long bad = 0;
  GW_DEV_TRY(m, hipMemcpy(&bad, flag, sizeof bad, hipMemcpyDeviceToHost));
  if (bad) return gw_sgns_fail(m, GW_ERR_RANGE, "walk %lld holds an id outside [0, %lld)", (long long)bad - 1, (long long)m->n);
  std::vector<unsigned long long> c((size_t)m->n);
  GW_DEV_TRY(m, hipMemcpy(c.data(), dv.counts.get(), c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  m->counts.resize((size_t)m->n);
  for (size_t v = 0; v < c.size(); ++v) m->counts[v] = (int64_t)c[v];
  return GW_OK;
}

int gw_sgns_dev_upload_vocab(gw_sgns* m) {
  GW_DEV_GUARD(m);
  gw_sgns_dev& dv = *m->dev;
  const size_t n = (size_t)m->n;
  GW_DEV_TRY(m, hipMemcpy(dv.J.get(), m->J.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
  GW_DEV_TRY(m, hipMemcpy(dv.thr.get(), m->thr.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
  GW_DEV_TRY(m, hipMemcpy(dv.keep.get(), m->keep_thr.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
  GW_DEV_TRY(m, hipMemcpy(dv.expt.get(), m->expt.data(), GW_SGNS_EXP_SIZE * sizeof(float), hipMemcpyHostToDevice));
  GW_DEV_TRY(m, hipMemset(dv.syn1.get(), 0, n * (size_t)m->pitch * sizeof(float)));
  const int64_t total = m->n * m->pitch, blocks = (total + 255) / 256;
  if (blocks > 0x7FFFFFFF) return gw_sgns_fail(m, GW_ERR_UNSUPPORTED, "n * dim too large for one launch");
  k_sgns_init<<<(unsigned)blocks, 256>>>(dv.syn0.get(), m->n, m->pitch, m->p.dim, m->p.seed);
  GW_DEV_TRY(m, hipGetLastError());
  GW_DEV_TRY(m, hipDeviceSynchronize());
  return GW_OK;
}

int gw_sgns_auto_concurrency(const gw_sgns* m, int64_t nwalks) {
  int64_t c = std::min<int64_t>(nwalks, 16 * (int64_t)std::max(m->dev->cus, 1));
  c = std::min<int64_t>(c, std::max<int64_t>(1, m->n / 32));
  return (int)std::max<int64_t>(c, 1);
}

int gw_sgns_dev_train(gw_sgns* m, const int32_t* walks_dev, int64_t nwalks, int walk_len, int epoch_begin,
                      int epoch_count, int concurrency, int64_t* stats, void* stream) {
  if (walk_len > kMaxWalkLen)
    return gw_sgns_fail(m, GW_ERR_UNSUPPORTED, "walk_len %d: the kernel keeps a walk in LDS (<= %d)", walk_len, kMaxWalkLen);
  GW_DEV_GUARD(m);
  gw_sgns_dev& dv = *m->dev;
  hipStream_t st = (hipStream_t)stream;
  int conc = concurrency > 0 ? concurrency : gw_sgns_auto_concurrency(m, nwalks);
  conc = (int)std::min<int64_t>(conc, nwalks);
  SgnsArgs A;
  A.walks = walks_dev;
  A.nwalks = nwalks;
  A.walk_len = walk_len;
  A.n = m->n;
  A.pitch = m->pitch;
  A.window = m->p.window;
  A.K = m->p.negative;
  A.epochs = m->p.epochs;
  A.conc = conc;
  A.alpha0 = m->p.alpha;
  A.min_alpha = m->p.min_alpha;
  A.seed = m->p.seed;
  A.J = dv.J.get();
  A.thr = dv.thr.get();
  A.keep = dv.keep.get();
  A.expt = dv.expt.get();
  A.syn0 = dv.syn0.get();
  A.syn1 = dv.syn1.get();
  A.stats = (unsigned long long*)dv.stats.get();
  GW_DEV_TRY(m, hipMemsetAsync(dv.stats.get(), 0, 8 * sizeof(long long), st));
  const void* fn = train_kernel(m->pitch);
  const unsigned grid = (unsigned)((conc + kWaves - 1) / kWaves);
  const size_t lds = (size_t)kWaves * 2 * (size_t)walk_len * sizeof(int32_t);
  for (int e = epoch_begin; e < epoch_begin + epoch_count; ++e) {
    A.epoch = e;
    void* args[] = {&A};
    GW_DEV_TRY(m, hipLaunchKernel(fn, dim3(grid), dim3(kWaves * GW_SGNS_LANES), args, lds, st));
  }
  long long h[8];
  GW_DEV_TRY(m, hipMemcpyAsync(h, dv.stats.get(), sizeof h, hipMemcpyDeviceToHost, st));
  GW_DEV_TRY(m, hipStreamSynchronize(st));
  if (h[5]) return gw_sgns_fail(m, GW_ERR_RANGE, "the walks hold an id outside [0, %lld)", (long long)m->n);
  for (int i = 0; i < 5; ++i) stats[i] = h[i];
  return GW_OK;
}

int gw_sgns_dev_export(gw_sgns* m, float* syn0, float* syn1neg) {
  GW_DEV_GUARD(m);
  gw_sgns_dev& dv = *m->dev;
  const size_t row = (size_t)m->p.dim * sizeof(float), pitch = (size_t)m->pitch * sizeof(float), n = (size_t)m->n;
  if (syn0) GW_DEV_TRY(m, hipMemcpy2D(syn0, row, dv.syn0.get(), pitch, row, n, hipMemcpyDeviceToHost));
  if (syn1neg) GW_DEV_TRY(m, hipMemcpy2D(syn1neg, row, dv.syn1.get(), pitch, row, n, hipMemcpyDeviceToHost));
  return GW_OK;
}

extern "C" int gw_sgns_kernel_attrs(gw_sgns* m, int walk_len, int32_t* vgprs, int32_t* scratch_bytes,
                                    int32_t* lds_bytes) {
  if (!m) return gw_sgns_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (m->device < 0) return gw_sgns_fail(m, GW_ERR_STATE, "host evaluation launches no kernel");
  if (walk_len < 1 || walk_len > kMaxWalkLen) return gw_sgns_fail(m, GW_ERR_INVALID, "walk_len %d", walk_len);
  GW_DEV_GUARD(m);
  hipFuncAttributes fa;
  GW_DEV_TRY(m, hipFuncGetAttributes(&fa, train_kernel(m->pitch)));
  if (vgprs) *vgprs = fa.numRegs;
  if (scratch_bytes) *scratch_bytes = (int32_t)fa.localSizeBytes;
  if (lds_bytes) *lds_bytes = (int32_t)(fa.sharedSizeBytes + (size_t)kWaves * 2 * (size_t)walk_len * sizeof(int32_t));
  return GW_OK;
}

float* gw_sgns_dev_vectors(gw_sgns* m) { return m->dev->syn0.get(); }
