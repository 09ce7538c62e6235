// Weighted naive SimRank on gfx950.
//
// Reference: DeepSim/TopSimAll/src/simrank/weighted/WeightedSimRank.java
//   ctor        :25-35  sim = tempSim = I
//   compute     :40-58  STEP (= 50) rounds of tempSim[i][j] = sim(i,j) for i<j,
//                       mirrored, copied back; postProcess zeroes the diagonal
//   sim(v,w)    :68-93  1 if v==w; T[v], T[w] = sums of the two weight maps;
//                       0 if deg(v)==0 or deg(w)==0; else
//                       C * (sum over list entries vn, wn of
//                            map_v[vn] * map_w[wn] * sim[vn][wn]) / (T[v]*T[w])
// With N[v][a] = the summed weights of v's adjacency entries that point at a
// the double loop is (N S N^T)[v][w]; N = N^T (WGraph.addEdge puts one value
// both ways) and S is symmetric, so one round is the two row-gather passes of
// gw_simrank.hip with a weight per streamed entry:
//   pass 1: U[j][i]  = sum_{e in row j} wt[e] * S[i][nbr e]           (U = N S)
//   pass 2: S'[i][j] = C * sum_{e in row j} wt[e] * U[i][nbr e] / (T_i T_j), j > i
// Same skeleton as k_sr_gather (compact graph of the m non-isolated vertices,
// one 1024-thread workgroup per row i, input row in LDS when it fits, row-
// padded entry stream with head bits, lane sums, segmented DPP scan, chunk
// carry, LDS output window).  What differs: the layout has 8 entries per lane
// per chunk, not 16, so that the current and the prefetched chunk (8 offsets
// + 8 fp64 weights each: 48 VGPRs) fit the 128 VGPRs a lane has at 1024
// threads without scratch; the weight stream runs parallel to the offset
// stream (12 B per entry), padding entries carry weight 0.0 and gather 0.0
// (the zero slot in LDS, forced in the HBM-row variant), so padding never
// forms 0 * NaN; the lane sum is p += w[k] * x in entry order (a multiply and
// an add: -ffp-contract=off); pass 2 divides C * val by T_i * T_j in fp64 with
// no guard, as the reference does (zero totals give NaN / Inf and propagate).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "gw_device_common.h"
#include "gw_simrank_scan.h"

namespace {

constexpr int WSR_K = 8;                 // adjacency entries per lane per chunk
constexpr int WSR_CHUNK = 64 * WSR_K;    // entries per wave per chunk

struct WsrArgs {
  int64_t m;
  const int64_t* poff;    // [m+1] row starts in the padded stream (multiples of WSR_K)
  const uint32_t* ent;    // [poff[m] + WSR_CHUNK] byte offset (8 * compact neighbour) into a row; padding 8 * m
  const double* wt;       // [poff[m] + WSR_CHUNK] weight of the entry; padding 0.0
  const uint16_t* heads;  // [(poff[m] + WSR_CHUNK) / 8] bit 0 of word g: entries 8g..8g+7 start a row
  const double* tot;      // [m] weight totals T of the compact rows
  double C;
};

// k_sr_gather (gw_simrank.hip) with a weight per entry; see the file comment.
template <bool LDS_ROW, bool PASS2>
__global__ void __launch_bounds__(SR_BLOCK) k_wsr_gather(WsrArgs A, const double* __restrict__ src,
                                                         double* __restrict__ dst, int last, int win) {
  extern __shared__ double lds[];
  const int64_t m = A.m;
  double* const in_row = lds;
  double* const out_win = LDS_ROW ? lds + m + 1 : lds;
  const int64_t i = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (PASS2 && threadIdx.x == 0) dst[i * m + i] = last ? 0.0 : 1.0;  // tempSim[i][i] stays 1
  const double* row = src + i * m;
  if (LDS_ROW) {
    for (int64_t b = threadIdx.x; b < m; b += SR_BLOCK) in_row[b] = row[b];
    if (threadIdx.x == 0) in_row[m] = 0.0;  // the padding entries' slot
  }
  const uint32_t pad_off = (uint32_t)m * 8u;
  const uint64_t below_incl = (lane == 63) ? ~0ull : ((2ull << lane) - 1);

  for (int64_t j0 = PASS2 ? i + 1 : 0; j0 < m; j0 += win) {
    const int64_t j1 = min(m, j0 + (int64_t)win);
    __syncthreads();  // in_row staged / previous window flushed
    {
      const int64_t e_lo = A.poff[j0], tot = A.poff[j1] - e_lo;
      const int64_t t0 = e_lo + tot * wave / SR_WAVES, t1 = e_lo + tot * (wave + 1) / SR_WAVES;
      const int64_t ra = wave == 0 ? j0 : first_row_at(A.poff, j0, j1, t0);
      const int64_t rb = wave == SR_WAVES - 1 ? j1 : first_row_at(A.poff, j0, j1, t1);
      const int64_t eb = A.poff[ra], ee = A.poff[rb];
      if (eb < ee) {
        // eb, ee are row starts: multiples of WSR_K, so every lane's 8 entries
        // lie inside one row and the slice is chunk-aligned
        const uint32_t* ep = A.ent + eb + WSR_K * lane;
        const double* wp = A.wt + eb + WSR_K * lane;
        const uint16_t* hp = A.heads + eb / WSR_K + lane;
        const int pe = (int)(ee - eb);  // slice = chunk positions [0, pe)
        int cur_row = (int)(ra - j0);   // the slice's first head flag is dropped: its row is cur_row
        double chunk_carry = 0.0;
        uint4 n[2];
        double2 nw[4];
        uint32_t nh;
#pragma unroll
        for (int q = 0; q < 2; ++q) n[q] = *reinterpret_cast<const uint4*>(ep + 4 * q);
#pragma unroll
        for (int q = 0; q < 4; ++q) nw[q] = *reinterpret_cast<const double2*>(wp + 2 * q);
        nh = *hp;
        for (int pos = 0; pos < pe; pos += WSR_CHUNK) {
          const uint32_t en[WSR_K] = {n[0].x, n[0].y, n[0].z, n[0].w, n[1].x, n[1].y, n[1].z, n[1].w};
          const double ew[WSR_K] = {nw[0].x, nw[0].y, nw[1].x, nw[1].y, nw[2].x, nw[2].y, nw[3].x, nw[3].y};
          uint32_t fl = nh & 1u;  // this lane's entries start a row
          if (pos + WSR_CHUNK < pe) {
#pragma unroll
            for (int q = 0; q < 2; ++q) n[q] = *reinterpret_cast<const uint4*>(ep + pos + WSR_CHUNK + 4 * q);
#pragma unroll
            for (int q = 0; q < 4; ++q) nw[q] = *reinterpret_cast<const double2*>(wp + pos + WSR_CHUNK + 2 * q);
            nh = hp[(pos + WSR_CHUNK) / WSR_K];
          }
          const int p0 = pos + WSR_K * lane;
          const bool live = p0 < pe;  // lanes past the slice end add zeros to its last row
          // one row's 8 entries, weight times gathered value, summed in entry order
          double p = 0.0;
#pragma unroll
          for (int k = 0; k < WSR_K; ++k) {
            double x;
            if (LDS_ROW) {
              x = *reinterpret_cast<const double*>(reinterpret_cast<const char*>(in_row) + en[k]);
            } else {  // the padding offset is one past the row: read a real element, use 0
              const uint32_t o = en[k] < pad_off ? en[k] : 0u;
              x = *reinterpret_cast<const double*>(reinterpret_cast<const char*>(row) + o);
              if (en[k] >= pad_off) x = 0.0;
            }
            p += ew[k] * x;
          }
          if (!live) p = 0.0;
          if (!live || p0 == 0) fl = 0u;
          const uint64_t headmask = __ballot(fl != 0);
          const int incl = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(headmask >> 32),
                                                          __builtin_amdgcn_mbcnt_lo((uint32_t)headmask, 0u)) +
                           (int)fl;
          const int total = __popcll(headmask);
          // lane 0 without a head continues the row of the previous chunk
          if (lane == 0 && fl == 0) p = chunk_carry + p;
          const uint64_t hb = headmask & below_incl;
          const int seg_start = hb ? 63 - __builtin_clzll(hb) : 0;
          const double S = seg_scan(p, lane, seg_start);
          const double prevS = dpp_f64<0x138>(S);  // wave_shr:1
          const int r = cur_row + incl;            // this lane's row
          if (fl) out_win[r - 1] = lane == 0 ? chunk_carry : prevS;  // the previous row is complete
          // the lane holding the slice's last entries writes that row
          if (live && p0 + WSR_K >= pe) out_win[r] = S;
          const uint64_t Sb = __double_as_longlong(S);
          chunk_carry = __longlong_as_double(
              (long long)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(Sb >> 32), 63) << 32) |
                          (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)Sb, 63)));
          cur_row += total;
        }
      }
    }
    __syncthreads();
    const int64_t nrow = j1 - j0;
    const double Ti = PASS2 ? A.tot[i] : 0.0;
    for (int64_t t = threadIdx.x; t < nrow; t += SR_BLOCK) {
      const int64_t j = j0 + t;
      const double val = out_win[t];
      if (!PASS2) {
        dst[j * m + i] = val;  // U = N S, stored transposed
      } else {
        const double sv = A.C * val / (Ti * A.tot[j]);  // WeightedSimRank.java:92, no guard
        dst[i * m + j] = sv;
        dst[j * m + i] = sv;
      }
    }
  }
}

template <bool LDS_ROW, bool PASS2>
hipError_t launch_pass(const WsrArgs& A, const double* src, double* dst, int last, int win, hipStream_t s) {
  const size_t lds = ((LDS_ROW ? (size_t)A.m + 1 : 0) + (size_t)win) * sizeof(double);
  hipError_t e = hipFuncSetAttribute((const void*)k_wsr_gather<LDS_ROW, PASS2>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  k_wsr_gather<LDS_ROW, PASS2><<<(unsigned)A.m, SR_BLOCK, lds, s>>>(A, src, dst, last, win);
  return hipGetLastError();
}

}  // namespace

void gw_dev_wsimrank_release(gw_graph* g) {
  gw_dev_free(g->wsr_work);
  gw_dev_free(g->wsr_x);
  gw_dev_free(g->wsr_ent);
  gw_dev_free(g->wsr_wt);
  gw_dev_free(g->wsr_heads);
  gw_dev_free(g->wsr_poff);
  gw_dev_free(g->wsr_tot);
  gw_dev_free(g->wsr_rows);
  g->wsr_n = 0;
  g->wsr_m = 0;
}

// Compact layout (built once per graph on the host): non-isolated vertices in
// ascending id order, their totals, and the row-padded streams of neighbour
// ranks and weights (each row starts on an 8-entry group; padding = 8 * m,
// the zero slot, with weight 0.0) with one head bit per group.
static int wsr_build_layout(gw_graph* g) {
  const int64_t n = g->n;
  const double* w = gw_entry_weights(g);
  std::vector<double> totals;
  gw_weight_totals(g, &totals);
  std::vector<int32_t> rank((size_t)n, -1), rows;
  std::vector<int64_t> poff(1, 0);
  std::vector<double> tot;
  rows.reserve((size_t)n);
  for (int64_t v = 0; v < n; ++v) {
    const int64_t d = g->offsets[v + 1] - g->offsets[v];
    if (d > 0) {
      rank[v] = (int32_t)rows.size();
      rows.push_back((int32_t)v);
      tot.push_back(totals[(size_t)v]);
      poff.push_back(poff.back() + (d + WSR_K - 1) / WSR_K * WSR_K);
    }
  }
  const int64_t m = (int64_t)rows.size();
  const int64_t padded = poff.back() + WSR_CHUNK;  // + one chunk: a slice's first loads stay in bounds
  std::vector<uint32_t> ent((size_t)padded, (uint32_t)m * (uint32_t)sizeof(double));
  std::vector<double> wt((size_t)padded, 0.0);
  std::vector<uint16_t> heads((size_t)(padded / WSR_K), 0);
  for (int64_t r = 0; r < m; ++r) {
    const int64_t v = rows[(size_t)r], b = g->offsets[v], e = g->offsets[v + 1];
    heads[(size_t)(poff[(size_t)r] / WSR_K)] = 1;
    for (int64_t k = b; k < e; ++k) {
      ent[(size_t)(poff[(size_t)r] + (k - b))] = (uint32_t)rank[g->nbrs[k]] * (uint32_t)sizeof(double);
      wt[(size_t)(poff[(size_t)r] + (k - b))] = w[k];
    }
  }
  auto up = [&](auto*& dptr, const auto& vec) -> bool {
    const size_t bytes = std::max<size_t>(vec.size() * sizeof(vec[0]), 16);
    if (hipMalloc((void**)&dptr, bytes) != hipSuccess) {
      (void)hipGetLastError();
      dptr = nullptr;
      return false;
    }
    return vec.empty() || hipMemcpy(dptr, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice) == hipSuccess;
  };
  if (!up(g->wsr_ent, ent) || !up(g->wsr_wt, wt) || !up(g->wsr_heads, heads) || !up(g->wsr_poff, poff) ||
      !up(g->wsr_tot, tot) || !up(g->wsr_rows, rows)) {
    g->err = "weighted SimRank adjacency layout does not fit in device memory";
    return GW_ERR_NOMEM;
  }
  g->wsr_m = m;
  return GW_OK;
}

int gw_dev_simrank_weighted(gw_graph* g, double C, int iters, double* sim_dev, void* stream) {
  GW_HIP_TRY(hipSetDevice(g->device));
  const int64_t n = g->n;
  hipStream_t s = (hipStream_t)stream;
  if (g->wsr_n != n || !g->wsr_ent) {
    gw_dev_wsimrank_release(g);
    int rc = wsr_build_layout(g);
    if (rc != GW_OK) {
      gw_dev_wsimrank_release(g);
      return rc;
    }
    const int64_t m = g->wsr_m;
    const size_t mb = std::max<size_t>((size_t)m * (size_t)m * sizeof(double), 8);
    if (hipMalloc((void**)&g->wsr_work, mb) != hipSuccess || (m < n && hipMalloc((void**)&g->wsr_x, mb) != hipSuccess)) {
      (void)hipGetLastError();
      gw_dev_wsimrank_release(g);
      g->err = "weighted SimRank workspace (m*m doubles) does not fit in device memory";
      return GW_ERR_NOMEM;
    }
    g->wsr_n = n;
  }
  if (n == 0) return GW_OK;
  const int64_t m = g->wsr_m;
  double* X = m < n ? g->wsr_x : sim_dev;  // compact S (the output itself when nothing is isolated)
  if (m < n) GW_HIP_TRY(hipMemsetAsync(sim_dev, 0, (size_t)n * n * sizeof(double), s));
  if (m > 0) {
    GW_HIP_TRY(hipMemsetAsync(X, 0, (size_t)m * m * sizeof(double), s));
    const unsigned mbk = (unsigned)((m + 255) / 256);
    k_sr_identity<<<mbk, 256, 0, s>>>(m, X);
    GW_HIP_TRY(hipGetLastError());
    WsrArgs A{m, g->wsr_poff, g->wsr_ent, g->wsr_wt, g->wsr_heads, g->wsr_tot, C};
    // the same row placement and window rule as gw_dev_simrank_naive
    const int64_t cap = SR_LDS_BYTES / (int64_t)sizeof(double);
    const bool lds_row = m + 1 + SR_MIN_WIN <= cap && !g->opt.simrank_hbm_row;
    const int64_t win_auto = std::min<int64_t>(m, lds_row ? cap - m - 1 : cap);
    const int win = (int)(g->opt.simrank_window > 0 ? std::min<int64_t>(win_auto, g->opt.simrank_window) : win_auto);
    for (int r = 0; r < iters; ++r) {  // while (r++ < STEP), WeightedSimRank.java:42
      const int last = r == iters - 1;
      hipError_t e = lds_row ? launch_pass<true, false>(A, X, g->wsr_work, 0, win, s)
                             : launch_pass<false, false>(A, X, g->wsr_work, 0, win, s);
      if (e == hipSuccess)
        e = lds_row ? launch_pass<true, true>(A, g->wsr_work, X, last, win, s)
                    : launch_pass<false, true>(A, g->wsr_work, X, last, win, s);
      GW_HIP_TRY(e);
    }
    if (iters <= 0) {
      k_sr_zero_diag<<<mbk, 256, 0, s>>>(m, X);
      GW_HIP_TRY(hipGetLastError());
    }
    if (m < n) {
      dim3 grid((unsigned)std::min<int64_t>((m + 255) / 256, 64), (unsigned)m);
      k_sr_expand<<<grid, 256, 0, s>>>(m, n, g->wsr_rows, X, sim_dev);
      GW_HIP_TRY(hipGetLastError());
    }
  }
  return GW_OK;
}

extern "C" int gw_simrank_weighted_host(gw_graph* g, double C, int iters, double* sim) {
  if (!g) return gw_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  GW_GUARD_DEVICE(g, g->device);  // restores the caller's current device on return
  int rc = gw_wsimrank_check(g, iters, true);
  if (rc != GW_OK) return rc;
  if (g->n > 0 && !sim) return gw_fail(g, GW_ERR_INVALID, "bad arguments");
  GW_HIP_TRY(hipSetDevice(g->device));
  const int64_t n = g->n;
  if (n == 0) return GW_OK;
  double* d_sim = nullptr;
  gw_dev_scratch scratch(g);
  if (scratch.alloc(&d_sim, n * n)) return gw_fail(g, GW_ERR_NOMEM, "n*n result does not fit in device memory");
  rc = gw_dev_simrank_weighted(g, C, iters, d_sim, nullptr);
  if (rc != GW_OK) return rc;
  const hipError_t e = hipMemcpy(sim, d_sim, (size_t)n * n * sizeof(double), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return gw_fail(g, GW_ERR_DEVICE, "%s", hipGetErrorString(e));
  return GW_OK;
}

extern "C" int gw_simrank_weighted_kernel_attrs(gw_graph* g, int32_t vgprs[4], int32_t scratch_bytes[4],
                                                int32_t lds_bytes[4]) {
  if (!g) return gw_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (g->device < 0) return gw_fail(g, GW_ERR_STATE, "graph is not on a device");
  GW_GUARD_DEVICE(g, g->device);
  const void* fns[4] = {(const void*)k_wsr_gather<true, false>, (const void*)k_wsr_gather<false, false>,
                        (const void*)k_wsr_gather<true, true>, (const void*)k_wsr_gather<false, true>};
  for (int i = 0; i < 4; ++i) {
    hipFuncAttributes fa;
    const hipError_t e = hipFuncGetAttributes(&fa, fns[i]);
    if (e != hipSuccess) return gw_fail(g, GW_ERR_DEVICE, "hipFuncGetAttributes: %s", hipGetErrorString(e));
    if (vgprs) vgprs[i] = (int32_t)fa.numRegs;
    if (scratch_bytes) scratch_bytes[i] = (int32_t)fa.localSizeBytes;
    if (lds_bytes) lds_bytes[i] = (int32_t)fa.sharedSizeBytes;
  }
  return GW_OK;
}
