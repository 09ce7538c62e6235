// What the SimRank gather kernels share (gw_simrank.hip: k_sr_gather,
// gw_wsimrank.hip: k_wsr_gather): the workgroup shape and LDS budget, the
// identity / diagonal / expand kernels around the rounds, the slice search
// and the wave-wide segmented DPP scan.  Device code, one copy per
// translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int SR_BLOCK = 1024;
constexpr int SR_WAVES = SR_BLOCK / 64;
constexpr int64_t SR_LDS_BYTES = 152 * 1024;     // dynamic LDS per workgroup (input row + window)
constexpr int64_t SR_MIN_WIN = 2048;             // smallest output window (rows)

__global__ void k_sr_identity(int64_t n, double* __restrict__ S) {
  const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (v < n) S[v * n + v] = 1.0;  // SimRank.java:27-30
}

__global__ void k_sr_zero_diag(int64_t n, double* __restrict__ S) {
  const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (v < n) S[v * n + v] = 0.0;  // postProcess, SimRank.java:62-65
}

// out[rows[a]][rows[b]] = X[a][b] (out pre-zeroed: isolated rows/cols are 0)
__global__ void k_sr_expand(int64_t m, int64_t n, const int32_t* __restrict__ rows, const double* __restrict__ X,
                            double* __restrict__ out) {
  const int64_t a = blockIdx.y;
  const int64_t ra = rows[a];
  for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < m; b += (int64_t)gridDim.x * blockDim.x)
    out[ra * n + rows[b]] = X[a * m + b];
}

// first row r in [lo, hi] with off[r] >= e (off is non-decreasing)
__device__ __forceinline__ int64_t first_row_at(const int64_t* __restrict__ off, int64_t lo, int64_t hi, int64_t e) {
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (off[mid] < e)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// DPP lane moves (gfx9 wave64 controls): row_shr:d = 0x110+d, row_bcast:15 =
// 0x142, row_bcast:31 = 0x143, wave_shr:1 = 0x138.  Invalid sources read 0.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ double dpp_f64(double v) {
  const uint64_t u = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, ROW_MASK, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, ROW_MASK, 0xF, true);
  return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo));
}
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ int dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, true);
}

// Segmented inclusive sum over the wave: lane l sums lanes [seg_start(l), l].
__device__ __forceinline__ double seg_scan(double S, int lane, int seg) {
  const int r = lane & 15;
  double t;
  t = dpp_f64<0x111>(S); if (r >= 1 && lane - 1 >= seg) S += t;
  t = dpp_f64<0x112>(S); if (r >= 2 && lane - 2 >= seg) S += t;
  t = dpp_f64<0x114>(S); if (r >= 4 && lane - 4 >= seg) S += t;
  t = dpp_f64<0x118>(S); if (r >= 8 && lane - 8 >= seg) S += t;
  t = dpp_f64<0x142, 0xA>(S); if ((lane & 16) && (lane & ~15) - 1 >= seg) S += t;
  t = dpp_f64<0x143, 0xC>(S); if (lane >= 32 && 31 >= seg) S += t;
  return S;
}

}  // namespace
