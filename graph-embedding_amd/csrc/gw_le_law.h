// The Laplacian-eigenmap law (IsoMap_LE/simRank.py:95-123, IsoMap_LE/LE.py:35-51
// made sparse and symmetric): Chebyshev-filtered block subspace iteration on
// S = D^-1/2 W D^-1/2 in fp64.
//
// One definition for the kernels (gw_le.hip) and the host evaluation
// (gw_le_host.cpp, device = -1).  Both sides compile this source with
// -ffp-contract=off; every fused multiply-add is an explicit fma, every other
// operation rounds once, only + - * / and sqrt are used (no libm on either
// side), and no order depends on tiles, grid, thread count or timing, so the
// two agree bit for bit.  The small m x m eigenproblems (cyclic Jacobi), the
// selection and the stopping rule are host code shared by both modes.
//
//   a_ij      the caller's entries: -1 ends a row; j == i, NaN and <= 0 are dropped; of what
//             remains a repeated j keeps the last value.  With self_loops = 1 (LE.py's own matrix:
//             its knn lists the point itself, so W[i][i] = exp(0) = 1 stands in W and in D) an entry
//             j == i is kept as a_ii under the same rules: it is its own transpose (mean and max of
//             a_ii with itself are a_ii), counts in d_i and becomes the diagonal entry S_ii.  With
//             y = s o u, u'(I - S)u = sum over i < j of w_ij (y_i - y_j)^2 (the diagonal cancels) and
//             u'(I + S)u = sum over i < j of w_ij (y_i + y_j)^2 + sum over i of 2 w_ii y_i^2, both
//             >= 0: the spectrum of S stays within [-1, 1] and the filter's interval holds.
//   w_ij      (a_ij + a_ji) / 2 (GW_LE_SYM_MEAN) or max(a_ij, a_ji) (GW_LE_SYM_MAX), absent = 0
//   d_i       w_ij added over j ascending from +0; d_i == 0: the row is isolated (s_i = 0, no entries)
//   s_i       1 / sqrt(d_i);  S_ij = (w_ij * s_i) * s_j, CSR with ascending columns
//   start     X[i][c] = gw_le_start(seed, i, c) in [-1, 1), 0 on isolated rows
//   S x       row i, column c: fma(S_ij, x[j][c], t) over the row's entries ascending from +0 (gw_le_row_dot
//             states it per entry); then gw_le_combine.  A row is never split.
//   A^T B     (and column sums of squares): rows in chunks of GW_LE_CHUNK; inside a chunk an fma chain over
//             ascending rows from +0; chunk partials added in ascending chunk order from +0.  Only i <= j is
//             computed, [j][i] is its copy.
//   X Q       out[i][c] = fma(X[i][k], Q[k][c], acc) over k ascending from +0
//   residual  d = fma(-theta_c, x, y); sum of d * d under the chunk law; r_c = sqrt(sum)
//   output    v = s_i * x[i][c]; nrm_c = sqrt(sum of v * v under the chunk law); f = v / nrm_c, negated when the
//             entry of largest |v| (lowest row among equals) is negative; 0 on isolated rows; fp32 = (float)f
#pragma once
#include <stdint.h>

#include "../../include/graphwalk.h"
#include "gw_philox.h"

#define GW_LE_CHUNK 512      // rows per partial of the tall-skinny products
#define GW_LE_MAX_BLOCK 256  // device path
#define GW_TAG_LE 0x6C65586Du  // "leXm": the start block

#define GW_LE_FMA(a, b, c) __builtin_fma((a), (b), (c))
#define GW_LE_SQRT(a) __builtin_sqrt(a)

#define GW_LE_PLAIN 0  // out = t
#define GW_LE_AXPY 1   // out = fma(alpha, t, beta * x)
#define GW_LE_CHEB 2   // out = fma(alpha, t, fma(beta, x, gamma * z))

// 32 Philox bits u -> u * 2^-31 - 1, exact
GW_HD double gw_le_start(uint64_t seed, int64_t i, int c) {
  const struct gw_u4 r = gw_philox((uint32_t)i, (uint32_t)((uint64_t)i >> 32), (uint32_t)c, 0u, (uint32_t)seed,
                                   (uint32_t)(seed >> 32) ^ GW_TAG_LE);
  return (double)r.x * 4.656612873077392578125e-10 - 1.0;
}

// t = (S x)[i][c]: vals / cols are the row's entries, x the block with `pitch` doubles per row
GW_HD double gw_le_row_dot(const double* vals, const int32_t* cols, int64_t count, const double* x, int64_t pitch,
                           int64_t c) {
  double t = 0.0;
  for (int64_t e = 0; e < count; ++e) t = GW_LE_FMA(vals[e], x[(int64_t)cols[e] * pitch + c], t);
  return t;
}

GW_HD double gw_le_combine(int mode, double alpha, double t, double beta, double x, double gamma, double z) {
  if (mode == GW_LE_PLAIN) return t;
  if (mode == GW_LE_AXPY) return GW_LE_FMA(alpha, t, beta * x);
  return GW_LE_FMA(alpha, t, GW_LE_FMA(beta, x, gamma * z));
}

// the term of a residual's sum of squares
GW_HD double gw_le_res_term(double theta, double x, double y) { return GW_LE_FMA(-theta, x, y); }

// one output entry from v = s_i * x, the column's norm and sign
GW_HD double gw_le_out(double s, double x, double nrm, int negate) {
  if (s == 0.0) return 0.0;
  const double f = (s * x) / nrm;
  return negate ? -f : f;
}
