// The spring-layout law: the Fruchterman-Reingold force simulation of networkx
// 3.4.2's dense _fruchterman_reingold (the layout under nx.draw_spring, which
// IsoMap_LE/simRank.py:show ends in), stated for a sparse matrix, fp64 throughout.
//
// One definition for the kernels (gw_layout.hip) and the host evaluation
// (gw_layout_host.cpp, device = -1).  Both sides compile this source with
// -ffp-contract=off and no fast-math flag; the operations are +, -, *, /,
// comparisons and gw_layout_sqrt.  fp64 / and sqrt are correctly rounded on
// gfx950 as on the host, so equal operands in an equal order give equal bits.
//
// Matrix A (a CSR, or top-k rows as gw_le_set_rows takes them), used as listed:
//   an id of -1 ends a row; an id equal to its row is dropped; an id outside
//   [-1, n) gives GW_ERR_RANGE; a value that is not finite gives GW_ERR_INVALID;
//   a negative value stands (it repels); repeated ids stay separate entries, whose
//   terms add.  No symmetrisation, no sorting: the stored order is the law's.
//
// One iteration at temperature t, for every vertex i, dim coordinates c:
//   d_ij[c] = pos_i[c] - pos_j[c];  d2_ij = d[0]*d[0] + d[1]*d[1] (+ d[2]*d[2]), left to right
//   R_i[c]  = sum_j d_ij[c] * (k*k / max(d2_ij, 1e-4))          every j, j = i included (+0)
//   T_i[c]  = sum_e d_ie[c] * ((a_e * max(sqrt(d2_ie), 0.01)) / k)   the entries of row i
//   disp_i  = R_i - T_i;  len_i = sqrt(disp[0]^2 + disp[1]^2 (+ disp[2]^2));  len_i < 0.01: len_i = 0.1
//   step_i  = disp_i * (t / len_i), +0 for a fixed vertex;  pos_i += step_i
// networkx clips the distance at 0.01 and divides k*k by its square; R clips d2 at
// 1e-4 and divides by it, which spares the all-pairs path a root per pair.  The two
// differ by rounding only.
//
// The order of every sum (a function of n alone, never of a device or a launch):
//   R_i     columns in chunks of GW_LAYOUT_CHUNK consecutive ids.  In a chunk, strand
//           a (of GW_LAYOUT_STRANDS) takes the chunk's columns number a, a + STRANDS,
//           ... ascending from +0; the chunk's sum is the strands added ascending
//           from +0; R_i is the chunks' sums added ascending from +0.  (A workgroup
//           owns one chunk for a block of rows; the strands are a thread's
//           independent accumulators.)
//   T_i     the row's entries in stored order from +0.
//   norm    s_i = step[0]^2 + step[1]^2 (+ step[2]^2); vertices in blocks of
//           GW_LAYOUT_BLOCK consecutive ids, a block summed ascending from +0, the
//           blocks' sums added ascending from +0; the run stops after an iteration
//           with sqrt(sum) / n < threshold.
//   means   of the rescale: per coordinate, the same blocks.
//
// Cooling: t0 = 0.1 * max(extent of coordinate 0, extent of coordinate 1) over the
// starting positions (a maximum and a minimum: no order), dt = t0 / (iterations + 1),
// t -= dt after every iteration.
//
// Rescale (networkx's rescale_layout and the shift after it): pos -= mean per
// coordinate (sum / n); lim = max |pos|; lim > 0: pos *= scale / lim; pos += center.
#pragma once
#include <stdint.h>

#include "../../include/graphwalk.h"
#include "gw_philox.h"  // GW_HD

#define GW_LAYOUT_CHUNK 1024
#define GW_LAYOUT_STRANDS 4
#define GW_LAYOUT_BLOCK 64

// loops over coordinates and strands have constant trip counts: the kernels keep their arrays in registers
#if defined(__clang__)
#define GW_LAYOUT_UNROLL _Pragma("unroll")
#else
#define GW_LAYOUT_UNROLL _Pragma("GCC unroll 8")
#endif

// the one root both sides compile (correctly rounded on gfx950 and on the host)
GW_HD double gw_layout_sqrt(double x) { return __builtin_sqrt(x); }

// acc += the repulsion term of column position pj on row position pi
template <int DIM>
GW_HD void gw_layout_pair(const double* pi, const double* pj, double kk, double* acc) {
  double d[DIM];
GW_LAYOUT_UNROLL
  for (int c = 0; c < DIM; ++c) d[c] = pi[c] - pj[c];
  double d2 = d[0] * d[0];
GW_LAYOUT_UNROLL
  for (int c = 1; c < DIM; ++c) d2 = d2 + d[c] * d[c];
  const double f = kk / (d2 < 1e-4 ? 1e-4 : d2);
GW_LAYOUT_UNROLL
  for (int c = 0; c < DIM; ++c) acc[c] = acc[c] + d[c] * f;
}

// out[DIM] = the sum of one chunk: cols holds the positions of its m <= GW_LAYOUT_CHUNK columns
template <int DIM>
GW_HD void gw_layout_chunk(const double* pi, const double* cols, int m, double kk, double* out) {
  double acc[GW_LAYOUT_STRANDS][DIM];
GW_LAYOUT_UNROLL
  for (int a = 0; a < GW_LAYOUT_STRANDS; ++a)
GW_LAYOUT_UNROLL
    for (int c = 0; c < DIM; ++c) acc[a][c] = 0.0;
  int j = 0;
  for (; j + GW_LAYOUT_STRANDS <= m; j += GW_LAYOUT_STRANDS) {
GW_LAYOUT_UNROLL
    for (int a = 0; a < GW_LAYOUT_STRANDS; ++a) gw_layout_pair<DIM>(pi, cols + (int64_t)(j + a) * DIM, kk, acc[a]);
  }
GW_LAYOUT_UNROLL
  for (int a = 0; a < GW_LAYOUT_STRANDS; ++a)
    if (j + a < m) gw_layout_pair<DIM>(pi, cols + (int64_t)(j + a) * DIM, kk, acc[a]);
GW_LAYOUT_UNROLL
  for (int c = 0; c < DIM; ++c) {
    double s = 0.0;
GW_LAYOUT_UNROLL
    for (int a = 0; a < GW_LAYOUT_STRANDS; ++a) s = s + acc[a][c];
    out[c] = s;
  }
}

// term[DIM] = the attraction term of one entry (neighbour position pj, value a)
template <int DIM>
GW_HD void gw_layout_pull(const double* pi, const double* pj, double a, double k, double* term) {
  double d[DIM];
GW_LAYOUT_UNROLL
  for (int c = 0; c < DIM; ++c) d[c] = pi[c] - pj[c];
  double d2 = d[0] * d[0];
GW_LAYOUT_UNROLL
  for (int c = 1; c < DIM; ++c) d2 = d2 + d[c] * d[c];
  const double dist = gw_layout_sqrt(d2);
  const double w = (a * (dist < 0.01 ? 0.01 : dist)) / k;
GW_LAYOUT_UNROLL
  for (int c = 0; c < DIM; ++c) term[c] = d[c] * w;
}

// disp = R - T, step = disp * (t / len) or +0; returns s_i, the vertex's share of the stop norm
template <int DIM>
GW_HD double gw_layout_move(const double* R, const double* T, double t, int fixed, double* disp, double* step) {
GW_LAYOUT_UNROLL
  for (int c = 0; c < DIM; ++c) disp[c] = R[c] - T[c];
  double l2 = disp[0] * disp[0];
GW_LAYOUT_UNROLL
  for (int c = 1; c < DIM; ++c) l2 = l2 + disp[c] * disp[c];
  double len = gw_layout_sqrt(l2);
  if (len < 0.01) len = 0.1;
  const double f = t / len;
GW_LAYOUT_UNROLL
  for (int c = 0; c < DIM; ++c) step[c] = fixed ? 0.0 : disp[c] * f;
  double s = step[0] * step[0];
GW_LAYOUT_UNROLL
  for (int c = 1; c < DIM; ++c) s = s + step[c] * step[c];
  return s;
}

// one block of a sum over vertices: x[first * stride], x[(first + 1) * stride], ... for the block's vertices below n
GW_HD double gw_layout_block_sum(const double* x, int64_t stride, int64_t block, int64_t n) {
  const int64_t i0 = block * GW_LAYOUT_BLOCK;
  const int64_t i1 = i0 + GW_LAYOUT_BLOCK < n ? i0 + GW_LAYOUT_BLOCK : n;
  double s = 0.0;
  for (int64_t i = i0; i < i1; ++i) s = s + x[i * stride];
  return s;
}

// the stop test on the sum of every s_i
GW_HD int gw_layout_stops(double sum, int64_t n, double threshold) {
  return gw_layout_sqrt(sum) / (double)n < threshold;
}

GW_HD double gw_layout_t0(double min0, double max0, double min1, double max1) {
  const double e0 = max0 - min0, e1 = max1 - min1;
  return (e0 < e1 ? e1 : e0) * 0.1;
}
