// The neighbour-graph law: the k Euclidean nearest neighbours of every point and
// their heat-kernel weights (IsoMap_LE/LE.py:35-60: knn, then
// W[i][j] = exp(-|x_i - x_j|^2 / t)), given one fp64 order.
//
// One definition for the kernels (gw_nng.hip) and the host evaluation
// (gw_nng_host.cpp, device = -1).  Both sides compile this source with
// -ffp-contract=off; every fused multiply-add is an explicit fma, every other
// operation rounds once, only + - * / and gw_ovr_exp (gw_ovr_law.h, itself made
// of those) are used (no libm on either side), and no order depends on tiles,
// grid, thread count or timing, so the two agree bit for bit.
//
// Features are the caller's fp32 widened; everything else is fp64.
//   d2(i,j)  e = (double)x[i][k] - (double)x[j][k], acc = fma(e, e, acc) over k = 0 .. dim-1
//            ascending from +0: the reference's difference form (LE.py:42-44), not
//            |a|^2 + |b|^2 - 2 a.b.  It is never negative, exactly 0 for equal rows, and
//            d2(i,j) and d2(j,i) have the same bits (e only changes sign).  No split-K, no
//            reassociation.
//   row of v the candidates are the j != v whose d2(v,j) is neither NaN nor +inf; they
//            stand by d2 ascending, then id ascending (a total order).
//            include_self = 0: the first topk of them.
//            include_self = 1 (LE.py's knn: a point is its own nearest neighbour): entry 0
//            is (v, d2 = 0, weight 1.0) whatever row v holds, then the first topk - 1
//            candidates.  Where other rows equal row v exactly, numpy's argsort may put one
//            of them first and leave v out of the reference's row; here v always leads.
//   weight   heat_t > 0: w = gw_ovr_exp(-(d2 / heat_t)): exactly 1.0 at d2 = 0, +0 once
//            d2 / heat_t > 700 (such an entry is listed, and is no edge for gw_le);
//            heat_t == 0: every listed weight is 1.0 (Belkin and Niyogi's simple-minded
//            variant).
// A row with fewer listed entries than topk is padded with (-1, 0.0), d2 0.0.
#pragma once
#include <stdint.h>

#include "../../include/graphwalk.h"
#include "gw_ovr_law.h"  // gw_ovr_exp: the project's fp64 exp for x <= 0

#define GW_NNG_MAX_DIM 1024   // device path
#define GW_NNG_MAX_TOPK 128   // device path

#define GW_NNG_FMA(a, b, c) __builtin_fma((a), (b), (c))

// one column of d2: both features widened, one subtract, one fma
GW_HD double gw_nng_step(double a, double b, double acc) {
  const double e = a - b;
  return GW_NNG_FMA(e, e, acc);
}

GW_HD double gw_nng_d2(const float* a, const float* b, int dim) {
  double acc = 0.0;
  for (int k = 0; k < dim; ++k) acc = gw_nng_step((double)a[k], (double)b[k], acc);
  return acc;
}

// may a candidate at squared distance d2 stand in a row?  NaN and +inf may not (d2 is never negative).
GW_HD int gw_nng_listed(double d2) { return d2 < __builtin_inf(); }

// the law's total order: does (da, ia) stand before (db, ib)?  Neither distance is NaN.
GW_HD int gw_nng_before(double da, int32_t ia, double db, int32_t ib) { return da < db || (da == db && ia < ib); }

GW_HD double gw_nng_weight(double d2, double heat_t) { return heat_t > 0.0 ? gw_ovr_exp(-(d2 / heat_t)) : 1.0; }
