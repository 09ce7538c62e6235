// The nearest-neighbour law: all-pairs top-k of an embedding (gensim's
// KeyedVectors.most_similar, DeepSim/src/main.py:287; IsoMap_LE/LE.py:53-60 knn)
// given one fp64 order.
//
// One definition for the kernels (gw_knn.hip) and the host evaluation
// (gw_knn_host.cpp, device = -1).  Both sides compile this source with
// -ffp-contract=off; every fused multiply-add is an explicit fma, every other
// operation rounds once, only * / and sqrt are used besides (no libm on either
// side), and no order depends on tiles, grid or timing, so the two agree bit
// for bit.
//
// Features are the caller's fp32 widened; everything else is fp64.
//   dot(i,j) = fma((double)x[i][k], (double)x[j][k], acc) over k = 0 .. dim-1 ascending from +0
//              (no split-K, no reassociation; the product commutes, so dot(i,j) and dot(j,i)
//              have the same bits)
//   nrm(i)   = sqrt(dot(i,i)), correctly rounded
//   GW_KNN_DOT     s(i,j) = dot(i,j)
//   GW_KNN_COSINE  s(i,j) = dot(i,j) / (nrm(i) * nrm(j)): one multiply, one divide; a row with
//                  nrm == 0 has no neighbours and is nobody's neighbour
// The row of source v holds the topk candidates j != v of largest s(v,j).  A NaN score is
// never listed.  The order is total: score descending, then id ascending (gw_topsim's row
// order; +0 and -0 are equal scores).  A row with fewer than topk listed candidates is
// padded with (-1, 0.0).
#pragma once
#include <stdint.h>

#include "../../include/graphwalk.h"
#include "gw_philox.h"

#define GW_KNN_MAX_DIM 1024   // device path
#define GW_KNN_MAX_TOPK 128   // device path

#define GW_KNN_FMA(a, b, c) __builtin_fma((a), (b), (c))
#define GW_KNN_SQRT(a) __builtin_sqrt(a)

GW_HD double gw_knn_dot(const float* a, const float* b, int dim) {
  double acc = 0.0;
  for (int k = 0; k < dim; ++k) acc = GW_KNN_FMA((double)a[k], (double)b[k], acc);
  return acc;
}

GW_HD double gw_knn_nrm(const float* a, int dim) { return GW_KNN_SQRT(gw_knn_dot(a, a, dim)); }

// s(i,j) from dot(i,j); ni, nj are read under GW_KNN_COSINE only
GW_HD double gw_knn_score(int metric, double dot, double ni, double nj) {
  return metric == GW_KNN_COSINE ? dot / (ni * nj) : dot;
}

// may candidate j (j != v is the caller's) with score s stand in the row of a source of norm ni?
GW_HD int gw_knn_listed(int metric, double s, double ni, double nj) {
  if (metric == GW_KNN_COSINE && (ni == 0.0 || nj == 0.0)) return 0;
  return s == s;
}

// the law's total order: does (sa, ia) stand before (sb, ib)?  Neither score is NaN.
GW_HD int gw_knn_before(double sa, int32_t ia, double sb, int32_t ib) { return sa > sb || (sa == sb && ia < ib); }
