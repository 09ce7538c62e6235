// The geodesic law: shortest-path distances from a source over a sparse graph
// with non-negative fp64 lengths (Isomap's second step, Tenenbaum, de Silva and
// Langford 2000; landmark Isomap, de Silva and Tenenbaum 2003).
//
// One definition for the kernels (gw_geo.hip) and the host evaluation
// (gw_geo_host.cpp, device = -1).  Both sides compile this source with
// -ffp-contract=off; the only operations are +, comparisons and, while the graph
// is assembled (on the host in both modes), __builtin_sqrt.
//
// Input rows (top-k layout as gw_le_set_rows takes, or a CSR):
//   an id of -1 ends a row; an id equal to its row is dropped; a value that is NaN,
//   negative or +inf is dropped; -0.0 counts as +0.0; an id outside [-1, n) gives
//   GW_ERR_RANGE; a repeated id keeps the smallest value.
//   squared = 1  the values are squared distances (gw_nng_query's out_d2) and the
//                length is __builtin_sqrt(value), taken during assembly, so device
//                and host lengths are the same bits by construction;
//   squared = 0  the values are the lengths.
//   GW_GEO_SYM_UNION (default)  l_ij = min of the listed a_ij and a_ji: an edge
//                listed one way stands both ways (Isomap's graph, and sklearn's);
//   GW_GEO_DIRECTED             the rows as listed.
// The result is a CSR with ascending columns, assembled and validated on the host.
//
// Distance:
//   dist(s, s) = +0;
//   dist(s, v) = the minimum over all paths s = v0, ..., vm = v of
//                ((0 + l(v0,v1)) + l(v1,v2)) + ... added left to right;
//   dist(s, v) = +inf where there is no path; a sum that overflows to +inf counts
//                as unreachable.
//
// Why no order of evaluation matters (so: do not "fix" the atomics).  Rounding of
// + is monotone: a <= b implies fl(a + l) <= fl(b + l).  With l >= 0 also
// fl(a + l) >= a.  Let F(v) be the minimum above.  (1) Every value any schedule
// ever stores in dist[v] is the left-to-right sum of some path to v, hence >= F(v).
// (2) If u precedes v on a path that attains F(v), its prefix attains F(u): a
// smaller prefix sum would, by monotonicity, give a sum <= F(v) along the rest of
// the path, and F(v) is the minimum.  So once dist[u] = F(u) has been relaxed over
// (u, v), dist[v] = F(v), and by induction over the hops of an attaining path every
// schedule that relaxes each improved vertex again ends at F: Dijkstra, Bellman-Ford
// in any order, near-far buckets and racing atomic minima all land on the same bits.
// A minimum, unlike a floating-point sum, does not depend on arrival order.
//
// Distances are >= +0 and never NaN, so their bit patterns order as unsigned 64-bit
// integers and +inf lies above every finite value: the kernels relax with integer
// atomic minima on the bit patterns.
//
// Components: connected components of the symmetrised graph (also for
// GW_GEO_DIRECTED: weak components) by host union-find; a component's id is its
// lowest vertex; the main component is the largest, the lowest id winning ties.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/graphwalk.h"
#include "gw_philox.h"  // GW_HD

#define GW_GEO_INF_BITS 0x7FF0000000000000ull

// may a listed value stand as an edge?  NaN, negative and +inf may not; -0.0 may (as +0.0)
GW_HD int gw_geo_listed(double v) { return v >= 0.0 && v < __builtin_inf(); }

// the length of a listed value: -0.0 becomes +0.0; squared: its root
GW_HD double gw_geo_length(double v, int squared) {
  const double a = v == 0.0 ? 0.0 : v;
  return squared ? __builtin_sqrt(a) : a;
}

GW_HD unsigned long long gw_geo_bits(double d) {
  unsigned long long b;
  memcpy(&b, &d, sizeof b);
  return b;
}

GW_HD double gw_geo_double(unsigned long long b) {
  double d;
  memcpy(&d, &b, sizeof d);
  return d;
}

// one relaxation: the candidate distance of v through u, as a bit pattern.  du is a finite distance, l a length;
// an overflowing sum gives the +inf pattern, which improves nothing.
GW_HD unsigned long long gw_geo_relax(unsigned long long du, double l) { return gw_geo_bits(gw_geo_double(du) + l); }
