// gw_simrank_weighted_ref: the weighted SimRank recurrence
// (simrank/weighted/WeightedSimRank.java:40-93) on the host, in the two-pass
// sparse form the kernel uses (gw_wsimrank.hip): per round
//   U[j][i]  = sum_{e in row j} wt[e] * S[i][nbr e]
//   S'[i][j] = C * sum_{e in row j} wt[e] * U[i][nbr e] / (T_i T_j),  j > i, mirrored
// fp64, entry order within a row, rows ascending, one output row per OpenMP
// task.  No device.  The CPU baseline of tools/bench_wsimrank.py and the
// subject of the CPU tests; equal to the kernel up to summation order.
#include <algorithm>
#include <vector>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "gw_internal.h"

extern "C" int gw_simrank_weighted_ref(const gw_graph* g_, double C, int iters, int nthreads, double* sim) {
  if (!g_) return gw_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  gw_graph* g = const_cast<gw_graph*>(g_);  // the error slot only
  int rc = gw_wsimrank_check(g, iters, false);
  if (rc != GW_OK) return rc;
  const int64_t n = g->n;
  if (n > 0 && !sim) return gw_fail(g, GW_ERR_INVALID, "bad arguments");
  if (n == 0) return GW_OK;
  const double* wt = gw_entry_weights(g);
  std::vector<double> T;
  gw_weight_totals(g, &T);
  const int64_t* off = g->offsets.data();
  const int32_t* nb = g->nbrs.data();
  std::vector<int32_t> live;  // vertices with an adjacency entry: every other row and column is 0
  for (int64_t v = 0; v < n; ++v)
    if (off[v + 1] > off[v]) live.push_back((int32_t)v);
  const int64_t m = (int64_t)live.size();
  std::fill(sim, sim + n * n, 0.0);
  for (int64_t v = 0; v < n; ++v) sim[v * n + v] = 1.0;
  std::vector<double> U((size_t)(n * n), 0.0);
#ifdef _OPENMP
  const int nt = nthreads > 0 ? nthreads : omp_get_max_threads();
#else
  (void)nthreads;
#endif
  for (int r = 0; r < iters; ++r) {
#pragma omp parallel for schedule(dynamic, 4) num_threads(nt)
    for (int64_t a = 0; a < m; ++a) {
      const int64_t i = live[(size_t)a];
      const double* row = sim + i * n;
      for (int64_t b = 0; b < m; ++b) {
        const int64_t j = live[(size_t)b];
        double p = 0.0;
        for (int64_t k = off[j]; k < off[j + 1]; ++k) p += wt[k] * row[nb[k]];
        U[(size_t)(j * n + i)] = p;
      }
    }
#pragma omp parallel for schedule(dynamic, 4) num_threads(nt)
    for (int64_t a = 0; a < m; ++a) {
      const int64_t i = live[(size_t)a];
      const double* row = U.data() + i * n;
      for (int64_t b = a + 1; b < m; ++b) {
        const int64_t j = live[(size_t)b];
        double p = 0.0;
        for (int64_t k = off[j]; k < off[j + 1]; ++k) p += wt[k] * row[nb[k]];
        const double sv = C * p / (T[(size_t)i] * T[(size_t)j]);  // :92, no guard
        sim[i * n + j] = sv;  // rows i < j: a thread writes its own row i and column i
        sim[j * n + i] = sv;
      }
    }
  }
  for (int64_t v = 0; v < n; ++v) sim[v * n + v] = 0.0;  // postProcess (:63-66)
  return GW_OK;
}
