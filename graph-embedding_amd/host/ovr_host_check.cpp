// Stand-alone check of the one-vs-rest host code (csrc/gw_ovr_host.cpp built
// with -DGW_OVR_HOST_ONLY): features with a pitch, labels with an absent and an
// everywhere-present column and rows with no and every label, a gathered fit
// over more than one row block, decision values, counts, export and the error
// paths.  Meant to be built with -fsanitize=address,undefined and run as a
// plain program; exit status 0 and "ovr host check ok" = clean.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "graphwalk.h"

#define CHECK(expr)                                                          \
  do {                                                                       \
    const int rc_ = (expr);                                                  \
    if (rc_ != GW_OK) {                                                      \
      fprintf(stderr, "%s -> %d: %s\n", #expr, rc_, gw_ovr_last_error(m));   \
      return 1;                                                              \
    }                                                                        \
  } while (0)

int main() {
  const int n = 150, dim = 7, pitch = 9, L = 5, T = 131;
  gw_ovr* m = nullptr;
  gw_ovr_params_t p = {};
  p.struct_size = (int32_t)sizeof p;
  p.dim = dim;
  p.labels = L;
  p.max_newton = 50;
  p.max_cg = 50;
  p.C = 1.0;
  p.gtol = 1e-8;
  CHECK(gw_ovr_create(-1, n, &p, &m));
  uint32_t s = 2463534242u;
  auto next = [&s]() { return s = s * 1664525u + 1013904223u; };
  // exactly n * pitch - (pitch - dim) floats: the last row's pad does not exist
  std::vector<float> x((size_t)n * pitch - (pitch - dim));
  std::vector<int64_t> row_off(n + 1, 0);
  std::vector<int32_t> ids;
  for (int v = 0; v < n; ++v) {
    const int c = (int)((next() >> 8) % 3);
    for (int j = 0; j < dim; ++j)
      x[(size_t)v * pitch + j] = (float)((j % 3 == c ? 1.5 : 0.0) + ((int)((next() >> 8) % 2001) - 1000) * 1e-3);
    if (v != 140) {
      for (int l = 0; l < 3; ++l)
        if (l == c || (next() >> 8) % 10 == 0 || v == 141) ids.push_back(l);
      if (v == 141) ids.push_back(3);  // label 3: no training row has it
      ids.push_back(4);                // label 4: every row but 140
    }
    row_off[v + 1] = (int64_t)ids.size();
  }
  std::vector<int64_t> order(n);
  CHECK(gw_ovr_order(7, 1, n, order.data()));
  // rows 140 (k = 0) and 141 (k = L) go to the held-out end
  for (int want = 140; want <= 141; ++want)
    for (int i = 0; i < n; ++i)
      if (order[i] == want) {
        const int64_t t = order[n - 1 - (want - 140)];
        order[n - 1 - (want - 140)] = want;
        order[i] = t;
        break;
      }
  CHECK(gw_ovr_set_features(m, x.data(), pitch));
  CHECK(gw_ovr_set_labels(m, row_off.data(), ids.data()));
  gw_ovr_stats_t st;
  CHECK(gw_ovr_fit(m, order.data(), T, &st, nullptr));
  std::vector<double> W((size_t)L * (dim + 1)), gn(L), z((size_t)(n - T) * L);
  std::vector<int32_t> state(L), it(L);
  std::vector<int64_t> counts((size_t)L * 3);
  CHECK(gw_ovr_export(m, W.data(), state.data(), it.data(), gn.data()));
  CHECK(gw_ovr_decision(m, order.data() + T, n - T, z.data()));
  CHECK(gw_ovr_score(m, order.data() + T, n - T, counts.data(), nullptr));
  CHECK(gw_ovr_score(m, order.data(), 0, counts.data(), nullptr));
  if (state[3] != GW_OVR_CONST_NEG || state[4] != GW_OVR_CONST_POS || st.fitted != 3 || st.constant != 2) {
    fprintf(stderr, "states %d %d %d %d %d\n", state[0], state[1], state[2], state[3], state[4]);
    return 1;
  }
  for (int l = 0; l < 3; ++l)
    if (!isfinite(gn[l]) || it[l] < 1) return 1;
  // the error paths leave nothing behind
  if (gw_ovr_fit(m, order.data(), n + 1, nullptr, nullptr) != GW_ERR_INVALID) return 1;
  order[1] = order[0];
  if (gw_ovr_fit(m, order.data(), T, nullptr, nullptr) != GW_ERR_INVALID) return 1;
  order[1] = n;
  if (gw_ovr_fit(m, order.data(), T, nullptr, nullptr) != GW_ERR_RANGE) return 1;
  if (gw_ovr_score(m, order.data() + T, n - T, counts.data(), nullptr) != GW_ERR_STATE) return 1;
  ids[0] = L;
  if (gw_ovr_set_labels(m, row_off.data(), ids.data()) != GW_ERR_RANGE) return 1;
  gw_ovr_free(m);
  printf("ovr host check ok: %lld passes, newton max %d\n", (long long)st.passes, st.newton_max);
  return 0;
}
