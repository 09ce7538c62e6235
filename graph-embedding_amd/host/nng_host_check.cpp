// Stand-alone check of the neighbour-graph host code (csrc/gw_nng_host.cpp built
// with -DGW_NNG_HOST_ONLY): a matrix with a pitch whose last row's pad does not
// exist, exact ties (duplicated rows), a NaN row, topk > n, both include_self
// values, heat_t 0 / ordinary / tiny, repeated and unordered sources,
// sources = NULL, out_d2 = NULL and the error paths.  Every row is compared with
// a brute-force restatement.  Meant to be built with -fsanitize=address,undefined
// and run as a plain program; exit status 0 and "nng host check ok" = clean.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "graphwalk.h"

#define CHECK(expr)                                                          \
  do {                                                                       \
    const int rc_ = (expr);                                                  \
    if (rc_ != GW_OK) {                                                      \
      fprintf(stderr, "%s -> %d: %s\n", #expr, rc_, gw_nng_last_error(m));   \
      return 1;                                                              \
    }                                                                        \
  } while (0)

#define EXPECT(cond)                                       \
  do {                                                     \
    if (!(cond)) {                                         \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond);   \
      return 1;                                            \
    }                                                      \
  } while (0)

struct Ent {
  double d2;
  int32_t j;
};

// the others of v by brute force: small integers, so every d2 is exact in any order
static std::vector<Ent> brute(const std::vector<float>& x, int n, int dim, int pitch, int v) {
  std::vector<Ent> row;
  for (int j = 0; j < n; ++j) {
    if (j == v) continue;
    double a = 0;
    for (int k = 0; k < dim; ++k) {
      const double e = (double)x[(size_t)v * pitch + k] - (double)x[(size_t)j * pitch + k];
      a += e * e;
    }
    if (a == a && a < INFINITY) row.push_back({a, j});
  }
  std::stable_sort(row.begin(), row.end(), [](const Ent& a, const Ent& b) { return a.d2 < b.d2; });  // ids ascend among equals
  return row;
}

int main() {
  const int n = 90, dim = 5, pitch = 8;
  uint32_t s = 2463534242u;
  auto next = [&s]() { return s = s * 1664525u + 1013904223u; };
  // exactly n * pitch - (pitch - dim) floats: the last row's pad does not exist
  std::vector<float> x((size_t)n * pitch - (pitch - dim), NAN);
  for (int v = 0; v < n; ++v)
    for (int k = 0; k < dim; ++k) x[(size_t)v * pitch + k] = (float)((int)((next() >> 8) % 9) - 4);
  for (int k = 0; k < dim; ++k) {
    x[(size_t)40 * pitch + k] = x[(size_t)7 * pitch + k];  // ties: rows 7, 40 and 89 are one point
    x[(size_t)89 * pitch + k] = x[(size_t)7 * pitch + k];
  }
  x[(size_t)11 * pitch + 2] = NAN;  // a NaN row: it lists itself alone and nobody lists it
  gw_nng* m = nullptr;
  for (int self : {1, 0})
    for (double heat : {0.0, 15.0, 1e-3})
      for (int topk : {6, n + 10}) {  // topk > n: padded rows
        gw_nng_params_t p = {};
        p.struct_size = (int32_t)sizeof p;
        p.dim = dim;
        p.topk = topk;
        p.include_self = self;
        p.heat_t = heat;
        CHECK(gw_nng_create(-1, n, &p, &m));
        std::vector<int32_t> ids((size_t)n * topk, 77);
        std::vector<double> w((size_t)n * topk, 77.0), d2((size_t)n * topk, 77.0);
        EXPECT(gw_nng_query(m, nullptr, 0, ids.data(), w.data(), d2.data(), nullptr) == GW_ERR_STATE);
        CHECK(gw_nng_set_vectors(m, x.data(), pitch));
        const std::vector<int32_t> src = {89, 11, 7, 40, 7, 0, 89};  // unordered, repeated, the NaN row, the last row
        for (int pass = 0; pass < 2; ++pass) {
          const int64_t rows = pass ? n : (int64_t)src.size();
          CHECK(gw_nng_query(m, pass ? nullptr : src.data(), pass ? -5 : rows, ids.data(), w.data(),
                             pass ? nullptr : d2.data(), nullptr));
          for (int64_t r = 0; r < rows; ++r) {
            const int v = pass ? (int)r : src[(size_t)r];
            const std::vector<Ent> ref = brute(x, n, dim, pitch, v);
            for (int t = 0; t < topk; ++t) {
              const size_t o = (size_t)r * topk + t;
              if (self && t == 0) {
                EXPECT(ids[o] == v && w[o] == 1.0 && (pass || d2[o] == 0.0));
                continue;
              }
              const size_t e = (size_t)(t - self);
              const bool have = e < ref.size();
              EXPECT(ids[o] == (have ? ref[e].j : -1));
              if (!pass) EXPECT(d2[o] == (have ? ref[e].d2 : 0.0));
              if (!have) EXPECT(w[o] == 0.0);
              else if (heat == 0.0 || ref[e].d2 == 0.0) EXPECT(w[o] == 1.0);
              else if (ref[e].d2 / heat > 700.0) EXPECT(w[o] == 0.0);
              else EXPECT(fabs(w[o] - exp(-ref[e].d2 / heat)) <= 1e-15 * exp(-ref[e].d2 / heat));
            }
            if (v == 11) EXPECT(ids[(size_t)r * topk + self] == -1);
          }
        }
        // the error paths write nothing
        std::vector<int32_t> keep = ids;
        std::vector<int32_t> bad = {3, n, 4};
        EXPECT(gw_nng_query(m, bad.data(), 3, ids.data(), w.data(), d2.data(), nullptr) == GW_ERR_RANGE);
        bad[1] = -1;
        EXPECT(gw_nng_query(m, bad.data(), 3, ids.data(), w.data(), nullptr, nullptr) == GW_ERR_RANGE);
        EXPECT(ids == keep);
        EXPECT(gw_nng_query(m, bad.data(), 0, nullptr, nullptr, nullptr, nullptr) == GW_OK);
        EXPECT(gw_nng_query(m, bad.data(), -1, ids.data(), w.data(), nullptr, nullptr) == GW_ERR_INVALID);
        EXPECT(gw_nng_query(m, bad.data(), 1, nullptr, w.data(), nullptr, nullptr) == GW_ERR_INVALID);
        EXPECT(gw_nng_set_vectors(m, x.data(), dim - 1) == GW_ERR_INVALID);
        EXPECT(gw_nng_set_vectors(m, nullptr, pitch) == GW_ERR_INVALID);
        EXPECT(gw_nng_tiles(m, nullptr, nullptr, nullptr, nullptr) == GW_ERR_DEVICE);  // built without the device path
        CHECK(gw_nng_set_rows(m, n - 1));
        EXPECT(gw_nng_query(m, nullptr, 0, ids.data(), w.data(), nullptr, nullptr) == GW_ERR_STATE);
        gw_nng_free(m);
        m = nullptr;
      }
  gw_nng_params_t p = {};
  p.struct_size = (int32_t)sizeof p;
  p.dim = 0;
  p.topk = 1;
  EXPECT(gw_nng_create(-1, n, &p, &m) == GW_ERR_INVALID);
  p.dim = 1;
  p.topk = 0;
  EXPECT(gw_nng_create(-1, n, &p, &m) == GW_ERR_INVALID);
  p.topk = 1;
  p.include_self = 2;
  EXPECT(gw_nng_create(-1, n, &p, &m) == GW_ERR_INVALID);
  p.include_self = 0;
  p.heat_t = -1.0;
  EXPECT(gw_nng_create(-1, n, &p, &m) == GW_ERR_INVALID);
  p.heat_t = NAN;
  EXPECT(gw_nng_create(-1, n, &p, &m) == GW_ERR_INVALID);
  p.heat_t = 1.0;
  p.struct_size = 3;
  EXPECT(gw_nng_create(-1, n, &p, &m) == GW_ERR_INVALID);
  p.struct_size = (int32_t)sizeof p;
  EXPECT(gw_nng_create(-1, 0, &p, &m) == GW_ERR_INVALID);
  EXPECT(gw_nng_create(0, n, &p, &m) == GW_ERR_DEVICE);
  printf("nng host check ok\n");
  return 0;
}
