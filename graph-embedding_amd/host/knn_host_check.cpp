// Stand-alone check of the nearest-neighbour host code (csrc/gw_knn_host.cpp
// built with -DGW_KNN_HOST_ONLY): a matrix with a pitch whose last row's pad
// does not exist, exact ties (duplicated rows), a zero row, topk > n - 1,
// repeated and unordered sources, sources = NULL, gw_topk_label_agreement and
// the error paths.  Every row is compared with a brute-force restatement.
// Meant to be built with -fsanitize=address,undefined and run as a plain
// program; exit status 0 and "knn host check ok" = clean.
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
      fprintf(stderr, "%s -> %d: %s\n", #expr, rc_, gw_knn_last_error(m));   \
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
  double s;
  int32_t j;
};

// the row of v by brute force: small integers, so every dot is exact in any order
static std::vector<Ent> brute(const std::vector<float>& x, int n, int dim, int pitch, int metric, int v) {
  std::vector<double> nrm(n);
  for (int i = 0; i < n; ++i) {
    double a = 0;
    for (int k = 0; k < dim; ++k) a += (double)x[(size_t)i * pitch + k] * x[(size_t)i * pitch + k];
    nrm[i] = sqrt(a);
  }
  std::vector<Ent> row;
  for (int j = 0; j < n; ++j) {
    if (j == v || (metric == GW_KNN_COSINE && (nrm[j] == 0 || nrm[v] == 0))) continue;
    double a = 0;
    for (int k = 0; k < dim; ++k) a += (double)x[(size_t)v * pitch + k] * x[(size_t)j * pitch + k];
    row.push_back({metric == GW_KNN_COSINE ? a / (nrm[v] * nrm[j]) : a, j});
  }
  std::stable_sort(row.begin(), row.end(), [](const Ent& a, const Ent& b) { return a.s > b.s; });  // ids ascend among equals
  return row;
}

int main() {
  const int n = 90, dim = 5, pitch = 8;
  uint32_t s = 2463534242u;
  auto next = [&s]() { return s = s * 1664525u + 1013904223u; };
  // exactly n * pitch - (pitch - dim) floats: the last row's pad does not exist
  std::vector<float> x((size_t)n * pitch - (pitch - dim), NAN);
  for (int v = 0; v < n; ++v)
    for (int k = 0; k < dim; ++k) x[(size_t)v * pitch + k] = (float)((int)((next() >> 8) % 7) - 3);
  for (int k = 0; k < dim; ++k) {
    x[(size_t)11 * pitch + k] = 0.f;                        // a zero row
    x[(size_t)40 * pitch + k] = x[(size_t)7 * pitch + k];   // ties: rows 7, 40 and 89 are one vector
    x[(size_t)89 * pitch + k] = x[(size_t)7 * pitch + k];
  }
  gw_knn* m = nullptr;
  for (int metric : {GW_KNN_COSINE, GW_KNN_DOT})
    for (int topk : {6, n + 10}) {  // topk > n - 1: padded rows
      gw_knn_params_t p = {};
      p.struct_size = (int32_t)sizeof p;
      p.dim = dim;
      p.topk = topk;
      p.metric = metric;
      CHECK(gw_knn_create(-1, n, &p, &m));
      std::vector<int32_t> ids((size_t)n * topk, 77);
      std::vector<double> sc((size_t)n * topk, 77.0);
      EXPECT(gw_knn_query(m, nullptr, 0, ids.data(), sc.data(), nullptr) == GW_ERR_STATE);
      CHECK(gw_knn_set_vectors(m, x.data(), pitch));
      const std::vector<int32_t> src = {89, 11, 7, 40, 7, 0, 89};  // unordered, repeated, the zero row, the last row
      for (int pass = 0; pass < 2; ++pass) {
        const int64_t rows = pass ? n : (int64_t)src.size();
        CHECK(gw_knn_query(m, pass ? nullptr : src.data(), pass ? -5 : rows, ids.data(), sc.data(), nullptr));
        for (int64_t r = 0; r < rows; ++r) {
          const int v = pass ? (int)r : src[(size_t)r];
          const std::vector<Ent> ref = brute(x, n, dim, pitch, metric, v);
          for (int t = 0; t < topk; ++t) {
            const bool have = (size_t)t < ref.size();
            EXPECT(ids[(size_t)r * topk + t] == (have ? ref[(size_t)t].j : -1));
            EXPECT(sc[(size_t)r * topk + t] == (have ? ref[(size_t)t].s : 0.0));
          }
          if (metric == GW_KNN_COSINE && v == 11) EXPECT(ids[(size_t)r * topk] == -1);
        }
      }
      // the error paths write nothing
      std::vector<int32_t> keep = ids;
      std::vector<int32_t> bad = {3, n, 4};
      EXPECT(gw_knn_query(m, bad.data(), 3, ids.data(), sc.data(), nullptr) == GW_ERR_RANGE);
      bad[1] = -1;
      EXPECT(gw_knn_query(m, bad.data(), 3, ids.data(), sc.data(), nullptr) == GW_ERR_RANGE);
      EXPECT(ids == keep);
      EXPECT(gw_knn_query(m, bad.data(), 0, nullptr, nullptr, nullptr) == GW_OK);
      EXPECT(gw_knn_query(m, bad.data(), -1, ids.data(), sc.data(), nullptr) == GW_ERR_INVALID);
      EXPECT(gw_knn_query(m, bad.data(), 1, nullptr, sc.data(), nullptr) == GW_ERR_INVALID);
      EXPECT(gw_knn_set_vectors(m, x.data(), dim - 1) == GW_ERR_INVALID);
      EXPECT(gw_knn_set_vectors(m, nullptr, pitch) == GW_ERR_INVALID);
      EXPECT(gw_knn_tiles(m, nullptr, nullptr, nullptr, nullptr) == GW_ERR_DEVICE);  // built without the device path
      CHECK(gw_knn_set_rows(m, n - 1));
      EXPECT(gw_knn_query(m, nullptr, 0, ids.data(), sc.data(), nullptr) == GW_ERR_STATE);
      gw_knn_free(m);
      m = nullptr;
    }
  gw_knn_params_t p = {};
  p.struct_size = (int32_t)sizeof p;
  p.dim = 0;
  p.topk = 1;
  EXPECT(gw_knn_create(-1, n, &p, &m) == GW_ERR_INVALID);
  p.dim = 1;
  p.topk = 0;
  EXPECT(gw_knn_create(-1, n, &p, &m) == GW_ERR_INVALID);
  p.topk = 1;
  p.metric = 2;
  EXPECT(gw_knn_create(-1, n, &p, &m) == GW_ERR_INVALID);
  p.metric = 0;
  p.struct_size = 3;
  EXPECT(gw_knn_create(-1, n, &p, &m) == GW_ERR_INVALID);
  p.struct_size = (int32_t)sizeof p;
  EXPECT(gw_knn_create(-1, 0, &p, &m) == GW_ERR_INVALID);
  EXPECT(gw_knn_create(0, n, &p, &m) == GW_ERR_DEVICE);
  // label agreement: vertex 2 has no label, row 1 is padded after one entry, row 2 is all padding
  const int64_t off[] = {0, 2, 3, 3, 5};
  const int32_t lab[] = {0, 3, 3, 1, 3};
  const int32_t nb[] = {1, 2, 3, 0, -1, -1, -1, -1, -1};
  double acc[3];
  EXPECT(gw_topk_label_agreement(nb, 3, 3, nullptr, off, lab, 4, acc) == GW_OK);
  EXPECT(acc[0] == 1.0 && acc[1] == 2.0 / 3.0 && acc[2] == 3.0 / 4.0);
  EXPECT(gw_topk_label_agreement(nb + 6, 1, 3, nullptr, off, lab, 4, acc) == GW_OK && acc[0] == 0.0 && acc[2] == 0.0);
  const int32_t far[] = {4, -1, -1};
  EXPECT(gw_topk_label_agreement(far, 1, 3, nullptr, off, lab, 4, acc) == GW_ERR_RANGE);
  printf("knn host check ok\n");
  return 0;
}
