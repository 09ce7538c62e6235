// Stand-alone check of the Laplacian-eigenmap host code (csrc/gw_le_host.cpp
// built with -DGW_LE_HOST_ONLY): rows with padding, self entries, NaN and
// non-positive scores and repeated ids; a ring with its closed-form spectrum,
// iterated (block < rows) and exact (block clamped); two rings and an isolated
// vertex; a CSR whose nbrs end exactly at offsets[n]; gw_le_apply; the error
// paths.  Meant to be built with -fsanitize=address,undefined and run as a
// plain program; exit status 0 and "le host check ok" = clean.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "graphwalk.h"

#define CHECK(expr)                                                         \
  do {                                                                      \
    const int rc_ = (expr);                                                 \
    if (rc_ != GW_OK) {                                                     \
      fprintf(stderr, "%s -> %d: %s\n", #expr, rc_, gw_le_last_error(m));   \
      return 1;                                                             \
    }                                                                       \
  } while (0)

#define EXPECT(cond)                                       \
  do {                                                     \
    if (!(cond)) {                                         \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond);   \
      return 1;                                            \
    }                                                      \
  } while (0)

static gw_le_params_t params(int dim, int block) {
  gw_le_params_t p;
  memset(&p, 0, sizeof p);
  p.struct_size = (int32_t)sizeof p;
  p.dim = dim;
  p.block = block;
  p.cheb_degree = 8;
  p.max_iters = 200;
  p.tol = 1e-9;
  p.min_eigenvalue = 1e-5;
  p.seed = 5;
  return p;
}

// rings of the given lengths one after another, then `extra` vertices without edges, as an exactly sized CSR
static void rings(const std::vector<int>& lens, int extra, std::vector<int64_t>& off, std::vector<int32_t>& nb) {
  off.assign(1, 0);
  nb.clear();
  int base = 0;
  for (int L : lens) {
    for (int i = 0; i < L; ++i) {
      nb.push_back(base + (i + L - 1) % L);
      nb.push_back(base + (i + 1) % L);
      off.push_back((int64_t)nb.size());
    }
    base += L;
  }
  for (int i = 0; i < extra; ++i) off.push_back((int64_t)nb.size());
}

int main() {
  gw_le* m = nullptr;
  const double pi = 3.14159265358979323846;
  // a ring of 12: lambda_k = 1 - cos(2 pi k / 12); once iterated, once with the block clamped to the 12 rows
  for (int block : {8, 40}) {
    std::vector<int64_t> off;
    std::vector<int32_t> nb;
    rings({12}, 0, off, nb);
    gw_le_params_t p = params(4, block);
    CHECK(gw_le_create(-1, 12, &p, &m));
    EXPECT(gw_le_solve(m, nullptr, nullptr) == GW_ERR_STATE);
    CHECK(gw_le_set_csr(m, off.data(), nb.data(), nullptr));
    gw_le_stats_t st;
    CHECK(gw_le_solve(m, &st, nullptr));
    EXPECT(st.state == GW_LE_CONVERGED && st.skipped == 1 && st.isolated == 0 && st.block_used == (block < 12 ? block : 12));
    if (block > 12) EXPECT(st.iters == 1 && st.applies == 1);
    double lam[4], res[4];
    std::vector<double> vec(12 * 4);
    CHECK(gw_le_export(m, lam, vec.data(), res));
    for (int c = 0; c < 4; ++c) {
      EXPECT(fabs(lam[c] - (1.0 - cos(2 * pi * (1 + c / 2) / 12))) < 1e-9);
      double nrm = 0;
      for (int i = 0; i < 12; ++i) nrm += vec[i * 4 + c] * vec[i * 4 + c];
      EXPECT(fabs(nrm - 1.0) < 1e-13);
    }
    float* f32 = nullptr;
    int64_t pitch = 0;
    CHECK(gw_le_vectors_dev(m, &f32, &pitch));
    EXPECT(pitch == 4);
    for (int i = 0; i < 48; ++i) EXPECT(f32[i] == (float)vec[i]);
    // y = S x on an exactly sized block: S of the unweighted ring is 1/2 on both neighbours
    std::vector<double> x(12 * 3), y(12 * 3, 7.0);
    for (int i = 0; i < 36; ++i) x[i] = (double)((i * 7) % 11) - 5.0;
    CHECK(gw_le_apply(m, x.data(), y.data(), 3));
    for (int i = 0; i < 12; ++i)
      for (int c = 0; c < 3; ++c)
        EXPECT(fabs(y[i * 3 + c] - 0.5 * (x[((i + 11) % 12) * 3 + c] + x[((i + 1) % 12) * 3 + c])) < 1e-14);
    EXPECT(gw_le_apply(m, x.data(), y.data(), 0) == GW_ERR_INVALID);
    EXPECT(gw_le_tiles(m, nullptr, nullptr, nullptr) == GW_OK);
    EXPECT(gw_le_kernel_attrs(m, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == GW_ERR_DEVICE);
    gw_le_free(m);
    m = nullptr;
  }
  {  // two rings and an isolated vertex: two zero eigenvalues, one row of zeros
    std::vector<int64_t> off;
    std::vector<int32_t> nb;
    rings({12, 9}, 1, off, nb);
    gw_le_params_t p = params(3, 8);
    CHECK(gw_le_create(-1, 22, &p, &m));
    CHECK(gw_le_set_csr(m, off.data(), nb.data(), nullptr));
    gw_le_stats_t st;
    CHECK(gw_le_solve(m, &st, nullptr));
    EXPECT(st.state == GW_LE_CONVERGED && st.skipped == 2 && st.isolated == 1);
    std::vector<double> vec(22 * 3);
    CHECK(gw_le_export(m, nullptr, vec.data(), nullptr));
    for (int c = 0; c < 3; ++c) EXPECT(vec[21 * 3 + c] == 0.0);
    // a block that cannot hold the zero eigenvalues, dim and one more
    gw_le_free(m);
    p = params(2, 4);
    CHECK(gw_le_create(-1, 22, &p, &m));
    CHECK(gw_le_set_csr(m, off.data(), nb.data(), nullptr));
    EXPECT(gw_le_solve(m, &st, nullptr) == GW_ERR_CAPACITY);
    EXPECT(strstr(gw_le_last_error(m), "block 5 needed") != nullptr);
    EXPECT(gw_le_export(m, nullptr, vec.data(), nullptr) == GW_ERR_STATE);
    gw_le_free(m);
    m = nullptr;
  }
  {  // rows: padding, a self entry, NaN, a non-positive score, a repeated id, and nothing read behind the -1
    const int n = 4, topk = 4;
    const int32_t ids[n * topk] = {1, 0, 1, -1,   /* self; 1 twice: the last (0.5) stays */
                                   2, 3, -1, 99,  /* 99 stands behind the padding */
                                   3, 0, 1, 2,    /* NaN, non-positive, ok, self */
                                   -1, 0, 0, 0};
    const double sc[n * topk] = {0.25, 9.0, 0.5, 0.0, 1.0, 0.125, 0.0, 0.0, NAN, -1.0, 2.0, 5.0, 0.0, 0.0, 0.0, 0.0};
    gw_le_params_t p = params(1, 4);
    p.symmetrize = GW_LE_SYM_MAX;
    CHECK(gw_le_create(-1, n, &p, &m));
    CHECK(gw_le_set_rows(m, ids, sc, topk));
    // a: (0,1) = .5, (1,2) = 1, (1,3) = .125, (2,1) = 2;  max: w01 = .5, w12 = 2, w13 = .125
    const double w[4][4] = {{0, .5, 0, 0}, {.5, 0, 2, .125}, {0, 2, 0, 0}, {0, .125, 0, 0}};
    double d[4], x[4] = {1, -2, 3, 5}, y[4];
    for (int i = 0; i < 4; ++i) d[i] = w[i][0] + w[i][1] + w[i][2] + w[i][3];
    CHECK(gw_le_apply(m, x, y, 1));
    for (int i = 0; i < 4; ++i) {
      double r = 0;
      for (int j = 0; j < 4; ++j) r += w[i][j] / sqrt(d[i] * d[j]) * x[j];
      EXPECT(fabs(y[i] - r) < 1e-14);
    }
    int32_t bad[n * topk];
    memcpy(bad, ids, sizeof bad);
    bad[5] = n;
    EXPECT(gw_le_set_rows(m, bad, sc, topk) == GW_ERR_RANGE);
    EXPECT(gw_le_apply(m, x, y, 1) == GW_ERR_STATE);  // a failed set leaves no operator
    bad[5] = -2;
    EXPECT(gw_le_set_rows(m, bad, sc, topk) == GW_ERR_RANGE);
    EXPECT(gw_le_set_rows(m, nullptr, sc, topk) == GW_ERR_INVALID);
    gw_le_free(m);
    m = nullptr;
  }
  gw_le_params_t p = params(4, 4);
  EXPECT(gw_le_create(-1, 10, &p, &m) == GW_ERR_INVALID);  // dim >= block
  p = params(0, 4);
  EXPECT(gw_le_create(-1, 10, &p, &m) == GW_ERR_INVALID);
  p = params(2, 4);
  p.symmetrize = 2;
  EXPECT(gw_le_create(-1, 10, &p, &m) == GW_ERR_INVALID);
  p = params(2, 4);
  p.tol = 0.0;
  EXPECT(gw_le_create(-1, 10, &p, &m) == GW_ERR_INVALID);
  p = params(2, 4);
  p.struct_size = 3;
  EXPECT(gw_le_create(-1, 10, &p, &m) == GW_ERR_INVALID);
  p = params(2, 4);
  EXPECT(gw_le_create(-1, 0, &p, &m) == GW_ERR_INVALID);
  EXPECT(gw_le_create(0, 10, &p, &m) == GW_ERR_DEVICE);  // built without the device path
  printf("le host check ok\n");
  return 0;
}
