// Stand-alone check of the SDNE host code (csrc/gw_sdne_host.cpp built with
// -DGW_SDNE_HOST_ONLY): sparse rows with an empty row and a row tail that is
// never trained on, a reduction longer than one chunk, gradients, 3 training
// steps in two pieces, the encoding, the state, then the same rows dense and
// the error paths, then the graph loss (nonzero_weight, first_order, shuffle)
// on a square CSR matrix.  Meant to be built with -fsanitize=address,undefined and
// run as a plain program; exit status 0 and "sdne host check ok" = clean.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "graphwalk.h"

#define CHECK(expr)                                                             \
  do {                                                                          \
    const int rc_ = (expr);                                                     \
    if (rc_ != GW_OK) {                                                         \
      fprintf(stderr, "%s -> %d: %s\n", #expr, rc_, gw_sdne_last_error(m));     \
      return 1;                                                                 \
    }                                                                           \
  } while (0)

int main() {
  const int u0 = 131, u1 = 9, u2 = 5, u3 = 7, B = 6, N = 2 * B + 3;
  gw_sdne* m = nullptr;
  gw_sdne_params_t p = {};
  p.struct_size = (int32_t)sizeof p;
  const int units[5] = {u0, u1, u2, u3, u0};
  for (int i = 0; i < 5; ++i) p.units[i] = units[i];
  p.batch = B;
  p.learning_rate = 0.01;
  p.beta1 = 0.9;
  p.beta2 = 0.999;
  p.epsilon = 1e-8;
  p.weight_decay = 0.1;
  p.kl_weight = 0.1;
  p.kl_target = 0.005;
  p.seed = 42;
  p.nonzero_weight = 1.0;
  CHECK(gw_sdne_create(-1, &p, &m));
  uint32_t x = 12345u;
  auto next = [&x]() { return x = x * 1664525u + 1013904223u; };
  std::vector<int64_t> offs(N + 1, 0);
  std::vector<int32_t> cols;
  std::vector<float> vals;
  for (int r = 0; r < N; ++r) {
    const int n = r == 4 ? 0 : 3 + (int)(next() >> 8) % 5;
    int c = (int)(next() >> 8) % 11;
    for (int e = 0; e < n && c < u0; ++e) {
      cols.push_back(c);
      vals.push_back(0.25f * (float)(1 + e));
      c += 1 + (int)(next() >> 8) % 23;
    }
    offs[(size_t)r + 1] = (int64_t)cols.size();
  }
  CHECK(gw_sdne_set_rows_csr(m, offs.data(), cols.data(), vals.data(), N));
  const size_t numel[8] = {(size_t)u0 * u1, (size_t)u1, (size_t)u1 * u2, (size_t)u2,
                           (size_t)u2 * u3, (size_t)u3, (size_t)u3 * u0, (size_t)u0};
  std::vector<float> g[8], par[8], am[8], av[8];
  float *gp[8], *pp[8], *mp[8], *vp[8];
  for (int t = 0; t < 8; ++t) {
    g[t].resize(numel[t]), par[t].resize(numel[t]), am[t].resize(numel[t]), av[t].resize(numel[t]);
    gp[t] = g[t].data(), pp[t] = par[t].data(), mp[t] = t == 3 ? nullptr : am[t].data(), vp[t] = av[t].data();
  }
  CHECK(gw_sdne_gradients(m, 1, gp));
  double loss[3];
  CHECK(gw_sdne_train(m, 0, 2, loss, nullptr));
  CHECK(gw_sdne_train(m, 2, 1, loss + 2, nullptr));
  CHECK(gw_sdne_export(m, pp, mp, vp));
  std::vector<float> enc((size_t)N * u2), tail((size_t)3 * u2);
  CHECK(gw_sdne_encode(m, 0, N, enc.data()));
  CHECK(gw_sdne_encode(m, N - 3, 3, tail.data()));
  if (memcmp(tail.data(), enc.data() + (size_t)(N - 3) * u2, tail.size() * sizeof(float)) != 0) return 1;
  float* vec = nullptr;
  int64_t pitch = 0;
  CHECK(gw_sdne_vectors_dev(m, &vec, &pitch));
  if (pitch != u2 || memcmp(vec, enc.data(), enc.size() * sizeof(float)) != 0) return 1;
  for (int i = 0; i < 3; ++i)
    if (!isfinite(loss[i])) {
      fprintf(stderr, "loss %d not finite\n", i);
      return 1;
    }
  // the same rows dense, with a pitch wider than the row, encode to the same bits
  const int64_t dp = u0 + 3;
  std::vector<float> dense((size_t)N * dp, 0.0f);
  for (int r = 0; r < N; ++r)
    for (int64_t e = offs[(size_t)r]; e < offs[(size_t)r + 1]; ++e) dense[(size_t)(r * dp + cols[(size_t)e])] = vals[(size_t)e];
  CHECK(gw_sdne_set_rows_dense(m, dense.data(), N, dp));
  std::vector<float> enc2((size_t)N * u2);
  CHECK(gw_sdne_encode(m, 0, N, enc2.data()));
  if (memcmp(enc.data(), enc2.data(), enc.size() * sizeof(float)) != 0) {
    fprintf(stderr, "dense and CSR rows encode differently\n");
    return 1;
  }
  // the error paths leave nothing behind
  if (gw_sdne_set_rows_csr(m, offs.data(), cols.data(), vals.data(), B - 1) != GW_ERR_INVALID) return 1;
  if (gw_sdne_train(m, 0, 1, nullptr, nullptr) != GW_OK) return 1;  // the earlier rows are still set
  const int32_t saved = cols[1];
  cols[1] = cols[0];
  if (gw_sdne_set_rows_csr(m, offs.data(), cols.data(), vals.data(), N) != GW_ERR_INVALID) return 1;
  cols[1] = u0;
  if (gw_sdne_set_rows_csr(m, offs.data(), cols.data(), vals.data(), N) != GW_ERR_RANGE) return 1;
  cols[1] = saved;
  if (gw_sdne_encode(m, N - 1, 2, nullptr) != GW_ERR_INVALID) return 1;
  gw_sdne_free(m);
  gw_sdne* bad = nullptr;
  p.units[4] = u0 + 1;
  if (gw_sdne_create(-1, &p, &bad) != GW_ERR_INVALID || bad) return 1;
  // the graph loss: weighted nonzeros, the first-order term and shuffled batches on a square CSR matrix with an
  // empty row, a few steps across an epoch boundary and one gradients call
  {
    const int n = 2 * B + 3;
    gw_sdne_params_t q = p;
    q.units[0] = q.units[4] = n;
    q.nonzero_weight = 3.0;
    q.first_order = 0.7;
    q.shuffle = 1;
    CHECK(gw_sdne_create(-1, &q, &m));
    std::vector<int64_t> so(n + 1, 0);
    std::vector<int32_t> sc;
    std::vector<float> sv;
    for (int r = 0; r < n; ++r) {
      for (int c = 0; c < n && r != 4; ++c)
        if (c != r && (next() >> 8) % 3 == 0) {
          sc.push_back(c);
          sv.push_back(0.5f + 0.25f * (float)((next() >> 8) % 4));
        }
      so[(size_t)r + 1] = (int64_t)sc.size();
    }
    if (gw_sdne_set_rows_csr(m, so.data(), sc.data(), sv.data(), n - 1) != GW_ERR_INVALID) return 1;  // not square
    CHECK(gw_sdne_set_rows_csr(m, so.data(), sc.data(), sv.data(), n));
    std::vector<int64_t> ids((size_t)B);
    std::vector<char> seen((size_t)n, 0);
    for (int t = 0; t < 2; ++t) {  // epoch 0: 2B distinct rows
      CHECK(gw_sdne_batch_rows(m, t, ids.data()));
      for (const int64_t r : ids) {
        if (r < 0 || r >= n || seen[(size_t)r]) return 1;
        seen[(size_t)r] = 1;
      }
    }
    double gl[5];
    CHECK(gw_sdne_train(m, 0, 3, gl, nullptr));
    CHECK(gw_sdne_train(m, 3, 2, gl + 3, nullptr));
    const size_t gn[8] = {(size_t)n * u1, (size_t)u1, (size_t)u1 * u2, (size_t)u2,
                          (size_t)u2 * u3, (size_t)u3, (size_t)u3 * n, (size_t)n};
    std::vector<float> gg[8];
    float* ggp[8];
    for (int t = 0; t < 8; ++t) gg[t].resize(gn[t]), ggp[t] = gg[t].data();
    CHECK(gw_sdne_gradients(m, 5, ggp));
    std::vector<float> genc((size_t)n * u2);
    CHECK(gw_sdne_encode(m, 0, n, genc.data()));
    for (int i = 0; i < 5; ++i)
      if (!isfinite(gl[i])) return 1;
    for (const float v : gg[2])
      if (!isfinite(v)) return 1;
    gw_sdne_free(m);
    q.nonzero_weight = 0.0;
    if (gw_sdne_create(-1, &q, &bad) != GW_ERR_INVALID || bad) return 1;
    q.nonzero_weight = 3.0, q.first_order = -1.0;
    if (gw_sdne_create(-1, &q, &bad) != GW_ERR_INVALID || bad) return 1;
    q.first_order = 0.7, q.shuffle = 2;
    if (gw_sdne_create(-1, &q, &bad) != GW_ERR_INVALID || bad) return 1;
  }
  printf("sdne host check ok: loss %.6f %.6f %.6f\n", loss[0], loss[1], loss[2]);
  return 0;
}
