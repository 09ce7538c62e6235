// Stand-alone check of the DeepSim host code (csrc/gw_deepsim_host.cpp built
// with -DGW_DEEPSIM_HOST_ONLY): build a table with empty, short and dropped
// entries, train 3 steps of the host law, read batch, gradients and state
// back, write the embedding.  Meant to be built with -fsanitize=address,undefined
// and run as a plain program; exit status 0 and "deepsim host check ok" = clean.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "graphwalk.h"

#define CHECK(expr)                                                                          \
  do {                                                                                       \
    const int rc_ = (expr);                                                                  \
    if (rc_ != GW_OK) {                                                                      \
      fprintf(stderr, "%s -> %d: %s\n", #expr, rc_, gw_deepsim_last_error(m));               \
      return 1;                                                                              \
    }                                                                                        \
  } while (0)

int main(int argc, char** argv) {
  const int V = 37, topk = 5, dim = 12, window = 2, batch = 8, nwalks = 20, L = 9;
  gw_deepsim* m = nullptr;
  gw_deepsim_params_t p = {};
  p.struct_size = (int32_t)sizeof p;
  p.vertex_num = V;
  p.dim = dim;
  p.window = window;
  p.batch = batch;
  p.fallback = GW_DEEPSIM_FALLBACK_POSITION;
  p.learning_rate = 0.001;
  p.beta1 = 0.9;
  p.beta2 = 0.999;
  p.epsilon = 1e-8;
  p.score_scale = 1.0;
  p.seed = 42;
  CHECK(gw_deepsim_create(-1, &p, &m));
  std::vector<int32_t> ids((size_t)V * topk, -1);
  std::vector<double> sc((size_t)V * topk, 0.0);
  uint32_t x = 12345u;
  auto next = [&x]() { return x = x * 1664525u + 1013904223u; };
  for (int v = 0; v < V; ++v) {
    const int n = v % 6 == 2 ? 0 : 1 + (int)(next() >> 8) % topk;
    for (int e = 0; e < n; ++e) {
      ids[(size_t)v * topk + e] = (v + 1 + e * 3) % V;
      sc[(size_t)v * topk + e] = e == n - 1 && v % 4 == 0 ? 1e-9 : 0.9 / (1 + e);
    }
  }
  CHECK(gw_deepsim_set_simrank(m, ids.data(), sc.data(), topk));
  std::vector<int32_t> walks((size_t)nwalks * L);
  std::vector<int64_t> labels((size_t)V);
  for (int v = 0; v < V; ++v) labels[(size_t)v] = (v * 5) % V;
  for (size_t i = 0; i < walks.size(); ++i) walks[i] = (int32_t)((next() >> 8) % V);
  for (int i = 3; i < L; ++i) walks[(size_t)2 * L + i] = -1;  // too short to be drawn
  for (int i = 0; i < L; ++i) walks[(size_t)7 * L + i] = -1;
  CHECK(gw_deepsim_set_walks(m, walks.data(), nwalks, L, labels.data(), V));
  const int W = 2 * window + 1;
  std::vector<int32_t> centre(batch), tid((size_t)batch * W), tn(batch);
  std::vector<float> tval((size_t)batch * W), ysum(batch);
  CHECK(gw_deepsim_batch(m, 0, centre.data(), tid.data(), tval.data(), tn.data(), ysum.data()));
  std::vector<float> gw1((size_t)V * dim), gb1(dim), gw2((size_t)dim * V), gb2(V);
  CHECK(gw_deepsim_gradients(m, 0, gw1.data(), gb1.data(), gw2.data(), gb2.data()));
  double loss[3];
  CHECK(gw_deepsim_train(m, 0, 2, loss, nullptr));
  CHECK(gw_deepsim_train(m, 2, 1, loss + 2, nullptr));
  std::vector<float> w1((size_t)V * dim), b1(dim), w2((size_t)dim * V), b2(V), mw1((size_t)V * dim), vb2(V);
  float* par[4] = {w1.data(), b1.data(), w2.data(), b2.data()};
  float* am[4] = {mw1.data(), nullptr, nullptr, nullptr};
  float* av[4] = {nullptr, nullptr, nullptr, vb2.data()};
  CHECK(gw_deepsim_export(m, par, am, av));
  for (int i = 0; i < 3; ++i)
    if (!isfinite(loss[i])) {
      fprintf(stderr, "loss %d not finite\n", i);
      return 1;
    }
  if (argc > 1) CHECK(gw_write_deepsim_text(argv[1], w1.data(), V, dim));
  // the error paths leave nothing behind
  if (gw_deepsim_set_walks(m, walks.data(), 3, L, nullptr, 0) != GW_ERR_INVALID) return 1;
  walks[0] = V;
  if (gw_deepsim_set_walks(m, walks.data(), nwalks, L, labels.data(), V) != GW_ERR_RANGE) return 1;
  gw_deepsim_free(m);
  printf("deepsim host check ok: loss %.6f %.6f %.6f\n", loss[0], loss[1], loss[2]);
  return 0;
}
