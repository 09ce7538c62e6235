// The SDNE training law: the reference's four-layer dense autoencoder
// (SDNE/SDNE.py: model and loss :66-122, batches :153-157, encoding :170-172)
// given one float order.
//
// One definition for the kernels (gw_sdne.hip) and the host evaluation
// (gw_sdne_host.cpp, device = -1).  Both sides compile this source with
// -ffp-contract=off; every fused multiply-add below is an explicit fmaf, every
// other operation rounds once, and no order depends on launch geometry, so the
// two agree bit for bit.
//
// Float order (B = batch, units u0..u4 with u4 = u0, KC = GW_SDNE_KC, Bf = (float)B):
//   product        out[r][c] over a reduction index k in [0, K): chunk n = k in [n*KC, min(K, (n+1)*KC));
//                  chunk 0 is an fmaf chain over k ascending starting from the bias (forward) or +0
//                  (backward); every later chunk is the same chain from +0; out = chunk 0, then the later
//                  chunks added in ascending order by plain adds.  K <= KC is a single chain.
//   step t         rows gw_sdne_row(i), i in [0, B): nb = floor(N / B), epoch e = t / nb, slot s = (t mod nb) * B + i;
//                  shuffle off: row = s (the reference's ordered batches, the last N mod B rows never drawn);
//                  shuffle on: row = gw_feistel_perm(s, N, seed low ^ (uint32)(e >> 32), seed high ^ "sdP0",
//                  (uint32)e), so an epoch's nb * B slots are distinct rows of all N and each epoch leaves another
//                  N mod B of them out.  The encoding is always in row order.
//   z1 = x . w1 + b1 (K = u0), h1 = max(z1, +0)
//   z2 = h1 . w2 + b2 (K = u1): the embedding; h2 = max(z2, +0)
//   z3 = h2 . w3 + b3 (K = u2), h3 = max(z3, +0)
//   y  = h3 . w4 + b4 (K = u3)
//   dz4[b][i]      = (w * (y - x)) / Bf, w = bw where x != 0, else 1.0f; bw = (float)beta * (float)beta, one fp32
//                  multiply on the host (the paper's weighting of nonzero entries; at beta = 1, 1 * d = d: the
//                  reference's expression bit for bit)
//   q              = (rows ascending of (h2[b][j] over j ascending, plain adds from +0), plain adds from +0)
//                    / (float)(B * u2)
//   klg            = gw_sdne_kl_grad(q, ...): one scalar
//   dz3            = dz4 . w4^T (K = u0), 0 where z3 <= 0
//   dz2            = (dz3 . w3^T (K = u3)) + klg, 0 where z2 <= 0; with alpha > 0, + g1 by one plain add after the
//                  mask (z2 feeds the first-order term before the relu, so the term is not masked); with alpha = 0 no
//                  add happens at all
//   g1[i][c]       the first-order term L1 = (alpha / B) * sum over i, j in the batch of a_ij * |z2_i - z2_j|^2,
//                  a_ij = x_i[row(j)] read from the staged batch (needs N = u0): S_ij = a_ij + a_ji (one plain add),
//                  acc = the fmaf chain over j ascending from +0 of fmaf(S_ij, z2[i][c] - z2[j][c], acc),
//                  g1 = coef * acc, coef = (float)(2 * alpha / B) computed in fp64 and cast once.  Skipping a j with
//                  S_ij = 0 leaves the bits alone for finite z2: acc starts at +0 and a sum of round-to-nearest is
//                  -0 only when both terms are, so acc is never -0 and fmaf(+-0, d, acc) = acc.
//   dz1            = dz2 . w2^T (K = u2), 0 where z1 <= 0
//   dW_l[i][j]     = product over b (K = B) of in_l[b][i] * dz_l[b][j], in_l = x, h1, h2, h3;
//                    g = fmaf(wd, W_l[i][j], dW_l[i][j])
//   db_l[j]        = plain adds of dz_l[b][j] over b ascending from +0; g = fmaf(wd, b_l[j], db_l[j])
//   Adam           = gw_sdne_adam below on all eight tensors, lr_t computed in fp64 on the host and cast once;
//                    every backward product reads the weights of before the step
// The reported loss is computed in fp64 and is not part of the bit law: sum(w * (y - x)^2) / 2 / B + the decay and
// KL terms + L1.
#pragma once
#include <math.h>

#include "gw_philox.h"

#define GW_TAG_SDNE_INIT 0x73644930u  // "sdI0": initial w1..w4
#define GW_TAG_SDNE_PERM 0x73645030u  // "sdP0": an epoch's row permutation

#define GW_SDNE_KC 128           // reduction chunk of the law
#define GW_SDNE_MAX_HIDDEN 1024  // device path: u1, u2, u3
#define GW_SDNE_MAX_BATCH 128    // device path (= KC: a weight gradient is a single chain)

// tensor t = 2 * layer + (0 weight | 1 bias), layer 0..3
#define GW_SDNE_NT 8

GW_HD int64_t gw_sdne_chunks(int64_t K) { return (K + GW_SDNE_KC - 1) / GW_SDNE_KC; }

// row of slot i of step t (see "step t" above)
GW_HD int64_t gw_sdne_row(uint64_t seed, int shuffle, int64_t N, int64_t B, uint64_t t, int64_t i) {
  const uint64_t nb = (uint64_t)(N / B);
  const uint64_t e = t / nb;
  const uint64_t s = (t % nb) * (uint64_t)B + (uint64_t)i;
  if (!shuffle) return (int64_t)s;
  return (int64_t)gw_feistel_perm(s, (uint64_t)N, (uint32_t)seed ^ (uint32_t)(e >> 32),
                                  (uint32_t)(seed >> 32) ^ GW_TAG_SDNE_PERM, (uint32_t)e);
}

// the weighted reconstruction gradient of one entry
GW_HD float gw_sdne_dz4(float y, float x, float bw, float Bf) {
  const float d = y - x;
  const float w = x != 0.0f ? bw : 1.0f;
  const float wdv = w * d;
  return wdv / Bf;
}

// d/dh2 of kl_w * KL(p || q), q = mean(h2): one scalar for the whole batch
GW_HD float gw_sdne_kl_grad(float q, float p, float klw, float count) {
  const float a = q + 1e-8f;
  const float t1 = p / a;
  const float omq = 1.0f - q;
  const float d = omq + 1e-8f;
  const float omp = 1.0f - p;
  const float t2 = omp / d;
  const float s = t2 - t1;
  const float w = klw * s;
  return w / count;
}

struct gw_sdne_adam_c {
  float b1, omb1, b2, omb2, eps, lr_t;
};

// TF1 AdamOptimizer: lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t), t = step + 1 (fp64, one cast)
GW_HD struct gw_sdne_adam_c gw_sdne_adam_consts(double lr, double beta1, double beta2, double eps, uint64_t step) {
  struct gw_sdne_adam_c c;
  const double t = (double)(step + 1);
  c.b1 = (float)beta1;
  c.omb1 = (float)(1.0 - beta1);
  c.b2 = (float)beta2;
  c.omb2 = (float)(1.0 - beta2);
  c.eps = (float)eps;
  c.lr_t = (float)(lr * sqrt(1.0 - pow(beta2, t)) / (1.0 - pow(beta1, t)));
  return c;
}

GW_HD void gw_sdne_adam(float* th, float* m, float* v, float g, const struct gw_sdne_adam_c c) {
  const float m1 = c.b1 * *m;
  const float m2 = c.omb1 * g;
  const float mn = m1 + m2;
  const float gg = g * g;
  const float v1 = c.b2 * *v;
  const float v2 = c.omb2 * gg;
  const float vn = v1 + v2;
  const float den = sqrtf(vn) + c.eps;
  const float num = c.lr_t * mn;
  const float q = num / den;
  *m = mn;
  *v = vn;
  *th = *th - q;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// initial value of element `index` of tensor `tensor` (host only, fp64):
// truncated_normal(stddev 0.1): Box-Muller, redrawn while |z| > 2
static inline float gw_sdne_init(uint64_t seed, uint64_t index, uint32_t tensor) {
  for (uint32_t attempt = 0;; ++attempt) {
    const struct gw_u4 u = gw_philox((uint32_t)index, (uint32_t)(index >> 32), tensor, attempt, (uint32_t)seed,
                                     (uint32_t)(seed >> 32) ^ GW_TAG_SDNE_INIT);
    const double u1 = ((double)u.x + 1.0) * 2.3283064365386963e-10;
    const double u2 = (double)u.y * 2.3283064365386963e-10;
    const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
    if (fabs(z) <= 2.0) return (float)(0.1 * z);
  }
}
#endif
