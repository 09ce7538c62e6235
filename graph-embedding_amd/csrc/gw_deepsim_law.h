// The DeepSim training law: the reference's SimRank-guided one-hidden-layer
// net (DeepSim/src/DeepSim.py: get_batch :268-342, deepSim :111-195) made
// counter-based and given one float order.
//
// One definition for the kernels (gw_deepsim.hip) and the host evaluation
// (gw_deepsim_host.cpp, device = -1).  Both sides compile this source with
// -ffp-contract=off; every fused multiply-add below is an explicit fmaf, every
// other operation rounds once, and no order depends on launch geometry, so the
// two agree bit for bit.
//
// Float order (B = batch, d = dim, V = vertex_num, TW = GW_DS_TW):
//   hidden[b][h]  = max(w1[c_b][h] + b1[h], +0)
//   logits[b][j]  = fmaf chain over h ascending, starting from b2[j]
//   tile T        = columns [T*TW, min(V, (T+1)*TW))
//   m_T[b]        = max of the tile's logits (exact)
//   s_T[b]        = sum over the tile's j ascending of exp(l - m_T), plain adds from +0
//   M[b]          = max_T m_T;  S[b] = fmaf(s_T, exp(m_T - M), S) over T ascending from +0
//   dlogits[b][j] = ((exp(l - M) / S) * ysum - y[b][j]) / (float)B
//   part[T][b][h] = fmaf(dlogits[b][j], w2[h][j], acc) over the tile's j ascending from +0
//   dhidden[b][h] = plain adds of part[T][b][h] over T ascending from +0; 0 where w1[c]+b1 <= 0
//   dw2[h][j]     = fmaf(hidden[b][h], dlogits[b][j], acc) over b ascending from +0
//   db2[j]        = plain adds of dlogits[b][j] over b ascending from +0
//   dw1[c]        = plain adds of dhidden[b] over the slots b with centre c, ascending, from +0
//   db1[h]        = plain adds of dhidden[b][h] over b ascending from +0
//   Adam          = gw_ds_adam below, lr_t computed in fp64 on the host and cast once
#pragma once
#include <math.h>

#include "gw_philox.h"

#define GW_TAG_DS_BATCH 0x64734230u  // "dsB0": position draw of a slot
#define GW_TAG_DS_INIT 0x64734930u   // "dsI0": initial w1 / w2
#define GW_TAG_DS_PERM 0x64735030u   // "dsP0": the step's walk permutation

#define GW_DS_TW 64           // column-tile width of the law
#define GW_DS_MAX_WINDOW 64   // device path
#define GW_DS_MAX_TOPK 1024   // device path
#define GW_DS_DROP 1e-8       // read_simrank keeps value > 1e-8

#define GW_DS_W1 0
#define GW_DS_B1 1
#define GW_DS_W2 2
#define GW_DS_B2 3

GW_HD uint32_t gw_ds_f2u(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  return u;
}
GW_HD float gw_ds_u2f(uint32_t u) {
  float x;
  __builtin_memcpy(&x, &u, 4);
  return x;
}

// slot s of step t takes the walk eligible[gw_ds_walk_slot(...)]: distinct within a step.
// The Feistel tweak is t's low word; t's high word goes into k0.
GW_HD uint64_t gw_ds_walk_slot(uint64_t seed, uint64_t t, uint32_t s, uint64_t n_eligible) {
  return gw_feistel_perm((uint64_t)s, n_eligible, (uint32_t)seed ^ (uint32_t)(t >> 32),
                         (uint32_t)(seed >> 32) ^ GW_TAG_DS_PERM, (uint32_t)t);
}

// position in [k, len - k) of slot s of step t in a walk of `len` >= 2k+1 tokens
GW_HD int gw_ds_pos(uint64_t seed, uint64_t t, uint32_t s, int len, int k) {
  const struct gw_u4 u = gw_philox((uint32_t)t, (uint32_t)(t >> 32), s, 0u, (uint32_t)seed,
                                   (uint32_t)(seed >> 32) ^ GW_TAG_DS_BATCH);
  return k + (int)(((uint64_t)u.x * (uint64_t)(uint32_t)(len - 2 * k)) >> 32);
}

// sim(c, j): binary search in the id-sorted row of the centre (get_batch :303-316)
GW_HD float gw_ds_lookup(const int32_t* ids, const float* vals, int cnt, int32_t j, float fallback) {
  int lo = 0, hi = cnt - 1;
  while (lo <= hi) {
    const int mid = (lo + hi) >> 1;
    const int32_t v = ids[mid];
    if (v == j) return vals[mid];
    if (j > v)
      lo = mid + 1;
    else
      hi = mid - 1;
  }
  return fallback;
}

// exp(x) for x <= 0: n = round(x * log2 e), r = x - n * ln 2 (two fmaf), a degree-7
// Horner polynomial in fmaf, then 2^n added to the exponent field.  x < -86 gives +0.
GW_HD float gw_ds_exp(float x) {
  if (!(x >= -86.0f)) return 0.0f;
  const float t = x * 1.44269502162933349609375f;
  const int n = (int)(t - 0.5f);  // t <= 0: truncation rounds half away from zero
  const float nf = (float)n;
  float r = fmaf(nf, -0.693145751953125f, x);
  r = fmaf(nf, -1.428606765330187045037746429443359375e-06f, r);
  float p = 1.98412701138295233249664306640625e-04f;  // 1/5040
  p = fmaf(p, r, 1.38888892251998186111450195312500e-03f);
  p = fmaf(p, r, 8.33333376795053482055664062500000e-03f);
  p = fmaf(p, r, 4.16666679084300994873046875000000e-02f);
  p = fmaf(p, r, 1.66666671633720397949218750000000e-01f);
  p = fmaf(p, r, 0.5f);
  p = fmaf(p, r, 1.0f);
  p = fmaf(p, r, 1.0f);
  return gw_ds_u2f(gw_ds_f2u(p) + ((uint32_t)n << 23));
}

// dlogits of one element: l its logit, M / S the row's maximum and exp-sum
GW_HD float gw_ds_dlogit(float l, float M, float S, float ysum, float y, float Bf) {
  const float p = gw_ds_exp(l - M) / S;
  const float a = p * ysum;
  const float g = a - y;
  return g / Bf;
}

struct gw_ds_adam_c {
  float b1, omb1, b2, omb2, eps, lr_t;
};

// TF1 AdamOptimizer: lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t), t = step + 1 (fp64, one cast)
GW_HD struct gw_ds_adam_c gw_ds_adam_consts(double lr, double beta1, double beta2, double eps, uint64_t step) {
  struct gw_ds_adam_c c;
  const double t = (double)(step + 1);
  c.b1 = (float)beta1;
  c.omb1 = (float)(1.0 - beta1);
  c.b2 = (float)beta2;
  c.omb2 = (float)(1.0 - beta2);
  c.eps = (float)eps;
  c.lr_t = (float)(lr * sqrt(1.0 - pow(beta2, t)) / (1.0 - pow(beta1, t)));
  return c;
}

GW_HD void gw_ds_adam(float* th, float* m, float* v, float g, const struct gw_ds_adam_c c) {
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
static inline float gw_ds_init(uint64_t seed, uint64_t index, uint32_t tensor) {
  for (uint32_t attempt = 0;; ++attempt) {
    const struct gw_u4 u = gw_philox((uint32_t)index, (uint32_t)(index >> 32), tensor, attempt, (uint32_t)seed,
                                     (uint32_t)(seed >> 32) ^ GW_TAG_DS_INIT);
    const double u1 = ((double)u.x + 1.0) * 2.3283064365386963e-10;
    const double u2 = (double)u.y * 2.3283064365386963e-10;
    const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
    if (fabs(z) <= 2.0) return (float)(0.1 * z);
  }
}
#endif
