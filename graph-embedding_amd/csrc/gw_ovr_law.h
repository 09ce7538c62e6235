// The one-vs-rest scoring law: the reference's classify.scoring
// (node2vec/src/classify.py, DeepSim/src/classify.py: TopKRanker over
// OneVsRestClassifier(LogisticRegression(penalty='l2')), f1_score) given one
// fp64 order.
//
// One definition for the kernels (gw_ovr.hip) and the host evaluation
// (gw_ovr_host.cpp, device = -1).  Both sides compile this source with
// -ffp-contract=off; every fused multiply-add below is an explicit fma, every
// other operation rounds once, only + - * /, sqrt and gw_ovr_exp are used (no
// libm on either side), and no order depends on launch geometry, so the two
// agree bit for bit.
//
// Problem, per label c over the training rows T (x~ = (x, 1), y in {0, 1}):
//   f_c(w) = 1/2 w.w + C * sum_i log(1 + exp(-s_i w.x~_i)),  s_i = 2 y_i - 1
//   grad   = w + C * sum_i (sigma(z_i) - y_i) x~_i,           z_i = w.x~_i
//   H v    = v + C * sum_i D_i (x~_i.v) x~_i,                 D_i = sigma(z_i)(1 - sigma(z_i))
// A label with no positive or no negative training row is not fitted
// (GW_OVR_CONST_NEG / GW_OVR_CONST_POS, decision value -inf / +inf).
//
// Solver: Newton-CG from w = 0, every label its own state machine
// (gw_ovr_label_step) fed by shared passes over the gathered rows.  A pass
// computes, for every label that still runs, q = sum_i coef_i x~_i with
//   GW_OVR_MODE_GRAD  t_i = x~_i.wt (the trial point), z_i := t_i, D_i := its D,
//                     coef_i = sigma(t_i) - y_i              -> grad = wt + C q
//   GW_OVR_MODE_HV    t_i = x~_i.p (the CG direction), coef_i = D_i t_i -> H p = p + C q
// z and D stay in memory between passes.  A Newton step: CG on H s = -g from
// s = 0 until |r| <= GW_OVR_CG_TOL |g| or max_cg products, then the trial
// wt = w + alpha s, alpha = 1, 1/2, 1/4, ... until |grad(wt)| < |grad(w)|.
// The merit is the gradient norm, not f, so that no logarithm is needed:
// d/dalpha |grad(w + alpha s)|^2 at 0 is 2 g.H s = 2 g.(r - g) <= -1.8 |g|^2,
// so a small enough step is accepted, and with the unique minimiser a
// monotone |grad| -> 0 is convergence.  More than GW_OVR_MAX_HALVINGS
// halvings, or max_newton accepted steps without meeting the stop, end the
// label as GW_OVR_NOT_CONVERGED.  Stop: |grad(w)| <= gtol |grad(0)|.
// A finished label is frozen: later passes skip it, and since no label's
// arithmetic reads another's, fitting a label alone gives the same bits.
//
// Sum orders (RB = GW_OVR_RB rows per block, d = dim):
//   t_i       = fma(x_ij, v_j, t) over j = 0 .. d-1 ascending from +0, then t + v_d
//   part[b][j]= fma(coef_i, x_ij, part) over the rows i of block b ascending from +0  (j < d)
//   part[b][d]= part + coef_i over the rows i of block b ascending from +0
//   q[j]      = q + part[b][j] over b ascending from +0
//   dots      = fma(a_j, b_j, acc) over j = 0 .. d ascending from +0
// Features are the caller's fp32 widened; everything else is fp64.
//
// Prediction: a row with k true labels gets the k labels of largest decision
// value z = w.x~ (order above); of equal values the larger label index wins,
// which is what argsort()[-k:] gives under a stable sort (numpy's default sort
// promises no order among equals).  Label l is predicted iff
//   #{m : z_m > z_l or (z_m == z_l and m > l)} < k.
// Counts per label: tp, fp, fn over the scored rows.
//
// Shuffle: order[i] = gw_feistel_perm(i, n, k0 = seed low ^ shuffle,
// k1 = seed high ^ "ovS0", tweak = shuffle high word).
#pragma once
#include <stdint.h>

#include "../../include/graphwalk.h"
#include "gw_philox.h"

#define GW_TAG_OVR_SHUFFLE 0x6F765330u  // "ovS0"

#define GW_OVR_RB 64            // rows per partial block of the law
#define GW_OVR_CG_TOL 0.1       // inexact CG: |r| <= 0.1 |g|
#define GW_OVR_MAX_HALVINGS 30  // alpha down to 2^-30
#define GW_OVR_MAX_DIM 1024     // device path
#define GW_OVR_MAX_LABELS 1024  // device path

#define GW_OVR_MODE_IDLE 0
#define GW_OVR_MODE_GRAD 1
#define GW_OVR_MODE_HV 2

// label states GW_OVR_CONST_NEG .. GW_OVR_NOT_CONVERGED: include/graphwalk.h
#define GW_OVR_RUNNING 4  // internal: never exported

// correctly rounded on both sides (the device expands sqrt and / to IEEE sequences: no fast-math flag is given)
#define GW_OVR_FMA(a, b, c) __builtin_fma((a), (b), (c))
#define GW_OVR_SQRT(a) __builtin_sqrt(a)

GW_HD uint64_t gw_ovr_perm(uint64_t seed, uint64_t shuffle, uint64_t i, uint64_t n) {
  return gw_feistel_perm(i, n, (uint32_t)seed ^ (uint32_t)shuffle, (uint32_t)(seed >> 32) ^ GW_TAG_OVR_SHUFFLE,
                         (uint32_t)(shuffle >> 32));
}

GW_HD uint64_t gw_ovr_d2u(double x) {
  uint64_t u;
  __builtin_memcpy(&u, &x, 8);
  return u;
}
GW_HD double gw_ovr_u2d(uint64_t u) {
  double x;
  __builtin_memcpy(&x, &u, 8);
  return x;
}

// exp(x) for x <= 0: n = round(x * log2 e), r = x - n * ln 2 (two fma), the degree-13
// Taylor polynomial in Horner form (|r| <= 0.35: the first dropped term is below 4e-18),
// then 2^n added to the exponent field.  x < -700 (and NaN) gives +0.
GW_HD double gw_ovr_exp(double x) {
  if (!(x >= -700.0)) return 0.0;
  const double t = x * 1.4426950408889634;
  const int n = (int)(t - 0.5);  // t <= 0: truncation rounds half away from zero
  const double nf = (double)n;
  double r = GW_OVR_FMA(nf, -6.93147180369123816490e-01, x);
  r = GW_OVR_FMA(nf, -1.90821492927058770002e-10, r);
  double p = 1.0 / 6227020800.0;
  p = GW_OVR_FMA(p, r, 1.0 / 479001600.0);
  p = GW_OVR_FMA(p, r, 1.0 / 39916800.0);
  p = GW_OVR_FMA(p, r, 1.0 / 3628800.0);
  p = GW_OVR_FMA(p, r, 1.0 / 362880.0);
  p = GW_OVR_FMA(p, r, 1.0 / 40320.0);
  p = GW_OVR_FMA(p, r, 1.0 / 5040.0);
  p = GW_OVR_FMA(p, r, 1.0 / 720.0);
  p = GW_OVR_FMA(p, r, 1.0 / 120.0);
  p = GW_OVR_FMA(p, r, 1.0 / 24.0);
  p = GW_OVR_FMA(p, r, 1.0 / 6.0);
  p = GW_OVR_FMA(p, r, 0.5);
  p = GW_OVR_FMA(p, r, 1.0);
  p = GW_OVR_FMA(p, r, 1.0);
  return gw_ovr_u2d(gw_ovr_d2u(p) + ((uint64_t)(int64_t)n << 52));
}

// sigma(z) and D = sigma (1 - sigma) from e = exp(-|z|): no cancellation at either end
GW_HD void gw_ovr_sigma(double z, double* sig, double* D) {
  const double a = z < 0.0 ? z : -z;
  const double e = gw_ovr_exp(a);
  const double o = 1.0 + e;
  const double hi = 1.0 / o, lo = e / o;
  *sig = z < 0.0 ? lo : hi;
  *D = lo / o;
}

// the pass's coefficient of one (row, label): see the modes above
GW_HD double gw_ovr_coef(int mode, double t, double y, double* z, double* D) {
  if (mode == GW_OVR_MODE_GRAD) {
    double sig, dd;
    gw_ovr_sigma(t, &sig, &dd);
    *z = t;
    *D = dd;
    return sig - y;
  }
  return *D * t;
}

GW_HD double gw_ovr_dot(const double* a, const double* b, int D) {
  double acc = 0.0;
  for (int j = 0; j < D; ++j) acc = GW_OVR_FMA(a[j], b[j], acc);
  return acc;
}

// per-label solver state; the vectors are D = dim + 1 doubles each
struct gw_ovr_label {
  int32_t mode;      // what the next pass computes for this label
  int32_t state;     // GW_OVR_*
  int32_t newton;    // accepted Newton steps
  int32_t cg;        // products of the running CG
  int32_t halvings;  // of the running trial
  int32_t started;   // grad(0) seen
  double gnorm0, gnorm, rr, alpha;
};

struct gw_ovr_consts {
  double C, gtol;
  int32_t max_newton, max_cg;
};

GW_HD void gw_ovr_label_init(struct gw_ovr_label* s, int state) {
  s->state = state;
  s->mode = state == GW_OVR_RUNNING ? GW_OVR_MODE_GRAD : GW_OVR_MODE_IDLE;
  s->newton = s->cg = s->halvings = s->started = 0;
  s->gnorm0 = s->gnorm = s->rr = 0.0;
  s->alpha = 1.0;
}

// One transition of a running label after a pass gave q (D doubles).  w, wt (what the next
// GW_OVR_MODE_GRAD pass reads), g, sv (the CG solution), r, p (what the next GW_OVR_MODE_HV pass reads).
GW_HD void gw_ovr_label_step(struct gw_ovr_label* s, const struct gw_ovr_consts k, int D, const double* q, double* w,
                             double* wt, double* g, double* sv, double* r, double* p) {
  if (s->mode == GW_OVR_MODE_GRAD) {
    // gradient at the trial point, into r (free while no CG runs)
    for (int j = 0; j < D; ++j) r[j] = GW_OVR_FMA(k.C, q[j], wt[j]);
    const double gn = GW_OVR_SQRT(gw_ovr_dot(r, r, D));
    if (!s->started) {
      s->started = 1;
      s->gnorm0 = gn;
    } else if (!(gn < s->gnorm)) {
      if (++s->halvings > GW_OVR_MAX_HALVINGS) {
        s->state = GW_OVR_NOT_CONVERGED;
        s->mode = GW_OVR_MODE_IDLE;
        return;
      }
      s->alpha = s->alpha * 0.5;
      for (int j = 0; j < D; ++j) wt[j] = GW_OVR_FMA(s->alpha, sv[j], w[j]);
      return;
    } else {
      s->newton += 1;
    }
    for (int j = 0; j < D; ++j) {
      w[j] = wt[j];
      g[j] = r[j];
    }
    s->gnorm = gn;
    if (gn <= k.gtol * s->gnorm0) {
      s->state = GW_OVR_FITTED;
      s->mode = GW_OVR_MODE_IDLE;
      return;
    }
    if (s->newton >= k.max_newton) {
      s->state = GW_OVR_NOT_CONVERGED;
      s->mode = GW_OVR_MODE_IDLE;
      return;
    }
    for (int j = 0; j < D; ++j) {
      sv[j] = 0.0;
      r[j] = -g[j];
      p[j] = r[j];
    }
    s->rr = gw_ovr_dot(r, r, D);
    s->cg = 0;
    s->mode = GW_OVR_MODE_HV;
    return;
  }
  // GW_OVR_MODE_HV: q = X~' D X~ p; H p into wt (free while the CG runs)
  for (int j = 0; j < D; ++j) wt[j] = GW_OVR_FMA(k.C, q[j], p[j]);
  const double pHp = gw_ovr_dot(p, wt, D);
  const double a = s->rr / pHp;
  for (int j = 0; j < D; ++j) {
    sv[j] = GW_OVR_FMA(a, p[j], sv[j]);
    r[j] = GW_OVR_FMA(-a, wt[j], r[j]);
  }
  const double rr = gw_ovr_dot(r, r, D);
  s->cg += 1;
  if (GW_OVR_SQRT(rr) <= GW_OVR_CG_TOL * s->gnorm || s->cg >= k.max_cg) {
    s->alpha = 1.0;
    s->halvings = 0;
    for (int j = 0; j < D; ++j) wt[j] = GW_OVR_FMA(s->alpha, sv[j], w[j]);
    s->mode = GW_OVR_MODE_GRAD;
    return;
  }
  const double beta = rr / s->rr;
  for (int j = 0; j < D; ++j) p[j] = GW_OVR_FMA(beta, p[j], r[j]);
  s->rr = rr;
}

// is label l among the k largest of z[0 .. L)?  (ties to the larger index)
GW_HD int gw_ovr_predicted(const double* z, int L, int l, int k) {
  const double zl = z[l];
  int rank = 0;
  for (int m = 0; m < L; ++m) rank += (z[m] > zl || (z[m] == zl && m > l)) ? 1 : 0;
  return rank < k;
}
