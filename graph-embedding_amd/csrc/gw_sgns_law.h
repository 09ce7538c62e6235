// The skip-gram / negative-sampling (SGNS) training law: gensim's
// Word2Vec(sg=1, hs=0, negative=K) inner loop (the reference's
// learn_embeddings, node2vec/src/main.py:92-101) made counter-based.
//
// One definition for the kernel (gw_sgns.hip) and the host evaluation
// (gw_sgns_host.cpp, device = -1): every draw and every fp32 operation below
// is compiled into both, with -ffp-contract=off on both sides, so the two
// agree bit for bit when the kernel runs one wave (concurrency = 1).
//
// Order of the law: epochs, walks, kept positions, pairs, targets, all
// ascending.  A row of `pitch` = 4*ceil(dim/4) floats (zero padded) is dealt
// to 64 lanes in 16 B chunks: chunk q = c*64 + lane (c ascending) holds the
// elements 4q..4q+3.  A dot product is each lane's sum over its chunks in
// that order (p = p + a*b, one rounding per multiply and per add), then the
// butterfly p[l] = p[l] + p[l ^ o] for o = 32, 16, 8, 4, 2, 1 (every lane
// ends with the same bits).  The keying is documented in graphwalk.h.
#pragma once
#include "gw_philox.h"

#define GW_TAG_SGNS_TOK 0x73675430u   // "sgT0": subsampling + window draw of a token
#define GW_TAG_SGNS_NEG 0x73674E30u   // "sgN0": negative draws
#define GW_TAG_SGNS_INIT 0x73674930u  // "sgI0": initial syn0

#define GW_SGNS_LANES 64
#define GW_SGNS_MAX_DIM 1024
#define GW_SGNS_MAX_WINDOW 1023    // pair slots 0..2*window fit 11 bits
#define GW_SGNS_MAX_NEG 511        // negative slots fit 9 bits
#define GW_SGNS_MAX_EPOCHS 4096    // epoch index fits 12 bits
#define GW_SGNS_MAX_POS (1 << 20)  // walk positions (walk_len) fit 20 bits
#define GW_SGNS_EXP_SIZE 1000
#define GW_SGNS_MAX_EXP 6.0f
#define GW_SGNS_EXP_SCALE 83.33333587646484375f  // (float)(1000.0 / 12.0)

// x = subsampling word (token kept iff gw_sgns_keep(x, keep_thr[id])),
// y = window word (b = y % window)
GW_HD struct gw_u4 gw_sgns_tok_draw(uint64_t seed, uint32_t epoch, uint64_t walk, uint32_t pos) {
  return gw_philox((uint32_t)walk, (uint32_t)(walk >> 32), pos, epoch, (uint32_t)seed,
                   (uint32_t)(seed >> 32) ^ GW_TAG_SGNS_TOK);
}
GW_HD bool gw_sgns_keep(uint32_t x, uint32_t thr) { return x < thr || thr == 0xFFFFFFFFu; }

// negative `k` of pair slot `slot` of the centre token at walk position `pos`
GW_HD int32_t gw_sgns_neg_draw(uint64_t seed, uint32_t epoch, uint64_t walk, uint32_t pos, uint32_t slot, uint32_t k,
                               uint32_t n, const int32_t* J, const uint32_t* thr) {
  const struct gw_u4 u = gw_philox((uint32_t)walk, (uint32_t)(walk >> 32), pos, (epoch << 20) | (slot << 9) | k,
                                   (uint32_t)seed, (uint32_t)(seed >> 32) ^ GW_TAG_SGNS_NEG);
  const uint32_t c = (uint32_t)(((uint64_t)u.x * (uint64_t)n) >> 32);
  return u.y < thr[c] ? (int32_t)c : J[c];
}

GW_HD float gw_sgns_init(uint64_t seed, uint32_t v, uint32_t d, int dim) {
  const struct gw_u4 u = gw_philox(v, 0u, d, 0u, (uint32_t)seed, (uint32_t)(seed >> 32) ^ GW_TAG_SGNS_INIT);
  return (float)((gw_u01(u.x) - 0.5) / (double)dim);
}

// learning rate of walk w of epoch e (fp64, then one cast)
GW_HD float gw_sgns_alpha(double alpha0, double min_alpha, int64_t e, int64_t w, int64_t epochs, int64_t nwalks) {
  const double prog = (double)(e * nwalks + w) / (double)(epochs * nwalks);
  return (float)(alpha0 - (alpha0 - min_alpha) * prog);
}

// g of one target from its dot product f; false = skipped (|f| >= MAX_EXP,
// as gensim; a NaN is skipped too)
GW_HD bool gw_sgns_grad(float f, float label, float alpha, const float* expt, float* g) {
  if (!(f > -GW_SGNS_MAX_EXP && f < GW_SGNS_MAX_EXP)) return false;
  int idx = (int)((f + GW_SGNS_MAX_EXP) * GW_SGNS_EXP_SCALE);
  if (idx > GW_SGNS_EXP_SIZE - 1) idx = GW_SGNS_EXP_SIZE - 1;
  *g = (label - expt[idx]) * alpha;
  return true;
}

GW_HD float gw_sgns_fma2(float acc, float a, float b) {  // acc + a*b, two roundings
  const float m = a * b;
  return acc + m;
}
