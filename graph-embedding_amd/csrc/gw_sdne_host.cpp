// SDNE trainer: C ABI, argument checks, initial values and the host evaluation
// of the training law (device = -1).  The law itself is gw_sdne_law.h; the
// kernels are gw_sdne.hip.
//
// This file depends on nothing but the C++ library, so that it also builds as
// a plain host program (-DGW_SDNE_HOST_ONLY: no device path) for sanitizer
// runs (host/sdne_host_check.cpp).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>

#include "gw_sdne_internal.h"
#include "gw_sdne_law.h"
#include "gw_trainer_fail.h"

static thread_local std::string g_sdne_err;

int gw_sdne_fail(gw_sdne* m, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  gw_trainer_vfail(m ? &m->err : nullptr, &g_sdne_err, code, fmt, ap);
  va_end(ap);
  return code;
}

#ifdef GW_SDNE_HOST_ONLY
static int no_dev(gw_sdne* m) { return gw_sdne_fail(m, GW_ERR_DEVICE, "built without the device path"); }
int gw_sdne_dev_alloc(gw_sdne* m, const std::vector<float>*) { return no_dev(m); }
void gw_sdne_dev_free(gw_sdne*) {}
int gw_sdne_dev_set_rows(gw_sdne* m) { return no_dev(m); }
int gw_sdne_dev_train(gw_sdne* m, int64_t, int64_t, double*, void*) { return no_dev(m); }
int gw_sdne_dev_gradients(gw_sdne* m, int64_t, float* const*) { return no_dev(m); }
int gw_sdne_dev_batch_rows(gw_sdne* m, int64_t, int64_t*) { return no_dev(m); }
int gw_sdne_dev_encode(gw_sdne* m, int64_t, int64_t, float*) { return no_dev(m); }
int gw_sdne_dev_export(gw_sdne* m, float* const*, float* const*, float* const*) { return no_dev(m); }
float* gw_sdne_dev_vectors(gw_sdne* m) { return no_dev(m), nullptr; }
#endif

extern "C" const char* gw_sdne_last_error(const gw_sdne* m) { return m ? m->err.c_str() : g_sdne_err.c_str(); }

extern "C" int gw_sdne_create(int device, const gw_sdne_params_t* params, gw_sdne** out) {
  if (!out) return gw_sdne_fail(nullptr, GW_ERR_INVALID, "NULL out");
  *out = nullptr;
  gw_sdne_params_t p;
  memset(&p, 0, sizeof p);
  p.units[1] = 400;
  p.units[2] = 100;
  p.units[3] = 300;
  p.batch = 100;
  p.learning_rate = 0.01;
  p.beta1 = 0.9;
  p.beta2 = 0.999;
  p.epsilon = 1e-8;
  p.weight_decay = 0.1;
  p.kl_weight = 0.1;
  p.kl_target = 0.005;
  p.nonzero_weight = 1.0;
  if (params) {
    if (params->struct_size < (int32_t)sizeof(int32_t))
      return gw_sdne_fail(nullptr, GW_ERR_INVALID, "gw_sdne_params_t.struct_size %d", (int)params->struct_size);
    memcpy(&p, params, std::min((size_t)params->struct_size, sizeof p));
  }
  p.struct_size = (int32_t)sizeof p;
  if (p.units[4] == 0) p.units[4] = p.units[0];
  for (int i = 0; i < 5; ++i)
    if (p.units[i] < 1) return gw_sdne_fail(nullptr, GW_ERR_INVALID, "units[%d] = %d must be positive", i, p.units[i]);
  if (p.units[4] != p.units[0])
    return gw_sdne_fail(nullptr, GW_ERR_INVALID, "units[4] = %d must equal units[0] = %d (an autoencoder)", p.units[4],
                        p.units[0]);
  if (p.batch < 1 || p.batch > (1 << 20)) return gw_sdne_fail(nullptr, GW_ERR_INVALID, "batch %d", p.batch);
  if (!(p.learning_rate > 0.0) || !isfinite(p.learning_rate) || !(p.beta1 >= 0.0 && p.beta1 < 1.0) ||
      !(p.beta2 >= 0.0 && p.beta2 < 1.0) || !(p.epsilon > 0.0) || !isfinite(p.weight_decay) || !isfinite(p.kl_weight) ||
      !(p.kl_target > 0.0 && p.kl_target < 1.0))
    return gw_sdne_fail(nullptr, GW_ERR_INVALID, "bad learning_rate / beta / epsilon / weight_decay / kl_weight / kl_target");
  if (!isfinite(p.nonzero_weight) || !(p.nonzero_weight > 0.0))
    return gw_sdne_fail(nullptr, GW_ERR_INVALID, "nonzero_weight %g must be finite and positive", p.nonzero_weight);
  if (!isfinite(p.first_order) || !(p.first_order >= 0.0))
    return gw_sdne_fail(nullptr, GW_ERR_INVALID, "first_order %g must be finite and not negative", p.first_order);
  if (p.shuffle != 0 && p.shuffle != 1)
    return gw_sdne_fail(nullptr, GW_ERR_INVALID, "shuffle %d must be 0 or 1", p.shuffle);
  if (device < -1) return gw_sdne_fail(nullptr, GW_ERR_INVALID, "device %d", device);
  if (device >= 0) {
    if (p.units[1] > GW_SDNE_MAX_HIDDEN || p.units[2] > GW_SDNE_MAX_HIDDEN || p.units[3] > GW_SDNE_MAX_HIDDEN)
      return gw_sdne_fail(nullptr, GW_ERR_UNSUPPORTED,
                          "hidden widths %d, %d, %d: the kernels take at most %d (device = -1 takes any)", p.units[1],
                          p.units[2], p.units[3], GW_SDNE_MAX_HIDDEN);
    if (p.batch > GW_SDNE_MAX_BATCH)
      return gw_sdne_fail(nullptr, GW_ERR_UNSUPPORTED, "batch %d: the kernels take at most %d (device = -1 takes any)",
                          p.batch, GW_SDNE_MAX_BATCH);
  }
  gw_sdne* m = new (std::nothrow) gw_sdne();
  if (!m) return gw_sdne_fail(nullptr, GW_ERR_NOMEM, "out of memory");
  m->device = device;
  m->p = p;
  for (int i = 0; i < 5; ++i) m->u[i] = p.units[i];
  m->B = p.batch;
  std::vector<float> init[8];
  for (int t = 0; t < 8; ++t) {
    init[t].assign(gw_sdne_numel(m, t), 0.0f);
    if (!(t & 1))
      for (size_t i = 0; i < init[t].size(); ++i) init[t][i] = gw_sdne_init(p.seed, (uint64_t)i, (uint32_t)t);
  }
  if (device >= 0) {
    const int rc = gw_sdne_dev_alloc(m, init);
    if (rc != GW_OK) {
      g_sdne_err = m->err;
      gw_sdne_dev_free(m);
      delete m;
      return rc;
    }
  } else {
    for (int t = 0; t < 8; ++t) {
      m->par[t].swap(init[t]);
      m->am[t].assign(m->par[t].size(), 0.0f);
      m->av[t].assign(m->par[t].size(), 0.0f);
    }
  }
  *out = m;
  return GW_OK;
}

extern "C" int gw_sdne_free(gw_sdne* m) {
  if (!m) return GW_OK;
  if (m->device >= 0) gw_sdne_dev_free(m);
  delete m;
  return GW_OK;
}

static int rows_set(gw_sdne* m) {
  if (m->device >= 0) {
    const int rc = gw_sdne_dev_set_rows(m);
    if (rc != GW_OK) return rc;
  } else {
    m->enc.assign((size_t)m->N * (size_t)m->u[2], 0.0f);
  }
  m->have_rows = true;
  return GW_OK;
}

// the first-order term reads a_ij = x_i[row(j)]: the rows are a square matrix
static bool square_ok(gw_sdne* m, int64_t n) {
  if (!(m->p.first_order > 0.0) || n == m->u[0]) return true;
  gw_sdne_fail(m, GW_ERR_INVALID,
               "first_order > 0: the first-order term reads the adjacency, so the %lld rows must equal the row "
               "width %d",
               (long long)n, m->u[0]);
  return false;
}

extern "C" int gw_sdne_set_rows_dense(gw_sdne* m, const float* rows, int64_t n, int64_t pitch) {
  if (!m) return gw_sdne_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!rows || n < 1 || pitch < m->u[0]) return gw_sdne_fail(m, GW_ERR_INVALID, "bad row arguments");
  if (n < m->B) return gw_sdne_fail(m, GW_ERR_INVALID, "%lld rows, fewer than the batch of %d", (long long)n, m->B);
  if (!square_ok(m, n)) return GW_ERR_INVALID;
  m->have_rows = false;
  m->sparse = false;
  m->rows = rows;
  m->pitch = pitch;
  m->N = n;
  m->offs.clear();
  m->cols.clear();
  m->vals.clear();
  return rows_set(m);
}

extern "C" int gw_sdne_set_rows_csr(gw_sdne* m, const int64_t* offsets, const int32_t* cols, const float* vals,
                                    int64_t n) {
  if (!m) return gw_sdne_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!offsets || n < 1 || offsets[0] != 0) return gw_sdne_fail(m, GW_ERR_INVALID, "bad row arguments");
  if (n < m->B) return gw_sdne_fail(m, GW_ERR_INVALID, "%lld rows, fewer than the batch of %d", (long long)n, m->B);
  if (!square_ok(m, n)) return GW_ERR_INVALID;
  for (int64_t r = 0; r < n; ++r)
    if (offsets[r + 1] < offsets[r]) return gw_sdne_fail(m, GW_ERR_INVALID, "offsets decrease at row %lld", (long long)r);
  const int64_t nnz = offsets[n];
  if (nnz > 0 && !cols) return gw_sdne_fail(m, GW_ERR_INVALID, "NULL cols");
  std::vector<int32_t> row;
  for (int64_t r = 0; r < n; ++r) {
    row.assign(cols + offsets[r], cols + offsets[r + 1]);
    for (const int32_t c : row)
      if (c < 0 || c >= m->u[0])
        return gw_sdne_fail(m, GW_ERR_RANGE, "row %lld: column %d outside [0, %d)", (long long)r, (int)c, m->u[0]);
    std::sort(row.begin(), row.end());
    for (size_t e = 1; e < row.size(); ++e)
      if (row[e] == row[e - 1])
        return gw_sdne_fail(m, GW_ERR_INVALID, "row %lld: column %d twice", (long long)r, (int)row[e]);
  }
  m->have_rows = false;
  m->sparse = true;
  m->rows = nullptr;
  m->pitch = 0;
  m->N = n;
  m->offs.assign(offsets, offsets + n + 1);
  m->cols.assign(cols, cols + nnz);
  if (vals)
    m->vals.assign(vals, vals + nnz);
  else
    m->vals.assign((size_t)nnz, 1.0f);
  return rows_set(m);
}

static int ready(gw_sdne* m, int64_t step_begin, int64_t step_count) {
  if (!m) return gw_sdne_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->have_rows) return gw_sdne_fail(m, GW_ERR_STATE, "call gw_sdne_set_rows_dense or gw_sdne_set_rows_csr first");
  if (step_begin < 0 || step_count < 0 || step_begin > INT64_MAX - step_count)
    return gw_sdne_fail(m, GW_ERR_INVALID, "bad step range");
  return GW_OK;
}

// ---- the law on the host -------------------------------------------------------
// The chains below are explicit fmaf; where the CPU has FMA units the same functions are also compiled for them
// (fmaf is exact either way, so the bits do not depend on which one runs).
#if defined(__x86_64__) && defined(__GNUC__)
#define GW_SDNE_FMA_CLONE 1
#else
#define GW_SDNE_FMA_CLONE 0
#endif

// acc[c] = fmaf(a[k * a_ks], bm[k * ldb + c], acc[c]) for k in [k0, k1) ascending, every c in [0, n)
static inline __attribute__((always_inline)) void axpy_body(float* acc, const float* a, int64_t a_ks, const float* bm,
                                                            int64_t ldb, int64_t k0, int64_t k1, int64_t n) {
  for (int64_t k = k0; k < k1; ++k) {
    const float av = a[k * a_ks];
    const float* br = bm + k * ldb;
    for (int64_t c = 0; c < n; ++c) acc[c] = fmaf(av, br[c], acc[c]);
  }
}
// acc[i] = fmaf(a[k], w[i * ldw + k], acc[i]) for k in [k0, k1) ascending, i in [0, 8)
static inline __attribute__((always_inline)) void dot8_body(float* acc, const float* a, const float* w, int64_t ldw,
                                                            int64_t k0, int64_t k1, int ni) {
  float r[8];
  for (int i = 0; i < 8; ++i) r[i] = acc[i];
  if (ni == 8) {
    for (int64_t k = k0; k < k1; ++k)
      for (int i = 0; i < 8; ++i) r[i] = fmaf(a[k], w[i * ldw + k], r[i]);
  } else {
    for (int64_t k = k0; k < k1; ++k)
      for (int i = 0; i < ni; ++i) r[i] = fmaf(a[k], w[i * ldw + k], r[i]);
  }
  for (int i = 0; i < 8; ++i) acc[i] = r[i];
}
static void axpy_plain(float* acc, const float* a, int64_t a_ks, const float* bm, int64_t ldb, int64_t k0, int64_t k1,
                       int64_t n) {
  axpy_body(acc, a, a_ks, bm, ldb, k0, k1, n);
}
static void dot8_plain(float* acc, const float* a, const float* w, int64_t ldw, int64_t k0, int64_t k1, int ni) {
  dot8_body(acc, a, w, ldw, k0, k1, ni);
}
#if GW_SDNE_FMA_CLONE
__attribute__((target("avx2,fma"))) static void axpy_fma(float* acc, const float* a, int64_t a_ks, const float* bm,
                                                         int64_t ldb, int64_t k0, int64_t k1, int64_t n) {
  axpy_body(acc, a, a_ks, bm, ldb, k0, k1, n);
}
__attribute__((target("avx2,fma"))) static void dot8_fma(float* acc, const float* a, const float* w, int64_t ldw,
                                                         int64_t k0, int64_t k1, int ni) {
  dot8_body(acc, a, w, ldw, k0, k1, ni);
}
static bool have_fma() {
  static const bool v = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
  return v;
}
#else
static bool have_fma() { return false; }
#define axpy_fma axpy_plain
#define dot8_fma dot8_plain
#endif

// out[r][c] (r < M, c < N, row length N) = the law's product over k < K of a[r * a_rs + k * a_ks] * bm[k * N + c],
// chunk 0 starting from bias (NULL: +0)
static void product_axpy(int64_t M, int64_t N, int64_t K, const float* a, int64_t a_rs, int64_t a_ks, const float* bm,
                         const float* bias, float* out) {
  const bool fma = have_fma();
#pragma omp parallel
  {
    std::vector<float> acc((size_t)N);
#pragma omp for schedule(static)
    for (int64_t r = 0; r < M; ++r) {
      float* o = out + r * N;
      for (int64_t k0 = 0; k0 < K; k0 += GW_SDNE_KC) {
        const int64_t k1 = std::min(K, k0 + GW_SDNE_KC);
        float* dst = k0 == 0 ? o : acc.data();
        for (int64_t c = 0; c < N; ++c) dst[c] = k0 == 0 && bias ? bias[c] : 0.0f;
        (fma ? axpy_fma : axpy_plain)(dst, a + r * a_rs, a_ks, bm, N, k0, k1, N);
        if (k0 > 0)
          for (int64_t c = 0; c < N; ++c) o[c] = o[c] + acc[(size_t)c];
      }
    }
  }
}

// out[r][i] (r < M, i < I, row length I) = the law's product over k < K of a[r * K + k] * w[i * K + k], from +0
static void product_dot(int64_t M, int64_t I, int64_t K, const float* a, const float* w, float* out) {
  const bool fma = have_fma();
  const int64_t ni8 = (I + 7) / 8;
#pragma omp parallel for schedule(static) collapse(2)
  for (int64_t r = 0; r < M; ++r)
    for (int64_t ib = 0; ib < ni8; ++ib) {
      const int64_t i0 = ib * 8;
      const int ni = (int)std::min<int64_t>(8, I - i0);
      float tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int64_t k0 = 0; k0 < K; k0 += GW_SDNE_KC) {
        const int64_t k1 = std::min(K, k0 + GW_SDNE_KC);
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        (fma ? dot8_fma : dot8_plain)(acc, a + r * K, w + i0 * K, K, k0, k1, ni);
        for (int i = 0; i < ni; ++i) tot[i] = k0 == 0 ? acc[i] : tot[i] + acc[i];
      }
      for (int i = 0; i < ni; ++i) out[r * I + i0 + i] = tot[i];
    }
}

// rows ids[0..M) (NULL: row0, row0 + 1, ..) of the input as a dense [M][u0]
static void host_stage(const gw_sdne* m, const int64_t* ids, int64_t row0, int64_t M, std::vector<float>* x) {
  const int64_t u0 = m->u[0];
  x->assign((size_t)(M * u0), 0.0f);
  for (int64_t b = 0; b < M; ++b) {
    float* xr = x->data() + b * u0;
    const int64_t r = ids ? ids[b] : row0 + b;
    if (m->sparse) {
      for (int64_t e = m->offs[(size_t)r]; e < m->offs[(size_t)(r + 1)]; ++e)
        xr[m->cols[(size_t)e]] = m->vals[(size_t)e];
    } else {
      memcpy(xr, m->rows + r * m->pitch, (size_t)u0 * sizeof(float));
    }
  }
}

static void host_batch_rows(const gw_sdne* m, uint64_t t, int64_t* ids) {
  for (int64_t i = 0; i < m->B; ++i) ids[i] = gw_sdne_row(m->p.seed, m->p.shuffle, m->N, m->B, t, i);
}

static void relu_of(const std::vector<float>& z, std::vector<float>* h) {
  h->resize(z.size());
  for (size_t i = 0; i < z.size(); ++i) (*h)[i] = z[i] > 0.0f ? z[i] : 0.0f;
}

struct HostAct {
  std::vector<float> x, z1, h1, z2, h2, z3, h3, y;
};

// z1, h1, z2 of M staged rows (the encoder); with `full` the rest of the forward pass
static void host_forward(const gw_sdne* m, int64_t M, bool full, HostAct* A) {
  const int* u = m->u;
  A->z1.resize((size_t)(M * u[1]));
  product_axpy(M, u[1], u[0], A->x.data(), u[0], 1, m->par[0].data(), m->par[1].data(), A->z1.data());
  relu_of(A->z1, &A->h1);
  A->z2.resize((size_t)(M * u[2]));
  product_axpy(M, u[2], u[1], A->h1.data(), u[1], 1, m->par[2].data(), m->par[3].data(), A->z2.data());
  if (!full) return;
  relu_of(A->z2, &A->h2);
  A->z3.resize((size_t)(M * u[3]));
  product_axpy(M, u[3], u[2], A->h2.data(), u[2], 1, m->par[4].data(), m->par[5].data(), A->z3.data());
  relu_of(A->z3, &A->h3);
  A->y.resize((size_t)(M * u[4]));
  product_axpy(M, u[4], u[3], A->h3.data(), u[3], 1, m->par[6].data(), m->par[7].data(), A->y.data());
}

// one step: the gradient of step t's batch at the current parameters into g[8] (resized here) and its loss; the
// parameters are not touched
static double host_gradient(const gw_sdne* m, uint64_t t, std::vector<float> g[8], bool want_loss) {
  const int* u = m->u;
  const int64_t B = m->B;
  const float wd = (float)m->p.weight_decay;
  const float bf = (float)m->p.nonzero_weight;
  const float bw = bf * bf;
  const double alpha = m->p.first_order;
  std::vector<int64_t> ids((size_t)B);
  host_batch_rows(m, t, ids.data());
  HostAct A;
  host_stage(m, ids.data(), 0, B, &A.x);
  host_forward(m, B, true, &A);
  const float Bf = (float)B;
  // the first-order term: S[i][j] = a_ij + a_ji, g1 = coef * (the chain over j ascending)
  std::vector<float> S, g1;
  if (alpha > 0.0) {
    const int64_t u0 = u[0], u2 = u[2];
    S.resize((size_t)(B * B));
    g1.resize((size_t)(B * u2));
    for (int64_t i = 0; i < B; ++i)
      for (int64_t j = 0; j < B; ++j)
        S[(size_t)(i * B + j)] = A.x[(size_t)(i * u0 + ids[(size_t)j])] + A.x[(size_t)(j * u0 + ids[(size_t)i])];
    const float coef = (float)(2.0 * alpha / (double)B);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < B; ++i) {
      const float* zi = A.z2.data() + i * u2;
      float* gi = g1.data() + i * u2;
      for (int64_t c = 0; c < u2; ++c) gi[c] = 0.0f;
      for (int64_t j = 0; j < B; ++j) {
        const float s = S[(size_t)(i * B + j)];
        const float* zj = A.z2.data() + j * u2;
        for (int64_t c = 0; c < u2; ++c) {
          const float d = zi[c] - zj[c];
          gi[c] = fmaf(s, d, gi[c]);
        }
      }
      for (int64_t c = 0; c < u2; ++c) gi[c] = coef * gi[c];
    }
  }
  std::vector<float> dz4((size_t)(B * u[4])), dz3((size_t)(B * u[3])), dz2((size_t)(B * u[2])), dz1((size_t)(B * u[1]));
  for (size_t i = 0; i < dz4.size(); ++i) dz4[i] = gw_sdne_dz4(A.y[i], A.x[i], bw, Bf);
  float qs = 0.0f;
  for (int64_t b = 0; b < B; ++b) {
    float rs = 0.0f;
    for (int64_t j = 0; j < u[2]; ++j) rs = rs + A.h2[(size_t)(b * u[2] + j)];
    qs = qs + rs;
  }
  const float count = (float)(B * (int64_t)u[2]);
  const float q = qs / count;
  const float klg = gw_sdne_kl_grad(q, (float)m->p.kl_target, (float)m->p.kl_weight, count);
  product_dot(B, u[3], u[4], dz4.data(), m->par[6].data(), dz3.data());
  for (size_t i = 0; i < dz3.size(); ++i) dz3[i] = A.z3[i] > 0.0f ? dz3[i] : 0.0f;
  product_dot(B, u[2], u[3], dz3.data(), m->par[4].data(), dz2.data());
  for (size_t i = 0; i < dz2.size(); ++i) {
    const float v = dz2[i] + klg;
    dz2[i] = A.z2[i] > 0.0f ? v : 0.0f;
  }
  if (alpha > 0.0)
    for (size_t i = 0; i < dz2.size(); ++i) dz2[i] = dz2[i] + g1[i];
  product_dot(B, u[1], u[2], dz2.data(), m->par[2].data(), dz1.data());
  for (size_t i = 0; i < dz1.size(); ++i) dz1[i] = A.z1[i] > 0.0f ? dz1[i] : 0.0f;
  const float* in[4] = {A.x.data(), A.h1.data(), A.h2.data(), A.h3.data()};
  const float* dz[4] = {dz1.data(), dz2.data(), dz3.data(), dz4.data()};
  for (int l = 0; l < 4; ++l) {
    const int64_t I = u[l], J = u[l + 1];
    std::vector<float>& gw = g[2 * l];
    std::vector<float>& gb = g[2 * l + 1];
    gw.resize((size_t)(I * J));
    gb.resize((size_t)J);
    product_axpy(I, J, B, in[l], 1, I, dz[l], nullptr, gw.data());
    const float* W = m->par[2 * l].data();
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < I * J; ++e) gw[(size_t)e] = fmaf(wd, W[e], gw[(size_t)e]);
    for (int64_t j = 0; j < J; ++j) {
      float s = 0.0f;
      for (int64_t b = 0; b < B; ++b) s = s + dz[l][b * J + j];
      gb[(size_t)j] = fmaf(wd, m->par[2 * l + 1][(size_t)j], s);
    }
  }
  if (!want_loss) return 0.0;
  // the reported loss (fp64, not part of the bit law)
  double rec = 0.0;
  for (size_t i = 0; i < A.y.size(); ++i) {
    const double d = (double)A.y[i] - (double)A.x[i];
    rec += (A.x[i] != 0.0f ? (double)bw : 1.0) * (d * d);
  }
  double l1 = 0.0;
  if (alpha > 0.0)
    for (int64_t i = 0; i < B; ++i)
      for (int64_t j = 0; j < B; ++j) {
        const double a = (double)A.x[(size_t)(i * u[0] + ids[(size_t)j])];
        if (a == 0.0) continue;
        double s = 0.0;
        for (int64_t c = 0; c < u[2]; ++c) {
          const double d = (double)A.z2[(size_t)(i * u[2] + c)] - (double)A.z2[(size_t)(j * u[2] + c)];
          s += d * d;
        }
        l1 += a * s;
      }
  double reg = 0.0;
  for (int t8 = 0; t8 < 8; ++t8) {
    double s = 0.0;
    for (const float v : m->par[t8]) s += (double)v * (double)v;
    reg += s;
  }
  const double p = m->p.kl_target, qd = (double)q;
  const double kl = p * log(p / (qd + 1e-8)) + (1.0 - p) * log((1.0 - p) / (1.0 - qd + 1e-8));
  return rec / 2.0 / (double)B + m->p.weight_decay * reg / 2.0 + m->p.kl_weight * kl + alpha / (double)B * l1;
}

static int host_train(gw_sdne* m, int64_t step_begin, int64_t step_count, double* loss_out) {
  std::vector<float> g[8];
  for (int64_t i = 0; i < step_count; ++i) {
    const uint64_t t = (uint64_t)(step_begin + i);
    const double loss = host_gradient(m, t, g, loss_out != nullptr);
    if (loss_out) loss_out[i] = loss;
    const gw_sdne_adam_c c = gw_sdne_adam_consts(m->p.learning_rate, m->p.beta1, m->p.beta2, m->p.epsilon, t);
    for (int t8 = 0; t8 < 8; ++t8) {
      float* th = m->par[t8].data();
      float* am = m->am[t8].data();
      float* av = m->av[t8].data();
      const float* gg = g[t8].data();
      const int64_t n = (int64_t)g[t8].size();
#pragma omp parallel for schedule(static)
      for (int64_t e = 0; e < n; ++e) gw_sdne_adam(&th[e], &am[e], &av[e], gg[e], c);
    }
  }
  return GW_OK;
}

extern "C" int gw_sdne_train(gw_sdne* m, int64_t step_begin, int64_t step_count, double* loss_out, void* stream) {
  const int rc = ready(m, step_begin, step_count);
  if (rc != GW_OK) return rc;
  if (step_count == 0) return GW_OK;
  return m->device < 0 ? host_train(m, step_begin, step_count, loss_out)
                       : gw_sdne_dev_train(m, step_begin, step_count, loss_out, stream);
}

extern "C" int gw_sdne_gradients(gw_sdne* m, int64_t step, float* const grads[8]) {
  const int rc = ready(m, step, 0);
  if (rc != GW_OK) return rc;
  if (!grads) return gw_sdne_fail(m, GW_ERR_INVALID, "NULL grads");
  if (m->device >= 0) return gw_sdne_dev_gradients(m, step, grads);
  std::vector<float> g[8];
  host_gradient(m, (uint64_t)step, g, false);
  for (int t = 0; t < 8; ++t)
    if (grads[t]) memcpy(grads[t], g[t].data(), g[t].size() * sizeof(float));
  return GW_OK;
}

extern "C" int gw_sdne_batch_rows(gw_sdne* m, int64_t step, int64_t* rows) {
  const int rc = ready(m, step, 0);
  if (rc != GW_OK) return rc;
  if (!rows) return gw_sdne_fail(m, GW_ERR_INVALID, "NULL rows");
  if (m->device >= 0) return gw_sdne_dev_batch_rows(m, step, rows);
  host_batch_rows(m, (uint64_t)step, rows);
  return GW_OK;
}

extern "C" int gw_sdne_encode(gw_sdne* m, int64_t row_begin, int64_t row_count, float* out) {
  const int rc = ready(m, 0, 0);
  if (rc != GW_OK) return rc;
  if (row_begin < 0 || row_count < 0 || row_begin > m->N || row_count > m->N - row_begin)
    return gw_sdne_fail(m, GW_ERR_INVALID, "rows [%lld, +%lld) outside [0, %lld)", (long long)row_begin,
                        (long long)row_count, (long long)m->N);
  if (row_count == 0) return GW_OK;
  if (m->device >= 0) return gw_sdne_dev_encode(m, row_begin, row_count, out);
  const int64_t u2 = m->u[2];
  HostAct A;
  for (int64_t r0 = row_begin; r0 < row_begin + row_count; r0 += 256) {
    const int64_t M = std::min<int64_t>(256, row_begin + row_count - r0);
    host_stage(m, nullptr, r0, M, &A.x);
    host_forward(m, M, false, &A);
    memcpy(m->enc.data() + r0 * u2, A.z2.data(), (size_t)(M * u2) * sizeof(float));
  }
  if (out) memcpy(out, m->enc.data() + row_begin * u2, (size_t)(row_count * u2) * sizeof(float));
  return GW_OK;
}

extern "C" int gw_sdne_export(gw_sdne* m, float* const par[8], float* const adam_m[8], float* const adam_v[8]) {
  if (!m) return gw_sdne_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (m->device >= 0) return gw_sdne_dev_export(m, par, adam_m, adam_v);
  for (int t = 0; t < 8; ++t) {
    const size_t bytes = gw_sdne_numel(m, t) * sizeof(float);
    if (par && par[t]) memcpy(par[t], m->par[t].data(), bytes);
    if (adam_m && adam_m[t]) memcpy(adam_m[t], m->am[t].data(), bytes);
    if (adam_v && adam_v[t]) memcpy(adam_v[t], m->av[t].data(), bytes);
  }
  return GW_OK;
}

extern "C" int gw_sdne_vectors_dev(gw_sdne* m, float** ptr, int64_t* pitch) {
  if (!m || !ptr || !pitch) return gw_sdne_fail(m, GW_ERR_INVALID, "NULL argument");
  if (!m->have_rows) return gw_sdne_fail(m, GW_ERR_STATE, "no rows set");
  *ptr = m->device < 0 ? m->enc.data() : gw_sdne_dev_vectors(m);
  *pitch = m->u[2];
  return GW_OK;
}
