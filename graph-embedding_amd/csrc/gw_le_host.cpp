// Laplacian eigenmaps: C ABI, argument checks, the assembly of S, the solver
// (shared by both modes: orthonormalisation, Rayleigh-Ritz, selection, filter)
// and the host evaluation of the law (device = -1).  The law itself is
// gw_le_law.h; the kernels are gw_le.hip.
//
// This file depends on nothing but the C++ library, so that it also builds as
// a plain host program (-DGW_LE_HOST_ONLY: no device path) for sanitizer runs
// (host/le_host_check.cpp).
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <numeric>
#include <vector>

#include "gw_le_internal.h"
#include "gw_trainer_fail.h"

static thread_local std::string g_le_err;

int gw_le_fail(gw_le* m, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  gw_trainer_vfail(m ? &m->err : nullptr, &g_le_err, code, fmt, ap);
  va_end(ap);
  return code;
}

#ifdef GW_LE_HOST_ONLY
static int no_dev(gw_le* m) { return gw_le_fail(m, GW_ERR_DEVICE, "built without the device path"); }
int gw_le_dev_alloc(gw_le* m) { return no_dev(m); }
void gw_le_dev_free(gw_le*) {}
int gw_le_dev_upload(gw_le* m) { return no_dev(m); }
int gw_le_dev_prepare(gw_le* m) { return no_dev(m); }
int gw_le_dev_init(gw_le* m, int) { return no_dev(m); }
int gw_le_dev_apply(gw_le* m, int, double, double, double, int, int, int) { return no_dev(m); }
int gw_le_dev_gram(gw_le* m, int, int, double*) { return no_dev(m); }
int gw_le_dev_rotate(gw_le* m, int, int, const double*) { return no_dev(m); }
int gw_le_dev_resid(gw_le* m, int, int, const double*, double*) { return no_dev(m); }
int gw_le_dev_colstat(gw_le* m, int, int, int, double*, int32_t*) { return no_dev(m); }
int gw_le_dev_output(gw_le* m, int, int, int, const double*, const int32_t*) { return no_dev(m); }
int gw_le_dev_export(gw_le* m, double*) { return no_dev(m); }
int gw_le_dev_vectors(gw_le* m, float**) { return no_dev(m); }
int gw_le_dev_apply_user(gw_le* m, const double*, double*, int) { return no_dev(m); }
extern "C" int gw_le_kernel_attrs(gw_le* m, int, const char**, int32_t*, int32_t*, int32_t*, int32_t*) {
  return no_dev(m);
}
extern "C" int gw_le_time_kernel(gw_le* m, int, int, double*) { return no_dev(m); }
#endif

extern "C" const char* gw_le_last_error(const gw_le* m) { return m ? m->err.c_str() : g_le_err.c_str(); }

extern "C" int gw_le_create(int device, int64_t n, const gw_le_params_t* params, gw_le** out) {
  if (!out) return gw_le_fail(nullptr, GW_ERR_INVALID, "NULL out");
  *out = nullptr;
  gw_le_params_t p;
  memset(&p, 0, sizeof p);
  p.dim = 128;
  p.cheb_degree = 20;
  p.max_iters = 100;
  p.symmetrize = GW_LE_SYM_MEAN;
  p.tol = 1e-8;
  p.min_eigenvalue = 1e-5;
  if (params) {
    if (params->struct_size < (int32_t)sizeof(int32_t))
      return gw_le_fail(nullptr, GW_ERR_INVALID, "gw_le_params_t.struct_size %d", (int)params->struct_size);
    memcpy(&p, params, std::min((size_t)params->struct_size, sizeof p));
  }
  p.struct_size = (int32_t)sizeof p;
  if (p.block == 0 && p.dim >= 1 && p.dim <= 0x7FFFFFFF - 32) p.block = p.dim + 32;
  if (p.dim < 1 || p.block < 1) return gw_le_fail(nullptr, GW_ERR_INVALID, "dim %d and block %d must be positive", p.dim, p.block);
  if (p.dim >= p.block) return gw_le_fail(nullptr, GW_ERR_INVALID, "dim %d must be below block %d", p.dim, p.block);
  if (p.cheb_degree < 1 || p.max_iters < 1)
    return gw_le_fail(nullptr, GW_ERR_INVALID, "cheb_degree %d and max_iters %d must be positive", p.cheb_degree, p.max_iters);
  if (!(p.tol > 0.0) || p.min_eigenvalue != p.min_eigenvalue)
    return gw_le_fail(nullptr, GW_ERR_INVALID, "tol must be positive and min_eigenvalue a number");
  if (p.symmetrize != GW_LE_SYM_MEAN && p.symmetrize != GW_LE_SYM_MAX)
    return gw_le_fail(nullptr, GW_ERR_INVALID, "symmetrize %d", p.symmetrize);
  if (p.self_loops != 0 && p.self_loops != 1) return gw_le_fail(nullptr, GW_ERR_INVALID, "self_loops %d", p.self_loops);
  if (device < -1) return gw_le_fail(nullptr, GW_ERR_INVALID, "device %d", device);
  if (n < 1 || n >= (int64_t)1 << 31) return gw_le_fail(nullptr, GW_ERR_INVALID, "n %lld out of range", (long long)n);
  if (device >= 0 && p.block > GW_LE_MAX_BLOCK)
    return gw_le_fail(nullptr, GW_ERR_UNSUPPORTED, "block %d: the kernels take block <= %d (device = -1 takes any)", p.block,
                      GW_LE_MAX_BLOCK);
  gw_le* m = new (std::nothrow) gw_le();
  if (!m) return gw_le_fail(nullptr, GW_ERR_NOMEM, "out of memory");
  m->device = device;
  m->p = p;
  m->n = n;
  if (device >= 0) {
    const int rc = gw_le_dev_alloc(m);
    if (rc != GW_OK) {
      g_le_err = m->err;
      gw_le_dev_free(m);
      delete m;
      return rc;
    }
  }
  *out = m;
  return GW_OK;
}

extern "C" int gw_le_free(gw_le* m) {
  if (!m) return GW_OK;
  if (m->device >= 0) gw_le_dev_free(m);
  delete m;
  return GW_OK;
}

// ---- assembly of S -------------------------------------------------------------
namespace {

struct Ent {
  int32_t j;
  double a;
};

// a_ij of the law as a CSR with ascending columns; count(i) = entries offered for row i, at(i, e) = the e-th
template <typename Count, typename At>
int build_a(gw_le* m, Count count, At at, std::vector<int64_t>& off, std::vector<Ent>& ent) {
  const int64_t n = m->n;
  off.assign((size_t)n + 1, 0);
  ent.clear();
  std::vector<Ent> row;
  for (int64_t i = 0; i < n; ++i) {
    row.clear();
    const int64_t cnt = count(i);
    for (int64_t e = 0; e < cnt; ++e) {
      const Ent x = at(i, e);
      if (x.j == -1) break;  // padding ends the row
      if (x.j < 0 || x.j >= n)
        return gw_le_fail(m, GW_ERR_RANGE, "row %lld: id %d outside [-1, %lld)", (long long)i, (int)x.j, (long long)n);
      if ((x.j == i && !m->p.self_loops) || !(x.a > 0.0)) continue;  // self entries (unless kept), NaN and non-positive weights
      row.push_back(x);
    }
    std::stable_sort(row.begin(), row.end(), [](const Ent& a, const Ent& b) { return a.j < b.j; });
    for (size_t e = 0; e < row.size(); ++e)
      if (e + 1 == row.size() || row[e + 1].j != row[e].j) ent.push_back(row[e]);  // a repeated id keeps the last
    off[(size_t)i + 1] = (int64_t)ent.size();
  }
  return GW_OK;
}

int assemble(gw_le* m, const std::vector<int64_t>& aoff, const std::vector<Ent>& a) {
  const int64_t n = m->n;
  // the transpose, rows ascending within a column by construction
  std::vector<int64_t> toff((size_t)n + 1, 0);
  for (const Ent& e : a) toff[(size_t)e.j + 1] += 1;
  for (int64_t i = 0; i < n; ++i) toff[(size_t)i + 1] += toff[(size_t)i];
  std::vector<Ent> t(a.size());
  {
    std::vector<int64_t> pos(toff.begin(), toff.end() - 1);
    for (int64_t i = 0; i < n; ++i)
      for (int64_t e = aoff[(size_t)i]; e < aoff[(size_t)i + 1]; ++e) t[(size_t)pos[(size_t)a[(size_t)e].j]++] = {(int32_t)i, a[(size_t)e].a};
  }
  const bool mean = m->p.symmetrize == GW_LE_SYM_MEAN;
  m->off.assign((size_t)n + 1, 0);
  m->col.clear();
  m->val.clear();
  m->s.assign((size_t)n, 0.0);
  for (int64_t i = 0; i < n; ++i) {  // merge row i of a and of its transpose
    int64_t p = aoff[(size_t)i], q = toff[(size_t)i];
    const int64_t pe = aoff[(size_t)i + 1], qe = toff[(size_t)i + 1];
    double d = 0.0;
    while (p < pe || q < qe) {
      const int32_t jp = p < pe ? a[(size_t)p].j : 0x7FFFFFFF, jq = q < qe ? t[(size_t)q].j : 0x7FFFFFFF;
      const int32_t j = std::min(jp, jq);
      const double x = jp == j ? a[(size_t)p++].a : 0.0, y = jq == j ? t[(size_t)q++].a : 0.0;
      const double w = mean ? (x + y) / 2.0 : (x > y ? x : y);
      m->col.push_back(j);
      m->val.push_back(w);
      d = d + w;
    }
    m->off[(size_t)i + 1] = (int64_t)m->col.size();
    m->s[(size_t)i] = d > 0.0 ? 1.0 / GW_LE_SQRT(d) : 0.0;
  }
  m->nz_rows = 0;
  for (int64_t i = 0; i < n; ++i) {
    const double si = m->s[(size_t)i];
    m->nz_rows += si != 0.0;
    for (int64_t e = m->off[(size_t)i]; e < m->off[(size_t)i + 1]; ++e)
      m->val[(size_t)e] = (m->val[(size_t)e] * si) * m->s[(size_t)m->col[(size_t)e]];
  }
  m->have_op = true;
  m->solved = false;
  return m->device >= 0 ? gw_le_dev_upload(m) : GW_OK;
}

}  // namespace

extern "C" int gw_le_set_rows(gw_le* m, const int32_t* ids, const double* scores, int topk) {
  if (!m) return gw_le_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!ids || !scores || topk < 1) return gw_le_fail(m, GW_ERR_INVALID, "NULL rows or topk below 1");
  m->have_op = false;
  std::vector<int64_t> off;
  std::vector<Ent> a;
  const int rc = build_a(
      m, [topk](int64_t) { return (int64_t)topk; },
      [=](int64_t i, int64_t e) { return Ent{ids[i * topk + e], scores[i * topk + e]}; }, off, a);
  return rc != GW_OK ? rc : assemble(m, off, a);
}

extern "C" int gw_le_set_csr(gw_le* m, const int64_t* offsets, const int32_t* nbrs, const double* weights) {
  if (!m) return gw_le_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!offsets || (!nbrs && offsets[m->n] > 0)) return gw_le_fail(m, GW_ERR_INVALID, "NULL offsets or nbrs");
  m->have_op = false;
  for (int64_t i = 0; i < m->n; ++i)
    if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) return gw_le_fail(m, GW_ERR_INVALID, "offsets must not descend");
  std::vector<int64_t> off;
  std::vector<Ent> a;
  const int rc = build_a(
      m, [=](int64_t i) { return offsets[i + 1] - offsets[i]; },
      [=](int64_t i, int64_t e) { return Ent{nbrs[offsets[i] + e], weights ? weights[offsets[i] + e] : 1.0}; }, off, a);
  return rc != GW_OK ? rc : assemble(m, off, a);
}

// ---- the law on the host ---------------------------------------------------------
namespace {

void host_apply_block(const gw_le* m, int mode, double alpha, double beta, double gamma, const double* x, double* y,
                      const double* z, int64_t cols) {
  const int64_t n = m->n;
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; ++i) {
    const int64_t b = m->off[(size_t)i], cnt = m->off[(size_t)i + 1] - b;
    for (int64_t c = 0; c < cols; ++c) {
      const double t = gw_le_row_dot(m->val.data() + b, m->col.data() + b, cnt, x, cols, c);
      y[i * cols + c] = gw_le_combine(mode, alpha, t, beta, x[i * cols + c], gamma, z ? z[i * cols + c] : 0.0);
    }
  }
}

void host_init(gw_le* m, int dst) {
  const int64_t n = m->n, mb = m->m;
  double* x = m->hb[dst].data();
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < n; ++i)
    for (int64_t c = 0; c < mb; ++c) x[i * mb + c] = m->s[(size_t)i] == 0.0 ? 0.0 : gw_le_start(m->p.seed, i, (int)c);
}

// C[i][j] = sum over rows of A[r][i] * B[r][j] under the chunk law, i <= j computed and mirrored
void host_gram(const gw_le* m, const double* A, const double* B, double* C) {
  const int64_t n = m->n, mb = m->m, chunks = (n + GW_LE_CHUNK - 1) / GW_LE_CHUNK;
  const int64_t group = 32;
  std::vector<double> part((size_t)(std::min(group, chunks) * mb * mb));
  std::fill(C, C + mb * mb, 0.0);
  for (int64_t g0 = 0; g0 < chunks; g0 += group) {
    const int64_t g1 = std::min(chunks, g0 + group);
#pragma omp parallel for schedule(static)
    for (int64_t ch = g0; ch < g1; ++ch) {
      double* P = part.data() + (ch - g0) * mb * mb;
      std::fill(P, P + mb * mb, 0.0);
      const int64_t r1 = std::min(n, (ch + 1) * GW_LE_CHUNK);
      for (int64_t r = ch * GW_LE_CHUNK; r < r1; ++r)
        for (int64_t i = 0; i < mb; ++i) {
          const double a = A[r * mb + i];
          for (int64_t j = i; j < mb; ++j) P[i * mb + j] = GW_LE_FMA(a, B[r * mb + j], P[i * mb + j]);
        }
    }
    for (int64_t ch = g0; ch < g1; ++ch) {
      const double* P = part.data() + (ch - g0) * mb * mb;
      for (int64_t i = 0; i < mb; ++i)
        for (int64_t j = i; j < mb; ++j) C[i * mb + j] = C[i * mb + j] + P[i * mb + j];
    }
  }
  for (int64_t i = 0; i < mb; ++i)
    for (int64_t j = i + 1; j < mb; ++j) C[j * mb + i] = C[i * mb + j];
}

void host_rotate(const gw_le* m, const double* X, double* out, const double* Q) {
  const int64_t n = m->n, mb = m->m;
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < n; ++i) {
    double* o = out + i * mb;
    for (int64_t c = 0; c < mb; ++c) o[c] = 0.0;
    for (int64_t k = 0; k < mb; ++k) {
      const double xk = X[i * mb + k];
      for (int64_t c = 0; c < mb; ++c) o[c] = GW_LE_FMA(xk, Q[k * mb + c], o[c]);
    }
  }
}

// Column sums of squares under the chunk law.  theta != NULL: of fma(-theta_c, x, y) over all m columns; else of
// s_i * x over columns col0 .. col0 + dim, with negate[c] = the entry of largest magnitude (lowest row) is negative.
void host_colsq(const gw_le* m, const double* X, const double* Y, const double* theta, int64_t col0, int64_t dim,
                double* sumsq, int32_t* negate) {
  const int64_t n = m->n, mb = m->m, chunks = (n + GW_LE_CHUNK - 1) / GW_LE_CHUNK;
  std::vector<double> part((size_t)(chunks * dim)), amax((size_t)(chunks * dim), 0.0);
  std::vector<int64_t> arow((size_t)(chunks * dim), -1);
#pragma omp parallel for schedule(static)
  for (int64_t ch = 0; ch < chunks; ++ch) {
    const int64_t r1 = std::min(n, (ch + 1) * GW_LE_CHUNK);
    for (int64_t c = 0; c < dim; ++c) {
      double acc = 0.0, best = 0.0;
      int64_t brow = -1;
      for (int64_t r = ch * GW_LE_CHUNK; r < r1; ++r) {
        const double x = X[r * mb + col0 + c];
        const double v = theta ? gw_le_res_term(theta[c], x, Y[r * mb + col0 + c]) : m->s[(size_t)r] * x;
        acc = GW_LE_FMA(v, v, acc);
        const double av = v < 0.0 ? -v : v;
        if (av > best) {
          best = av;
          brow = r;
        }
      }
      part[(size_t)(ch * dim + c)] = acc;
      amax[(size_t)(ch * dim + c)] = best;
      arow[(size_t)(ch * dim + c)] = brow;
    }
  }
  for (int64_t c = 0; c < dim; ++c) {
    double acc = 0.0, best = 0.0;
    int64_t brow = -1;
    for (int64_t ch = 0; ch < chunks; ++ch) {
      acc = acc + part[(size_t)(ch * dim + c)];
      if (amax[(size_t)(ch * dim + c)] > best) {
        best = amax[(size_t)(ch * dim + c)];
        brow = arow[(size_t)(ch * dim + c)];
      }
    }
    sumsq[c] = acc;
    if (negate) negate[c] = brow >= 0 && m->s[(size_t)brow] * X[brow * mb + col0 + c] < 0.0;
  }
}

void host_output(gw_le* m, const double* X, int64_t col0, int64_t dim, const double* nrm, const int32_t* negate) {
  const int64_t n = m->n, mb = m->m;
  m->out64.resize((size_t)(n * dim));
  m->out32.resize((size_t)(n * dim));
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < n; ++i)
    for (int64_t c = 0; c < dim; ++c) {
      const double f = gw_le_out(m->s[(size_t)i], X[i * mb + col0 + c], nrm[c], negate[c]);
      m->out64[(size_t)(i * dim + c)] = f;
      m->out32[(size_t)(i * dim + c)] = (float)f;
    }
}

// ---- the backend of the solver: one body per mode ---------------------------------
int op_prepare(gw_le* m) {
  if (m->device >= 0) return gw_le_dev_prepare(m);
  for (auto& b : m->hb) b.assign((size_t)(m->n * m->m), 0.0);
  return GW_OK;
}
int op_init(gw_le* m, int dst) {
  if (m->device >= 0) return gw_le_dev_init(m, dst);
  host_init(m, dst);
  return GW_OK;
}
int op_apply(gw_le* m, int mode, double alpha, double beta, double gamma, int src, int dst, int z) {
  if (m->device >= 0) return gw_le_dev_apply(m, mode, alpha, beta, gamma, src, dst, z);
  host_apply_block(m, mode, alpha, beta, gamma, m->hb[src].data(), m->hb[dst].data(), z >= 0 ? m->hb[z].data() : nullptr,
                   m->m);
  return GW_OK;
}
int op_gram(gw_le* m, int a, int b, double* C) {
  if (m->device >= 0) return gw_le_dev_gram(m, a, b, C);
  host_gram(m, m->hb[a].data(), m->hb[b].data(), C);
  return GW_OK;
}
int op_rotate(gw_le* m, int src, int dst, const double* Q) {
  if (m->device >= 0) return gw_le_dev_rotate(m, src, dst, Q);
  host_rotate(m, m->hb[src].data(), m->hb[dst].data(), Q);
  return GW_OK;
}
int op_resid(gw_le* m, int x, int y, const double* theta, double* sumsq) {
  if (m->device >= 0) return gw_le_dev_resid(m, x, y, theta, sumsq);
  host_colsq(m, m->hb[x].data(), m->hb[y].data(), theta, 0, m->m, sumsq, nullptr);
  return GW_OK;
}
int op_colstat(gw_le* m, int x, int col0, int dim, double* sumsq, int32_t* negate) {
  if (m->device >= 0) return gw_le_dev_colstat(m, x, col0, dim, sumsq, negate);
  host_colsq(m, m->hb[x].data(), nullptr, nullptr, col0, dim, sumsq, negate);
  return GW_OK;
}
int op_output(gw_le* m, int x, int col0, int dim, const double* nrm, const int32_t* negate) {
  if (m->device >= 0) return gw_le_dev_output(m, x, col0, dim, nrm, negate);
  host_output(m, m->hb[x].data(), col0, dim, nrm, negate);
  return GW_OK;
}

// ---- m x m symmetric eigenproblem: cyclic Jacobi, rows (p, q) in a fixed order ------
// w[k] and column k of V (V[i * n + k]) are the pairs, in no particular order.
void jacobi(int n, std::vector<double>& A_in, std::vector<double>& V, std::vector<double>& w) {
  const size_t ld = (size_t)n + 8;  // rows padded: a column walk does not stay in one cache set at n = 256
  std::vector<double> A(ld * n, 0.0), Vt(ld * n, 0.0);  // row k of Vt = eigenvector k, so a rotation walks two rows
  double norm2 = 0.0;
  for (int i = 0; i < n; ++i) {
    Vt[i * ld + i] = 1.0;
    for (int j = 0; j < n; ++j) {
      A[i * ld + j] = A_in[(size_t)i * n + j];
      norm2 = norm2 + A[i * ld + j] * A[i * ld + j];
    }
  }
  const double tiny = 1e-32 * norm2;  // an off-diagonal entry below 1e-16 * ||A||_F is left alone
  for (int sweep = 0; sweep < 60; ++sweep) {
    int rotations = 0;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        double* __restrict rp = A.data() + p * ld;
        double* __restrict rq = A.data() + q * ld;
        const double apq = rp[q], app = rp[p], aqq = rq[q];
        if (apq * apq <= tiny || apq * apq <= 1e-33 * (app < 0 ? -app : app) * (aqq < 0 ? -aqq : aqq)) continue;
        rotations += 1;
        const double th = (aqq - app) / (2.0 * apq);
        const double ath = th < 0 ? -th : th;
        double t = 1.0 / (ath + GW_LE_SQRT(th * th + 1.0));
        if (th < 0) t = -t;
        const double c = 1.0 / GW_LE_SQRT(t * t + 1.0), s = t * c;
#pragma omp simd
        for (int k = 0; k < n; ++k) {  // rows p and q (p != q: the two never overlap)
          const double x = rp[k], y = rq[k];
          rp[k] = c * x - s * y;
          rq[k] = s * x + c * y;
        }
        rp[p] = app - t * apq;
        rq[q] = aqq + t * apq;
        rp[q] = 0.0;
        rq[p] = 0.0;
        for (int k = 0; k < n; ++k) {  // and the columns, their copies
          if (k == p || k == q) continue;
          A[k * ld + p] = rp[k];
          A[k * ld + q] = rq[k];
        }
        double* __restrict vp = Vt.data() + p * ld;
        double* __restrict vq = Vt.data() + q * ld;
#pragma omp simd
        for (int k = 0; k < n; ++k) {
          const double x = vp[k], y = vq[k];
          vp[k] = c * x - s * y;
          vq[k] = s * x + c * y;
        }
      }
    if (!rotations) break;
  }
  w.resize((size_t)n);
  V.resize((size_t)n * n);
  for (int k = 0; k < n; ++k) {
    w[(size_t)k] = A[k * ld + k];
    for (int i = 0; i < n; ++i) V[(size_t)i * n + k] = Vt[k * ld + i];
  }
}

// X (block x) <- an orthonormal basis of its span; `spare` is overwritten.  On return x names the block that holds it.
int orthonormalise(gw_le* m, int& x, int& spare) {
  const int mb = m->m;
  std::vector<double> G((size_t)mb * mb), A, V, w, Q((size_t)mb * mb), t((size_t)mb);
  for (int pass = 0;; ++pass) {
    int rc = op_gram(m, x, x, G.data());
    if (rc != GW_OK) return rc;
    double dev = 0.0;
    bool finite = true;
    for (int i = 0; i < mb; ++i)
      for (int j = 0; j < mb; ++j) {
        const double d = G[(size_t)i * mb + j] - (i == j ? 1.0 : 0.0);
        finite = finite && d == d && d - d == 0.0;
        dev = std::max(dev, d < 0 ? -d : d);
      }
    if (!finite) return gw_le_fail(m, GW_ERR_STATE, "the block is not finite");
    if (dev <= 1e-13 * mb) return GW_OK;
    if (pass == 6) return gw_le_fail(m, GW_ERR_STATE, "orthonormalisation stalled at %.3g after 6 passes", dev);
    for (int i = 0; i < mb; ++i) t[(size_t)i] = G[(size_t)i * mb + i] > 0.0 ? 1.0 / GW_LE_SQRT(G[(size_t)i * mb + i]) : 0.0;
    A.resize((size_t)mb * mb);
    for (int i = 0; i < mb; ++i)
      for (int j = 0; j < mb; ++j) A[(size_t)i * mb + j] = (G[(size_t)i * mb + j] * t[(size_t)i]) * t[(size_t)j];
    jacobi(mb, A, V, w);
    double wmax = 0.0;
    for (double v : w) wmax = std::max(wmax, v);
    for (int k = 0; k < mb; ++k) {
      const double lam = std::max(w[(size_t)k], 1e-15 * wmax);
      const double r = lam > 0.0 ? 1.0 / GW_LE_SQRT(lam) : 0.0;
      for (int i = 0; i < mb; ++i) Q[(size_t)i * mb + k] = (t[(size_t)i] * V[(size_t)i * mb + k]) * r;
    }
    rc = op_rotate(m, x, spare, Q.data());
    if (rc != GW_OK) return rc;
    std::swap(x, spare);
  }
}

int solve(gw_le* m) {
  const int dim = m->p.dim;
  m->m = (int)std::min<int64_t>(m->p.block, m->nz_rows);
  const int mb = m->m;
  gw_le_stats_t& st = m->st;
  memset(&st, 0, sizeof st);
  st.block_used = mb;
  st.isolated = m->n - m->nz_rows;
  if (mb < 1) return gw_le_fail(m, GW_ERR_CAPACITY, "every row is isolated: no eigenpair above min_eigenvalue (dim %d)", dim);
  int rc = op_prepare(m);
  if (rc != GW_OK) return rc;
  int X = 0, Y = 1, T = 2, U = 3;
  rc = op_init(m, X);
  if (rc != GW_OK) return rc;
  std::vector<double> H((size_t)mb * mb), V, w, Q((size_t)mb * mb), ss((size_t)mb);
  std::vector<int> order((size_t)mb);
  m->theta.assign((size_t)mb, 0.0);
  m->resid.assign((size_t)mb, 0.0);
  for (;;) {
    rc = orthonormalise(m, X, U);
    if (rc != GW_OK) return rc;
    rc = op_apply(m, GW_LE_PLAIN, 1.0, 0.0, 0.0, X, Y, -1);  // Rayleigh-Ritz
    if (rc != GW_OK) return rc;
    st.applies += 1;
    rc = op_gram(m, X, Y, H.data());
    if (rc != GW_OK) return rc;
    jacobi(mb, H, V, w);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&w](int a, int b) { return w[(size_t)a] > w[(size_t)b]; });
    for (int k = 0; k < mb; ++k) {
      m->theta[(size_t)k] = w[(size_t)order[(size_t)k]];
      for (int i = 0; i < mb; ++i) Q[(size_t)i * mb + k] = V[(size_t)i * mb + order[(size_t)k]];
    }
    rc = op_rotate(m, X, U, Q.data());
    if (rc != GW_OK) return rc;
    std::swap(X, U);
    rc = op_rotate(m, Y, U, Q.data());
    if (rc != GW_OK) return rc;
    std::swap(Y, U);
    rc = op_resid(m, X, Y, m->theta.data(), ss.data());
    if (rc != GW_OK) return rc;
    for (int k = 0; k < mb; ++k) m->resid[(size_t)k] = GW_LE_SQRT(ss[(size_t)k]);
    st.iters += 1;
    int skipped = 0;
    while (skipped < mb && 1.0 - m->theta[(size_t)skipped] <= m->p.min_eigenvalue) ++skipped;
    st.skipped = m->skipped = skipped;
    if ((int64_t)skipped + dim + 1 > mb && mb < m->nz_rows)
      return gw_le_fail(m, GW_ERR_CAPACITY, "%d eigenvalues <= min_eigenvalue and dim %d do not fit block %d: block %lld needed",
                        skipped, dim, mb, (long long)skipped + dim + 1);
    if ((int64_t)skipped + dim > mb)
      return gw_le_fail(m, GW_ERR_CAPACITY, "the graph has %d eigenvalues above min_eigenvalue, fewer than dim %d", mb - skipped,
                        dim);
    double rmax = 0.0;
    for (int k = 0; k < skipped + dim; ++k) rmax = std::max(rmax, m->resid[(size_t)k]);
    st.max_residual = rmax;
    if (rmax <= m->p.tol) {
      st.state = GW_LE_CONVERGED;
      break;
    }
    if (st.iters >= m->p.max_iters) {
      st.state = GW_LE_NOT_CONVERGED;
      break;
    }
    // Chebyshev filter on [-1, b], b the block's smallest Ritz value (kept off -1 so that the interval has width)
    const double a = -1.0, b = std::max(m->theta[(size_t)mb - 1], -0.99);
    const double c = (a + b) / 2.0, e = (b - a) / 2.0;
    rc = op_apply(m, GW_LE_AXPY, 1.0 / e, -c / e, 0.0, X, T, -1);  // T1 = (S T0 - c T0) / e
    if (rc != GW_OK) return rc;
    st.applies += 1;
    int prev = X, cur = T, next = Y;
    for (int k = 2; k <= m->p.cheb_degree; ++k) {
      rc = op_apply(m, GW_LE_CHEB, 2.0 / e, -2.0 * c / e, -1.0, cur, next, prev);
      if (rc != GW_OK) return rc;
      st.applies += 1;
      const int old = prev;
      prev = cur;
      cur = next;
      next = old;
    }
    // cur holds the filtered block; the other three are free
    const int was[4] = {X, Y, T, U};
    int freeb[3], nf = 0;
    for (int b4 : was)
      if (b4 != cur) freeb[nf++] = b4;
    X = cur;
    Y = freeb[0];
    T = freeb[1];
    U = freeb[2];
  }
  // output: the wanted columns, scaled, signed, rounded
  std::vector<double> nrm((size_t)dim);
  std::vector<int32_t> neg((size_t)dim);
  rc = op_colstat(m, X, m->skipped, dim, nrm.data(), neg.data());
  if (rc != GW_OK) return rc;
  for (int c = 0; c < dim; ++c) nrm[(size_t)c] = GW_LE_SQRT(nrm[(size_t)c]);
  rc = op_output(m, X, m->skipped, dim, nrm.data(), neg.data());
  if (rc != GW_OK) return rc;
  m->solved = true;
  return GW_OK;
}

}  // namespace

extern "C" int gw_le_solve(gw_le* m, gw_le_stats_t* stats, void* stream) {
  if (!m) return gw_le_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->have_op) return gw_le_fail(m, GW_ERR_STATE, "call gw_le_set_rows or gw_le_set_csr first");
  m->solved = false;
  m->stream = stream;
  const int rc = solve(m);
  m->stream = nullptr;
  if (stats) *stats = m->st;
  return rc;
}

extern "C" int gw_le_export(gw_le* m, double* eigenvalues, double* vectors, double* residuals) {
  if (!m) return gw_le_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->solved) return gw_le_fail(m, GW_ERR_STATE, "call gw_le_solve first");
  const int dim = m->p.dim;
  for (int c = 0; c < dim; ++c) {
    if (eigenvalues) eigenvalues[c] = 1.0 - m->theta[(size_t)(m->skipped + c)];
    if (residuals) residuals[c] = m->resid[(size_t)(m->skipped + c)];
  }
  if (!vectors) return GW_OK;
  if (m->device >= 0) return gw_le_dev_export(m, vectors);
  memcpy(vectors, m->out64.data(), sizeof(double) * m->out64.size());
  return GW_OK;
}

extern "C" int gw_le_vectors_dev(gw_le* m, float** ptr, int64_t* pitch) {
  if (!m || !ptr) return gw_le_fail(m, GW_ERR_INVALID, "NULL handle or ptr");
  if (!m->solved) return gw_le_fail(m, GW_ERR_STATE, "call gw_le_solve first");
  if (pitch) *pitch = m->p.dim;
  if (m->device >= 0) return gw_le_dev_vectors(m, ptr);
  *ptr = m->out32.data();
  return GW_OK;
}

extern "C" int gw_le_apply(gw_le* m, const double* x, double* y, int cols) {
  if (!m) return gw_le_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->have_op) return gw_le_fail(m, GW_ERR_STATE, "call gw_le_set_rows or gw_le_set_csr first");
  if (!x || !y || cols < 1) return gw_le_fail(m, GW_ERR_INVALID, "NULL block or cols below 1");
  if (m->device >= 0) return gw_le_dev_apply_user(m, x, y, cols);
  host_apply_block(m, GW_LE_PLAIN, 1.0, 0.0, 0.0, x, y, nullptr, cols);
  return GW_OK;
}

extern "C" int gw_le_tiles(const gw_le* m, int32_t* rows_per_wg, int32_t* chunk, int32_t* cols_per_pass) {
  if (!m) return gw_le_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (rows_per_wg) *rows_per_wg = 4;  // one row of S per wave, four waves (gw_le.hip asserts it)
  if (chunk) *chunk = GW_LE_CHUNK;
  if (cols_per_pass) *cols_per_pass = 64;
  return GW_OK;
}
