// One-vs-rest scorer: C ABI, argument checks, the host evaluation of the law
// (device = -1).  The law itself is gw_ovr_law.h; the kernels are gw_ovr.hip.
//
// This file depends on nothing but the C++ library, so that it also builds as
// a plain host program (-DGW_OVR_HOST_ONLY: no device path) for sanitizer
// runs (host/ovr_host_check.cpp).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <new>

#include "gw_ovr_internal.h"
#include "gw_trainer_fail.h"

static thread_local std::string g_ovr_err;

int gw_ovr_fail(gw_ovr* m, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  gw_trainer_vfail(m ? &m->err : nullptr, &g_ovr_err, code, fmt, ap);
  va_end(ap);
  return code;
}

#ifdef GW_OVR_HOST_ONLY
static int no_dev(gw_ovr* m) { return gw_ovr_fail(m, GW_ERR_DEVICE, "built without the device path"); }
int gw_ovr_dev_alloc(gw_ovr* m) { return no_dev(m); }
void gw_ovr_dev_free(gw_ovr*) {}
int gw_ovr_dev_upload_labels(gw_ovr* m) { return no_dev(m); }
int gw_ovr_dev_fit(gw_ovr* m, const int64_t*, int64_t, const uint8_t*, int64_t*, void*) { return no_dev(m); }
int gw_ovr_dev_score(gw_ovr* m, const int64_t*, int64_t, int64_t*, void*) { return no_dev(m); }
int gw_ovr_dev_decision(gw_ovr* m, const int64_t*, int64_t, double*) { return no_dev(m); }
extern "C" int gw_ovr_kernel_attrs(gw_ovr* m, int, const char**, int32_t*, int32_t*, int32_t*, int32_t*) {
  return no_dev(m);
}
#endif

extern "C" const char* gw_ovr_last_error(const gw_ovr* m) { return m ? m->err.c_str() : g_ovr_err.c_str(); }

extern "C" int gw_ovr_create(int device, int64_t n, const gw_ovr_params_t* params, gw_ovr** out) {
  if (!out) return gw_ovr_fail(nullptr, GW_ERR_INVALID, "NULL out");
  *out = nullptr;
  gw_ovr_params_t p;
  memset(&p, 0, sizeof p);
  p.dim = 128;
  p.max_newton = 100;
  p.max_cg = 200;
  p.C = 1.0;
  p.gtol = 1e-8;
  if (params) {
    if (params->struct_size < (int32_t)sizeof(int32_t))
      return gw_ovr_fail(nullptr, GW_ERR_INVALID, "gw_ovr_params_t.struct_size %d", (int)params->struct_size);
    memcpy(&p, params, std::min((size_t)params->struct_size, sizeof p));
  }
  p.struct_size = (int32_t)sizeof p;
  if (n < 1 || n >= (int64_t)1 << 40) return gw_ovr_fail(nullptr, GW_ERR_INVALID, "n %lld out of range", (long long)n);
  if (p.dim < 1 || p.labels < 1 || p.dim > (1 << 20) || p.labels > (1 << 20))
    return gw_ovr_fail(nullptr, GW_ERR_INVALID, "dim %d and labels %d must be positive", p.dim, p.labels);
  if (p.max_newton < 1 || p.max_cg < 1)
    return gw_ovr_fail(nullptr, GW_ERR_INVALID, "max_newton %d and max_cg %d must be positive", p.max_newton, p.max_cg);
  if (!(p.C > 0.0) || !(p.C <= 1e300) || !(p.gtol >= 0.0) || !(p.gtol < 1.0))
    return gw_ovr_fail(nullptr, GW_ERR_INVALID, "C must be positive and finite, gtol in [0, 1)");
  if (device < -1) return gw_ovr_fail(nullptr, GW_ERR_INVALID, "device %d", device);
  if (device >= 0 && (p.dim > GW_OVR_MAX_DIM || p.labels > GW_OVR_MAX_LABELS))
    return gw_ovr_fail(nullptr, GW_ERR_UNSUPPORTED, "dim %d / labels %d: the kernels take dim <= %d and labels <= %d "
                       "(device = -1 takes any)", p.dim, p.labels, GW_OVR_MAX_DIM, GW_OVR_MAX_LABELS);
  gw_ovr* m = new (std::nothrow) gw_ovr();
  if (!m) return gw_ovr_fail(nullptr, GW_ERR_NOMEM, "out of memory");
  m->device = device;
  m->p = p;
  m->n = n;
  m->L = p.labels;
  m->D = p.dim + 1;
  if (device >= 0) {
    const int rc = gw_ovr_dev_alloc(m);
    if (rc != GW_OK) {
      g_ovr_err = m->err;
      gw_ovr_dev_free(m);
      delete m;
      return rc;
    }
  }
  *out = m;
  return GW_OK;
}

extern "C" int gw_ovr_free(gw_ovr* m) {
  if (!m) return GW_OK;
  if (m->device >= 0) gw_ovr_dev_free(m);
  delete m;
  return GW_OK;
}

extern "C" int gw_ovr_set_features(gw_ovr* m, const float* x, int64_t pitch) {
  if (!m) return gw_ovr_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!x || pitch < m->p.dim) return gw_ovr_fail(m, GW_ERR_INVALID, "NULL features or pitch below dim");
  m->x = x;
  m->pitch = pitch;
  m->have_x = true;
  m->fitted = false;
  return GW_OK;
}

extern "C" int gw_ovr_set_labels(gw_ovr* m, const int64_t* row_off, const int32_t* ids) {
  if (!m) return gw_ovr_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!row_off || row_off[0] != 0) return gw_ovr_fail(m, GW_ERR_INVALID, "row_off must start at 0");
  m->have_y = false;
  m->fitted = false;
  for (int64_t v = 0; v < m->n; ++v)
    if (row_off[v + 1] < row_off[v] || row_off[v + 1] - row_off[v] > m->L)
      return gw_ovr_fail(m, GW_ERR_INVALID, "row %lld: bad label count", (long long)v);
  const int64_t nnz = row_off[m->n];
  if (nnz > 0 && !ids) return gw_ovr_fail(m, GW_ERR_INVALID, "NULL ids");
  std::vector<uint8_t> seen((size_t)m->L, 0);
  for (int64_t v = 0; v < m->n; ++v) {
    for (int64_t e = row_off[v]; e < row_off[v + 1]; ++e) {
      if (ids[e] < 0 || ids[e] >= m->L)
        return gw_ovr_fail(m, GW_ERR_RANGE, "row %lld: label %d outside [0, %d)", (long long)v, (int)ids[e], m->L);
      if (seen[(size_t)ids[e]]) return gw_ovr_fail(m, GW_ERR_INVALID, "row %lld repeats label %d", (long long)v, (int)ids[e]);
      seen[(size_t)ids[e]] = 1;
    }
    for (int64_t e = row_off[v]; e < row_off[v + 1]; ++e) seen[(size_t)ids[e]] = 0;
  }
  m->row_off.assign(row_off, row_off + m->n + 1);
  m->ids.assign(ids, ids + nnz);
  if (m->device >= 0) {
    const int rc = gw_ovr_dev_upload_labels(m);
    if (rc != GW_OK) return rc;
  }
  m->have_y = true;
  return GW_OK;
}

extern "C" int gw_ovr_order(uint64_t seed, uint64_t shuffle, int64_t n, int64_t* order) {
  if (n < 0 || (n > 0 && !order) || n >= (int64_t)1 << 40) return gw_ovr_fail(nullptr, GW_ERR_INVALID, "bad arguments");
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < n; ++i) order[i] = (int64_t)gw_ovr_perm(seed, shuffle, (uint64_t)i, (uint64_t)n);
  return GW_OK;
}

// distinct rows inside [0, n)
static int check_rows(gw_ovr* m, const int64_t* rows, int64_t count, bool distinct) {
  if (count > 0 && !rows) return gw_ovr_fail(m, GW_ERR_INVALID, "NULL rows");
  std::vector<uint8_t> seen(distinct ? (size_t)m->n : 0, 0);
  for (int64_t i = 0; i < count; ++i) {
    const int64_t v = rows[i];
    if (v < 0 || v >= m->n)
      return gw_ovr_fail(m, GW_ERR_RANGE, "entry %lld: row %lld outside [0, %lld)", (long long)i, (long long)v,
                         (long long)m->n);
    if (distinct) {
      if (seen[(size_t)v]) return gw_ovr_fail(m, GW_ERR_INVALID, "entry %lld repeats row %lld", (long long)i, (long long)v);
      seen[(size_t)v] = 1;
    }
  }
  return GW_OK;
}

// ---- the law on the host -------------------------------------------------------
static double host_dot_row(const float* xr, const double* v, int d) {
  double t = 0.0;
  for (int j = 0; j < d; ++j) t = GW_OVR_FMA((double)xr[j], v[j], t);
  return t + v[d];
}

// one pass: q[l] for every running label; vec = {q, w, wt, g, sv, r, p}, each [L][D]
static void host_pass(const gw_ovr* m, const int64_t* rows, int64_t T, const uint8_t* y, double* z, double* Dd,
                      double* const vec[7], std::vector<double>* part) {
  const int L = m->L, D = m->D, d = D - 1;
  const int64_t nb = (T + GW_OVR_RB - 1) / GW_OVR_RB;
  std::vector<int> act;
  for (int l = 0; l < L; ++l)
    if (m->lab[(size_t)l].mode != GW_OVR_MODE_IDLE) act.push_back(l);
  const size_t na = act.size();
  part->resize((size_t)nb * na * (size_t)D);
#pragma omp parallel for schedule(dynamic, 1)
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t i0 = b * GW_OVR_RB;
    const int rn = (int)std::min<int64_t>(GW_OVR_RB, T - i0);
    double coef[GW_OVR_RB];
    for (size_t a = 0; a < na; ++a) {
      const int l = act[a], mode = m->lab[(size_t)l].mode;
      const double* v = (mode == GW_OVR_MODE_GRAD ? vec[2] : vec[6]) + (size_t)l * D;
      for (int r = 0; r < rn; ++r) {
        const float* xr = m->x + rows[i0 + r] * m->pitch;
        const size_t at = (size_t)(i0 + r) * L + l;
        coef[r] = gw_ovr_coef(mode, host_dot_row(xr, v, d), (double)y[at], &z[at], &Dd[at]);
      }
      double* pt = part->data() + ((size_t)b * na + a) * D;
      for (int j = 0; j < D; ++j) pt[j] = 0.0;
      for (int r = 0; r < rn; ++r) {
        const float* xr = m->x + rows[i0 + r] * m->pitch;
        const double c = coef[r];
        for (int j = 0; j < d; ++j) pt[j] = GW_OVR_FMA(c, (double)xr[j], pt[j]);
        pt[d] = pt[d] + c;
      }
    }
  }
  for (size_t a = 0; a < na; ++a) {
    double* q = vec[0] + (size_t)act[a] * D;
    for (int j = 0; j < D; ++j) q[j] = 0.0;
    for (int64_t b = 0; b < nb; ++b) {
      const double* pt = part->data() + ((size_t)b * na + a) * D;
      for (int j = 0; j < D; ++j) q[j] = q[j] + pt[j];
    }
  }
}

static int host_fit(gw_ovr* m, const int64_t* rows, int64_t T, const uint8_t* y, int64_t* passes) {
  const int L = m->L, D = m->D;
  const size_t LD = (size_t)L * D;
  std::vector<double> store(7 * LD, 0.0), z((size_t)T * L, 0.0), Dd((size_t)T * L, 0.0), part;
  double* vec[7];
  for (int t = 0; t < 7; ++t) vec[t] = store.data() + (size_t)t * LD;
  const gw_ovr_consts k = {m->p.C, m->p.gtol, m->p.max_newton, m->p.max_cg};
  for (;;) {
    bool any = false;
    for (int l = 0; l < L; ++l) any = any || m->lab[(size_t)l].mode != GW_OVR_MODE_IDLE;
    if (!any) break;
    host_pass(m, rows, T, y, z.data(), Dd.data(), vec, &part);
    *passes += 1;
#pragma omp parallel for schedule(dynamic, 1)
    for (int l = 0; l < L; ++l)
      if (m->lab[(size_t)l].mode != GW_OVR_MODE_IDLE) {
        const size_t o = (size_t)l * D;
        gw_ovr_label_step(&m->lab[(size_t)l], k, D, vec[0] + o, vec[1] + o, vec[2] + o, vec[3] + o, vec[4] + o,
                          vec[5] + o, vec[6] + o);
      }
  }
  m->W.assign(vec[1], vec[1] + LD);
  return GW_OK;
}

extern "C" int gw_ovr_fit(gw_ovr* m, const int64_t* order, int64_t train_count, gw_ovr_stats_t* stats, void* stream) {
  if (!m) return gw_ovr_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->have_x || !m->have_y)
    return gw_ovr_fail(m, GW_ERR_STATE, "call gw_ovr_set_features and gw_ovr_set_labels first");
  m->fitted = false;  // a failing fit leaves the handle unfitted
  if (train_count < 1 || train_count > m->n)
    return gw_ovr_fail(m, GW_ERR_INVALID, "train_count %lld outside [1, %lld]", (long long)train_count, (long long)m->n);
  int rc = check_rows(m, order, train_count, true);
  if (rc != GW_OK) return rc;
  const int L = m->L;
  const int64_t T = train_count;
  std::vector<uint8_t> y((size_t)T * L, 0);
  std::vector<int64_t> pos((size_t)L, 0);
  for (int64_t i = 0; i < T; ++i)
    for (int64_t e = m->row_off[(size_t)order[i]]; e < m->row_off[(size_t)order[i] + 1]; ++e) {
      y[(size_t)i * L + m->ids[(size_t)e]] = 1;
      pos[(size_t)m->ids[(size_t)e]] += 1;
    }
  m->lab.resize((size_t)L);
  for (int l = 0; l < L; ++l)
    gw_ovr_label_init(&m->lab[(size_t)l],
                      pos[(size_t)l] == 0 ? GW_OVR_CONST_NEG : (pos[(size_t)l] == T ? GW_OVR_CONST_POS : GW_OVR_RUNNING));
  int64_t passes = 0;
  rc = m->device < 0 ? host_fit(m, order, T, y.data(), &passes) : gw_ovr_dev_fit(m, order, T, y.data(), &passes, stream);
  if (rc != GW_OK) return rc;
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->passes = passes;
    for (int l = 0; l < L; ++l) {
      const gw_ovr_label& s = m->lab[(size_t)l];
      stats->fitted += s.state == GW_OVR_FITTED;
      stats->constant += s.state == GW_OVR_CONST_NEG || s.state == GW_OVR_CONST_POS;
      stats->not_converged += s.state == GW_OVR_NOT_CONVERGED;
      stats->newton_max = std::max(stats->newton_max, s.newton);
    }
  }
  m->fitted = true;
  return GW_OK;
}

static void host_decision(const gw_ovr* m, const int64_t* rows, int64_t count, double* z) {
  const int L = m->L, D = m->D;
  const double inf = std::numeric_limits<double>::infinity();
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < count; ++i) {
    const float* xr = m->x + rows[i] * m->pitch;
    for (int l = 0; l < L; ++l) {
      const int st = m->lab[(size_t)l].state;
      z[(size_t)i * L + l] = st == GW_OVR_CONST_NEG ? -inf
                             : st == GW_OVR_CONST_POS ? inf
                                                      : host_dot_row(xr, m->W.data() + (size_t)l * D, D - 1);
    }
  }
}

static int scoring_ready(gw_ovr* m, const int64_t* rows, int64_t count) {
  if (!m) return gw_ovr_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->fitted) return gw_ovr_fail(m, GW_ERR_STATE, "call gw_ovr_fit first");
  if (count < 0) return gw_ovr_fail(m, GW_ERR_INVALID, "negative count");
  return check_rows(m, rows, count, false);
}

extern "C" int gw_ovr_decision(gw_ovr* m, const int64_t* rows, int64_t count, double* z) {
  const int rc = scoring_ready(m, rows, count);
  if (rc != GW_OK) return rc;
  if (count > 0 && !z) return gw_ovr_fail(m, GW_ERR_INVALID, "NULL z");
  if (count == 0) return GW_OK;
  if (m->device >= 0) return gw_ovr_dev_decision(m, rows, count, z);
  host_decision(m, rows, count, z);
  return GW_OK;
}

extern "C" int gw_ovr_score(gw_ovr* m, const int64_t* rows, int64_t count, int64_t* counts, void* stream) {
  const int rc = scoring_ready(m, rows, count);
  if (rc != GW_OK) return rc;
  if (!counts) return gw_ovr_fail(m, GW_ERR_INVALID, "NULL counts");
  const int L = m->L;
  memset(counts, 0, (size_t)L * 3 * sizeof(int64_t));
  if (count == 0) return GW_OK;
  if (m->device >= 0) return gw_ovr_dev_score(m, rows, count, counts, stream);
  std::vector<double> z((size_t)count * L);
  host_decision(m, rows, count, z.data());
  std::vector<uint8_t> truth((size_t)L);
  for (int64_t i = 0; i < count; ++i) {
    const int64_t b = m->row_off[(size_t)rows[i]], e = m->row_off[(size_t)rows[i] + 1];
    std::fill(truth.begin(), truth.end(), 0);
    for (int64_t q = b; q < e; ++q) truth[(size_t)m->ids[(size_t)q]] = 1;
    for (int l = 0; l < L; ++l) {
      const int pred = gw_ovr_predicted(z.data() + (size_t)i * L, L, l, (int)(e - b));
      counts[(size_t)l * 3 + 0] += pred && truth[(size_t)l];
      counts[(size_t)l * 3 + 1] += pred && !truth[(size_t)l];
      counts[(size_t)l * 3 + 2] += !pred && truth[(size_t)l];
    }
  }
  return GW_OK;
}

extern "C" int gw_ovr_export(gw_ovr* m, double* W, int32_t* state, int32_t* newton_iters, double* gnorm) {
  if (!m) return gw_ovr_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->fitted) return gw_ovr_fail(m, GW_ERR_STATE, "call gw_ovr_fit first");
  if (W) memcpy(W, m->W.data(), m->W.size() * sizeof(double));
  for (int l = 0; l < m->L; ++l) {
    if (state) state[l] = m->lab[(size_t)l].state;
    if (newton_iters) newton_iters[l] = m->lab[(size_t)l].newton;
    if (gnorm) gnorm[l] = m->lab[(size_t)l].gnorm;
  }
  return GW_OK;
}
