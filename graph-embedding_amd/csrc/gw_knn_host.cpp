// Nearest neighbours of an embedding: C ABI, argument checks, the host
// evaluation of the law (device = -1) and gw_topk_label_agreement.  The law
// itself is gw_knn_law.h; the kernels are gw_knn.hip.
//
// This file depends on nothing but the C++ library, so that it also builds as
// a plain host program (-DGW_KNN_HOST_ONLY: no device path) for sanitizer
// runs (host/knn_host_check.cpp).
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <utility>
#include <vector>

#include "gw_knn_internal.h"
#include "gw_trainer_fail.h"

static thread_local std::string g_knn_err;

int gw_knn_fail(gw_knn* m, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  gw_trainer_vfail(m ? &m->err : nullptr, &g_knn_err, code, fmt, ap);
  va_end(ap);
  return code;
}

#ifdef GW_KNN_HOST_ONLY
static int no_dev(gw_knn* m) { return gw_knn_fail(m, GW_ERR_DEVICE, "built without the device path"); }
int gw_knn_dev_alloc(gw_knn* m) { return no_dev(m); }
void gw_knn_dev_free(gw_knn*) {}
int gw_knn_dev_query(gw_knn* m, const int32_t*, int64_t, int32_t*, double*, void*) { return no_dev(m); }
extern "C" int gw_knn_kernel_attrs(gw_knn* m, int, const char**, int32_t*, int32_t*, int32_t*, int32_t*) {
  return no_dev(m);
}
extern "C" int gw_knn_tiles(const gw_knn* m, int32_t*, int32_t*, int32_t*, int32_t*) {
  return no_dev(const_cast<gw_knn*>(m));
}
extern "C" int gw_knn_fma_rate(gw_knn* m, int, int, double*) { return no_dev(m); }
#endif

extern "C" const char* gw_knn_last_error(const gw_knn* m) { return m ? m->err.c_str() : g_knn_err.c_str(); }

extern "C" int gw_knn_create(int device, int64_t n, const gw_knn_params_t* params, gw_knn** out) {
  if (!out) return gw_knn_fail(nullptr, GW_ERR_INVALID, "NULL out");
  *out = nullptr;
  gw_knn_params_t p;
  memset(&p, 0, sizeof p);
  p.dim = 128;
  p.topk = 20;
  p.metric = GW_KNN_COSINE;
  const int rc = gw_pairs_read_params<gw_knn>(params, &p, "gw_knn_params_t");
  if (rc != GW_OK) return rc;
  if (p.dim < 1 || p.topk < 1) return gw_knn_fail(nullptr, GW_ERR_INVALID, "dim %d and topk %d must be positive", p.dim, p.topk);
  if (p.metric != GW_KNN_COSINE && p.metric != GW_KNN_DOT) return gw_knn_fail(nullptr, GW_ERR_INVALID, "metric %d", p.metric);
  return gw_pairs_create(device, n, p, GW_KNN_MAX_DIM, GW_KNN_MAX_TOPK, gw_knn_dev_alloc, gw_knn_dev_free, &g_knn_err, out);
}

extern "C" int gw_knn_free(gw_knn* m) {
  if (!m) return GW_OK;
  if (m->device >= 0) gw_knn_dev_free(m);
  delete m;
  return GW_OK;
}

extern "C" int gw_knn_set_rows(gw_knn* m, int64_t n) { return gw_pairs_set_rows(m, n); }

extern "C" int gw_knn_set_vectors(gw_knn* m, const float* x, int64_t pitch) { return gw_pairs_set_vectors(m, x, pitch); }

// ---- the law on the host -------------------------------------------------------
namespace {
struct HostLaw {
  const gw_knn* m;
  const double* nrm;  // [n] under GW_KNN_COSINE
  int64_t keep;
  int32_t* out_ids;
  double* out_scores;
  bool score(int64_t v, int64_t j, double* s) const {
    const int metric = m->p.metric;
    const double nv = metric == GW_KNN_COSINE ? nrm[v] : 0.0, nj = metric == GW_KNN_COSINE ? nrm[j] : 0.0;
    *s = gw_knn_score(metric, gw_knn_dot(m->x + v * m->pitch, m->x + j * m->pitch, m->p.dim), nv, nj);
    return gw_knn_listed(metric, *s, nv, nj) != 0;
  }
  static int before(double sa, int32_t ia, double sb, int32_t ib) { return gw_knn_before(sa, ia, sb, ib); }
  void write_row(int64_t r, int64_t, const std::pair<double, int32_t>* cand, size_t kept) const {
    const int64_t topk = m->p.topk;
    for (int64_t t = 0; t < topk; ++t) {
      out_ids[r * topk + t] = (size_t)t < kept ? cand[t].second : -1;
      out_scores[r * topk + t] = (size_t)t < kept ? cand[t].first : 0.0;
    }
  }
};
}  // namespace

static void host_query(const gw_knn* m, const int32_t* sources, int64_t nsrc, int32_t* out_ids, double* out_scores) {
  const int64_t n = m->n;
  std::vector<double> nrm;
  if (m->p.metric == GW_KNN_COSINE) {
    nrm.resize((size_t)n);
#pragma omp parallel for schedule(static)
    for (int64_t j = 0; j < n; ++j) nrm[(size_t)j] = gw_knn_nrm(m->x + j * m->pitch, m->p.dim);
  }
  gw_pairs_host_rows(HostLaw{m, nrm.data(), m->p.topk, out_ids, out_scores}, n, sources, nsrc);
}

extern "C" int gw_knn_query(gw_knn* m, const int32_t* sources, int64_t nsrc, int32_t* out_ids, double* out_scores,
                            void* stream) {
  if (!m) return gw_knn_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->have_x) return gw_knn_fail(m, GW_ERR_STATE, "call gw_knn_set_vectors first");
  if (!sources) nsrc = m->n;
  if (nsrc < 0) return gw_knn_fail(m, GW_ERR_INVALID, "negative nsrc");
  if (nsrc == 0) return GW_OK;
  if (!out_ids || !out_scores) return gw_knn_fail(m, GW_ERR_INVALID, "NULL output");
  if (m->device >= 0) return gw_knn_dev_query(m, sources, nsrc, out_ids, out_scores, stream);
  const int rc = gw_pairs_check_sources(m, sources, nsrc);
  if (rc != GW_OK) return rc;
  host_query(m, sources, nsrc, out_ids, out_scores);
  return GW_OK;
}

extern "C" int gw_topk_label_agreement(const int32_t* ids, int64_t nrows, int topk, const int32_t* row_ids,
                                       const int64_t* lab_off, const int32_t* lab_ids, int64_t n, double* acc) {
  if (nrows < 0 || topk < 1 || n < 0 || !acc || (nrows > 0 && !ids) || !lab_off)
    return gw_knn_fail(nullptr, GW_ERR_INVALID, "bad arguments");
  if (lab_off[n] > 0 && !lab_ids) return gw_knn_fail(nullptr, GW_ERR_INVALID, "NULL lab_ids");
  std::vector<int64_t> hit((size_t)topk, 0), seen((size_t)topk, 0);  // per position t: neighbours there, and those that agree
  for (int64_t r = 0; r < nrows; ++r) {
    const int64_t v = row_ids ? row_ids[r] : r;
    if (v < 0 || v >= n) return gw_knn_fail(nullptr, GW_ERR_RANGE, "row %lld: vertex %lld outside [0, %lld)", (long long)r,
                                             (long long)v, (long long)n);
    for (int t = 0; t < topk; ++t) {
      const int64_t j = ids[r * topk + t];
      if (j == -1) break;  // padding ends the row
      if (j < 0 || j >= n) return gw_knn_fail(nullptr, GW_ERR_RANGE, "row %lld: id %lld outside [-1, %lld)", (long long)r,
                                               (long long)j, (long long)n);
      // two ascending label lists: do they meet?
      int64_t a = lab_off[v], b = lab_off[j];
      bool common = false;
      while (a < lab_off[v + 1] && b < lab_off[j + 1]) {
        if (lab_ids[a] == lab_ids[b]) {
          common = true;
          break;
        }
        if (lab_ids[a] < lab_ids[b]) ++a; else ++b;
      }
      seen[(size_t)t] += 1;
      hit[(size_t)t] += common ? 1 : 0;
    }
  }
  int64_t s = 0, h = 0;
  for (int t = 0; t < topk; ++t) {  // the first min(t + 1, listed) neighbours of every row
    s += seen[(size_t)t];
    h += hit[(size_t)t];
    acc[t] = s ? (double)h / (double)s : 0.0;
  }
  return GW_OK;
}
