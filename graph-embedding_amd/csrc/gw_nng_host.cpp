// Neighbour graph of points: C ABI, argument checks and the host evaluation of
// the law (device = -1).  The law itself is gw_nng_law.h; the kernels are
// gw_nng.hip.
//
// This file depends on nothing but the C++ library, so that it also builds as
// a plain host program (-DGW_NNG_HOST_ONLY: no device path) for sanitizer
// runs (host/nng_host_check.cpp).
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <utility>

#include "gw_nng_internal.h"
#include "gw_trainer_fail.h"

static thread_local std::string g_nng_err;

int gw_nng_fail(gw_nng* m, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  gw_trainer_vfail(m ? &m->err : nullptr, &g_nng_err, code, fmt, ap);
  va_end(ap);
  return code;
}

#ifdef GW_NNG_HOST_ONLY
static int no_dev(gw_nng* m) { return gw_nng_fail(m, GW_ERR_DEVICE, "built without the device path"); }
int gw_nng_dev_alloc(gw_nng* m) { return no_dev(m); }
void gw_nng_dev_free(gw_nng*) {}
int gw_nng_dev_query(gw_nng* m, const int32_t*, int64_t, int32_t*, double*, double*, void*) { return no_dev(m); }
extern "C" int gw_nng_kernel_attrs(gw_nng* m, int, const char**, int32_t*, int32_t*, int32_t*, int32_t*) {
  return no_dev(m);
}
extern "C" int gw_nng_tiles(const gw_nng* m, int32_t*, int32_t*, int32_t*, int32_t*) {
  return no_dev(const_cast<gw_nng*>(m));
}
#endif

extern "C" const char* gw_nng_last_error(const gw_nng* m) { return m ? m->err.c_str() : g_nng_err.c_str(); }

extern "C" int gw_nng_create(int device, int64_t n, const gw_nng_params_t* params, gw_nng** out) {
  if (!out) return gw_nng_fail(nullptr, GW_ERR_INVALID, "NULL out");
  *out = nullptr;
  gw_nng_params_t p;
  memset(&p, 0, sizeof p);
  p.dim = 3;
  p.topk = 10;
  p.include_self = 1;
  p.heat_t = 0.0;
  const int rc = gw_pairs_read_params<gw_nng>(params, &p, "gw_nng_params_t");
  if (rc != GW_OK) return rc;
  if (p.dim < 1 || p.topk < 1) return gw_nng_fail(nullptr, GW_ERR_INVALID, "dim %d and topk %d must be positive", p.dim, p.topk);
  if (p.include_self != 0 && p.include_self != 1) return gw_nng_fail(nullptr, GW_ERR_INVALID, "include_self %d", p.include_self);
  if (!(p.heat_t >= 0.0)) return gw_nng_fail(nullptr, GW_ERR_INVALID, "heat_t must be a number >= 0 (0: unit weights)");
  return gw_pairs_create(device, n, p, GW_NNG_MAX_DIM, GW_NNG_MAX_TOPK, gw_nng_dev_alloc, gw_nng_dev_free, &g_nng_err, out);
}

extern "C" int gw_nng_free(gw_nng* m) {
  if (!m) return GW_OK;
  if (m->device >= 0) gw_nng_dev_free(m);
  delete m;
  return GW_OK;
}

extern "C" int gw_nng_set_rows(gw_nng* m, int64_t n) { return gw_pairs_set_rows(m, n); }

extern "C" int gw_nng_set_vectors(gw_nng* m, const float* x, int64_t pitch) { return gw_pairs_set_vectors(m, x, pitch); }

// ---- the law on the host -------------------------------------------------------
namespace {
struct HostLaw {
  const gw_nng* m;
  int64_t keep;  // others listed per row
  int32_t* out_ids;
  double* out_weights;
  double* out_d2;  // may be NULL
  bool score(int64_t v, int64_t j, double* s) const {
    *s = gw_nng_d2(m->x + v * m->pitch, m->x + j * m->pitch, m->p.dim);
    return gw_nng_listed(*s) != 0;
  }
  static int before(double da, int32_t ia, double db, int32_t ib) { return gw_nng_before(da, ia, db, ib); }
  void write_row(int64_t r, int64_t v, const std::pair<double, int32_t>* cand, size_t kept) const {
    const int64_t topk = m->p.topk, self = m->p.include_self;
    for (int64_t t = 0; t < topk; ++t) {
      int32_t id = -1;
      double d2 = 0.0, w = 0.0;
      if (self && t == 0) {
        id = (int32_t)v;
        w = 1.0;
      } else if ((size_t)(t - self) < kept) {
        id = cand[t - self].second;
        d2 = cand[t - self].first;
        w = gw_nng_weight(d2, m->p.heat_t);
      }
      out_ids[r * topk + t] = id;
      out_weights[r * topk + t] = w;
      if (out_d2) out_d2[r * topk + t] = d2;
    }
  }
};
}  // namespace

extern "C" int gw_nng_query(gw_nng* m, const int32_t* sources, int64_t nsrc, int32_t* out_ids, double* out_weights,
                            double* out_d2, void* stream) {
  if (!m) return gw_nng_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->have_x) return gw_nng_fail(m, GW_ERR_STATE, "call gw_nng_set_vectors first");
  if (!sources) nsrc = m->n;
  if (nsrc < 0) return gw_nng_fail(m, GW_ERR_INVALID, "negative nsrc");
  if (nsrc == 0) return GW_OK;
  if (!out_ids || !out_weights) return gw_nng_fail(m, GW_ERR_INVALID, "NULL output");
  if (m->device >= 0) return gw_nng_dev_query(m, sources, nsrc, out_ids, out_weights, out_d2, stream);
  const int rc = gw_pairs_check_sources(m, sources, nsrc);
  if (rc != GW_OK) return rc;
  gw_pairs_host_rows(HostLaw{m, m->p.topk - m->p.include_self, out_ids, out_weights, out_d2}, m->n, sources, nsrc);
  return GW_OK;
}
