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

#include <algorithm>
#include <new>
#include <utility>
#include <vector>

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

static int check_rows(gw_nng* m, int device, int64_t n) {
  if (n < 1 || n >= (int64_t)1 << 40) return gw_nng_fail(m, GW_ERR_INVALID, "n %lld out of range", (long long)n);
  if (device >= 0 && n >= (int64_t)1 << 31)
    return gw_nng_fail(m, GW_ERR_UNSUPPORTED, "n %lld: the kernels take n < 2^31 (device = -1 takes any)", (long long)n);
  return GW_OK;
}

extern "C" int gw_nng_create(int device, int64_t n, const gw_nng_params_t* params, gw_nng** out) {
  if (!out) return gw_nng_fail(nullptr, GW_ERR_INVALID, "NULL out");
  *out = nullptr;
  gw_nng_params_t p;
  memset(&p, 0, sizeof p);
  p.dim = 3;
  p.topk = 10;
  p.include_self = 1;
  p.heat_t = 0.0;
  if (params) {
    if (params->struct_size < (int32_t)sizeof(int32_t))
      return gw_nng_fail(nullptr, GW_ERR_INVALID, "gw_nng_params_t.struct_size %d", (int)params->struct_size);
    memcpy(&p, params, std::min((size_t)params->struct_size, sizeof p));
  }
  p.struct_size = (int32_t)sizeof p;
  if (p.dim < 1 || p.topk < 1) return gw_nng_fail(nullptr, GW_ERR_INVALID, "dim %d and topk %d must be positive", p.dim, p.topk);
  if (p.include_self != 0 && p.include_self != 1) return gw_nng_fail(nullptr, GW_ERR_INVALID, "include_self %d", p.include_self);
  if (!(p.heat_t >= 0.0)) return gw_nng_fail(nullptr, GW_ERR_INVALID, "heat_t must be a number >= 0 (0: unit weights)");
  if (device < -1) return gw_nng_fail(nullptr, GW_ERR_INVALID, "device %d", device);
  int rc = check_rows(nullptr, device, n);
  if (rc != GW_OK) return rc;
  if (device >= 0 && (p.dim > GW_NNG_MAX_DIM || p.topk > GW_NNG_MAX_TOPK))
    return gw_nng_fail(nullptr, GW_ERR_UNSUPPORTED, "dim %d / topk %d: the kernels take dim <= %d and topk <= %d "
                       "(device = -1 takes any)", p.dim, p.topk, GW_NNG_MAX_DIM, GW_NNG_MAX_TOPK);
  gw_nng* m = new (std::nothrow) gw_nng();
  if (!m) return gw_nng_fail(nullptr, GW_ERR_NOMEM, "out of memory");
  m->device = device;
  m->p = p;
  m->n = n;
  if (device >= 0) {
    rc = gw_nng_dev_alloc(m);
    if (rc != GW_OK) {
      g_nng_err = m->err;
      gw_nng_dev_free(m);
      delete m;
      return rc;
    }
  }
  *out = m;
  return GW_OK;
}

extern "C" int gw_nng_free(gw_nng* m) {
  if (!m) return GW_OK;
  if (m->device >= 0) gw_nng_dev_free(m);
  delete m;
  return GW_OK;
}

extern "C" int gw_nng_set_rows(gw_nng* m, int64_t n) {
  if (!m) return gw_nng_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  const int rc = check_rows(m, m->device, n);
  if (rc != GW_OK) return rc;
  m->n = n;
  m->have_x = false;  // the vectors set before had another row count
  return GW_OK;
}

extern "C" int gw_nng_set_vectors(gw_nng* m, const float* x, int64_t pitch) {
  if (!m) return gw_nng_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!x || pitch < m->p.dim) return gw_nng_fail(m, GW_ERR_INVALID, "NULL vectors or pitch below dim");
  m->x = x;
  m->pitch = pitch;
  m->have_x = true;
  return GW_OK;
}

// ---- the law on the host -------------------------------------------------------
static void host_query(const gw_nng* m, const int32_t* sources, int64_t nsrc, int32_t* out_ids, double* out_weights,
                       double* out_d2) {
  const int dim = m->p.dim;
  const int64_t n = m->n, topk = m->p.topk, self = m->p.include_self;
  const double heat_t = m->p.heat_t;
  const auto before = [](const std::pair<double, int32_t>& a, const std::pair<double, int32_t>& b) {
    return gw_nng_before(a.first, a.second, b.first, b.second) != 0;
  };
#pragma omp parallel
  {
    std::vector<std::pair<double, int32_t>> cand;
#pragma omp for schedule(dynamic, 8)
    for (int64_t r = 0; r < nsrc; ++r) {
      const int64_t v = sources ? sources[r] : r;
      const float* xv = m->x + v * m->pitch;
      cand.clear();
      if (topk > self)
        for (int64_t j = 0; j < n; ++j) {
          if (j == v) continue;
          const double d2 = gw_nng_d2(xv, m->x + j * m->pitch, dim);
          if (gw_nng_listed(d2)) cand.emplace_back(d2, (int32_t)j);
        }
      const size_t keep = std::min<size_t>(cand.size(), (size_t)(topk - self));
      std::partial_sort(cand.begin(), cand.begin() + (ptrdiff_t)keep, cand.end(), before);
      for (int64_t t = 0; t < topk; ++t) {
        int32_t id = -1;
        double d2 = 0.0, w = 0.0;
        if (self && t == 0) {
          id = (int32_t)v;
          w = 1.0;
        } else if ((size_t)(t - self) < keep) {
          id = cand[(size_t)(t - self)].second;
          d2 = cand[(size_t)(t - self)].first;
          w = gw_nng_weight(d2, heat_t);
        }
        out_ids[r * topk + t] = id;
        out_weights[r * topk + t] = w;
        if (out_d2) out_d2[r * topk + t] = d2;
      }
    }
  }
}

extern "C" int gw_nng_query(gw_nng* m, const int32_t* sources, int64_t nsrc, int32_t* out_ids, double* out_weights,
                            double* out_d2, void* stream) {
  if (!m) return gw_nng_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->have_x) return gw_nng_fail(m, GW_ERR_STATE, "call gw_nng_set_vectors first");
  if (!sources) nsrc = m->n;
  if (nsrc < 0) return gw_nng_fail(m, GW_ERR_INVALID, "negative nsrc");
  if (nsrc == 0) return GW_OK;
  if (!out_ids || !out_weights) return gw_nng_fail(m, GW_ERR_INVALID, "NULL output");
  if (m->device >= 0) return gw_nng_dev_query(m, sources, nsrc, out_ids, out_weights, out_d2, stream);
  if (sources)
    for (int64_t r = 0; r < nsrc; ++r)
      if (sources[r] < 0 || sources[r] >= m->n)
        return gw_nng_fail(m, GW_ERR_RANGE, "entry %lld: source %d outside [0, %lld)", (long long)r, (int)sources[r],
                           (long long)m->n);
  host_query(m, sources, nsrc, out_ids, out_weights, out_d2);
  return GW_OK;
}
