// Spring layout: C ABI, the checks of the matrix and the arguments, and the host
// evaluation of the law (device = -1).  The law itself is gw_layout_law.h; the
// kernels are gw_layout.hip.
//
// This file depends on nothing but the C++ library, so that it also builds as
// a plain host program (-DGW_LAYOUT_HOST_ONLY: no device path) for sanitizer
// runs, as the other families' host files do.
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <new>

#include "gw_layout_internal.h"
#include "gw_trainer_fail.h"

static thread_local std::string g_layout_err;

int gw_layout_fail(gw_layout* m, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  gw_trainer_vfail(m ? &m->err : nullptr, &g_layout_err, code, fmt, ap);
  va_end(ap);
  return code;
}

#ifdef GW_LAYOUT_HOST_ONLY
static int no_dev(gw_layout* m) { return gw_layout_fail(m, GW_ERR_DEVICE, "built without the device path"); }
int gw_layout_dev_alloc(gw_layout* m) { return no_dev(m); }
void gw_layout_dev_free(gw_layout*) {}
int gw_layout_dev_upload(gw_layout* m) { return no_dev(m); }
int gw_layout_dev_upload_fixed(gw_layout* m) { return no_dev(m); }
int gw_layout_dev_run(gw_layout* m, double*, double, int32_t, double, void*, int32_t*) { return no_dev(m); }
int gw_layout_dev_step(gw_layout* m, const double*, double, double, double*, double*, void*) { return no_dev(m); }
int gw_layout_dev_rescale(gw_layout* m, double*, double, const double*, void*) { return no_dev(m); }
extern "C" int gw_layout_kernel_attrs(gw_layout* m, int, const char**, int32_t*, int32_t*, int32_t*, int32_t*) {
  return no_dev(m);
}
extern "C" int gw_layout_tiles(const gw_layout* m, int32_t*, int32_t*, int32_t*, int32_t*) {
  return no_dev(const_cast<gw_layout*>(m));
}
#endif

extern "C" const char* gw_layout_last_error(const gw_layout* m) { return m ? m->err.c_str() : g_layout_err.c_str(); }

extern "C" int gw_layout_create(int device, int64_t n, int dim, const gw_layout_params_t* params, gw_layout** out) {
  if (!out) return gw_layout_fail(nullptr, GW_ERR_INVALID, "NULL out");
  *out = nullptr;
  gw_layout_params_t p;
  memset(&p, 0, sizeof p);
  if (params) {
    if (params->struct_size < (int32_t)sizeof(int32_t))
      return gw_layout_fail(nullptr, GW_ERR_INVALID, "gw_layout_params_t.struct_size %d", (int)params->struct_size);
    memcpy(&p, params, std::min((size_t)params->struct_size, sizeof p));
  }
  p.struct_size = (int32_t)sizeof p;
  if (device < -1) return gw_layout_fail(nullptr, GW_ERR_INVALID, "device %d", device);
  if (n < 1 || n >= (int64_t)1 << 31)
    return gw_layout_fail(nullptr, GW_ERR_INVALID, "n %lld out of range", (long long)n);
  if (dim != 2 && dim != 3) return gw_layout_fail(nullptr, GW_ERR_INVALID, "dim %d: 2 or 3", dim);
  if (p.reserved != 0) return gw_layout_fail(nullptr, GW_ERR_INVALID, "reserved %d: must be 0", (int)p.reserved);
  gw_layout* m = new (std::nothrow) gw_layout();
  if (!m) return gw_layout_fail(nullptr, GW_ERR_NOMEM, "out of memory");
  m->device = device;
  m->n = n;
  m->dim = dim;
  m->p = p;
  m->fixed.assign((size_t)n, 0);
  if (device >= 0) {
    const int rc = gw_layout_dev_alloc(m);
    if (rc != GW_OK) {
      g_layout_err = m->err;
      gw_layout_dev_free(m);
      delete m;
      return rc;
    }
  }
  *out = m;
  return GW_OK;
}

extern "C" int gw_layout_free(gw_layout* m) {
  if (!m) return GW_OK;
  if (m->device >= 0) gw_layout_dev_free(m);
  delete m;
  return GW_OK;
}

// ---- the matrix ------------------------------------------------------------------
namespace {

// cnt(i): entries listed in row i; get(i, e, &id, &value)
template <class Cnt, class Get>
int assemble(gw_layout* m, Cnt cnt, Get get) {
  const int64_t n = m->n;
  m->have_graph = false;
  m->off.assign((size_t)n + 1, 0);
  m->col.clear();
  m->val.clear();
  for (int64_t i = 0; i < n; ++i) {
    const int64_t c = cnt(i);
    for (int64_t e = 0; e < c; ++e) {
      int32_t id;
      double v;
      get(i, e, &id, &v);
      if (id == -1) break;
      if (id < -1 || id >= n)
        return gw_layout_fail(m, GW_ERR_RANGE, "row %lld entry %lld: id %d outside [-1, %lld)", (long long)i,
                              (long long)e, (int)id, (long long)n);
      if (!(v - v == 0.0))
        return gw_layout_fail(m, GW_ERR_INVALID, "row %lld entry %lld: the value is not finite", (long long)i,
                              (long long)e);
      if (id == i) continue;
      m->col.push_back(id);
      m->val.push_back(v);
    }
    m->off[(size_t)i + 1] = (int64_t)m->col.size();
  }
  if (m->device >= 0) {
    const int rc = gw_layout_dev_upload(m);
    if (rc != GW_OK) return rc;
  }
  m->have_graph = true;
  return GW_OK;
}

}  // namespace

extern "C" int gw_layout_set_rows(gw_layout* m, const int32_t* ids, const double* values, int topk) {
  if (!m) return gw_layout_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!ids || !values || topk < 1) return gw_layout_fail(m, GW_ERR_INVALID, "NULL rows or topk below 1");
  return assemble(
      m, [topk](int64_t) { return (int64_t)topk; },
      [=](int64_t i, int64_t e, int32_t* id, double* v) {
        *id = ids[i * topk + e];
        *v = values[i * topk + e];
      });
}

extern "C" int gw_layout_set_csr(gw_layout* m, const int64_t* offsets, const int32_t* nbrs, const double* values) {
  if (!m) return gw_layout_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!offsets || (!nbrs && offsets[m->n] > 0)) return gw_layout_fail(m, GW_ERR_INVALID, "NULL offsets or nbrs");
  for (int64_t i = 0; i < m->n; ++i)
    if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) {
      m->have_graph = false;
      return gw_layout_fail(m, GW_ERR_INVALID, "offsets must not descend");
    }
  return assemble(
      m, [=](int64_t i) { return offsets[i + 1] - offsets[i]; },
      [=](int64_t i, int64_t e, int32_t* id, double* v) {
        *id = nbrs[offsets[i] + e];
        *v = values ? values[offsets[i] + e] : 1.0;
      });
}

extern "C" int gw_layout_set_fixed(gw_layout* m, const int32_t* ids, int64_t count) {
  if (!m) return gw_layout_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (count < 0 || (count > 0 && !ids)) return gw_layout_fail(m, GW_ERR_INVALID, "NULL ids or a negative count");
  for (int64_t r = 0; r < count; ++r)
    if (ids[r] < 0 || ids[r] >= m->n)
      return gw_layout_fail(m, GW_ERR_RANGE, "entry %lld: id %d outside [0, %lld)", (long long)r, (int)ids[r],
                            (long long)m->n);
  m->fixed.assign((size_t)m->n, 0);
  for (int64_t r = 0; r < count; ++r) m->fixed[(size_t)ids[r]] = 1;
  return m->device >= 0 ? gw_layout_dev_upload_fixed(m) : GW_OK;
}

// ---- the law on the host ---------------------------------------------------------
namespace {

// one iteration at temperature t: nxt = pos + step, disp (may be NULL), s[i] = the vertex's share of the norm
template <int DIM>
void host_iterate(const gw_layout* m, const double* pos, double k, double t, double* disp_out, double* nxt, double* s) {
  const int64_t n = m->n, chunks = gw_layout_chunks(n);
  const double kk = k * k;
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < n; ++i) {
    const double* pi = pos + i * DIM;
    double R[DIM], T[DIM], part[DIM], disp[DIM], step[DIM];
    for (int c = 0; c < DIM; ++c) R[c] = T[c] = 0.0;
    for (int64_t ch = 0; ch < chunks; ++ch) {
      const int64_t c0 = ch * GW_LAYOUT_CHUNK;
      gw_layout_chunk<DIM>(pi, pos + c0 * DIM, (int)std::min<int64_t>(GW_LAYOUT_CHUNK, n - c0), kk, part);
      for (int c = 0; c < DIM; ++c) R[c] = R[c] + part[c];
    }
    for (int64_t e = m->off[(size_t)i]; e < m->off[(size_t)i + 1]; ++e) {
      gw_layout_pull<DIM>(pi, pos + (int64_t)m->col[(size_t)e] * DIM, m->val[(size_t)e], k, part);
      for (int c = 0; c < DIM; ++c) T[c] = T[c] + part[c];
    }
    const double si = gw_layout_move<DIM>(R, T, t, m->fixed[(size_t)i], disp, step);
    if (s) s[i] = si;
    for (int c = 0; c < DIM; ++c) {
      if (disp_out) disp_out[i * DIM + c] = disp[c];
      nxt[i * DIM + c] = pi[c] + step[c];
    }
  }
}

double host_blocked_sum(const double* x, int64_t stride, int64_t n) {
  double total = 0.0;
  for (int64_t b = 0; b < gw_layout_blocks(n); ++b) total = total + gw_layout_block_sum(x, stride, b, n);
  return total;
}

template <int DIM>
int host_run(gw_layout* m, double* pos, double k, int32_t iterations, double threshold, int32_t* done) {
  const int64_t n = m->n;
  double mn[2] = {pos[0], pos[1]}, mx[2] = {pos[0], pos[1]};
  for (int64_t i = 1; i < n; ++i)
    for (int c = 0; c < 2; ++c) {
      const double x = pos[i * DIM + c];
      if (x < mn[c]) mn[c] = x;
      if (x > mx[c]) mx[c] = x;
    }
  double t = gw_layout_t0(mn[0], mx[0], mn[1], mx[1]);
  const double dt = t / (double)(iterations + 1);
  std::vector<double> nxt((size_t)(n * DIM)), s((size_t)n);
  int32_t it = 0;
  while (it < iterations) {
    host_iterate<DIM>(m, pos, k, t, nullptr, nxt.data(), s.data());
    memcpy(pos, nxt.data(), sizeof(double) * (size_t)(n * DIM));
    t = t - dt;
    ++it;
    if (gw_layout_stops(host_blocked_sum(s.data(), 1, n), n, threshold)) break;
  }
  if (done) *done = it;
  return GW_OK;
}

template <int DIM>
void host_rescale(const gw_layout* m, double* pos, double scale, const double* center) {
  const int64_t n = m->n;
  double lim = 0.0;
  for (int c = 0; c < DIM; ++c) {
    const double mean = host_blocked_sum(pos + c, DIM, n) / (double)n;
    for (int64_t i = 0; i < n; ++i) {
      const double v = pos[i * DIM + c] - mean;
      pos[i * DIM + c] = v;
      const double a = v < 0.0 ? -v : v;
      if (a > lim) lim = a;
    }
  }
  const double f = lim > 0.0 ? scale / lim : 1.0;
  for (int64_t i = 0; i < n; ++i)
    for (int c = 0; c < DIM; ++c) {
      const double v = lim > 0.0 ? pos[i * DIM + c] * f : pos[i * DIM + c];
      pos[i * DIM + c] = v + (center ? center[c] : 0.0);
    }
}

// k in use, or a failure
int resolve_k(gw_layout* m, double k, double* out) {
  if (!(k >= 0.0) || !(k - k == 0.0)) return gw_layout_fail(m, GW_ERR_INVALID, "k must be a finite number >= 0 (0: sqrt(1/n))");
  *out = k == 0.0 ? gw_layout_sqrt(1.0 / (double)m->n) : k;
  return GW_OK;
}

}  // namespace

extern "C" int gw_layout_run(gw_layout* m, double* pos, double k, int32_t iterations, double threshold, void* stream,
                             int32_t* iterations_done) {
  if (!m) return gw_layout_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (iterations_done) *iterations_done = 0;
  if (!m->have_graph) return gw_layout_fail(m, GW_ERR_STATE, "call gw_layout_set_rows or gw_layout_set_csr first");
  double ku;
  const int rc = resolve_k(m, k, &ku);
  if (rc != GW_OK) return rc;
  if (threshold != threshold) return gw_layout_fail(m, GW_ERR_INVALID, "threshold is NaN");
  if (iterations < 0) return gw_layout_fail(m, GW_ERR_INVALID, "iterations %d", (int)iterations);
  if (!pos) return gw_layout_fail(m, GW_ERR_INVALID, "NULL pos");
  if (iterations == 0) return GW_OK;
  if (m->device >= 0) return gw_layout_dev_run(m, pos, ku, iterations, threshold, stream, iterations_done);
  return m->dim == 2 ? host_run<2>(m, pos, ku, iterations, threshold, iterations_done)
                     : host_run<3>(m, pos, ku, iterations, threshold, iterations_done);
}

extern "C" int gw_layout_step(gw_layout* m, const double* pos_in, double k, double t, double* disp_out, double* pos_out,
                              void* stream) {
  if (!m) return gw_layout_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->have_graph) return gw_layout_fail(m, GW_ERR_STATE, "call gw_layout_set_rows or gw_layout_set_csr first");
  double ku;
  const int rc = resolve_k(m, k, &ku);
  if (rc != GW_OK) return rc;
  if (t != t) return gw_layout_fail(m, GW_ERR_INVALID, "t is NaN");
  if (!pos_in || !pos_out || pos_in == pos_out)
    return gw_layout_fail(m, GW_ERR_INVALID, "NULL positions, or pos_out is pos_in");
  if (m->device >= 0) return gw_layout_dev_step(m, pos_in, ku, t, disp_out, pos_out, stream);
  if (m->dim == 2) host_iterate<2>(m, pos_in, ku, t, disp_out, pos_out, nullptr);
  else host_iterate<3>(m, pos_in, ku, t, disp_out, pos_out, nullptr);
  return GW_OK;
}

extern "C" int gw_layout_rescale(gw_layout* m, double* pos, double scale, const double* center, void* stream) {
  if (!m) return gw_layout_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!pos) return gw_layout_fail(m, GW_ERR_INVALID, "NULL pos");
  if (scale != scale) return gw_layout_fail(m, GW_ERR_INVALID, "scale is NaN");
  if (m->device >= 0) return gw_layout_dev_rescale(m, pos, scale, center, stream);
  if (m->dim == 2) host_rescale<2>(m, pos, scale, center);
  else host_rescale<3>(m, pos, scale, center);
  return GW_OK;
}
