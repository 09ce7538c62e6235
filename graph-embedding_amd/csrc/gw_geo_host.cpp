// Geodesics on a sparse graph: C ABI, the assembly of the graph, the union-find,
// the argument checks and the host evaluation of the law (device = -1).  The law
// itself is gw_geo_law.h; the kernels are gw_geo.hip.
//
// This file depends on nothing but the C++ library, so that it also builds as
// a plain host program (-DGW_GEO_HOST_ONLY: no device path) for sanitizer
// runs, as the other families' host files do.
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <new>
#include <utility>

#include "gw_geo_internal.h"
#include "gw_trainer_fail.h"

static thread_local std::string g_geo_err;

int gw_geo_fail(gw_geo* m, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  gw_trainer_vfail(m ? &m->err : nullptr, &g_geo_err, code, fmt, ap);
  va_end(ap);
  return code;
}

#ifdef GW_GEO_HOST_ONLY
static int no_dev(gw_geo* m) { return gw_geo_fail(m, GW_ERR_DEVICE, "built without the device path"); }
int gw_geo_dev_alloc(gw_geo* m) { return no_dev(m); }
void gw_geo_dev_free(gw_geo*) {}
int gw_geo_dev_upload(gw_geo* m) { return no_dev(m); }
int gw_geo_dev_query(gw_geo* m, const int32_t*, int64_t, double*, int64_t, void*) { return no_dev(m); }
extern "C" int gw_geo_kernel_attrs(gw_geo* m, int, const char**, int32_t*, int32_t*, int32_t*, int32_t*) {
  return no_dev(m);
}
extern "C" int gw_geo_tiles(const gw_geo* m, int32_t*, int32_t*, int32_t*) { return no_dev(const_cast<gw_geo*>(m)); }
#endif

extern "C" const char* gw_geo_last_error(const gw_geo* m) { return m ? m->err.c_str() : g_geo_err.c_str(); }

extern "C" int gw_geo_create(int device, int64_t n, const gw_geo_params_t* params, gw_geo** out) {
  if (!out) return gw_geo_fail(nullptr, GW_ERR_INVALID, "NULL out");
  *out = nullptr;
  gw_geo_params_t p;
  memset(&p, 0, sizeof p);
  p.symmetrize = GW_GEO_SYM_UNION;
  if (params) {
    if (params->struct_size < (int32_t)sizeof(int32_t))
      return gw_geo_fail(nullptr, GW_ERR_INVALID, "gw_geo_params_t.struct_size %d", (int)params->struct_size);
    memcpy(&p, params, std::min((size_t)params->struct_size, sizeof p));
  }
  p.struct_size = (int32_t)sizeof p;
  if (device < -1) return gw_geo_fail(nullptr, GW_ERR_INVALID, "device %d", device);
  if (n < 1 || n >= (int64_t)1 << 31) return gw_geo_fail(nullptr, GW_ERR_INVALID, "n %lld out of range", (long long)n);
  if (p.symmetrize != GW_GEO_SYM_UNION && p.symmetrize != GW_GEO_DIRECTED)
    return gw_geo_fail(nullptr, GW_ERR_INVALID, "symmetrize %d", p.symmetrize);
  if (p.squared != 0 && p.squared != 1) return gw_geo_fail(nullptr, GW_ERR_INVALID, "squared %d", p.squared);
  if (p.round_cap < 0) return gw_geo_fail(nullptr, GW_ERR_INVALID, "round_cap %d", p.round_cap);
  if (!(p.delta >= 0.0)) return gw_geo_fail(nullptr, GW_ERR_INVALID, "delta must be a number >= 0 (0: chosen)");
  gw_geo* m = new (std::nothrow) gw_geo();
  if (!m) return gw_geo_fail(nullptr, GW_ERR_NOMEM, "out of memory");
  m->device = device;
  m->n = n;
  m->p = p;
  m->cap = p.round_cap > 0 ? p.round_cap - 1 : -1;
  if (device >= 0) {
    const int rc = gw_geo_dev_alloc(m);
    if (rc != GW_OK) {
      g_geo_err = m->err;
      gw_geo_dev_free(m);
      delete m;
      return rc;
    }
  }
  *out = m;
  return GW_OK;
}

extern "C" int gw_geo_free(gw_geo* m) {
  if (!m) return GW_OK;
  if (m->device >= 0) gw_geo_dev_free(m);
  delete m;
  return GW_OK;
}

// ---- assembly ------------------------------------------------------------------
namespace {

struct Tri {
  int32_t r, c;
  double l;
};

int32_t uf_find(std::vector<int32_t>& parent, int32_t v) {
  while (parent[(size_t)v] != v) {
    parent[(size_t)v] = parent[(size_t)parent[(size_t)v]];
    v = parent[(size_t)v];
  }
  return v;
}

// cnt(i): entries listed in row i; get(i, e, &id, &value)
template <class Cnt, class Get>
int assemble(gw_geo* m, Cnt cnt, Get get) {
  const int64_t n = m->n;
  const bool both = m->p.symmetrize == GW_GEO_SYM_UNION;
  m->have_graph = false;
  std::vector<Tri> t;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t c = cnt(i);
    for (int64_t e = 0; e < c; ++e) {
      int32_t id;
      double v;
      get(i, e, &id, &v);
      if (id == -1) break;
      if (id < -1 || id >= n)
        return gw_geo_fail(m, GW_ERR_RANGE, "row %lld entry %lld: id %d outside [-1, %lld)", (long long)i, (long long)e,
                           (int)id, (long long)n);
      if (id == i || !gw_geo_listed(v)) continue;
      const double l = gw_geo_length(v, m->p.squared);
      t.push_back(Tri{(int32_t)i, id, l});
      if (both) t.push_back(Tri{id, (int32_t)i, l});
    }
  }
  // a repeated (row, column) keeps the smallest length: it sorts first
  std::sort(t.begin(), t.end(), [](const Tri& a, const Tri& b) {
    return a.r != b.r ? a.r < b.r : a.c != b.c ? a.c < b.c : a.l < b.l;
  });
  m->off.assign((size_t)n + 1, 0);
  m->col.clear();
  m->len.clear();
  std::vector<int32_t> parent((size_t)n);
  for (int64_t i = 0; i < n; ++i) parent[(size_t)i] = (int32_t)i;
  double sum = 0.0;
  for (size_t k = 0; k < t.size(); ++k) {
    if (k && t[k].r == t[k - 1].r && t[k].c == t[k - 1].c) continue;
    m->col.push_back(t[k].c);
    m->len.push_back(t[k].l);
    ++m->off[(size_t)t[k].r + 1];
    sum += t[k].l;
    const int32_t a = uf_find(parent, t[k].r), b = uf_find(parent, t[k].c);
    if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);  // the root is the component's lowest vertex
  }
  for (int64_t i = 0; i < n; ++i) m->off[(size_t)i + 1] += m->off[(size_t)i];
  // components: ids, count, the largest (lowest id first, so ties go to it)
  m->comp.assign((size_t)n, 0);
  std::vector<int64_t> size((size_t)n, 0);
  for (int64_t i = 0; i < n; ++i) ++size[(size_t)(m->comp[(size_t)i] = uf_find(parent, (int32_t)i))];
  m->st = gw_geo_stats_t{};
  m->st.entries = (int64_t)m->col.size();
  m->main_comp = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (size[(size_t)i] > 0) ++m->st.components;
    if (size[(size_t)i] > size[(size_t)m->main_comp]) m->main_comp = (int32_t)i;
  }
  m->st.main_component_size = size[(size_t)m->main_comp];
  // the device schedule's bucket width: the caller's, or four mean edge lengths (a bucket then spans a few hops,
  // so a round's barriers are shared by several; measured in DESIGN.md §18).  It never changes a result.
  const double mean = m->col.empty() ? 0.0 : sum / (double)m->col.size();
  m->delta = m->p.delta > 0.0 ? m->p.delta : (mean > 0.0 && mean < __builtin_inf() ? 4.0 * mean : 1.0);
  if (m->device >= 0) {
    const int rc = gw_geo_dev_upload(m);
    if (rc != GW_OK) return rc;
  }
  m->have_graph = true;
  return GW_OK;
}

}  // namespace

extern "C" int gw_geo_set_rows(gw_geo* m, const int32_t* ids, const double* values, int topk) {
  if (!m) return gw_geo_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!ids || !values || topk < 1) return gw_geo_fail(m, GW_ERR_INVALID, "NULL rows or topk below 1");
  return assemble(
      m, [topk](int64_t) { return (int64_t)topk; },
      [=](int64_t i, int64_t e, int32_t* id, double* v) {
        *id = ids[i * topk + e];
        *v = values[i * topk + e];
      });
}

extern "C" int gw_geo_set_csr(gw_geo* m, const int64_t* offsets, const int32_t* nbrs, const double* values) {
  if (!m) return gw_geo_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!offsets || (!nbrs && offsets[m->n] > 0)) return gw_geo_fail(m, GW_ERR_INVALID, "NULL offsets or nbrs");
  for (int64_t i = 0; i < m->n; ++i)
    if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) {
      m->have_graph = false;
      return gw_geo_fail(m, GW_ERR_INVALID, "offsets must not descend");
    }
  return assemble(
      m, [=](int64_t i) { return offsets[i + 1] - offsets[i]; },
      [=](int64_t i, int64_t e, int32_t* id, double* v) {
        *id = nbrs[offsets[i] + e];
        *v = values ? values[offsets[i] + e] : 1.0;
      });
}

extern "C" int gw_geo_components(gw_geo* m, int32_t* component_of, int32_t* main_component) {
  if (!m) return gw_geo_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->have_graph) return gw_geo_fail(m, GW_ERR_STATE, "call gw_geo_set_rows or gw_geo_set_csr first");
  if (component_of) memcpy(component_of, m->comp.data(), sizeof(int32_t) * (size_t)m->n);
  if (main_component) *main_component = m->main_comp;
  return GW_OK;
}

extern "C" int gw_geo_stats(gw_geo* m, gw_geo_stats_t* stats) {
  if (!m || !stats) return gw_geo_fail(m, GW_ERR_INVALID, "NULL handle or stats");
  if (!m->have_graph) return gw_geo_fail(m, GW_ERR_STATE, "call gw_geo_set_rows or gw_geo_set_csr first");
  *stats = m->st;
  return GW_OK;
}

// ---- the law on the host: binary-heap Dijkstra per source ------------------------
namespace {

int64_t host_source(const gw_geo* m, int64_t s, double* row) {
  using item = std::pair<unsigned long long, int32_t>;  // (distance bits, vertex): the bits order as the distances
  const int64_t n = m->n;
  const double inf = __builtin_inf();
  for (int64_t v = 0; v < n; ++v) row[v] = inf;
  row[s] = 0.0;
  std::vector<item> heap{item{0ull, (int32_t)s}};
  int64_t relaxed = 0;
  while (!heap.empty()) {
    std::pop_heap(heap.begin(), heap.end(), std::greater<item>());
    const item top = heap.back();
    heap.pop_back();
    const int64_t u = top.second;
    if (top.first != gw_geo_bits(row[u])) continue;  // an entry a later improvement made stale
    for (int64_t e = m->off[(size_t)u]; e < m->off[(size_t)u + 1]; ++e) {
      const int32_t v = m->col[(size_t)e];
      const unsigned long long nd = gw_geo_relax(top.first, m->len[(size_t)e]);
      ++relaxed;
      if (nd < gw_geo_bits(row[v])) {  // the +inf pattern of an overflowing sum improves nothing
        row[v] = gw_geo_double(nd);
        heap.push_back(item{nd, v});
        std::push_heap(heap.begin(), heap.end(), std::greater<item>());
      }
    }
  }
  return relaxed;
}

}  // namespace

extern "C" int gw_geo_query(gw_geo* m, const int32_t* sources, int64_t nsrc, double* out, int64_t pitch, void* stream) {
  if (!m) return gw_geo_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->have_graph) return gw_geo_fail(m, GW_ERR_STATE, "call gw_geo_set_rows or gw_geo_set_csr first");
  if (!sources) nsrc = m->n;
  if (nsrc < 0) return gw_geo_fail(m, GW_ERR_INVALID, "negative nsrc");
  if (nsrc == 0) return GW_OK;
  if (!out || pitch < m->n) return gw_geo_fail(m, GW_ERR_INVALID, "NULL output or pitch below n");
  m->st.rounds_max = m->st.relaxations = 0;
  m->st.fallbacks = 0;
  if (m->device >= 0) return gw_geo_dev_query(m, sources, nsrc, out, pitch, stream);
  if (sources)
    for (int64_t r = 0; r < nsrc; ++r)
      if (sources[r] < 0 || sources[r] >= m->n)
        return gw_geo_fail(m, GW_ERR_RANGE, "entry %lld: source %d outside [0, %lld)", (long long)r, (int)sources[r],
                           (long long)m->n);
  int64_t relaxed = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : relaxed)
  for (int64_t r = 0; r < nsrc; ++r) relaxed += host_source(m, sources ? sources[r] : r, out + r * pitch);
  m->st.relaxations = relaxed;
  return GW_OK;
}
