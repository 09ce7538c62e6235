// What the host sides of the all-pairs top-k families (gw_knn_host.cpp, gw_nng_host.cpp) have in common:
// the handle's base, the row and vector setters, the params prologue, the create skeleton, the range check of
// the sources and the host evaluation of a row.  It includes only the C++ library, so the host-only builds
// (-DGW_KNN_HOST_ONLY, -DGW_NNG_HOST_ONLY) can use it.
//
// A handle H derives from gw_pairs_handle, has params `p` with dim and topk, and gw_fail_of(H*) names its *_fail.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/graphwalk.h"

struct gw_pairs_handle {
  int device = -1;  // -1: host evaluation
  int64_t n = 0;
  const float* x = nullptr;  // caller's rows (host or device memory)
  int64_t pitch = 0;
  bool have_x = false;
  std::string err;
};

template <class H>
int gw_pairs_check_rows(H* m, int device, int64_t n) {
  if (n < 1 || n >= (int64_t)1 << 40) return gw_fail_of(m)(m, GW_ERR_INVALID, "n %lld out of range", (long long)n);
  if (device >= 0 && n >= (int64_t)1 << 31)
    return gw_fail_of(m)(m, GW_ERR_UNSUPPORTED, "n %lld: the kernels take n < 2^31 (device = -1 takes any)", (long long)n);
  return GW_OK;
}

template <class H>
int gw_pairs_set_rows(H* m, int64_t n) {
  if (!m) return gw_fail_of(m)(nullptr, GW_ERR_INVALID, "NULL handle");
  const int rc = gw_pairs_check_rows(m, m->device, n);
  if (rc != GW_OK) return rc;
  m->n = n;
  m->have_x = false;  // the vectors set before had another row count
  return GW_OK;
}

template <class H>
int gw_pairs_set_vectors(H* m, const float* x, int64_t pitch) {
  if (!m) return gw_fail_of(m)(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!x || pitch < m->p.dim) return gw_fail_of(m)(m, GW_ERR_INVALID, "NULL vectors or pitch below dim");
  m->x = x;
  m->pitch = pitch;
  m->have_x = true;
  return GW_OK;
}

// *p holds the defaults: the caller's first struct_size bytes go over them (`name`: the struct's, for the message)
template <class H, class P>
int gw_pairs_read_params(const P* params, P* p, const char* name) {
  if (params) {
    if (params->struct_size < (int32_t)sizeof(int32_t))
      return gw_fail_of((H*)nullptr)(nullptr, GW_ERR_INVALID, "%s.struct_size %d", name, (int)params->struct_size);
    memcpy(p, params, std::min((size_t)params->struct_size, sizeof *p));
  }
  p->struct_size = (int32_t)sizeof *p;
  return GW_OK;
}

// The rest of *_create behind the family's own parameter checks: device, n, the device path's limits, the
// handle and its device state.  *tls is the family's handle-less error string.
template <class H, class P>
int gw_pairs_create(int device, int64_t n, const P& p, int max_dim, int max_topk, int (*dev_alloc)(H*),
                    void (*dev_free)(H*), std::string* tls, H** out) {
  const auto fail = gw_fail_of((H*)nullptr);
  if (device < -1) return fail(nullptr, GW_ERR_INVALID, "device %d", device);
  int rc = gw_pairs_check_rows((H*)nullptr, device, n);
  if (rc != GW_OK) return rc;
  if (device >= 0 && (p.dim > max_dim || p.topk > max_topk))
    return fail(nullptr, GW_ERR_UNSUPPORTED, "dim %d / topk %d: the kernels take dim <= %d and topk <= %d "
                "(device = -1 takes any)", p.dim, p.topk, max_dim, max_topk);
  H* m = new (std::nothrow) H();
  if (!m) return fail(nullptr, GW_ERR_NOMEM, "out of memory");
  m->device = device;
  m->p = p;
  m->n = n;
  if (device >= 0) {
    rc = dev_alloc(m);
    if (rc != GW_OK) {
      *tls = m->err;
      dev_free(m);
      delete m;
      return rc;
    }
  }
  *out = m;
  return GW_OK;
}

// host memory
template <class H>
int gw_pairs_check_sources(H* m, const int32_t* sources, int64_t nsrc) {
  if (sources)
    for (int64_t r = 0; r < nsrc; ++r)
      if (sources[r] < 0 || sources[r] >= m->n)
        return gw_fail_of(m)(m, GW_ERR_RANGE, "entry %lld: source %d outside [0, %lld)", (long long)r, (int)sources[r],
                             (long long)m->n);
  return GW_OK;
}

// The law on the host, row by row.  L gives keep (entries selected per row; 0: no candidate is looked at),
// score(v, j, &s) (may j stand in the row of v, and with which value), before (the law's total order) and
// write_row(r, v, cand, kept): row r, of source v, from its `kept` best (value, id) in order.
template <class Law>
void gw_pairs_host_rows(const Law& L, int64_t n, const int32_t* sources, int64_t nsrc) {
  using cand_t = std::pair<double, int32_t>;
  const auto before = [](const cand_t& a, const cand_t& b) { return Law::before(a.first, a.second, b.first, b.second) != 0; };
#pragma omp parallel
  {
    std::vector<cand_t> cand;
#pragma omp for schedule(dynamic, 8)
    for (int64_t r = 0; r < nsrc; ++r) {
      const int64_t v = sources ? sources[r] : r;
      cand.clear();
      if (L.keep > 0)
        for (int64_t j = 0; j < n; ++j) {
          double s;
          if (j != v && L.score(v, j, &s)) cand.emplace_back(s, (int32_t)j);
        }
      const size_t kept = std::min<size_t>(cand.size(), (size_t)L.keep);
      std::partial_sort(cand.begin(), cand.begin() + (ptrdiff_t)kept, cand.end(), before);
      L.write_row(r, v, cand.data(), kept);
    }
  }
}
