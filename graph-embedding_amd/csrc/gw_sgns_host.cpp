// SGNS trainer: C ABI, vocabulary / sampler construction, the host evaluation
// of the training law (device = -1) and the word2vec text writer.  The law
// itself is gw_sgns_law.h; the kernels are gw_sgns.hip.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <new>

#include "gw_internal.h"
#include "gw_sgns_internal.h"
#include "gw_sgns_law.h"
#include "gw_trainer_fail.h"

// the handle-less error of this family is the library-wide one (gw_last_error(NULL))
int gw_sgns_fail(gw_sgns* m, int code, const char* fmt, ...) {
  std::string tls;
  va_list ap;
  va_start(ap, fmt);
  gw_trainer_vfail(m ? &m->err : nullptr, &tls, code, fmt, ap);
  va_end(ap);
  gw_set_tls_error(tls);
  return code;
}

extern "C" const char* gw_sgns_last_error(const gw_sgns* m) { return m ? m->err.c_str() : gw_last_error(nullptr); }

extern "C" int gw_sgns_create(int device, int64_t n, const gw_sgns_params_t* params, gw_sgns** out) {
  if (!out) return gw_sgns_fail(nullptr, GW_ERR_INVALID, "NULL out");
  *out = nullptr;
  gw_sgns_params_t p;
  memset(&p, 0, sizeof p);
  p.struct_size = (int32_t)sizeof p;
  p.dim = 128;
  p.window = 5;
  p.negative = 5;
  p.epochs = 5;
  p.alpha = 0.025;
  p.min_alpha = 0.0001;
  p.sample = 1e-3;
  if (params) {
    if (params->struct_size < (int32_t)sizeof(int32_t))
      return gw_sgns_fail(nullptr, GW_ERR_INVALID, "gw_sgns_params_t.struct_size %d", (int)params->struct_size);
    const size_t take = std::min((size_t)params->struct_size, sizeof p);
    memcpy(&p, params, take);
    p.struct_size = (int32_t)sizeof p;
  }
  if (n < 1 || n >= (int64_t)INT32_MAX) return gw_sgns_fail(nullptr, GW_ERR_INVALID, "n %lld out of range", (long long)n);
  if (p.dim < 1 || p.dim > GW_SGNS_MAX_DIM) return gw_sgns_fail(nullptr, GW_ERR_INVALID, "dim %d not in [1, 1024]", p.dim);
  if (p.window < 1 || p.window > GW_SGNS_MAX_WINDOW)
    return gw_sgns_fail(nullptr, GW_ERR_INVALID, "window %d not in [1, 1023]", p.window);
  if (p.negative < 0 || p.negative > GW_SGNS_MAX_NEG)
    return gw_sgns_fail(nullptr, GW_ERR_INVALID, "negative %d not in [0, 511]", p.negative);
  if (p.epochs < 1 || p.epochs > GW_SGNS_MAX_EPOCHS)
    return gw_sgns_fail(nullptr, GW_ERR_INVALID, "epochs %d not in [1, 4096]", p.epochs);
  if (!(p.sample >= 0.0) || !isfinite(p.alpha) || !isfinite(p.min_alpha))
    return gw_sgns_fail(nullptr, GW_ERR_INVALID, "bad sample / alpha");
  if (device < -1) return gw_sgns_fail(nullptr, GW_ERR_INVALID, "device %d", device);
  gw_sgns* m = new (std::nothrow) gw_sgns();
  if (!m) return gw_sgns_fail(nullptr, GW_ERR_NOMEM, "out of memory");
  m->device = device;
  m->n = n;
  m->p = p;
  m->pitch = (p.dim + 3) / 4 * 4;
  if (device >= 0) {
    const int rc = gw_sgns_dev_alloc(m);
    if (rc != GW_OK) {
      gw_set_tls_error(m->err);
      gw_sgns_dev_free(m);
      delete m;
      return rc;
    }
  }
  *out = m;
  return GW_OK;
}

extern "C" int gw_sgns_free(gw_sgns* m) {
  if (!m) return GW_OK;
  if (m->device >= 0) gw_sgns_dev_free(m);
  delete m;
  return GW_OK;
}

// counts of a host corpus; GW_ERR_RANGE on an id outside [0, n)
static int host_count(gw_sgns* m, const int32_t* walks, int64_t nwalks, int walk_len) {
  m->counts.assign((size_t)m->n, 0);
  for (int64_t w = 0; w < nwalks; ++w) {
    const int32_t* row = walks + w * (int64_t)walk_len;
    for (int i = 0; i < walk_len; ++i) {
      const int32_t v = row[i];
      if (v == -1) break;
      if (v < 0 || v >= m->n)
        return gw_sgns_fail(m, GW_ERR_RANGE, "walk %lld position %d: id %d outside [0, %lld)", (long long)w, i, (int)v,
                            (long long)m->n);
      ++m->counts[(size_t)v];
    }
  }
  return GW_OK;
}

// keep thresholds, alias table of cnt^0.75 and the exp table from m->counts
static void build_tables(gw_sgns* m) {
  const int64_t n = m->n;
  double T = 0.0;
  for (int64_t v = 0; v < n; ++v) T += (double)m->counts[(size_t)v];
  m->keep_thr.assign((size_t)n, 0xFFFFFFFFu);
  if (m->p.sample > 0.0) {
    const double st = m->p.sample * T;
    for (int64_t v = 0; v < n; ++v) {
      const double c = (double)m->counts[(size_t)v];
      if (c <= 0.0) continue;
      const double keep = (sqrt(c / st) + 1.0) * st / c;
      if (keep < 1.0) m->keep_thr[(size_t)v] = (uint32_t)std::min(keep * 4294967296.0, 4294967294.0);
    }
  }
  // Vose alias method over q[v] = n * cnt^0.75 / Z (fp64), O(n)
  std::vector<double> q((size_t)n);
  double Z = 0.0;
  for (int64_t v = 0; v < n; ++v) {
    q[(size_t)v] = pow((double)m->counts[(size_t)v], 0.75);
    Z += q[(size_t)v];
  }
  m->J.resize((size_t)n);
  m->thr.assign((size_t)n, 0xFFFFFFFFu);
  std::vector<int32_t> small, large;
  for (int64_t v = 0; v < n; ++v) {
    m->J[(size_t)v] = (int32_t)v;
    q[(size_t)v] = Z > 0.0 ? q[(size_t)v] * (double)n / Z : 1.0;
    (q[(size_t)v] < 1.0 ? small : large).push_back((int32_t)v);
  }
  while (!small.empty() && !large.empty()) {
    const int32_t s = small.back(), l = large.back();
    small.pop_back();
    m->J[(size_t)s] = l;
    q[(size_t)l] = (q[(size_t)l] + q[(size_t)s]) - 1.0;
    if (q[(size_t)l] < 1.0) {
      large.pop_back();
      small.push_back(l);
    }
  }
  // whatever is left on either list keeps probability 1 (J = itself)
  for (int32_t v : small) q[(size_t)v] = 1.0;
  for (int32_t v : large) q[(size_t)v] = 1.0;
  for (int64_t v = 0; v < n; ++v) {
    const double x = q[(size_t)v];
    m->thr[(size_t)v] = x >= 1.0 ? 0xFFFFFFFFu : (uint32_t)(x < 0.0 ? 0.0 : x * 4294967296.0);
    if (x >= 1.0) m->J[(size_t)v] = (int32_t)v;  // the 2^-32 a full threshold misses stays with v
  }
  m->expt.resize(GW_SGNS_EXP_SIZE);
  for (int i = 0; i < GW_SGNS_EXP_SIZE; ++i) {
    const double e = exp(((double)i / GW_SGNS_EXP_SIZE * 2.0 - 1.0) * (double)GW_SGNS_MAX_EXP);
    m->expt[(size_t)i] = (float)(e / (e + 1.0));
  }
}

extern "C" int gw_sgns_build_vocab(gw_sgns* m, const int32_t* walks, int64_t nwalks, int walk_len) {
  if (!m) return gw_sgns_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (nwalks < 0 || walk_len < 1 || walk_len > GW_SGNS_MAX_POS || (nwalks > 0 && !walks))
    return gw_sgns_fail(m, GW_ERR_INVALID, "bad corpus arguments");
  m->vocab = false;
  int rc = m->device < 0 ? host_count(m, walks, nwalks, walk_len) : gw_sgns_dev_count(m, walks, nwalks, walk_len);
  if (rc != GW_OK) return rc;
  build_tables(m);
  if (m->device < 0) {
    m->syn0.assign((size_t)m->n * m->pitch, 0.0f);
    m->syn1.assign((size_t)m->n * m->pitch, 0.0f);
    for (int64_t v = 0; v < m->n; ++v)
      for (int d = 0; d < m->p.dim; ++d)
        m->syn0[(size_t)v * m->pitch + d] = gw_sgns_init(m->p.seed, (uint32_t)v, (uint32_t)d, m->p.dim);
  } else {
    rc = gw_sgns_dev_upload_vocab(m);
    if (rc != GW_OK) return rc;
  }
  m->vocab = true;
  return GW_OK;
}

// ---- the law on the host: 64 virtual lanes, the kernel's order ----------------
static float host_dot(const float* a, const float* b, int pitch) {
  float p[GW_SGNS_LANES];
  const int chunks = pitch / 4;
  const int active = std::min(chunks, GW_SGNS_LANES);  // lanes past the row hold +0
  for (int l = 0; l < active; ++l) {
    float s = 0.0f;
    for (int q = l; q < chunks; q += GW_SGNS_LANES)
      for (int e = 0; e < 4; ++e) s = gw_sgns_fma2(s, a[4 * q + e], b[4 * q + e]);
    p[l] = s;
  }
  for (int l = active; l < GW_SGNS_LANES; ++l) p[l] = 0.0f;
  // lane 0 of the butterfly p[l] += p[l ^ o]: at each level it only needs the
  // lanes below o, and a level whose partners are all +0 changes nothing (a
  // partial is never -0: it starts at +0)
  for (int o = GW_SGNS_LANES / 2; o >= 1; o >>= 1) {
    if (o >= active) continue;
    for (int l = 0; l < o; ++l) p[l] = p[l] + p[l + o];
  }
  return p[0];
}

static int host_train(gw_sgns* m, const int32_t* walks, int64_t nwalks, int walk_len, int e0, int ecount,
                      int64_t st[5]) {
  const int pitch = m->pitch, window = m->p.window, K = m->p.negative;
  const uint64_t seed = m->p.seed;
  std::vector<int32_t> s((size_t)walk_len), pos((size_t)walk_len), bb((size_t)walk_len);
  std::vector<float> neu((size_t)pitch);
  for (int e = e0; e < e0 + ecount; ++e) {
    for (int64_t w = 0; w < nwalks; ++w) {
      const int32_t* row = walks + w * (int64_t)walk_len;
      const float alpha = gw_sgns_alpha(m->p.alpha, m->p.min_alpha, e, w, m->p.epochs, nwalks);
      int cnt = 0;
      for (int i = 0; i < walk_len; ++i) {
        const int32_t v = row[i];
        if (v == -1) break;
        if (v < 0 || v >= m->n) return gw_sgns_fail(m, GW_ERR_RANGE, "walk %lld: id %d outside [0, n)", (long long)w, (int)v);
        const gw_u4 u = gw_sgns_tok_draw(seed, (uint32_t)e, (uint64_t)w, (uint32_t)i);
        if (!gw_sgns_keep(u.x, m->keep_thr[(size_t)v])) continue;
        s[(size_t)cnt] = v;
        pos[(size_t)cnt] = i;
        bb[(size_t)cnt] = (int32_t)(u.y % (uint32_t)window);
        ++cnt;
      }
      st[0] += cnt;
      for (int i = 0; i < cnt; ++i) {
        const int32_t centre = s[(size_t)i];
        const int lo = i - window + bb[(size_t)i], hi = i + window - bb[(size_t)i];
        for (int j = std::max(lo, 0); j <= std::min(hi, cnt - 1); ++j) {
          if (j == i) continue;
          const uint32_t slot = (uint32_t)(j - (i - window));
          float* l1 = &m->syn0[(size_t)s[(size_t)j] * pitch];
          std::fill(neu.begin(), neu.end(), 0.0f);
          ++st[1];
          st[2] += K;
          for (int k = 0; k <= K; ++k) {
            int32_t t = centre;
            if (k > 0) {
              t = gw_sgns_neg_draw(seed, (uint32_t)e, (uint64_t)w, (uint32_t)pos[(size_t)i], slot, (uint32_t)(k - 1),
                                   (uint32_t)m->n, m->J.data(), m->thr.data());
              if (t == centre) {
                ++st[3];
                continue;
              }
            }
            float* r = &m->syn1[(size_t)t * pitch];
            const float f = host_dot(l1, r, pitch);
            float g;
            if (!gw_sgns_grad(f, k == 0 ? 1.0f : 0.0f, alpha, m->expt.data(), &g)) {
              ++st[4];
              continue;
            }
            for (int d = 0; d < pitch; ++d) {
              neu[(size_t)d] = gw_sgns_fma2(neu[(size_t)d], g, r[d]);
              r[d] = gw_sgns_fma2(r[d], g, l1[d]);
            }
          }
          for (int d = 0; d < pitch; ++d) l1[d] = l1[d] + neu[(size_t)d];
        }
      }
    }
  }
  return GW_OK;
}

extern "C" int gw_sgns_train(gw_sgns* m, const int32_t* walks, int64_t nwalks, int walk_len, int epoch_begin,
                             int epoch_count, int concurrency, gw_sgns_stats_t* stats, void* stream) {
  if (!m) return gw_sgns_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->vocab) return gw_sgns_fail(m, GW_ERR_STATE, "call gw_sgns_build_vocab first");
  if (nwalks < 0 || walk_len < 1 || walk_len > GW_SGNS_MAX_POS || (nwalks > 0 && !walks) || concurrency < 0)
    return gw_sgns_fail(m, GW_ERR_INVALID, "bad corpus arguments");
  if (epoch_begin < 0 || epoch_count < 0 || (int64_t)epoch_begin + epoch_count > m->p.epochs)
    return gw_sgns_fail(m, GW_ERR_INVALID, "epochs [%d, %d) outside the schedule's %d", epoch_begin,
                        epoch_begin + epoch_count, (int)m->p.epochs);
  if (nwalks == 0 || epoch_count == 0) return GW_OK;
  int64_t st[5] = {0, 0, 0, 0, 0};
  const int rc = m->device < 0
                     ? host_train(m, walks, nwalks, walk_len, epoch_begin, epoch_count, st)
                     : gw_sgns_dev_train(m, walks, nwalks, walk_len, epoch_begin, epoch_count, concurrency, st, stream);
  if (rc != GW_OK) return rc;
  if (stats) {
    stats->tokens_kept += st[0];
    stats->pairs += st[1];
    stats->negatives += st[2];
    stats->negatives_centre += st[3];
    stats->targets_clipped += st[4];
  }
  return GW_OK;
}

extern "C" int gw_sgns_export(gw_sgns* m, float* syn0, float* syn1neg, int64_t* counts) {
  if (!m) return gw_sgns_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->vocab) return gw_sgns_fail(m, GW_ERR_STATE, "call gw_sgns_build_vocab first");
  if (counts) memcpy(counts, m->counts.data(), sizeof(int64_t) * (size_t)m->n);
  if (m->device >= 0) return gw_sgns_dev_export(m, syn0, syn1neg);
  const int dim = m->p.dim;
  for (int64_t v = 0; v < m->n; ++v) {
    if (syn0) memcpy(syn0 + v * dim, &m->syn0[(size_t)v * m->pitch], sizeof(float) * (size_t)dim);
    if (syn1neg) memcpy(syn1neg + v * dim, &m->syn1[(size_t)v * m->pitch], sizeof(float) * (size_t)dim);
  }
  return GW_OK;
}

extern "C" int gw_sgns_sampler_export(const gw_sgns* m, int32_t* J, uint32_t* thr, uint32_t* keep_thr) {
  if (!m) return gw_sgns_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->vocab) return gw_sgns_fail(const_cast<gw_sgns*>(m), GW_ERR_STATE, "call gw_sgns_build_vocab first");
  if (J) memcpy(J, m->J.data(), sizeof(int32_t) * (size_t)m->n);
  if (thr) memcpy(thr, m->thr.data(), sizeof(uint32_t) * (size_t)m->n);
  if (keep_thr) memcpy(keep_thr, m->keep_thr.data(), sizeof(uint32_t) * (size_t)m->n);
  return GW_OK;
}

extern "C" int gw_sgns_vectors_dev(gw_sgns* m, float** ptr, int64_t* pitch) {
  if (!m || !ptr || !pitch) return gw_sgns_fail(m, GW_ERR_INVALID, "NULL argument");
  if (!m->vocab) return gw_sgns_fail(m, GW_ERR_STATE, "call gw_sgns_build_vocab first");
  *ptr = m->device < 0 ? m->syn0.data() : gw_sgns_dev_vectors(m);
  *pitch = m->pitch;
  return GW_OK;
}

extern "C" int gw_sgns_auto_concurrency_for(const gw_sgns* m, int64_t nwalks, int32_t* concurrency) {
  if (!m || !concurrency) return gw_sgns_fail(nullptr, GW_ERR_INVALID, "NULL argument");
  *concurrency = m->device < 0 ? 1 : gw_sgns_auto_concurrency(m, nwalks);
  return GW_OK;
}

extern "C" int gw_write_word2vec_text(const char* path, const float* syn0, const int64_t* counts,
                                      const int64_t* labels, int64_t n, int dim) {
  if (!path || !syn0 || !counts || n < 0 || dim < 1) return gw_sgns_fail(nullptr, GW_ERR_INVALID, "bad arguments");
  std::vector<int64_t> rows;
  for (int64_t v = 0; v < n; ++v)
    if (counts[v] > 0) rows.push_back(v);
  // count descending, label ascending (gensim sorts by count only; its tie
  // order is its vocabulary dict's, arbitrary under the reference's Python)
  std::sort(rows.begin(), rows.end(), [&](int64_t a, int64_t b) {
    if (counts[a] != counts[b]) return counts[a] > counts[b];
    return (labels ? labels[a] : a) < (labels ? labels[b] : b);
  });
  FILE* f = fopen(path, "w");
  if (!f) return gw_sgns_fail(nullptr, GW_ERR_IO, "cannot open '%s' for writing", path);
  bool ok = fprintf(f, "%lld %d\n", (long long)rows.size(), dim) > 0;
  for (size_t r = 0; ok && r < rows.size(); ++r) {
    const int64_t v = rows[r];
    ok = fprintf(f, "%lld", (long long)(labels ? labels[v] : v)) > 0;
    for (int d = 0; ok && d < dim; ++d) ok = fprintf(f, " %f", (double)syn0[v * dim + d]) > 0;
    ok = ok && fputc('\n', f) != EOF;
  }
  if (fclose(f) != 0) ok = false;
  if (!ok) return gw_sgns_fail(nullptr, GW_ERR_IO, "write to '%s' failed", path);
  return GW_OK;
}
