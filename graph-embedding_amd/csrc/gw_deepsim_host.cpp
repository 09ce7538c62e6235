// DeepSim trainer: C ABI, SimRank table build, initial values, the host
// evaluation of the training law (device = -1) and the save_embeddings writer.
// The law itself is gw_deepsim_law.h; the kernels are gw_deepsim.hip.
//
// This file depends on nothing but the C++ library, so that it also builds as
// a plain host program (-DGW_DEEPSIM_HOST_ONLY: no device path) for sanitizer
// runs (host/deepsim_host_check.cpp).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>

#include "gw_deepsim_internal.h"
#include "gw_deepsim_law.h"
#include "gw_trainer_fail.h"

static thread_local std::string g_ds_err;

int gw_deepsim_fail(gw_deepsim* m, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  gw_trainer_vfail(m ? &m->err : nullptr, &g_ds_err, code, fmt, ap);
  va_end(ap);
  return code;
}

#ifdef GW_DEEPSIM_HOST_ONLY
static int no_dev(gw_deepsim* m) { return gw_deepsim_fail(m, GW_ERR_DEVICE, "built without the device path"); }
int gw_ds_dev_alloc(gw_deepsim* m, const std::vector<float>*) { return no_dev(m); }
void gw_ds_dev_free(gw_deepsim*) {}
int gw_ds_dev_fetch_table(gw_deepsim* m, const int32_t*, const double*, int, std::vector<int32_t>*,
                          std::vector<double>*) { return no_dev(m); }
int gw_ds_dev_upload_table(gw_deepsim* m) { return no_dev(m); }
int gw_ds_dev_scan_walks(gw_deepsim* m, std::vector<int32_t>*) { return no_dev(m); }
int gw_ds_dev_upload_elig(gw_deepsim* m) { return no_dev(m); }
int gw_ds_dev_train(gw_deepsim* m, int64_t, int64_t, double*, void*) { return no_dev(m); }
int gw_ds_dev_gradients(gw_deepsim* m, int64_t, float*, float*, float*, float*) { return no_dev(m); }
int gw_ds_dev_batch(gw_deepsim* m, int64_t, int32_t*, int32_t*, float*, int32_t*, float*) { return no_dev(m); }
int gw_ds_dev_export(gw_deepsim* m, float* const*, float* const*, float* const*) { return no_dev(m); }
float* gw_ds_dev_vectors(gw_deepsim* m) { return no_dev(m), nullptr; }
#endif

extern "C" const char* gw_deepsim_last_error(const gw_deepsim* m) { return m ? m->err.c_str() : g_ds_err.c_str(); }

extern "C" int gw_deepsim_create(int device, const gw_deepsim_params_t* params, gw_deepsim** out) {
  if (!out) return gw_deepsim_fail(nullptr, GW_ERR_INVALID, "NULL out");
  *out = nullptr;
  gw_deepsim_params_t p;
  memset(&p, 0, sizeof p);
  p.dim = 128;
  p.window = 10;
  p.batch = 128;
  p.fallback = GW_DEEPSIM_FALLBACK_ROW_MIN;
  p.learning_rate = 0.001;
  p.beta1 = 0.9;
  p.beta2 = 0.999;
  p.epsilon = 1e-8;
  p.score_scale = 1.0;
  if (params) {
    if (params->struct_size < (int32_t)sizeof(int32_t))
      return gw_deepsim_fail(nullptr, GW_ERR_INVALID, "gw_deepsim_params_t.struct_size %d", (int)params->struct_size);
    memcpy(&p, params, std::min((size_t)params->struct_size, sizeof p));
  }
  p.struct_size = (int32_t)sizeof p;
  if (p.vertex_num < 1 || p.vertex_num >= (int64_t)INT32_MAX)
    return gw_deepsim_fail(nullptr, GW_ERR_INVALID, "vertex_num %lld out of range", (long long)p.vertex_num);
  if (p.dim < 1 || p.window < 1 || p.batch < 1 || p.dim > (1 << 20) || p.window > (1 << 20) || p.batch > (1 << 20))
    return gw_deepsim_fail(nullptr, GW_ERR_INVALID, "dim %d, window %d and batch %d must be positive", p.dim, p.window,
                           p.batch);
  if (p.fallback != GW_DEEPSIM_FALLBACK_ROW_MIN && p.fallback != GW_DEEPSIM_FALLBACK_POSITION)
    return gw_deepsim_fail(nullptr, GW_ERR_INVALID, "fallback %d", p.fallback);
  if (!(p.learning_rate > 0.0) || !(p.beta1 >= 0.0 && p.beta1 < 1.0) || !(p.beta2 >= 0.0 && p.beta2 < 1.0) ||
      !(p.epsilon > 0.0) || !isfinite(p.score_scale) || !isfinite(p.learning_rate))
    return gw_deepsim_fail(nullptr, GW_ERR_INVALID, "bad learning_rate / beta / epsilon / score_scale");
  if (device < -1) return gw_deepsim_fail(nullptr, GW_ERR_INVALID, "device %d", device);
  if (device >= 0) {
    if (p.dim % 32 || p.dim > 128 || p.batch % 32 || p.batch > 128)
      return gw_deepsim_fail(nullptr, GW_ERR_UNSUPPORTED,
                             "dim %d / batch %d: the kernels take multiples of 32 in [32, 128] (device = -1 takes any)",
                             p.dim, p.batch);
    if (p.window > GW_DS_MAX_WINDOW)
      return gw_deepsim_fail(nullptr, GW_ERR_UNSUPPORTED, "window %d: the kernels take window <= %d", p.window,
                             GW_DS_MAX_WINDOW);
  }
  gw_deepsim* m = new (std::nothrow) gw_deepsim();
  if (!m) return gw_deepsim_fail(nullptr, GW_ERR_NOMEM, "out of memory");
  m->device = device;
  m->p = p;
  m->V = p.vertex_num;
  m->W = 2 * p.window + 1;
  m->ntiles = (int)((m->V + GW_DS_TW - 1) / GW_DS_TW);
  std::vector<float> init[4];
  for (int t = 0; t < 4; ++t) {
    init[t].assign(gw_ds_numel(m, t), 0.0f);
    if (t == GW_DS_W1 || t == GW_DS_W2)
      for (size_t i = 0; i < init[t].size(); ++i) init[t][i] = gw_ds_init(p.seed, (uint64_t)i, (uint32_t)t);
  }
  if (device >= 0) {
    const int rc = gw_ds_dev_alloc(m, init);
    if (rc != GW_OK) {
      g_ds_err = m->err;
      gw_ds_dev_free(m);
      delete m;
      return rc;
    }
  } else {
    for (int t = 0; t < 4; ++t) {
      m->par[t].swap(init[t]);
      m->am[t].assign(m->par[t].size(), 0.0f);
      m->av[t].assign(m->par[t].size(), 0.0f);
    }
  }
  *out = m;
  return GW_OK;
}

extern "C" int gw_deepsim_free(gw_deepsim* m) {
  if (!m) return GW_OK;
  if (m->device >= 0) gw_ds_dev_free(m);
  delete m;
  return GW_OK;
}

extern "C" int gw_deepsim_set_simrank(gw_deepsim* m, const int32_t* ids, const double* scores, int topk) {
  if (!m) return gw_deepsim_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!ids || !scores || topk < 1) return gw_deepsim_fail(m, GW_ERR_INVALID, "bad table arguments");
  if (m->device >= 0 && topk > GW_DS_MAX_TOPK)
    return gw_deepsim_fail(m, GW_ERR_UNSUPPORTED, "topk %d: the kernels take topk <= %d", topk, GW_DS_MAX_TOPK);
  m->have_tab = false;
  std::vector<int32_t> hid;
  std::vector<double> hsc;
  if (m->device >= 0) {
    const int rc = gw_ds_dev_fetch_table(m, ids, scores, topk, &hid, &hsc);
    if (rc != GW_OK) return rc;
    ids = hid.data();
    scores = hsc.data();
  }
  const int64_t V = m->V;
  m->topk = topk;
  m->tab_id.assign((size_t)V * topk, -1);
  m->tab_val.assign((size_t)V * topk, 0.0f);
  m->tab_cnt.assign((size_t)V, 0);
  m->tem.assign((size_t)V, 0.0f);
  std::vector<std::pair<int32_t, double>> row;
  for (int64_t v = 0; v < V; ++v) {
    row.clear();
    for (int e = 0; e < topk; ++e) {
      const int32_t id = ids[v * topk + e];
      if (id == -1) continue;
      if (id < 0 || id >= V)
        return gw_deepsim_fail(m, GW_ERR_RANGE, "table row %lld entry %d: id %d outside [0, %lld)", (long long)v, e,
                               (int)id, (long long)V);
      const double s = scores[v * topk + e] * m->p.score_scale;
      if (!(s > GW_DS_DROP)) continue;
      row.emplace_back(id, s);
    }
    if (!row.empty()) m->tem[(size_t)v] = (float)row.back().second;
    std::stable_sort(row.begin(), row.end());
    m->tab_cnt[(size_t)v] = (int32_t)row.size();
    for (size_t e = 0; e < row.size(); ++e) {
      m->tab_id[(size_t)v * topk + e] = row[e].first;
      m->tab_val[(size_t)v * topk + e] = (float)row[e].second;
    }
  }
  if (m->device >= 0) {
    const int rc = gw_ds_dev_upload_table(m);
    if (rc != GW_OK) return rc;
  }
  m->have_tab = true;
  return GW_OK;
}

extern "C" int gw_deepsim_set_walks(gw_deepsim* m, const int32_t* walks, int64_t nwalks, int walk_len,
                                    const int64_t* labels, int64_t n_labels) {
  if (!m) return gw_deepsim_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (nwalks < 0 || walk_len < 1 || (nwalks > 0 && !walks) || (labels && n_labels < 1) ||
      nwalks > INT64_MAX / walk_len)
    return gw_deepsim_fail(m, GW_ERR_INVALID, "bad corpus arguments");
  m->have_walks = false;
  m->walks = walks;
  m->nwalks = nwalks;
  m->walk_len = walk_len;
  m->has_labels = labels != nullptr;
  m->labels.clear();
  if (labels) m->labels.assign(labels, labels + n_labels);  // only labels a token uses must lie in [0, V)
  std::vector<int32_t> len((size_t)nwalks, 0);
  if (m->device >= 0) {
    const int rc = gw_ds_dev_scan_walks(m, &len);
    if (rc != GW_OK) return rc;
  } else {
    const int64_t lim = m->has_labels ? n_labels : m->V;
    for (int64_t w = 0; w < nwalks; ++w) {
      const int32_t* row = walks + w * (int64_t)walk_len;
      int i = 0;
      for (; i < walk_len; ++i) {
        const int32_t v = row[i];
        if (v == -1) break;
        const int64_t mv = v < 0 || v >= lim ? -1 : (m->has_labels ? labels[v] : (int64_t)v);
        if (mv < 0 || mv >= m->V)
          return gw_deepsim_fail(m, GW_ERR_RANGE, "walk %lld position %d: token %d maps outside [0, %lld)", (long long)w,
                                 i, (int)v, (long long)m->V);
      }
      len[(size_t)w] = i;
    }
  }
  m->elig.clear();
  m->elig_len.clear();
  for (int64_t w = 0; w < nwalks; ++w)
    if (len[(size_t)w] >= m->W) {
      m->elig.push_back(w);
      m->elig_len.push_back(len[(size_t)w]);
    }
  if ((int64_t)m->elig.size() < m->p.batch)
    return gw_deepsim_fail(m, GW_ERR_INVALID, "%lld walks of at least %d tokens, fewer than the batch of %d",
                           (long long)m->elig.size(), m->W, (int)m->p.batch);
  if (m->p.fallback == GW_DEEPSIM_FALLBACK_POSITION && (int64_t)walk_len - m->p.window > m->V)
    return gw_deepsim_fail(m, GW_ERR_RANGE, "fallback by position: walk_len - window = %d exceeds vertex_num %lld",
                           walk_len - (int)m->p.window, (long long)m->V);
  if (m->device >= 0) {
    const int rc = gw_ds_dev_upload_elig(m);
    if (rc != GW_OK) return rc;
  }
  m->have_walks = true;
  return GW_OK;
}

static int ready(gw_deepsim* m, int64_t step_begin, int64_t step_count) {
  if (!m) return gw_deepsim_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (!m->have_tab || !m->have_walks)
    return gw_deepsim_fail(m, GW_ERR_STATE, "call gw_deepsim_set_simrank and gw_deepsim_set_walks first");
  if (step_begin < 0 || step_count < 0 || step_begin > INT64_MAX - step_count)
    return gw_deepsim_fail(m, GW_ERR_INVALID, "bad step range");
  return GW_OK;
}

// ---- the law on the host -------------------------------------------------------
struct HostBatch {
  std::vector<int32_t> centre, tgt_id, tgt_n;
  std::vector<float> tgt_val, ysum;
};

static void host_batch(const gw_deepsim* m, uint64_t t, HostBatch* hb) {
  const int B = m->p.batch, W = m->W, k = m->p.window;
  hb->centre.assign((size_t)B, 0);
  hb->tgt_id.assign((size_t)B * W, -1);
  hb->tgt_val.assign((size_t)B * W, 0.0f);
  hb->tgt_n.assign((size_t)B, 0);
  hb->ysum.assign((size_t)B, 0.0f);
  for (int s = 0; s < B; ++s) {
    const uint64_t e = gw_ds_walk_slot(m->p.seed, t, (uint32_t)s, (uint64_t)m->elig.size());
    const int32_t* row = m->walks + m->elig[(size_t)e] * (int64_t)m->walk_len;
    const int pos = gw_ds_pos(m->p.seed, t, (uint32_t)s, m->elig_len[(size_t)e], k);
    int32_t* ids = &hb->tgt_id[(size_t)s * W];
    float* vals = &hb->tgt_val[(size_t)s * W];
    int n = 0;
    for (int i = 0; i < W; ++i) {
      const int32_t tok = row[pos - k + i];
      const int32_t v = m->has_labels ? (int32_t)m->labels[(size_t)tok] : tok;
      if (i == k) hb->centre[(size_t)s] = v;
      bool seen = false;
      for (int q = 0; q < n && !seen; ++q) seen = ids[q] == v;
      if (!seen) ids[n++] = v;
    }
    const int32_t c = hb->centre[(size_t)s];
    const float fb = m->p.fallback == GW_DEEPSIM_FALLBACK_ROW_MIN ? m->tem[(size_t)c] : m->tem[(size_t)pos];
    float ys = 0.0f;
    for (int q = 0; q < n; ++q) {
      vals[q] = gw_ds_lookup(&m->tab_id[(size_t)c * m->topk], &m->tab_val[(size_t)c * m->topk], m->tab_cnt[(size_t)c],
                             ids[q], fb);
      ys = ys + vals[q];
    }
    hb->tgt_n[(size_t)s] = n;
    hb->ysum[(size_t)s] = ys;
  }
}

// one step: the gradient of step t's batch at the current parameters into g[4]
// (resized here) and its loss; the parameters are not touched
static double host_gradient(const gw_deepsim* m, uint64_t t, std::vector<float> g[4]) {
  const int B = m->p.batch, d = m->p.dim, W = m->W;
  const int64_t V = m->V;
  const float* w1 = m->par[0].data();
  const float* b1 = m->par[1].data();
  const float* w2 = m->par[2].data();
  const float* b2 = m->par[3].data();
  HostBatch hb;
  host_batch(m, t, &hb);
  std::vector<float> hid((size_t)B * d), pre((size_t)B * d), lg((size_t)B * V), dl((size_t)B * V);
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < d; ++h) {
      const float x = w1[(size_t)hb.centre[(size_t)b] * d + h] + b1[h];
      pre[(size_t)b * d + h] = x;
      hid[(size_t)b * d + h] = x > 0.0f ? x : 0.0f;
    }
  for (int b = 0; b < B; ++b) {
    float* l = &lg[(size_t)b * V];
    for (int64_t j = 0; j < V; ++j) l[j] = b2[j];
    for (int h = 0; h < d; ++h) {
      const float x = hid[(size_t)b * d + h];
      const float* wr = w2 + (size_t)h * V;
      for (int64_t j = 0; j < V; ++j) l[j] = fmaf(x, wr[j], l[j]);
    }
  }
  double loss = 0.0;
  std::vector<float> y((size_t)V);
  const float Bf = (float)B;
  for (int b = 0; b < B; ++b) {
    const float* l = &lg[(size_t)b * V];
    std::vector<float> tm((size_t)m->ntiles), ts((size_t)m->ntiles);
    float M = -INFINITY;
    for (int T = 0; T < m->ntiles; ++T) {
      const int64_t j0 = (int64_t)T * GW_DS_TW, j1 = std::min(V, j0 + GW_DS_TW);
      float mx = l[j0];
      for (int64_t j = j0 + 1; j < j1; ++j) mx = l[j] > mx ? l[j] : mx;
      float s = 0.0f;
      for (int64_t j = j0; j < j1; ++j) s = s + gw_ds_exp(l[j] - mx);
      tm[(size_t)T] = mx;
      ts[(size_t)T] = s;
      M = mx > M ? mx : M;
    }
    float S = 0.0f;
    for (int T = 0; T < m->ntiles; ++T) S = fmaf(ts[(size_t)T], gw_ds_exp(tm[(size_t)T] - M), S);
    std::fill(y.begin(), y.end(), 0.0f);
    double lb = 0.0;
    const double logS = log((double)S);
    for (int q = 0; q < hb.tgt_n[(size_t)b]; ++q) {
      const int32_t j = hb.tgt_id[(size_t)b * W + q];
      const float yv = hb.tgt_val[(size_t)b * W + q];
      y[(size_t)j] = yv;
      lb += (double)yv * ((double)l[j] - (double)M - logS);
    }
    loss += -lb;
    float* dr = &dl[(size_t)b * V];
    for (int64_t j = 0; j < V; ++j) dr[j] = gw_ds_dlogit(l[j], M, S, hb.ysum[(size_t)b], y[(size_t)j], Bf);
  }
  loss /= (double)B;
  for (int t4 = 0; t4 < 4; ++t4) g[t4].assign(gw_ds_numel(m, t4), 0.0f);
  // dhidden: tile partials, then tiles ascending, then the relu mask
  std::vector<float> dh((size_t)B * d, 0.0f);
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < d; ++h) {
      float acc = 0.0f;
      const float* wr = w2 + (size_t)h * V;
      const float* dr = &dl[(size_t)b * V];
      for (int T = 0; T < m->ntiles; ++T) {
        const int64_t j0 = (int64_t)T * GW_DS_TW, j1 = std::min(V, j0 + GW_DS_TW);
        float part = 0.0f;
        for (int64_t j = j0; j < j1; ++j) part = fmaf(dr[j], wr[j], part);
        acc = acc + part;
      }
      dh[(size_t)b * d + h] = pre[(size_t)b * d + h] > 0.0f ? acc : 0.0f;
    }
  // dw2 (b ascending fmaf chain), db2
  float* g2 = g[2].data();
  for (int h = 0; h < d; ++h)
    for (int b = 0; b < B; ++b) {
      const float x = hid[(size_t)b * d + h];
      const float* dr = &dl[(size_t)b * V];
      float* gr = g2 + (size_t)h * V;
      for (int64_t j = 0; j < V; ++j) gr[j] = fmaf(x, dr[j], gr[j]);
    }
  for (int b = 0; b < B; ++b)
    for (int64_t j = 0; j < V; ++j) g[3][(size_t)j] = g[3][(size_t)j] + dl[(size_t)b * V + j];
  // dw1 rows (slots ascending), db1
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < d; ++h) {
      float* p = &g[0][(size_t)hb.centre[(size_t)b] * d + h];
      *p = *p + dh[(size_t)b * d + h];
      g[1][(size_t)h] = g[1][(size_t)h] + dh[(size_t)b * d + h];
    }
  return loss;
}

static int host_train(gw_deepsim* m, int64_t step_begin, int64_t step_count, double* loss_out) {
  std::vector<float> g[4];
  for (int64_t i = 0; i < step_count; ++i) {
    const uint64_t t = (uint64_t)(step_begin + i);
    const double loss = host_gradient(m, t, g);
    if (loss_out) loss_out[i] = loss;
    const gw_ds_adam_c c = gw_ds_adam_consts(m->p.learning_rate, m->p.beta1, m->p.beta2, m->p.epsilon, t);
    for (int t4 = 0; t4 < 4; ++t4)
      for (size_t e = 0; e < g[t4].size(); ++e) gw_ds_adam(&m->par[t4][e], &m->am[t4][e], &m->av[t4][e], g[t4][e], c);
  }
  return GW_OK;
}

extern "C" int gw_deepsim_train(gw_deepsim* m, int64_t step_begin, int64_t step_count, double* loss_out,
                                void* stream) {
  const int rc = ready(m, step_begin, step_count);
  if (rc != GW_OK) return rc;
  if (step_count == 0) return GW_OK;
  return m->device < 0 ? host_train(m, step_begin, step_count, loss_out)
                       : gw_ds_dev_train(m, step_begin, step_count, loss_out, stream);
}

extern "C" int gw_deepsim_gradients(gw_deepsim* m, int64_t step, float* gw1, float* gb1, float* gw2, float* gb2) {
  const int rc = ready(m, step, 0);
  if (rc != GW_OK) return rc;
  if (m->device >= 0) return gw_ds_dev_gradients(m, step, gw1, gb1, gw2, gb2);
  std::vector<float> g[4];
  host_gradient(m, (uint64_t)step, g);
  float* out[4] = {gw1, gb1, gw2, gb2};
  for (int t = 0; t < 4; ++t)
    if (out[t]) memcpy(out[t], g[t].data(), g[t].size() * sizeof(float));
  return GW_OK;
}

extern "C" int gw_deepsim_batch(gw_deepsim* m, int64_t step, int32_t* centre, int32_t* tgt_id, float* tgt_val,
                                int32_t* tgt_n, float* ysum) {
  const int rc = ready(m, step, 0);
  if (rc != GW_OK) return rc;
  if (m->device >= 0) return gw_ds_dev_batch(m, step, centre, tgt_id, tgt_val, tgt_n, ysum);
  HostBatch hb;
  host_batch(m, (uint64_t)step, &hb);
  if (centre) memcpy(centre, hb.centre.data(), hb.centre.size() * sizeof(int32_t));
  if (tgt_id) memcpy(tgt_id, hb.tgt_id.data(), hb.tgt_id.size() * sizeof(int32_t));
  if (tgt_val) memcpy(tgt_val, hb.tgt_val.data(), hb.tgt_val.size() * sizeof(float));
  if (tgt_n) memcpy(tgt_n, hb.tgt_n.data(), hb.tgt_n.size() * sizeof(int32_t));
  if (ysum) memcpy(ysum, hb.ysum.data(), hb.ysum.size() * sizeof(float));
  return GW_OK;
}

extern "C" int gw_deepsim_export(gw_deepsim* m, float* const par[4], float* const adam_m[4], float* const adam_v[4]) {
  if (!m) return gw_deepsim_fail(nullptr, GW_ERR_INVALID, "NULL handle");
  if (m->device >= 0) return gw_ds_dev_export(m, par, adam_m, adam_v);
  for (int t = 0; t < 4; ++t) {
    const size_t bytes = gw_ds_numel(m, t) * sizeof(float);
    if (par && par[t]) memcpy(par[t], m->par[t].data(), bytes);
    if (adam_m && adam_m[t]) memcpy(adam_m[t], m->am[t].data(), bytes);
    if (adam_v && adam_v[t]) memcpy(adam_v[t], m->av[t].data(), bytes);
  }
  return GW_OK;
}

extern "C" int gw_deepsim_vectors_dev(gw_deepsim* m, float** ptr, int64_t* pitch) {
  if (!m || !ptr || !pitch) return gw_deepsim_fail(m, GW_ERR_INVALID, "NULL argument");
  *ptr = m->device < 0 ? m->par[0].data() : gw_ds_dev_vectors(m);
  *pitch = m->p.dim;
  return GW_OK;
}

// str(numpy.float32(x)): the shortest digits that read back as x, positional
// for 1e-4 <= |x| < 1e16, else scientific with at least two exponent digits
static int format_np_float32(float x, char* out) {
  if (isnan(x)) return sprintf(out, "nan");
  if (isinf(x)) return sprintf(out, x < 0 ? "-inf" : "inf");
  if (x == 0.0f) return sprintf(out, signbit(x) ? "-0.0" : "0.0");
  char buf[32];
  int prec = 0;
  for (; prec < 9; ++prec) {
    snprintf(buf, sizeof buf, "%.*e", prec, (double)x);
    if (strtof(buf, nullptr) == x) break;
  }
  // buf = [-]d[.ddd]e[+-]XX
  const char* p = buf;
  char* o = out;
  if (*p == '-') *o++ = *p++;
  char digits[16];
  int nd = 0;
  for (; *p != 'e'; ++p)
    if (*p != '.') digits[nd++] = *p;
  const int e10 = atoi(p + 1);
  const double ax = fabs((double)x);
  if (ax >= 1e16 || ax < 1e-4) {
    *o++ = digits[0];
    if (nd > 1) {
      *o++ = '.';
      for (int i = 1; i < nd; ++i) *o++ = digits[i];
    }
    o += sprintf(o, "e%c%02d", e10 < 0 ? '-' : '+', abs(e10));
    return (int)(o - out);
  }
  if (e10 >= 0) {
    for (int i = 0; i <= e10; ++i) *o++ = i < nd ? digits[i] : '0';
    *o++ = '.';
    if (nd > e10 + 1)
      for (int i = e10 + 1; i < nd; ++i) *o++ = digits[i];
    else
      *o++ = '0';
  } else {
    *o++ = '0';
    *o++ = '.';
    for (int i = 0; i < -e10 - 1; ++i) *o++ = '0';
    for (int i = 0; i < nd; ++i) *o++ = digits[i];
  }
  *o = 0;
  return (int)(o - out);
}

extern "C" int gw_write_deepsim_text(const char* path, const float* w1, int64_t n, int dim) {
  if (!path || (!w1 && n > 0) || n < 0 || dim < 1) return gw_deepsim_fail(nullptr, GW_ERR_INVALID, "bad arguments");
  FILE* f = fopen(path, "w");
  if (!f) return gw_deepsim_fail(nullptr, GW_ERR_IO, "cannot open '%s' for writing", path);
  bool ok = fprintf(f, "%lld %d\n", (long long)n, dim) > 0;
  char buf[64];
  for (int64_t v = 0; ok && v < n; ++v) {
    ok = fprintf(f, "%lld", (long long)v) > 0;
    for (int h = 0; ok && h < dim; ++h) {
      buf[0] = ' ';
      const int len = format_np_float32(w1[v * dim + h], buf + 1);
      ok = fwrite(buf, 1, (size_t)len + 1, f) == (size_t)len + 1;
    }
    ok = ok && fputc('\n', f) != EOF;
  }
  if (fclose(f) != 0) ok = false;
  if (!ok) return gw_deepsim_fail(nullptr, GW_ERR_IO, "write to '%s' failed", path);
  return GW_OK;
}
