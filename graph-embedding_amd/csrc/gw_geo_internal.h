// gw_geo handle shared by gw_geo_host.cpp (C ABI, assembly, union-find, checks,
// host law) and gw_geo.hip (kernels).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "gw_geo_law.h"

struct gw_geo {
  int device = -1;  // -1: host evaluation
  int64_t n = 0;
  gw_geo_params_t p{};
  bool have_graph = false;
  // the assembled graph: CSR, columns ascending, lengths under the law
  std::vector<int64_t> off;
  std::vector<int32_t> col;
  std::vector<double> len;
  double delta = 1.0;  // the device schedule's bucket width in use (p.delta, or chosen at assembly)
  int64_t cap = -1;    // the device schedule's round cap from p.round_cap (-1: its own choice)
  // components of the symmetrised graph
  std::vector<int32_t> comp;
  int32_t main_comp = 0;
  gw_geo_stats_t st{};
  std::string err;
  struct gw_geo_dev* dev = nullptr;  // device state (device >= 0), defined and owned by gw_geo.hip
};

int gw_geo_fail(gw_geo* m, int code, const char* fmt, ...);
inline auto gw_fail_of(const gw_geo*) { return &gw_geo_fail; }  // for the shared plumbing (gw_trainer_device.h)

// device entry points (gw_geo.hip)
int gw_geo_dev_alloc(gw_geo* m);
void gw_geo_dev_free(gw_geo* m);
// uploads m->off, m->col, m->len
int gw_geo_dev_upload(gw_geo* m);
// sources (device memory, or NULL for 0 .. n-1) are range-checked on the device before anything is written;
// fills rounds_max, relaxations and fallbacks of m->st
int gw_geo_dev_query(gw_geo* m, const int32_t* sources, int64_t nsrc, double* out, int64_t pitch, void* stream);
