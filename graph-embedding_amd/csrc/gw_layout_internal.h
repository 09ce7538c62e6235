// gw_layout handle shared by gw_layout_host.cpp (C ABI, the matrix's checks, host
// law) and gw_layout.hip (kernels).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "gw_layout_law.h"

struct gw_layout {
  int device = -1;  // -1: host evaluation
  int64_t n = 0;
  int dim = 2;
  gw_layout_params_t p{};
  bool have_graph = false;
  // the matrix as listed, less the diagonal: CSR in stored order
  std::vector<int64_t> off;
  std::vector<int32_t> col;
  std::vector<double> val;
  std::vector<uint8_t> fixed;  // [n]: 1 = the vertex does not move
  std::string err;
  struct gw_layout_dev* dev = nullptr;  // device state (device >= 0), defined and owned by gw_layout.hip
};

int gw_layout_fail(gw_layout* m, int code, const char* fmt, ...);
inline auto gw_fail_of(const gw_layout*) { return &gw_layout_fail; }  // for the shared plumbing (gw_trainer_device.h)

inline int64_t gw_layout_chunks(int64_t n) { return (n + GW_LAYOUT_CHUNK - 1) / GW_LAYOUT_CHUNK; }
inline int64_t gw_layout_blocks(int64_t n) { return (n + GW_LAYOUT_BLOCK - 1) / GW_LAYOUT_BLOCK; }

// device entry points (gw_layout.hip); k is the one in use (never 0)
int gw_layout_dev_alloc(gw_layout* m);
void gw_layout_dev_free(gw_layout* m);
int gw_layout_dev_upload(gw_layout* m);        // m->off, m->col, m->val
int gw_layout_dev_upload_fixed(gw_layout* m);  // m->fixed
int gw_layout_dev_run(gw_layout* m, double* pos, double k, int32_t iterations, double threshold, void* stream,
                      int32_t* iterations_done);
int gw_layout_dev_step(gw_layout* m, const double* pos_in, double k, double t, double* disp_out, double* pos_out,
                       void* stream);
int gw_layout_dev_rescale(gw_layout* m, double* pos, double scale, const double* center, void* stream);
