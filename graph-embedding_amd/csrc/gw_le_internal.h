// gw_le handle shared by gw_le_host.cpp (C ABI, checks, operator assembly, the
// solver and the host law) and gw_le.hip (kernels).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/graphwalk.h"
#include "gw_le_law.h"

#define GW_LE_BLOCKS 4  // n x m blocks the solver rotates between

struct gw_le {
  int device = -1;  // -1: host evaluation
  gw_le_params_t p{};
  int64_t n = 0;
  // S as CSR (host copy in both modes) and s_i; s_i == 0 marks an isolated row
  std::vector<int64_t> off;
  std::vector<int32_t> col;
  std::vector<double> val, s;
  int64_t nz_rows = 0;  // non-isolated rows
  bool have_op = false, solved = false;
  int m = 0;       // block in use
  int skipped = 0;
  std::vector<double> theta, resid;     // [m] of the last Rayleigh-Ritz step
  std::vector<double> hb[GW_LE_BLOCKS];  // host mode: the blocks
  std::vector<double> out64;             // host mode: [n][dim]; device mode: filled by gw_le_export
  std::vector<float> out32;              // host mode: [n][dim]
  gw_le_stats_t st{};
  void* stream = nullptr;            // of the running solve
  struct gw_le_dev* dev = nullptr;   // device state (device >= 0), defined and owned by gw_le.hip
  std::string err;
};

int gw_le_fail(gw_le* m, int code, const char* fmt, ...);
inline auto gw_fail_of(const gw_le*) { return &gw_le_fail; }  // for the shared device plumbing

// device entry points (gw_le.hip).  Blocks are named by index 0 .. GW_LE_BLOCKS-1; C, Q, theta, sumsq, nrm and
// negate are host arrays (the m x m and m-long transfers of an outer iteration).
int gw_le_dev_alloc(gw_le* m);
void gw_le_dev_free(gw_le* m);
int gw_le_dev_upload(gw_le* m);   // the operator, after assembly
int gw_le_dev_prepare(gw_le* m);  // blocks and partials for m->m
int gw_le_dev_init(gw_le* m, int dst);
int gw_le_dev_apply(gw_le* m, int mode, double alpha, double beta, double gamma, int src, int dst, int z);
int gw_le_dev_gram(gw_le* m, int a, int b, double* C);
int gw_le_dev_rotate(gw_le* m, int src, int dst, const double* Q);
int gw_le_dev_resid(gw_le* m, int x, int y, const double* theta, double* sumsq);
int gw_le_dev_colstat(gw_le* m, int x, int col0, int dim, double* sumsq, int32_t* negate);
int gw_le_dev_output(gw_le* m, int x, int col0, int dim, const double* nrm, const int32_t* negate);
int gw_le_dev_export(gw_le* m, double* vectors);
int gw_le_dev_vectors(gw_le* m, float** ptr);
int gw_le_dev_apply_user(gw_le* m, const double* x, double* y, int cols);
