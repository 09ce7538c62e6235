// Host plumbing shared by the device halves of the trainer families (gw_sgns.hip, gw_deepsim.hip, gw_ovr.hip).
// A handle H has `int device`, a `dev` pointer to its device state, and gw_fail_of(H*) naming its *_fail.
#pragma once
#include <new>
#include <type_traits>

#include "gw_device_common.h"

#define GW_DEV_TRY(m, expr)                                                                                 \
  do {                                                                                                      \
    hipError_t _e = (expr);                                                                                 \
    if (_e != hipSuccess) return gw_fail_of(m)((m), GW_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

// select the handle's device for the rest of the scope or fail with GW_ERR_DEVICE
#define GW_DEV_GUARD(m)                \
  gw_device_guard gw_dg_((m)->device); \
  if (!gw_dg_.ok) return gw_fail_of(m)((m), GW_ERR_DEVICE, "cannot select HIP device %d", (m)->device)

// What every *_dev_alloc does first: the device exists, and m->dev is an empty device state.
template <typename H>
int gw_trainer_open_device(H* m) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    return gw_fail_of(m)(m, GW_ERR_DEVICE, "no HIP device visible (device = -1 evaluates the law on the host)");
  if (m->device >= count) return gw_fail_of(m)(m, GW_ERR_INVALID, "device ordinal out of range");
  m->dev = new (std::nothrow) std::remove_pointer_t<decltype(m->dev)>();
  return m->dev ? GW_OK : gw_fail_of(m)(m, GW_ERR_NOMEM, "out of memory");
}

// One kernel of a family's table; dyn is the dynamic LDS its launch asks for.
struct gw_kernel_entry {
  const char* name;
  const void* fn;
  size_t dyn;
};

// *count = N; the first min(N, cap) entries of every non-NULL array are filled.
template <typename H, size_t N>
int gw_trainer_kernel_attrs(H* m, const gw_kernel_entry (&ks)[N], int cap, const char** names, int32_t* vgprs,
                            int32_t* scratch_bytes, int32_t* lds_bytes, int32_t* count) {
  if (count) *count = (int32_t)N;
  for (int i = 0; i < (int)N && i < cap; ++i) {
    hipFuncAttributes fa;
    GW_DEV_TRY(m, hipFuncGetAttributes(&fa, ks[i].fn));
    if (names) names[i] = ks[i].name;
    if (vgprs) vgprs[i] = fa.numRegs;
    if (scratch_bytes) scratch_bytes[i] = (int32_t)fa.localSizeBytes;
    if (lds_bytes) lds_bytes[i] = (int32_t)(fa.sharedSizeBytes + ks[i].dyn);
  }
  return GW_OK;
}
