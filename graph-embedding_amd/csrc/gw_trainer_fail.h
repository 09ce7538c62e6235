// The one body behind gw_sgns_fail, gw_deepsim_fail and gw_ovr_fail.  It
// includes only the C++ library, so the host-only builds of the trainers
// (-DGW_DEEPSIM_HOST_ONLY, -DGW_OVR_HOST_ONLY) can use it.
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include <string>

// Formats the message into the handle's error (handle_err may be NULL: no
// handle yet) and into *tls, the string the family's handle-less last-error
// reads.  Returns code.
inline int gw_trainer_vfail(std::string* handle_err, std::string* tls, int code, const char* fmt, va_list ap) {
  char buf[1024];
  vsnprintf(buf, sizeof buf, fmt, ap);
  if (handle_err) *handle_err = buf;
  *tls = buf;
  return code;
}
