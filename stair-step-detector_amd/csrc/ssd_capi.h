/*
 * ssd_capi.h — what the units of the C ABI that call HIP share.  Internal to libssd_hip.so: hidden like
 * ssd_host.h, which it includes, so the library exports what include/ssd_hip.h declares and nothing of this.
 *
 * The units today: ssd_capi.hip, everything that runs on a handle, and ssd_capi_device.cpp, plain C++, the entries that take no handle
 * but call HIP; the device unit uses HIP_TRY and hip_fail and nothing else of ssd_capi.hip, and no ssd_handle.  ssd_capi.hip holds five
 * layers top to bottom - core (handle life, settings, enqueue_impl, fetch, timing), the host feed, the camera table, the ordered passes
 * behind a whole enqueue, the stand-alone frame passes - each using only the layers above it; a layer that becomes a unit of its own
 * (plain C++, HOST_SRCS in the Makefile) declares here exactly what crosses its boundary, in a section named after the layer that
 * defines it, and keeps everything else static.
 */
#ifndef SSD_CAPI_H_
#define SSD_CAPI_H_

#include "ssd_owned.h"
#include "ssd_host.h"

#include <string>

#pragma GCC visibility push(hidden)

#define HIP_TRY(expr)                                                                                   \
  do                                                                                                    \
  {                                                                                                     \
    const hipError_t e_ = (expr);                                                                       \
    if(e_ != hipSuccess)                                                                                \
      return fail(SSD_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                        \
  } while(0)

/* a failed HIP call as a return code: SSD_E_NOMEM or SSD_E_HIP (ssd_owned.h), `what` in front of HIP's text */
inline int hip_fail(hipError_t e, const std::string &what)
{
  return fail(ssd::hip_error_code(e), what + hipGetErrorString(e));
}

#pragma GCC visibility pop

#endif
