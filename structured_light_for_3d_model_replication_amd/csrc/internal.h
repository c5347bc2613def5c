// internal.h -- host plumbing shared by the library's translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/slgpu.h"

// Sets the calling thread's slg_last_error() text (printf-style) and returns `code`.  Defined in
// slgpu.hip, beside the text.
int slg_internal_fail(int code, const char* fmt, ...);

// After a kernel launch: SLG_OK, or SLG_ERR_HIP with "<what>: <the runtime's message>".
inline int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  return SLG_OK;
}
