// internal.h -- host plumbing shared by the library's translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/slgpu.h"

// Sets the calling thread's slg_last_error() text (printf-style) and returns `code`.  Defined in
// slgpu.hip, beside the text.
int slg_internal_fail(int code, const char* fmt, ...);

// The two host functions of stats.hip the fused unit (slgpu.hip) calls: the thresholds of
// n_views views into their workspace slices (slg_decode_stats_batch's checks and launches), and
// the launch that only arms a slice's look-back words (slg_triangulate: the mask comes with the maps).
int slg_stats_batch(const slg_capture* caps, int n_views, const slg_decode_params* dp, char* ws, int64_t ws_stride,
                    hipStream_t s);
int slg_stats_arm(int64_t n_px, void* workspace, hipStream_t s);

// After a kernel launch: SLG_OK, or SLG_ERR_HIP with "<what>: <the runtime's message>".
inline int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  return SLG_OK;
}
