// capture_checks.h -- the capture checks the fused unit (slgpu.hip) and the stats unit
// (stats.hip) share.  Host only; every name is TU-local.
#pragma once
#include "internal.h"
#include "workspace.h"

namespace {

const auto fail = slg_internal_fail;       // (the units' short name for it)

int check_enough_frames(const slg_capture* cap) {
  if (cap->n_frames < 4)
    return fail(SLG_ERR_NOT_ENOUGH, "Not enough images (got %d, need at least 4).", cap->n_frames);
  return SLG_OK;
}

// The slices of a launch lie ws_stride apart: checked once there is a second one.
int check_ws_stride(bool several, int64_t ws_stride, int64_t n_px) {
  if (several && (ws_stride < ws_total(n_px) || (ws_stride & 255)))
    return fail(SLG_ERR_INVALID, "ws_stride too small or not 256-aligned");
  return SLG_OK;
}

int check_capture(const slg_capture* cap) {
  if (!cap || !cap->frames) return fail(SLG_ERR_INVALID, "capture frames is NULL");
  if (cap->height < 1 || cap->width < 1) return fail(SLG_ERR_INVALID, "bad image size %dx%d", cap->width, cap->height);
  const int64_t n_px = int64_t(cap->height) * cap->width;
  if (n_px >= (int64_t(1) << 31)) return fail(SLG_ERR_UNSUPPORTED, "image larger than 2^31 pixels");
  if (n_px * 3 + 64 >= (int64_t(1) << 32))        // texture reads take 32-bit byte offsets
    return fail(SLG_ERR_UNSUPPORTED, "image larger than 1.43e9 pixels");
  if (cap->height > 65535 || cap->width > 65535) return fail(SLG_ERR_UNSUPPORTED, "image side above 65535 pixels");
  if (cap->frame_stride < ((n_px + 7) & ~int64_t(7)) || (cap->frame_stride & 7))
    return fail(SLG_ERR_INVALID, "frame_stride must be >= round_up(H*W, 8) and a multiple of 8");
  if (reinterpret_cast<uintptr_t>(cap->frames) & 7) return fail(SLG_ERR_INVALID, "frames must be 8-byte aligned");
  if (int64_t(cap->n_frames > 0 ? cap->n_frames : 0) * cap->frame_stride >= (int64_t(1) << 32))
    return fail(SLG_ERR_UNSUPPORTED, "frame stack larger than 4 GiB");   // 32-bit buffer offsets
  return SLG_OK;
}

// Views of one launch share one geometry; `msg` says whose.
constexpr const char* kBatchGeometry = "all views of a batch must share one geometry";
int check_same_geometry(const slg_capture& cap, const slg_capture& first, const char* msg) {
  if (cap.height != first.height || cap.width != first.width) return fail(SLG_ERR_INVALID, "%s", msg);
  return SLG_OK;
}

}  // namespace
