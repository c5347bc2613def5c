// fused_params.h -- the kernel arguments of the fused path: the decode plan, the launch-wide
// MainParams, the per-view ViewIO / FinIO and main3's Main3Params, with their layout checks.
// Host and device; every name is TU-local.
#pragma once
#include "workspace.h"

namespace {

constexpr int kMaxViews = 16;               // views per main3 launch

// Decode plan of one view: per axis, the frame index of the first pattern, the pairs to read,
// the pre-shift and the post-shift (make_plan).
struct Plan {
  int32_t col_first, col_pairs, col_pre, col_post;
  int32_t row_first, row_pairs, row_pre, row_post;
};

struct MainParams {
  // frames source
  const uint8_t* frames;
  int64_t stride;
  // maps source
  const int32_t* in_col;
  const int32_t* in_row;
  const uint8_t* in_mask;
  // common
  const uint8_t* texture;
  int64_t n_px;
  int32_t width;
  Plan plan;
  // maps output
  int32_t* out_col;
  int32_t* out_row;
  uint8_t* out_mask;
  // calibration
  const double* rays;
  double fx, fy, cx, cy;
  double rfx, rfy;            // RN(1/fx), RN(1/fy) when div_fast (Markstein divisions)
  int32_t div_fast;
  int32_t rays_fast;          // host-verified: every pixel's ray takes the Markstein path (tri_item FAST)
  double o0, o1, o2;
  int32_t num_pre;            // pcol (and prow in row_mode 2): split pair planes with numer, not d
  int32_t pad_np;
  const double* pcol;
  int32_t n_pcol;
  const double* prow;
  int32_t n_prow;
  double tol;
  // outputs
  void* xyz;
  uint8_t* bgr;
  int64_t* count;
  WsHeader* ws;
  uint64_t* states;        // [2][n_tiles]
  int64_t n_tiles;
  void* scratch_xyz;       // row_mode 2 row cloud
  uint8_t* scratch_bgr;
  int32_t dbg;             // env SLG_DBG; read only by the profiling instance (PROF): bit0 no
                           // look-back wait, bit1 trivial triangulation, bit2 no output stores,
                           // bit3 no BGR stores, bit6 per-workgroup phase records, bit7 no XYZ stores
  uint32_t help_after;     // look-back: s_sleep(2) units before a silent predecessor is helped
                           // (kHelpAfter; env SLG_HELP_AFTER=0 forces the helper path in tests)
};

struct ViewIO {
  const uint8_t* frames;      // SRC_FRAMES: [F][stride]
  const uint8_t* texture;     // [n_px][3] BGR
  const int32_t* in_col;      // !SRC_FRAMES: maps
  const int32_t* in_row;
  const uint8_t* in_mask;
  void* xyz;
  uint8_t* bgr;
  int64_t* count;
  WsHeader* ws;
  uint64_t* states;           // [2][n_tiles]
  void* scratch_xyz;          // row_mode 2 row cloud
  uint8_t* scratch_bgr;
  int64_t stride;             // frame stride of this view
  Plan plan;                  // decode plan of this view (frames present)
  const uint8_t* hn_white;    // batch after next: white / black of the view in this slot, whose
  const uint8_t* hn_black;    // Otsu histograms this launch computes per tile (NULL: none)
  uint32_t* hn_part;          // -> [n_tiles][kPartWords] of this view's workspace slice
};

// A view whose Otsu partials (carried by an EARLIER launch on the same stream) this launch
// turns into thresholds, with finishing workgroups placed at the front of its grid: the
// streaming pipeline's stats pass then costs no kernel and no cross-stream wait of its own.
struct FinIO {
  const uint32_t* parts;      // [n_tiles][kPartWords] partials in the view's workspace slice
  WsHeader* ws;               // the slice: thresholds out, look-back words armed
};

struct Main3Params {
  MainParams c;               // geometry, decode plan, calibration (per-view pointers unused)
  int32_t n_views;
  int32_t n_fin;              // views finished by this launch (FinIO), 0: none
  int32_t fin_blocks;         // finishing workgroups per such view (the grid's first n_fin*fin_blocks)
  int32_t pad_m3;
  int64_t n_state_words;      // look-back words per view slice (finishing arms them)
  int64_t pad_zero;           // zero bytes the last tile's partial counted past n_px
  ViewIO v[kMaxViews];
  FinIO fin[kMaxViews];
};

static_assert(sizeof(Main3Params) <= 4096, "kernel arguments");
static_assert(sizeof(Plan) == 32 && offsetof(MainParams, plan) == 60 && offsetof(MainParams, out_col) == 96 &&
              sizeof(MainParams) == 328 && offsetof(ViewIO, plan) == 104 && offsetof(ViewIO, hn_white) == 136 &&
              sizeof(ViewIO) == 160, "kernel argument layout (Plan sits where its eight fields did)");

__device__ inline MainParams view_params(const Main3Params& P, int view) {
  MainParams q = P.c;
  const ViewIO& io = P.v[view];
  q.frames = io.frames; q.texture = io.texture;
  q.in_col = io.in_col; q.in_row = io.in_row; q.in_mask = io.in_mask;
  q.xyz = io.xyz; q.bgr = io.bgr; q.count = io.count;
  q.ws = io.ws; q.states = io.states;
  q.scratch_xyz = io.scratch_xyz; q.scratch_bgr = io.scratch_bgr;
  q.stride = io.stride;
  q.plan = io.plan;
  return q;
}

}  // namespace
