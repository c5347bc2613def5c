// workspace.h -- the per-view device workspace (header words, look-back states, row-cloud
// scratch, per-tile Otsu partials) and the block / tile sizes its layout depends on.  Host and
// device; every name is TU-local (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace {

constexpr int kBlock = 256;                 // 4 waves of 64
constexpr int kPx = 8;                      // pixels per lane (one 8-byte load per frame)
#ifndef SLG_TILE_BLOCK
#define SLG_TILE_BLOCK 512
#endif
constexpr int kTileBlock = SLG_TILE_BLOCK;  // main3 workgroup: 512 lanes, 322.6 vs 331.3 us per
                                            // 12-view launch with 256 (half the look-backs per pixel)
constexpr int kTilePx = kTileBlock * kPx;   // 4096 pixels per main3 tile (one look-back entry)

// ------------------------------------------------------------------ workspace layout
struct WsHeader {
  uint32_t hist[3][256];   // otsu: 0 white, 1 clip(white-black,0,255); percentile: 0 black
  uint32_t max_diff_enc;   // max(white-black) + 256 (0 = none yet)
  uint32_t ticket;         // stats_kernel arrival counter
  uint32_t lb_ticket;      // main3 tiles that published their column-stream aggregate (lookback_scan)
  uint32_t error;          // bit 0: look-back spin timeout; 1: a look-back helper ran
  int32_t smin;            // mask: white >= smin
  int32_t cmin;            //       (white - black) >= cmin
  uint32_t lb_ticket_row;  // the same for the row stream (row_mode 2)
  int32_t pad0;
  double thr_s;            // float thresholds (for inspection / tests)
  double thr_c;
  int64_t totals[2];       // column / row stream point totals
  // Otsu only: pixels with white >= smin, and with white - black >= cmin (n_px when cmin <= 0,
  // which the clipped histogram cannot count); their minimum bounds the valid pixels, so the
  // point count of row_mode 0/1 (resident jobs size their clouds with it).  n_px otherwise.
  int64_t above[2];
  // Resident-job arena (slg_workspace_set_arena; NULL cursor: none).  The Otsu tail that sets a
  // view's thresholds also reserves its cloud's region: arena_off = atomicAdd(cursor, need),
  // need = min(above) * arena_mult (an upper bound of its points), or -1 when the arena has no
  // room left (the fused launch then stores nothing for it; the host re-runs it).
  int64_t arena_off;
  int32_t arena_mult;      // points per valid pixel at most: 1 (row_mode 0/1) or 2 (row_mode 2)
  int32_t pad4;
  unsigned long long* arena_cursor;
  int64_t arena_cap;       // points the arena holds
  uint64_t pad3[2];
};
constexpr int kHistCopies = 16;            // partial histograms: blocks spread their atomics
constexpr int64_t kHistPartOff = 8192;      // uint32 [kHistCopies][2][256] after the header
constexpr int64_t kHeaderBytes = 65536;
static_assert(sizeof(WsHeader) <= kHistPartOff, "header");
#define SLG_WS_AT(f, o) (offsetof(WsHeader, f) == (o))
static_assert(SLG_WS_AT(hist, 0) && SLG_WS_AT(max_diff_enc, 3072) && SLG_WS_AT(ticket, 3076) && SLG_WS_AT(lb_ticket, 3080) &&
              SLG_WS_AT(error, 3084) && SLG_WS_AT(smin, 3088) && SLG_WS_AT(cmin, 3092) && SLG_WS_AT(lb_ticket_row, 3096) &&
              SLG_WS_AT(pad0, 3100) && SLG_WS_AT(thr_s, 3104) && SLG_WS_AT(thr_c, 3112) && SLG_WS_AT(totals, 3120) &&
              SLG_WS_AT(above, 3136) && SLG_WS_AT(arena_off, 3152) && SLG_WS_AT(arena_mult, 3160) && SLG_WS_AT(pad4, 3164) &&
              SLG_WS_AT(arena_cursor, 3168) && SLG_WS_AT(arena_cap, 3176) && SLG_WS_AT(pad3, 3184) && sizeof(WsHeader) == 3200,
              "the header the host reads: engine.py's WS_HEADER dtype names every field (tests/test_ws_header.py)");
#undef SLG_WS_AT

__host__ __device__ inline int64_t n_tiles_of(int64_t n_px) { return (n_px + kTilePx - 1) / kTilePx; }
__host__ __device__ inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
__host__ __device__ inline int64_t states_off(int64_t) { return kHeaderBytes; }
__host__ __device__ inline int64_t n_state_words(int64_t n_px) { return 2 * n_tiles_of(n_px); }   // [stream][tile]
__host__ __device__ inline int64_t states_bytes(int64_t n_px) { return align_up(n_state_words(n_px) * 8, 256); }
__host__ __device__ inline int64_t scratch_xyz_off(int64_t n_px) { return kHeaderBytes + states_bytes(n_px); }
__host__ __device__ inline int64_t scratch_bgr_off(int64_t n_px) { return scratch_xyz_off(n_px) + align_up(n_px * 24, 256); }
__host__ __device__ inline int64_t parts_off(int64_t n_px) { return scratch_bgr_off(n_px) + align_up(n_px * 3, 256); }
// per tile: the Otsu histograms of the batch after next over the tile's pixels, u16 [2][256]
constexpr int64_t kPartWords = 256;         // packed u16 pairs per tile
__host__ __device__ inline int64_t ws_total(int64_t n_px) { return parts_off(n_px) + align_up(n_tiles_of(n_px) * kPartWords * 4, 256); }

}  // namespace
