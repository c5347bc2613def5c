// slgpu.hip -- the structured-light hot path on MI355X (gfx950, CDNA4): the fused decode +
// triangulate kernel, its launch code and the C ABI entries that run it.
//
// Path (reference): Gray-code decode  server/processing.py:28-124, server/sl_system.py:516-588
//                   ray-plane triangulation  server/processing.py:127-234, sl_system.py:592-661
// C ABI: include/slgpu.h.  Design and rooflines: DESIGN.md; the files of csrc/: DESIGN.md §11.
// main3_kernel and everything it inlines (fused_params.h, decode.h, triangulate.h, lookback.h,
// carried_hist.h, otsu.h) stay in this one translation unit and in the anonymous namespace:
// main3_symbol() spells the mangled name.
//
// Kernels here
//   main3_kernel<...> fused decode + triangulate + ordered compaction, one 4096-pixel tile per
//                     workgroup, up to 16 views per launch (phases A to D: the comment at the
//                     kernel); the grid's first workgroups can turn a carried batch's Otsu
//                     partials into thresholds.
//   decode_maps_kernel  the decode alone, to correspondence maps (slg_decode).
//   row_tail_kernel   row_mode 2: moves the row cloud behind the column cloud.
//   set_arena_kernel  the resident-job arena words of the workspace headers.
//   pinhole_kernel    bitwise Nc == pinhole(cam_K) test.
// Host side: argument checks and the decode plan, the main3 instance table (pick_main refuses an
// instance the library's code object lacks), the batched launch code, the C ABI.
//
// Numerics: every floating-point expression follows NumPy's operation order with
// -ffp-contract=off (no FMA contraction), IEEE-correct f64 division and sqrt, so the fp64
// results equal the reference bit for bit; integer/byte work is exact by construction.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <limits.h>
#include <type_traits>
#include <stdlib.h>
#include <math.h>
#include <string>
#include <vector>
#include <algorithm>
#include <mutex>
#include <dlfcn.h>

#include "capture_checks.h"
#include "code_object.h"
#include "fused_params.h"
#include "decode.h"
#include "triangulate.h"
#include "lookback.h"
#include "carried_hist.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMapsPx = kBlock * kPx;       // 2048 pixels per decode_maps workgroup

// Correspondence maps of 2048 pixels per workgroup (slg_decode): col/row int32, mask uint8.
// (Plan-specialised instances as main3's measured the same: 21.3 vs 21.4 us at 1080p, r3an2.)
__global__ __launch_bounds__(kBlock) void decode_maps_kernel(MainParams p) {
  const int64_t px0 = int64_t(blockIdx.x) * kMapsPx + int64_t(threadIdx.x) * kPx;
  const bool tail = px0 + kPx > p.n_px;       // lane-level guard for the ragged end
  uint32_t valid;
  int col[kPx], row[kPx];
  decode_lane<1, 1, 8>(p, px0, tail, valid, col, row);
  if (px0 + kPx <= p.n_px) {
    int4* oc = reinterpret_cast<int4*>(p.out_col + px0);
    int4* orr = reinterpret_cast<int4*>(p.out_row + px0);
    oc[0] = make_int4(col[0], col[1], col[2], col[3]);
    oc[1] = make_int4(col[4], col[5], col[6], col[7]);
    orr[0] = make_int4(row[0], row[1], row[2], row[3]);
    orr[1] = make_int4(row[4], row[5], row[6], row[7]);
    uint32_t m0 = 0, m1 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      m0 |= ((valid >> k) & 1u) << (8 * k);
      m1 |= ((valid >> (k + 4)) & 1u) << (8 * k);
    }
    *reinterpret_cast<uint2*>(p.out_mask + px0) = make_uint2(m0, m1);
  } else {
    for (int k = 0; k < kPx; ++k)
      if (px0 + k < p.n_px) {
        p.out_col[px0 + k] = col[k];
        p.out_row[px0 + k] = row[k];
        p.out_mask[px0 + k] = uint8_t((valid >> k) & 1u);
      }
  }
}

// ------------------------------------------------------------------ main3: occupancy-first fused kernel
// One launch covers up to kMaxViews views of one geometry (grid = tiles x views, views
// interleaved).  Per kTileBlock-lane workgroup and kTilePx-pixel tile:
//  A  every lane decodes its 8 pixels (all used frames in flight, 8-byte coalesced loads); a
//     block scan compacts the tile's valid pixels into LDS items (code, BGR, pixel offset);
//  B  the lanes triangulate the items one workgroup-width at a time (fp64, NumPy order) --
//     balanced over the waves whatever the foreground layout; points stay in registers and one ballot
//     per wave and round gives every kept point its rank;
//  C  one barrier shares the per-(round, wave) counts, wave 0 resolves the tile's offset by
//     decoupled look-back (helping a long-silent predecessor, so waiting always ends);
//  D  each lane stores its points at offset + rank: consecutive lanes write consecutive
//     points, so the compacted stores coalesce without an LDS staging copy.
// 49 KB of LDS (24 KB at 256 lanes) and no point staging keep two 512-lane workgroups per CU
// resident, so one tile's decode stream overlaps another's fp64 work and look-back.
#ifndef SLG_DECODE_BATCH
#define SLG_DECODE_BATCH 11                // pairs per axis in flight per lane (4/6/8/11: 31.7/30.3/28.7/27.5 us/view)
#endif
#ifndef SLG_M3_WAVES
#define SLG_M3_WAVES 4                     // waves per SIMD main3 is register-budgeted for
#endif

// BGR bytes of pixel k (0..7) from the lane's 24 texture bytes t[0..5].
__device__ inline uint32_t bgr_of(const uint32_t (&t)[6], int k) {
  const int b = 3 * k, w = b >> 2, s = 8 * (b & 3);
  const uint64_t pair = uint64_t(t[w]) | (uint64_t(w + 1 < 6 ? t[w + 1] : 0u) << 32);
  return uint32_t(pair >> s) & 0xffffffu;
}

// Block-wide exclusive scan of one int per lane: (exclusive prefix, block total).
__device__ inline int2 block_scan(int x, int* s_wtot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(incl, o);
    if (lane >= o) incl += y;
  }
  if (lane == 63) s_wtot[wave] = incl;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kTileBlock / 64; ++w) {
    off += w < wave ? s_wtot[w] : 0;
    tot += s_wtot[w];
  }
  return make_int2(off + incl - x, tot);
}

#ifndef SLG_X64_KEEP_T
#define SLG_X64_KEEP_T 1                   // f64 XYZ, pinhole rays: t in registers, ray recomputed in phase D
#endif

// PROF: the profiling instance (SLG_DBG set): honours the ablation bits of MainParams::dbg and
// writes per-workgroup phase records; the production instances carry none of that code.
constexpr int kPlanGray = 0x100;           // PLAN bit: every view of the launch is a gray capture

template <int ROW_MODE, int XYZ64, int SRC_FRAMES, int RAYS, bool PROF, int PLAN = 0>
__global__ __launch_bounds__(kTileBlock, ROW_MODE == 2 && XYZ64 ? 2 : SLG_M3_WAVES) void main3_kernel(Main3Params P) {
  using XT = typename std::conditional<XYZ64 != 0, double, float>::type;
  constexpr int NS = ROW_MODE == 2 ? 2 : 1;
  constexpr int kB = kTileBlock;
  constexpr int kIt = kTilePx / kB;        // 8 item rounds of one workgroup at most
  __shared__ __attribute__((aligned(16))) uint2 s_item[kItemSlots];  // valid item: (col | row << 16, u | v << 16)
  __shared__ uint32_t s_bgr[kBgrSlots];    // its BGR (24 bits)
  __shared__ int s_wtot[kB / 64];
  __shared__ int s_cnt[NS][kIt][kB / 64];  // kept points per (round, wave)
  __shared__ int s_loc[NS][kIt][kB / 64];  // their exclusive offsets within the tile (phase C)
  __shared__ uint64_t s_excl[NS];
  // the carried batch's nibble planes and histograms in LDS of their own (68 KB per workgroup,
  // two per CU): each wave stages its lane data as soon as phase A ends, no extra barrier
  // (289.7 vs 291.6 us per launch against aliasing the item arrays after phase B)
  __shared__ __attribute__((aligned(16))) uint2 s_hstage[(kB / 64) * 256];   // [wave][4 planes][64 lanes]
  __shared__ uint32_t s_hn[512];                                      // histograms

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = int(P.c.n_tiles);
  const int n_fin_wg = P.n_fin * P.fin_blocks;      // finishing workgroups come first
  if (int(blockIdx.x) < n_fin_wg) {
    const int fv = int(blockIdx.x) / P.fin_blocks;
    otsu_from_parts(P.fin[fv].parts, P.fin[fv].ws, tiles, P.c.n_px, P.n_state_words, P.pad_zero,
                    int(blockIdx.x) - fv * P.fin_blocks, P.fin_blocks, reinterpret_cast<uint32_t*>(s_item), s_bgr);
    static_assert(kPartsLdsWords * 4 <= sizeof(s_item), "the finishing workgroups' Otsu LDS");
    return;
  }
  const int bid = int(blockIdx.x) - n_fin_wg;
  // Views interleaved in dispatch order: each view's look-back chain has only ~1/n_views of
  // the resident workgroups in flight, so a tile waits on fewer, similar predecessors.
  const int tile = bid / P.n_views;
  const int view = bid - tile * P.n_views;
  const MainParams p = view_params(P, view);
  // resident-job arena (WsHeader::arena_off, set with the thresholds by an earlier kernel): the
  // view's column cloud starts at aoff in the arena the cloud pointers name; -1: no room, store nothing
  const int64_t aoff = p.ws->arena_cursor ? p.ws->arena_off : 0;
  const int64_t tile_px = int64_t(tile) * kTilePx;
  const int64_t px0 = tile_px + int64_t(tid) * kPx;
  const bool tail = tile == tiles - 1;               // block-uniform: guarded reads only here
  const int tile_v0 = int(tile_px / p.width);
  // PROF, SLG_DBG bit 6: per workgroup one 32-byte record {A decode, B triangulate, C
  // look-back, D stores (100 MHz ticks), look-back polls, sleep units, items, start} written to
  // view 0's partials region (tools/kbench.py "phases"; the host refuses it when a batch is
  // carried, whose partials live there).
  const bool prof = PROF && (p.dbg & 64) != 0;
  uint64_t t_phase = prof ? __builtin_amdgcn_s_memrealtime() : 0;
  // the record lives in LDS (tid 0 writes it): as a register array it pushed the profiling
  // instance into VGPR spills once the production decode reached the register limit
  __shared__ uint32_t s_rec[8];
  if (prof && tid == 0) s_rec[7] = uint32_t(t_phase);                // start time (low 32 bits)
  auto stamp = [&](int k) {
    if (prof) {                                      // every lane keeps the time: a scalar, no VGPR pair
      const uint64_t t = __builtin_amdgcn_s_memrealtime();
      if (tid == 0) s_rec[k] = uint32_t(t - t_phase);
      t_phase = t;
    }
  };

  // stats pass of the batch after next (hist_next_*): loads now, counting during phase C
  const bool hn = P.v[view].hn_part != nullptr;     // block-uniform
  uint2 hn_w, hn_b;
  if (hn) {
    hist_next_load(P.v[view].hn_white, P.v[view].hn_black, p.n_px, px0, hn_w, hn_b);
  }
  // ------------------------------------------------------------ A: decode + tile compaction
  int n_items;
  {
    uint32_t tex[6] = {0, 0, 0, 0, 0, 0};
    // texture NULL: a gray capture, whose cv2.imread(files[0]) is frame 0 replicated -- the white
    // bytes decode_lane has already read give the colour, no texture bytes are read at all.
    // Plan instances fix it at compile time (kPlanGray set: gray; clear: colour, the texture code
    // exactly as before -- a run-time test cost colour captures 1.4 %, profiles/r4r); the generic
    // instance tests each view.
    const bool gray = (PLAN & kPlanGray) != 0 || ((PLAN & 0xff) == 0 && p.texture == nullptr);
    auto load_tex = [&](uint2 white) {
      if (gray) {
        tex[0] = white.x;
        tex[1] = white.y;
      } else if (!tail) {
        const uint32_t tq = uint32_t(px0) * 3u;   // n_px * 3 < 2^32 (host: slg_capture checks)
        const uint2 t0 = ld_once8_buf(p.texture, tq), t1 = ld_once8_buf(p.texture, tq + 8u),
                    t2 = ld_once8_buf(p.texture, tq + 16u);
        tex[0] = t0.x; tex[1] = t0.y; tex[2] = t1.x; tex[3] = t1.y; tex[4] = t2.x; tex[5] = t2.y;
      } else {
        for (int k = 0; k < 3 * kPx; ++k)
          if (px0 * 3 + k < p.n_px * 3) tex[k >> 2] |= uint32_t(p.texture[px0 * 3 + k]) << (8 * (k & 3));
      }
    };
    uint32_t valid;
    int col[kPx], row[kPx];
    if constexpr (SRC_FRAMES) {
      // mask first: a lane with a valid pixel issues its texture loads, then its pattern loads
      decode_lane<ROW_MODE, SRC_FRAMES, SLG_DECODE_BATCH, true, PLAN>(p, px0, tail, valid, col, row, load_tex);
    } else {
      // maps source (slg_triangulate): only lanes with a valid pixel read their 24 texture
      // bytes, once the mask is known (the block scan's barrier covers part of the latency)
      decode_lane<ROW_MODE, SRC_FRAMES, SLG_DECODE_BATCH, false, PLAN>(p, px0, tail, valid, col, row);
      if (valid != 0u) load_tex(make_uint2(0u, 0u));
    }
    const int2 sc = block_scan(__popc(valid), s_wtot);
    n_items = sc.y;
    int m = sc.x;
    int u = int(tile_px - int64_t(tile_v0) * p.width) + tid * kPx, v = tile_v0;   // lane's first pixel
    while (u >= p.width) { u -= p.width; ++v; }
#pragma unroll
    for (int k = 0; k < kPx; ++k) {
      if (valid & (1u << k)) {
        s_item[item_slot(m)] = make_uint2(pack_code<ROW_MODE>(p, col[k], row[k]), uint32_t(u) | (uint32_t(v) << 16));
        s_bgr[bgr_slot(m)] = gray ? ((tex[k >> 2] >> (8 * (k & 3))) & 0xffu) * 0x010101u : bgr_of(tex, k);
        ++m;
      }
      if (++u == p.width) { u = 0; ++v; }
    }
  }
  __syncthreads();

  stamp(0);
  if (hn) {                                          // block-uniform; counted in phase C
    for (int i = tid; i < 512; i += kB) s_hn[i] = 0;
    hist_next_stage(hn_w, hn_b, p.n_px, px0, s_hstage);
  }
  // ------------------------------------------------------------ B: triangulate, balanced
  // Item m = tid + kB * i: every wave gets an equal share of the tile's valid pixels.
  // Points stay in registers across the look-back (recomputing them after it instead frees
  // ~15 VGPRs for a fifth wave per SIMD but measured 6% slower).
  // f64 XYZ with pinhole rays (x64_keep_t): only t (and tr) stay in registers across the look-back
  // -- 48 VGPRs of points pushed the instance past 128 VGPRs into scratch -- and phase D
  // recomputes the ray from the item's (u, v): the same code on the same inputs, the same bits.
  constexpr bool KT = XYZ64 && RAYS == SLG_RAYS_PINHOLE && SLG_X64_KEEP_T;
  constexpr int NC = KT ? 1 : 3;
  // the static round schedules (tri_rounds_static), but for row_mode 2 with f32 XYZ: two streams
  // of points at 128 VGPRs already spill under the grouped schedule, which that instance keeps
  constexpr int kStatic = (ROW_MODE == 2 && !XYZ64) ? 0 : SLG_TRI_STATIC;
  XT pts[NS][kIt][NC];
  uint64_t km[NS][kIt];
  // the grouped schedule: full groups, then a pair, then a single round: the tail takes at most
  // 3 rounds, so groups of 1, 2 or 4 (8 left rounds 4..7 of a tile uncomputed: wrong counts,
  // caught by bench verify)
  static_assert(kIt % SLG_TRI_GROUP == 0 && (SLG_TRI_GROUP == 1 || SLG_TRI_GROUP == 2 || SLG_TRI_GROUP == 4),
                "grouped rounds");
  const bool trivial = PROF && (p.dbg & 2);          // ablation: no triangulation arithmetic
  if (p.rays_fast && !trivial) {
    // Several rounds per step: independent straight-line fp64 chains per lane whose plane
    // gathers (L2, high latency under the streaming load) are all in flight together.  The
    // tile's round count is block-uniform, so no empty round is computed: one straight-line
    // schedule per round count (tri_rounds_static), or, where kStatic is 0, full groups of
    // SLG_TRI_GROUP rounds, then a pair, then a single round.
    const int rounds = (n_items + kB - 1) / kB;
    int i = 0;
    auto all_rounds = [&](auto np) {
      constexpr int NP = decltype(np)::value;
      // static schedules: the straight-line instance of the tile's round count -- up to
      // SLG_TRI_STATIC rounds every gather in one round trip, longer tiles (none in the C2
      // views) as rounds 0..3, then the rest; SLG_TRI_STATIC 0 keeps the grouped schedule below
      static_assert(SLG_TRI_STATIC == 0 || (SLG_TRI_STATIC >= 4 && SLG_TRI_STATIC <= 8), "static round schedules");
      if constexpr (kStatic > 0) {
        auto stat = [&](auto rc) {
          constexpr int R = decltype(rc)::value;
          if constexpr (R <= kStatic && R <= kIt) {
            tri_rounds_static<0, R, ROW_MODE, RAYS, XT, NS, kIt, NP, NC, PROF ? 2 : 0>(p, n_items, s_item, pts, km);
          } else if constexpr (R > 4 && R <= kIt) {
            tri_rounds_static<0, 4, ROW_MODE, RAYS, XT, NS, kIt, NP, NC>(p, n_items, s_item, pts, km);
            tri_rounds_static<4, R - 4, ROW_MODE, RAYS, XT, NS, kIt, NP, NC>(p, n_items, s_item, pts, km);
          }
        };
        switch (rounds) {
          case 1: stat(std::integral_constant<int, 1>()); break;
          case 2: stat(std::integral_constant<int, 2>()); break;
          case 3: stat(std::integral_constant<int, 3>()); break;
          case 4: stat(std::integral_constant<int, 4>()); break;
          case 5: stat(std::integral_constant<int, 5>()); break;
          case 6: stat(std::integral_constant<int, 6>()); break;
          case 7: stat(std::integral_constant<int, 7>()); break;
          case 8: stat(std::integral_constant<int, 8>()); break;
          default: break;                            // no item: nothing to triangulate
        }
        i = rounds;
        return;
      }
#pragma unroll
      for (int g = 0; g + SLG_TRI_GROUP <= kIt; g += SLG_TRI_GROUP)
        if (i + SLG_TRI_GROUP <= rounds) {
          tri_rounds_at<SLG_TRI_GROUP, ROW_MODE, RAYS, XT, NS, kIt, NP>(p, g, n_items, s_item, pts, km);
          i = g + SLG_TRI_GROUP;
        }
      if (SLG_TRI_GROUP > 2 && i + 2 <= rounds) {
        tri_rounds_at<2, ROW_MODE, RAYS, XT, NS, kIt, NP>(p, i, n_items, s_item, pts, km);
        i += 2;
      }
      if (i < rounds) {
        tri_rounds_at<1, ROW_MODE, RAYS, XT, NS, kIt, NP>(p, i, n_items, s_item, pts, km);
        i += 1;
      }
    };
    // numerator tables or not: a block-uniform choice between two straight-line instances,
    // so neither computes the other's numerator and selects
    if (p.num_pre) all_rounds(std::integral_constant<int, 1>());
    else all_rounds(std::integral_constant<int, 2>());
#pragma unroll
    for (int r = 0; r < kIt; ++r)
      if (r >= i) {
#pragma unroll
        for (int s2 = 0; s2 < NS; ++s2) km[s2][r] = 0;
      }
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < kIt; ++r) {
#pragma unroll
        for (int s2 = 0; s2 < NS; ++s2) s_cnt[s2][r][wave] = __popcll(km[s2][r]);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < kIt; ++i) {
#pragma unroll
      for (int s = 0; s < NS; ++s) km[s][i] = 0;
      if (i * kB < n_items) {                          // block-uniform
        const int m = tid + kB * i;
        const bool in = m < n_items;
        const uint2 it = s_item[item_slot(m)];          // read unconditionally (m < kTilePx) ...
        const uint32_t sc = it.x, suv = it.y;
        const uint32_t code = in ? sc : 0u, uv = in ? suv : 0u;   // ... garbage past n_items masked
        const int u = int(uv & 0xffffu), v = int(uv >> 16);
        TriOut o{};
        if (trivial) {                                 // the item's words as its point, kept by every stream
          o.x = double(code & 0xffff); o.y = double(code >> 16); o.z = double(u); o.rx = double(v);
          o.keep = ROW_MODE == 2 ? 3u : 1u;
        } else {
          o = tri_item<ROW_MODE, RAYS>(p, code, u, v);
        }
        tri_store(o, in ? o.keep : 0u, i, pts, km);
      }
      if (lane == 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) s_cnt[s][i][wave] = __popcll(km[s][i]);
      }
    }
  }
  __syncthreads();

  stamp(1);
  // ------------------------------------------------------------ C: tile offset (look-back)
  uint32_t polls = 0, naps = 0;
  if (wave == 0) {
#pragma unroll 1
    for (int s = 0; s < NS; ++s) {
      // one lane per (round, wave) count: the tile aggregate and, for phase D, each (round,
      // wave)'s offset within the tile -- one wave-wide scan instead of per-round sums later
      constexpr int kEnt = kIt * (kB / 64);           // 64 for 512-lane tiles, 32 for 256
      static_assert(kEnt <= 64, "one lane per (round, wave)");
      const int cnt = lane < kEnt ? (&s_cnt[s][0][0])[lane] : 0;
      int incl = cnt;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
      }
      if (lane < kEnt) (&s_loc[s][0][0])[lane] = incl - cnt;
      const int agg = __shfl(incl, 63);
      uint64_t* st = p.states + int64_t(s) * tiles;
      uint64_t excl;
      int ht;
      // a lone view's launch: the last tile to publish scans them all (lookback_scan: 1.3 us
      // off a one-view call; in 16-view launches the walks are hidden and the scan cost 1.3 %;
      // views of more than kScanTiles tiles span several waves of workgroups, whose staggered
      // walks end sooner, while the scan of every tile would delay the last one)
      const bool lone = P.n_views == 1 && tiles <= kScanTiles;
      if (!(lone && lookback_scan<PROF>(p, st, tile, tiles, agg, s == 0 ? &p.ws->lb_ticket : &p.ws->lb_ticket_row, excl)))
      while (!lookback_scalar<PROF>(p, st, tile, agg, lone, excl, ht, polls, naps)) {
        // a predecessor has not published for long (it may not be dispatched yet): publish
        // its aggregate for it, computed by this wave, and look back again
        const int hagg = tile_keep_count_wave<ROW_MODE, SRC_FRAMES, RAYS>(p, ht, s);
        if (lane == 0) {
          publish_agg(&st[ht], hagg);
          atomicOr(&p.ws->error, 2u);                // diagnostic: a helper ran (not an error)
        }
      }
      if (lane == 0) {
        s_excl[s] = excl;
        if (tail) {
          p.ws->totals[s] = int64_t(excl) + agg;
          if (ROW_MODE != 2) *p.count = int64_t(excl) + agg;
          if (s == 0 && p.ws->arena_cursor) p.count[1] = aoff;   // arena mode: count[2]
        }
      }
    }
  } else if (hn) {                                   // waves 1..: next-batch histograms meanwhile
    hist_next_count(s_hstage, s_hn, wave - 1, kB / 64 - 1);
  }
  __syncthreads();
  if (hn) hist_next_write(s_hn, P.v[view].hn_part + int64_t(tile) * kPartWords);

  stamp(2);
  // ------------------------------------------------------------ D: ordered stores from registers
  if (PROF && (p.dbg & 4)) return;                   // ablation: no output stores
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  // the point of round i, stream s: from registers, or (KT) Oc + r * t with the ray recomputed
  auto point_of = [&](int s, int i, XT& x, XT& y, XT& z) {
    if constexpr (KT) {
      const uint32_t uv = s_item[item_slot(tid + kB * i)].y;
      double r0, r1, r2;
      if (p.rays_fast) tri_ray<RAYS, true>(p, int(uv & 0xffffu), int(uv >> 16), r0, r1, r2);
      else tri_ray<RAYS, false>(p, int(uv & 0xffffu), int(uv >> 16), r0, r1, r2);
      const double t = pts[s][i][0];
      x = p.o0 + r0 * t; y = p.o1 + r1 * t; z = p.o2 + r2 * t;
    } else {
      x = pts[s][i][0]; y = pts[s][i][NC - 1 < 1 ? 0 : 1]; z = pts[s][i][NC - 1];
    }
  };
  // (tried and measured no faster, in git history: BGR staged through LDS as 16-byte stores,
  // phase D's LDS reads hoisted, non-temporal stores, f64 XYZ through a per-wave LDS window or
  // as 16 + 8-byte stores -- DESIGN.md §4)
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int64_t base = int64_t(s_excl[s]) + (s == 0 ? aoff : 0);
    XT* gx = reinterpret_cast<XT*>(s == 0 ? p.xyz : p.scratch_xyz);
    uint8_t* gb = s == 0 ? p.bgr : p.scratch_bgr;
    if (s == 0 && aoff < 0) continue;                // arena without room for the view
#pragma unroll
    for (int i = 0; i < kIt; ++i) {
      if ((km[s][i] >> lane) & 1ull) {
        const int l = s_loc[s][i][wave] + __popcll(km[s][i] & lt);
        const int64_t q = base + l;
        const uint32_t c = s_bgr[bgr_slot(tid + kB * i)];
        if (!(PROF && (p.dbg & 128))) {              // PROF ablation bit 7: no XYZ stores
          XT x, y, z;
          point_of(s, i, x, y, z);
          gx[3 * q] = x; gx[3 * q + 1] = y; gx[3 * q + 2] = z;
        }
        if (!(PROF && (p.dbg & 8))) {                // PROF ablation bit 3: no BGR stores
          gb[3 * q] = uint8_t(c); gb[3 * q + 1] = uint8_t(c >> 8); gb[3 * q + 2] = uint8_t(c >> 16);
        }
      }
    }
  }
  if (prof) {
    __syncthreads();
    stamp(3);
    if (tid == 0) {
      s_rec[4] = polls; s_rec[5] = naps; s_rec[6] = uint32_t(n_items);
      uint4* out = reinterpret_cast<uint4*>(reinterpret_cast<char*>(P.v[0].ws) + parts_off(p.n_px)) + 2 * bid;
      out[0] = make_uint4(s_rec[0], s_rec[1], s_rec[2], s_rec[3]);
      out[1] = make_uint4(s_rec[4], s_rec[5], s_rec[6], s_rec[7]);
    }
  }
}

// row_mode 2: append the row cloud (workspace scratch) behind the column cloud.
template <int XYZ64>
__global__ __launch_bounds__(kBlock) void row_tail_kernel(WsHeader* ws, const void* sx, const uint8_t* sb,
                                                          void* xyz, uint8_t* bgr, int64_t* count) {
  using XT = typename std::conditional<XYZ64 != 0, double, float>::type;
  const int64_t nc = ws->totals[0], nr = ws->totals[1];
  const int64_t aoff = ws->arena_cursor ? ws->arena_off : 0;     // resident-job arena (main3)
  const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i == 0) *count = nc + nr;
  if (i >= nr || aoff < 0) return;
  const XT* s = reinterpret_cast<const XT*>(sx);
  XT* d = reinterpret_cast<XT*>(xyz);
  const int64_t q = aoff + nc + i;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    d[q * 3 + c] = s[i * 3 + c];
    bgr[q * 3 + c] = sb[i * 3 + c];
  }
}

// slg_workspace_set_arena: the arena words of n slices' headers.
__global__ __launch_bounds__(64) void set_arena_kernel(char* ws, int64_t stride, int n, unsigned long long* cursor,
                                                       int64_t cap, int mult) {
  const int v = int(blockIdx.x) * 64 + int(threadIdx.x);
  if (v >= n) return;
  WsHeader* h = reinterpret_cast<WsHeader*>(ws + int64_t(v) * stride);
  h->arena_cursor = cursor;
  h->arena_cap = cap;
  h->arena_mult = mult;
  h->arena_off = 0;
}

__global__ __launch_bounds__(kBlock) void pinhole_kernel(const double* rays, int64_t n_px, int width, double fx,
                                                         double fy, double cx, double cy,
                                                         unsigned long long* mismatches) {
  const int64_t px = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  unsigned bad = 0;
  if (px < n_px) {
    const int v = int(px / width), u = int(px - int64_t(v) * width);
    const double x = (double(u) - cx) / fx;
    const double y = (double(v) - cy) / fy;
    const double n = sqrt((x * x + y * y) + 1.0);
    const double r[3] = {x / n, y / n, 1.0 / n};
#pragma unroll
    for (int c = 0; c < 3; ++c)
      bad += __double_as_longlong(r[c]) != __double_as_longlong(rays[c * n_px + px]);
  }
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(mismatches, (unsigned long long)bad);
}

// ------------------------------------------------------------------ host side
thread_local char g_err[512] = "";         // slg_last_error(); written by slg_internal_fail alone

int ceil_log2(int n) {
  int b = 0;
  while ((1ll << b) < (long long)n) ++b;
  return b;
}

// Which frames each axis reads and how the code is shifted (processing.py:80-122,
// sl_system.py:546-585).
int make_plan(const slg_capture* cap, const slg_decode_params* dp, Plan* out) {   // out may be NULL
  Plan tmp;
  Plan* pl = out ? out : &tmp;
  if (const int rc = check_enough_frames(cap)) return rc;
  if (dp->proj_cols < 1 || dp->proj_rows < 1) return fail(SLG_ERR_INVALID, "projector size must be positive");
  const int Bc = ceil_log2(dp->proj_cols), Br = ceil_log2(dp->proj_rows);
  if (Bc > kMaxBits || Br > kMaxBits)
    return fail(SLG_ERR_UNSUPPORTED, "at most %d code bits per axis (got %d, %d)", kMaxBits, Bc, Br);
  const int n = cap->n_frames;
  if (dp->variant == SLG_VARIANT_PROCESSING) {
    const int nc = dp->n_sets_col < 1 ? 1 : (dp->n_sets_col > Bc ? Bc : dp->n_sets_col);
    const int nr = dp->n_sets_row < 1 ? 1 : (dp->n_sets_row > Br ? Br : dp->n_sets_row);
    int kc = 0, kr = 0;
    for (int b = 0; b < nc; ++b) kc += (2 + 2 * b + 1 < n);          // processing.py:94
    for (int b = 0; b < nr; ++b) kr += (2 + 2 * Bc + 2 * b + 1 < n);
    *pl = {2, kc, nc - kc, Bc - nc, 2 + 2 * Bc, kr, nr - kr, Br - nr};
  } else if (dp->variant == SLG_VARIANT_SLSYSTEM) {
    int idx = 2, kc = 0, kr = 0;
    for (int b = 0; b < Bc; ++b) {                                  // sl_system.py:557-562
      if (idx >= n) break;
      if (idx + 1 >= n) return fail(SLG_ERR_INDEX, "list index out of range");
      idx += 2; ++kc;
    }
    const int row_first = idx;
    for (int b = 0; b < Br; ++b) {
      if (idx >= n) break;
      if (idx + 1 >= n) return fail(SLG_ERR_INDEX, "list index out of range");
      idx += 2; ++kr;
    }
    *pl = {2, kc, Bc - kc, 0, row_first, kr, Br - kr, 0};
  } else {
    return fail(SLG_ERR_INVALID, "unknown variant %d", dp->variant);
  }
  return SLG_OK;
}

int fill_calib(MainParams& mp, const slg_calib* c, const slg_tri_params* tp, int64_t n_px, int width) {
  if (!c || !tp) return fail(SLG_ERR_INVALID, "calib/tri params NULL");
  if (tp->row_mode < 0 || tp->row_mode > 2) return fail(SLG_ERR_INVALID, "row_mode must be 0, 1 or 2");
  if (c->ray_mode == SLG_RAYS_TABLE && !c->rays) return fail(SLG_ERR_INVALID, "ray table is NULL");
  if (c->ray_mode != SLG_RAYS_TABLE && c->ray_mode != SLG_RAYS_PINHOLE) return fail(SLG_ERR_INVALID, "bad ray_mode");
  if (!c->col_planes || c->n_col_planes < 1) return fail(SLG_ERR_INVALID, "column planes missing");
  if (tp->row_mode != 0 && (!c->row_planes || c->n_row_planes < 1)) return fail(SLG_ERR_INVALID, "row planes missing");
  if ((reinterpret_cast<uintptr_t>(c->col_planes) | reinterpret_cast<uintptr_t>(c->row_planes)) & 15)
    return fail(SLG_ERR_INVALID, "plane tables must be 16-byte aligned");
  mp.rays = c->rays;
  mp.fx = c->fx; mp.fy = c->fy; mp.cx = c->cx; mp.cy = c->cy;
  auto vetted = [](double b) {                     // b and RN(1/b) normal, far from over/underflow
    const double m = fabs(b);
    return std::isfinite(b) && m > 0x1p-900 && m < 0x1p900;
  };
  mp.rfx = 1.0 / c->fx;
  mp.rfy = 1.0 / c->fy;
  mp.div_fast = vetted(c->fx) && vetted(c->fy) ? 1 : 0;
  // rays_fast: tri_item's Markstein conditions hold for every column and row of the image
  // (x = (u-cx)/fx and y = (v-cy)/fy in range, so n = |(x, y, 1)| < 2^450 as well).
  auto ok_num = [](double a) { const double m = fabs(a); return m == 0.0 || (m > 0x1p-900 && m < 0x1p900); };
  bool fast = c->ray_mode == SLG_RAYS_TABLE || mp.div_fast;
  const int64_t height = width > 0 ? n_px / width : 0;
  for (int64_t u = 0; fast && c->ray_mode == SLG_RAYS_PINHOLE && u < width; ++u) {
    const double ax = double(u) - c->cx, x = ax / c->fx;
    fast = ok_num(ax) && ok_num(x) && fabs(x) < 0x1p449;
  }
  for (int64_t v = 0; fast && c->ray_mode == SLG_RAYS_PINHOLE && v < height; ++v) {
    const double ay = double(v) - c->cy, y = ay / c->fy;
    fast = ok_num(ay) && ok_num(y) && fabs(y) < 0x1p449;
  }
  mp.rays_fast = fast ? 1 : 0;
  mp.o0 = c->oc[0]; mp.o1 = c->oc[1]; mp.o2 = c->oc[2];
  mp.pcol = c->col_planes; mp.n_pcol = c->n_col_planes;
  mp.prow = c->row_planes; mp.n_prow = c->n_row_planes;
  // optional per-plane numerators (slg_calib, ABI 2)
  mp.num_pre = c->col_planes_num && (tp->row_mode != 2 || c->row_planes_num) ? 1 : 0;
  if (mp.num_pre) {
    mp.pcol = c->col_planes_num;
    if (tp->row_mode == 2) mp.prow = c->row_planes_num;
  }
  if ((reinterpret_cast<uintptr_t>(c->col_planes_num) | reinterpret_cast<uintptr_t>(c->row_planes_num)) & 15)
    return fail(SLG_ERR_INVALID, "numerator plane tables must be 16-byte aligned");
  mp.tol = tp->epipolar_tol;
  mp.n_px = n_px;
  mp.width = width;
  return SLG_OK;
}

// Output + workspace pointers of one view.
int fill_view(ViewIO& io, const slg_cloud* out, const slg_tri_params* tp, int64_t n_px, void* ws) {
  if (!out || !out->xyz || !out->bgr || !out->count) return fail(SLG_ERR_INVALID, "output cloud buffers NULL");
  const int64_t need = tp->row_mode == 2 ? 2 * n_px : n_px;
  if (out->capacity < need) return fail(SLG_ERR_INVALID, "cloud capacity %lld < %lld", (long long)out->capacity, (long long)need);
  io.xyz = out->xyz;
  io.bgr = out->bgr;
  io.count = out->count;
  io.ws = reinterpret_cast<WsHeader*>(ws);
  io.states = reinterpret_cast<uint64_t*>(static_cast<char*>(ws) + states_off(n_px));
  io.scratch_xyz = static_cast<char*>(ws) + scratch_xyz_off(n_px);
  io.scratch_bgr = reinterpret_cast<uint8_t*>(static_cast<char*>(ws) + scratch_bgr_off(n_px));
  return SLG_OK;
}

int debug_flags() {   // profiling ablations only; unset in production
  const char* e = getenv("SLG_DBG");
  return e ? atoi(e) : 0;
}

constexpr int kMainDbgBits = 1 | 2 | 4 | 8 | 64 | 128 | 512;   // 512: the instance alone   // bits main3's profiling instance reads

uint32_t help_after() {   // look-back helper delay; SLG_HELP_AFTER=0 forces the helper (tests)
  const char* e = getenv("SLG_HELP_AFTER");
  return e ? uint32_t(atoi(e)) : kHelpAfter;
}

using Main3Fn = void (*)(Main3Params);

// Production instances for every (source, row_mode, xyz, ray) case; the profiling instance
// (SLG_DBG with any main3 bit) exists for the benchmark shape only: row_mode 1, f32 XYZ, frames,
// pinhole rays (tools/kbench.py).
// Decode plans main3 has specialised instances for (PLAN = (col_pairs << 4) | row_pairs), with
// row_mode 1 and pinhole rays: C2's 11 + 10 bits (1920x1080 projector, row_scale 2), the
// reference's default 11 + 11 (processing.py:29-30; C3, C5) and C4's 12 + 12; row_mode 0: C1's
// 10 column bits.
#define SLG_PLAN_C2 0xBA
#define SLG_PLAN_1080P 0xBB
#define SLG_PLAN_C4 0xCC
#define SLG_PLAN_C1 0xA0           // row_mode 0, 10 column bits (1024-wide projector), no row pairs

// Every main3 instance the library can launch, one table: pick_main only returns pointers from
// it, and only those whose device code is in the library's gfx950 code object
// (device_symbols): the HIP runtime aborts the process on a launch -- or any query -- of a kernel
// whose code object lacks it (a round-5 run ended that way: DESIGN.md §4), so a missing
// instance must be caught before the runtime sees it.
struct Main3Inst {
  int src, row_mode, x64, rays, plan;
  bool prof;
  Main3Fn fn;
};
#define SLG_M3(S, RM, X, R, P, PL) {S, RM, X, R, PL, P, main3_kernel<RM, X, S, R, P, PL>},
#define SLG_M3_GENERIC(S)                                                                          \
  SLG_M3(S, 0, 0, 0, false, 0) SLG_M3(S, 0, 0, 1, false, 0) SLG_M3(S, 0, 1, 0, false, 0)          \
  SLG_M3(S, 0, 1, 1, false, 0) SLG_M3(S, 1, 0, 0, false, 0) SLG_M3(S, 1, 0, 1, false, 0)          \
  SLG_M3(S, 1, 1, 0, false, 0) SLG_M3(S, 1, 1, 1, false, 0) SLG_M3(S, 2, 0, 0, false, 0)          \
  SLG_M3(S, 2, 0, 1, false, 0) SLG_M3(S, 2, 1, 0, false, 0) SLG_M3(S, 2, 1, 1, false, 0)
#define SLG_M3_PLAN(RM, PL) SLG_M3(1, RM, 0, 1, false, PL) SLG_M3(1, RM, 1, 1, false, PL)         \
  SLG_M3(1, RM, 0, 1, false, (PL) | kPlanGray) SLG_M3(1, RM, 1, 1, false, (PL) | kPlanGray)
const Main3Inst kMain3Table[] = {
#ifdef SLG_FAST_BUILD   // register/spill inspection builds only: the benchmark's instances alone
    SLG_M3(1, 1, 0, 1, false, SLG_PLAN_C2) SLG_M3(1, 1, 0, 1, false, 0)
#else
    SLG_M3_GENERIC(0) SLG_M3_GENERIC(1)
    SLG_M3_PLAN(1, SLG_PLAN_C2) SLG_M3_PLAN(1, SLG_PLAN_1080P) SLG_M3_PLAN(1, SLG_PLAN_C4)
    SLG_M3_PLAN(0, SLG_PLAN_C1)
    SLG_M3(1, 1, 0, 1, true, SLG_PLAN_C2) SLG_M3(1, 1, 0, 1, true, 0)
#endif
};
#undef SLG_M3_PLAN
#undef SLG_M3_GENERIC
#undef SLG_M3

// Itanium name of main3_kernel<RM, X, S, R, P, PL> (anonymous namespace), as the code object and
// the runtime's registration spell it.
std::string main3_symbol(const Main3Inst& k) {
  auto li = [](int v) { return "Li" + (v < 0 ? "n" + std::to_string(-v) : std::to_string(v)) + "E"; };
  return "_ZN12_GLOBAL__N_112main3_kernelI" + li(k.row_mode) + li(k.x64) + li(k.src) + li(k.rays) +
         std::string(k.prof ? "Lb1E" : "Lb0E") + li(k.plan) + "EEvNS_11Main3ParamsE";
}

// Symbol names of this library's gfx950 code objects, read once from its own file (found by
// dladdr; code_object.cpp).  File reads only -- no HIP call, so nothing here can trip the
// runtime's abort.  Empty when the file cannot be read.
const std::vector<std::string>& device_symbols() {
  static std::vector<std::string> names;
  static std::once_flag once;
  std::call_once(once, [] {
    Dl_info info{};
    if (dladdr(reinterpret_cast<void*>(&slg_version), &info) && info.dli_fname)
      names = slg_code_object_symbols(info.dli_fname);
  });
  return names;
}

bool device_has(const std::string& name) {
  const auto& v = device_symbols();
  return std::binary_search(v.begin(), v.end(), name);
}

// The instance the calling thread's last pick_main returned (slg_last_kernel; NULL: none).
thread_local const Main3Inst* g_last_main = nullptr;

// The kernel of a (source, row_mode, xyz, rays, plan) launch: the plan's specialised instance
// if the table has one, else the generic one; the profiling instance when SLG_DBG asks for it.
// NULL (and *why set) when the table has none or its device code is missing.
Main3Fn pick_main(int src, int row_mode, int x64, int rays, int plan, const char** why) {
  g_last_main = nullptr;
  const bool prof = (debug_flags() & kMainDbgBits) != 0;
  const Main3Inst* hit = nullptr;
  for (int pass = 0; pass < 2 && !hit; ++pass) {
    const int want = pass == 0 ? plan : 0;
    if (pass == 1 && plan == 0) break;
    for (const Main3Inst& k : kMain3Table)
      if (k.src == src && k.row_mode == row_mode && k.x64 == x64 && k.rays == rays && k.plan == want && k.prof == prof) {
        hit = &k;
        break;
      }
  }
  if (!hit) {
    *why = prof ? "no kernel for this configuration (SLG_DBG profiling: row_mode 1, f32, frames, pinhole only)"
                : "no kernel for this configuration";
    return nullptr;
  }
  if (!device_has(main3_symbol(*hit))) {
    *why = "the library's code object lacks this kernel instance (rebuild libslgpu.so)";
    return nullptr;
  }
  g_last_main = hit;
  return hit->fn;
}

// One main3 launch over mp.n_views views (<= kMaxViews), then the row_mode-2 tails.
int launch_main3(Main3Fn fn, const char* why, Main3Params& mp, const slg_tri_params* tp, const slg_cloud* outs,
                 hipStream_t s) {
  if (!fn) return fail(SLG_ERR_UNSUPPORTED, "%s", why ? why : "no kernel for this configuration");
  mp.c.dbg = debug_flags();
  mp.c.help_after = help_after();
  const int64_t grid = int64_t(mp.n_fin) * mp.fin_blocks + mp.c.n_tiles * mp.n_views;
  if (grid > INT_MAX) return fail(SLG_ERR_UNSUPPORTED, "batch too large for one launch");
  hipLaunchKernelGGL(fn, dim3(unsigned(grid)), dim3(kTileBlock), 0, s, mp);
  int rc = check_launch("main kernel");
  if (rc || !tp || tp->row_mode != 2) return rc;
  const unsigned tg = unsigned((mp.c.n_px + kBlock - 1) / kBlock);
  for (int v = 0; v < mp.n_views; ++v) {
    const ViewIO& io = mp.v[v];
    if (tp->xyz_f64)
      hipLaunchKernelGGL(row_tail_kernel<1>, dim3(tg), dim3(kBlock), 0, s, io.ws, io.scratch_xyz, io.scratch_bgr, outs[v].xyz, outs[v].bgr, outs[v].count);
    else
      hipLaunchKernelGGL(row_tail_kernel<0>, dim3(tg), dim3(kBlock), 0, s, io.ws, io.scratch_xyz, io.scratch_bgr, outs[v].xyz, outs[v].bgr, outs[v].count);
    rc = check_launch("row_tail_kernel");
    if (rc) return rc;
  }
  return SLG_OK;
}

// Views of one batch must share the launch-wide parameters.
int check_batch(const slg_capture* caps, int n_views) {
  for (int v = 0; v < n_views; ++v) {
    const int rc = check_capture(&caps[v]);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(caps[v].texture) & 7) return fail(SLG_ERR_INVALID, "texture must be 8-byte aligned");
    if (const int rg = check_same_geometry(caps[v], caps[0], kBatchGeometry)) return rg;
  }
  return SLG_OK;
}

// Fused decode + triangulate of n_views views (thresholds already in each view's workspace
// slice): one main3 launch per kMaxViews views.  timing_events: 2 per launch, or NULL.
int fused_batch(const slg_capture* caps, int n_views, const slg_decode_params* dp, const slg_calib* calib,
                const slg_tri_params* tp, char* ws, int64_t ws_stride, const slg_cloud* outs,
                void* const* timing_events, hipStream_t s, const slg_capture* next = nullptr, int n_next = 0,
                char* fin_ws = nullptr, int n_fin = 0) {
  if (!caps || n_views < 1 || !dp || !ws || !outs) return fail(SLG_ERR_INVALID, "NULL argument");
  int rc = check_batch(caps, n_views);
  if (rc) return rc;
  if (n_fin) {                                      // finish thresholds carried by an earlier launch
    if (!fin_ws || n_fin < 0 || n_fin > kMaxViews) return fail(SLG_ERR_INVALID, "finish: NULL or more than 16 views");
    if (dp->thresh_mode != SLG_THRESH_OTSU) return fail(SLG_ERR_UNSUPPORTED, "carried histograms need thresh_mode OTSU");
  }
  if (n_next) {                                     // the batch after next rides along (Otsu only)
    if (!next || n_next < 0 || n_next > n_views) return fail(SLG_ERR_INVALID, "next batch: NULL or more views than this batch");
    if (dp->thresh_mode != SLG_THRESH_OTSU) return fail(SLG_ERR_UNSUPPORTED, "next-batch histograms need thresh_mode OTSU");
    if (debug_flags() & 64)   // the phase records would land on the carried partials
      return fail(SLG_ERR_UNSUPPORTED, "SLG_DBG phase records cannot run with a carried batch");
    for (int v = 0; v < n_next; ++v) {
      rc = check_capture(&next[v]);
      if (!rc) rc = check_enough_frames(&next[v]);
      if (rc) return rc;
      if ((rc = check_same_geometry(next[v], caps[0], "next batch must share this batch's geometry"))) return rc;
    }
  }
  std::vector<Plan> plans(static_cast<size_t>(n_views));   // one make_plan per view: it validates too
  for (int v = 0; v < n_views; ++v) {
    rc = make_plan(&caps[v], dp, &plans[size_t(v)]);
    if (rc) return rc;
  }
  const int64_t n_px = int64_t(caps[0].height) * caps[0].width;
  // every slice of this launch (its views, the carried next batch, the finished batch) is
  // ws_stride apart; the finished batch's slices are read with THIS batch's geometry and
  // decode parameters (include/slgpu.h, slg_decode_triangulate_batch_carry)
  rc = check_ws_stride(n_views > 1 || n_next > 1 || n_fin > 1, ws_stride, n_px);
  if (rc) return rc;
  Main3Params mp{};
  rc = fill_calib(mp.c, calib, tp, n_px, caps[0].width);
  if (rc) return rc;
  mp.c.n_tiles = n_tiles_of(n_px);
  for (int v0 = 0, launch = 0; v0 < n_views; v0 += kMaxViews, ++launch) {
    mp.n_views = n_views - v0 < kMaxViews ? n_views - v0 : kMaxViews;
    int plan = -1;                                  // the views' common pair counts, else 0
    bool all_gray = true, any_gray = false;         // gray captures (texture NULL)
    for (int k = 0; k < mp.n_views; ++k) {
      const Plan& pl = plans[size_t(v0 + k)];
      const int rp = tp->row_mode == 0 ? 0 : pl.row_pairs;     // row_mode 0 reads no row frame
      const int key = pl.col_pairs <= 15 && rp <= 15 ? (pl.col_pairs << 4) | rp : 0;
      plan = plan < 0 || plan == key ? key : 0;
      all_gray = all_gray && !caps[v0 + k].texture;
      any_gray = any_gray || !caps[v0 + k].texture;
    }
    // a mixed launch runs the generic instance (per-view test); a plan instance is all one kind
    if (plan > 0 && any_gray) plan = all_gray ? (plan | kPlanGray) : 0;
    const char* why = nullptr;
    const Main3Fn fn = pick_main(1, tp->row_mode, tp->xyz_f64 ? 1 : 0, calib->ray_mode, plan < 0 ? 0 : plan, &why);
    for (int k = 0; k < mp.n_views; ++k) {
      const int v = v0 + k;
      ViewIO& io = mp.v[k];
      io = ViewIO{};
      rc = fill_view(io, &outs[v], tp, n_px, ws + int64_t(v) * ws_stride);
      if (rc) return rc;
      io.frames = caps[v].frames;
      io.texture = caps[v].texture;
      io.stride = caps[v].frame_stride;
      io.plan = plans[size_t(v)];
      if (v < n_next) {
        io.hn_white = next[v].frames;
        io.hn_black = next[v].frames + next[v].frame_stride;
        io.hn_part = reinterpret_cast<uint32_t*>(ws + int64_t(v) * ws_stride + parts_off(n_px));
      }
    }
    mp.n_fin = launch == 0 ? n_fin : 0;             // the first launch finishes them all
    if (mp.n_fin) {
      const int64_t nb = (mp.c.n_tiles + 127) / 128;   // ~128 partials (128 KB) per workgroup
      mp.fin_blocks = int(nb < 1 ? 1 : (nb > kPartsBlocksMax ? kPartsBlocksMax : nb));
      mp.n_state_words = n_state_words(n_px);
      mp.pad_zero = mp.c.n_tiles * kTilePx - n_px;
      for (int k = 0; k < n_fin; ++k) {
        char* slice = fin_ws + int64_t(k) * ws_stride;
        mp.fin[k].parts = reinterpret_cast<const uint32_t*>(slice + parts_off(n_px));
        mp.fin[k].ws = reinterpret_cast<WsHeader*>(slice);
      }
    }
    if (timing_events && timing_events[2 * launch]) (void)hipEventRecord(static_cast<hipEvent_t>(timing_events[2 * launch]), s);
    rc = launch_main3(fn, why, mp, tp, &outs[v0], s);
    if (rc) return rc;
    if (timing_events && timing_events[2 * launch + 1]) (void)hipEventRecord(static_cast<hipEvent_t>(timing_events[2 * launch + 1]), s);
  }
  return SLG_OK;
}

}  // namespace

// The library's one error entry (internal.h).
int slg_internal_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// ==================================================================== C ABI
extern "C" {

int32_t slg_version(void) { return SLG_ABI_VERSION; }

#ifndef SLG_BUILD_ID
#define SLG_BUILD_ID "unknown"
#endif
const char* slg_build_id(void) { return SLG_BUILD_ID; }

int32_t slg_kernel_table(char* buf, int64_t cap) {
  if (!buf || cap < 1) return -fail(SLG_ERR_INVALID, "buf NULL or cap < 1");
  int64_t at = 0;
  int32_t missing = 0;
  buf[0] = 0;
  for (const Main3Inst& k : kMain3Table) {
    const std::string name = main3_symbol(k);
    const bool has = device_has(name);
    missing += has ? 0 : 1;
    const std::string line = name + (has ? "\t1\n" : "\t0\n");
    if (at + int64_t(line.size()) < cap) {
      memcpy(buf + at, line.data(), line.size());
      at += int64_t(line.size());
      buf[at] = 0;
    }
  }
  return missing;
}

int32_t slg_last_kernel(char* buf, int64_t cap) {
  if (!buf || cap < 1) return fail(SLG_ERR_INVALID, "buf NULL or cap < 1");
  buf[0] = 0;
  if (!g_last_main) return 0;
  const std::string name = main3_symbol(*g_last_main);
  if (int64_t(name.size()) >= cap) return fail(SLG_ERR_INVALID, "buf too small for the symbol");
  memcpy(buf, name.c_str(), name.size() + 1);
  return 0;
}

const char* slg_last_error(void) { return g_err; }

int64_t slg_workspace_bytes(int64_t n_pixels) { return n_pixels > 0 ? ws_total(n_pixels) : kHeaderBytes; }

int32_t slg_workspace_init(void* workspace, int64_t workspace_bytes, void* stream) {
  if (!workspace) return fail(SLG_ERR_INVALID, "workspace NULL");
  const int64_t n = workspace_bytes < kHeaderBytes ? workspace_bytes : kHeaderBytes;
  if (hipMemsetAsync(workspace, 0, size_t(n), static_cast<hipStream_t>(stream)) != hipSuccess)
    return fail(SLG_ERR_HIP, "hipMemsetAsync failed");
  return SLG_OK;
}

int32_t slg_decode(const slg_capture* cap, const slg_decode_params* dp, void* workspace, int32_t* col_out,
                   int32_t* row_out, uint8_t* mask_out, void* stream) {
  int rc = check_capture(cap);
  if (rc) return rc;
  if (!dp || !workspace || !col_out || !row_out || !mask_out) return fail(SLG_ERR_INVALID, "NULL argument");
  if ((reinterpret_cast<uintptr_t>(col_out) | reinterpret_cast<uintptr_t>(row_out)) & 15 ||
      reinterpret_cast<uintptr_t>(mask_out) & 7)
    return fail(SLG_ERR_INVALID, "map outputs must be 16-byte (col,row) / 8-byte (mask) aligned");
  MainParams mp{};
  rc = make_plan(cap, dp, &mp.plan);
  if (rc) return rc;
  const int64_t n_px = int64_t(cap->height) * cap->width;
  mp.frames = cap->frames;
  mp.stride = cap->frame_stride;
  mp.n_px = n_px;
  mp.width = cap->width;
  mp.out_col = col_out; mp.out_row = row_out; mp.out_mask = mask_out;
  mp.ws = reinterpret_cast<WsHeader*>(workspace);
  mp.n_tiles = n_tiles_of(n_px);
  hipLaunchKernelGGL(decode_maps_kernel, dim3(unsigned((n_px + kMapsPx - 1) / kMapsPx)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), mp);
  return check_launch("decode_maps_kernel");
}

int32_t slg_triangulate(const slg_maps* maps, const slg_calib* calib, const slg_tri_params* tp, void* workspace,
                        const slg_cloud* out, void* stream) {
  if (!maps || !maps->col || !maps->mask || !maps->texture || !workspace) return fail(SLG_ERR_INVALID, "NULL argument");
  if (maps->height < 1 || maps->width < 1) return fail(SLG_ERR_INVALID, "bad map size");
  if (tp && tp->row_mode != 0 && !maps->row) return fail(SLG_ERR_INVALID, "row map required for row_mode 1/2");
  if ((reinterpret_cast<uintptr_t>(maps->col) | reinterpret_cast<uintptr_t>(maps->row)) & 15 ||
      (reinterpret_cast<uintptr_t>(maps->mask) | reinterpret_cast<uintptr_t>(maps->texture)) & 7)
    return fail(SLG_ERR_INVALID, "maps must be 16-byte (col,row) / 8-byte (mask,texture) aligned");
  const int64_t n_px = int64_t(maps->height) * maps->width;
  Main3Params m3{};
  int rc = fill_calib(m3.c, calib, tp, n_px, maps->width);
  if (rc) return rc;
  rc = fill_view(m3.v[0], out, tp, n_px, workspace);
  if (rc) return rc;
  m3.c.n_tiles = n_tiles_of(n_px);
  m3.n_views = 1;
  hipStream_t s = static_cast<hipStream_t>(stream);
  rc = slg_stats_arm(n_px, workspace, s);
  if (rc) return rc;
  m3.v[0].in_col = maps->col; m3.v[0].in_row = maps->row; m3.v[0].in_mask = maps->mask;
  m3.v[0].texture = maps->texture;
  const char* why = nullptr;
  const Main3Fn fn = pick_main(0, tp->row_mode, tp->xyz_f64 ? 1 : 0, calib->ray_mode, 0, &why);
  return launch_main3(fn, why, m3, tp, out, s);
}

static int reconstruct_impl(const slg_capture* cap, const slg_decode_params* dp, const slg_calib* calib,
                            const slg_tri_params* tp, void* workspace, const slg_cloud* out, void* stream,
                            bool with_stats) {
  if (!cap || !dp || !workspace) return fail(SLG_ERR_INVALID, "NULL argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (with_stats) {
    int rc = check_batch(cap, 1);
    if (!rc) rc = make_plan(cap, dp, nullptr);
    if (!rc) rc = slg_stats_batch(cap, 1, dp, static_cast<char*>(workspace), 0, s);
    if (rc) return rc;
  }
  return fused_batch(cap, 1, dp, calib, tp, static_cast<char*>(workspace), 0, out, nullptr, s);
}

int32_t slg_reconstruct(const slg_capture* cap, const slg_decode_params* dp, const slg_calib* calib,
                        const slg_tri_params* tp, void* workspace, const slg_cloud* out, void* stream) {
  return reconstruct_impl(cap, dp, calib, tp, workspace, out, stream, true);
}

int32_t slg_decode_triangulate(const slg_capture* cap, const slg_decode_params* dp, const slg_calib* calib,
                               const slg_tri_params* tp, void* workspace, const slg_cloud* out, void* stream) {
  return reconstruct_impl(cap, dp, calib, tp, workspace, out, stream, false);
}

int32_t slg_reconstruct_batch(const slg_capture* caps, int32_t n_views, const slg_decode_params* dp,
                              const slg_calib* calib, const slg_tri_params* tp, void* workspace,
                              int64_t ws_stride, const slg_cloud* outs, void* const* timing_events,
                              void* stream) {
  if (!caps || n_views < 1 || !dp || !workspace || !outs) return fail(SLG_ERR_INVALID, "NULL argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  int rc = check_batch(caps, n_views);              // validate everything before enqueueing
  for (int v = 0; v < n_views && !rc; ++v) rc = make_plan(&caps[v], dp, nullptr);
  if (rc) return rc;
  for (int v0 = 0, launch = 0; v0 < n_views; v0 += kMaxViews, ++launch) {
    const int nb = n_views - v0 < kMaxViews ? n_views - v0 : kMaxViews;
    rc = slg_stats_batch(caps + v0, nb, dp, ws + int64_t(v0) * ws_stride, ws_stride, s);
    if (rc) return rc;
    rc = fused_batch(caps + v0, nb, dp, calib, tp, ws + int64_t(v0) * ws_stride, ws_stride, outs + v0,
                     timing_events ? timing_events + 2 * launch : nullptr, s);
    if (rc) return rc;
  }
  return SLG_OK;
}

int32_t slg_decode_triangulate_batch(const slg_capture* caps, int32_t n_views, const slg_decode_params* dp,
                                     const slg_calib* calib, const slg_tri_params* tp, void* workspace,
                                     int64_t ws_stride, const slg_cloud* outs, void* const* timing_events,
                                     void* stream) {
  return fused_batch(caps, n_views, dp, calib, tp, static_cast<char*>(workspace), ws_stride, outs, timing_events,
                     static_cast<hipStream_t>(stream));
}

int32_t slg_decode_triangulate_batch_next(const slg_capture* caps, int32_t n_views, const slg_decode_params* dp,
                                          const slg_calib* calib, const slg_tri_params* tp, void* workspace,
                                          int64_t ws_stride, const slg_cloud* outs, const slg_capture* next,
                                          int32_t n_next, void* const* timing_events, void* stream) {
  return fused_batch(caps, n_views, dp, calib, tp, static_cast<char*>(workspace), ws_stride, outs, timing_events,
                     static_cast<hipStream_t>(stream), next, next ? n_next : 0);
}

int32_t slg_decode_triangulate_batch_carry(const slg_capture* caps, int32_t n_views, const slg_decode_params* dp,
                                           const slg_calib* calib, const slg_tri_params* tp, void* workspace,
                                           int64_t ws_stride, const slg_cloud* outs, const slg_capture* next,
                                           int32_t n_next, void* fin_workspace, int32_t n_fin,
                                           void* const* timing_events, void* stream) {
  return fused_batch(caps, n_views, dp, calib, tp, static_cast<char*>(workspace), ws_stride, outs, timing_events,
                     static_cast<hipStream_t>(stream), next, next ? n_next : 0, static_cast<char*>(fin_workspace),
                     fin_workspace ? n_fin : 0);
}

int32_t slg_workspace_set_arena(void* workspace, int64_t ws_stride, int32_t n_slices, int64_t* cursor,
                                int64_t capacity_points, int32_t points_per_valid, void* stream) {
  if (!workspace || n_slices < 1 || (n_slices > 1 && (ws_stride < kHeaderBytes || (ws_stride & 255))))
    return fail(SLG_ERR_INVALID, "bad workspace / stride");
  if (cursor && (capacity_points < 0 || (points_per_valid != 1 && points_per_valid != 2)))
    return fail(SLG_ERR_INVALID, "arena capacity < 0 or points_per_valid not 1 / 2");
  if (reinterpret_cast<uintptr_t>(cursor) & 7) return fail(SLG_ERR_INVALID, "cursor must be 8-byte aligned");
  hipLaunchKernelGGL(set_arena_kernel, dim3(unsigned((n_slices + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream),
                     static_cast<char*>(workspace), ws_stride, int(n_slices),
                     reinterpret_cast<unsigned long long*>(cursor), cursor ? capacity_points : 0,
                     cursor ? points_per_valid : 0);
  return check_launch("set_arena_kernel");
}

int32_t slg_rays_match_pinhole(const double* rays, int32_t height, int32_t width, double fx, double fy, double cx,
                               double cy, int64_t* mismatches, void* stream) {
  if (!rays || !mismatches || height < 1 || width < 1) return fail(SLG_ERR_INVALID, "bad argument");
  const int64_t n_px = int64_t(height) * width;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(mismatches, 0, sizeof(int64_t), s) != hipSuccess) return fail(SLG_ERR_HIP, "hipMemsetAsync failed");
  hipLaunchKernelGGL(pinhole_kernel, dim3(unsigned((n_px + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, rays, n_px,
                     int(width), fx, fy, cx, cy, reinterpret_cast<unsigned long long*>(mismatches));
  return check_launch("pinhole_kernel");
}

}  // extern "C"
