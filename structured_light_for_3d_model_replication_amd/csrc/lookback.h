// lookback.h -- the decoupled look-back of main3_kernel's ordered compaction: the state words,
// the scalar walk, the lone view's scan, and the helper that computes a silent predecessor's
// aggregate.  Device only; every name is TU-local.
#pragma once
#include "triangulate.h"

namespace {

constexpr uint64_t kFlagAgg = 1ull << 62;
constexpr uint64_t kFlagInc = 2ull << 62;
constexpr uint64_t kValMask = (1ull << 62) - 1;

__device__ inline uint64_t ld_state(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void st_state(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Keep-count of another tile of the same view, computed by the calling wave alone: the
// aggregate a predecessor that has not published for a long time would publish (it may not
// have been dispatched yet).  Same arithmetic as main3's phases A/B => same value.
template <int ROW_MODE, int SRC_FRAMES, int RAYS>
__device__ int tile_keep_count_wave(const MainParams& p, int tile, int stream) {
  const int lane = threadIdx.x & 63;
  int cnt = 0;
  const int64_t tile_px = int64_t(tile) * kTilePx;
#pragma unroll 1
  for (int i = lane; i < kTilePx; i += 64) {
    const int64_t px = tile_px + i;
    int col, row;
    if (px < p.n_px && decode_px<ROW_MODE, SRC_FRAMES>(p, px, col, row)) {
      const int v = int(px / p.width), u = int(px - int64_t(v) * p.width);
      const TriOut o = tri_item<ROW_MODE, RAYS>(p, pack_code<ROW_MODE>(p, col, row), u, v);
      cnt += (o.keep >> stream) & 1u;
    }
  }
  return wave_sum(cnt);
}

__device__ inline void publish_agg(uint64_t* w, int agg) {   // unless a helper already did
  unsigned long long expect = 0;
  __hip_atomic_compare_exchange_strong(reinterpret_cast<unsigned long long*>(w), &expect,
                                       (unsigned long long)(kFlagAgg | uint64_t(agg)), __ATOMIC_RELAXED,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr unsigned kNapCap = 8;         // back-off cap: 8 x s_sleep(2) ~ 1k clocks between re-polls
constexpr unsigned kHelpAfter = 2048;   // s_sleep(2) units (~0.1 ms) before asking for help

// Look-back words st[b .. b+7] read by one scalar load that misses the scalar cache (glc): the
// poll goes to L2 without queueing behind the co-resident workgroup's frame stream in the
// CU's vector-memory pipeline (a vector poll waits behind up to ~180 KB of streaming loads).
__device__ inline void ld_state8_scalar(const uint64_t* p, uint64_t (&v)[8]) {
  typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
  u32x16 r;
  const uint64_t a = reinterpret_cast<uint64_t>(p);   // uniform: pinned to SGPRs for the "s" operand
  const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(a));          // (the builtin returns int:
  const uint32_t hi = __builtin_amdgcn_readfirstlane(uint32_t(a >> 32));    //  widen only as uint32)
  const uint64_t sa = (uint64_t(hi) << 32) | lo;
  asm volatile("s_load_dwordx16 %0, %1, 0x0 glc\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(sa) : "memory");
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = uint64_t(r[2 * k]) | (uint64_t(r[2 * k + 1]) << 32);
}

// Decoupled look-back over static tile ids (wave 0 calls it, lane 0 publishes).  Returns true
// with the exclusive prefix of `agg` over the view's tiles before `tile`, or false with the
// nearest predecessor that has not published for p.help_after (it may not be dispatched yet:
// dispatch order is not guaranteed): the caller then computes that tile's aggregate itself
// (tile_keep_count_wave) and retries, so waiting always ends.  Polled 8 predecessors at a time
// with wave-uniform scalar loads, newest first: aggregates are summed as they appear and the
// walk stops at the first inclusive prefix; an unpublished entry is re-polled after a capped
// back-off.  Published values never change (0 -> aggregate -> inclusive), so a stale read only
// delays the walk, never changes the sum.
template <bool PROF>
__device__ bool lookback_scalar(const MainParams& p, uint64_t* st, int tile, int agg, bool published,
                                uint64_t& excl_out, int& help_tile, uint32_t& polls, uint32_t& naps) {
  const int lane = threadIdx.x & 63;
  if (PROF && (p.dbg & 1)) { excl_out = uint64_t(tile) * kTilePx; return true; }   // ablation: no wait
  if (tile == 0) {
    if (lane == 0 && !published) st_state(&st[0], kFlagInc | uint64_t(agg));
    excl_out = 0;
    return true;
  }
  if (lane == 0 && !published) st_state(&st[tile], kFlagAgg | uint64_t(agg));
  uint64_t excl = 0;
  int j = tile - 1;                          // newest predecessor not summed yet
  unsigned slept = 0, nap = 1;
  for (;;) {
    ++polls;
    const int b = j >= 7 ? j - 7 : 0;
    uint64_t v[8];
    ld_state8_scalar(st + b, v);
    bool done = false, stall = false;
#pragma unroll
    for (int k = 7; k >= 0; --k) {
      if (done || stall || b + k > j) continue;
      const uint64_t f = v[k] >> 62;
      if (f == 0) { stall = true; continue; }
      excl += v[k] & kValMask;
      j = b + k - 1;
      done = f == 2;
    }
    if (done || j < 0) break;
    if (stall) {
      if (slept >= p.help_after) {
        help_tile = j;
        return false;
      }
      for (unsigned z = 0; z < nap; ++z) __builtin_amdgcn_s_sleep(2);
      slept += nap;
      naps += nap;
      nap = nap < kNapCap ? nap * 2 : kNapCap;
    }
  }
  if (lane == 0) st_state(&st[tile], kFlagInc | (excl + uint64_t(agg)));
  excl_out = excl;
  return true;
}

// Publishes this tile's aggregate (tile 0: its inclusive prefix) and takes a ticket.  The last of
// the view's tiles to do so finds every tile's word published: it scans them all, 8 consecutive
// tiles per lane (a segmented scan: an inclusive word restarts the running sum), publishes every
// tile's inclusive prefix, and returns true with its own exclusive prefix.  The others return
// false and walk back (lookback_scalar) as before; a walk that is still polling when the scan
// lands meets an inclusive prefix at its next poll.  A lone view's launch has every tile in
// flight at once, so without the scan its walks are ~6.7 polls of ~0.8 us each
// (profiles/r7w).  The values written are the ones the walks compute, so a word only ever
// goes 0 -> aggregate -> inclusive prefix, whichever writer gets there first.
constexpr int kScanPer = 8;                // lookback_scan: consecutive tiles per lane
constexpr int kScanTiles = 2 * 64 * kScanPer;   // lone views up to 1024 tiles (4.2 MP) take the scan
template <bool PROF>
__device__ bool lookback_scan(const MainParams& p, uint64_t* st, int tile, int tiles, int agg, uint32_t* ticket,
                              uint64_t& excl_out) {
  const int lane = threadIdx.x & 63;
  if (PROF && (p.dbg & 1)) return false;     // ablation (lookback_scalar): no wait
  // (no release / acquire fences: on gfx950 an agent-scope one writes back or invalidates the
  // L2 -- the bench shape took 716 instead of 313 us per step with them.  The words and the
  // ticket are agent-scope atomics, performed at the L2 that owns the address, and the ticket is
  // taken after vmcnt(0): the hardware assumption of stats_kernel's ticket)
  uint32_t t = 0;
  if (lane == 0) {
    st_state(&st[tile], (tile == 0 ? kFlagInc : kFlagAgg) | uint64_t(agg));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  t = __builtin_amdgcn_readfirstlane(t);
  if (t != uint32_t(tiles - 1)) return false;
  // kScanPer consecutive tiles per lane: their words loaded at once, summed in the lane, then one
  // wave-wide segmented scan of the lane totals; blocks of 64 * kScanPer tiles in order
  uint64_t carry = 0, mine = 0;
  for (int c0 = 0; c0 < tiles; c0 += 64 * kScanPer) {
    const int i0 = c0 + kScanPer * lane;
    uint64_t w[kScanPer];
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) w[k] = i0 + k < tiles ? ld_state(&st[i0 + k]) : 0;
    uint64_t x = 0;                          // the lane's running segmented sum
    bool f = false;                          // an inclusive word seen in the lane so far
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
      const bool inc = (w[k] >> 62) == 2;
      x = inc ? (w[k] & kValMask) : x + (w[k] & kValMask);
      f = f || inc;
    }
    uint64_t sx = x;                         // inclusive segmented scan of the lane totals
    bool sf = f;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t xo = __shfl_up(sx, o);
      const bool fo = __shfl_up(int(sf), o) != 0;
      if (lane >= o && !sf) { sx += xo; sf = fo; }
    }
    uint64_t ex = __shfl_up(sx, 1);          // the lanes before this one (+ carry unless they hold
    const bool ef = lane > 0 && __shfl_up(int(sf), 1) != 0;   //  an inclusive word)
    ex = (lane == 0 ? 0 : ex) + (ef ? 0 : carry);
    x = ex;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
      const bool inc = (w[k] >> 62) == 2;
      x = inc ? (w[k] & kValMask) : x + (w[k] & kValMask);
      if (i0 + k < tiles && !inc) st_state(&st[i0 + k], kFlagInc | x);
      if (i0 + k == tile) mine = x;
    }
    carry = __shfl(x, 63);
  }
  mine = __builtin_amdgcn_readlane(uint32_t(mine), (tile % (64 * kScanPer)) / kScanPer) |
         (uint64_t(__builtin_amdgcn_readlane(uint32_t(mine >> 32), (tile % (64 * kScanPer)) / kScanPer)) << 32);
  excl_out = mine - uint64_t(agg);
  return true;
}

}  // namespace
