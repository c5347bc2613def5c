// carried_hist.h -- the Otsu histograms of the batch after next, carried per tile by a fused
// launch (hist_next_*).  Device only; every name is TU-local.
#pragma once
#include "decode.h"

namespace {

// The Otsu histograms (white, clip(white - black)) of another capture over this tile's pixel
// range, as u16 counts [2][256] packed in pairs (1 KB per tile) -- the stats pass of the batch
// after next, carried by this fused launch (stats_kernel's partials mode sums the tiles).
// Split so it costs neither latency nor chain time: the loads are issued when the workgroup
// starts (hist_next_load), the nibble planes staged once the points are computed
// (hist_next_stage), the matrix-core counting done by waves 1..3 while wave 0 runs the
// look-back (hist_next_count, as mfma_hist_chunk) and the partial written after it
// (hist_next_write).  Bytes past n_px count as 0 (pad_zero).
__device__ inline void hist_next_load(const uint8_t* white, const uint8_t* black, int64_t n_px, int64_t o,
                                      uint2& wq, uint2& bq) {
  wq = make_uint2(0, 0);
  bq = make_uint2(0, 0);
  if (o < n_px) {                            // frames readable to round_up(n, 8)
    wq = ld_once8_buf(white, uint32_t(o));     // o < n_px < 2^31
    bq = ld_once8_buf(black, uint32_t(o));
  }
}

// stage: [wave][hi_w, lo_w, hi_d, lo_d][64 lanes] uint2 (the lane's 8 pixels per plane)
__device__ inline void hist_next_stage(uint2 wq, uint2 bq, int64_t n_px, int64_t o, uint2* stage) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (o + 8 > n_px) {                        // tail: zero the bytes at or past n_px
    const uint64_t mk = o >= n_px ? 0ull : (~0ull >> (64 - 8 * (n_px - o)));
    wq.x &= uint32_t(mk); wq.y &= uint32_t(mk >> 32);
    bq.x &= uint32_t(mk); bq.y &= uint32_t(mk >> 32);
  }
  const uint32_t m4 = 0x0f0f0f0fu;
  const uint32_t d0 = sub_sat_u8x4(wq.x, bq.x), d1 = sub_sat_u8x4(wq.y, bq.y);
  uint2* st = stage + wave * 256;
  st[lane] = make_uint2((wq.x >> 4) & m4, (wq.y >> 4) & m4);
  st[64 + lane] = make_uint2(wq.x & m4, wq.y & m4);
  st[128 + lane] = make_uint2((d0 >> 4) & m4, (d1 >> 4) & m4);
  st[192 + lane] = make_uint2(d0 & m4, d1 & m4);
}

// Steps h, h + n_help, ... of the tile's kTilePx / 64 MFMA steps (64 pixels each), added to
// s_h[512] (zeroed beforehand) with LDS atomics.
__device__ inline void hist_next_count(const uint2* stage, uint32_t* s_h, int h, int n_help) {
  const int lane = threadIdx.x & 63;
  const uint32_t repx = (uint32_t(lane & 15) * 0x01010101u) ^ 0x0f0f0f0fu;
  v4i32 acc_w = {0, 0, 0, 0}, acc_d = {0, 0, 0, 0};
  for (int step = h; step < kTilePx / 64; step += n_help) {
    const uint2* st = stage + (step >> 3) * 256 + 8 * (step & 7) + 2 * (lane >> 4);   // lanes src, src+1
    const uint4 hw = *reinterpret_cast<const uint4*>(st);
    const uint4 lw = *reinterpret_cast<const uint4*>(st + 64);
    const uint4 hd = *reinterpret_cast<const uint4*>(st + 128);
    const uint4 ld = *reinterpret_cast<const uint4*>(st + 192);
    const v4i32 aw = {onehot16(hw.x, repx), onehot16(hw.y, repx), onehot16(hw.z, repx), onehot16(hw.w, repx)};
    const v4i32 bw = {onehot16(lw.x, repx), onehot16(lw.y, repx), onehot16(lw.z, repx), onehot16(lw.w, repx)};
    const v4i32 ad = {onehot16(hd.x, repx), onehot16(hd.y, repx), onehot16(hd.z, repx), onehot16(hd.w, repx)};
    const v4i32 bd = {onehot16(ld.x, repx), onehot16(ld.y, repx), onehot16(ld.z, repx), onehot16(ld.w, repx)};
    acc_w = __builtin_amdgcn_mfma_i32_16x16x64_i8(aw, bw, acc_w, 0, 0, 0);
    acc_d = __builtin_amdgcn_mfma_i32_16x16x64_i8(ad, bd, acc_d, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int bin = 16 * (4 * (lane >> 4) + r) + (lane & 15);
    if (acc_w[r]) atomicAdd(&s_h[bin], uint32_t(acc_w[r]) >> 8);
    if (acc_d[r]) atomicAdd(&s_h[256 + bin], uint32_t(acc_d[r]) >> 8);
  }
}

__device__ inline void hist_next_write(const uint32_t* s_h, uint32_t* part) {
  for (int i = threadIdx.x; i < kPartWords; i += kTileBlock) part[i] = s_h[2 * i] | (s_h[2 * i + 1] << 16);
}

}  // namespace
