// decode.h -- the bit-plane decode of the fused path: SWAR byte compares, packed Gray -> binary,
// the frame loads (8-byte buffer loads, paired 16-byte loads) and the per-lane / per-pixel decode
// main3_kernel, decode_maps_kernel and the look-back helper share.  Device only; every name is
// TU-local.
#pragma once
#include "fused_params.h"
#include "otsu.h"

namespace {   // (fp contract off: otsu.h's pragma)

constexpr int kMaxBits = 15;                // packed 16-bit code lanes

// Per-byte unsigned p > i on 4 packed bytes: 0x80 in every byte lane where p > i.
__device__ inline uint32_t gt_u8x4(uint32_t p, uint32_t i) {
  // per byte p > i in bit 7 (other bits garbage: callers mask with 0x80808080):
  // f(p, i, d) = (p & ~i) | (~(p ^ i) & ~d), d = (i | 0x80) - (p & 0x7f) per byte, one v_bitop3
  const uint32_t d = (i | 0x80808080u) - (p & 0x7f7f7f7fu);
  uint32_t r;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x71" : "=v"(r) : "v"(p), "v"(i), "v"(d));
  return r;
}

// Gray -> binary on two packed 16-bit lanes (values < 2^15): prefix XOR from the top.
__device__ inline uint32_t gray2bin_x2(uint32_t x) {
  x ^= (x >> 1) & 0x7fff7fffu;
  x ^= (x >> 2) & 0x3fff3fffu;
  x ^= (x >> 4) & 0x0fff0fffu;
  x ^= (x >> 8) & 0x00ff00ffu;
  return x;
}

// ------------------------------------------------------------------ decode (shared by the kernels)
// Bit planes of 4 pixels accumulate one byte per pixel: plane b's compare mask (bit 7 of each
// byte: pattern > inverse) enters at bit 7 while the earlier planes shift down, two VALU ops per
// word per plane.  Planes 0-7 go to word A, planes 8-14 to word B.  After n planes, bit-reversing
// the word (v_bfrev: bits within a byte AND the byte order) leaves pixel k's code MSB-first in
// byte 3-k: A' byte = code >> m, B' byte = code & (2^m - 1), m = max(n - 8, 0).
struct PlaneAcc {
  uint32_t a[2], b[2];       // [pixels 0-3, 4-7]
};

__device__ inline void acc_plane(uint32_t& w, uint32_t m) { w = (w >> 1) | (m & 0x80808080u); }

template <bool HI>
__device__ inline void acc_pair(PlaneAcc& q, uint2 pv, uint2 iv) {
  const uint32_t m0 = gt_u8x4(pv.x, iv.x);
  const uint32_t m1 = gt_u8x4(pv.y, iv.y);
  if (HI) { acc_plane(q.b[0], m0); acc_plane(q.b[1], m1); }
  else { acc_plane(q.a[0], m0); acc_plane(q.a[1], m1); }
}

// The n-plane Gray codes of the lane's 8 pixels as two per word (16-bit halves), converted
// like gray2bin_x2(code << pre) << post: w[2h] = pixels (4h, 4h+2) in (high, low) halves,
// w[2h+1] = pixels (4h+1, 4h+3).
__device__ inline void acc_codes(const PlaneAcc& q, int n, int pre, int post, uint32_t (&w)[4]) {
  const int m = n > 8 ? n - 8 : 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t A = __builtin_bitreverse32(q.a[h]), B = __builtin_bitreverse32(q.b[h]);
    const uint32_t hi = (((A >> 8) & 0x00ff00ffu) << m) | ((B >> 8) & 0x00ff00ffu);
    const uint32_t lo = ((A & 0x00ff00ffu) << m) | (B & 0x00ff00ffu);
    w[2 * h] = gray2bin_x2(hi << pre) << post;
    w[2 * h + 1] = gray2bin_x2(lo << pre) << post;
  }
}

// code of pixel k (0..7) from acc_codes' words
__device__ inline int unpack_code(const uint32_t (&w)[4], int k) {
  const uint32_t a = w[((k >> 2) << 1) | (k & 1)];
  return int((a >> (16 * (1 - ((k >> 1) & 1)))) & 0xffffu);
}

// 8 once-read bytes at base + off as a buffer load (scalar descriptor, 32-bit lane offset).
__device__ inline uint2 ld_once8_buf(const uint8_t* base, uint32_t off) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base), 0, 0xffffffff, 0x00020000);
  const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, SLG_NT_LOADS ? 2 : 0);   // aux 2: nt
  return make_uint2(v[0], v[1]);
}

// 8 frame bytes at pixel lp (clamped in-bounds by the caller; rows are padded to >= 8 px).
// As a buffer load: the frame's base lives in a scalar resource descriptor and the lane offset
// is a 32-bit VGPR (buffer_load_dwordx2 ... offen nt), so the address costs no VALU at all.
__device__ inline uint2 ld_frame8(const MainParams& p, int frame, int64_t lp) {
  // one descriptor for the whole stack, the frame's offset in the scalar soffset (a capture's
  // frames span < 4 GiB: check_capture)
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.frames), 0, 0xffffffff, 0x00020000);
  const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, uint32_t(lp), uint32_t(frame) * uint32_t(p.stride),
                                                      SLG_NT_LOADS ? 2 : 0);   // aux 2: nt
  return make_uint2(v[0], v[1]);
}

// Paired 16-byte frame loads (two-axis decodes): lanes 2j and 2j+1 own pixels [q, q + 16) of the
// tile (q = the even lane's px0, a multiple of 16).  For a frame pair (a, a + 1) -- white / black,
// or a pattern / inverse pair -- the even lane reads 16 bytes of frame a and the odd lane 16 bytes
// of frame a + 1 at q, then the two trade halves (DPP quad_perm [1,0,3,2]), so each holds its own
// 8 pixels of both frames.  Half the vector-memory instructions of two 8-byte loads per lane and
// the same 128-byte lines (tools/fetch_probe.hip: C2's mask-gated reads 11.1 vs 12.1-12.4 us;
// the bench's C2 step 305.5 vs 309.8 us, f64 neutral, profiles/r7l).  Pairing the texture and the
// carried white / black loads too measured slower or neutral (306.2 / 310.6 us; as buffer loads
// 311.2 vs 310.5, profiles/r7l).  An unaligned caller stack keeps the 8-byte loads (GPU test).
// Needs 16-byte aligned frames and stride (else the 8-byte loads run) and both lanes of a pair
// active at the trade.

struct PairLd {
  uint32_t v[4];
};
__device__ inline PairLd ld_pair16(const MainParams& p, int frame_a, uint32_t voff) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.frames), 0, 0xffffffff, 0x00020000);
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, uint32_t(frame_a) * uint32_t(p.stride),
                                                       SLG_NT_LOADS ? 2 : 0);   // aux 2: nt
  return {{v[0], v[1], v[2], v[3]}};
}
// a = this lane's 8 bytes of frame a, b = of frame a + 1
__device__ inline void pair_split(const PairLd& L, bool odd, uint2& a, uint2& b) {
  const uint32_t s0 = odd ? L.v[0] : L.v[2], s1 = odd ? L.v[1] : L.v[3];
  const uint32_t r0 = uint32_t(__builtin_amdgcn_update_dpp(0, int(s0), 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
  const uint32_t r1 = uint32_t(__builtin_amdgcn_update_dpp(0, int(s1), 0xB1, 0xf, 0xf, false));
  a = odd ? make_uint2(r0, r1) : make_uint2(L.v[0], L.v[1]);
  b = odd ? make_uint2(L.v[2], L.v[3]) : make_uint2(r0, r1);
}

// Decode the 8 pixels of one lane: mask bits + column / row codes.  Frame loads of both axes
// are issued up to kBatch pairs at a time before any is consumed (memory-level parallelism).
// `tail` (wave-uniform) is set only in the last tile, where map/texture reads need guards;
// frame reads never do: the frame stride is >= round_up(H*W, 8) and out-of-image lanes read
// pixel 0 (their mask bits are cleared).
// MF (mask first, the fused reconstruction only): the mask is computed from white / black before
// any pattern frame is read, and a lane none of whose 8 pixels is valid reads no pattern frame at
// all (its codes are never used: the reference masks them out, processing.py:121-124,157).  The
// memory system then fetches only the 64-byte segments a valid pixel lies in.  `pre()` runs once
// the lane is known to hold a valid pixel, before its pattern loads (the texture loads).
struct NoPre {
  __device__ void operator()(uint2) const {}
};

// The lane's 8 mask bits: white >= smin, white - black >= cmin, inside the image.
__device__ inline uint32_t mask_bits(uint2 w, uint2 bl, int smin, int cmin, int64_t px0, int64_t n_px) {
  uint32_t valid = 0;
#pragma unroll
  for (int k = 0; k < kPx; ++k) {
    const int wv = ((k < 4 ? w.x : w.y) >> (8 * (k & 3))) & 0xff;
    const int bv = ((k < 4 ? bl.x : bl.y) >> (8 * (k & 3))) & 0xff;
    valid |= uint32_t((wv >= smin) & ((wv - bv) >= cmin) & (px0 + k < n_px)) << k;
  }
  return valid;
}

// PLAN: (col_pairs << 4) | row_pairs as compile-time constants (main3's specialised instances for
// the common capture layouts, SLG_PLAN_*; every view of such a launch has that plan), or 0: the
// counts come from the view's plan at run time.
// Constant counts make every frame load unconditional, so the decode consumes each pair as it
// lands (vmcnt(n) in issue order) instead of after a vmcnt(0) for the whole batch, and drop the
// per-pair branches (243.3 vs 259.8 us per 12-view launch, profiles/r3m).
template <int ROW_MODE, int SRC_FRAMES, int kBatch, bool MF = false, int PLAN = 0, class Pre = NoPre>
__device__ inline void decode_lane(const MainParams& p, int64_t px0, bool tail, uint32_t& valid,
                                   int (&col)[kPx], int (&row)[kPx], Pre pre = Pre()) {
  valid = 0;
  if (SRC_FRAMES) {
    const int smin = p.ws->smin, cmin = p.ws->cmin;
    const int64_t lp = px0 < p.n_px ? px0 : 0;
    // paired 16-byte loads (wave-uniform choice): the pair's base pixel, clamped like lp
    // (column-only decodes -- row_mode 0, C1's 10 pairs -- measured 2-5 % slower paired: there the
    // lanes a partner drags into the decode cost more than the halved loads save)
    const bool paired = ROW_MODE != 0 &&
                        ((reinterpret_cast<uintptr_t>(p.frames) | uint64_t(p.stride)) & 15) == 0;
    const bool odd = (threadIdx.x & 1) != 0;
    const int64_t q = px0 & ~int64_t(15);
    const uint32_t vo = uint32_t(q < p.n_px ? q : 0) + (odd ? uint32_t(p.stride) : 0u);
    uint2 w, bl;
    if (paired) pair_split(ld_pair16(p, 0, vo), odd, w, bl);
    else { w = ld_frame8(p, 0, lp); bl = ld_frame8(p, 1, lp); }
    if constexpr (MF) {
      valid = mask_bits(w, bl, smin, cmin, px0, p.n_px);
#pragma unroll
      for (int k = 0; k < kPx; ++k) col[k] = row[k] = 0;
      // paired: a pair reads its pattern frames if either lane has a valid pixel (both must
      // take part in the trades); the other lane's codes are never used
      const uint32_t go = paired ? (valid | uint32_t(__builtin_amdgcn_update_dpp(0, int(valid), 0xB1, 0xf, 0xf, false)))
                                 : valid;
      if (go == 0u) return;
      if (valid != 0u) pre(w);                    // (white bytes: a gray capture's texture)
    }
    PlaneAcc qc = {{0, 0}, {0, 0}}, qr = {{0, 0}, {0, 0}};
    const int np_c = PLAN ? ((PLAN >> 4) & 15) : p.plan.col_pairs;
    const int np_r = ROW_MODE == 0 ? 0 : (PLAN ? (PLAN & 15) : p.plan.row_pairs);
    // compile-time trip count (kMaxBits pairs max), fully unrolled: only forward, wave-uniform
    // branches remain, so the loads of a batch stay in flight together (no vmcnt(0) per load)
    if (paired) {
#pragma unroll
      for (int b0 = 0; b0 < kMaxBits; b0 += kBatch) {
        PairLd cl[kBatch], rl[kBatch];
#pragma unroll
        for (int g = 0; g < kBatch; ++g)
          if (b0 + g < np_c) cl[g] = ld_pair16(p, p.plan.col_first + 2 * (b0 + g), vo);
#pragma unroll
        for (int g = 0; g < kBatch; ++g)
          if (b0 + g < np_r) rl[g] = ld_pair16(p, p.plan.row_first + 2 * (b0 + g), vo);
#pragma unroll
        for (int g = 0; g < kBatch; ++g)
          if (b0 + g < np_c) {
            uint2 pv, iv;
            pair_split(cl[g], odd, pv, iv);
            if (b0 + g < 8) acc_pair<false>(qc, pv, iv);
            else acc_pair<true>(qc, pv, iv);
          }
#pragma unroll
        for (int g = 0; g < kBatch; ++g)
          if (b0 + g < np_r) {
            uint2 pv, iv;
            pair_split(rl[g], odd, pv, iv);
            if (b0 + g < 8) acc_pair<false>(qr, pv, iv);
            else acc_pair<true>(qr, pv, iv);
          }
      }
    } else {
#pragma unroll
    for (int b0 = 0; b0 < kMaxBits; b0 += kBatch) {
      uint2 cp[kBatch], ci[kBatch], rp[kBatch], ri[kBatch];
#pragma unroll
      for (int g = 0; g < kBatch; ++g)
        if (b0 + g < np_c) {
          cp[g] = ld_frame8(p, p.plan.col_first + 2 * (b0 + g), lp);
          ci[g] = ld_frame8(p, p.plan.col_first + 2 * (b0 + g) + 1, lp);
        }
#pragma unroll
      for (int g = 0; g < kBatch; ++g)
        if (b0 + g < np_r) {
          rp[g] = ld_frame8(p, p.plan.row_first + 2 * (b0 + g), lp);
          ri[g] = ld_frame8(p, p.plan.row_first + 2 * (b0 + g) + 1, lp);
        }
#pragma unroll
      for (int g = 0; g < kBatch; ++g)
        if (b0 + g < np_c) {
          if (b0 + g < 8) acc_pair<false>(qc, cp[g], ci[g]);
          else acc_pair<true>(qc, cp[g], ci[g]);
        }
#pragma unroll
      for (int g = 0; g < kBatch; ++g)
        if (b0 + g < np_r) {
          if (b0 + g < 8) acc_pair<false>(qr, rp[g], ri[g]);
          else acc_pair<true>(qr, rp[g], ri[g]);
        }
    }
    }
    uint32_t ac[4], ar[4];
    acc_codes(qc, np_c, p.plan.col_pre, p.plan.col_post, ac);
    acc_codes(qr, np_r, p.plan.row_pre, p.plan.row_post, ar);
    if constexpr (!MF) valid = mask_bits(w, bl, smin, cmin, px0, p.n_px);
#pragma unroll
    for (int k = 0; k < kPx; ++k) {
      col[k] = unpack_code(ac, k);
      row[k] = ROW_MODE != 0 ? unpack_code(ar, k) : 0;
    }
  } else {
    if (!tail) {
      const uint2 mv = *reinterpret_cast<const uint2*>(p.in_mask + px0);
      const int4* ic = reinterpret_cast<const int4*>(p.in_col + px0);
      const int4 c0 = ic[0], c1 = ic[1];
      col[0] = c0.x; col[1] = c0.y; col[2] = c0.z; col[3] = c0.w;
      col[4] = c1.x; col[5] = c1.y; col[6] = c1.z; col[7] = c1.w;
      if constexpr (ROW_MODE != 0) {
        const int4* ir = reinterpret_cast<const int4*>(p.in_row + px0);
        const int4 r0 = ir[0], r1 = ir[1];
        row[0] = r0.x; row[1] = r0.y; row[2] = r0.z; row[3] = r0.w;
        row[4] = r1.x; row[5] = r1.y; row[6] = r1.z; row[7] = r1.w;
      } else {
#pragma unroll
        for (int k = 0; k < kPx; ++k) row[k] = 0;
      }
#pragma unroll
      for (int k = 0; k < kPx; ++k) valid |= uint32_t((((k < 4 ? mv.x : mv.y) >> (8 * (k & 3))) & 0xff) != 0) << k;
    } else {
#pragma unroll
      for (int k = 0; k < kPx; ++k) {
        const bool in = px0 + k < p.n_px;
        col[k] = in ? p.in_col[px0 + k] : 0;
        row[k] = (in && ROW_MODE != 0) ? p.in_row[px0 + k] : 0;
        valid |= uint32_t(in && p.in_mask[px0 + k] != 0) << k;
      }
    }
  }
}

// clamp like np.clip(idx, 0, n-1) (processing.py:159,189) and pack col | row << 16
template <int ROW_MODE>
__device__ inline uint32_t pack_code(const MainParams& p, int c, int r) {
  c = c < 0 ? 0 : (c > p.n_pcol - 1 ? p.n_pcol - 1 : c);
  r = ROW_MODE == 0 ? 0 : (r < 0 ? 0 : (r > p.n_prow - 1 ? p.n_prow - 1 : r));
  return uint32_t(c) | (uint32_t(r) << 16);
}

// One pixel decoded exactly as decode_lane decodes it, with byte loads and few registers
// (the look-back helper path only).
template <int ROW_MODE, int SRC_FRAMES>
__device__ inline bool decode_px(const MainParams& p, int64_t px, int& col, int& row) {
  if (SRC_FRAMES) {
    const uint8_t* f = p.frames + px;
    const int wv = f[0], bv = f[p.stride];
    uint32_t c = 0, r = 0;
    for (int b = 0; b < p.plan.col_pairs; ++b)
      c = (c << 1) | uint32_t(f[int64_t(p.plan.col_first + 2 * b) * p.stride] > f[int64_t(p.plan.col_first + 2 * b + 1) * p.stride]);
    col = int(gray2bin_x2(c << p.plan.col_pre) << p.plan.col_post);
    if (ROW_MODE != 0) {
      for (int b = 0; b < p.plan.row_pairs; ++b)
        r = (r << 1) | uint32_t(f[int64_t(p.plan.row_first + 2 * b) * p.stride] > f[int64_t(p.plan.row_first + 2 * b + 1) * p.stride]);
      r = gray2bin_x2(r << p.plan.row_pre) << p.plan.row_post;
    }
    row = int(r);
    return (wv >= p.ws->smin) & ((wv - bv) >= p.ws->cmin);
  }
  col = p.in_col[px];
  row = ROW_MODE != 0 ? p.in_row[px] : 0;
  return p.in_mask[px] != 0;
}

}  // namespace
