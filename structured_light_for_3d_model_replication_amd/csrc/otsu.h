// otsu.h -- device code of the mask thresholds: wave helpers, the one-wave Otsu (OpenCV's
// operation order), the NumPy percentile, the matrix-core histograms, and the "thresholds from
// summed histograms / from per-tile partials" tails shared by stats_kernel, parts_kernel,
// hist_thresholds_kernel (stats.hip) and main3's finishing workgroups (slgpu.hip).  Device only; every name
// is TU-local.  SLG_OTSU_MARK(k): a hook per part of otsu_wave (tools/otsu_probe.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <utility>

#include "../../include/slgpu.h"
#include "workspace.h"

#pragma clang fp contract(off)

namespace {

#ifndef SLG_NT_LOADS
#define SLG_NT_LOADS 1                     // frames / texture are read once: non-temporal loads
#endif
// Once-read stream (frames, texture): non-temporal 8-byte load (global_load_dwordx2 nt).
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
__device__ inline uint2 ld_once8(const void* ptr) {
#if SLG_NT_LOADS
  const u32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(ptr));
  return make_uint2(v.x, v.y);
#else
  return *reinterpret_cast<const uint2*>(ptr);
#endif
}

template <class T>
__device__ inline T wave_sum(T x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// a / b correctly rounded from y = RN(1/b) (Markstein): with y correctly rounded and q1
// faithful, q2 = RN(q1 + (a - b*q1) * y) = RN(a / b); q0 = RN(a*y) is within 1.5 ulp, so one
// correction makes q1 faithful and the second one is exact (tools/markstein_check.c checks it
// against IEEE division).  Valid while nothing over/underflows: div_rn_ok() vets a, the
// caller vets b and y.
__device__ inline double div_rn(double a, double b, double y) {
  const double q0 = a * y;
  const double q1 = fma(fma(-b, q0, a), y, q0);
  return fma(fma(-b, q1, a), y, q1);
}
__device__ inline bool div_rn_ok(double a) {
  const double m = fabs(a);
  return m == 0.0 || (m > 0x1p-900 && m < 0x1p900);
}

// OpenCV getThreshVal_Otsu_8u (see oracle/sl_oracle.py:otsu_from_hist) evaluated by one wave.
// Bit-exact with the sequential fp64 loop: only order-independent pieces run in parallel.
//  * mu = sum(i*h[i]) of exact integers (< 2^53) == OpenCV's sequential double sum;
//  * q1 (running sum of p_i = h[i]*scale) is one sequential add chain (same rounding as the
//    loop); it alone decides which bins OpenCV skips, so the skip flags, i*p_i and
//    y = RN(1/q1) are then computed lane-parallel, bin i on lane i/4;
//  * the remaining chain mu1 = (mu1*q1_prev + i*p_i)/q1 runs on wave-uniform registers up to
//    the last unskipped bin, each division as the Markstein pair div_rn(., q1, y) (IEEE
//    division when div_rn_ok refuses the numerator): 7 dependent fp64 ops per bin instead of a
//    full IEEE division sequence;
//  * sigma per bin and the first-maximum argmax (strict '>' from 0) are lane-parallel.
__device__ inline double readlane_f64(double v, int l) {
  const uint64_t b = uint64_t(__double_as_longlong(v));
  const uint32_t lo = __builtin_amdgcn_readlane(uint32_t(b), l);
  const uint32_t hi = __builtin_amdgcn_readlane(uint32_t(b >> 32), l);
  return __longlong_as_double((long long)((uint64_t(hi) << 32) | lo));
}

// otsu_wave's exact mu1 run over bins [lo, hi] (the rerun when the speculative chain misses):
// each quotient as the Markstein pair div_rn(a, q1, y).
__device__ inline void mu1_run_exact(int lo, int hi, const double (&ip)[4], const double (&q1r)[4],
                                     const double (&yr)[4], double (&m1r)[4]) {
  const int lane = threadIdx.x & 63;
  double mu1 = 0.0, q_prev = 0.0;                    // bin i's previous q1 is bin i-1's q1 (mu1 = 0 at lo)
  for (int l = lo >> 2; l <= (hi >> 2); ++l) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = 4 * l + j;
      if (i < lo || i > hi) continue;                // scalar: first and last lane only
      const double a = mu1 * q_prev + readlane_f64(ip[j], l);
      q_prev = readlane_f64(q1r[j], l);
      mu1 = div_rn(a, q_prev, readlane_f64(yr[j], l));
      if (lane == l) m1r[j] = mu1;
    }
  }
}

// Pixels of a 256-bin histogram at or above bin m (the wave's sum).  n when m <= 0: the clipped
// difference histogram puts every negative white - black into bin 0, so it cannot tell which of
// them reach a threshold below 1 (for white, m <= 0 is every pixel anyway).
__device__ __attribute__((always_inline)) inline int64_t hist_at_least_wave(const uint32_t* h, int m, int64_t n) {
  if (m <= 0) return n;
  const int lane = threadIdx.x & 63;
  uint64_t a = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int b = 64 * j + lane;
    if (b >= m) a += h[b];
  }
  return int64_t(wave_sum(a));
}

// The resident-job arena reservation of one view, by the thread that finishes its thresholds,
// from its two `above` counts: see WsHeader::arena_off.
__device__ inline void arena_reserve(WsHeader* ws, int64_t a0, int64_t a1) {
  unsigned long long* cur = ws->arena_cursor;
  if (!cur) return;
  const int64_t need = (a0 < a1 ? a0 : a1) * int64_t(ws->arena_mult);
  const int64_t off = int64_t(atomicAdd(cur, (unsigned long long)need));
  ws->arena_off = off + need <= ws->arena_cap ? off : -1;
}

// The two serial chains of otsu_wave (q1, then mu1) run on wave-uniform registers fed from LDS:
// every lane computes the same chain, its per-bin operands read as broadcast LDS words, and only
// the value after each lane's four bins is captured (one 64-bit select per four steps); each
// lane then redoes its own four steps from its left neighbour's capture -- the same operations on
// the same values in the same order, so the same bits.  A dependent fp64 op costs ~5 clocks
// (tools/dp_latency_probe.hip), so a step costs its instruction count (profiles/r5y: 7.8 us for
// one 1080p histogram).  lds: kOtsuLds doubles of this wave's own.
#ifndef SLG_OTSU_MARK
#define SLG_OTSU_MARK(k)                   // tools/otsu_probe.hip: a timestamp per part of otsu_wave
#endif
#ifndef SLG_OTSU_UNROLL
#define SLG_OTSU_UNROLL 2                  // the chain loops: steps per loop body
#endif
constexpr int kOtsuLds = 5 * 256;          // p_i [256] + the mu1 chain's {q1[i-1], ip, y, c} [256][4]

__device__ __attribute__((always_inline)) inline double otsu_wave(const uint32_t* h, int64_t n, double* lds) {
  SLG_OTSU_MARK(0);
  const int lane = threadIdx.x & 63;
  const double scale = 1.0 / double(n);
  const double eps = double(__FLT_EPSILON__);
  double* sp = lds;                 // p_i
  double pv[4], ip[4], q1r[4], yr[4], m1r[4], ar[4];
  uint64_t isum = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = 4 * lane + j;
    pv[j] = double(h[i]) * scale;
    ip[j] = double(i) * pv[j];
    isum += uint64_t(i) * h[i];
    q1r[j] = yr[j] = m1r[j] = ar[j] = 0.0;
    sp[i] = pv[j];
  }
  isum = wave_sum(isum);
  const double mu = double(isum) * scale;
  SLG_OTSU_MARK(1);
  // 1. the q1 chain (OpenCV's order) from broadcast LDS reads (wave-local: the wave's own LDS ops
  // are in order, the fence only keeps the compiler from moving them)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  {
    double q1 = 0.0, qcap = 0.0;
#pragma unroll SLG_OTSU_UNROLL
    for (int l0 = 0; l0 < 64; l0 += 4) {
      double pp[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) pp[k] = sp[4 * l0 + k];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) q1 = q1 + pp[4 * t + j];
        qcap = lane == l0 + t ? q1 : qcap;
      }
    }
    double q = __shfl_up(qcap, 1);
    if (lane == 0) q = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      q = q + pv[j];
      q1r[j] = q;
    }
  }
  SLG_OTSU_MARK(2);
  uint32_t okr = 0;                                  // 2. bit j: bin 4*lane+j not skipped
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double q2 = 1.0 - q1r[j];
    if (!(fmin(q1r[j], q2) < eps || fmax(q1r[j], q2) > 1.0 - eps)) {
      okr |= 1u << j;
      yr[j] = 1.0 / q1r[j];
    }
  }
  // 3. the mu1 chain.  The unskipped bins form one run [lo, hi]: q1 never decreases and
  // q2 = RN(1 - q1) never increases, so each skip test holds on a prefix plus a suffix of the
  // bins, and mu1 is still 0 at lo.  Over the run every bin is the same few dependent ops,
  // each quotient taken speculatively as fma(a, y, a * c) with c = fma(-q1, y, 1) * y (y + c
  // is 1/q1 to ~2^-105): faithful, and RN(a / q1) unless a / q1 sits within ~2^-105 of a
  // rounding boundary -- so every bin is checked afterwards (Markstein: RN(m + (a - q1 m) y)
  // = RN(a / q1) for faithful m) and the run is redone exactly on a miss.  That needs every
  // numerator to suit div_rn: a is 0, or at least ~1/n (an empty bin's mu1 *= q1 then / q1
  // moves a by ulps), so n <= 2^52 keeps a far inside its range.  Anything else (never seen)
  // takes the general loop: per-bin skip flags, IEEE division when refused.
  SLG_OTSU_MARK(3);
  const uint64_t lanes_ok = __ballot(okr != 0);
  int lo = 256, hi = -1, n_ok = 0;
  if (lanes_ok) {
    const int l_lo = __builtin_ctzll(lanes_ok), l_hi = 63 - __builtin_clzll(lanes_ok);
    lo = 4 * l_lo + __builtin_ctz(__builtin_amdgcn_readlane(okr, l_lo));
    hi = 4 * l_hi + 31 - __builtin_clz(__builtin_amdgcn_readlane(okr, l_hi));
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) n_ok += __popcll(__ballot((okr >> j) & 1u));
  double mu1 = 0.0;
  SLG_OTSU_MARK(4);
  if (n_ok == hi - lo + 1 && n <= (int64_t(1) << 52)) {
    {                                                // per bin {q1[i-1], ip, y, c}, 32 bytes
      double* sops = lds + 256;
      const double qprev0 = __shfl_up(q1r[3], 1);
      double cr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double* o = sops + 4 * (4 * lane + j);
        cr[j] = fma(-q1r[j], yr[j], 1.0) * yr[j];
        o[0] = j == 0 ? qprev0 : q1r[j - 1];
        o[1] = ip[j];
        o[2] = yr[j];
        o[3] = cr[j];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // the chain over [lo, hi] (mu1 is 0 at lo, whatever q1[lo-1]), one capture per 4 bins:
      // mcap of lane l = mu1 after bin min(4l + 3, hi)
      double mu1c = 0.0, mcap = 0.0;
      const int g_lo = lo >> 2, g_hi = hi >> 2;
      // the edge groups (partial) apart, so the middle ones are one straight-line body the
      // scheduler can unroll and issue the next group's LDS reads ahead in (an explicitly
      // double-buffered form measured no faster: the buffers were shuffled through extra
      // registers, profiles/r5x)
      auto edge = [&](int l) {
        double o[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) o[k] = sops[16 * l + k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = 4 * l + j;
          if (i >= lo && i <= hi) {                  // (wave-uniform)
            const double a = mu1c * o[4 * j] + o[4 * j + 1];
            mu1c = fma(a, o[4 * j + 2], a * o[4 * j + 3]);
          }
        }
        mcap = lane == l ? mu1c : mcap;
      };
      edge(g_lo);
#pragma unroll SLG_OTSU_UNROLL
      for (int l = g_lo + 1; l < g_hi; ++l) {
        double o[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) o[k] = sops[16 * l + k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double a = mu1c * o[4 * j] + o[4 * j + 1];
          mu1c = fma(a, o[4 * j + 2], a * o[4 * j + 3]);
        }
        mcap = lane == l ? mu1c : mcap;
      }
      if (g_hi > g_lo) edge(g_hi);
      // every lane redoes its own bins from its left neighbour's capture (0 before g_lo)
      double m = __shfl_up(mcap, 1);
      if (lane <= g_lo) m = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = 4 * lane + j;
        const double qp = j == 0 ? qprev0 : q1r[j - 1];
        const double a = m * qp + ip[j];
        const double mj = fma(a, yr[j], a * cr[j]);
        if (i >= lo && i <= hi) {
          m = mj;
          m1r[j] = mj;
          ar[j] = a;
        }
      }
    }
    SLG_OTSU_MARK(5);
    uint32_t miss = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double r = fma(-q1r[j], m1r[j], ar[j]);   // exact remainder
      if ((okr >> j) & 1u) miss |= uint32_t(fma(r, yr[j], m1r[j]) != m1r[j]);
    }
    if (__ballot(miss != 0)) mu1_run_exact(lo, hi, ip, q1r, yr, m1r);
  } else {
    const int l_end = 64 - __builtin_clzll(lanes_ok | 1ull);   // lanes with work: [0, l_end)
    double q_prev = 0.0;
    for (int l = 0; l < l_end; ++l) {
      const uint32_t okl = __builtin_amdgcn_readlane(okr, l);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        mu1 *= q_prev;                               // mu1 *= q1 (previous q1)
        const double q = readlane_f64(q1r[j], l);
        if (okl & (1u << j)) {
          const double a = mu1 + readlane_f64(ip[j], l);
          mu1 = div_rn_ok(a) ? div_rn(a, q, readlane_f64(yr[j], l)) : a / q;
          if (lane == l) m1r[j] = mu1;
        }
        q_prev = q;
      }
    }
  }
  SLG_OTSU_MARK(6);
  double best = 0.0;
  int best_i = INT_MAX;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!(okr & (1u << j))) continue;
    const double q1j = q1r[j], q2 = 1.0 - q1j, mu1j = m1r[j];
    const double mu2 = (mu - q1j * mu1j) / q2;
    const double sigma = q1j * q2 * (mu1j - mu2) * (mu1j - mu2);
    if (sigma > best) { best = sigma; best_i = 4 * lane + j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o);
    const int oi = __shfl_xor(best_i, o);
    if (ob > best || (ob == best && oi < best_i)) { best = ob; best_i = oi; }
  }
  SLG_OTSU_MARK(7);
  return best_i == INT_MAX ? 0.0 : double(best_i);
}

// smallest integer x in [lo, 256] with double(x) > thr (256 = none reachable)
__device__ inline int int_threshold(double thr, int lo) {
  if (!(thr == thr)) return 256;                 // NaN: comparison always false
  if (thr < double(lo)) return lo;
  if (thr >= 256.0) return 256;
  return int(floor(thr)) + 1;
}

// k-th smallest value (0-based) from a 256-bin histogram.
__device__ __attribute__((always_inline)) inline int kth_from_hist(const uint32_t* h, int64_t k) {
  int64_t c = 0;
  for (int v = 0; v < 256; ++v) {
    c += h[v];
    if (c > k) return v;
  }
  return 255;
}

// np.percentile(float32 image, 95) with method 'linear' (numpy 2.x _quantile/_lerp, float32).
__device__ __attribute__((always_inline)) inline float percentile95_from_hist(const uint32_t* h, int64_t n) {
  const float q = 95.0f / 100.0f;                       // np.true_divide(95, float32(100))
  const float vi = float(n - 1) * q;                    // (n-1) * quantiles, float32
  float prev = floorf(vi);
  float next = prev + 1.0f;
  const float gamma = vi - prev;
  int64_t pi = int64_t(prev), ni = int64_t(next);
  if (vi >= float(n - 1)) { pi = n - 1; ni = n - 1; }   // index -1 -> last element
  const float a = float(kth_from_hist(h, pi));
  const float b = float(kth_from_hist(h, ni));
  const float diff = b - a;
  float r = a + diff * gamma;
  if (gamma >= 0.5f) r = b - diff * (1.0f - gamma);
  return r;
}

// ---- Otsu histograms on the i8 matrix cores.  For 64 pixels v_k (k = 16 * lane-group + byte),
// A[m][k] = 16 * [v_k >> 4 == m] and B[k][n] = 16 * [v_k & 15 == n], so one
// v_mfma_i32_16x16x64_i8 adds 256 x the count of every value v = 16m + n: no LDS atomics (which
// retire about one lane per clock).  The 16 lanes of a row group (lane >> 4) hold the same 16
// pixels, each against its own m or n = lane & 15.  Operand dwords are built in two VALU ops:
// ((nib ^ (m ^ 15)) + 1) & 0x10 = 16 - (nib ^ m) masked to bit 4, i.e. 0x10 iff nib == m (no
// carries between bytes: every byte stays in 1..16).  Lane maps checked by
// tools/mfma_hist_probe.hip; C/D: col = lane & 15, row = 4 * (lane >> 4) + r.
//
// main3's carried count (hist_next_count: other waves' pixels) stages nibble planes in LDS and
// reads them with broadcast ds_read_b128.  stats_kernel counts each wave's own pixels
// (hist_chunk_dpp): MFMA step i takes row group g's pixels from lane 16 g + i by a DPP
// row_newbcast folded into the operand's add, so no LDS at all -- the LDS form read 4 KB per wave
// and step through the CU's LDS port, four waves per CU, which bounded the count.  The folded
// add cannot also take the xor, so those operands are step functions, 0x10 iff nib >= m
// ((nib + 16 - m) & 0x10), the MFMA sums S[m][n] = #{hi >= m, lo >= n}, and the wave's
// histogram is the 2-D difference S[m][n] - S[m+1][n] - S[m][n+1] + S[m+1][n+1] taken once on
// the accumulators (hist_from_cumulative).
typedef int v4i32 __attribute__((ext_vector_type(4)));
constexpr int kHistChunk = 1024;            // pixels per wave and MFMA chunk (16 per lane)
constexpr int64_t kHistMaxChunks = 8000;    // per wave: 8000 * 1024 * 256 < 2^31 (i32 accumulators)

__device__ inline uint32_t sub_sat_u8x4(uint32_t w, uint32_t b) {   // per byte max(w - b, 0)
  const uint32_t dl = ((w & 0x00ff00ffu) | 0x01000100u) - (b & 0x00ff00ffu);   // 256 + w - b
  const uint32_t dh = (((w >> 8) & 0x00ff00ffu) | 0x01000100u) - ((b >> 8) & 0x00ff00ffu);
  const uint32_t ml = ((dl >> 8) & 0x00010001u) * 0xffu, mh = ((dh >> 8) & 0x00010001u) * 0xffu;
  return (dl & ml) | ((dh & mh) << 8);
}

__device__ inline int onehot16(uint32_t nib, uint32_t repx) {      // bytes: 0x10 iff nib == m
  return int(((nib ^ repx) + 0x01010101u) & 0x10101010u);
}

// Step I of a chunk: per byte 0x10 iff the nibble of lane 16 * (lane >> 4) + I >= m, where
// c = (16 - m) per byte, m = lane & 15.  Bytes stay in 1..31: no carries.
template <int I>
__device__ inline int ge16_bcast(uint32_t plane, uint32_t c) {
  const uint32_t b = uint32_t(__builtin_amdgcn_update_dpp(0, int(plane), 0x150 + I, 0xf, 0xf, false));  // row_newbcast:I
  return int((b + c) & 0x10101010u);
}

// pl: the lane's 16 pixels as nibble planes {hi(w)[4], lo(w)[4], hi(d)[4], lo(d)[4]}
template <int I>
__device__ inline void hist_step_dpp(const uint32_t (&pl)[16], uint32_t c, v4i32& acc_w, v4i32& acc_d) {
  const v4i32 aw = {ge16_bcast<I>(pl[0], c), ge16_bcast<I>(pl[1], c), ge16_bcast<I>(pl[2], c), ge16_bcast<I>(pl[3], c)};
  const v4i32 bw = {ge16_bcast<I>(pl[4], c), ge16_bcast<I>(pl[5], c), ge16_bcast<I>(pl[6], c), ge16_bcast<I>(pl[7], c)};
  const v4i32 ad = {ge16_bcast<I>(pl[8], c), ge16_bcast<I>(pl[9], c), ge16_bcast<I>(pl[10], c), ge16_bcast<I>(pl[11], c)};
  const v4i32 bd = {ge16_bcast<I>(pl[12], c), ge16_bcast<I>(pl[13], c), ge16_bcast<I>(pl[14], c), ge16_bcast<I>(pl[15], c)};
  acc_w = __builtin_amdgcn_mfma_i32_16x16x64_i8(aw, bw, acc_w, 0, 0, 0);
  acc_d = __builtin_amdgcn_mfma_i32_16x16x64_i8(ad, bd, acc_d, 0, 0, 0);
}

template <int... Is>
__device__ inline void hist_steps_dpp(std::integer_sequence<int, Is...>, const uint32_t (&pl)[16], uint32_t c,
                                      v4i32& acc_w, v4i32& acc_d) {
  (hist_step_dpp<Is>(pl, c, acc_w, acc_d), ...);
}

// One wave adds its 1024 pixels (pixel c + 16 * lane + byte: white w[], clip(white - black) d[])
// into its cumulative accumulators S_w, S_d (256 x #{hi >= m, lo >= n}).
__device__ inline void hist_chunk_dpp(const uint32_t (&w)[4], const uint32_t (&d)[4], v4i32& acc_w, v4i32& acc_d) {
  const uint32_t m4 = 0x0f0f0f0fu;
  const uint32_t c = (16u - uint32_t(threadIdx.x & 15)) * 0x01010101u;
  uint32_t pl[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    pl[q] = (w[q] >> 4) & m4; pl[4 + q] = w[q] & m4;
    pl[8 + q] = (d[q] >> 4) & m4; pl[12 + q] = d[q] & m4;
  }
  hist_steps_dpp(std::make_integer_sequence<int, 16>(), pl, c, acc_w, acc_d);
}

// S (this lane's C/D entries: row 4 * (lane >> 4) + r, col lane & 15) -> the histogram entries
// S[m][n] - S[m+1][n] - S[m][n+1] + S[m+1][n+1], S past row / column 15 being 0.
__device__ inline v4i32 hist_from_cumulative(v4i32 s) {
  const int lane = threadIdx.x & 63;
  const int below = __shfl_down(s[0], 16);        // row 4 * (g + 1): lane + 16, same column
  v4i32 dm;
  dm[0] = s[0] - s[1]; dm[1] = s[1] - s[2]; dm[2] = s[2] - s[3]; dm[3] = s[3] - (lane < 48 ? below : 0);
  v4i32 h;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int right = __shfl_down(dm[r], 1);       // column n + 1: lane + 1
    h[r] = dm[r] - ((lane & 15) != 15 ? right : 0);
  }
  return h;
}

// 16 pixels of white and clip(white - black) for lane `lane` of the chunk at c; bytes at or
// past n_px read as 0 (the last arriver removes them from bin 0).
__device__ inline void hist_load(const uint8_t* white, const uint8_t* black, int64_t c, int64_t n_px,
                                 uint32_t (&w)[4], uint32_t (&d)[4]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int h = 0; h < 2; ++h) {             // two 8-byte loads
    const int64_t o = c + 16 * lane + 8 * h;
    const int64_t so = o < n_px ? o : 0;    // frames readable to round_up(n, 8)
    uint2 wq = ld_once8(white + so);
    uint2 bq = ld_once8(black + so);
    if (o + 8 > n_px) {                     // tail: zero the bytes at or past n_px
      const int64_t keep = n_px - o;        // <= 0: none
      const uint64_t mk = keep <= 0 ? 0 : (~0ull >> (64 - 8 * keep));
      wq.x &= uint32_t(mk); wq.y &= uint32_t(mk >> 32);
      bq.x &= uint32_t(mk); bq.y &= uint32_t(mk >> 32);
    }
    w[2 * h] = wq.x; w[2 * h + 1] = wq.y;
    d[2 * h] = sub_sat_u8x4(wq.x, bq.x); d[2 * h + 1] = sub_sat_u8x4(wq.y, bq.y);
  }
}

// The mask thresholds of a view from its summed histograms into ws (stats_kernel's last arriver,
// hist_thresholds_kernel): Otsu of hg[0..255] (white) and hg[256..511] (clip(white - black)) by
// waves 0 and 1 concurrently, with the bound of the valid pixels (WsHeader::above); or the
// percentile rule from hg[0..255] (black) and maxd = max(white - black) + 256.  otsu_lds: two
// waves' kOtsuLds doubles.  Then the resident-job arena reservation (no cursor: nothing).
__device__ __attribute__((always_inline)) inline void set_thresholds(const uint32_t* hg, uint32_t maxd, int64_t n_px,
                                                                     bool otsu, WsHeader* ws, double* otsu_lds,
                                                                     int64_t* s_above) {
  const int tid = threadIdx.x, wave = tid >> 6;
  if (otsu) {
    if (wave < 2) {                            // wave 0: white, wave 1: clip(w-b); concurrently
      const double thr = otsu_wave(hg + 256 * wave, n_px, otsu_lds + wave * kOtsuLds);
      const int m = int_threshold(thr, wave == 0 ? 0 : -255);
      const int64_t above = hist_at_least_wave(hg + 256 * wave, m, n_px);
      if ((tid & 63) == 0) {
        if (wave == 0) { ws->smin = m; ws->thr_s = thr; } else { ws->cmin = m; ws->thr_c = thr; }
        ws->above[wave] = above;
        s_above[wave] = above;
      }
    }
  } else if (tid < 2) {
    double thr;
    if (tid == 0) {
      const float nf = percentile95_from_hist(hg, n_px);
      thr = double(nf * 1.5f);                           // noise_floor * 1.5 (float32)
    } else {
      const float dr = float(int(maxd) - 256);           // np.max(contrast)
      thr = double(dr * 0.05f);                          // dynamic_range * 0.05 (float32)
    }
    const int m = int_threshold(thr, tid == 0 ? 0 : -255);
    if (tid == 0) { ws->smin = m; ws->thr_s = thr; } else { ws->cmin = m; ws->thr_c = thr; }
    ws->above[tid] = n_px;                     // (the percentile histogram is black's: no bound)
    s_above[tid] = n_px;
  }
  __syncthreads();
  if (tid == 0) arena_reserve(ws, s_above[0], s_above[1]);
}

// The view's histogram copies summed into hg[0..511] by 256 lanes (lane t: bins t and t + 256),
// every copy of both bins loaded before any is summed: one round trip (a loop over the two bins
// took two, 1.6 us of a one-view call's stats launch).  pad: the zero padding past n_px, taken
// off bins 0 and 256.  Agent-scope atomic loads: see stats_kernel's ticket.
__device__ __attribute__((always_inline)) inline void sum_hist_copies(const uint32_t* hist_part, int tid, uint32_t pad,
                                                                     uint32_t* hg) {
  uint32_t v[2][kHistCopies];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < kHistCopies; ++c)
      v[r][c] = __hip_atomic_load(hist_part + c * 512 + tid + 256 * r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    uint32_t acc = 0;
#pragma unroll
    for (int c = 0; c < kHistCopies; ++c) acc += v[r][c];
    hg[tid + 256 * r] = acc - (tid == 0 ? pad : 0u);
  }
}

// Otsu thresholds from the per-tile partial histograms a fused launch left in each view's
// workspace slice (the carried "batch after next", hist_next_*): the lean counterpart of
// stats_kernel for the streaming pipeline.  It runs on a side stream BESIDE a fused launch, so
// it holds as few CU resources as it can: 2 KB of LDS, no frame reads, every partial of a
// workgroup's tile range in flight at once (kPartsInFlight loads per lane), then <= 512 global
// adds, a ticket, and the same Otsu tail as stats_kernel in the last arriver.
constexpr int kPartsInFlight = 16;
constexpr int kPartsLdsWords = 512 + 4 * kOtsuLds + 4;
constexpr int kPartsBlocksMax = 64;         // workgroups per view (each sums a contiguous tile range)

// One workgroup's share of "thresholds from partials" for one view: workgroup `block` of
// `n_blocks` sums its contiguous range of the view's n_parts per-tile partials, adds them into
// the view's histogram copies, takes a ticket; the last arriver runs Otsu, writes the mask
// thresholds and resets the histogram state.  Also zeroes the view's look-back words (arming
// the main launch that will use these thresholds; ordered by the kernel boundary).  256 lanes;
// hg: kPartsLdsWords words of LDS (512 histogram words + 2 x kOtsuLds doubles + 2 int64,
// 16-byte aligned), s_last: one.  Used by parts_kernel and by main3's finishing workgroups.
__device__ __attribute__((always_inline)) inline void otsu_from_parts(const uint32_t* pp, WsHeader* ws, int64_t n_parts, int64_t n_px,
                                int64_t n_state_words, int64_t pad_zero, int block, int n_blocks,
                                uint32_t* hg, uint32_t* s_last) {
  const int tid = threadIdx.x, wave = tid >> 6;
  int64_t* s_above = reinterpret_cast<int64_t*>(hg + 512 + 4 * kOtsuLds);
  const bool act = tid < kBlock;               // the work is laid out for 256 lanes (a 512-lane
  uint32_t* hist_part = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ws) + kHistPartOff);
  uint64_t* states = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(ws) + states_off(n_px));
  if (act) {                                   // main3 workgroup's upper half only syncs)
    for (int64_t i = int64_t(block) * kBlock + tid; i < n_state_words; i += int64_t(n_blocks) * kBlock)
      states[i] = 0;
    if (block == 0 && tid == 0) ws->lb_ticket = ws->lb_ticket_row = 0;

    // thread t owns packed word t (bins 2t, 2t+1 of [white 0..255 | clip 256..511])
    const int64_t per = (n_parts + n_blocks - 1) / n_blocks;
    const int64_t t0 = int64_t(block) * per, t1 = t0 + per < n_parts ? t0 + per : n_parts;
    uint32_t a0 = 0, a1 = 0;
    for (int64_t k0 = t0; k0 < t1; k0 += kPartsInFlight) {
      uint32_t v[kPartsInFlight];
#pragma unroll
      for (int j = 0; j < kPartsInFlight; ++j)
        v[j] = k0 + j < t1 ? pp[(k0 + j) * kPartWords + tid] : 0u;
#pragma unroll
      for (int j = 0; j < kPartsInFlight; ++j) { a0 += v[j] & 0xffffu; a1 += v[j] >> 16; }
    }
    uint32_t* dst = hist_part + (block % kHistCopies) * 512 + 2 * tid;
    if (a0) atomicAdd(dst, a0);
    if (a1) atomicAdd(dst + 1, a1);
  }

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (atomics only: see stats_kernel)
  __syncthreads();
  if (tid == 0) {
    const uint32_t t = __hip_atomic_fetch_add(&ws->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_last = (t == uint32_t(n_blocks) - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (!*s_last) return;
  if (act) sum_hist_copies(hist_part, tid, uint32_t(pad_zero), hg);
  __syncthreads();
  if (wave < 2) {                              // wave 0: white, wave 1: clip(w-b); concurrently
    const double thr = otsu_wave(hg + 256 * wave, n_px, reinterpret_cast<double*>(hg + 512) + wave * kOtsuLds);
    const int m = int_threshold(thr, wave == 0 ? 0 : -255);
    const int64_t above = hist_at_least_wave(hg + 256 * wave, m, n_px);
    if ((tid & 63) == 0) {
      if (wave == 0) { ws->smin = m; ws->thr_s = thr; } else { ws->cmin = m; ws->thr_c = thr; }
      ws->above[wave] = above;
      s_above[wave] = above;
    }
  }
  __syncthreads();
  if (tid == 0) arena_reserve(ws, s_above[0], s_above[1]);
  for (int i = tid; act && i < kHistCopies * 512; i += kBlock) hist_part[i] = 0;
  if (tid == 0) { ws->max_diff_enc = 0; ws->ticket = 0; }
}

}  // namespace
