// stats.hip -- the mask thresholds of a view on MI355X (gfx950): histograms of white / black,
// Otsu as OpenCV or the NumPy percentile, by the device code of otsu.h.
//
// Kernels here
//   stats_kernel      white/black histograms (+ max contrast) -> last-arriving workgroup turns
//                     them into integer mask thresholds; also zeroes the compaction state of the
//                     next main launch.
//   parts_kernel, hist_thresholds_kernel  the same thresholds from per-tile partial histograms a
//                     fused launch carried, or from histograms summed over the ranks' bands.
// Host side: the batched launch code and the five stats entries of the C ABI; the fused unit
// calls slg_stats_batch and slg_stats_arm (internal.h).
#include <hip/hip_runtime.h>

#include "capture_checks.h"
#include "otsu.h"

#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------ stats kernel
constexpr int kMaxBatch = 16;               // views per batched stats launch (blockIdx.y)
constexpr int kStatsPx = 32;                // pixels per lane per stats iteration
constexpr int kStatsBlocks = 64;            // stats workgroups per view (at most), percentile path
#ifndef SLG_STATS_OTSU_BLOCKS
#define SLG_STATS_OTSU_BLOCKS 64                 // 128: 2.6% and 256: 10% slower bench (slot contention)
#endif
constexpr int kStatsBlocksOtsu = SLG_STATS_OTSU_BLOCKS;   // matrix-core Otsu path
#ifndef SLG_STATS_BLOCKS_ONE
#define SLG_STATS_BLOCKS_ONE 256   // r3ao: 64 -> 51.7, 128 -> 42.2, 256 -> 40.0, 512 -> 39.9 us (1080p, Otsu)
#endif
constexpr int kStatsBlocksOne = SLG_STATS_BLOCKS_ONE;   // one-view launches (nothing runs beside them)
#ifndef SLG_OTSU_ONE_CHUNKS
#define SLG_OTSU_ONE_CHUNKS 2
#endif
constexpr int kOtsuOneChunks = SLG_OTSU_ONE_CHUNKS;

struct StatsParams {
  const uint8_t* white[kMaxBatch];
  const uint8_t* black[kMaxBatch];
  WsHeader* wsv[kMaxBatch];
  int64_t n_px;
  int64_t n_state_words;   // look-back words zeroed here for the next main launch
  int32_t thresh_mode;
  int32_t pad;
  double shadow_val;
  double contrast_val;
  int32_t pad2[2];
  const uint32_t* parts[kMaxBatch];   // parts_kernel: per-tile partial histograms of each view
  int64_t n_parts;                    // tiles per view
  int64_t pad_zero;                   // zero pixels counted past n_px (removed from bin 0)
  uint32_t* hist_out;                 // one view, histograms only (slg_decode_histograms): no thresholds
};

#ifndef SLG_STATS_MINB
#define SLG_STATS_MINB 1     // stats_kernel workgroups per CU its registers are budgeted for
#endif

__global__ __launch_bounds__(kBlock, SLG_STATS_MINB) void stats_kernel(StatsParams p) {
  // 16 sub-histograms per kind (wave x lane&3), rows padded to 257 words so the copies of one
  // bin sit in different banks: a flat background costs at most 16-way same-address adds.
  constexpr int kRow = 257;
  __shared__ __attribute__((aligned(16))) uint32_t sh[16 * 2 * kRow];
  static_assert(512 * 4 + 2 * kOtsuLds * 8 <= 16 * 2 * kRow * 4, "Otsu tail: histograms + two waves' LDS");
  __shared__ uint32_t s_maxd;
  __shared__ uint32_t s_last;
  __shared__ int64_t s_above[2];
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int view = blockIdx.y;               // batched launches: one grid row per view
  WsHeader* ws = p.wsv[view];
  const uint8_t* white = p.white[view];
  const uint8_t* black = p.black[view];
  uint32_t* hist_part = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ws) + kHistPartOff);
  uint64_t* states = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(ws) + states_off(p.n_px));

  // Arm the compaction state of the following main launch (ordered by the kernel boundary).
  for (int64_t i = int64_t(blockIdx.x) * kBlock + tid; i < p.n_state_words; i += int64_t(gridDim.x) * kBlock)
    states[i] = 0;
  if (blockIdx.x == 0 && tid == 0) ws->lb_ticket = ws->lb_ticket_row = 0;

  if (p.thresh_mode == SLG_THRESH_MANUAL) {
    if (blockIdx.x == 0 && tid < 2) {
      const double thr = tid == 0 ? p.shadow_val : p.contrast_val;
      const int m = int_threshold(thr, tid == 0 ? 0 : -255);
      if (tid == 0) { ws->smin = m; ws->thr_s = thr; } else { ws->cmin = m; ws->thr_c = thr; }
      ws->above[tid] = p.n_px;                 // manual thresholds: no histogram, no bound
    }
    if (blockIdx.x == 0 && tid == 0) arena_reserve(ws, p.n_px, p.n_px);
    return;
  }

  for (int i = tid; i < 16 * 2 * kRow; i += kBlock) sh[i] = 0;
  if (tid == 0) s_maxd = 0;
  __syncthreads();

  // hist kinds: otsu -> [0] white, [1] clip(white-black); percentile -> [0] black.
  const bool otsu = p.thresh_mode == SLG_THRESH_OTSU;
  if (otsu) {                                  // matrix-core histograms (hist_chunk_dpp)
    v4i32 acc_w = {0, 0, 0, 0}, acc_d = {0, 0, 0, 0};
    const int lane = tid & 63;
    const int64_t step = int64_t(gridDim.x) * (kBlock / 64) * kHistChunk;
    int64_t c = (int64_t(blockIdx.x) * (kBlock / 64) + wave) * kHistChunk;
    uint32_t w[4], d[4];
    if (c < p.n_px) hist_load(white, black, c, p.n_px, w, d);
    for (; c < p.n_px; c += step) {            // next chunk's loads in flight during the MFMAs
      uint32_t wn[4], dn[4];
      const bool more = c + step < p.n_px;
      if (more) hist_load(white, black, c + step, p.n_px, wn, dn);
      hist_chunk_dpp(w, d, acc_w, acc_d);
      if (more) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { w[q] = wn[q]; d[q] = dn[q]; }
      }
    }
    acc_w = hist_from_cumulative(acc_w);
    acc_d = hist_from_cumulative(acc_d);
#pragma unroll
    for (int r = 0; r < 4; ++r) {              // wave sub-histograms: row-major bins 16*row + col
      const int bin = 16 * (4 * (lane >> 4) + r) + (lane & 15);
      if (acc_w[r]) atomicAdd(&sh[(2 * wave) * kRow + bin], uint32_t(acc_w[r]) >> 8);
      if (acc_d[r]) atomicAdd(&sh[(2 * wave + 1) * kRow + bin], uint32_t(acc_d[r]) >> 8);
    }
  }
  // percentile: LDS adds into 16 sub-histograms, kStatsPx consecutive pixels per lane and step
  uint32_t local_max = 0;
  if (!otsu) {
    uint32_t* h0 = sh + (4 * wave + (tid & 3)) * 2 * kRow;
    const int64_t per_block = int64_t(kBlock) * kStatsPx;
    for (int64_t b0 = int64_t(blockIdx.x) * per_block; b0 < p.n_px; b0 += int64_t(gridDim.x) * per_block) {
      const int64_t px0 = b0 + int64_t(tid) * kStatsPx;
      uint2 w[kStatsPx / 8], b[kStatsPx / 8];
#pragma unroll
      for (int q = 0; q < kStatsPx / 8; ++q) {
        const int64_t o = px0 + 8 * q < p.n_px ? px0 + 8 * q : 0;   // frames readable to round_up(n, 8)
        w[q] = *reinterpret_cast<const uint2*>(white + o);
        b[q] = *reinterpret_cast<const uint2*>(black + o);
      }
      // (a guard, not a break: with the break the loop stayed rolled and w[] / b[] went to
      // scratch, indexed at run time)
#pragma unroll
      for (int k = 0; k < kStatsPx; ++k) {
        if (px0 + k < p.n_px) {
          const uint2 wq = w[k >> 3], bq = b[k >> 3];
          const int wv = (((k & 7) < 4 ? wq.x : wq.y) >> (8 * (k & 3))) & 0xff;
          const int bv = (((k & 7) < 4 ? bq.x : bq.y) >> (8 * (k & 3))) & 0xff;
          atomicAdd(&h0[bv], 1u);
          local_max = max(local_max, uint32_t(wv - bv + 256));
        }
      }
    }
  }
  if (!otsu) atomicMax(&s_maxd, local_max);
  __syncthreads();
  for (int i = tid; i < 2 * 256; i += kBlock) {
    const int kind = i >> 8, bin = i & 255;
    uint32_t v = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) v += sh[(2 * c + kind) * kRow + bin];
    if (v) atomicAdd(hist_part + (blockIdx.x % kHistCopies) * 512 + i, v);
  }
  if (!otsu && tid == 0 && s_maxd) atomicMax(&ws->max_diff_enc, s_maxd);

  // Publish (every wave drains its atomics, barrier) then take a ticket.  Hardware assumption
  // (no release / acquire fences): what the last arriver reads -- the histogram copies,
  // max_diff_enc -- is written and read by agent-scope atomics only, which gfx950 performs at
  // the L2 that owns the address (the device's point of coherence for agent scope, whichever
  // XCD issues them); a returned vmcnt means the add has been performed there, so a ticket
  // taken after vmcnt(0) orders every earlier add before the last arriver's atomic loads.  No
  // L2 write-back or invalidate is needed (an agent-scope fence is one of each, per workgroup).
  // tests/test_gpu_configs.py::test_concurrent_stats_thresholds checks the thresholds of many
  // concurrent multi-view launches against the oracle.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const uint32_t t = __hip_atomic_fetch_add(&ws->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (t == gridDim.x - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;

  // Last arriver: read the global histograms, compute thresholds, reset for reuse.
  uint32_t* hg = sh;                           // reuse the sub-histograms for the global ones
  sum_hist_copies(hist_part, tid, otsu ? uint32_t(p.pad_zero) : 0u, hg);
  if (tid == 0) s_maxd = __hip_atomic_load(&ws->max_diff_enc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (p.hist_out) {                            // histograms only: a band of a view split over ranks
    for (int i = tid; i < 512; i += kBlock) p.hist_out[i] = hg[i];
    if (tid == 0) p.hist_out[512] = s_maxd;
  } else {
    set_thresholds(hg, s_maxd, p.n_px, otsu, ws, reinterpret_cast<double*>(sh + 512), s_above);
  }
  for (int i = tid; i < kHistCopies * 512; i += kBlock) hist_part[i] = 0;
  if (tid == 0) { ws->max_diff_enc = 0; ws->ticket = 0; }
}

// Thresholds of a view whose histograms were summed over the bands of rows the ranks hold
// (slg_thresholds_from_histograms; SURVEY 8(e), the one exchange step of a single-view split):
// block 0 runs set_thresholds on hist[513] (as slg_decode_histograms wrote it, summed), every
// block zeroes this band's look-back words for the following fused launch (kernel boundary).
__global__ __launch_bounds__(kBlock) void hist_thresholds_kernel(const uint32_t* hist, WsHeader* ws, int64_t n_px,
                                                                 int32_t thresh_mode, int64_t n_state_words) {
  __shared__ __attribute__((aligned(16))) uint32_t hg[512 + 4 * kOtsuLds];
  __shared__ int64_t s_above[2];
  const int tid = threadIdx.x;
  uint64_t* states = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(ws) + states_off(0));
  for (int64_t i = int64_t(blockIdx.x) * kBlock + tid; i < n_state_words; i += int64_t(gridDim.x) * kBlock)
    states[i] = 0;
  if (blockIdx.x != 0) return;
  if (tid == 0) ws->lb_ticket = ws->lb_ticket_row = 0;
  for (int i = tid; i < 512; i += kBlock) hg[i] = hist[i];
  __syncthreads();
  set_thresholds(hg, hist[512], n_px, thresh_mode == SLG_THRESH_OTSU, ws, reinterpret_cast<double*>(hg + 512), s_above);
}

__global__ __launch_bounds__(kBlock) void parts_kernel(StatsParams p) {
  __shared__ __attribute__((aligned(16))) uint32_t hg[kPartsLdsWords];   // + the Otsu tail's LDS
  __shared__ uint32_t s_last;
  otsu_from_parts(p.parts[blockIdx.y], p.wsv[blockIdx.y], p.n_parts, p.n_px, p.n_state_words, p.pad_zero,
                  int(blockIdx.x), int(gridDim.x), hg, &s_last);
}

// One stats launch for n_views views (<= kMaxBatch) of one geometry; view v reads white/black
// from whites[v] / blacks[v] and owns the workspace slice at workspace + v * ws_stride.
// from_parts: Otsu from the per-tile partial histograms in each slice (written by a fused
// launch's next-batch pass) instead of from white/black frames.
int stats_launch_batch(const uint8_t* const* whites, const uint8_t* const* blacks, int n_views, int64_t n_px,
                       const slg_decode_params* dp, char* workspace, int64_t ws_stride, hipStream_t s,
                       bool from_parts = false, uint32_t* hist_out = nullptr) {
  StatsParams sp{};
  sp.hist_out = hist_out;
  for (int v = 0; v < n_views; ++v) {
    sp.white[v] = whites ? whites[v] : nullptr;
    sp.black[v] = blacks ? blacks[v] : nullptr;
    sp.wsv[v] = reinterpret_cast<WsHeader*>(workspace + int64_t(v) * ws_stride);
    if (from_parts) sp.parts[v] = reinterpret_cast<const uint32_t*>(workspace + int64_t(v) * ws_stride + parts_off(n_px));
  }
  sp.n_parts = n_tiles_of(n_px);
  sp.pad_zero = from_parts ? sp.n_parts * kTilePx - n_px : align_up(n_px, kHistChunk) - n_px;
  sp.n_px = n_px;
  sp.n_state_words = n_state_words(n_px);
  sp.thresh_mode = dp ? dp->thresh_mode : SLG_THRESH_MANUAL;
  sp.shadow_val = dp ? dp->shadow_val : 0.0;
  sp.contrast_val = dp ? dp->contrast_val : 0.0;
  // Few fat workgroups per view: each merges its sub-histograms into the view's histogram with
  // <= 512 global atomics, and a batch's stats pass takes few CU slots next to a fused launch.
  // One-view Otsu launches: kOtsuOneChunks MFMA chunks per wave.
  const bool otsu_one = n_views == 1 && sp.thresh_mode == SLG_THRESH_OTSU;
  const int64_t px_per_block = otsu_one ? int64_t(kBlock / 64) * kHistChunk * kOtsuOneChunks : int64_t(kBlock) * kStatsPx;
  int64_t grid = (n_px + px_per_block - 1) / px_per_block;
  const int64_t cap = otsu_one ? 4 * kStatsBlocksOne : n_views == 1 ? kStatsBlocksOne
                    : sp.thresh_mode == SLG_THRESH_OTSU ? kStatsBlocksOtsu : kStatsBlocks;
  if (grid > cap) grid = cap;
  if (sp.thresh_mode == SLG_THRESH_OTSU) {   // bound chunks per wave (i32 MFMA accumulators)
    const int64_t per_block = int64_t(kBlock / 64) * kHistChunk * kHistMaxChunks;
    const int64_t need = (n_px + per_block - 1) / per_block;
    if (grid < need) grid = need;
  }
  if (from_parts) {   // ~2 x kPartsInFlight tiles per workgroup: one or two rounds of loads
    grid = (sp.n_parts + 2 * kPartsInFlight - 1) / (2 * kPartsInFlight);
    grid = grid < 1 ? 1 : (grid > kPartsBlocksMax ? kPartsBlocksMax : grid);
    hipLaunchKernelGGL(parts_kernel, dim3(unsigned(grid), unsigned(n_views)), dim3(kBlock), 0, s, sp);
    return check_launch("parts_kernel");
  }
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(stats_kernel, dim3(unsigned(grid), unsigned(n_views)), dim3(kBlock), 0, s, sp);
  return check_launch("stats_kernel");
}

int stats_launch(const uint8_t* white, const uint8_t* black, int64_t n_px, const slg_decode_params* dp,
                 void* workspace, hipStream_t s) {
  return stats_launch_batch(&white, &black, 1, n_px, dp, static_cast<char*>(workspace), 0, s);
}

// The checks slg_decode_stats and slg_decode_histograms share, in their order: the capture, the
// NULL arguments (`others`: the entry's further pointers are set), the frame count.
int check_one_view(const slg_capture* cap, const slg_decode_params* dp, const void* workspace, bool others = true) {
  if (const int rc = check_capture(cap)) return rc;
  if (!dp || !workspace || !others) return fail(SLG_ERR_INVALID, "NULL argument");
  return check_enough_frames(cap);
}

}  // namespace

// Stats of n_views views (one launch per kMaxBatch views).
int slg_stats_batch(const slg_capture* caps, int n_views, const slg_decode_params* dp, char* ws, int64_t ws_stride,
                    hipStream_t s) {
  if (!caps || n_views < 1 || !dp || !ws) return fail(SLG_ERR_INVALID, "NULL argument");
  if (dp->thresh_mode < 0 || dp->thresh_mode > 2) return fail(SLG_ERR_INVALID, "bad thresh_mode");
  for (int v = 0; v < n_views; ++v) {
    int rc = check_capture(&caps[v]);
    if (!rc) rc = check_enough_frames(&caps[v]);
    if (rc) return rc;
    if ((rc = check_same_geometry(caps[v], caps[0], kBatchGeometry))) return rc;
  }
  const int64_t n_px = int64_t(caps[0].height) * caps[0].width;
  if (const int rc = check_ws_stride(n_views > 1, ws_stride, n_px)) return rc;
  for (int v0 = 0; v0 < n_views; v0 += kMaxBatch) {
    const int nb = n_views - v0 < kMaxBatch ? n_views - v0 : kMaxBatch;
    const uint8_t* wh[kMaxBatch];
    const uint8_t* bl[kMaxBatch];
    for (int v = 0; v < nb; ++v) {
      wh[v] = caps[v0 + v].frames;
      bl[v] = caps[v0 + v].frames + caps[v0 + v].frame_stride;
    }
    const int rc = stats_launch_batch(wh, bl, nb, n_px, dp, ws + int64_t(v0) * ws_stride, ws_stride, s);
    if (rc) return rc;
  }
  return SLG_OK;
}

int slg_stats_arm(int64_t n_px, void* workspace, hipStream_t s) {
  return stats_launch(nullptr, nullptr, n_px, nullptr, workspace, s);   // manual mode: arms states only
}

extern "C" {

int32_t slg_decode_stats(const slg_capture* cap, const slg_decode_params* dp, void* workspace, void* stream) {
  if (const int rc = check_one_view(cap, dp, workspace)) return rc;
  if (dp->thresh_mode < 0 || dp->thresh_mode > 2) return fail(SLG_ERR_INVALID, "bad thresh_mode");
  const int64_t n_px = int64_t(cap->height) * cap->width;
  return stats_launch(cap->frames, cap->frames + cap->frame_stride, n_px, dp, workspace,
                      static_cast<hipStream_t>(stream));
}

int32_t slg_decode_histograms(const slg_capture* cap, const slg_decode_params* dp, void* workspace,
                              uint32_t* hist_out, void* stream) {
  if (const int rc = check_one_view(cap, dp, workspace, hist_out != nullptr)) return rc;
  if (dp->thresh_mode != SLG_THRESH_OTSU && dp->thresh_mode != SLG_THRESH_PERCENTILE)
    return fail(SLG_ERR_INVALID, "histograms serve Otsu / percentile thresholds (manual ones need none)");
  if (reinterpret_cast<uintptr_t>(hist_out) & 3) return fail(SLG_ERR_INVALID, "hist_out must be 4-byte aligned");
  const int64_t n_px = int64_t(cap->height) * cap->width;
  const uint8_t* white = cap->frames;
  const uint8_t* black = cap->frames + cap->frame_stride;
  return stats_launch_batch(&white, &black, 1, n_px, dp, static_cast<char*>(workspace), 0,
                            static_cast<hipStream_t>(stream), false, hist_out);
}

int32_t slg_thresholds_from_histograms(const uint32_t* hist, int64_t n_pixels, const slg_decode_params* dp,
                                       void* workspace, int64_t n_band_pixels, void* stream) {
  if (!hist || !dp || !workspace) return fail(SLG_ERR_INVALID, "NULL argument");
  if (n_pixels < 1 || n_band_pixels < 1 || n_band_pixels > n_pixels || n_pixels >= (int64_t(1) << 31))
    return fail(SLG_ERR_INVALID, "need 1 <= n_band_pixels <= n_pixels < 2^31");
  if (dp->thresh_mode != SLG_THRESH_OTSU && dp->thresh_mode != SLG_THRESH_PERCENTILE)
    return fail(SLG_ERR_INVALID, "histograms serve Otsu / percentile thresholds (manual ones need none)");
  if (reinterpret_cast<uintptr_t>(hist) & 3) return fail(SLG_ERR_INVALID, "hist must be 4-byte aligned");
  const int64_t nsw = n_state_words(n_band_pixels);
  int64_t grid = (nsw + kBlock - 1) / kBlock;
  grid = grid < 1 ? 1 : (grid > 64 ? 64 : grid);
  hipLaunchKernelGGL(hist_thresholds_kernel, dim3(unsigned(grid)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                     hist, reinterpret_cast<WsHeader*>(workspace), n_pixels, dp->thresh_mode, nsw);
  return check_launch("hist_thresholds_kernel");
}

int32_t slg_decode_stats_batch(const slg_capture* caps, int32_t n_views, const slg_decode_params* dp,
                               void* workspace, int64_t ws_stride, void* stream) {
  return slg_stats_batch(caps, n_views, dp, static_cast<char*>(workspace), ws_stride, static_cast<hipStream_t>(stream));
}

int32_t slg_decode_stats_partials_batch(int32_t n_views, int32_t height, int32_t width, const slg_decode_params* dp,
                                        void* workspace, int64_t ws_stride, void* stream) {
  if (n_views < 1 || !dp || !workspace || height < 1 || width < 1) return fail(SLG_ERR_INVALID, "bad argument");
  if (dp->thresh_mode != SLG_THRESH_OTSU) return fail(SLG_ERR_UNSUPPORTED, "partial histograms are Otsu only");
  const int64_t n_px = int64_t(height) * width;
  if (const int rc = check_ws_stride(n_views > 1, ws_stride, n_px)) return rc;
  char* ws = static_cast<char*>(workspace);
  for (int v0 = 0; v0 < n_views; v0 += kMaxBatch) {
    const int nb = n_views - v0 < kMaxBatch ? n_views - v0 : kMaxBatch;
    const int rc = stats_launch_batch(nullptr, nullptr, nb, n_px, dp, ws + int64_t(v0) * ws_stride, ws_stride,
                                      static_cast<hipStream_t>(stream), true);
    if (rc) return rc;
  }
  return SLG_OK;
}

}  // extern "C"
