// cloud_filter.hip -- device point-cloud cleanup for gfx950: radius and statistical outlier
// removal over a packed fp64 cloud (ProcessingLogic.remove_radius_outlier,
// server/processing.py:430-448, and ProcessingLogic.remove_outliers, :367-388), on the grid and
// the walks of cloud_grid.h.  The semantics are Open3D's PointCloud::RemoveRadiusOutliers /
// RemoveStatisticalOutliers as published, restated (parity with an installed Open3D
// is unpinned).  Each rule lives in exactly one __device__ function (d2_rule and
// radius_neighbour_rule in cloud_grid.h, the others below); tests/cloud_ref.py holds the same
// rules for NumPy.
#include "cloud_grid.h"

using namespace slgcloud;

namespace {

// ---------------------------------------------------------------- the rules (one place each)
__device__ inline bool radius_keep_rule(int32_t count, int32_t nb_points) { return count > nb_points; }
// Mean distance to the min(k, N) nearest (self included): sqrt of each d2, summed ascending, / kk.
__device__ inline double avg_rule(double sum_sqrt, int kk) { return sum_sqrt / (double)kk; }
__device__ inline bool stat_counts_rule(double avg) { return avg > 0.0; }
__device__ inline bool stat_keep_rule(double avg, double thr) { return avg > 0.0 && avg < thr; }

// ---------------------------------------------------------------- radius count
// One workgroup per occupied cell (grid-stride).  The cell's points are the queries, one per
// thread, 256 at a time, against the cell's 3x3x3 block (block_walk).  A wave none of whose lanes
// holds a query skips the inner loop.
__global__ __launch_bounds__(256)
void radius_count_kernel(const Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                         const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ustart, double r2,
                         int32_t nb_points, uint8_t* __restrict__ keep, int32_t* __restrict__ counts) {
  __shared__ double tile[3 * kTile];
  __shared__ uint32_t rng[9][2];
  const int t = threadIdx.x;
  cell_batches(hdr, ukeys, ustart, rng, [&](uint32_t qb, uint32_t qe) {
    const uint32_t q = qb + t;
    const bool active = q < qe;
    const bool wave_active = qb + (uint32_t)(t & ~63) < qe;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (active) { px = sxyz[3 * (size_t)q]; py = sxyz[3 * (size_t)q + 1]; pz = sxyz[3 * (size_t)q + 2]; }
    int32_t cnt = 0;
    block_walk<true>(rng, sxyz, tile, wave_active, px, py, pz, [](int, uint32_t) {},
                     [&](int, double d2) { cnt += radius_neighbour_rule(d2, r2) ? 1 : 0; });
    if (active) {
      const uint32_t o = sidx[q];
      keep[o] = radius_keep_rule(cnt, nb_points) ? 1 : 0;
      if (counts) counts[o] = cnt;
    }
  });
}

// ---------------------------------------------------------------- kNN
// One point per thread: the ring walk with the d2 list and no radius, then the ascending sum.
// Points still open after kMaxRing rings go to the list of knn_far_kernel.
__global__ __launch_bounds__(64)
void knn_kernel(Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ustart, int64_t n, int k,
                double* __restrict__ avg, uint32_t* __restrict__ far) {
  extern __shared__ double lds[];
  if (hdr->status) return;
  const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (q >= n) return;
  TopK tk{lds + threadIdx.x, (int)(n < k ? n : k), 0, 0, -1.0};
  if (!ring_walk<false>(hdr, sxyz, sidx, ukeys, ustart, q, 0.0, tk)) {
    far[atomicAdd(&hdr->n_far, 1)] = (uint32_t)q;      // list order is free: each entry is independent
    return;
  }
  tk.sort();
  double sum = 0.0;
  for (int j = 0; j < tk.cnt; ++j) sum += sqrt(tk.lst[j * 64]);
  avg[sidx[q]] = avg_rule(sum, tk.kk);
}

// One wave per listed point scans the whole cloud: each lane keeps the top-kk of its stride,
// sorts it, and the wave merges the 64 sorted lists by taking the smallest head kk times, which
// yields the distances in ascending order for the left-to-right sum.
__global__ __launch_bounds__(64)
void knn_far_kernel(const Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx, int64_t n,
                    int k, double* __restrict__ avg, const uint32_t* __restrict__ far) {
  extern __shared__ double lds[];
  if (hdr->status) return;
  const int lane = threadIdx.x;
  const int nf = hdr->n_far;
  const int kk = (int)(n < k ? n : k);
  for (int f = blockIdx.x; f < nf; f += gridDim.x) {
    const int64_t q = far[f];
    const double p[3] = {sxyz[3 * q], sxyz[3 * q + 1], sxyz[3 * q + 2]};
    TopK tk{lds + lane, kk, 0, 0, -1.0};
    scan_range<false>(tk, sxyz, sidx, lane, (uint32_t)n, 64, p, 0.0);
    tk.sort();
    int head = 0;
    double sum = 0.0;
    for (int r = 0; r < kk; ++r) {
      const double v = head < tk.cnt ? tk.lst[head * 64] : kInf;
      const double m = wave_min(v);
      const unsigned long long who = __ballot(v == m);
      if (lane == __ffsll((long long)who) - 1) ++head;
      sum += sqrt(m);
    }
    if (lane == 0) avg[sidx[q]] = avg_rule(sum, kk);
  }
}

// ---------------------------------------------------------------- statistics (fixed order)
// Σ term(avg[i]) over the input order as a fixed tree: 8 consecutive elements per thread, a
// binary tree over the workgroup's 256 threads, then (sum_final_kernel) thread t over partials
// t, t + 256, ... and the same tree.  No atomics: two runs give the same bits.
// MODE 0: term = avg (avg > 0).  MODE 1: term = (avg - mean)^2 (avg > 0).
template <int MODE>
__device__ inline double stat_term(double a, double mean) {
  if (!stat_counts_rule(a)) return 0.0;
  return MODE == 0 ? a : (a - mean) * (a - mean);
}

template <int MODE>
__global__ __launch_bounds__(256)
void sum_partial_kernel(const Hdr* hdr, const double* __restrict__ avg, int64_t n, double* __restrict__ part) {
  __shared__ double sm[256];
  if (hdr->status) return;
  const double mean = hdr->mean;
  const int64_t base = (int64_t)blockIdx.x * kChunk + threadIdx.x * (kChunk / 256);
  double s = 0.0;
  for (int j = 0; j < kChunk / 256; ++j)
    if (base + j < n) s += stat_term<MODE>(avg[base + j], mean);
  s = block_tree_sum(s, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// mean = Σ / N; std = sqrt(Σ (avg - mean)^2 / (N - 1)); thr = mean + std_ratio * std.
template <int MODE>
__global__ __launch_bounds__(256)
void sum_final_kernel(Hdr* hdr, const double* __restrict__ part, int nb, int64_t n, double std_ratio,
                      double* __restrict__ stats_out) {
  __shared__ double sm[256];
  if (hdr->status) return;
  double s = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) s += part[b];
  s = block_tree_sum(s, sm);
  if (threadIdx.x != 0) return;
  if (MODE == 0) {
    hdr->mean = s / (double)n;
  } else {
    hdr->std = sqrt(s / (double)(n - 1));
    hdr->thr = hdr->mean + std_ratio * hdr->std;
    if (stats_out) { stats_out[0] = hdr->mean; stats_out[1] = hdr->std; stats_out[2] = hdr->thr; }
  }
}

__global__ __launch_bounds__(256)
void stat_keep_kernel(const Hdr* hdr, const double* __restrict__ avg, int64_t n, uint8_t* __restrict__ keep) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) keep[i] = stat_keep_rule(avg[i], hdr->thr) ? 1 : 0;
}

}  // namespace

void slgcloud::radius_count(const Ws& w, int64_t n, double r2, int32_t nb_points, uint8_t* keep, int32_t* counts,
                            hipStream_t st) {
  radius_count_kernel<<<(int)(n < 8192 ? n : 8192), 256, 0, st>>>(w.hdr, w.sxyz, w.idx_s, w.ukeys, w.ustart, r2,
                                                                 nb_points, keep, counts);
}

extern "C" int32_t slg_radius_outlier(const double* xyz, int64_t n, double radius, int32_t nb_points, void* ws,
                                      int64_t ws_bytes, uint8_t* keep_out, int32_t* counts_out, void* stream) {
  if (n <= 0 || !(radius > 0.0) || !xyz || !keep_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_radius_outlier: n <= 0, radius <= 0 or a NULL buffer");
  Ws w;
  int rc = begin_call("slg_radius_outlier", n, ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // cell = radius, widened by 2^-20: a pair the rule counts has |dx| < radius (1 + 2^-50), so its
  // cell coordinates differ by less than 1 - 2^-20 + 2^-28 (the rounding of two coordinates below
  // 2^21) and the pair always shares a 3x3x3 block, also when points sit exactly on cell faces
  if ((rc = bbox(xyz, n, w, radius * (1.0 + 0x1p-20), 0, st))) return rc;
  if ((rc = build_grid(xyz, n, w, st))) return rc;
  radius_count(w, n, radius * radius, nb_points, keep_out, counts_out, st);
  return check_launch("radius_count_kernel");
}

extern "C" int32_t slg_statistical_outlier(const double* xyz, int64_t n, int32_t nb_neighbors, double std_ratio,
                                           void* ws, int64_t ws_bytes, uint8_t* keep_out, double* avg_out,
                                           double* stats_out, void* stream) {
  if (n <= 0 || nb_neighbors < 1 || !xyz || !keep_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_statistical_outlier: n <= 0, nb_neighbors < 1 or a NULL buffer");
  if (nb_neighbors > kMaxK)
    return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_statistical_outlier: nb_neighbors > %d", kMaxK);
  Ws w;
  int rc = begin_call("slg_statistical_outlier", n, ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int k = nb_neighbors;
  if ((rc = knn_grid(xyz, n, w, k, st))) return rc;
  double* avg = avg_out ? avg_out : w.avg;
  const size_t lds = (size_t)(n < k ? n : k) * 64 * sizeof(double);
  knn_kernel<<<grid_of(n, 64), 64, lds, st>>>(w.hdr, w.sxyz, w.idx_s, w.ukeys, w.ustart, n, k, avg, w.far);
  knn_far_kernel<<<(int)(n < 1024 ? n : 1024), 64, lds, st>>>(w.hdr, w.sxyz, w.idx_s, n, k, avg, w.far);
  const int nb = grid_of(n, kChunk);
  sum_partial_kernel<0><<<nb, 256, 0, st>>>(w.hdr, avg, n, w.part);
  sum_final_kernel<0><<<1, 256, 0, st>>>(w.hdr, w.part, nb, n, std_ratio, stats_out);
  sum_partial_kernel<1><<<nb, 256, 0, st>>>(w.hdr, avg, n, w.part);
  sum_final_kernel<1><<<1, 256, 0, st>>>(w.hdr, w.part, nb, n, std_ratio, stats_out);
  stat_keep_kernel<<<grid_of(n, 256), 256, 0, st>>>(w.hdr, avg, n, keep_out);
  return check_launch("slg_statistical_outlier");
}
