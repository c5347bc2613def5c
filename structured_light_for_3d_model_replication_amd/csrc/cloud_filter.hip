// cloud_filter.hip — device point-cloud cleanup for gfx950: radius and statistical outlier
// removal and DBSCAN clustering over a packed fp64 cloud, and the order-preserving select that
// follows them (ProcessingLogic.remove_radius_outlier, server/processing.py:430-448,
// ProcessingLogic.remove_outliers, :367-388, and ProcessingLogic.keep_largest_cluster, :391-427).
//
// The semantics are Open3D's PointCloud::RemoveRadiusOutliers / RemoveStatisticalOutliers as
// published, restated (parity with an installed Open3D is unpinned).  Each rule
// lives in exactly one __device__ function below (d2_rule, radius_keep_rule, avg_rule,
// stat_threshold_rule, stat_keep_rule); tests/cloud_ref.py holds the same rules for NumPy.
//
// The same grid carries the voxel down-sample (a per-voxel ordered reduction) and the normal
// estimation (the kNN walk with the neighbours' indices kept), with the orientation and the
// centroid beside them: the Open3D steps of the merge tail and of the front of both meshing
// methods (server/processing.py:605-628, :653-670, :804-837; rules in DESIGN.md §10 and
// tests/normals_ref.py).
//
// All of them share one structure, a sparse uniform grid:
//   bbox (fixed-order reduction) -> integer cell coordinates floor((p - min) / cell) packed into
//   a 63-bit key (21 bits per axis, x lowest) -> stable radix sort of (key, index) -> points
//   gathered in sorted order -> table of unique keys + start offsets (binary search).
// x is the lowest key field, so the cells x0..x1 of one (y, z) row are one contiguous range of
// the sorted cloud: a 3x3x3 neighbourhood is 9 ranges.  No dense cell array exists, so far
// outliers (row_mode 2 clouds) cost nothing.
//
// Everything is separate launches on the caller's stream; no workgroup waits for another and
// nothing synchronises with the host.  Conditions only the device can see (a non-finite
// coordinate, an axis of 2^21 cells or more) set a status word at the front of the workspace;
// every later kernel of the call reads it and returns, so a bad input ends in the flag.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <string.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "internal.h"

namespace {

constexpr int kCellBits = 21;
constexpr int64_t kCellMax = (1ll << kCellBits) - 1;
constexpr int kMaxK = 64;
constexpr int kTile = 1024;        // candidate points staged in LDS per tile (24 KB)
constexpr int kChunk = 2048;       // points per workgroup in the fixed-order reductions
constexpr int kMaxRing = 6;        // Chebyshev rings the kNN walk takes before the whole-cloud kernel
constexpr double kInf = __builtin_huge_val();

// ---------------------------------------------------------------- the rules (one place each)
// Squared distance: the same expression, in the same order, as tests/cloud_ref.py:d2.
__device__ inline double d2_rule(double dx, double dy, double dz) { return (dx * dx + dy * dy) + dz * dz; }
// A neighbour counts when d2 < radius^2 (strict); the point itself counts.
__device__ inline bool radius_neighbour_rule(double d2, double r2) { return d2 < r2; }
__device__ inline bool radius_keep_rule(int32_t count, int32_t nb_points) { return count > nb_points; }
// DBSCAN: a point is core when its radius count (itself included) reaches min_points.
__device__ inline bool core_rule(int32_t count, int32_t min_points) { return count >= min_points; }
// Mean distance to the min(k, N) nearest (self included): sqrt of each d2, summed ascending, / kk.
__device__ inline double avg_rule(double sum_sqrt, int kk) { return sum_sqrt / (double)kk; }
__device__ inline bool stat_counts_rule(double avg) { return avg > 0.0; }
__device__ inline bool stat_keep_rule(double avg, double thr) { return avg > 0.0 && avg < thr; }

// ---------------------------------------------------------------- workspace
struct Hdr {            // 256 bytes at the front of the workspace
  int32_t status;       // SLG_FILTER_BAD_* bits
  int32_t n_unique;
  int32_t n_far;
  int32_t pad;
  double mn[3], mx[3];
  double cell;
  double slack;         // absolute rounding allowance on a face distance
  int32_t cmax[3];
  int32_t pad2;
  double mean, std, thr;
  int32_t n_clusters;   // slg_dbscan
  int32_t n_noise;
  unsigned long long best;   // (member count << 32) | ~label, by atomicMax: the lowest label wins a tie
};
static_assert(sizeof(Hdr) <= 256, "header");

struct Layout {
  size_t keys, keys_s, idx, idx_s, sxyz, pos, ukeys, ustart, part, avg, far, temp, temp_bytes, total;
};

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct U8ToU32 {
  __host__ __device__ uint32_t operator()(uint8_t v) const { return v ? 1u : 0u; }
};

hipError_t temp_bytes_for(int64_t n, size_t* out) {
  size_t a = 0, b = 0, c = 0;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                           (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0u, 63u,
                                           (hipStream_t)0);
  if (e != hipSuccess) return e;
  e = rocprim::exclusive_scan(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n,
                              rocprim::plus<uint32_t>(), (hipStream_t)0);
  if (e != hipSuccess) return e;
  auto it = rocprim::make_transform_iterator((const uint8_t*)nullptr, U8ToU32());
  e = rocprim::exclusive_scan(nullptr, c, it, (uint32_t*)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>(),
                              (hipStream_t)0);
  if (e != hipSuccess) return e;
  *out = a > b ? (a > c ? a : c) : (b > c ? b : c);
  return hipSuccess;
}

Layout make_layout(int64_t n, size_t temp_bytes) {
  Layout L;
  size_t o = 256;
  const size_t N = (size_t)n;
  L.keys = o;   o = up256(o + N * 8);
  L.keys_s = o; o = up256(o + N * 8);
  L.idx = o;    o = up256(o + N * 4);
  L.idx_s = o;  o = up256(o + N * 4);
  L.sxyz = o;   o = up256(o + N * 24);
  L.pos = o;    o = up256(o + N * 4);
  L.ukeys = o;  o = up256(o + N * 8);
  L.ustart = o; o = up256(o + (N + 1) * 4);
  L.part = o;   o = up256(o + ((N + kChunk - 1) / kChunk) * 6 * 8);
  L.avg = o;    o = up256(o + N * 8);
  L.far = o;    o = up256(o + N * 4);
  L.temp = o;   o = up256(o + temp_bytes);
  L.temp_bytes = temp_bytes;
  L.total = o;
  return L;
}

// ---------------------------------------------------------------- grid helpers
__device__ inline int64_t cell_coord(double p, double mn, double cell) {
  const double c = floor((p - mn) / cell);
  if (!(c > 0.0)) return 0;                 // also NaN
  return c > (double)kCellMax ? kCellMax : (int64_t)c;
}
__device__ inline uint64_t pack_key(int64_t x, int64_t y, int64_t z) {
  return ((uint64_t)z << (2 * kCellBits)) | ((uint64_t)y << kCellBits) | (uint64_t)x;
}
// First table entry with key >= k (nu when none).
__device__ inline int lower_bound(const uint64_t* __restrict__ a, int nu, uint64_t k) {
  int lo = 0, hi = nu;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// Sorted-cloud range [s, e) of the cells x0..x1 of row (y, z).
__device__ inline void row_range(const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ustart, int nu,
                                 int64_t x0, int64_t x1, int64_t y, int64_t z, uint32_t* s, uint32_t* e) {
  const int u0 = lower_bound(ukeys, nu, pack_key(x0, y, z));
  const int u1 = lower_bound(ukeys, nu, pack_key(x1, y, z) + 1);
  *s = ustart[u0];                           // ustart[nu] = n
  *e = ustart[u1];
}

// ---------------------------------------------------------------- bounding box (fixed order)
__global__ __launch_bounds__(256) void bbox_partial_kernel(const double* __restrict__ xyz, int64_t n, Hdr* hdr,
                                                           double* __restrict__ part) {
  __shared__ double sm[6][256];
  const int t = threadIdx.x;
  double lo[3] = {kInf, kInf, kInf}, hi[3] = {-kInf, -kInf, -kInf};
  bool bad = false;
  const int64_t base = (int64_t)blockIdx.x * kChunk;
  for (int j = 0; j < kChunk / 256; ++j) {
    const int64_t i = base + j * 256 + t;
    if (i < n) {
      for (int a = 0; a < 3; ++a) {
        const double v = xyz[3 * i + a];
        if (!isfinite(v)) bad = true;
        lo[a] = fmin(lo[a], v);
        hi[a] = fmax(hi[a], v);
      }
    }
  }
  if (bad) atomicOr(&hdr->status, SLG_FILTER_BAD_NONFINITE);
  for (int a = 0; a < 3; ++a) { sm[a][t] = lo[a]; sm[3 + a][t] = hi[a]; }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s)
      for (int a = 0; a < 3; ++a) {
        sm[a][t] = fmin(sm[a][t], sm[a][t + s]);
        sm[3 + a][t] = fmax(sm[3 + a][t], sm[3 + a][t + s]);
      }
    __syncthreads();
  }
  if (t < 6) part[(int64_t)blockIdx.x * 6 + t] = sm[t][0];
}

__device__ inline void set_cell(Hdr* hdr, double cell) {
  hdr->cell = cell;
  for (int a = 0; a < 3; ++a) hdr->cmax[a] = (int32_t)cell_coord(hdr->mx[a], hdr->mn[a], cell);
}

// Points per occupied cell the kNN grid aims for: the k nearest then lie within about one cell
// size, so the walk usually ends after ring 1.
__device__ inline double knn_target(int k) { return fmax(2.0, (double)k / 4.0); }

// One workgroup: folds the partial boxes, then fixes the cell size.  cell_in > 0: the radius
// filter's cell (= radius), and an axis of 2^21 cells or more is flagged.  cell_in <= 0: the kNN
// grid's first guess from the box alone; knn_refine_kernel corrects it from the occupancy.
__global__ __launch_bounds__(256) void bbox_final_kernel(const double* __restrict__ part, int nb, Hdr* hdr,
                                                         double cell_in, int64_t n, int k) {
  __shared__ double sm[6][256];
  const int t = threadIdx.x;
  double lo[3] = {kInf, kInf, kInf}, hi[3] = {-kInf, -kInf, -kInf};
  for (int b = t; b < nb; b += 256)
    for (int a = 0; a < 3; ++a) {
      lo[a] = fmin(lo[a], part[(int64_t)b * 6 + a]);
      hi[a] = fmax(hi[a], part[(int64_t)b * 6 + 3 + a]);
    }
  for (int a = 0; a < 3; ++a) { sm[a][t] = lo[a]; sm[3 + a][t] = hi[a]; }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s)
      for (int a = 0; a < 3; ++a) {
        sm[a][t] = fmin(sm[a][t], sm[a][t + s]);
        sm[3 + a][t] = fmax(sm[3 + a][t], sm[3 + a][t + s]);
      }
    __syncthreads();
  }
  if (t != 0 || hdr->status) return;
  double ext = 0.0, mag = 0.0;
  for (int a = 0; a < 3; ++a) {
    hdr->mn[a] = sm[a][0];
    hdr->mx[a] = sm[3 + a][0];
    ext = fmax(ext, sm[3 + a][0] - sm[a][0]);
    mag = fmax(mag, fmax(fabs(sm[a][0]), fabs(sm[3 + a][0])));
  }
  if (!isfinite(ext)) { atomicOr(&hdr->status, SLG_FILTER_BAD_EXTENT); return; }   // max - min overflowed
  hdr->slack = 0x1p-49 * fmax(mag, ext);
  if (cell_in > 0.0) {
    if (ext / cell_in >= (double)(kCellMax + 1)) { atomicOr(&hdr->status, SLG_FILTER_BAD_EXTENT); return; }
    set_cell(hdr, cell_in);
  } else {
    // a surface filling the box's largest face would put knn_target(k) points in a cell of this size
    double e[3] = {sm[3][0] - sm[0][0], sm[4][0] - sm[1][0], sm[5][0] - sm[2][0]};
    const double smallest = fmin(e[0], fmin(e[1], e[2]));
    const double area = smallest > 0.0 ? e[0] * e[1] * e[2] / smallest : fmax(e[0] * e[1], fmax(e[0] * e[2], e[1] * e[2]));
    double cell = sqrt(area * knn_target(k) / (double)n);
    if (!(cell > 0.0) || !isfinite(cell)) cell = ext > 0.0 ? ext / 1024.0 : 1.0;
    set_cell(hdr, fmax(cell, ext / (double)(1 << 20)));
  }
}

// kNN cell from occupancy: with o = N / (occupied cells) points per occupied cell and a cloud that
// is a surface (o ~ cell^2), rescale the cell so that an occupied cell holds about knn_target(k)
// points (far outliers inflate the box, so the first guess can be far too large); a factor of two
// either way is left alone; never below extent / 2^20 cells per axis.  Run between grid builds.
__global__ void knn_refine_kernel(Hdr* hdr, int64_t n, int k) {
  if (hdr->status || hdr->n_unique <= 0) return;
  const double target = knn_target(k);
  const double occ = (double)n / (double)hdr->n_unique;
  if (occ <= 2.0 * target && occ >= 0.5 * target) return;
  double ext = 0.0;
  for (int a = 0; a < 3; ++a) ext = fmax(ext, hdr->mx[a] - hdr->mn[a]);
  if (!(ext > 0.0)) return;
  double cell = hdr->cell * fmin(fmax(sqrt(target / occ), 1.0 / 64.0), 4.0);
  set_cell(hdr, fmax(cell, ext / (double)(1 << 20)));
}

// ---------------------------------------------------------------- grid build
__global__ __launch_bounds__(256) void keys_kernel(const double* __restrict__ xyz, int64_t n, const Hdr* hdr,
                                                   uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double cell = hdr->cell;
  keys[i] = pack_key(cell_coord(xyz[3 * i], hdr->mn[0], cell), cell_coord(xyz[3 * i + 1], hdr->mn[1], cell),
                     cell_coord(xyz[3 * i + 2], hdr->mn[2], cell));
  idx[i] = (uint32_t)i;
}

// Sorted copy of the points, and the run-start flags of the sorted keys.
__global__ __launch_bounds__(256) void gather_flags_kernel(const double* __restrict__ xyz, int64_t n, const Hdr* hdr,
                                                           const uint64_t* __restrict__ keys_s,
                                                           const uint32_t* __restrict__ idx_s,
                                                           double* __restrict__ sxyz, uint32_t* __restrict__ flags) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t src = idx_s[i];
  sxyz[3 * i] = xyz[3 * src];
  sxyz[3 * i + 1] = xyz[3 * src + 1];
  sxyz[3 * i + 2] = xyz[3 * src + 2];
  flags[i] = (i == 0 || keys_s[i] != keys_s[i - 1]) ? 1u : 0u;
}

// pos = exclusive scan of the run-start flags: run start i is table entry pos[i].
__global__ __launch_bounds__(256) void table_kernel(int64_t n, Hdr* hdr, const uint64_t* __restrict__ keys_s,
                                                    const uint32_t* __restrict__ pos, uint64_t* __restrict__ ukeys,
                                                    uint32_t* __restrict__ ustart) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool start = i == 0 || keys_s[i] != keys_s[i - 1];
  if (start) {
    ukeys[pos[i]] = keys_s[i];
    ustart[pos[i]] = (uint32_t)i;
  }
  if (i == n - 1) {
    const uint32_t nu = pos[i] + (start ? 1u : 0u);
    ustart[nu] = (uint32_t)n;
    hdr->n_unique = (int32_t)nu;
  }
}

// ---------------------------------------------------------------- radius count
// One workgroup per occupied cell (grid-stride).  The cell's points are the queries, one per
// thread, 256 at a time; the candidates are the 9 row ranges of the 3x3x3 block, staged through
// LDS in tiles of kTile points and read back as broadcasts (every lane the same address), so the
// inner loop is fp64 VALU fed from LDS.  A wave none of whose lanes holds a query skips the loop.
__global__ __launch_bounds__(256) void radius_count_kernel(const Hdr* hdr, const double* __restrict__ sxyz,
                                                           const uint32_t* __restrict__ sidx,
                                                           const uint64_t* __restrict__ ukeys,
                                                           const uint32_t* __restrict__ ustart, double r2,
                                                           int32_t nb_points, uint8_t* __restrict__ keep,
                                                           int32_t* __restrict__ counts) {
  __shared__ double tile[3 * kTile];
  __shared__ uint32_t rng[9][2];
  if (hdr->status) return;
  const int nu = hdr->n_unique;
  const int t = threadIdx.x;
  for (int u = blockIdx.x; u < nu; u += gridDim.x) {
    const uint64_t key = ukeys[u];
    const int64_t cx = key & kCellMax, cy = (key >> kCellBits) & kCellMax, cz = (key >> (2 * kCellBits)) & kCellMax;
    const uint32_t qs = ustart[u], qe = ustart[u + 1];
    __syncthreads();                         // the previous cell's ranges are no longer read
    if (t < 9) {
      const int64_t y = cy + (t % 3) - 1, z = cz + (t / 3) - 1;
      uint32_t s = 0, e = 0;
      if (y >= 0 && y <= hdr->cmax[1] && z >= 0 && z <= hdr->cmax[2])
        row_range(ukeys, ustart, nu, cx > 0 ? cx - 1 : 0, cx < hdr->cmax[0] ? cx + 1 : cx, y, z, &s, &e);
      rng[t][0] = s;
      rng[t][1] = e;
    }
    __syncthreads();
    for (uint32_t qb = qs; qb < qe; qb += 256) {
      const uint32_t q = qb + t;
      const bool active = q < qe;
      const bool wave_active = qb + (uint32_t)(t & ~63) < qe;
      double px = 0.0, py = 0.0, pz = 0.0;
      if (active) { px = sxyz[3 * (size_t)q]; py = sxyz[3 * (size_t)q + 1]; pz = sxyz[3 * (size_t)q + 2]; }
      int32_t cnt = 0;
      for (int r = 0; r < 9; ++r) {
        const uint32_t s = rng[r][0], e = rng[r][1];
        for (uint32_t tb = s; tb < e; tb += kTile) {
          const int m = (int)(e - tb < (uint32_t)kTile ? e - tb : (uint32_t)kTile);
          __syncthreads();                   // the previous tile has been consumed
          for (int w = t; w < 3 * m; w += 256) tile[w] = sxyz[3 * (size_t)tb + w];
          __syncthreads();
          if (wave_active) {
#pragma unroll 4
            for (int j = 0; j < m; ++j) {
              const double d2 = d2_rule(tile[3 * j] - px, tile[3 * j + 1] - py, tile[3 * j + 2] - pz);
              cnt += radius_neighbour_rule(d2, r2) ? 1 : 0;
            }
          }
        }
      }
      if (active) {
        const uint32_t o = sidx[q];
        keep[o] = radius_keep_rule(cnt, nb_points) ? 1 : 0;
        if (counts) counts[o] = cnt;
      }
    }
  }
}

// ---------------------------------------------------------------- kNN
// Per-lane top-kk list of d2 in LDS, lst[j * 64 + lane] (lanes on consecutive addresses):
// unsorted while filling, with the largest entry tracked; once full, a smaller d2 replaces the
// largest and the list is rescanned for the new one.
struct TopK {
  double* lst;      // this lane's column
  int kk, cnt, maxpos;
  double curmax;
  __device__ inline void insert(double d) {
    if (cnt < kk) {
      lst[cnt * 64] = d;
      if (d > curmax) { curmax = d; maxpos = cnt; }
      ++cnt;
    } else if (d < curmax) {
      lst[maxpos * 64] = d;
      double m = -1.0;
      int mp = 0;
      for (int j = 0; j < kk; ++j) {
        const double v = lst[j * 64];
        if (v > m) { m = v; mp = j; }
      }
      curmax = m;
      maxpos = mp;
    }
  }
  __device__ inline void sort() {            // ascending insertion sort of the cnt entries
    for (int a = 1; a < cnt; ++a) {
      const double v = lst[a * 64];
      int b = a - 1;
      while (b >= 0 && lst[b * 64] > v) { lst[(b + 1) * 64] = lst[b * 64]; --b; }
      lst[(b + 1) * 64] = v;
    }
  }
};

__device__ inline void scan_range(TopK& tk, const double* __restrict__ sxyz, uint32_t s, uint32_t e, double px,
                                  double py, double pz) {
  for (uint32_t j = s; j < e; ++j)
    tk.insert(d2_rule(sxyz[3 * (size_t)j] - px, sxyz[3 * (size_t)j + 1] - py, sxyz[3 * (size_t)j + 2] - pz));
}

// One point per thread: cells in Chebyshev rings around the point's cell until the list is full
// and its largest d2 is no larger than the squared distance to the nearest face of the block
// searched (faces at or past the cloud's box do not count: nothing lies beyond them).  The face
// distance gives up the header's absolute slack and a relative 1e-12, so rounding in the cell
// coordinates cannot end the walk early.  Points still open after kMaxRing rings go to the list
// of knn_far_kernel.
__global__ __launch_bounds__(64) void knn_kernel(Hdr* hdr, const double* __restrict__ sxyz,
                                                 const uint32_t* __restrict__ sidx,
                                                 const uint64_t* __restrict__ ukeys,
                                                 const uint32_t* __restrict__ ustart, int64_t n, int k,
                                                 double* __restrict__ avg, uint32_t* __restrict__ far) {
  extern __shared__ double lds[];
  if (hdr->status) return;
  const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (q >= n) return;
  const int nu = hdr->n_unique;
  const double h = hdr->cell;
  const double p[3] = {sxyz[3 * q], sxyz[3 * q + 1], sxyz[3 * q + 2]};
  int64_t c[3], cm[3];
  for (int a = 0; a < 3; ++a) { c[a] = cell_coord(p[a], hdr->mn[a], h); cm[a] = hdr->cmax[a]; }
  TopK tk{lds + threadIdx.x, (int)(n < k ? n : k), 0, 0, -1.0};
  bool done = false;
  for (int R = 0; R <= kMaxRing && !done; ++R) {
    for (int dz = -R; dz <= R; ++dz) {
      const int64_t z = c[2] + dz;
      if (z < 0 || z > cm[2]) continue;
      for (int dy = -R; dy <= R; ++dy) {
        const int64_t y = c[1] + dy;
        if (y < 0 || y > cm[1]) continue;
        uint32_t s, e;
        if (abs(dy) == R || abs(dz) == R) {  // a whole row of the shell
          row_range(ukeys, ustart, nu, c[0] - R < 0 ? 0 : c[0] - R, c[0] + R > cm[0] ? cm[0] : c[0] + R, y, z, &s, &e);
          scan_range(tk, sxyz, s, e, p[0], p[1], p[2]);
        } else {                             // the row's two end cells
          if (c[0] - R >= 0) {
            row_range(ukeys, ustart, nu, c[0] - R, c[0] - R, y, z, &s, &e);
            scan_range(tk, sxyz, s, e, p[0], p[1], p[2]);
          }
          if (c[0] + R <= cm[0]) {
            row_range(ukeys, ustart, nu, c[0] + R, c[0] + R, y, z, &s, &e);
            scan_range(tk, sxyz, s, e, p[0], p[1], p[2]);
          }
        }
      }
    }
    double bound = kInf;
    for (int a = 0; a < 3; ++a) {
      if (c[a] - R > 0) bound = fmin(bound, p[a] - (hdr->mn[a] + (double)(c[a] - R) * h));
      if (c[a] + R < cm[a]) bound = fmin(bound, (hdr->mn[a] + (double)(c[a] + R + 1) * h) - p[a]);
    }
    if (bound == kInf) {
      done = true;                           // the whole cloud has been searched
    } else if (tk.cnt == tk.kk) {
      const double b = fmax(bound - hdr->slack, 0.0);
      done = tk.curmax <= (b * b) * (1.0 - 1e-12);
    }
  }
  if (!done) {
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
__global__ __launch_bounds__(64) void knn_far_kernel(const Hdr* hdr, const double* __restrict__ sxyz,
                                                     const uint32_t* __restrict__ sidx, int64_t n, int k,
                                                     double* __restrict__ avg, const uint32_t* __restrict__ far) {
  extern __shared__ double lds[];
  if (hdr->status) return;
  const int lane = threadIdx.x;
  const int nf = hdr->n_far;
  const int kk = (int)(n < k ? n : k);
  for (int f = blockIdx.x; f < nf; f += gridDim.x) {
    const int64_t q = far[f];
    const double px = sxyz[3 * q], py = sxyz[3 * q + 1], pz = sxyz[3 * q + 2];
    TopK tk{lds + lane, kk, 0, 0, -1.0};
    for (int64_t j = lane; j < n; j += 64)
      tk.insert(d2_rule(sxyz[3 * j] - px, sxyz[3 * j + 1] - py, sxyz[3 * j + 2] - pz));
    tk.sort();
    int head = 0;
    double sum = 0.0;
    for (int r = 0; r < kk; ++r) {
      const double v = head < tk.cnt ? tk.lst[head * 64] : kInf;
      double m = v;
      for (int s = 32; s > 0; s >>= 1) m = fmin(m, __shfl_xor(m, s, 64));
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

__device__ inline double block_tree_sum(double v, double* sm) {
  const int t = threadIdx.x;
  sm[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sm[t] = sm[t] + sm[t + s];
    __syncthreads();
  }
  return sm[0];
}

template <int MODE>
__global__ __launch_bounds__(256) void sum_partial_kernel(const Hdr* hdr, const double* __restrict__ avg, int64_t n,
                                                          double* __restrict__ part) {
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
__global__ __launch_bounds__(256) void sum_final_kernel(Hdr* hdr, const double* __restrict__ part, int nb, int64_t n,
                                                        double std_ratio, double* __restrict__ stats_out) {
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

__global__ __launch_bounds__(256) void stat_keep_kernel(const Hdr* hdr, const double* __restrict__ avg, int64_t n,
                                                        uint8_t* __restrict__ keep) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) keep[i] = stat_keep_rule(avg[i], hdr->thr) ? 1 : 0;
}

// ---------------------------------------------------------------- select
__global__ __launch_bounds__(256) void select_kernel(const double* __restrict__ xyz, const uint8_t* __restrict__ bgr,
                                                     int64_t n, const uint8_t* __restrict__ keep,
                                                     const uint32_t* __restrict__ pos, double* __restrict__ oxyz,
                                                     uint8_t* __restrict__ obgr, int64_t* __restrict__ count,
                                                     int64_t capacity, int64_t* __restrict__ index_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t j = pos[i];
  if (keep[i] && j < capacity) {
    for (int a = 0; a < 3; ++a) oxyz[3 * j + a] = xyz[3 * i + a];
    if (bgr && obgr)
      for (int a = 0; a < 3; ++a) obgr[3 * j + a] = bgr[3 * i + a];
    if (index_out) index_out[j] = i;
  }
  if (i == n - 1) {
    const int64_t total = j + (keep[i] ? 1 : 0);
    *count = total < capacity ? total : capacity;
  }
}

// ---------------------------------------------------------------- DBSCAN
// Open3D's ClusterDBSCAN in closed form: core = count >= min_points; a cluster's
// core set is a connected component of the core-core neighbour graph; components are ranked by
// their smallest original core index; a non-core point takes the lowest label among its core
// neighbours, or -1.
//
// The components come from a lock-free union-find over parent[n], indexed by original index.
// Invariant: parent[x] <= x, and an entry only ever decreases (every write is an atomic min), so
// the structure is acyclic, every find ends, and a component's root is its smallest index.  A
// failed link means another lane linked first; the loop goes on from what that lane wrote and
// never waits for anything another workgroup has yet to publish.  Inside the union kernel every
// access to parent is an agent-scope atomic: a plain load could be served from a stale line.
constexpr uint32_t kNone = 0xFFFFFFFFu;

__device__ inline uint32_t par_load(uint32_t* parent, uint32_t i) {
  return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline uint32_t par_min(uint32_t* parent, uint32_t i, uint32_t v) {
  return __hip_atomic_fetch_min(parent + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Root of x, halving the path on the way (each step walks to a smaller index).
__device__ inline uint32_t uf_find(uint32_t* parent, uint32_t x) {
  uint32_t p = par_load(parent, x);
  while (p != x) {
    const uint32_t gp = par_load(parent, p);
    if (gp != p) par_min(parent, x, gp);
    x = p;
    p = gp;
  }
  return x;
}
// Joins the sets of a and b and returns the root both then share.  When the min lands on an
// entry that was no longer a root (old != hi), hi now points at min(old, lo) and the loop joins
// old with lo, which puts back whatever that write took apart; max(a, b) falls every round.
__device__ inline uint32_t uf_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return a;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t old = par_min(parent, hi, lo);
    if (old == hi) return lo;
    a = old;
    b = lo;
  }
}

// The 9 row ranges of the 3x3x3 block around cell `key` (threads 0..8), as radius_count_kernel.
__device__ inline void block_ranges(const Hdr* hdr, const uint64_t* __restrict__ ukeys,
                                    const uint32_t* __restrict__ ustart, int nu, uint64_t key, uint32_t (*rng)[2]) {
  const int t = threadIdx.x;
  if (t >= 9) return;
  const int64_t cx = key & kCellMax, cy = (key >> kCellBits) & kCellMax, cz = (key >> (2 * kCellBits)) & kCellMax;
  const int64_t y = cy + (t % 3) - 1, z = cz + (t / 3) - 1;
  uint32_t s = 0, e = 0;
  if (y >= 0 && y <= hdr->cmax[1] && z >= 0 && z <= hdr->cmax[2])
    row_range(ukeys, ustart, nu, cx > 0 ? cx - 1 : 0, cx < hdr->cmax[0] ? cx + 1 : cx, y, z, &s, &e);
  rng[t][0] = s;
  rng[t][1] = e;
}

// Per sorted position q: scidx[q] = the point's original index when it is core, else kNone (the
// word the later walks stage beside the coordinates); parent[i] = i; sizes[i] = 0.
__global__ __launch_bounds__(256) void dbscan_core_kernel(const Hdr* hdr, int64_t n, const uint32_t* __restrict__ sidx,
                                                          const int32_t* __restrict__ cnt, int32_t min_points,
                                                          uint32_t* __restrict__ scidx, uint32_t* __restrict__ parent,
                                                          int32_t* __restrict__ sizes) {
  if (hdr->status) return;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const uint32_t o = sidx[q];
  scidx[q] = core_rule(cnt[o], min_points) ? o : kNone;
  parent[q] = (uint32_t)q;
  sizes[q] = 0;
}

// Before any pair is looked at: a cell is split 2x2x2, and the core points of one sub-cell are
// linked to the smallest index among them.  Two points of one sub-cell are at most sqrt(3)/2 of
// the cell apart (plus 2^-30 of it for the rounding of the fine coordinate), well inside eps, so
// they are neighbours by the rule; the links are plain stores, each lane writing its own entry
// of a parent array nothing else touches during this launch.  The union kernel then meets a few
// dozen sets per query instead of a few hundred single points.  A point whose fine coordinate
// does not fall in its own cell (rounding at a face) stays alone.
__global__ __launch_bounds__(256) void dbscan_subcell_kernel(const Hdr* hdr, const double* __restrict__ sxyz,
                                                             const uint32_t* __restrict__ scidx,
                                                             const uint64_t* __restrict__ ukeys,
                                                             const uint32_t* __restrict__ ustart,
                                                             uint32_t* __restrict__ parent) {
  __shared__ uint32_t submin[8];
  if (hdr->status) return;
  const int nu = hdr->n_unique;
  const int t = threadIdx.x;
  const double half = 0.5 * hdr->cell;
  for (int u = blockIdx.x; u < nu; u += gridDim.x) {
    const uint64_t key = ukeys[u];
    const int64_t c[3] = {(int64_t)(key & kCellMax), (int64_t)((key >> kCellBits) & kCellMax),
                          (int64_t)((key >> (2 * kCellBits)) & kCellMax)};
    const uint32_t qs = ustart[u], qe = ustart[u + 1];
    __syncthreads();                         // the previous cell's minima are no longer read
    if (t < 8) submin[t] = kNone;
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {   // 0: the minima; 1: the links
      for (uint32_t q = qs + t; q < qe; q += 256) {
        const uint32_t me = scidx[q];
        if (me == kNone) continue;
        int sub = 0;
        for (int a = 0; a < 3; ++a) {
          const double f = floor((sxyz[3 * (size_t)q + a] - hdr->mn[a]) / half) - 2.0 * (double)c[a];
          sub = (f == 0.0 || f == 1.0) && sub >= 0 ? sub | ((int)f << a) : -1;
        }
        if (sub < 0) continue;
        if (pass == 0) atomicMin(&submin[sub], me);
        else if (submin[sub] != me) parent[me] = submin[sub];
      }
      __syncthreads();
    }
  }
}

// The radius walk again, one workgroup per occupied cell: core queries against core candidates.
// A pair is seen from both ends, so only the end with the larger index unites.  tpar holds the
// candidate's root as it stood when the tile was staged.  A candidate whose staged root is the
// query's current root, or the staged root of the candidate last united with (that set is the
// query's by now), is in the query's set already and costs no global access: a lane unites
// about once per distinct set among its neighbours, not once per neighbour.  Without that the
// kernel is bound by the latency of one lane's atomics while its wave waits (20 ms on a 1080p
// view at eps 5).  A batch of queries without a core point skips the walk.
__global__ __launch_bounds__(256) void dbscan_union_kernel(const Hdr* hdr, const double* __restrict__ sxyz,
                                                           const uint32_t* __restrict__ scidx,
                                                           const uint64_t* __restrict__ ukeys,
                                                           const uint32_t* __restrict__ ustart, double r2,
                                                           uint32_t* parent) {
  __shared__ double tile[3 * kTile];
  __shared__ uint32_t tci[kTile], tpar[kTile];
  __shared__ uint32_t rng[9][2];
  if (hdr->status) return;
  const int nu = hdr->n_unique;
  const int t = threadIdx.x;
  for (int u = blockIdx.x; u < nu; u += gridDim.x) {
    const uint32_t qs = ustart[u], qe = ustart[u + 1];
    __syncthreads();                         // the previous cell's ranges are no longer read
    block_ranges(hdr, ukeys, ustart, nu, ukeys[u], rng);
    __syncthreads();
    for (uint32_t qb = qs; qb < qe; qb += 256) {
      const uint32_t q = qb + t;
      const uint32_t me = q < qe ? scidx[q] : kNone;
      const bool core = me != kNone;
      if (!__syncthreads_or(core ? 1 : 0)) continue;
      const bool wave_active = __ballot(core) != 0;
      const uint32_t lim = core ? me : 0u;   // candidates below lim are this lane's to unite
      double px = 0.0, py = 0.0, pz = 0.0;
      if (core) { px = sxyz[3 * (size_t)q]; py = sxyz[3 * (size_t)q + 1]; pz = sxyz[3 * (size_t)q + 2]; }
      uint32_t hint = core ? uf_find(parent, me) : kNone;   // the root of this lane's set, as last seen
      uint32_t last = kNone;                 // the staged root of the last candidate united with
      for (int r = 0; r < 9; ++r) {
        const uint32_t s = rng[r][0], e = rng[r][1];
        for (uint32_t tb = s; tb < e; tb += kTile) {
          const int m = (int)(e - tb < (uint32_t)kTile ? e - tb : (uint32_t)kTile);
          __syncthreads();                   // the previous tile has been consumed
          for (int w = t; w < 3 * m; w += 256) tile[w] = sxyz[3 * (size_t)tb + w];
          for (int w = t; w < m; w += 256) {
            const uint32_t c = scidx[tb + w];
            tci[w] = c;
            tpar[w] = c == kNone ? kNone : uf_find(parent, c);
          }
          __syncthreads();
          if (wave_active) {
            for (int j = 0; j < m; ++j) {
              const uint32_t c = tci[j];
              const double d2 = d2_rule(tile[3 * j] - px, tile[3 * j + 1] - py, tile[3 * j + 2] - pz);
              const uint32_t cr = tpar[j];
              if (c < lim && radius_neighbour_rule(d2, r2) && cr != hint && cr != last) {
                hint = uf_unite(parent, hint, c);
                last = cr;
                par_min(parent, c, hint);    // a later staging of c then finds the root at once
                tpar[j] = hint;              // and the other waves of this workgroup see it now
              }
            }
          }
        }
      }
    }
  }
}

// root[i] = the root of core point i (kNone for a non-core point); flags[i] = i is a root.  The
// exclusive scan of flags over the original order is then the label of every root.
__global__ __launch_bounds__(256) void dbscan_flatten_kernel(const Hdr* hdr, int64_t n, const int32_t* __restrict__ cnt,
                                                             int32_t min_points, uint32_t* parent,
                                                             uint32_t* __restrict__ root, uint32_t* __restrict__ flags) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = core_rule(cnt[i], min_points) ? uf_find(parent, (uint32_t)i) : kNone;
  root[i] = r;
  flags[i] = r == (uint32_t)i ? 1u : 0u;
}

// sroot[q] = root of the point at sorted position q, for the border walk to stage; the cluster
// count from the end of the scan.
__global__ __launch_bounds__(256) void dbscan_sroot_kernel(Hdr* hdr, int64_t n, const uint32_t* __restrict__ sidx,
                                                           const uint32_t* __restrict__ root,
                                                           const uint32_t* __restrict__ flags,
                                                           const uint32_t* __restrict__ pos, uint32_t* __restrict__ sroot) {
  if (hdr->status) return;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  sroot[q] = root[sidx[q]];
  if (q == n - 1) hdr->n_clusters = (int32_t)(pos[q] + flags[q]);
}

// Labels.  A core point's is the scan value of its root.  A non-core point with a neighbour
// besides itself walks the block for the smallest root among its core neighbours (labels rise
// with the root index, so that is the smallest label); a batch of queries without such a point
// skips the walk, as does a wave.
__global__ __launch_bounds__(256) void dbscan_border_kernel(const Hdr* hdr, const double* __restrict__ sxyz,
                                                            const uint32_t* __restrict__ sidx,
                                                            const uint32_t* __restrict__ sroot,
                                                            const int32_t* __restrict__ cnt,
                                                            const uint32_t* __restrict__ pos,
                                                            const uint64_t* __restrict__ ukeys,
                                                            const uint32_t* __restrict__ ustart, double r2,
                                                            int32_t* __restrict__ labels) {
  __shared__ double tile[3 * kTile];
  __shared__ uint32_t tsr[kTile];
  __shared__ uint32_t rng[9][2];
  if (hdr->status) return;
  const int nu = hdr->n_unique;
  const int t = threadIdx.x;
  for (int u = blockIdx.x; u < nu; u += gridDim.x) {
    const uint32_t qs = ustart[u], qe = ustart[u + 1];
    __syncthreads();                         // the previous cell's ranges are no longer read
    block_ranges(hdr, ukeys, ustart, nu, ukeys[u], rng);
    __syncthreads();
    for (uint32_t qb = qs; qb < qe; qb += 256) {
      const uint32_t q = qb + t;
      const bool active = q < qe;
      uint32_t o = 0, best = kNone;
      bool need = false;
      if (active) {
        o = sidx[q];
        best = sroot[q];
        need = best == kNone && cnt[o] > 1;
      }
      if (__syncthreads_or(need ? 1 : 0)) {
        const bool wave_need = __ballot(need) != 0;
        double px = 0.0, py = 0.0, pz = 0.0;
        if (need) { px = sxyz[3 * (size_t)q]; py = sxyz[3 * (size_t)q + 1]; pz = sxyz[3 * (size_t)q + 2]; }
        for (int r = 0; r < 9; ++r) {
          const uint32_t s = rng[r][0], e = rng[r][1];
          for (uint32_t tb = s; tb < e; tb += kTile) {
            const int m = (int)(e - tb < (uint32_t)kTile ? e - tb : (uint32_t)kTile);
            __syncthreads();                 // the previous tile has been consumed
            for (int w = t; w < 3 * m; w += 256) tile[w] = sxyz[3 * (size_t)tb + w];
            for (int w = t; w < m; w += 256) tsr[w] = sroot[tb + w];
            __syncthreads();
            if (wave_need) {
#pragma unroll 4
              for (int j = 0; j < m; ++j) {
                const double d2 = d2_rule(tile[3 * j] - px, tile[3 * j + 1] - py, tile[3 * j + 2] - pz);
                const uint32_t sr = tsr[j];
                best = (need && radius_neighbour_rule(d2, r2) && sr < best) ? sr : best;
              }
            }
          }
        }
      }
      if (active) labels[o] = best == kNone ? -1 : (int32_t)pos[best];
    }
  }
}

// Members per label and the noise count.  Integer atomics (order-independent), one per distinct
// label of a wave: neighbours in the input order mostly share a label.
__global__ __launch_bounds__(256) void dbscan_sizes_kernel(Hdr* hdr, int64_t n, const int32_t* __restrict__ labels,
                                                           int32_t* __restrict__ sizes) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int32_t l = i < n ? labels[i] : -2;
  const unsigned long long noise = __ballot(l == -1);
  if (noise && lane == __ffsll((long long)noise) - 1) atomicAdd(&hdr->n_noise, (int32_t)__popcll(noise));
  bool todo = l >= 0;
  for (;;) {
    const unsigned long long open = __ballot(todo);
    if (!open) break;
    const int leader = __ffsll((long long)open) - 1;
    const int32_t l0 = __shfl(l, leader, 64);
    const unsigned long long same = __ballot(todo && l == l0);
    if (lane == leader) atomicAdd(&sizes[l0], (int32_t)__popcll(same));
    if (l == l0) todo = false;
  }
}

__global__ __launch_bounds__(256) void dbscan_argmax_kernel(Hdr* hdr, const int32_t* __restrict__ sizes) {
  if (hdr->status) return;
  const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (l >= hdr->n_clusters) return;
  atomicMax(&hdr->best, ((unsigned long long)(uint32_t)sizes[l] << 32) | (uint32_t)~(uint32_t)l);
}

__global__ __launch_bounds__(256) void dbscan_keep_kernel(const Hdr* hdr, int64_t n, const int32_t* __restrict__ labels,
                                                          uint8_t* __restrict__ keep, int32_t* __restrict__ info) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool any = hdr->n_clusters > 0;
  const int32_t largest = any ? (int32_t)~(uint32_t)hdr->best : -1;
  if (keep) keep[i] = any && labels[i] == largest ? 1 : 0;
  if (i == 0 && info) {
    info[0] = hdr->n_clusters;
    info[1] = largest;
    info[2] = any ? (int32_t)(hdr->best >> 32) : 0;
    info[3] = hdr->n_noise;
  }
}

// ---------------------------------------------------------------- voxel down-sample
// Open3D's VoxelDownSample, restated.  The grid is the one above with the origin
// at min - voxel/2 and the cell exactly `voxel`: cell_coord is then floor((p - vmin) / voxel) in
// IEEE subtraction and division, NumPy's own result.  The stable (key, index) sort delivers each
// voxel's members in ascending original index, which is the order of the sums.
constexpr int kVoxelLong = 64;     // members above which a voxel goes to the wave kernel

__device__ inline double voxel_origin_rule(double mn, double voxel) { return mn - voxel * 0.5; }
__device__ inline double voxel_mean_rule(double sum, uint32_t count) { return sum / (double)count; }
// exact mean of a colour channel, rounded half up, in integers
__device__ inline uint8_t colour_mean_rule(unsigned long long sum, uint32_t count) {
  return (uint8_t)((2ull * sum + count) / (2ull * count));
}

__global__ void voxel_setup_kernel(Hdr* hdr, double voxel) {
  if (hdr->status) return;
  double vmin[3], c[3];
  for (int a = 0; a < 3; ++a) {
    vmin[a] = voxel_origin_rule(hdr->mn[a], voxel);
    c[a] = floor((hdr->mx[a] - vmin[a]) / voxel);
    if (!(c[a] <= (double)kCellMax)) { atomicOr(&hdr->status, SLG_FILTER_BAD_EXTENT); return; }
  }
  for (int a = 0; a < 3; ++a) { hdr->mn[a] = vmin[a]; hdr->cmax[a] = (int32_t)c[a]; }
  hdr->cell = voxel;
}

// head[i] = 1 when original point i is the first (smallest-index) member of its voxel.  The
// exclusive scan of head over the original order is the voxel's place in the output.
__global__ __launch_bounds__(256) void voxel_heads_kernel(const Hdr* hdr, int64_t n, const uint64_t* __restrict__ keys_s,
                                                          const uint32_t* __restrict__ sidx,
                                                          uint32_t* __restrict__ head) {
  if (hdr->status) return;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  head[sidx[q]] = (q == 0 || keys_s[q] != keys_s[q - 1]) ? 1u : 0u;
}

struct VoxelOut {
  double* xyz;
  uint8_t* bgr;
  int64_t* first;
  int32_t* count;
};

__device__ inline void voxel_write(const VoxelOut& o, uint32_t slot, uint32_t first, uint32_t count, double sx,
                                   double sy, double sz, const unsigned long long* cs) {
  o.xyz[3 * (size_t)slot] = voxel_mean_rule(sx, count);
  o.xyz[3 * (size_t)slot + 1] = voxel_mean_rule(sy, count);
  o.xyz[3 * (size_t)slot + 2] = voxel_mean_rule(sz, count);
  if (o.bgr)
    for (int a = 0; a < 3; ++a) o.bgr[3 * (size_t)slot + a] = colour_mean_rule(cs[a], count);
  if (o.first) o.first[slot] = (int64_t)first;
  if (o.count) o.count[slot] = (int32_t)count;
}

// One lane per voxel: the left-to-right sum of its members.  A voxel of more than kVoxelLong
// members goes to the list of voxel_long_kernel (list order is free).
__global__ __launch_bounds__(256) void voxel_reduce_kernel(Hdr* hdr, const double* __restrict__ sxyz,
                                                           const uint32_t* __restrict__ sidx,
                                                           const uint8_t* __restrict__ bgr,
                                                           const uint32_t* __restrict__ ustart,
                                                           const uint32_t* __restrict__ place,
                                                           uint32_t* __restrict__ longlist, VoxelOut out,
                                                           int64_t* __restrict__ m_out) {
  if (hdr->status) return;
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int nu = hdr->n_unique;
  if (u == 0) *m_out = nu;
  if (u >= nu) return;
  const uint32_t s = ustart[u], e = ustart[u + 1];
  if (e - s > (uint32_t)kVoxelLong) {
    longlist[atomicAdd(&hdr->n_far, 1)] = (uint32_t)u;
    return;
  }
  double sx = sxyz[3 * (size_t)s], sy = sxyz[3 * (size_t)s + 1], sz = sxyz[3 * (size_t)s + 2];
  unsigned long long cs[3] = {0, 0, 0};
  const uint32_t first = sidx[s];
  if (bgr)
    for (int a = 0; a < 3; ++a) cs[a] = bgr[3 * (size_t)first + a];
  for (uint32_t j = s + 1; j < e; ++j) {
    sx += sxyz[3 * (size_t)j];
    sy += sxyz[3 * (size_t)j + 1];
    sz += sxyz[3 * (size_t)j + 2];
    if (bgr) {
      const size_t o = 3 * (size_t)sidx[j];
      for (int a = 0; a < 3; ++a) cs[a] += bgr[o + a];
    }
  }
  voxel_write(out, place[first], first, e - s, sx, sy, sz, cs);
}

// One wave per listed voxel: 64 members are loaded at a time, one per lane, and every lane then
// adds them in lane order from broadcasts, so the additions are the same sequence as the
// left-to-right sum while the loads run side by side.  Colour sums are integers (order-free).
__global__ __launch_bounds__(64) void voxel_long_kernel(const Hdr* hdr, const double* __restrict__ sxyz,
                                                        const uint32_t* __restrict__ sidx,
                                                        const uint8_t* __restrict__ bgr,
                                                        const uint32_t* __restrict__ ustart,
                                                        const uint32_t* __restrict__ place,
                                                        const uint32_t* __restrict__ longlist, VoxelOut out) {
  if (hdr->status) return;
  const int lane = threadIdx.x;
  const int nl = hdr->n_far;
  for (int f = blockIdx.x; f < nl; f += gridDim.x) {
    const uint32_t u = longlist[f];
    const uint32_t s = ustart[u], e = ustart[u + 1];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    unsigned long long cs[3] = {0, 0, 0};
    for (uint32_t base = s; base < e; base += 64) {
      const uint32_t j = base + lane;
      const int m = (int)(e - base < 64u ? e - base : 64u);
      double vx = 0.0, vy = 0.0, vz = 0.0;
      if (j < e) {
        vx = sxyz[3 * (size_t)j]; vy = sxyz[3 * (size_t)j + 1]; vz = sxyz[3 * (size_t)j + 2];
        if (bgr) {
          const size_t o = 3 * (size_t)sidx[j];
          for (int a = 0; a < 3; ++a) cs[a] += bgr[o + a];
        }
      }
      for (int t = 0; t < m; ++t) {
        const double bx = __shfl(vx, t, 64), by = __shfl(vy, t, 64), bz = __shfl(vz, t, 64);
        if (base == s && t == 0) { sx = bx; sy = by; sz = bz; }     // the sum starts at the first member
        else { sx += bx; sy += by; sz += bz; }
      }
    }
    for (int a = 0; a < 3; ++a)
      for (int sh = 32; sh > 0; sh >>= 1) cs[a] += __shfl_xor(cs[a], sh, 64);
    const uint32_t first = sidx[s];
    if (lane == 0) voxel_write(out, place[first], first, e - s, sx, sy, sz, cs);
  }
}

// ---------------------------------------------------------------- normals
// Open3D's EstimateNormals with KDTreeSearchParamHybrid, restated: the neighbours
// of a point are the first max_nn of all points in (d2, original index) order that have
// d2 < radius^2; nine raw moments summed in that order; cov = E[ab] - E[a]E[b]; the normal is the
// unit eigenvector of the smallest eigenvalue (cyclic Jacobi, kJacobiSweeps sweeps), signed so
// that the first non-zero of (nz, ny, nx) is positive.
constexpr int kJacobiSweeps = 5;

__device__ inline bool pair_before_rule(double a, uint32_t ai, double b, uint32_t bi) {
  return a < b || (a == b && ai < bi);
}

// The per-lane top-kk list of (d2, original index) in (d2, index) order: TopK with the index
// beside the distance, idx[j * 64 + lane] after the kk * 64 distances.
struct TopKI {
  double* lst;
  uint32_t* idx;
  int kk, cnt, maxpos;
  double curmax;
  uint32_t maxidx;
  // a candidate at distance d can only enter when the list is open or d is no larger than its largest
  __device__ inline bool wants(double d) const { return cnt < kk || d <= curmax; }
  __device__ inline void insert(double d, uint32_t i) {
    if (cnt < kk) {
      lst[cnt * 64] = d;
      idx[cnt * 64] = i;
      if (cnt == 0 || pair_before_rule(curmax, maxidx, d, i)) { curmax = d; maxidx = i; maxpos = cnt; }
      ++cnt;
    } else if (pair_before_rule(d, i, curmax, maxidx)) {
      lst[maxpos * 64] = d;
      idx[maxpos * 64] = i;
      double m = lst[0];
      uint32_t mi = idx[0];
      int mp = 0;
      for (int j = 1; j < kk; ++j) {
        const double v = lst[j * 64];
        if (v >= m) {
          const uint32_t vi = idx[j * 64];
          if (pair_before_rule(m, mi, v, vi)) { m = v; mi = vi; mp = j; }
        }
      }
      curmax = m;
      maxidx = mi;
      maxpos = mp;
    }
  }
  __device__ inline void sort() {            // ascending insertion sort by (d2, index)
    for (int a = 1; a < cnt; ++a) {
      const double v = lst[a * 64];
      const uint32_t vi = idx[a * 64];
      int b = a - 1;
      while (b >= 0 && pair_before_rule(v, vi, lst[b * 64], idx[b * 64])) {
        lst[(b + 1) * 64] = lst[b * 64];
        idx[(b + 1) * 64] = idx[b * 64];
        --b;
      }
      lst[(b + 1) * 64] = v;
      idx[(b + 1) * 64] = vi;
    }
  }
};

__device__ inline void scan_range_i(TopKI& tk, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                                    uint32_t s, uint32_t e, double px, double py, double pz, double r2) {
  for (uint32_t j = s; j < e; ++j) {
    const double d = d2_rule(sxyz[3 * (size_t)j] - px, sxyz[3 * (size_t)j + 1] - py, sxyz[3 * (size_t)j + 2] - pz);
    if (radius_neighbour_rule(d, r2) && tk.wants(d)) tk.insert(d, sidx[j]);
  }
}

struct Moments {        // the nine running sums
  double x, y, z, xx, xy, xz, yy, yz, zz;
  __device__ inline void clear() { x = y = z = xx = xy = xz = yy = yz = zz = 0.0; }
  __device__ inline void add(double px, double py, double pz) {
    x += px; y += py; z += pz;
    xx += px * px; xy += px * py; xz += px * pz;
    yy += py * py; yz += py * pz; zz += pz * pz;
  }
};
struct Cov { double xx, xy, xz, yy, yz, zz; };
struct Vec3 { double x, y, z; };

// cov from the nine sums over m neighbours: each sum / m, then E[ab] - E[a] E[b].
__device__ __forceinline__ Cov covariance_rule(const Moments& M, int m) {
  const double d = (double)m;
  const double ex = M.x / d, ey = M.y / d, ez = M.z / d;
  Cov c;
  c.xx = M.xx / d - ex * ex;
  c.xy = M.xy / d - ex * ey;
  c.xz = M.xz / d - ex * ez;
  c.yy = M.yy / d - ey * ey;
  c.yz = M.yz / d - ey * ez;
  c.zz = M.zz / d - ez * ez;
  return c;
}

// One Jacobi rotation in the (p, q) plane of a symmetric 3x3 matrix (r is the third index):
// app, aqq, apq the plane's entries, arp, arq the third row's; v?p, v?q the eigenvector columns.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                     double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp; arq = rq;
  const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
  v0p = a0; v0q = b0;
  const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
  v1p = a1; v1q = b1;
  const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
  v2p = a2; v2q = b2;
}

// The normal of a covariance: (0, 0, 1) with fewer than 3 neighbours or a zero matrix.
__device__ __forceinline__ Vec3 normal_rule(const Cov& c, int m) {
  const bool none = m < 3 || (c.xx == 0.0 && c.xy == 0.0 && c.xz == 0.0 && c.yy == 0.0 && c.yz == 0.0 && c.zz == 0.0);
  double a00 = c.xx, a01 = c.xy, a02 = c.xz, a11 = c.yy, a12 = c.yz, a22 = c.zz;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  if (!none)
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
      jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1), third 2
      jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), third 1
      jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), third 0
    }
  // the column of the first smallest diagonal entry, as two selects (a lookup by index would put
  // the columns into scratch)
  const bool s1 = a11 < a00;
  const double lam = s1 ? a11 : a00;
  double x = s1 ? v01 : v00, y = s1 ? v11 : v10, z = s1 ? v21 : v20;
  const bool s2 = a22 < lam;
  x = s2 ? v02 : x; y = s2 ? v12 : y; z = s2 ? v22 : z;
  const double len = sqrt((x * x + y * y) + z * z);
  x = x / len; y = y / len; z = z / len;
  const bool flip = z != 0.0 ? z < 0.0 : (y != 0.0 ? y < 0.0 : x < 0.0);   // the sign rule
  Vec3 n;
  n.x = none ? 0.0 : (flip ? -x : x);
  n.y = none ? 0.0 : (flip ? -y : y);
  n.z = none ? 1.0 : (flip ? -z : z);
  return n;
}

__device__ __forceinline__ void normals_write(const Moments& M, int m, uint32_t o, double* __restrict__ normals,
                                     double* __restrict__ cov_out, int32_t* __restrict__ m_out) {
  Cov c = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (m > 0) c = covariance_rule(M, m);
  const Vec3 nrm = normal_rule(c, m);
  normals[3 * (size_t)o] = nrm.x;
  normals[3 * (size_t)o + 1] = nrm.y;
  normals[3 * (size_t)o + 2] = nrm.z;
  if (cov_out) {
    double* co = cov_out + 6 * (size_t)o;
    co[0] = c.xx; co[1] = c.xy; co[2] = c.xz; co[3] = c.yy; co[4] = c.yz; co[5] = c.zz;
  }
  if (m_out) m_out[o] = m;
}

// knn_kernel's ring walk with the (d2, index) list and the radius: a candidate enters only with
// d2 < r2, and the walk also ends once the block searched covers the radius ball (r2 no larger
// than the squared face distance), so a point with fewer than max_nn neighbours inside the radius
// stops as soon as nothing further out could count.  Points open after kMaxRing rings (a radius
// of many cells around a point with few neighbours) go to normals_far_kernel.
__global__ __launch_bounds__(64) void normals_kernel(Hdr* hdr, const double* __restrict__ xyz,
                                                     const double* __restrict__ sxyz,
                                                     const uint32_t* __restrict__ sidx,
                                                     const uint64_t* __restrict__ ukeys,
                                                     const uint32_t* __restrict__ ustart, int64_t n, int k, double r2,
                                                     double* __restrict__ normals, double* __restrict__ cov_out,
                                                     int32_t* __restrict__ m_out, uint32_t* __restrict__ far) {
  extern __shared__ double lds[];
  if (hdr->status) return;
  const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (q >= n) return;
  const int nu = hdr->n_unique;
  const double h = hdr->cell;
  const double p[3] = {sxyz[3 * q], sxyz[3 * q + 1], sxyz[3 * q + 2]};
  int64_t c[3], cm[3];
  for (int a = 0; a < 3; ++a) { c[a] = cell_coord(p[a], hdr->mn[a], h); cm[a] = hdr->cmax[a]; }
  const int kk = (int)(n < k ? n : k);
  TopKI tk{lds + threadIdx.x, (uint32_t*)(lds + (size_t)kk * 64) + threadIdx.x, kk, 0, 0, -1.0, 0u};
  bool done = false;
  for (int R = 0; R <= kMaxRing && !done; ++R) {
    for (int dz = -R; dz <= R; ++dz) {
      const int64_t z = c[2] + dz;
      if (z < 0 || z > cm[2]) continue;
      for (int dy = -R; dy <= R; ++dy) {
        const int64_t y = c[1] + dy;
        if (y < 0 || y > cm[1]) continue;
        uint32_t s, e;
        if (abs(dy) == R || abs(dz) == R) {  // a whole row of the shell
          row_range(ukeys, ustart, nu, c[0] - R < 0 ? 0 : c[0] - R, c[0] + R > cm[0] ? cm[0] : c[0] + R, y, z, &s, &e);
          scan_range_i(tk, sxyz, sidx, s, e, p[0], p[1], p[2], r2);
        } else {                             // the row's two end cells
          if (c[0] - R >= 0) {
            row_range(ukeys, ustart, nu, c[0] - R, c[0] - R, y, z, &s, &e);
            scan_range_i(tk, sxyz, sidx, s, e, p[0], p[1], p[2], r2);
          }
          if (c[0] + R <= cm[0]) {
            row_range(ukeys, ustart, nu, c[0] + R, c[0] + R, y, z, &s, &e);
            scan_range_i(tk, sxyz, sidx, s, e, p[0], p[1], p[2], r2);
          }
        }
      }
    }
    double bound = kInf;
    for (int a = 0; a < 3; ++a) {
      if (c[a] - R > 0) bound = fmin(bound, p[a] - (hdr->mn[a] + (double)(c[a] - R) * h));
      if (c[a] + R < cm[a]) bound = fmin(bound, (hdr->mn[a] + (double)(c[a] + R + 1) * h) - p[a]);
    }
    if (bound == kInf) {
      done = true;                           // the whole cloud has been searched
    } else {
      const double b = fmax(bound - hdr->slack, 0.0);
      const double b2 = (b * b) * (1.0 - 1e-12);
      done = r2 <= b2 || (tk.cnt == tk.kk && tk.curmax <= b2);
    }
  }
  if (!done) {
    far[atomicAdd(&hdr->n_far, 1)] = (uint32_t)q;
    return;
  }
  tk.sort();
  Moments M;
  M.clear();
  for (int j = 0; j < tk.cnt; ++j) {
    const size_t o = 3 * (size_t)tk.idx[j * 64];
    M.add(xyz[o], xyz[o + 1], xyz[o + 2]);
  }
  normals_write(M, tk.cnt, sidx[q], normals, cov_out, m_out);
}

// knn_far_kernel with the (d2, index) order: the wave merges its 64 sorted lists by taking the
// smallest (d2, index) head until kk are taken or none is left; every lane adds the same moments.
__global__ __launch_bounds__(64) void normals_far_kernel(const Hdr* hdr, const double* __restrict__ xyz,
                                                         const double* __restrict__ sxyz,
                                                         const uint32_t* __restrict__ sidx, int64_t n, int k,
                                                         double r2, double* __restrict__ normals,
                                                         double* __restrict__ cov_out, int32_t* __restrict__ m_out,
                                                         const uint32_t* __restrict__ far) {
  extern __shared__ double lds[];
  if (hdr->status) return;
  const int lane = threadIdx.x;
  const int nf = hdr->n_far;
  const int kk = (int)(n < k ? n : k);
  for (int f = blockIdx.x; f < nf; f += gridDim.x) {
    const int64_t q = far[f];
    const double px = sxyz[3 * q], py = sxyz[3 * q + 1], pz = sxyz[3 * q + 2];
    TopKI tk{lds + lane, (uint32_t*)(lds + (size_t)kk * 64) + lane, kk, 0, 0, -1.0, 0u};
    for (int64_t j = lane; j < n; j += 64) {
      const double d = d2_rule(sxyz[3 * j] - px, sxyz[3 * j + 1] - py, sxyz[3 * j + 2] - pz);
      if (radius_neighbour_rule(d, r2) && tk.wants(d)) tk.insert(d, sidx[j]);
    }
    tk.sort();
    int head = 0, m = 0;
    Moments M;
    M.clear();
    for (int r = 0; r < kk; ++r) {
      const bool have = head < tk.cnt;
      const double v = have ? tk.lst[head * 64] : kInf;
      const uint32_t vi = have ? tk.idx[head * 64] : kNone;
      double best = v;
      for (int s = 32; s > 0; s >>= 1) best = fmin(best, __shfl_xor(best, s, 64));
      if (best == kInf) break;               // every list is used up (uniform over the wave)
      uint32_t bi = v == best ? vi : kNone;
      for (int s = 32; s > 0; s >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)bi, s, 64);
        bi = other < bi ? other : bi;
      }
      if (have && v == best && vi == bi) ++head;
      const size_t o = 3 * (size_t)bi;
      M.add(xyz[o], xyz[o + 1], xyz[o + 2]);
      ++m;
    }
    if (lane == 0) normals_write(M, m, sidx[q], normals, cov_out, m_out);
  }
}

// Open3D's OrientNormalsTowardsCameraLocation: negated when normal . (loc - p) < 0; `outward`
// then negates every normal (the reference's `* -1.0`).
__device__ inline bool orient_flip_rule(const double* nrm, const double* p, const double* loc) {
  const double rx = loc[0] - p[0], ry = loc[1] - p[1], rz = loc[2] - p[2];
  return (nrm[0] * rx + nrm[1] * ry) + nrm[2] * rz < 0.0;
}

__global__ __launch_bounds__(256) void orient_kernel(const double* __restrict__ xyz, double* __restrict__ normals,
                                                     int64_t n, const double* __restrict__ loc, int outward) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  const double l[3] = {loc[0], loc[1], loc[2]};
  double v[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
  const bool flip = orient_flip_rule(v, p, l) != (outward != 0);
  if (flip)
    for (int a = 0; a < 3; ++a) normals[3 * i + a] = -v[a];
}

// Per-axis sums over the input order with the fixed tree of sum_partial_kernel / sum_final_kernel.
__global__ __launch_bounds__(256) void axis_sum_partial_kernel(const double* __restrict__ xyz, int64_t n,
                                                               double* __restrict__ part) {
  __shared__ double sm[256];
  const int64_t base = (int64_t)blockIdx.x * kChunk + threadIdx.x * (kChunk / 256);
  for (int a = 0; a < 3; ++a) {
    double s = 0.0;
    for (int j = 0; j < kChunk / 256; ++j)
      if (base + j < n) s += xyz[3 * (base + j) + a];
    s = block_tree_sum(s, sm);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.x * 3 + a] = s;
    __syncthreads();                         // sm[0] has been read before the next axis overwrites it
  }
}

__global__ __launch_bounds__(256) void axis_sum_final_kernel(const double* __restrict__ part, int nb, int64_t n,
                                                             double* __restrict__ out) {
  __shared__ double sm[256];
  for (int a = 0; a < 3; ++a) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) s += part[(int64_t)b * 3 + a];
    s = block_tree_sum(s, sm);
    if (threadIdx.x == 0) out[a] = s / (double)n;
    __syncthreads();
  }
}

// ---------------------------------------------------------------- host side
int grid_of(int64_t n, int per) { return (int)((n + per - 1) / per); }

struct Ws {
  Hdr* hdr;
  uint64_t *keys, *keys_s, *ukeys;
  uint32_t *idx, *idx_s, *pos, *ustart, *far;
  double *sxyz, *part, *avg;
  void* temp;
  size_t temp_bytes;
};

int bind_ws(const char* who, int64_t n, void* ws, int64_t ws_bytes, Ws* w) {
  if (!ws || ((uintptr_t)ws & 7)) return slg_internal_fail(SLG_ERR_INVALID, "%s: workspace NULL or not 8-byte aligned", who);
  size_t tb = 0;
  if (temp_bytes_for(n, &tb) != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "%s: rocPRIM size query failed", who);
  const Layout L = make_layout(n, tb);
  if (ws_bytes >= 0 && (size_t)ws_bytes < L.total)
    return slg_internal_fail(SLG_ERR_INVALID, "%s: workspace of %lld bytes, slg_filter_ws_bytes gives %lld", who,
                             (long long)ws_bytes, (long long)L.total);
  char* b = (char*)ws;
  w->hdr = (Hdr*)b;
  w->keys = (uint64_t*)(b + L.keys);     w->keys_s = (uint64_t*)(b + L.keys_s);
  w->idx = (uint32_t*)(b + L.idx);       w->idx_s = (uint32_t*)(b + L.idx_s);
  w->sxyz = (double*)(b + L.sxyz);       w->pos = (uint32_t*)(b + L.pos);
  w->ukeys = (uint64_t*)(b + L.ukeys);   w->ustart = (uint32_t*)(b + L.ustart);
  w->part = (double*)(b + L.part);       w->avg = (double*)(b + L.avg);
  w->far = (uint32_t*)(b + L.far);       w->temp = b + L.temp;
  w->temp_bytes = L.temp_bytes;
  return SLG_OK;
}

// keys -> stable sort by key (so by original index within a key) -> sorted points -> cell table,
// with the cell size the header holds.
int build_grid(const double* xyz, int64_t n, const Ws& w, hipStream_t st) {
  const int g = grid_of(n, 256);
  keys_kernel<<<g, 256, 0, st>>>(xyz, n, w.hdr, w.keys, w.idx);
  size_t tb = w.temp_bytes;
  if (rocprim::radix_sort_pairs(w.temp, tb, (const uint64_t*)w.keys, w.keys_s, (const uint32_t*)w.idx, w.idx_s,
                                (size_t)n, 0u, 63u, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "cloud filter: radix sort failed");
  gather_flags_kernel<<<g, 256, 0, st>>>(xyz, n, w.hdr, w.keys_s, w.idx_s, w.sxyz, w.idx);   // idx: the flags
  tb = w.temp_bytes;
  if (rocprim::exclusive_scan(w.temp, tb, (const uint32_t*)w.idx, w.pos, 0u, (size_t)n, rocprim::plus<uint32_t>(),
                              st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "cloud filter: scan failed");
  table_kernel<<<g, 256, 0, st>>>(n, w.hdr, w.keys_s, w.pos, w.ukeys, w.ustart);
  return check_launch("cloud filter grid build");
}

int bbox(const double* xyz, int64_t n, const Ws& w, double cell, int k, hipStream_t st) {
  if (hipMemsetAsync(w.hdr, 0, 256, st) != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "cloud filter: memset failed");
  const int nb = grid_of(n, kChunk);
  bbox_partial_kernel<<<nb, 256, 0, st>>>(xyz, n, w.hdr, w.part);
  bbox_final_kernel<<<1, 256, 0, st>>>(w.part, nb, w.hdr, cell, n, k);
  return check_launch("cloud filter bounding box");
}

constexpr int64_t kMaxPoints = 1ll << 30;    // 32-bit sorted indices and offsets

}  // namespace

extern "C" {

int64_t slg_filter_ws_bytes(int64_t n, int32_t k) {
  if (n <= 0 || k < 0) return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_filter_ws_bytes: n <= 0 or k < 0");
  if (n > kMaxPoints || k > kMaxK)
    return -(int64_t)slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_filter_ws_bytes: more than 2^30 points or k > %d", kMaxK);
  size_t tb = 0;
  if (temp_bytes_for(n, &tb) != hipSuccess)
    return -(int64_t)slg_internal_fail(SLG_ERR_HIP, "slg_filter_ws_bytes: rocPRIM size query failed");
  return (int64_t)make_layout(n, tb).total;
}

int32_t slg_radius_outlier(const double* xyz, int64_t n, double radius, int32_t nb_points, void* ws, int64_t ws_bytes,
                           uint8_t* keep_out, int32_t* counts_out, void* stream) {
  if (n <= 0 || !(radius > 0.0) || !xyz || !keep_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_radius_outlier: n <= 0, radius <= 0 or a NULL buffer");
  if (n > kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_radius_outlier: more than 2^30 points");
  Ws w;
  int rc = bind_ws("slg_radius_outlier", n, ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // cell = radius, widened by 2^-20: a pair the rule counts has |dx| < radius (1 + 2^-50), so its
  // cell coordinates differ by less than 1 - 2^-20 + 2^-28 (the rounding of two coordinates below
  // 2^21) and the pair always shares a 3x3x3 block, also when points sit exactly on cell faces
  if ((rc = bbox(xyz, n, w, radius * (1.0 + 0x1p-20), 0, st))) return rc;
  if ((rc = build_grid(xyz, n, w, st))) return rc;
  const int64_t g = n < 8192 ? n : 8192;
  radius_count_kernel<<<(int)g, 256, 0, st>>>(w.hdr, w.sxyz, w.idx_s, w.ukeys, w.ustart, radius * radius, nb_points,
                                              keep_out, counts_out);
  return check_launch("radius_count_kernel");
}

int32_t slg_statistical_outlier(const double* xyz, int64_t n, int32_t nb_neighbors, double std_ratio, void* ws,
                                int64_t ws_bytes, uint8_t* keep_out, double* avg_out, double* stats_out,
                                void* stream) {
  if (n <= 0 || nb_neighbors < 1 || !xyz || !keep_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_statistical_outlier: n <= 0, nb_neighbors < 1 or a NULL buffer");
  if (nb_neighbors > kMaxK)
    return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_statistical_outlier: nb_neighbors > %d", kMaxK);
  if (n > kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_statistical_outlier: more than 2^30 points");
  Ws w;
  int rc = bind_ws("slg_statistical_outlier", n, ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int k = nb_neighbors;
  if ((rc = bbox(xyz, n, w, 0.0, k, st))) return rc;
  for (int pass = 0; pass < 3; ++pass) {       // first guess, then two occupancy refinements
    if (pass) knn_refine_kernel<<<1, 1, 0, st>>>(w.hdr, n, k);
    if ((rc = build_grid(xyz, n, w, st))) return rc;
  }
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

int32_t slg_dbscan(const double* xyz, int64_t n, double eps, int32_t min_points, void* ws, int64_t ws_bytes,
                   int32_t* labels_out, uint8_t* largest_keep_out, int32_t* info_out, void* stream) {
  if (n <= 0 || !(eps > 0.0) || min_points < 0 || !xyz || !labels_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_dbscan: n <= 0, eps <= 0, min_points < 0 or a NULL buffer");
  if (n > kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_dbscan: more than 2^30 points");
  Ws w;
  int rc = bind_ws("slg_dbscan", n, ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // The scratch lives in regions the radius path leaves idle: avg (counts, core words), far
  // (parent), and keys / keys_s / idx / pos once the grid is built.
  int32_t* cnt = (int32_t*)w.avg;
  uint32_t* scidx = (uint32_t*)w.avg + n;
  uint32_t* parent = w.far;
  uint32_t* root = (uint32_t*)w.keys_s;
  uint32_t* sroot = (uint32_t*)w.keys_s + n;
  int32_t* sizes = (int32_t*)w.keys;
  uint8_t* keep_scratch = (uint8_t*)((uint32_t*)w.keys + n);
  uint32_t* flags = w.idx;
  if ((rc = bbox(xyz, n, w, eps * (1.0 + 0x1p-20), 0, st))) return rc;     // the radius filter's cell
  if ((rc = build_grid(xyz, n, w, st))) return rc;
  const double r2 = eps * eps;
  const int cells = (int)(n < 8192 ? n : 8192);
  const int g = grid_of(n, 256);
  radius_count_kernel<<<cells, 256, 0, st>>>(w.hdr, w.sxyz, w.idx_s, w.ukeys, w.ustart, r2, 0, keep_scratch, cnt);
  dbscan_core_kernel<<<g, 256, 0, st>>>(w.hdr, n, w.idx_s, cnt, min_points, scidx, parent, sizes);
  dbscan_subcell_kernel<<<cells, 256, 0, st>>>(w.hdr, w.sxyz, scidx, w.ukeys, w.ustart, parent);
  dbscan_union_kernel<<<cells, 256, 0, st>>>(w.hdr, w.sxyz, scidx, w.ukeys, w.ustart, r2, parent);
  dbscan_flatten_kernel<<<g, 256, 0, st>>>(w.hdr, n, cnt, min_points, parent, root, flags);
  size_t tb = w.temp_bytes;
  if (rocprim::exclusive_scan(w.temp, tb, (const uint32_t*)flags, w.pos, 0u, (size_t)n, rocprim::plus<uint32_t>(),
                              st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "slg_dbscan: scan failed");
  dbscan_sroot_kernel<<<g, 256, 0, st>>>(w.hdr, n, w.idx_s, root, flags, w.pos, sroot);
  dbscan_border_kernel<<<cells, 256, 0, st>>>(w.hdr, w.sxyz, w.idx_s, sroot, cnt, w.pos, w.ukeys, w.ustart, r2,
                                              labels_out);
  dbscan_sizes_kernel<<<g, 256, 0, st>>>(w.hdr, n, labels_out, sizes);
  dbscan_argmax_kernel<<<g, 256, 0, st>>>(w.hdr, sizes);
  dbscan_keep_kernel<<<g, 256, 0, st>>>(w.hdr, n, labels_out, largest_keep_out, info_out);
  return check_launch("slg_dbscan");
}

int32_t slg_cloud_select(const double* xyz, const uint8_t* bgr, int64_t n, const uint8_t* keep, const slg_cloud* out,
                         int64_t* index_out, void* ws, void* stream) {
  if (n <= 0 || !xyz || !keep || !out || !out->xyz || !out->count)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_cloud_select: n <= 0 or a NULL buffer");
  if (n > kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_cloud_select: more than 2^30 points");
  Ws w;
  int rc = bind_ws("slg_cloud_select", n, ws, -1, &w);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  size_t tb = w.temp_bytes;
  auto it = rocprim::make_transform_iterator(keep, U8ToU32());
  if (rocprim::exclusive_scan(w.temp, tb, it, w.pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "slg_cloud_select: scan failed");
  select_kernel<<<grid_of(n, 256), 256, 0, st>>>(xyz, bgr, n, keep, w.pos, (double*)out->xyz, out->bgr, out->count,
                                                out->capacity, index_out);
  return check_launch("select_kernel");
}

int32_t slg_voxel_downsample(const double* xyz, const uint8_t* bgr, int64_t n, double voxel_size, void* ws,
                             int64_t ws_bytes, double* xyz_out, uint8_t* bgr_out, int64_t* first_index_out,
                             int32_t* count_out, int64_t* m_out, void* stream) {
  if (n <= 0 || !(voxel_size > 0.0) || !isfinite(voxel_size) || !xyz || !xyz_out || !m_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_voxel_downsample: n <= 0, voxel_size not finite and > 0, or a NULL buffer");
  if (n > kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_voxel_downsample: more than 2^30 points");
  Ws w;
  int rc = bind_ws("slg_voxel_downsample", n, ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = bbox(xyz, n, w, 0.0, 0, st))) return rc;       // the box; voxel_setup_kernel fixes origin and cell
  voxel_setup_kernel<<<1, 1, 0, st>>>(w.hdr, voxel_size);
  if ((rc = build_grid(xyz, n, w, st))) return rc;
  // keys is idle once sorted: the head flags and their scan live there
  uint32_t* head = (uint32_t*)w.keys;
  uint32_t* place = (uint32_t*)w.keys + n;
  const int g = grid_of(n, 256);
  voxel_heads_kernel<<<g, 256, 0, st>>>(w.hdr, n, w.keys_s, w.idx_s, head);
  size_t tb = w.temp_bytes;
  if (rocprim::exclusive_scan(w.temp, tb, (const uint32_t*)head, place, 0u, (size_t)n, rocprim::plus<uint32_t>(), st) !=
      hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "slg_voxel_downsample: scan failed");
  const VoxelOut out{xyz_out, bgr ? bgr_out : nullptr, first_index_out, count_out};
  voxel_reduce_kernel<<<g, 256, 0, st>>>(w.hdr, w.sxyz, w.idx_s, bgr, w.ustart, place, w.far, out, m_out);
  voxel_long_kernel<<<(int)(n < 1024 ? n : 1024), 64, 0, st>>>(w.hdr, w.sxyz, w.idx_s, bgr, w.ustart, place, w.far, out);
  return check_launch("slg_voxel_downsample");
}

int32_t slg_estimate_normals(const double* xyz, int64_t n, double radius, int32_t max_nn, void* ws, int64_t ws_bytes,
                             double* normals_out, double* cov_out, int32_t* m_out, void* stream) {
  if (n <= 0 || !(radius > 0.0) || !isfinite(radius) || max_nn < 3 || !xyz || !normals_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_estimate_normals: n <= 0, radius not finite and > 0, max_nn < 3 or a NULL buffer");
  if (max_nn > kMaxK) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_estimate_normals: max_nn > %d", kMaxK);
  if (n > kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_estimate_normals: more than 2^30 points");
  Ws w;
  int rc = bind_ws("slg_estimate_normals", n, ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int k = max_nn;
  if ((rc = bbox(xyz, n, w, 0.0, k, st))) return rc;
  for (int pass = 0; pass < 3; ++pass) {       // the kNN grid, as slg_statistical_outlier builds it
    if (pass) knn_refine_kernel<<<1, 1, 0, st>>>(w.hdr, n, k);
    if ((rc = build_grid(xyz, n, w, st))) return rc;
  }
  const size_t lds = (size_t)(n < k ? n : k) * 64 * (sizeof(double) + sizeof(uint32_t));
  const double r2 = radius * radius;
  normals_kernel<<<grid_of(n, 64), 64, lds, st>>>(w.hdr, xyz, w.sxyz, w.idx_s, w.ukeys, w.ustart, n, k, r2, normals_out,
                                                  cov_out, m_out, w.far);
  normals_far_kernel<<<(int)(n < 1024 ? n : 1024), 64, lds, st>>>(w.hdr, xyz, w.sxyz, w.idx_s, n, k, r2, normals_out,
                                                                  cov_out, m_out, w.far);
  return check_launch("slg_estimate_normals");
}

int32_t slg_orient_normals(const double* xyz, double* normals, int64_t n, const double* location, int32_t outward,
                           void* stream) {
  if (n <= 0 || !xyz || !normals || !location)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_orient_normals: n <= 0 or a NULL buffer");
  if (n > kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_orient_normals: more than 2^30 points");
  orient_kernel<<<grid_of(n, 256), 256, 0, (hipStream_t)stream>>>(xyz, normals, n, location, outward);
  return check_launch("orient_kernel");
}

int32_t slg_cloud_centroid(const double* xyz, int64_t n, void* ws, int64_t ws_bytes, double* centroid_out,
                           void* stream) {
  if (n <= 0 || !xyz || !centroid_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_cloud_centroid: n <= 0 or a NULL buffer");
  if (n > kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_cloud_centroid: more than 2^30 points");
  Ws w;
  int rc = bind_ws("slg_cloud_centroid", n, ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(n, kChunk);
  axis_sum_partial_kernel<<<nb, 256, 0, st>>>(xyz, n, w.part);
  axis_sum_final_kernel<<<1, 256, 0, st>>>(w.part, nb, n, centroid_out);
  return check_launch("slg_cloud_centroid");
}

}  // extern "C"
