// cloud_grid.h -- what the device cloud steps share (included, never compiled alone): the
// workspace header, the bump allocator every workspace layout is written with, the prologue of a
// call whose workspace is a grid with an extension behind it, the sparse uniform grid's device
// helpers, the two neighbour walks, the top-k lists, the wave-wide merge of 64 such lists and the
// list kernels' bodies built on it, the seeded draw, and the host functions of cloud_grid.hip.
// Users: cloud_filter.hip (radius count, statistical filter), cloud_cluster.hip (DBSCAN),
// cloud_normals.hip (voxel down-sample, normals), cloud_icp.hip (point-to-plane ICP's
// correspondence search), cloud_feature.hip (FPFH's neighbour lists), cloud_ransac.hip (the draws
// and the evaluation of a batch of hypotheses), cloud_plane.hip (the draws), cloud_orient.hip (the
// kNN lists and the EMST's walks of the tangent-plane orientation), cloud_mesh.hip (the allocator).
//
// The grid: bbox (fixed-order reduction) -> integer cell coordinates floor((p - min) / cell)
// packed into a 63-bit key (21 bits per axis, x lowest) -> stable radix sort of (key, index) ->
// points gathered in sorted order -> table of unique keys + start offsets (binary search).  x is
// the lowest key field, so the cells x0..x1 of one (y, z) row are one contiguous range of the
// sorted cloud: a 3x3x3 neighbourhood is 9 ranges.  No dense cell array exists, so far outliers
// (row_mode 2 clouds) cost nothing.
//
// Everything is separate launches on the caller's stream; no workgroup waits for another and
// nothing synchronises with the host.  Conditions only the device can see (a non-finite
// coordinate, an axis of 2^21 cells or more) set a status word at the front of the workspace;
// every later kernel of the call reads it and returns, so a bad input ends in the flag.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "internal.h"

namespace slgcloud {

constexpr int kCellBits = 21;
constexpr int64_t kCellMax = (1ll << kCellBits) - 1;
constexpr int kMaxK = 64;
constexpr int kTile = 1024;        // candidate points staged in LDS per tile (24 KB)
constexpr int kChunk = 2048;       // points per workgroup in the fixed-order reductions
constexpr int kMaxRing = 6;        // Chebyshev rings the kNN walk takes before the whole-cloud kernel
constexpr double kInf = __builtin_huge_val();
constexpr uint32_t kNone = 0xFFFFFFFFu;      // no index: not a core point, no root, an empty list head
constexpr int64_t kMaxPoints = 1ll << 30;    // 32-bit sorted indices and offsets

// ---------------------------------------------------------------- the shared rules
// Squared distance: the same expression, in the same order, as tests/cloud_ref.py:d2.
__device__ inline double d2_rule(double dx, double dy, double dz) { return (dx * dx + dy * dy) + dz * dz; }
// A neighbour counts when d2 < radius^2 (strict); the point itself counts.
__device__ inline bool radius_neighbour_rule(double d2, double r2) { return d2 < r2; }

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
static_assert(offsetof(Hdr, status) == 0, "cloud.py reads the status word at byte 0");
static_assert(offsetof(Hdr, n_far) == 8, "cloud.py reads n_far at byte 8 (far_count)");

struct Ws {             // the regions of make_layout (cloud_grid.hip), bound to a caller's workspace
  Hdr* hdr;
  uint64_t *keys, *keys_s, *ukeys;
  uint32_t *idx, *idx_s, *pos, *ustart, *far;
  double *sxyz, *part, *avg;
  void* temp;
  size_t temp_bytes;
};

// Scratch of slg_dbscan and slg_voxel_downsample in regions their grid leaves idle (cloud_grid.hip).
struct DbscanScratch {
  int32_t* cnt;
  uint32_t *scidx, *parent, *root, *sroot;
  int32_t* sizes;
  uint8_t* keep;
  uint32_t* flags;
};
struct VoxelScratch { uint32_t *head, *place; };

inline int grid_of(int64_t n, int per) { return (int)((n + per - 1) / per); }

// Every workspace layout: regions in order from byte `start` of the workspace at `base`, each a
// multiple of 256 bytes; off is the total so far.  A null base only sizes.  The grid's layout
// starts at 0, an extension's at up256(grid bytes), the mesher's behind its header.
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
struct Bump {
  uintptr_t base;
  size_t off;
  Bump(void* ws, size_t start) : base((uintptr_t)ws), off(start) {}
  template <class T> T* take(size_t count) {
    T* p = (T*)(base + off);
    off = up256(off + count * sizeof(T));
    return p;
  }
};

// ---------------------------------------------------------------- host side (cloud_grid.hip)
// The point cap and the workspace binding every entry point starts with.
int begin_call(const char* who, int64_t n, void* ws, int64_t ws_bytes, Ws* w);

// The bytes of a grid workspace of (n, k) with the regions layout(Bump&) takes behind it: what an
// extension's slg_*_ws_bytes returns after its own refusals (the grid's error code, negated, when
// the grid refuses).
template <class Layout>
int64_t ext_ws_bytes(int64_t n, int k, Layout layout) {
  const int64_t grid_bytes = slg_filter_ws_bytes(n, k);
  if (grid_bytes < 0) return grid_bytes;
  Bump b(nullptr, up256((size_t)grid_bytes));
  layout(b);
  return (int64_t)b.off;
}
// begin_call for such a workspace: the grid's bytes (its own error is passed on, its text already
// set), the grid bound to the front of ws, layout(Bump&) behind it, and ws_bytes against the
// total; `sizer` is the slg_*_ws_bytes the text names.
template <class Layout>
int begin_ext_call(const char* who, const char* sizer, int64_t n, int k, void* ws, int64_t ws_bytes, Ws* grid,
                   Layout layout) {
  const int64_t grid_bytes = slg_filter_ws_bytes(n, k);
  if (grid_bytes < 0) return (int32_t)-grid_bytes;
  if (int rc = begin_call(who, n, ws, -1, grid)) return rc;
  Bump b(ws, up256((size_t)grid_bytes));
  layout(b);
  if (ws_bytes < 0 || (size_t)ws_bytes < b.off)
    return slg_internal_fail(SLG_ERR_INVALID, "%s: workspace of %lld bytes, %s gives %lld", who, (long long)ws_bytes, sizer,
                             (long long)b.off);
  return SLG_OK;
}
DbscanScratch dbscan_scratch(const Ws& w, int64_t n);
VoxelScratch voxel_scratch(const Ws& w, int64_t n);
// Clears the header, folds the box and fixes the cell (bbox_final_kernel says how).
int bbox(const double* xyz, int64_t n, const Ws& w, double cell, int k, hipStream_t st);
// keys -> stable sort by (key, index) -> sorted points -> cell table, with the header's cell size.
int build_grid(const double* xyz, int64_t n, const Ws& w, hipStream_t st);
// The kNN grid: the box, the first guess of the cell and two occupancy refinements.
int knn_grid(const double* xyz, int64_t n, const Ws& w, int k, hipStream_t st);
// out = exclusive sum of in[0..n) through the workspace's rocPRIM scratch.
int scan_u32(const char* who, const Ws& w, const uint32_t* in, uint32_t* out, int64_t n, hipStream_t st);
// Launches the radius count on a built grid (cloud_filter.hip); slg_dbscan starts from it too.
void radius_count(const Ws& w, int64_t n, double r2, int32_t nb, uint8_t* keep, int32_t* counts, hipStream_t st);

// ---------------------------------------------------------------- grid helpers
__device__ inline int64_t cell_coord(double p, double mn, double cell) {
  const double c = floor((p - mn) / cell);
  if (!(c > 0.0)) return 0;                 // also NaN
  return c > (double)kCellMax ? kCellMax : (int64_t)c;
}
__device__ inline uint64_t pack_key(int64_t x, int64_t y, int64_t z) {
  return ((uint64_t)z << (2 * kCellBits)) | ((uint64_t)y << kCellBits) | (uint64_t)x;
}
__device__ inline void unpack_key(uint64_t key, int64_t* c) {
  c[0] = key & kCellMax;
  c[1] = (key >> kCellBits) & kCellMax;
  c[2] = (key >> (2 * kCellBits)) & kCellMax;
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
// The 9 row ranges of the 3x3x3 block around cell `key` (threads 0..8).
__device__ inline void block_ranges(const Hdr* hdr, const uint64_t* __restrict__ ukeys,
                                    const uint32_t* __restrict__ ustart, int nu, uint64_t key, uint32_t (*rng)[2]) {
  const int t = threadIdx.x;
  if (t >= 9) return;
  int64_t c[3];
  unpack_key(key, c);
  const int64_t y = c[1] + (t % 3) - 1, z = c[2] + (t / 3) - 1;
  uint32_t s = 0, e = 0;
  if (y >= 0 && y <= hdr->cmax[1] && z >= 0 && z <= hdr->cmax[2])
    row_range(ukeys, ustart, nu, c[0] > 0 ? c[0] - 1 : 0, c[0] < hdr->cmax[0] ? c[0] + 1 : c[0], y, z, &s, &e);
  rng[t][0] = s;
  rng[t][1] = e;
}

// ---------------------------------------------------------------- fixed-order trees (256 threads)
// Σ v over the workgroup as a binary tree in sm[256]; every thread gets the sum.
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
// min of lo[0..2] and max of hi[0..2] over the workgroup: the results are sm[a][0] and sm[3 + a][0].
__device__ inline void block_tree_minmax(const double* lo, const double* hi, double (*sm)[256]) {
  const int t = threadIdx.x;
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
}
__device__ inline double wave_min(double v) {
  for (int s = 32; s > 0; s >>= 1) v = fmin(v, __shfl_xor(v, s, 64));
  return v;
}

// ---------------------------------------------------------------- the block walk
// One workgroup per occupied cell (grid-stride): the 9 ranges of the cell's block into rng, then
// batch(qb, qe) for the cell's points [qb, qe) 256 at a time; thread t's query is qb + t.
template <class Batch>
__device__ inline void cell_batches(const Hdr* hdr, const uint64_t* __restrict__ ukeys,
                                    const uint32_t* __restrict__ ustart, uint32_t (*rng)[2], Batch batch) {
  if (hdr->status) return;
  const int nu = hdr->n_unique;
  for (int u = blockIdx.x; u < nu; u += gridDim.x) {
    const uint32_t qs = ustart[u], qe = ustart[u + 1];
    __syncthreads();                         // the previous cell's ranges are no longer read
    block_ranges(hdr, ukeys, ustart, nu, ukeys[u], rng);
    __syncthreads();
    for (uint32_t qb = qs; qb < qe; qb += 256) batch(qb, qe);
  }
}
// One batch of queries (one per thread, at (px, py, pz)) against the 9 ranges.  The candidates are
// staged through LDS in tiles of kTile points and read back as broadcasts (every lane the same
// address), so the inner loop is fp64 VALU fed from LDS.  stage(w, j) stages whatever words the
// kernel keeps beside the coordinates for tile slot w = sorted position j; cand(w, d2) sees every
// candidate of the tile.  A wave whose `gate` is off (none of its lanes holds a query that needs
// the walk) only stages and takes the barriers.  Every thread of the workgroup must call this.
template <bool kUnroll4, class Stage, class Cand>
__device__ inline void block_walk(const uint32_t (*rng)[2], const double* __restrict__ sxyz, double* tile, bool gate,
                                  double px, double py, double pz, Stage stage, Cand cand) {
  const int t = threadIdx.x;
  for (int r = 0; r < 9; ++r) {
    const uint32_t s = rng[r][0], e = rng[r][1];
    for (uint32_t tb = s; tb < e; tb += kTile) {
      const int m = (int)(e - tb < (uint32_t)kTile ? e - tb : (uint32_t)kTile);
      __syncthreads();                       // the previous tile has been consumed
      for (int w = t; w < 3 * m; w += 256) tile[w] = sxyz[3 * (size_t)tb + w];
      for (int w = t; w < m; w += 256) stage(w, tb + w);
      __syncthreads();
      if (!gate) continue;
      if constexpr (kUnroll4) {
#pragma unroll 4
        for (int j = 0; j < m; ++j) cand(j, d2_rule(tile[3 * j] - px, tile[3 * j + 1] - py, tile[3 * j + 2] - pz));
      } else {
        for (int j = 0; j < m; ++j) cand(j, d2_rule(tile[3 * j] - px, tile[3 * j + 1] - py, tile[3 * j + 2] - pz));
      }
    }
  }
}

// ---------------------------------------------------------------- top-k lists
// Per-lane top-kk lists in LDS, lst[j * 64 + lane] (lanes on consecutive addresses): unsorted
// while filling, with the largest entry tracked; once full, a smaller entry replaces the largest
// and the list is rescanned for the new one.  TopK orders by d2 alone; TopKI keeps the original
// index beside the distance (idx[j * 64 + lane] after the kk * 64 distances) and orders by
// (d2, index).  offer(d, sidx, j) is what the walks call for the candidate at sorted position j.
// Two types on purpose: the rescans differ (v > m from -1, against the pair order).
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
  __device__ inline void offer(double d, const uint32_t* __restrict__, size_t) { insert(d); }
  __device__ inline void sort() {            // ascending insertion sort of the cnt entries
    for (int a = 1; a < cnt; ++a) {
      const double v = lst[a * 64];
      int b = a - 1;
      while (b >= 0 && lst[b * 64] > v) { lst[(b + 1) * 64] = lst[b * 64]; --b; }
      lst[(b + 1) * 64] = v;
    }
  }
};

__device__ inline bool pair_before_rule(double a, uint32_t ai, double b, uint32_t bi) {
  return a < b || (a == b && ai < bi);
}

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
  __device__ inline void offer(double d, const uint32_t* __restrict__ sidx, size_t j) {
    if (wants(d)) insert(d, sidx[j]);
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

// The wave-wide merge of the 64 sorted per-lane lists of a whole-cloud kernel: kk times, the
// smallest (d2, index) head over the wave is taken, the lane that holds it advances, and
// emit(r, d2, index) sees entry r of the merged list (in every lane).  Returns the number taken.
// With kRadius the lists can be used up before kk are taken (fewer than kk points inside the
// radius) and the merge ends there; without it the lists hold the best kk <= n of the whole
// cloud, so they never are, and the test is left out.
template <bool kRadius, class Emit>
__device__ inline int wave_merge(const TopKI& tk, int kk, Emit emit) {
  int head = 0, r = 0;
  for (; r < kk; ++r) {
    const bool have = head < tk.cnt;
    const double v = have ? tk.lst[head * 64] : kInf;
    const uint32_t vi = have ? tk.idx[head * 64] : kNone;
    const double best = wave_min(v);
    if constexpr (kRadius) {
      if (best == kInf) break;                 // every list is used up (uniform over the wave)
    }
    uint32_t bi = v == best ? vi : kNone;
    for (int s = 32; s > 0; s >>= 1) {
      const uint32_t other = (uint32_t)__shfl_xor((int)bi, s, 64);
      bi = other < bi ? other : bi;
    }
    if (have && v == best && vi == bi) ++head;
    emit(r, best, bi);
  }
  return r;
}

// ---------------------------------------------------------------- the ring walk
// Offers the sorted positions s, s + step, ... below e to the list; with kRadius only those with
// d2 < r2.
template <bool kRadius, class List>
__device__ inline void scan_range(List& tk, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                                  uint32_t s, uint32_t e, uint32_t step, const double* p, double r2) {
  for (uint32_t j = s; j < e; j += step) {
    const double d = d2_rule(sxyz[3 * (size_t)j] - p[0], sxyz[3 * (size_t)j + 1] - p[1], sxyz[3 * (size_t)j + 2] - p[2]);
    if (!kRadius || radius_neighbour_rule(d, r2)) tk.offer(d, sidx, j);
  }
}

// The nearest neighbours of the query p, one query per thread: cells in
// Chebyshev rings around the query's cell until the list is full and its largest d2 is no larger
// than the squared distance to the nearest face of the block searched (faces at or past the
// cloud's box do not count: nothing lies beyond them).  The face distance gives up the header's
// absolute slack and a relative 1e-12, so rounding in the cell coordinates cannot end the walk
// early.  With kRadius a candidate enters only with d2 < r2, and the walk also ends once the
// block searched covers the radius ball (r2 no larger than the squared face distance), so a point
// with fewer than kk neighbours inside the radius stops as soon as nothing further out could
// count.  False when the point is still open after kMaxRing rings: it goes to the caller's
// whole-cloud kernel.
//
// kOutside: the query need not be a point of the grid and may lie outside its box (the ICP's
// transformed source points).  Its cell is then clamped into [0, cmax] per axis, and the face
// bound stays a lower bound on the distance to everything not yet searched: on an axis where the
// query lies beyond the box, the block's face on that side is at or past the box, so it is left
// out as before (nothing lies beyond it), and the opposite face's plane lies between the query
// and every point past it, so the query's distance to that plane, which is what the expression
// below computes, is no larger than the distance to any such point.  The rounding of that
// distance is relative to the query's coordinate; where that exceeds the header's slack (a query
// far outside), the bound itself is of the coordinate's size and the relative 1e-12 covers it.
template <bool kRadius, bool kOutside, class List>
__device__ inline bool ring_walk_at(const Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                                    const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ustart,
                                    const double* p, double r2, List& tk) {
  const int nu = hdr->n_unique;
  const double h = hdr->cell;
  int64_t c[3], cm[3];
  for (int a = 0; a < 3; ++a) {
    c[a] = cell_coord(p[a], hdr->mn[a], h);
    cm[a] = hdr->cmax[a];
    if (kOutside && c[a] > cm[a]) c[a] = cm[a];
  }
  bool done = false;
  for (int R = 0; R <= kMaxRing && !done; ++R) {
    for (int dz = -R; dz <= R; ++dz) {
      const int64_t z = c[2] + dz;
      if (z < 0 || z > cm[2]) continue;
      for (int dy = -R; dy <= R; ++dy) {
        const int64_t y = c[1] + dy;
        if (y < 0 || y > cm[1]) continue;
        auto cells = [&](int64_t x0, int64_t x1) {
          uint32_t s, e;
          row_range(ukeys, ustart, nu, x0, x1, y, z, &s, &e);
          scan_range<kRadius>(tk, sxyz, sidx, s, e, 1, p, r2);
        };
        if (abs(dy) == R || abs(dz) == R) {  // a whole row of the shell
          cells(c[0] - R < 0 ? 0 : c[0] - R, c[0] + R > cm[0] ? cm[0] : c[0] + R);
        } else {                             // the row's two end cells
          if (c[0] - R >= 0) cells(c[0] - R, c[0] - R);
          if (c[0] + R <= cm[0]) cells(c[0] + R, c[0] + R);
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
    } else if (kRadius || tk.cnt == tk.kk) {
      const double b = fmax(bound - hdr->slack, 0.0);
      const double b2 = (b * b) * (1.0 - 1e-12);
      done = (kRadius && r2 <= b2) || (tk.cnt == tk.kk && tk.curmax <= b2);
    }
  }
  return done;
}

// The walk for the grid's own point at sorted position q (it lies inside the box).
template <bool kRadius, class List>
__device__ inline bool ring_walk(const Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                                 const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ustart, int64_t q,
                                 double r2, List& tk) {
  const double p[3] = {sxyz[3 * q], sxyz[3 * q + 1], sxyz[3 * q + 2]};
  return ring_walk_at<kRadius, false>(hdr, sxyz, sidx, ukeys, ustart, p, r2, tk);
}

// ---------------------------------------------------------------- neighbour lists in global memory
// What FPFH (cloud_feature.hip, kRadius: the hybrid search) and the tangent-plane orientation
// (cloud_orient.hip, plain kNN) keep per point: a (d2, index) list sorted ascending, 64 queries to
// a block of kk x 64 entries (entry j of lane l at j * 64 + l, the layout TopKI walks), and with
// kRadius the number of entries of the list of sorted position q in cnt (without the radius every
// list holds kk <= n entries and cnt is not touched: pass null).  Each file has the two kernels
// that call these bodies.
//
// One query per thread (64 to a workgroup) at sorted position q: the ring walk with the list in
// global memory, sorted in place.  Queries open after kMaxRing rings go to the far list (at most
// one entry per point: n entries) and lists_far_body.
template <bool kRadius>
__device__ inline void lists_body(Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                                  const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ustart, int64_t n,
                                  int kk, double r2, double* lst_d, uint32_t* lst_i, int32_t* __restrict__ cnt,
                                  uint32_t* __restrict__ far) {
  if (hdr->status) return;
  const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (q >= n) return;
  const size_t base = (size_t)blockIdx.x * kk * 64 + threadIdx.x;
  TopKI tk{lst_d + base, lst_i + base, kk, 0, 0, -1.0, 0u};
  if (!ring_walk<kRadius>(hdr, sxyz, sidx, ukeys, ustart, q, r2, tk)) {
    far[atomicAdd(&hdr->n_far, 1)] = (uint32_t)q;
    return;
  }
  tk.sort();
  if constexpr (kRadius) cnt[q] = tk.cnt;
}

// One wave per far-list query (grid-stride), each workgroup with kk x 64 entries of scratch at
// far_d / far_i: each lane keeps the best kk of its stride of the whole cloud, wave_merge takes
// the smallest (d2, index) head kk times, and lane 0 writes the merged list into the query's slot.
template <bool kRadius>
__device__ inline void lists_far_body(const Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                                      int64_t n, int kk, double r2, double* far_d, uint32_t* far_i, double* lst_d,
                                      uint32_t* lst_i, int32_t* __restrict__ cnt, const uint32_t* __restrict__ far) {
  if (hdr->status) return;
  const int lane = threadIdx.x;
  const int nf = hdr->n_far;
  const size_t scratch = (size_t)blockIdx.x * kk * 64 + lane;
  for (int f = blockIdx.x; f < nf; f += gridDim.x) {
    const int64_t q = far[f];
    const double p[3] = {sxyz[3 * q], sxyz[3 * q + 1], sxyz[3 * q + 2]};
    TopKI tk{far_d + scratch, far_i + scratch, kk, 0, 0, -1.0, 0u};
    scan_range<kRadius>(tk, sxyz, sidx, lane, (uint32_t)n, 64, p, r2);
    tk.sort();
    const size_t slot = (size_t)(q / 64) * kk * 64 + (size_t)(q % 64);
    const int m = wave_merge<kRadius>(tk, kk, [&](int r, double d2, uint32_t i) {
      if (lane == 0) {
        lst_d[slot + (size_t)r * 64] = d2;
        lst_i[slot + (size_t)r * 64] = i;
      }
    });
    if constexpr (kRadius) {
      if (lane == 0) cnt[q] = m;
    }
  }
}

// ---------------------------------------------------------------- the seeded draw
// What the registration RANSAC (cloud_ransac.hip) and the plane RANSAC (cloud_plane.hip) draw
// their samples with; tests/feature_ref.py restates both.
// The finaliser of SplitMix64 (Steele, Lea, Flood 2014; Stafford's mix 13): integer operations only.
__device__ inline uint64_t mix64_rule(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// Draw k of trial t, with kStride draws reserved per trial: an index below m from the hash's upper
// 32 bits by a multiply-high.
template <int kStride>
__device__ inline uint32_t draw_rule(uint64_t seed, uint64_t t, uint32_t k, uint32_t m) {
  const uint64_t h = mix64_rule(mix64_rule(seed + 0x9E3779B97F4A7C15ull) + (t * (uint64_t)kStride + k));
  return (uint32_t)(((h >> 32) * (uint64_t)m) >> 32);
}

// ---------------------------------------------------------------- evaluating a transform
// What the ICP (cloud_icp.hip) and the RANSAC's batched evaluation (cloud_ransac.hip) share.
// PointCloud::Transform with a last row of 0 0 0 1: T is anything indexed 0..15, row-major.
template <class M>
__device__ inline void transform_point_rule(const M& T, const double* p, double* o) {
#pragma unroll
  for (int a = 0; a < 3; ++a) o[a] = ((T[4 * a] * p[0] + T[4 * a + 1] * p[1]) + T[4 * a + 2] * p[2]) + T[4 * a + 3];
}

// The correspondence of one query: the smallest (d2, target input index) among d2 < r2.  It has
// the members the walks read of a list (kk, cnt, curmax) and is held in registers.
struct Best1 {
  int kk, cnt;
  double curmax;
  uint32_t idx;
  __device__ inline void offer(double d, const uint32_t* __restrict__ sidx, size_t j) {
    if (cnt && d > curmax) return;
    const uint32_t i = sidx[j];
    if (!cnt || pair_before_rule(d, i, curmax, idx)) { curmax = d; idx = i; cnt = 1; }
  }
};

}  // namespace slgcloud
