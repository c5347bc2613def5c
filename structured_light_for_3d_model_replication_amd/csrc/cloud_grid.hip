// cloud_grid.hip -- the sparse uniform grid of the device cloud steps (cloud_grid.h says what it
// is): workspace layout and binding, bounding box, cell size, grid build, and the order-preserving
// select that follows the filters.  rocPRIM's 64-bit-key sort and 32-bit scans are instantiated
// here only; the other cloud files scan through scan_u32() (cloud_mesh.hip has its own types).
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "cloud_grid.h"

namespace slgcloud {

// ---------------------------------------------------------------- workspace
struct U8ToU32 {
  __host__ __device__ uint32_t operator()(uint8_t v) const { return v ? 1u : 0u; }
};

static hipError_t temp_bytes_for(int64_t n, size_t* out) {
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

// The regions of a workspace for n points at `base`, in order, each a multiple of 256 bytes;
// *total gets their sum (base may be null when only the size is wanted).
static Ws make_layout(void* base, int64_t n, size_t temp_bytes, size_t* total) {
  const size_t N = (size_t)n;
  Bump b(base, 0);
  Ws w;
  w.hdr = b.take<Hdr>(1);
  w.keys = b.take<uint64_t>(N);
  w.keys_s = b.take<uint64_t>(N);
  w.idx = b.take<uint32_t>(N);
  w.idx_s = b.take<uint32_t>(N);
  w.sxyz = b.take<double>(N * 3);
  w.pos = b.take<uint32_t>(N);
  w.ukeys = b.take<uint64_t>(N);
  w.ustart = b.take<uint32_t>(N + 1);
  w.part = b.take<double>(((N + kChunk - 1) / kChunk) * 6);
  w.avg = b.take<double>(N);
  w.far = b.take<uint32_t>(N);
  w.temp = b.take<uint8_t>(temp_bytes);
  w.temp_bytes = temp_bytes;
  *total = b.off;
  return w;
}

static int bind_ws(const char* who, int64_t n, void* ws, int64_t ws_bytes, Ws* w) {
  if (!ws || ((uintptr_t)ws & 7)) return slg_internal_fail(SLG_ERR_INVALID, "%s: workspace NULL or not 8-byte aligned", who);
  size_t tb = 0, total = 0;
  if (temp_bytes_for(n, &tb) != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "%s: rocPRIM size query failed", who);
  *w = make_layout(ws, n, tb, &total);
  if (ws_bytes >= 0 && (size_t)ws_bytes < total)
    return slg_internal_fail(SLG_ERR_INVALID, "%s: workspace of %lld bytes, slg_filter_ws_bytes gives %lld", who,
                             (long long)ws_bytes, (long long)total);
  return SLG_OK;
}

// slg_dbscan's scratch, in regions the radius path leaves idle; keys_s, keys and idx once the grid
// is built.  Each line: the region, its bytes per point, and what it holds.
DbscanScratch dbscan_scratch(const Ws& w, int64_t n) {
  static_assert(sizeof(int32_t) + sizeof(uint32_t) <= sizeof(*w.avg), "cnt + scidx in avg");
  static_assert(sizeof(uint32_t) <= sizeof(*w.far), "parent in far");
  static_assert(2 * sizeof(uint32_t) <= sizeof(*w.keys_s), "root + sroot in keys_s");
  static_assert(sizeof(int32_t) + sizeof(uint8_t) <= sizeof(*w.keys), "sizes + keep in keys");
  static_assert(sizeof(uint32_t) <= sizeof(*w.idx), "flags in idx");
  return DbscanScratch{(int32_t*)w.avg, (uint32_t*)w.avg + n,                     // avg, 8: cnt, scidx
                       w.far,                                                     // far, 4: parent
                       (uint32_t*)w.keys_s, (uint32_t*)w.keys_s + n,              // keys_s, 8: root, sroot
                       (int32_t*)w.keys, (uint8_t*)((uint32_t*)w.keys + n),       // keys, 8: sizes, keep
                       w.idx};                                                    // idx, 4: flags
}
// slg_voxel_downsample's scratch: keys (8 bytes per point) is idle once sorted, and holds the head
// flags, then their scan.
VoxelScratch voxel_scratch(const Ws& w, int64_t n) {
  static_assert(2 * sizeof(uint32_t) <= sizeof(*w.keys), "head + place in keys");
  return VoxelScratch{(uint32_t*)w.keys, (uint32_t*)w.keys + n};
}

namespace {

// ---------------------------------------------------------------- bounding box (fixed order)
__global__ __launch_bounds__(256)
void bbox_partial_kernel(const double* __restrict__ xyz, int64_t n, Hdr* hdr, double* __restrict__ part) {
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
  block_tree_minmax(lo, hi, sm);
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
__global__ __launch_bounds__(256)
void bbox_final_kernel(const double* __restrict__ part, int nb, Hdr* hdr, double cell_in, int64_t n, int k) {
  __shared__ double sm[6][256];
  const int t = threadIdx.x;
  double lo[3] = {kInf, kInf, kInf}, hi[3] = {-kInf, -kInf, -kInf};
  for (int b = t; b < nb; b += 256)
    for (int a = 0; a < 3; ++a) {
      lo[a] = fmin(lo[a], part[(int64_t)b * 6 + a]);
      hi[a] = fmax(hi[a], part[(int64_t)b * 6 + 3 + a]);
    }
  block_tree_minmax(lo, hi, sm);
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
__global__ __launch_bounds__(256)
void keys_kernel(const double* __restrict__ xyz, int64_t n, const Hdr* hdr, uint64_t* __restrict__ keys,
                 uint32_t* __restrict__ idx) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double cell = hdr->cell;
  keys[i] = pack_key(cell_coord(xyz[3 * i], hdr->mn[0], cell), cell_coord(xyz[3 * i + 1], hdr->mn[1], cell),
                     cell_coord(xyz[3 * i + 2], hdr->mn[2], cell));
  idx[i] = (uint32_t)i;
}

// Sorted copy of the points, and the run-start flags of the sorted keys.
__global__ __launch_bounds__(256)
void gather_flags_kernel(const double* __restrict__ xyz, int64_t n, const Hdr* hdr, const uint64_t* __restrict__ keys_s,
                         const uint32_t* __restrict__ idx_s, double* __restrict__ sxyz, uint32_t* __restrict__ flags) {
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
__global__ __launch_bounds__(256)
void table_kernel(int64_t n, Hdr* hdr, const uint64_t* __restrict__ keys_s, const uint32_t* __restrict__ pos,
                  uint64_t* __restrict__ ukeys, uint32_t* __restrict__ ustart) {
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

// ---------------------------------------------------------------- select
__global__ __launch_bounds__(256)
void select_kernel(const double* __restrict__ xyz, const uint8_t* __restrict__ bgr, int64_t n,
                   const uint8_t* __restrict__ keep, const uint32_t* __restrict__ pos, double* __restrict__ oxyz,
                   uint8_t* __restrict__ obgr, int64_t* __restrict__ count, int64_t capacity,
                   int64_t* __restrict__ index_out) {
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

}  // namespace

// ---------------------------------------------------------------- host side
int begin_call(const char* who, int64_t n, void* ws, int64_t ws_bytes, Ws* w) {
  if (n > kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "%s: more than 2^30 points", who);
  return bind_ws(who, n, ws, ws_bytes, w);
}

int scan_u32(const char* who, const Ws& w, const uint32_t* in, uint32_t* out, int64_t n, hipStream_t st) {
  size_t tb = w.temp_bytes;
  if (rocprim::exclusive_scan(w.temp, tb, in, out, 0u, (size_t)n, rocprim::plus<uint32_t>(), st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: scan failed", who);
  return SLG_OK;
}

int build_grid(const double* xyz, int64_t n, const Ws& w, hipStream_t st) {
  const int g = grid_of(n, 256);
  keys_kernel<<<g, 256, 0, st>>>(xyz, n, w.hdr, w.keys, w.idx);
  size_t tb = w.temp_bytes;
  if (rocprim::radix_sort_pairs(w.temp, tb, (const uint64_t*)w.keys, w.keys_s, (const uint32_t*)w.idx, w.idx_s,
                                (size_t)n, 0u, 63u, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "cloud filter: radix sort failed");
  gather_flags_kernel<<<g, 256, 0, st>>>(xyz, n, w.hdr, w.keys_s, w.idx_s, w.sxyz, w.idx);   // idx: the flags
  if (int rc = scan_u32("cloud filter", w, w.idx, w.pos, n, st)) return rc;
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

int knn_grid(const double* xyz, int64_t n, const Ws& w, int k, hipStream_t st) {
  int rc = bbox(xyz, n, w, 0.0, k, st);
  for (int pass = 0; pass < 3 && !rc; ++pass) {      // first guess, then two occupancy refinements
    if (pass) knn_refine_kernel<<<1, 1, 0, st>>>(w.hdr, n, k);
    rc = build_grid(xyz, n, w, st);
  }
  return rc;
}

}  // namespace slgcloud

using namespace slgcloud;

extern "C" int64_t slg_filter_ws_bytes(int64_t n, int32_t k) {
  if (n <= 0 || k < 0) return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_filter_ws_bytes: n <= 0 or k < 0");
  if (n > kMaxPoints || k > kMaxK)
    return -(int64_t)slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_filter_ws_bytes: more than 2^30 points or k > %d", kMaxK);
  size_t tb = 0, total = 0;
  if (temp_bytes_for(n, &tb) != hipSuccess)
    return -(int64_t)slg_internal_fail(SLG_ERR_HIP, "slg_filter_ws_bytes: rocPRIM size query failed");
  make_layout(nullptr, n, tb, &total);
  return (int64_t)total;
}

extern "C" int32_t slg_cloud_select(const double* xyz, const uint8_t* bgr, int64_t n, const uint8_t* keep,
                                    const slg_cloud* out, int64_t* index_out, void* ws, void* stream) {
  if (n <= 0 || !xyz || !keep || !out || !out->xyz || !out->count)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_cloud_select: n <= 0 or a NULL buffer");
  Ws w;
  if (int rc = begin_call("slg_cloud_select", n, ws, -1, &w)) return rc;
  hipStream_t st = (hipStream_t)stream;
  size_t tb = w.temp_bytes;
  auto it = rocprim::make_transform_iterator(keep, U8ToU32());
  if (rocprim::exclusive_scan(w.temp, tb, it, w.pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "slg_cloud_select: scan failed");
  select_kernel<<<grid_of(n, 256), 256, 0, st>>>(xyz, bgr, n, keep, w.pos, (double*)out->xyz, out->bgr, out->count,
                                                out->capacity, index_out);
  return check_launch("select_kernel");
}
