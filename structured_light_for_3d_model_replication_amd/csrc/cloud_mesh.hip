// cloud_mesh.hip -- watertight meshing of an oriented device cloud on a dense uniform grid
// (DESIGN.md §16): trilinear splat of the normals (a gather over cells sorted by key), divergence,
// a geometric multigrid solve of the Poisson equation, the iso value, marching tetrahedra over
// Kuhn's six tetrahedra per cell, the density trim, triangle normals and binary STL records.
// Every rule is one __device__ function restated in tests/mesh_ref.py; fp64 under
// -ffp-contract=off, integer atomics only (the status word), so the same input gives the same bits.
// Node arrays are [R+1]^3 with x fastest: node id (z (R+1) + y) (R+1) + x, cell id (z R + y) R + x.
//
// Every call takes a workspace whose first 256 bytes are the header below (the status word at
// byte 0 as for the filters); the rest is that stage's scratch (slg_mesh_ws_bytes).  The sorts and
// scans here are on other types than cloud_grid.hip's (32-bit keys, 64-bit sums, float64 keys), so
// rocPRIM is instantiated in this file as well.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "cloud_grid.h"
#include "mesh_rules.h"

namespace slgmesh {

using slgcloud::block_tree_sum;
using slgcloud::Bump;
using slgcloud::grid_of;
using slgcloud::kChunk;

constexpr int kMaxDepth = 10;

// ---------------------------------------------------------------- workspace
// Every stage's regions come from cloud_grid.h's Bump, started behind the header.

struct U8ToU64 {
  __host__ __device__ uint64_t operator()(uint8_t v) const { return v; }
};
struct PopToU64 {
  __host__ __device__ uint64_t operator()(uint8_t v) const { return (uint64_t)__builtin_popcount((unsigned)v); }
};
struct KeepToU64 {
  __host__ __device__ uint64_t operator()(uint8_t v) const { return v ? 0u : 1u; }
};

// rocPRIM's scratch by closed bounds, so that the sizes are functions of the counts alone (its own
// size query needs a device); every call checks what rocPRIM asks for against them.
static size_t sort_pairs_temp(size_t n) { return 12 * n + (4u << 20); }   // 32-bit keys and values: 8 n + lookback
static size_t sort_keys_temp(size_t n) { return 12 * n + (4u << 20); }    // float64 keys: 8 n + lookback
static size_t scan_temp(size_t n) { return n / 4 + (1u << 20); }          // lookback states only
static int fits(const char* who, hipError_t e, size_t need, size_t bound) {
  if (e != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "%s: rocPRIM size query failed", who);
  if (need > bound)
    return slg_internal_fail(SLG_ERR_HIP, "%s: rocPRIM asks for %lld bytes of scratch, the bound is %lld", who,
                             (long long)need, (long long)bound);
  return SLG_OK;
}
template <class Op>
static int scan_u8(const uint8_t* in, uint64_t* out, size_t n, void* temp, size_t tb, hipStream_t st) {
  auto it = rocprim::make_transform_iterator(in, Op());
  size_t need = 0;
  const hipError_t e = rocprim::exclusive_scan(nullptr, need, it, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), st);
  if (int rc = fits("cloud mesh scan", e, need, tb)) return rc;
  if (rocprim::exclusive_scan(temp, tb, it, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "cloud mesh: scan failed");
  return SLG_OK;
}

static size_t cube(int64_t v) { return (size_t)v * (size_t)v * (size_t)v; }

struct GridWs { slgcloud::Hdr* ghdr; double* part; };
static GridWs grid_ws(Bump& b, int64_t n) {
  GridWs w;
  w.ghdr = b.take<slgcloud::Hdr>(1);
  w.part = b.take<double>((size_t)grid_of(n, kChunk) * 6);
  return w;
}
struct SplatWs { uint32_t *keys, *keys_s, *idx, *idx_s, *cell_lo, *cell_hi; void* temp; size_t tb; };
static SplatWs splat_ws(Bump& b, int R, int64_t n) {
  SplatWs w;
  w.keys = b.take<uint32_t>(n);
  w.keys_s = b.take<uint32_t>(n);
  w.idx = b.take<uint32_t>(n);
  w.idx_s = b.take<uint32_t>(n);
  w.cell_lo = b.take<uint32_t>(cube(R));
  w.cell_hi = b.take<uint32_t>(cube(R));
  w.tb = sort_pairs_temp((size_t)n);
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
struct Level { double *u, *f, *tmp; };
struct SolveWs { Level lv[kMaxDepth]; int levels; };
static SolveWs solve_ws(Bump& b, int R) {      // level l has R >> l cells per axis, down to 2
  SolveWs w{};
  w.lv[0].tmp = b.take<double>(cube(R + 1));
  int l = 1;
  for (int r = R >> 1; r >= 2; r >>= 1, ++l) {
    w.lv[l].u = b.take<double>(cube(r + 1));
    w.lv[l].f = b.take<double>(cube(r + 1));
    w.lv[l].tmp = b.take<double>(cube(r + 1));
  }
  w.levels = l;
  return w;
}
struct IsoWs { double *vals, *part; };
static IsoWs iso_ws(Bump& b, int64_t n) {
  IsoWs w;
  w.vals = b.take<double>(n);
  w.part = b.take<double>(grid_of(n, kChunk));
  return w;
}
struct ExtractWs { uint8_t *mask, *tcount; uint64_t *vbase, *tbase; void* temp; size_t tb; };
static ExtractWs extract_ws(Bump& b, int R) {
  ExtractWs w;
  w.mask = b.take<uint8_t>(cube(R + 1));
  w.tcount = b.take<uint8_t>(cube(R));
  w.vbase = b.take<uint64_t>(cube(R + 1));
  w.tbase = b.take<uint64_t>(cube(R));
  w.tb = scan_temp(cube(R + 1));
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
struct QuantileWs { double* sorted; void* temp; size_t tb; };
static QuantileWs quantile_ws(Bump& b, int64_t n) {
  QuantileWs w;
  w.sorted = b.take<double>(n);
  w.tb = sort_keys_temp((size_t)n);
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
struct RemoveWs { uint64_t *newid, *tpos; uint8_t* tdrop; void* temp; size_t tb; };
static RemoveWs remove_ws(Bump& b, int64_t nv, int64_t nt) {
  RemoveWs w;
  w.newid = b.take<uint64_t>(nv);
  w.tpos = b.take<uint64_t>(nt > 0 ? nt : 1);
  w.tdrop = b.take<uint8_t>(nt > 0 ? nt : 1);
  w.tb = scan_temp((size_t)(nv > nt ? nv : nt));
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}

static bool pow2_in(int R, int lo, int hi) { return R >= lo && R <= hi && (R & (R - 1)) == 0; }

static int bind(const char* who, void* ws, int64_t ws_bytes, size_t need) {
  if (!ws || ((uintptr_t)ws & 255)) return slg_internal_fail(SLG_ERR_INVALID, "%s: workspace NULL or not 256-byte aligned", who);
  if (ws_bytes < 0 || (size_t)ws_bytes < need)
    return slg_internal_fail(SLG_ERR_INVALID, "%s: workspace of %lld bytes, slg_mesh_ws_bytes gives %lld", who,
                             (long long)ws_bytes, (long long)need);
  return SLG_OK;
}

// ---------------------------------------------------------------- the rules (cell_rule, the corner weights, the Jacobi update, the
// tetrahedron cases and the header are mesh_rules.h's, shared with cloud_band.hip)
// Trilinear value of a node field at p: the 8 corners of p's cell, z outermost, x innermost, from 0.
__device__ inline double trilinear_rule(const double* __restrict__ fld, const double* p, const MeshHdr* hdr) {
  const int R = hdr->R;
  const int64_t n1 = R + 1;
  int i[3];
  double t[3];
  for (int a = 0; a < 3; ++a) cell_rule(p[a], hdr->origin[a], hdr->h, R, &i[a], &t[a]);
  double acc = 0.0;
  for (int dz = 0; dz < 2; ++dz)
    for (int dy = 0; dy < 2; ++dy)
      for (int dx = 0; dx < 2; ++dx)
        acc = acc + corner_weight_rule(t, dx, dy, dz) * fld[((i[2] + dz) * n1 + (i[1] + dy)) * n1 + (i[0] + dx)];
  return acc;
}
// The six neighbours of interior node i: x-, x+, y-, y+, z-, z+ left to right.
__device__ inline double nbr_sum_rule(const double* __restrict__ u, int64_t i, int64_t n1, int64_t n2) {
  return ((((u[i - 1] + u[i + 1]) + u[i - n1]) + u[i + n1]) + u[i - n2]) + u[i + n2];
}
__device__ inline double residual_rule(double uc, double S, double f, double h2) { return f - (S - 6.0 * uc) / h2; }
// Node i of an n1^3 level -> (x, y, z) and whether it lies on the boundary.
__device__ inline bool node_xyz(uint32_t i, uint32_t n1, uint32_t* x, uint32_t* y, uint32_t* z) {
  const uint32_t q = i / n1;
  *x = i - q * n1;
  *z = q / n1;
  *y = q - *z * n1;
  return *x == 0 || *y == 0 || *z == 0 || *x == n1 - 1 || *y == n1 - 1 || *z == n1 - 1;
}
// Workgroup b of n -> the 256 nodes it works on.  The workgroups that share an XCD's L2 (b % 8
// labels them) take one contiguous slab of the level each, so that a slab's y and z neighbours are
// found in its own L2; a bijection for every n.  A choice of speed only: every node is a pure
// function of the input arrays.
__device__ inline uint64_t slab_block(uint32_t b, uint32_t n) {
  const uint32_t q = n / 8, r = n % 8, x = b % 8;
  return (uint64_t)((x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8);
}
__device__ inline int64_t code_offset(int code, int64_t n1) {
  return (code & 1) + ((code >> 1) & 1) * n1 + ((code >> 2) & 1) * n1 * n1;
}

namespace {

// ---------------------------------------------------------------- grid
__global__ void set_header_kernel(MeshHdr* hdr, int R, double ox, double oy, double oz, double h, double iso) {
  hdr->status = 0;
  hdr->R = R;
  hdr->nV = hdr->nT = 0;
  hdr->origin[0] = ox;
  hdr->origin[1] = oy;
  hdr->origin[2] = oz;
  hdr->h = h;
  hdr->iso = iso;
  hdr->thr = 0.0;
}

// side = scale * largest extent, origin = (min + max) / 2 - side / 2, h = side / R.
__global__ void grid_final_kernel(const slgcloud::Hdr* g, MeshHdr* hdr, int R, double scale) {
  hdr->status = g->status;
  hdr->R = R;
  hdr->nV = hdr->nT = 0;
  hdr->iso = hdr->thr = 0.0;
  if (g->status) return;
  double ext = 0.0;
  for (int a = 0; a < 3; ++a) ext = fmax(ext, g->mx[a] - g->mn[a]);
  if (!(ext > 0.0) || !isfinite(ext) || !isfinite(scale * ext)) { hdr->status = SLG_FILTER_BAD_EXTENT; return; }
  const double side = scale * ext;
  for (int a = 0; a < 3; ++a) hdr->origin[a] = (g->mn[a] + g->mx[a]) / 2.0 - side / 2.0;
  hdr->h = side / (double)R;
}

// ---------------------------------------------------------------- splat
__global__ __launch_bounds__(256)
void cell_keys_kernel(MeshHdr* hdr, const double* __restrict__ xyz, const double* __restrict__ nrm, int64_t n,
                      uint32_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  if (hdr->status) return;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int R = hdr->R;
  int i[3];
  double t;
  bool bad = false;
  for (int a = 0; a < 3; ++a) {
    cell_rule(xyz[3 * j + a], hdr->origin[a], hdr->h, R, &i[a], &t);
    if (!isfinite(nrm[3 * j + a])) bad = true;
  }
  if (bad) atomicOr(&hdr->status, SLG_FILTER_BAD_NONFINITE);
  keys[j] = ((uint32_t)i[2] * (uint32_t)R + (uint32_t)i[1]) * (uint32_t)R + (uint32_t)i[0];
  idx[j] = (uint32_t)j;
}

// cell_lo / cell_hi (cleared before): the sorted range of every occupied cell.
__global__ __launch_bounds__(256)
void cell_ranges_kernel(const MeshHdr* hdr, const uint32_t* __restrict__ keys_s, int64_t n, uint32_t* __restrict__ lo,
                        uint32_t* __restrict__ hi) {
  if (hdr->status) return;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint32_t k = keys_s[j];
  if (j == 0 || keys_s[j - 1] != k) lo[k] = (uint32_t)j;
  if (j == n - 1 || keys_s[j + 1] != k) hi[k] = (uint32_t)(j + 1);
}

// One thread per node: its 8 incident cells in ascending cell id, each cell's points in ascending
// input index (the stable sort's order), W += w and V += w * normal from 0.
__global__ __launch_bounds__(256)
void splat_kernel(const MeshHdr* hdr, const double* __restrict__ xyz, const double* __restrict__ nrm,
                  const uint32_t* __restrict__ idx_s, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                  double* __restrict__ W, double* __restrict__ V) {
  if (hdr->status) return;
  const int R = hdr->R;
  const uint32_t n1 = R + 1;
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (uint64_t)n1 * n1 * n1) return;
  uint32_t X, Y, Z;
  node_xyz((uint32_t)g, n1, &X, &Y, &Z);
  const double h = hdr->h, o[3] = {hdr->origin[0], hdr->origin[1], hdr->origin[2]};
  double w = 0.0, v[3] = {0.0, 0.0, 0.0};
  for (int ez = 0; ez < 2; ++ez)
    for (int ey = 0; ey < 2; ++ey)
      for (int ex = 0; ex < 2; ++ex) {
        const int cx = (int)X - 1 + ex, cy = (int)Y - 1 + ey, cz = (int)Z - 1 + ez;
        if (cx < 0 || cy < 0 || cz < 0 || cx >= R || cy >= R || cz >= R) continue;
        const size_t cell = ((size_t)cz * R + cy) * R + cx;
        const uint32_t e = hi[cell];
        for (uint32_t j = lo[cell]; j < e; ++j) {
          const size_t p = idx_s[j];
          int i;
          double t[3];
          for (int a = 0; a < 3; ++a) cell_rule(xyz[3 * p + a], o[a], h, R, &i, &t[a]);
          const double wt = corner_weight_rule(t, 1 - ex, 1 - ey, 1 - ez);
          w = w + wt;
          for (int a = 0; a < 3; ++a) v[a] = v[a] + wt * nrm[3 * p + a];
        }
      }
  W[g] = w;
  for (int a = 0; a < 3; ++a) V[3 * g + a] = v[a];
}

// f = div V by central differences: (dVx / 2h + dVy / 2h) + dVz / 2h at interior nodes, else 0.
__global__ __launch_bounds__(256)
void divergence_kernel(const MeshHdr* hdr, const double* __restrict__ V, double* __restrict__ f) {
  if (hdr->status) return;
  const uint32_t n1 = hdr->R + 1;
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (uint64_t)n1 * n1 * n1) return;
  uint32_t x, y, z;
  if (node_xyz((uint32_t)g, n1, &x, &y, &z)) { f[g] = 0.0; return; }
  const int64_t i = (int64_t)g, s1 = n1, s2 = (int64_t)n1 * n1;
  const double th = 2.0 * hdr->h;
  f[g] = ((V[3 * (i + 1)] - V[3 * (i - 1)]) / th + (V[3 * (i + s1) + 1] - V[3 * (i - s1) + 1]) / th) +
         (V[3 * (i + s2) + 2] - V[3 * (i - s2) + 2]) / th;
}

// ---------------------------------------------------------------- multigrid
// One damped Jacobi sweep (omega = 6/7) of an n1^3 level: one thread per node along x, so a wave
// reads and writes whole 512-byte runs of a row; the y and z neighbours come out of L2.
__global__ __launch_bounds__(256)
void smooth_kernel(const MeshHdr* hdr, const double* __restrict__ u, const double* __restrict__ f,
                   double* __restrict__ out, uint32_t n1, double mul) {
  if (hdr->status) return;
  const uint64_t g = slab_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  if (g >= (uint64_t)n1 * n1 * n1) return;
  uint32_t x, y, z;
  if (node_xyz((uint32_t)g, n1, &x, &y, &z)) { out[g] = 0.0; return; }
  const double hl = hdr->h * mul;
  out[g] = jacobi_rule(u[g], nbr_sum_rule(u, (int64_t)g, n1, (int64_t)n1 * n1), f[g], hl * hl);
}

__global__ __launch_bounds__(256)
void residual_kernel(const MeshHdr* hdr, const double* __restrict__ u, const double* __restrict__ f,
                     double* __restrict__ out, uint32_t n1, double mul) {
  if (hdr->status) return;
  const uint64_t g = slab_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  if (g >= (uint64_t)n1 * n1 * n1) return;
  uint32_t x, y, z;
  if (node_xyz((uint32_t)g, n1, &x, &y, &z)) { out[g] = 0.0; return; }
  const double hl = hdr->h * mul;
  out[g] = residual_rule(u[g], nbr_sum_rule(u, (int64_t)g, n1, (int64_t)n1 * n1), f[g], hl * hl);
}

// Full weighting: the 27 fine nodes around 2X, z outermost, weights (1/4, 1/2, 1/4) per axis.
__global__ __launch_bounds__(256)
void restrict_kernel(const MeshHdr* hdr, const double* __restrict__ r, double* __restrict__ fc, uint32_t n1c) {
  if (hdr->status) return;
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (uint64_t)n1c * n1c * n1c) return;
  uint32_t x, y, z;
  if (node_xyz((uint32_t)g, n1c, &x, &y, &z)) { fc[g] = 0.0; return; }
  const int64_t n1 = 2 * (int64_t)(n1c - 1) + 1, n2 = n1 * n1;
  const int64_t c = (2 * (int64_t)z * n1 + 2 * (int64_t)y) * n1 + 2 * (int64_t)x;
  const double w[3] = {0.25, 0.5, 0.25};
  double acc = 0.0;
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) acc = acc + ((w[dz + 1] * w[dy + 1]) * w[dx + 1]) * r[c + dz * n2 + dy * n1 + dx];
  fc[g] = acc;
}

// Trilinear prolongation added to the interior fine nodes: per axis the coarse node x / 2 (even x)
// or the two around it with weight 1/2 each (odd x), z outermost, lower node first, from 0.
__global__ __launch_bounds__(256)
void prolong_kernel(const MeshHdr* hdr, double* __restrict__ u, const double* __restrict__ e, uint32_t n1) {
  if (hdr->status) return;
  const uint64_t g = slab_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  if (g >= (uint64_t)n1 * n1 * n1) return;
  uint32_t c[3];
  if (node_xyz((uint32_t)g, n1, &c[0], &c[1], &c[2])) return;
  const int64_t m1 = (n1 - 1) / 2 + 1;
  int64_t lo[3];
  int cnt[3];
  double w[3];
  for (int a = 0; a < 3; ++a) {
    const bool odd = c[a] & 1;
    lo[a] = odd ? (c[a] - 1) / 2 : c[a] / 2;
    cnt[a] = odd ? 2 : 1;
    w[a] = odd ? 0.5 : 1.0;
  }
  double acc = 0.0;
  for (int dz = 0; dz < cnt[2]; ++dz)
    for (int dy = 0; dy < cnt[1]; ++dy)
      for (int dx = 0; dx < cnt[0]; ++dx)
        acc = acc + ((w[2] * w[1]) * w[0]) * e[((lo[2] + dz) * m1 + (lo[1] + dy)) * m1 + (lo[0] + dx)];
  u[g] = u[g] + acc;
}

// The R = 2 level: 27 nodes, the one interior node solved directly (its neighbours are 0).
__global__ void coarsest_kernel(const MeshHdr* hdr, double* __restrict__ u, const double* __restrict__ f, double mul) {
  if (hdr->status) return;
  const int t = threadIdx.x;
  const double hl = hdr->h * mul;
  if (t < 27) u[t] = t == 13 ? -((hl * hl) * f[13]) / 6.0 : 0.0;
}

// ---------------------------------------------------------------- iso value
__global__ __launch_bounds__(256)
void sample_kernel(const MeshHdr* hdr, const double* __restrict__ fld, const double* __restrict__ xyz, int64_t n,
                   double* __restrict__ out) {
  if (hdr->status) return;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double p[3] = {xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]};
  out[j] = trilinear_rule(fld, p, hdr);
}
// The fixed tree of slg_cloud_centroid on one array: 8 consecutive values per thread, the
// workgroup's tree, then the partials.
__global__ __launch_bounds__(256)
void sum_partial_kernel(const MeshHdr* hdr, const double* __restrict__ v, int64_t n, double* __restrict__ part) {
  __shared__ double sm[256];
  if (hdr->status) return;
  const int64_t base = (int64_t)blockIdx.x * kChunk + threadIdx.x * (kChunk / 256);
  double s = 0.0;
  for (int j = 0; j < kChunk / 256; ++j)
    if (base + j < n) s += v[base + j];
  s = block_tree_sum(s, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256)
void iso_final_kernel(MeshHdr* hdr, const double* __restrict__ part, int nb, int64_t n) {
  __shared__ double sm[256];
  if (hdr->status) return;
  double s = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) s += part[b];
  s = block_tree_sum(s, sm);
  if (threadIdx.x == 0) hdr->iso = s / (double)n;
}

// ---------------------------------------------------------------- marching tetrahedra
// Per node: the 7-bit mask of its crossing owned edges; per cell (the node at its 000 corner): the
// number of triangles of its six tetrahedra.
__global__ __launch_bounds__(256)
void count_kernel(const MeshHdr* hdr, const double* __restrict__ chi, uint8_t* __restrict__ mask,
                  uint8_t* __restrict__ tcount) {
  if (hdr->status) return;
  const int R = hdr->R;
  const uint32_t n1 = R + 1;
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (uint64_t)n1 * n1 * n1) return;
  uint32_t x, y, z;
  node_xyz((uint32_t)g, n1, &x, &y, &z);
  const double iso = hdr->iso;
  int in = inside_rule(chi[g], iso) ? 1 : 0;      // bit c: corner code c of the cell at this node
  for (int c = 1; c < 8; ++c) {
    if (x + (c & 1) > (uint32_t)R || y + ((c >> 1) & 1) > (uint32_t)R || z + ((c >> 2) & 1) > (uint32_t)R) continue;
    if (inside_rule(chi[(int64_t)g + code_offset(c, n1)], iso)) in |= 1 << c;
  }
  int m = 0;
  for (int e = 0; e < 7; ++e) {
    const int c = kEdgeCode[e];
    if (x + (c & 1) > (uint32_t)R || y + ((c >> 1) & 1) > (uint32_t)R || z + ((c >> 2) & 1) > (uint32_t)R) continue;
    if (((in >> c) & 1) != (in & 1)) m |= 1 << e;
  }
  mask[g] = (uint8_t)m;
  if (x < (uint32_t)R && y < (uint32_t)R && z < (uint32_t)R) {
    int nt = 0;
    for (int k = 0; k < 6; ++k) {
      int pc = 0;
      for (int v = 0; v < 4; ++v) pc += (in >> kTetCode[k][v]) & 1;
      nt += pc == 2 ? 2 : (pc == 1 || pc == 3) ? 1 : 0;
    }
    tcount[((size_t)z * R + y) * R + x] = (uint8_t)nt;
  }
}

__global__ void totals_kernel(MeshHdr* hdr, const uint8_t* mask, const uint64_t* vbase, const uint8_t* tcount,
                              const uint64_t* tbase, size_t M, size_t C) {
  if (hdr->status) return;
  hdr->nV = (int64_t)(vbase[M - 1] + (uint64_t)__popc((unsigned)mask[M - 1]));
  hdr->nT = (int64_t)(tbase[C - 1] + tcount[C - 1]);
}

// Vertices in ascending (owner node, edge type): p_a + t (p_b - p_a), t = (iso - chi_a) / (chi_b - chi_a),
// node positions origin + h * i; the density is the trilinear W at the vertex.
__global__ __launch_bounds__(256)
void vertices_kernel(const MeshHdr* hdr, const double* __restrict__ chi, const double* __restrict__ W,
                     const uint8_t* __restrict__ mask, const uint64_t* __restrict__ vbase, double* __restrict__ vert,
                     double* __restrict__ dens) {
  if (hdr->status) return;
  const uint32_t n1 = hdr->R + 1;
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (uint64_t)n1 * n1 * n1) return;
  const int m = mask[g];
  if (!m) return;
  uint32_t c[3];
  node_xyz((uint32_t)g, n1, &c[0], &c[1], &c[2]);
  const double iso = hdr->iso, h = hdr->h, ca = chi[g];
  uint64_t o = vbase[g];
  for (int e = 0; e < 7; ++e) {
    if (!((m >> e) & 1)) continue;
    const int code = kEdgeCode[e];
    const double cb = chi[(int64_t)g + code_offset(code, n1)];
    const double t = (iso - ca) / (cb - ca);
    double p[3];
    for (int a = 0; a < 3; ++a) {
      const double pa = hdr->origin[a] + h * (double)c[a];
      const double pb = hdr->origin[a] + h * (double)(c[a] + ((code >> a) & 1));
      p[a] = pa + t * (pb - pa);
      vert[3 * o + a] = p[a];
    }
    if (dens) dens[o] = trilinear_rule(W, p, hdr);
    ++o;
  }
}

// Triangles in ascending (cell, tetrahedron, triangle); a vertex id is its owner's base plus the
// number of crossing edges of lower type.
__global__ __launch_bounds__(256)
void triangles_kernel(const MeshHdr* hdr, const double* __restrict__ chi, const uint8_t* __restrict__ mask,
                      const uint64_t* __restrict__ vbase, const uint8_t* __restrict__ tcount,
                      const uint64_t* __restrict__ tbase, int32_t* __restrict__ tris) {
  if (hdr->status) return;
  const int R = hdr->R;
  const int64_t n1 = R + 1;
  const uint64_t cell = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= (uint64_t)R * R * R) return;
  if (!tcount[cell]) return;
  const uint32_t q = (uint32_t)cell / (uint32_t)R;
  const uint32_t x = (uint32_t)cell - q * R, z = q / (uint32_t)R, y = q - z * R;
  const int64_t node = ((int64_t)z * n1 + y) * n1 + x;
  const double iso = hdr->iso;
  int in = 0;
  for (int c = 0; c < 8; ++c)
    if (inside_rule(chi[node + code_offset(c, n1)], iso)) in |= 1 << c;
  uint64_t o = tbase[cell];
  for (int k = 0; k < 6; ++k) {
    int m = 0;
    for (int v = 0; v < 4; ++v) m |= ((in >> kTetCode[k][v]) & 1) << v;
    int tri[2][3][2];
    const int nt = tet_case_rule(m, kTetOdd[k], tri);
    for (int j = 0; j < nt; ++j, ++o)
      for (int e = 0; e < 3; ++e) {
        const int cp = kTetCode[k][tri[j][e][0]], cq = kTetCode[k][tri[j][e][1]];
        const int type = kTypeOfCode[cq ^ cp];
        const int64_t owner = node + code_offset(cp, n1);
        tris[3 * o + e] = (int32_t)(vbase[owner] + (uint64_t)__popc((unsigned)mask[owner] & ((1u << type) - 1u)));
      }
  }
}

// ---------------------------------------------------------------- trim
// numpy's linear quantile on the sorted values: lo, hi and g = q (n - 1) - lo are the host's.
__global__ void quantile_kernel(MeshHdr* hdr, const double* __restrict__ s, int64_t lo, int64_t hi, double g) {
  const double A = s[lo], B = s[hi], diff = B - A;
  hdr->thr = g >= 0.5 ? B - diff * (1.0 - g) : A + diff * g;
}

__global__ __launch_bounds__(256)
void tri_drop_kernel(const int32_t* __restrict__ tris, int64_t nt, const uint8_t* __restrict__ vmask,
                     uint8_t* __restrict__ tdrop) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  tdrop[t] = (vmask[tris[3 * t]] | vmask[tris[3 * t + 1]] | vmask[tris[3 * t + 2]]) ? 1 : 0;
}
__global__ __launch_bounds__(256)
void vert_select_kernel(const double* __restrict__ vert, const double* __restrict__ dens, int64_t nv,
                        const uint8_t* __restrict__ vmask, const uint64_t* __restrict__ newid,
                        double* __restrict__ overt, double* __restrict__ odens, MeshHdr* hdr) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv) return;
  const uint64_t j = newid[i];
  if (!vmask[i]) {
    for (int a = 0; a < 3; ++a) overt[3 * j + a] = vert[3 * i + a];
    if (dens && odens) odens[j] = dens[i];
  }
  if (i == nv - 1) hdr->nV = (int64_t)(j + (vmask[i] ? 0 : 1));
}
__global__ __launch_bounds__(256)
void tri_select_kernel(const int32_t* __restrict__ tris, int64_t nt, const uint8_t* __restrict__ tdrop,
                       const uint64_t* __restrict__ tpos, const uint64_t* __restrict__ newid,
                       int32_t* __restrict__ otris, MeshHdr* hdr) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  const uint64_t j = tpos[t];
  if (!tdrop[t])
    for (int a = 0; a < 3; ++a) otris[3 * j + a] = (int32_t)newid[tris[3 * t + a]];
  if (t == nt - 1) hdr->nT = (int64_t)(j + (tdrop[t] ? 0 : 1));
}

// ---------------------------------------------------------------- normals and STL
// Unit (b - a) x (c - a); (0, 0, 0) when its length is 0.
__device__ inline void triangle_normal_rule(const double* a, const double* b, const double* c, double* n) {
  const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const double x = u[1] * v[2] - u[2] * v[1], y = u[2] * v[0] - u[0] * v[2], z = u[0] * v[1] - u[1] * v[0];
  const double len = sqrt((x * x + y * y) + z * z);
  const bool ok = len > 0.0;
  n[0] = ok ? x / len : 0.0;
  n[1] = ok ? y / len : 0.0;
  n[2] = ok ? z / len : 0.0;
}
__global__ __launch_bounds__(256)
void normals_kernel(const double* __restrict__ vert, const int32_t* __restrict__ tris, int64_t nt,
                    double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  double n[3];
  triangle_normal_rule(vert + 3 * (int64_t)tris[3 * t], vert + 3 * (int64_t)tris[3 * t + 1],
                       vert + 3 * (int64_t)tris[3 * t + 2], n);
  for (int a = 0; a < 3; ++a) out[3 * t + a] = n[a];
}
// One 50-byte record per triangle: float32 normal, three float32 vertices, a zero attribute word.
__global__ __launch_bounds__(256)
void stl_pack_kernel(const double* __restrict__ vert, const int32_t* __restrict__ tris,
                     const double* __restrict__ nrm, int64_t nt, uint16_t* __restrict__ rec) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  uint16_t* o = rec + 25 * t;
  for (int k = 0; k < 12; ++k) {
    const double d = k < 3 ? nrm[3 * t + k] : vert[3 * (int64_t)tris[3 * t + (k - 3) / 3] + (k - 3) % 3];
    const uint32_t b = __float_as_uint((float)d);
    o[2 * k] = (uint16_t)(b & 0xFFFFu);
    o[2 * k + 1] = (uint16_t)(b >> 16);
  }
  o[24] = 0;
}

}  // namespace

// ---------------------------------------------------------------- host side
static int nodes_grid(int64_t n1) { return (int)((cube(n1) + 255) / 256); }

// One V(2,2) cycle from level l down and back.
static int vcycle(const MeshHdr* hdr, const SolveWs& w, int l, int R, hipStream_t st) {
  const int r = R >> l;
  const uint32_t n1 = r + 1;
  const double mul = (double)(1 << l);
  const Level& L = w.lv[l];
  if (r == 2) { coarsest_kernel<<<1, 64, 0, st>>>(hdr, L.u, L.f, mul); return SLG_OK; }
  const int g = nodes_grid(n1);
  smooth_kernel<<<g, 256, 0, st>>>(hdr, L.u, L.f, L.tmp, n1, mul);
  smooth_kernel<<<g, 256, 0, st>>>(hdr, L.tmp, L.f, L.u, n1, mul);
  residual_kernel<<<g, 256, 0, st>>>(hdr, L.u, L.f, L.tmp, n1, mul);
  const Level& C = w.lv[l + 1];
  const uint32_t n1c = r / 2 + 1;
  restrict_kernel<<<nodes_grid(n1c), 256, 0, st>>>(hdr, L.tmp, C.f, n1c);
  if (hipMemsetAsync(C.u, 0, cube(n1c) * sizeof(double), st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "slg_mesh_solve: memset failed");
  if (int rc = vcycle(hdr, w, l + 1, R, st)) return rc;
  prolong_kernel<<<g, 256, 0, st>>>(hdr, L.u, C.u, n1);
  smooth_kernel<<<g, 256, 0, st>>>(hdr, L.u, L.f, L.tmp, n1, mul);
  smooth_kernel<<<g, 256, 0, st>>>(hdr, L.tmp, L.f, L.u, n1, mul);
  return SLG_OK;
}

static size_t stage_bytes(int stage, int R, int64_t n, int64_t m) {
  Bump b(nullptr, SLG_MESH_HDR_BYTES);
  switch (stage) {
    case SLG_MESH_WS_GRID: grid_ws(b, n); break;
    case SLG_MESH_WS_SPLAT: splat_ws(b, R, n); break;
    case SLG_MESH_WS_SOLVE: solve_ws(b, R); break;
    case SLG_MESH_WS_ISO: iso_ws(b, n); break;
    case SLG_MESH_WS_EXTRACT: extract_ws(b, R); break;
    case SLG_MESH_WS_QUANTILE: quantile_ws(b, n); break;
    case SLG_MESH_WS_REMOVE: remove_ws(b, n, m); break;
    default: break;
  }
  return b.off;
}

}  // namespace slgmesh

using namespace slgmesh;

extern "C" int64_t slg_mesh_ws_bytes(int32_t stage, int32_t R, int64_t n, int64_t m) {
  const bool grid_stage = stage == SLG_MESH_WS_SPLAT || stage == SLG_MESH_WS_SOLVE || stage == SLG_MESH_WS_EXTRACT ||
                          stage == SLG_MESH_WS_ALL;
  if (stage < 0 || stage > SLG_MESH_WS_ALL || n < 0 || m < 0 || (grid_stage && (R < 1 || R > (1 << kMaxDepth))))
    return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_ws_bytes: unknown stage, R outside 1..1024 or a negative count");
  if (n > slgcloud::kMaxPoints && stage != SLG_MESH_WS_QUANTILE && stage != SLG_MESH_WS_REMOVE)
    return -(int64_t)slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_mesh_ws_bytes: more than 2^30 points");
  if (stage != SLG_MESH_WS_ALL) return (int64_t)stage_bytes(stage, R, n > 0 ? n : 1, m);
  size_t most = 0;
  for (int s = SLG_MESH_WS_GRID; s <= SLG_MESH_WS_EXTRACT; ++s) {
    const size_t b = stage_bytes(s, R, n > 0 ? n : 1, 0);
    most = b > most ? b : most;
  }
  return (int64_t)(most + 6 * cube(R + 1) * sizeof(double));        // + W, V (3), f and chi
}

extern "C" int32_t slg_mesh_set_header(void* ws, int32_t R, const double* origin, double h, double iso, void* stream) {
  if (!ws || !origin || R < 1 || R > (1 << kMaxDepth) || !(h > 0.0) || !isfinite(h))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_set_header: a NULL buffer, R outside 1..1024 or h not finite and > 0");
  set_header_kernel<<<1, 1, 0, (hipStream_t)stream>>>((MeshHdr*)ws, R, origin[0], origin[1], origin[2], h, iso);
  return check_launch("slg_mesh_set_header");
}

extern "C" int32_t slg_mesh_grid(const double* xyz, int64_t n, int32_t depth, double scale, void* ws, int64_t ws_bytes,
                                 void* stream) {
  if (n <= 0 || !xyz || depth < 2 || depth > kMaxDepth || !(scale >= 1.0) || !isfinite(scale))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_grid: n <= 0, a NULL buffer, depth outside 2..10 or scale not finite and >= 1");
  if (n > slgcloud::kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_mesh_grid: more than 2^30 points");
  if (int rc = bind("slg_mesh_grid", ws, ws_bytes, stage_bytes(SLG_MESH_WS_GRID, 0, n, 0))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const GridWs g = grid_ws(b, n);
  hipStream_t st = (hipStream_t)stream;
  slgcloud::Ws w{};
  w.hdr = g.ghdr;
  w.part = g.part;
  if (int rc = slgcloud::bbox(xyz, n, w, 0.0, 1, st)) return rc;
  grid_final_kernel<<<1, 1, 0, st>>>(g.ghdr, (MeshHdr*)ws, 1 << depth, scale);
  return check_launch("slg_mesh_grid");
}

extern "C" int32_t slg_mesh_splat(const double* xyz, const double* normals, int64_t n, int32_t R, void* ws,
                                  int64_t ws_bytes, double* W_out, double* V_out, void* stream) {
  if (n <= 0 || !xyz || !normals || !W_out || !V_out || !pow2_in(R, 1, 1 << kMaxDepth))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_splat: n <= 0, a NULL buffer (the splat needs normals) or R no power of two in 1..1024");
  if (n > slgcloud::kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_mesh_splat: more than 2^30 points");
  if (int rc = bind("slg_mesh_splat", ws, ws_bytes, stage_bytes(SLG_MESH_WS_SPLAT, R, n, 0))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const SplatWs w = splat_ws(b, R, n);
  MeshHdr* hdr = (MeshHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const int g = grid_of(n, 256);
  cell_keys_kernel<<<g, 256, 0, st>>>(hdr, xyz, normals, n, w.keys, w.idx);
  size_t tb = w.tb, need = 0;
  int bits = 0;
  while ((1 << bits) < R) ++bits;
  const hipError_t e = rocprim::radix_sort_pairs(nullptr, need, (const uint32_t*)w.keys, w.keys_s, (const uint32_t*)w.idx,
                                                 w.idx_s, (size_t)n, 0u, (unsigned)(3 * bits > 0 ? 3 * bits : 1), st);
  if (int rc = fits("slg_mesh_splat", e, need, tb)) return rc;
  if (rocprim::radix_sort_pairs(w.temp, tb, (const uint32_t*)w.keys, w.keys_s, (const uint32_t*)w.idx, w.idx_s, (size_t)n, 0u,
                                (unsigned)(3 * bits > 0 ? 3 * bits : 1), st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "slg_mesh_splat: radix sort failed");
  if (hipMemsetAsync(w.cell_lo, 0, cube(R) * 4, st) != hipSuccess || hipMemsetAsync(w.cell_hi, 0, cube(R) * 4, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "slg_mesh_splat: memset failed");
  cell_ranges_kernel<<<g, 256, 0, st>>>(hdr, w.keys_s, n, w.cell_lo, w.cell_hi);
  splat_kernel<<<nodes_grid(R + 1), 256, 0, st>>>(hdr, xyz, normals, w.idx_s, w.cell_lo, w.cell_hi, W_out, V_out);
  return check_launch("slg_mesh_splat");
}

extern "C" int32_t slg_mesh_divergence(const double* V, int32_t R, void* ws, double* f_out, void* stream) {
  if (!V || !ws || !f_out || !pow2_in(R, 1, 1 << kMaxDepth))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_divergence: a NULL buffer or R no power of two in 1..1024");
  divergence_kernel<<<nodes_grid(R + 1), 256, 0, (hipStream_t)stream>>>((const MeshHdr*)ws, V, f_out);
  return check_launch("slg_mesh_divergence");
}

extern "C" int32_t slg_mesh_solve(const double* f, int32_t R, int32_t cycles, void* ws, int64_t ws_bytes,
                                  double* chi_out, void* stream) {
  if (!f || !chi_out || f == chi_out || cycles < 0 || !pow2_in(R, 4, 1 << kMaxDepth))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_solve: a NULL buffer, chi == f, cycles < 0 or R no power of two in 4..1024");
  if (int rc = bind("slg_mesh_solve", ws, ws_bytes, stage_bytes(SLG_MESH_WS_SOLVE, R, 0, 0))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  SolveWs w = solve_ws(b, R);
  w.lv[0].u = chi_out;
  w.lv[0].f = (double*)f;                   // read only
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(chi_out, 0, cube(R + 1) * sizeof(double), st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "slg_mesh_solve: memset failed");
  for (int c = 0; c < cycles; ++c)
    if (int rc = vcycle((const MeshHdr*)ws, w, 0, R, st)) return rc;
  return check_launch("slg_mesh_solve");
}

extern "C" int32_t slg_mesh_sample(const double* field, const double* xyz, int64_t n, void* ws, double* out, void* stream) {
  if (!field || !xyz || !ws || !out || n <= 0)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_sample: n <= 0 or a NULL buffer");
  sample_kernel<<<grid_of(n, 256), 256, 0, (hipStream_t)stream>>>((const MeshHdr*)ws, field, xyz, n, out);
  return check_launch("slg_mesh_sample");
}

extern "C" int32_t slg_mesh_iso(const double* chi, const double* xyz, int64_t n, void* ws, int64_t ws_bytes, void* stream) {
  if (!chi || !xyz || n <= 0) return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_iso: n <= 0 or a NULL buffer");
  if (n > slgcloud::kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_mesh_iso: more than 2^30 points");
  if (int rc = bind("slg_mesh_iso", ws, ws_bytes, stage_bytes(SLG_MESH_WS_ISO, 0, n, 0))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const IsoWs w = iso_ws(b, n);
  MeshHdr* hdr = (MeshHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(n, kChunk);
  sample_kernel<<<grid_of(n, 256), 256, 0, st>>>(hdr, chi, xyz, n, w.vals);
  sum_partial_kernel<<<nb, 256, 0, st>>>(hdr, w.vals, n, w.part);
  iso_final_kernel<<<1, 256, 0, st>>>(hdr, w.part, nb, n);
  return check_launch("slg_mesh_iso");
}

extern "C" int32_t slg_mesh_count(const double* chi, int32_t R, void* ws, int64_t ws_bytes, void* stream) {
  if (!chi || R < 1 || R > (1 << kMaxDepth))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_count: a NULL buffer or R outside 1..1024");
  if (int rc = bind("slg_mesh_count", ws, ws_bytes, stage_bytes(SLG_MESH_WS_EXTRACT, R, 0, 0))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const ExtractWs w = extract_ws(b, R);
  MeshHdr* hdr = (MeshHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const size_t M = cube(R + 1), C = cube(R);
  count_kernel<<<nodes_grid(R + 1), 256, 0, st>>>(hdr, chi, w.mask, w.tcount);
  if (int rc = scan_u8<PopToU64>(w.mask, w.vbase, M, w.temp, w.tb, st)) return rc;
  if (int rc = scan_u8<U8ToU64>(w.tcount, w.tbase, C, w.temp, w.tb, st)) return rc;
  totals_kernel<<<1, 1, 0, st>>>(hdr, w.mask, w.vbase, w.tcount, w.tbase, M, C);
  return check_launch("slg_mesh_count");
}

extern "C" int32_t slg_mesh_emit(const double* chi, const double* W, int32_t R, void* ws, int64_t ws_bytes,
                                 double* vertices_out, int64_t n_vertices, double* densities_out, int32_t* triangles_out,
                                 int64_t n_triangles, void* stream) {
  if (!chi || R < 1 || R > (1 << kMaxDepth) || n_vertices < 0 || n_triangles < 0 || (n_vertices && !vertices_out) ||
      (n_triangles && !triangles_out) || (W && n_vertices && !densities_out))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_emit: a NULL buffer, R outside 1..1024 or a negative count");
  if (n_vertices >= (1ll << 31)) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_mesh_emit: 2^31 vertices or more");
  if (int rc = bind("slg_mesh_emit", ws, ws_bytes, stage_bytes(SLG_MESH_WS_EXTRACT, R, 0, 0))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const ExtractWs w = extract_ws(b, R);
  const MeshHdr* hdr = (const MeshHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  if (n_vertices)
    vertices_kernel<<<nodes_grid(R + 1), 256, 0, st>>>(hdr, chi, W, w.mask, w.vbase, vertices_out, W ? densities_out : nullptr);
  if (n_triangles)
    triangles_kernel<<<nodes_grid(R), 256, 0, st>>>(hdr, chi, w.mask, w.vbase, w.tcount, w.tbase, triangles_out);
  return check_launch("slg_mesh_emit");
}

extern "C" int32_t slg_mesh_quantile(const double* values, int64_t n, double q, void* ws, int64_t ws_bytes, void* stream) {
  if (!values || n <= 0 || !(q >= 0.0 && q <= 1.0))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_quantile: n <= 0, a NULL buffer or q outside [0, 1]");
  if (int rc = bind("slg_mesh_quantile", ws, ws_bytes, stage_bytes(SLG_MESH_WS_QUANTILE, 0, n, 0))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const QuantileWs w = quantile_ws(b, n);
  hipStream_t st = (hipStream_t)stream;
  size_t tb = w.tb, need = 0;
  const hipError_t e = rocprim::radix_sort_keys(nullptr, need, values, w.sorted, (size_t)n, 0u, 64u, st);
  if (int rc = fits("slg_mesh_quantile", e, need, tb)) return rc;
  if (rocprim::radix_sort_keys(w.temp, tb, values, w.sorted, (size_t)n, 0u, 64u, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "slg_mesh_quantile: radix sort failed");
  const double vi = q * (double)(n - 1);
  const double fl = floor(vi);
  const int64_t lo = (int64_t)fl, hi = lo + 1 < n ? lo + 1 : n - 1;
  quantile_kernel<<<1, 1, 0, st>>>((MeshHdr*)ws, w.sorted, lo, hi, vi - fl);
  return check_launch("slg_mesh_quantile");
}

extern "C" int32_t slg_mesh_remove(const double* vertices, const double* densities, int64_t n_vertices,
                                   const int32_t* triangles, int64_t n_triangles, const uint8_t* mask, void* ws,
                                   int64_t ws_bytes, double* vertices_out, double* densities_out, int32_t* triangles_out,
                                   void* stream) {
  if (n_vertices <= 0 || n_triangles < 0 || !vertices || !mask || !vertices_out || (n_triangles && (!triangles || !triangles_out)))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_remove: no vertices, a negative count or a NULL buffer");
  if (n_vertices >= (1ll << 31)) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_mesh_remove: 2^31 vertices or more");
  if (int rc = bind("slg_mesh_remove", ws, ws_bytes, stage_bytes(SLG_MESH_WS_REMOVE, 0, n_vertices, n_triangles))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const RemoveWs w = remove_ws(b, n_vertices, n_triangles);
  MeshHdr* hdr = (MeshHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(hdr, 0, SLG_MESH_HDR_BYTES, st) != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "slg_mesh_remove: memset failed");
  if (int rc = scan_u8<KeepToU64>(mask, w.newid, (size_t)n_vertices, w.temp, w.tb, st)) return rc;
  vert_select_kernel<<<grid_of(n_vertices, 256), 256, 0, st>>>(vertices, densities, n_vertices, mask, w.newid, vertices_out,
                                                              densities_out, hdr);
  if (n_triangles) {
    tri_drop_kernel<<<grid_of(n_triangles, 256), 256, 0, st>>>(triangles, n_triangles, mask, w.tdrop);
    if (int rc = scan_u8<KeepToU64>(w.tdrop, w.tpos, (size_t)n_triangles, w.temp, w.tb, st)) return rc;
    tri_select_kernel<<<grid_of(n_triangles, 256), 256, 0, st>>>(triangles, n_triangles, w.tdrop, w.tpos, w.newid,
                                                                triangles_out, hdr);
  }
  return check_launch("slg_mesh_remove");
}

extern "C" int32_t slg_mesh_triangle_normals(const double* vertices, const int32_t* triangles, int64_t n_triangles,
                                             double* normals_out, void* stream) {
  if (n_triangles <= 0 || !vertices || !triangles || !normals_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_triangle_normals: no triangles or a NULL buffer");
  normals_kernel<<<grid_of(n_triangles, 256), 256, 0, (hipStream_t)stream>>>(vertices, triangles, n_triangles, normals_out);
  return check_launch("slg_mesh_triangle_normals");
}

extern "C" int32_t slg_mesh_stl_pack(const double* vertices, const int32_t* triangles, const double* normals,
                                     int64_t n_triangles, uint8_t* records_out, void* stream) {
  if (n_triangles <= 0 || !vertices || !triangles || !normals || !records_out || ((uintptr_t)records_out & 1))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_stl_pack: no triangles or a NULL or odd buffer");
  stl_pack_kernel<<<grid_of(n_triangles, 256), 256, 0, (hipStream_t)stream>>>(vertices, triangles, normals, n_triangles,
                                                                             (uint16_t*)records_out);
  return check_launch("slg_mesh_stl_pack");
}
