// cloud_band.hip -- the banded cascadic watertight mesher (include/slgpu_band.h):
// a dense solve at a base depth (cloud_mesh.hip's exports) carries the far field, every finer level
// exists only in blocks of 8^3 cells near the points, starts from the prolonged coarser solution and
// is smoothed by a fixed number of Jacobi sweeps, and the surface is extracted inside the finest
// band.  Everything that is not named here is §16's rule from mesh_rules.h; every rule is one
// __device__ function restated in tests/band_ref.py (on tests/mesh_ref.py); fp64 under
// -ffp-contract=off, integer atomics only (the status word and the header's counts), so the same
// input gives the same bits.
//
// Storage: a level of R cells has nb = R / 8 blocks per axis; block b owns the cells and the nodes
// [8 b, 8 b + 8) per axis, so the nodes fall into nb1^3 = (nb + 1)^3 node blocks.  `table` gives a
// stored node block's rank (ascending id) or -1, `ids` the id of a rank, a node field is
// double [n_blocks * 512] with entry rank * 512 + (lz 8 + ly) 8 + lx, and `inc` holds per stored
// node which of its 8 incident cells are active.  A scan over the stored nodes is therefore the
// order (block, local node) of the rule's vertices and triangles, without a sort.
#include "mesh_keys.h"
#include "mesh_rules.h"

#include "../../include/slgpu_band.h"

namespace slgband {

using slgcloud::block_tree_sum;
using slgcloud::Bump;
using slgcloud::grid_of;
using slgcloud::kChunk;
using slgmesh::MeshHdr;
using slgmeshpost::fits;
using slgmeshpost::scan_u8;

struct BandHdr {        // slgpu_band.h: the mesh header, then the level's counts
  MeshHdr m;
  double unused[7];
  unsigned long long stats[8];   // SLG_BAND_STAT_*
};
static_assert(sizeof(BandHdr) <= SLG_MESH_HDR_BYTES && offsetof(BandHdr, stats) == 128, "mesh.py's offsets");

constexpr int kB = SLG_BAND_BLOCK, kB3 = kB * kB * kB;
static_assert(kB == 8 && kB3 == 512, "the shifts and masks below");

static size_t cube(int64_t v) { return (size_t)v * (size_t)v * (size_t)v; }
static int nb1_of(int R) { return R / kB + 1; }
static bool level_R(int R) { return R >= kB && R <= (1 << SLG_BAND_MAX_DEPTH) && (R & (R - 1)) == 0; }
static size_t scan_temp(size_t n) { return n / 4 + (1u << 20); }                   // lookback states only
static size_t sort_pairs_temp(size_t n) { return 16 * n + (4u << 20); }            // 64-bit keys, 32-bit values: 12 n + lookback

struct I32OfU8 {
  __host__ __device__ int32_t operator()(uint8_t v) const { return v; }
};

// ---------------------------------------------------------------- workspace
struct BlocksWs { uint8_t* nodeblk; void* temp; size_t tb; };
static BlocksWs blocks_ws(Bump& b, int R) {
  BlocksWs w;
  const size_t m = cube(nb1_of(R));
  w.nodeblk = b.take<uint8_t>(m);
  w.tb = scan_temp(m);
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
struct SplatWs { uint64_t *keys, *keys_s; uint32_t *idx, *idx_s; void* temp; size_t tb; };
static SplatWs splat_ws(Bump& b, int64_t n) {
  SplatWs w;
  w.keys = b.take<uint64_t>(n);
  w.keys_s = b.take<uint64_t>(n);
  w.idx = b.take<uint32_t>(n);
  w.idx_s = b.take<uint32_t>(n);
  w.tb = sort_pairs_temp((size_t)n);
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
struct IsoWs { double *vals, *part; };
static IsoWs iso_ws(Bump& b, int64_t n) {
  IsoWs w;
  w.vals = b.take<double>(n);
  w.part = b.take<double>(grid_of(n, kChunk));
  return w;
}
struct ExtractWs { uint8_t *mask, *vcount, *tcount; uint64_t *vbase, *tbase; void* temp; size_t tb; };
static ExtractWs extract_ws(Bump& b, int64_t n_blocks) {
  ExtractWs w;
  const size_t m = (size_t)n_blocks * kB3;
  w.mask = b.take<uint8_t>(m);
  w.vcount = b.take<uint8_t>(m);
  w.tcount = b.take<uint8_t>(m);
  w.vbase = b.take<uint64_t>(m);
  w.tbase = b.take<uint64_t>(m);
  w.tb = scan_temp(m);
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
static size_t stage_bytes(int stage, int R, int64_t n, int64_t n_blocks) {
  Bump b(nullptr, 0);
  switch (stage) {
    case SLG_BAND_WS_BLOCKS: blocks_ws(b, R); break;
    case SLG_BAND_WS_SPLAT: splat_ws(b, n); break;
    case SLG_BAND_WS_ISO: iso_ws(b, n); break;
    case SLG_BAND_WS_EXTRACT: extract_ws(b, n_blocks); break;
    default: break;
  }
  return b.off;
}
static int bind(const char* who, void* ws, int64_t ws_bytes, size_t need) {
  return slgmeshpost::bind(who, "slg_band_ws_bytes", ws, ws_bytes, need);
}
// What every entry point asks of a level's arguments.
static int level_args(const char* who, int R, const void* hdr, int64_t n_blocks) {
  if (!level_R(R)) return slg_internal_fail(SLG_ERR_INVALID, "%s: R no power of two in 8..4096", who);
  if (!hdr || ((uintptr_t)hdr & 255)) return slg_internal_fail(SLG_ERR_INVALID, "%s: header NULL or not 256-byte aligned", who);
  if (n_blocks < 1 || (size_t)n_blocks > cube(nb1_of(R)))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: n_blocks outside 1..(R/8+1)^3", who);
  return SLG_OK;
}
static int points_args(const char* who, int64_t n) {
  if (n <= 0) return slg_internal_fail(SLG_ERR_INVALID, "%s: n <= 0", who);
  if (n > slgcloud::kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "%s: more than 2^30 points", who);
  return SLG_OK;
}

// ---------------------------------------------------------------- addressing
// A kernel of a level runs only on a good status and with the count of stored blocks the header holds.
__device__ inline bool live(const BandHdr* hdr, int64_t n_blocks) {
  return !hdr->m.status && (unsigned long long)n_blocks == hdr->stats[SLG_BAND_STAT_NODE_BLOCKS];
}
__device__ inline void block_xyz(uint32_t b, uint32_t nb1, int* x, int* y, int* z) {
  const uint32_t q = b / nb1;
  *x = (int)(b - q * nb1);
  *z = (int)(q / nb1);
  *y = (int)(q - (uint32_t)*z * nb1);
}
// The cell block (bx, by, bz)'s byte of a seed or active array; 0 outside the grid.
__device__ inline int block_flag(const uint8_t* __restrict__ a, int nb1, int bx, int by, int bz) {
  if ((unsigned)bx >= (unsigned)nb1 || (unsigned)by >= (unsigned)nb1 || (unsigned)bz >= (unsigned)nb1) return 0;
  return a[((size_t)bz * nb1 + by) * nb1 + bx];
}
// The slot of node (x, y, z) in a level's node fields; -1 when its block is not stored.
__device__ inline int64_t node_slot(const int32_t* __restrict__ table, int nb1, int64_t n_blocks, int x, int y, int z) {
  const int bx = x >> 3, by = y >> 3, bz = z >> 3;
  if ((unsigned)bx >= (unsigned)nb1 || (unsigned)by >= (unsigned)nb1 || (unsigned)bz >= (unsigned)nb1) return -1;
  const int32_t r = table[((size_t)bz * nb1 + by) * nb1 + bx];
  if (r < 0 || r >= n_blocks) return -1;
  return (int64_t)r * kB3 + (((z & 7) * kB + (y & 7)) * kB + (x & 7));
}
__device__ inline double node_value(const double* __restrict__ fld, const int32_t* __restrict__ table, int nb1,
                                    int64_t n_blocks, int x, int y, int z) {
  const int64_t s = node_slot(table, nb1, n_blocks, x, y, z);
  return s < 0 ? 0.0 : fld[s];
}
// Thread t of the workgroup of stored block `rank`: its node and its slot.
__device__ inline void stored_node(const int32_t* __restrict__ ids, int nb1, int* x, int* y, int* z) {
  int bx, by, bz;
  block_xyz((uint32_t)ids[blockIdx.x], (uint32_t)nb1, &bx, &by, &bz);
  const int t = threadIdx.x;
  *x = bx * kB + (t & 7);
  *y = by * kB + ((t >> 3) & 7);
  *z = bz * kB + (t >> 6);
}
// Trilinear value of a banded node field at p (§16's trilinear_rule; a node that is not stored reads as 0).
__device__ inline double band_trilinear_rule(const double* __restrict__ fld, const int32_t* __restrict__ table, int nb1,
                                             int64_t n_blocks, const double* p, const BandHdr* hdr) {
  const int R = hdr->m.R;
  int i[3];
  double t[3];
  for (int a = 0; a < 3; ++a) slgmesh::cell_rule(p[a], hdr->m.origin[a], hdr->m.h, R, &i[a], &t[a]);
  double acc = 0.0;
  for (int dz = 0; dz < 2; ++dz)
    for (int dy = 0; dy < 2; ++dy)
      for (int dx = 0; dx < 2; ++dx)
        acc = acc + slgmesh::corner_weight_rule(t, dx, dy, dz) * node_value(fld, table, nb1, n_blocks, i[0] + dx, i[1] + dy, i[2] + dz);
  return acc;
}
// The owned edge with corner code c lies in an active cell: one of the incident cells node - 1 + e
// with e = 1 on every axis the edge runs along.
__device__ inline bool edge_active_rule(int inc, int c) {
  int allow = 0;
  for (int e = 0; e < 8; ++e)
    if ((e & c) == c) allow |= 1 << e;
  return (inc & allow) != 0;
}

namespace {

using namespace slgmesh;

// ---------------------------------------------------------------- the level's header
__global__ void level_header_kernel(const MeshHdr* base, BandHdr* hdr, int R, double ratio) {
  hdr->m.status = base->status;
  hdr->m.R = R;
  hdr->m.nV = hdr->m.nT = 0;
  for (int a = 0; a < 3; ++a) hdr->m.origin[a] = base->origin[a];
  hdr->m.h = base->h / ratio;                  // a power of two: side / R exactly
  hdr->m.iso = hdr->m.thr = 0.0;
  for (int k = 0; k < 7; ++k) hdr->unused[k] = 0.0;
  for (int k = 0; k < 8; ++k) hdr->stats[k] = 0;
}

// ---------------------------------------------------------------- blocks
// A block is seeded when a point's cell lies in it (a plain store of 1 into the cleared array).
__global__ __launch_bounds__(256)
void seed_kernel(const BandHdr* hdr, const double* __restrict__ xyz, int64_t n, uint8_t* __restrict__ seed, int nb1) {
  if (hdr->m.status) return;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  int i[3];
  double t;
  for (int a = 0; a < 3; ++a) cell_rule(xyz[3 * j + a], hdr->m.origin[a], hdr->m.h, hdr->m.R, &i[a], &t);
  seed[((size_t)(i[2] >> 3) * nb1 + (i[1] >> 3)) * nb1 + (i[0] >> 3)] = 1;
}
// A block is active when it or one of its 26 neighbours inside the grid is seeded.
__global__ __launch_bounds__(256)
void active_kernel(BandHdr* hdr, const uint8_t* __restrict__ seed, uint8_t* __restrict__ active, int nb1) {
  if (hdr->m.status) return;
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in = g < (uint64_t)nb1 * nb1 * nb1;
  int s = 0, a = 0;
  if (in) {
    int bx, by, bz;
    block_xyz((uint32_t)g, (uint32_t)nb1, &bx, &by, &bz);
    if (bx < nb1 - 1 && by < nb1 - 1 && bz < nb1 - 1) {
      s = seed[g];
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) a |= block_flag(seed, nb1, bx + dx, by + dy, bz + dz);
    }
    active[g] = (uint8_t)(a ? 1 : 0);
  }
  const int ns = __syncthreads_count(s), na = __syncthreads_count(a);
  if (threadIdx.x == 0) {
    if (ns) atomicAdd(&hdr->stats[SLG_BAND_STAT_SEEDED], (unsigned long long)ns);
    if (na) atomicAdd(&hdr->stats[SLG_BAND_STAT_ACTIVE], (unsigned long long)na);
  }
}
// A node block holds a band node when one of the cell blocks b - {0, 1}^3 is active.
__global__ __launch_bounds__(256)
void node_block_kernel(const BandHdr* hdr, const uint8_t* __restrict__ active, uint8_t* __restrict__ nodeblk, int nb1) {
  if (hdr->m.status) return;
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (uint64_t)nb1 * nb1 * nb1) return;
  int bx, by, bz, a = 0;
  block_xyz((uint32_t)g, (uint32_t)nb1, &bx, &by, &bz);
  for (int ez = 0; ez < 2; ++ez)
    for (int ey = 0; ey < 2; ++ey)
      for (int ex = 0; ex < 2; ++ex) a |= block_flag(active, nb1, bx - ex, by - ey, bz - ez);
  nodeblk[g] = (uint8_t)(a ? 1 : 0);
}
// table (the exclusive scan of nodeblk) -> rank or -1; the last entry gives the count.
__global__ __launch_bounds__(256)
void table_kernel(BandHdr* hdr, const uint8_t* __restrict__ nodeblk, int32_t* __restrict__ table, uint64_t m) {
  if (hdr->m.status) return;
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= m) return;
  const int32_t r = table[g];
  if (g == m - 1) hdr->stats[SLG_BAND_STAT_NODE_BLOCKS] = (unsigned long long)(r + nodeblk[g]);
  table[g] = nodeblk[g] ? r : -1;
}
__global__ __launch_bounds__(256)
void block_ids_kernel(const BandHdr* hdr, const int32_t* __restrict__ table, int64_t n_blocks, int32_t* __restrict__ ids, uint64_t m) {
  if (!live(hdr, n_blocks)) return;
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= m) return;
  const int32_t r = table[g];
  if (r >= 0 && r < n_blocks) ids[r] = (int32_t)g;
}
// Per stored node: which of its 8 incident cells are active.
__global__ __launch_bounds__(512)
void incident_kernel(BandHdr* hdr, const uint8_t* __restrict__ active, const int32_t* __restrict__ ids, int64_t n_blocks,
                     uint8_t* __restrict__ inc, int nb1) {
  if (!live(hdr, n_blocks)) return;
  const int R = hdr->m.R;
  int x, y, z, m = 0;
  stored_node(ids, nb1, &x, &y, &z);
  for (int e = 0; e < 8; ++e) {
    const int cx = x - 1 + (e & 1), cy = y - 1 + ((e >> 1) & 1), cz = z - 1 + (e >> 2);
    if (cx < 0 || cy < 0 || cz < 0 || cx >= R || cy >= R || cz >= R) continue;
    if (block_flag(active, nb1, cx >> 3, cy >> 3, cz >> 3)) m |= 1 << e;
  }
  inc[(size_t)blockIdx.x * kB3 + threadIdx.x] = (uint8_t)m;
  const int nband = __syncthreads_count(m != 0), nint = __syncthreads_count(m == 255);
  if (threadIdx.x == 0) {
    if (nband) atomicAdd(&hdr->stats[SLG_BAND_STAT_BAND_NODES], (unsigned long long)nband);
    if (nint) atomicAdd(&hdr->stats[SLG_BAND_STAT_INTERIOR_NODES], (unsigned long long)nint);
  }
}

// ---------------------------------------------------------------- splat and divergence
__global__ __launch_bounds__(256)
void cell_keys_kernel(BandHdr* hdr, const double* __restrict__ xyz, const double* __restrict__ nrm, int64_t n,
                      uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  if (hdr->m.status) return;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int R = hdr->m.R;
  int i[3];
  double t;
  bool bad = false;
  for (int a = 0; a < 3; ++a) {
    cell_rule(xyz[3 * j + a], hdr->m.origin[a], hdr->m.h, R, &i[a], &t);
    if (!isfinite(nrm[3 * j + a])) bad = true;
  }
  if (bad) atomicOr(&hdr->m.status, SLG_FILTER_BAD_NONFINITE);
  keys[j] = ((uint64_t)i[2] * (uint64_t)R + (uint64_t)i[1]) * (uint64_t)R + (uint64_t)i[0];
  idx[j] = (uint32_t)j;
}
// §16's gather per stored node: its incident cells in ascending cell id, each cell's points in
// ascending input index, W += w and V += w * normal from 0.  An inactive cell holds no point and
// an active cell of an unseeded block neither, so neither is searched.
__global__ __launch_bounds__(512)
void splat_kernel(const BandHdr* hdr, const double* __restrict__ xyz, const double* __restrict__ nrm,
                  const uint64_t* __restrict__ keys_s, const uint32_t* __restrict__ idx_s, int64_t n,
                  const uint8_t* __restrict__ seed, const int32_t* __restrict__ ids, const uint8_t* __restrict__ inc,
                  int64_t n_blocks, double* __restrict__ W, double* __restrict__ V, int nb1) {
  if (!live(hdr, n_blocks)) return;
  const int R = hdr->m.R;
  int X, Y, Z;
  stored_node(ids, nb1, &X, &Y, &Z);
  const size_t g = (size_t)blockIdx.x * kB3 + threadIdx.x;
  const int m = inc[g];
  const double h = hdr->m.h, o[3] = {hdr->m.origin[0], hdr->m.origin[1], hdr->m.origin[2]};
  double w = 0.0, v[3] = {0.0, 0.0, 0.0};
  for (int ez = 0; ez < 2; ++ez)
    for (int ey = 0; ey < 2; ++ey)
      for (int ex = 0; ex < 2; ++ex) {
        if (!((m >> (ex + 2 * ey + 4 * ez)) & 1)) continue;
        const int cx = X - 1 + ex, cy = Y - 1 + ey, cz = Z - 1 + ez;
        if (!block_flag(seed, nb1, cx >> 3, cy >> 3, cz >> 3)) continue;
        const uint64_t key = ((uint64_t)cz * (uint64_t)R + (uint64_t)cy) * (uint64_t)R + (uint64_t)cx;
        for (int64_t j = slgmeshpost::lower_bound(keys_s, n, key); j < n && keys_s[j] == key; ++j) {
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
// f = div V by §16's central differences at interior nodes, 0 at every other stored node.
__global__ __launch_bounds__(512)
void divergence_kernel(const BandHdr* hdr, const double* __restrict__ V, const int32_t* __restrict__ table,
                       const int32_t* __restrict__ ids, const uint8_t* __restrict__ inc, int64_t n_blocks,
                       double* __restrict__ f, int nb1) {
  if (!live(hdr, n_blocks)) return;
  int x, y, z;
  stored_node(ids, nb1, &x, &y, &z);
  const size_t g = (size_t)blockIdx.x * kB3 + threadIdx.x;
  if (inc[g] != 255) { f[g] = 0.0; return; }
  double d[3];
  for (int a = 0; a < 3; ++a) {
    const int64_t lo = node_slot(table, nb1, n_blocks, x - (a == 0), y - (a == 1), z - (a == 2));
    const int64_t hi = node_slot(table, nb1, n_blocks, x + (a == 0), y + (a == 1), z + (a == 2));
    d[a] = (hi < 0 ? 0.0 : V[3 * hi + a]) - (lo < 0 ? 0.0 : V[3 * lo + a]);
  }
  const double th = 2.0 * hdr->m.h;
  f[g] = (d[0] / th + d[1] / th) + d[2] / th;
}

// ---------------------------------------------------------------- the cascade
// u = 0.125 * (0 + P(parent)) at band nodes off the box boundary, 0 at every other stored node.  P
// is §16's prolongation: per axis the coarse node x / 2 (even x) or the two around it with weight
// 1/2 each (odd x), z outermost, lower node first, from 0.  The parent is the dense base level
// (ptable null) or a banded one; the parents of a band node are band nodes (the bands nest).
__global__ __launch_bounds__(512)
void prolong_kernel(const BandHdr* hdr, const double* __restrict__ parent, const int32_t* __restrict__ ptable,
                    int64_t pblocks, const int32_t* __restrict__ ids, const uint8_t* __restrict__ inc, int64_t n_blocks,
                    double* __restrict__ u, int nb1) {
  if (!live(hdr, n_blocks)) return;
  const int R = hdr->m.R;
  int c[3];
  stored_node(ids, nb1, &c[0], &c[1], &c[2]);
  const size_t g = (size_t)blockIdx.x * kB3 + threadIdx.x;
  const bool edge = c[0] == 0 || c[1] == 0 || c[2] == 0 || c[0] >= R || c[1] >= R || c[2] >= R;
  if (!inc[g] || edge) { u[g] = 0.0; return; }
  const int64_t m1 = R / 2 + 1;
  const int pnb1 = R / 2 / kB + 1;
  int lo[3], cnt[3];
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
      for (int dx = 0; dx < cnt[0]; ++dx) {
        const double e = ptable ? node_value(parent, ptable, pnb1, pblocks, lo[0] + dx, lo[1] + dy, lo[2] + dz)
                                : parent[((lo[2] + dz) * m1 + (lo[1] + dy)) * m1 + (lo[0] + dx)];
        acc = acc + ((w[2] * w[1]) * w[0]) * e;
      }
  u[g] = 0.125 * (0.0 + acc);
}

// One damped Jacobi sweep of a banded level: one workgroup per stored block, one thread per node.
// The block's 8^3 values and the six face layers of its neighbours go through LDS (10^3 doubles,
// corners and edges unused); an interior node takes §16's update, every other stored node keeps
// its value.  24 bytes per node and sweep: u and f read, u written.
__global__ __launch_bounds__(512)
void smooth_kernel(const BandHdr* hdr, const int32_t* __restrict__ table, const int32_t* __restrict__ ids,
                   const uint8_t* __restrict__ inc, int64_t n_blocks, const double* __restrict__ f,
                   const double* __restrict__ u, double* __restrict__ out, int nb1) {
  __shared__ double tile[10][10][10];
  if (!live(hdr, n_blocks)) return;
  const int t = threadIdx.x, lx = t & 7, ly = (t >> 3) & 7, lz = t >> 6;
  const size_t g = (size_t)blockIdx.x * kB3 + t;
  const double uc = u[g];
  tile[lz + 1][ly + 1][lx + 1] = uc;
  if (t < 384) {                               // face t / 64: x-, x+, y-, y+, z-, z+; its 64 nodes (p, q)
    int bx, by, bz;
    block_xyz((uint32_t)ids[blockIdx.x], (uint32_t)nb1, &bx, &by, &bz);
    const int face = t >> 6, axis = face >> 1, side = face & 1, p = t & 7, q = (t >> 3) & 7;
    const int d = side ? 1 : -1;
    const int nx = bx + (axis == 0 ? d : 0), ny = by + (axis == 1 ? d : 0), nz = bz + (axis == 2 ? d : 0);
    int32_t r = -1;
    if ((unsigned)nx < (unsigned)nb1 && (unsigned)ny < (unsigned)nb1 && (unsigned)nz < (unsigned)nb1)
      r = table[((size_t)nz * nb1 + ny) * nb1 + nx];
    const int far = side ? 0 : 7, near = side ? 9 : 0;      // the neighbour's layer, and where it goes in the tile
    int sx, sy, sz, tx, ty, tz;
    if (axis == 0) { sx = far; sy = p; sz = q; tx = near; ty = p + 1; tz = q + 1; }
    else if (axis == 1) { sx = p; sy = far; sz = q; tx = p + 1; ty = near; tz = q + 1; }
    else { sx = p; sy = q; sz = far; tx = p + 1; ty = q + 1; tz = near; }
    tile[tz][ty][tx] = (r >= 0 && r < n_blocks) ? u[(size_t)r * kB3 + ((sz * kB + sy) * kB + sx)] : 0.0;
  }
  __syncthreads();
  double v = uc;
  if (inc[g] == 255) {
    const int X = lx + 1, Y = ly + 1, Z = lz + 1;
    const double S = ((((tile[Z][Y][X - 1] + tile[Z][Y][X + 1]) + tile[Z][Y - 1][X]) + tile[Z][Y + 1][X]) + tile[Z - 1][Y][X]) +
                     tile[Z + 1][Y][X];
    v = jacobi_rule(uc, S, f[g], hdr->m.h * hdr->m.h);
  }
  out[g] = v;
}

// ---------------------------------------------------------------- iso value
__global__ __launch_bounds__(256)
void sample_kernel(const BandHdr* hdr, const double* __restrict__ chi, const int32_t* __restrict__ table, int64_t n_blocks,
                   const double* __restrict__ xyz, int64_t n, double* __restrict__ out, int nb1) {
  if (!live(hdr, n_blocks)) return;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double p[3] = {xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]};
  out[j] = band_trilinear_rule(chi, table, nb1, n_blocks, p, hdr);
}
// The fixed tree of slg_cloud_centroid on one array (§16's iso value).
__global__ __launch_bounds__(256)
void sum_partial_kernel(const BandHdr* hdr, int64_t n_blocks, const double* __restrict__ v, int64_t n, double* __restrict__ part) {
  __shared__ double sm[256];
  if (!live(hdr, n_blocks)) return;
  const int64_t base = (int64_t)blockIdx.x * kChunk + threadIdx.x * (kChunk / 256);
  double s = 0.0;
  for (int j = 0; j < kChunk / 256; ++j)
    if (base + j < n) s += v[base + j];
  s = block_tree_sum(s, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256)
void iso_final_kernel(BandHdr* hdr, int64_t n_blocks, const double* __restrict__ part, int nb, int64_t n) {
  __shared__ double sm[256];
  if (!live(hdr, n_blocks)) return;
  double s = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) s += part[b];
  s = block_tree_sum(s, sm);
  if (threadIdx.x == 0) hdr->m.iso = s / (double)n;
}

// ---------------------------------------------------------------- marching tetrahedra inside the band
// bit c: corner code c of the cell at this node is inside; a corner that is not stored (it is no
// band node, so no active cell and no active edge reads it) counts as outside.
__device__ inline int corners_inside(const double* __restrict__ chi, const int32_t* __restrict__ table, int nb1,
                                     int64_t n_blocks, int x, int y, int z, double iso) {
  int in = 0;
  for (int c = 0; c < 8; ++c) {
    const int64_t s = node_slot(table, nb1, n_blocks, x + (c & 1), y + ((c >> 1) & 1), z + (c >> 2));
    if (s >= 0 && inside_rule(chi[s], iso)) in |= 1 << c;
  }
  return in;
}
// Per stored node: the mask of its owned edges that cross the iso value and lie in an active cell,
// their number, and the number of triangles of its cell's six tetrahedra when that cell is active.
__global__ __launch_bounds__(512)
void count_kernel(const BandHdr* hdr, const double* __restrict__ chi, const int32_t* __restrict__ table,
                  const int32_t* __restrict__ ids, const uint8_t* __restrict__ inc, int64_t n_blocks,
                  uint8_t* __restrict__ mask, uint8_t* __restrict__ vcount, uint8_t* __restrict__ tcount, int nb1) {
  if (!live(hdr, n_blocks)) return;
  int x, y, z;
  stored_node(ids, nb1, &x, &y, &z);
  const size_t g = (size_t)blockIdx.x * kB3 + threadIdx.x;
  const int nf = inc[g];
  int m = 0, nt = 0;
  if (nf) {
    const int in = corners_inside(chi, table, nb1, n_blocks, x, y, z, hdr->m.iso);
    for (int e = 0; e < 7; ++e) {
      const int c = kEdgeCode[e];
      if (edge_active_rule(nf, c) && ((in >> c) & 1) != (in & 1)) m |= 1 << e;
    }
    if (nf & 128)
      for (int k = 0; k < 6; ++k) {
        int pc = 0;
        for (int v = 0; v < 4; ++v) pc += (in >> kTetCode[k][v]) & 1;
        nt += pc == 2 ? 2 : (pc == 1 || pc == 3) ? 1 : 0;
      }
  }
  mask[g] = (uint8_t)m;
  vcount[g] = (uint8_t)__popc((unsigned)m);
  tcount[g] = (uint8_t)nt;
}
__global__ void totals_kernel(BandHdr* hdr, int64_t n_blocks, const uint8_t* vcount, const uint64_t* vbase,
                              const uint8_t* tcount, const uint64_t* tbase, size_t M) {
  if (!live(hdr, n_blocks)) return;
  hdr->m.nV = (int64_t)(vbase[M - 1] + vcount[M - 1]);
  hdr->m.nT = (int64_t)(tbase[M - 1] + tcount[M - 1]);
}
// Vertices in ascending (block, local node, edge type): §16's position and t; the density is the
// trilinear W at the vertex.
__global__ __launch_bounds__(512)
void vertices_kernel(const BandHdr* hdr, const double* __restrict__ chi, const double* __restrict__ W,
                     const int32_t* __restrict__ table, const int32_t* __restrict__ ids, int64_t n_blocks,
                     const uint8_t* __restrict__ mask, const uint64_t* __restrict__ vbase, double* __restrict__ vert,
                     double* __restrict__ dens, int64_t n_vertices, int nb1) {
  if (!live(hdr, n_blocks)) return;
  const size_t g = (size_t)blockIdx.x * kB3 + threadIdx.x;
  const int m = mask[g];
  if (!m) return;
  int c[3];
  stored_node(ids, nb1, &c[0], &c[1], &c[2]);
  const double iso = hdr->m.iso, h = hdr->m.h, ca = chi[g];
  uint64_t o = vbase[g];
  for (int e = 0; e < 7; ++e) {
    if (!((m >> e) & 1)) continue;
    const int code = kEdgeCode[e];
    const double cb = node_value(chi, table, nb1, n_blocks, c[0] + (code & 1), c[1] + ((code >> 1) & 1), c[2] + (code >> 2));
    const double t = (iso - ca) / (cb - ca);
    if (o >= (uint64_t)n_vertices) return;
    double p[3];
    for (int a = 0; a < 3; ++a) {
      const double pa = hdr->m.origin[a] + h * (double)c[a];
      const double pb = hdr->m.origin[a] + h * (double)(c[a] + ((code >> a) & 1));
      p[a] = pa + t * (pb - pa);
      vert[3 * o + a] = p[a];
    }
    if (dens) dens[o] = band_trilinear_rule(W, table, nb1, n_blocks, p, hdr);
    ++o;
  }
}
// Triangles in ascending (block, local cell, tetrahedron, triangle); a vertex id is its owner's base
// plus the number of the owner's vertices of lower type.
__global__ __launch_bounds__(512)
void triangles_kernel(const BandHdr* hdr, const double* __restrict__ chi, const int32_t* __restrict__ table,
                      const int32_t* __restrict__ ids, int64_t n_blocks, const uint8_t* __restrict__ mask,
                      const uint64_t* __restrict__ vbase, const uint8_t* __restrict__ tcount,
                      const uint64_t* __restrict__ tbase, int32_t* __restrict__ tris, int64_t n_triangles, int nb1) {
  if (!live(hdr, n_blocks)) return;
  const size_t g = (size_t)blockIdx.x * kB3 + threadIdx.x;
  if (!tcount[g]) return;
  int x, y, z;
  stored_node(ids, nb1, &x, &y, &z);
  const int in = corners_inside(chi, table, nb1, n_blocks, x, y, z, hdr->m.iso);
  uint64_t o = tbase[g];
  for (int k = 0; k < 6; ++k) {
    int m = 0;
    for (int v = 0; v < 4; ++v) m |= ((in >> kTetCode[k][v]) & 1) << v;
    int tri[2][3][2];
    const int nt = tet_case_rule(m, kTetOdd[k], tri);
    for (int j = 0; j < nt; ++j, ++o) {
      if (o >= (uint64_t)n_triangles) return;
      for (int e = 0; e < 3; ++e) {
        const int cp = kTetCode[k][tri[j][e][0]], cq = kTetCode[k][tri[j][e][1]];
        const int type = kTypeOfCode[cq ^ cp];
        const int64_t owner = node_slot(table, nb1, n_blocks, x + (cp & 1), y + ((cp >> 1) & 1), z + (cp >> 2));
        tris[3 * o + e] = owner < 0 ? -1 : (int32_t)(vbase[owner] + (uint64_t)__popc((unsigned)mask[owner] & ((1u << type) - 1u)));
      }
    }
  }
}

}  // namespace
}  // namespace slgband

using namespace slgband;

extern "C" int64_t slg_band_ws_bytes(int32_t stage, int32_t R, int64_t n, int64_t n_blocks) {
  if (stage < SLG_BAND_WS_BLOCKS || stage > SLG_BAND_WS_EXTRACT || n < 0 || n_blocks < 0)
    return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_band_ws_bytes: unknown stage or a negative count");
  if (stage == SLG_BAND_WS_BLOCKS && !level_R(R))
    return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_band_ws_bytes: R no power of two in 8..4096");
  if (stage == SLG_BAND_WS_EXTRACT && (n_blocks < 1 || n_blocks >= (1ll << 31)))
    return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_band_ws_bytes: n_blocks outside 1..2^31-1");
  if (n > slgcloud::kMaxPoints) return -(int64_t)slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_band_ws_bytes: more than 2^30 points");
  return (int64_t)stage_bytes(stage, R, n > 0 ? n : 1, n_blocks);
}

extern "C" int32_t slg_band_level(const void* base_ws, int32_t base_R, int32_t R, void* hdr, void* stream) {
  if (!base_ws || !hdr || ((uintptr_t)hdr & 255) || !level_R(R) || base_R < 4 || base_R >= R || (base_R & (base_R - 1)))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_band_level: a NULL or misaligned header, R no power of two in 8..4096 or "
                                              "base_R no power of two in 4..R/2");
  level_header_kernel<<<1, 1, 0, (hipStream_t)stream>>>((const MeshHdr*)base_ws, (BandHdr*)hdr, R, (double)(R / base_R));
  return check_launch("slg_band_level");
}

extern "C" int32_t slg_band_blocks(const double* xyz, int64_t n, int32_t R, void* hdr, uint8_t* seed, uint8_t* active,
                                   int32_t* table, void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = points_args("slg_band_blocks", n)) return rc;
  if (int rc = level_args("slg_band_blocks", R, hdr, 1)) return rc;
  if (!xyz || !seed || !active || !table) return slg_internal_fail(SLG_ERR_INVALID, "slg_band_blocks: a NULL buffer");
  if (int rc = bind("slg_band_blocks", ws, ws_bytes, stage_bytes(SLG_BAND_WS_BLOCKS, R, 0, 0))) return rc;
  Bump b(ws, 0);
  const BlocksWs w = blocks_ws(b, R);
  BandHdr* h = (BandHdr*)hdr;
  hipStream_t st = (hipStream_t)stream;
  const int nb1 = nb1_of(R);
  const size_t m = cube(nb1);
  const int g = (int)((m + 255) / 256);
  if (hipMemsetAsync(seed, 0, m, st) != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "slg_band_blocks: memset failed");
  seed_kernel<<<grid_of(n, 256), 256, 0, st>>>(h, xyz, n, seed, nb1);
  active_kernel<<<g, 256, 0, st>>>(h, seed, active, nb1);
  node_block_kernel<<<g, 256, 0, st>>>(h, active, w.nodeblk, nb1);
  auto it = rocprim::make_transform_iterator((const uint8_t*)w.nodeblk, I32OfU8());
  size_t need = 0;
  const hipError_t e = rocprim::exclusive_scan(nullptr, need, it, table, (int32_t)0, m, rocprim::plus<int32_t>(), st);
  if (int rc = fits("slg_band_blocks", e, need, w.tb)) return rc;
  size_t tb = w.tb;
  if (rocprim::exclusive_scan(w.temp, tb, it, table, (int32_t)0, m, rocprim::plus<int32_t>(), st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "slg_band_blocks: scan failed");
  table_kernel<<<g, 256, 0, st>>>(h, w.nodeblk, table, (uint64_t)m);
  return check_launch("slg_band_blocks");
}

extern "C" int32_t slg_band_nodes(int32_t R, void* hdr, const uint8_t* active, const int32_t* table, int64_t n_blocks,
                                  int32_t* block_ids, uint8_t* incident, void* stream) {
  if (int rc = level_args("slg_band_nodes", R, hdr, n_blocks)) return rc;
  if (!active || !table || !block_ids || !incident) return slg_internal_fail(SLG_ERR_INVALID, "slg_band_nodes: a NULL buffer");
  hipStream_t st = (hipStream_t)stream;
  const int nb1 = nb1_of(R);
  const size_t m = cube(nb1);
  block_ids_kernel<<<(int)((m + 255) / 256), 256, 0, st>>>((const BandHdr*)hdr, table, n_blocks, block_ids, (uint64_t)m);
  incident_kernel<<<(unsigned)n_blocks, kB3, 0, st>>>((BandHdr*)hdr, active, block_ids, n_blocks, incident, nb1);
  return check_launch("slg_band_nodes");
}

extern "C" int32_t slg_band_splat(const double* xyz, const double* normals, int64_t n, int32_t R, void* hdr,
                                  const uint8_t* seed, const int32_t* table, const int32_t* block_ids,
                                  const uint8_t* incident, int64_t n_blocks, void* ws, int64_t ws_bytes, double* W_out,
                                  double* V_out, void* stream) {
  if (int rc = points_args("slg_band_splat", n)) return rc;
  if (int rc = level_args("slg_band_splat", R, hdr, n_blocks)) return rc;
  if (!xyz || !normals || !seed || !table || !block_ids || !incident || !W_out || !V_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_band_splat: a NULL buffer (the splat needs normals)");
  if (int rc = bind("slg_band_splat", ws, ws_bytes, stage_bytes(SLG_BAND_WS_SPLAT, R, n, 0))) return rc;
  Bump b(ws, 0);
  const SplatWs w = splat_ws(b, n);
  BandHdr* h = (BandHdr*)hdr;
  hipStream_t st = (hipStream_t)stream;
  cell_keys_kernel<<<grid_of(n, 256), 256, 0, st>>>(h, xyz, normals, n, w.keys, w.idx);
  unsigned bits = 0;
  while ((1 << bits) < R) ++bits;
  bits *= 3;
  size_t need = 0;
  const hipError_t e = rocprim::radix_sort_pairs(nullptr, need, (const uint64_t*)w.keys, w.keys_s, (const uint32_t*)w.idx, w.idx_s,
                                                 (size_t)n, 0u, bits, st);
  if (int rc = fits("slg_band_splat", e, need, w.tb)) return rc;
  size_t tb = w.tb;
  if (rocprim::radix_sort_pairs(w.temp, tb, (const uint64_t*)w.keys, w.keys_s, (const uint32_t*)w.idx, w.idx_s, (size_t)n, 0u, bits,
                                st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "slg_band_splat: radix sort failed");
  splat_kernel<<<(unsigned)n_blocks, kB3, 0, st>>>(h, xyz, normals, w.keys_s, w.idx_s, n, seed, block_ids, incident, n_blocks, W_out,
                                                  V_out, nb1_of(R));
  return check_launch("slg_band_splat");
}

extern "C" int32_t slg_band_divergence(const double* V, int32_t R, const void* hdr, const int32_t* table,
                                       const int32_t* block_ids, const uint8_t* incident, int64_t n_blocks, double* f_out,
                                       void* stream) {
  if (int rc = level_args("slg_band_divergence", R, hdr, n_blocks)) return rc;
  if (!V || !table || !block_ids || !incident || !f_out) return slg_internal_fail(SLG_ERR_INVALID, "slg_band_divergence: a NULL buffer");
  divergence_kernel<<<(unsigned)n_blocks, kB3, 0, (hipStream_t)stream>>>((const BandHdr*)hdr, V, table, block_ids, incident, n_blocks,
                                                                        f_out, nb1_of(R));
  return check_launch("slg_band_divergence");
}

extern "C" int32_t slg_band_prolong(const double* parent, const int32_t* parent_table, int64_t parent_blocks, int32_t R,
                                    const void* hdr, const int32_t* block_ids, const uint8_t* incident, int64_t n_blocks,
                                    double* u_out, void* stream) {
  if (int rc = level_args("slg_band_prolong", R, hdr, n_blocks)) return rc;
  if (!parent || !block_ids || !incident || !u_out) return slg_internal_fail(SLG_ERR_INVALID, "slg_band_prolong: a NULL buffer");
  if (parent_table && (R < 2 * kB || parent_blocks < 1 || (size_t)parent_blocks > cube(nb1_of(R / 2))))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_band_prolong: a banded parent needs R >= 16 and parent_blocks in 1..(R/16+1)^3");
  prolong_kernel<<<(unsigned)n_blocks, kB3, 0, (hipStream_t)stream>>>((const BandHdr*)hdr, parent, parent_table, parent_blocks,
                                                                     block_ids, incident, n_blocks, u_out, nb1_of(R));
  return check_launch("slg_band_prolong");
}

extern "C" int32_t slg_band_smooth(const double* f, int32_t R, const void* hdr, const int32_t* table,
                                   const int32_t* block_ids, const uint8_t* incident, int64_t n_blocks, int32_t sweeps,
                                   double* u, double* tmp, void* stream) {
  if (int rc = level_args("slg_band_smooth", R, hdr, n_blocks)) return rc;
  if (!f || !table || !block_ids || !incident || !u || !tmp || u == tmp || sweeps < 0)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_band_smooth: a NULL buffer, u == tmp or sweeps < 0");
  const int nb1 = nb1_of(R);
  for (int s = 0; s < sweeps; ++s) {
    smooth_kernel<<<(unsigned)n_blocks, kB3, 0, (hipStream_t)stream>>>((const BandHdr*)hdr, table, block_ids, incident, n_blocks, f,
                                                                      s & 1 ? tmp : u, s & 1 ? u : tmp, nb1);
  }
  return check_launch("slg_band_smooth");
}

extern "C" int32_t slg_band_iso(const double* chi, const double* xyz, int64_t n, int32_t R, void* hdr, const int32_t* table,
                                int64_t n_blocks, void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = points_args("slg_band_iso", n)) return rc;
  if (int rc = level_args("slg_band_iso", R, hdr, n_blocks)) return rc;
  if (!chi || !xyz || !table) return slg_internal_fail(SLG_ERR_INVALID, "slg_band_iso: a NULL buffer");
  if (int rc = bind("slg_band_iso", ws, ws_bytes, stage_bytes(SLG_BAND_WS_ISO, R, n, 0))) return rc;
  Bump b(ws, 0);
  const IsoWs w = iso_ws(b, n);
  BandHdr* h = (BandHdr*)hdr;
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(n, kChunk);
  sample_kernel<<<grid_of(n, 256), 256, 0, st>>>(h, chi, table, n_blocks, xyz, n, w.vals, nb1_of(R));
  sum_partial_kernel<<<nb, 256, 0, st>>>(h, n_blocks, w.vals, n, w.part);
  iso_final_kernel<<<1, 256, 0, st>>>(h, n_blocks, w.part, nb, n);
  return check_launch("slg_band_iso");
}

extern "C" int32_t slg_band_count(const double* chi, int32_t R, void* hdr, const int32_t* table, const int32_t* block_ids,
                                  const uint8_t* incident, int64_t n_blocks, void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = level_args("slg_band_count", R, hdr, n_blocks)) return rc;
  if (!chi || !table || !block_ids || !incident) return slg_internal_fail(SLG_ERR_INVALID, "slg_band_count: a NULL buffer");
  if (int rc = bind("slg_band_count", ws, ws_bytes, stage_bytes(SLG_BAND_WS_EXTRACT, R, 0, n_blocks))) return rc;
  Bump b(ws, 0);
  const ExtractWs w = extract_ws(b, n_blocks);
  BandHdr* h = (BandHdr*)hdr;
  hipStream_t st = (hipStream_t)stream;
  const size_t M = (size_t)n_blocks * kB3;
  count_kernel<<<(unsigned)n_blocks, kB3, 0, st>>>(h, chi, table, block_ids, incident, n_blocks, w.mask, w.vcount, w.tcount, nb1_of(R));
  if (int rc = scan_u8("slg_band_count", w.vcount, w.vbase, M, w.temp, w.tb, st)) return rc;
  if (int rc = scan_u8("slg_band_count", w.tcount, w.tbase, M, w.temp, w.tb, st)) return rc;
  totals_kernel<<<1, 1, 0, st>>>(h, n_blocks, w.vcount, w.vbase, w.tcount, w.tbase, M);
  return check_launch("slg_band_count");
}

extern "C" int32_t slg_band_emit(const double* chi, const double* W, int32_t R, const void* hdr, const int32_t* table,
                                 const int32_t* block_ids, const uint8_t* incident, int64_t n_blocks, void* ws,
                                 int64_t ws_bytes, double* vertices_out, int64_t n_vertices, double* densities_out,
                                 int32_t* triangles_out, int64_t n_triangles, void* stream) {
  if (int rc = level_args("slg_band_emit", R, hdr, n_blocks)) return rc;
  if (!chi || !table || !block_ids || !incident || n_vertices < 0 || n_triangles < 0 || (n_vertices && !vertices_out) ||
      (n_triangles && !triangles_out) || (W && n_vertices && !densities_out))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_band_emit: a NULL buffer or a negative count");
  if (n_vertices >= (1ll << 31)) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_band_emit: 2^31 vertices or more");
  if (int rc = bind("slg_band_emit", ws, ws_bytes, stage_bytes(SLG_BAND_WS_EXTRACT, R, 0, n_blocks))) return rc;
  Bump b(ws, 0);
  const ExtractWs w = extract_ws(b, n_blocks);
  const BandHdr* h = (const BandHdr*)hdr;
  hipStream_t st = (hipStream_t)stream;
  const int nb1 = nb1_of(R);
  if (n_vertices)
    vertices_kernel<<<(unsigned)n_blocks, kB3, 0, st>>>(h, chi, W, table, block_ids, n_blocks, w.mask, w.vbase, vertices_out,
                                                       W ? densities_out : nullptr, n_vertices, nb1);
  if (n_triangles)
    triangles_kernel<<<(unsigned)n_blocks, kB3, 0, st>>>(h, chi, table, block_ids, n_blocks, w.mask, w.vbase, w.tcount, w.tbase,
                                                        triangles_out, n_triangles, nb1);
  return check_launch("slg_band_emit");
}
