// cloud_audit.hip -- the audit of an indexed triangle mesh in HBM: edge classes,
// duplicated and degenerate triangles, connected components, vertex fans, signed volume and area,
// and the selection that keeps chosen triangles with the vertices they use.  Our rules, Open3D /
// MeshLab parity unpinned; every rule is restated in tests/audit_ref.py.  fp64 under
// -ffp-contract=off in fixed-order trees and integer atomics only, so the same input gives the same
// bits.  Self-intersection is not tested.
//
// An undirected edge (min, max) is the 64-bit key min << 32 | max (mesh_keys.h), its value the
// position 3 t + e with the direction bit on top; one stable radix sort of the pairs puts every edge
// into a run whose positions ascend, and everything about connectivity is a binary search in the
// sorted keys and a union-find over the runs.
//
// The union-find is cloud_cluster.hip's, restated: parent[x] <= x and an entry only ever decreases
// (every write is an atomic min), so the structure is acyclic, every find ends and a set's root is
// its smallest index, whatever the order of the unions.  Inside a union kernel every access to
// parent is an agent-scope atomic: a plain load could be served from a stale line.
#include "mesh_keys.h"

#include "../../include/slgpu_audit.h"

namespace slgaudit {

using namespace slgmeshpost;
using slgcloud::block_tree_sum;
using slgcloud::kNone;

constexpr int kChunk = SLG_AUDIT_CHUNK;
constexpr uint32_t kDirBit = 0x80000000u;

struct AuditHdr {
  int32_t status;       // SLG_FILTER_BAD_INDEX
  int32_t R;            // unused
  int64_t nV, nT;       // audit: the referenced vertices; select: the new counts
  int64_t nC;           // components
  int64_t largest;      // triangles of the largest component
  unsigned long long best;   // (size << 32) | ~label by atomicMax
  double unused[10];
  int64_t stats[8];     // SLG_AUDIT_STAT_*
};
static_assert(sizeof(AuditHdr) <= SLG_MESH_HDR_BYTES, "header");
static_assert(offsetof(AuditHdr, nV) == 8 && offsetof(AuditHdr, nT) == 16 && offsetof(AuditHdr, nC) == 24 &&
              offsetof(AuditHdr, largest) == 32 && offsetof(AuditHdr, stats) == 128, "mesh.py's offsets");

// ---------------------------------------------------------------- workspace
struct AuditWs { uint64_t *k, *s, *tpos; uint32_t *val, *sval, *parent, *root, *cparent, *vroot, *vbits; uint8_t *tflag, *vbad;
                 void* temp; size_t tb; };
static AuditWs audit_ws(Bump& b, int64_t nv, int64_t nt) {
  AuditWs w;
  const size_t n3 = 3 * (size_t)nt;
  w.k = b.take<uint64_t>(n3);
  w.s = b.take<uint64_t>(n3);
  w.val = b.take<uint32_t>(n3);
  w.sval = b.take<uint32_t>(n3);
  w.parent = b.take<uint32_t>(nt);
  w.root = b.take<uint32_t>(nt);
  w.tflag = b.take<uint8_t>(nt);
  w.tpos = b.take<uint64_t>(nt);
  w.cparent = b.take<uint32_t>(n3);
  w.vroot = b.take<uint32_t>(nv);
  w.vbits = b.take<uint32_t>(nv);
  w.vbad = b.take<uint8_t>(nv);
  w.tb = sort_pairs_temp(n3);
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
struct MeasureWs { double* part; };
static MeasureWs measure_ws(Bump& b, int64_t nt) {
  MeasureWs w;
  w.part = b.take<double>(2 * (size_t)grid_of(nt, kChunk));
  return w;
}
struct SelectWs { uint8_t *tflag, *vref; uint64_t *tpos, *vpos; void* temp; size_t tb; };
static SelectWs select_ws(Bump& b, int64_t nv, int64_t nt) {
  SelectWs w;
  w.tflag = b.take<uint8_t>(nt);
  w.vref = b.take<uint8_t>(nv);
  w.tpos = b.take<uint64_t>(nt);
  w.vpos = b.take<uint64_t>(nv);
  w.tb = sort_temp((size_t)(nv > nt ? nv : nt));
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
static size_t stage_bytes(int stage, int64_t nv, int64_t nt) {
  Bump b(nullptr, SLG_MESH_HDR_BYTES);
  if (stage == SLG_AUDIT_WS_AUDIT) audit_ws(b, nv, nt);
  else if (stage == SLG_AUDIT_WS_MEASURE) measure_ws(b, nt);
  else select_ws(b, nv, nt);
  return b.off;
}

namespace {

// ---------------------------------------------------------------- union-find (cloud_cluster.hip's)
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
// Joins the sets of a and b.  When the min lands on an entry that was no longer a root
// (old != hi), hi now points at min(old, lo) and the loop joins old with lo, which puts back
// whatever that write took apart; max(a, b) falls every round.
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

// One add per wave of the lanes where `on` holds.
__device__ inline void wave_count(int64_t* dst, bool on) {
  const unsigned long long m = __ballot(on);
  if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd((unsigned long long*)dst, (unsigned long long)__popcll(m));
}

// ---------------------------------------------------------------- edges
// Per triangle: its class byte, the referenced bit of its vertices and its three pairs.  A
// degenerate triangle and one with an index outside 0 .. V - 1 (which sets the status word) give
// the sentinel (V, 0), which sorts behind every edge.
__global__ __launch_bounds__(256)
void edge_keys_kernel(AuditHdr* hdr, const int32_t* __restrict__ tris, int64_t nt, int64_t nv, uint64_t* __restrict__ k,
                      uint32_t* __restrict__ val, uint8_t* __restrict__ tclass, uint32_t* __restrict__ vbits) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool degenerate = false;
  if (t < nt) {
    const int32_t v[3] = {tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]};
    const bool bad = v[0] < 0 || v[1] < 0 || v[2] < 0 || v[0] >= nv || v[1] >= nv || v[2] >= nv;
    if (bad) atomicOr(&hdr->status, SLG_FILTER_BAD_INDEX);
    degenerate = !bad && (v[0] == v[1] || v[1] == v[2] || v[2] == v[0]);
    tclass[t] = degenerate ? SLG_AUDIT_TRIANGLE_DEGENERATE : 0;
    if (!bad)
      for (int e = 0; e < 3; ++e) atomicOr(&vbits[v[e]], (uint32_t)SLG_AUDIT_VERTEX_REFERENCED);
    const uint64_t none = edge_key((uint32_t)nv, 0u);
    for (int e = 0; e < 3; ++e) {
      const uint32_t a = (uint32_t)v[e], b = (uint32_t)v[e == 2 ? 0 : e + 1];
      const uint32_t pos = (uint32_t)(3 * t + e);
      k[3 * t + e] = bad || degenerate ? none : edge_key(a < b ? a : b, a < b ? b : a);
      val[3 * t + e] = pos | (a > b ? kDirBit : 0u);
    }
  }
  wave_count(&hdr->stats[SLG_AUDIT_STAT_DEGENERATE], degenerate);
}

// The vertex of triangle t that is not on its edge e.
__device__ inline int32_t third_vertex(const int32_t* __restrict__ tris, uint32_t pos) {
  const uint32_t t = pos / 3, e = pos - 3 * t;
  return tris[3 * (int64_t)t + (e + 2) % 3];
}

// One lane per sorted entry.  A run's first entry counts the run and marks its two vertices; the
// entry of a triangle's edge between its two smallest indices looks through the run's earlier
// entries for a triangle with the same third vertex (the duplicate rule).
__global__ __launch_bounds__(256)
void edge_class_kernel(AuditHdr* hdr, const int32_t* __restrict__ tris, const uint64_t* __restrict__ s,
                       const uint32_t* __restrict__ sval, int64_t n, int64_t nv, uint32_t* __restrict__ vbits,
                       uint8_t* __restrict__ tclass) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int m = 0;
  bool inconsistent = false, duplicate = false;
  if (i < n) {
    const uint64_t key = s[i];
    if (key_src(key) < (uint64_t)nv) {
      const int64_t lb = lower_bound(s, n, key);
      if (lb == i) {
        const int64_t ub = lower_bound(s, n, key + 1);
        m = (int)(ub - lb > 3 ? 3 : ub - lb);
        inconsistent = m == 2 && ((sval[i] ^ sval[i + 1]) & kDirBit) == 0;
        const uint32_t bits = (m == 1 ? SLG_AUDIT_VERTEX_BOUNDARY : 0) | (m == 3 ? SLG_AUDIT_VERTEX_NONMANIFOLD_EDGE : 0) |
                              (inconsistent ? SLG_AUDIT_VERTEX_INCONSISTENT : 0);
        if (bits) {                              // (nothing to add on a consistent manifold edge)
          atomicOr(&vbits[key_src(key)], bits);
          atomicOr(&vbits[key_dst(key)], bits);
        }
      }
      const uint32_t pos = sval[i] & ~kDirBit;
      const int32_t c = third_vertex(tris, pos);
      if ((uint64_t)(uint32_t)c > key_dst(key)) {          // this edge joins the triangle's two smallest indices
        for (int64_t j = lb; j < i && !duplicate; ++j) duplicate = third_vertex(tris, sval[j] & ~kDirBit) == c;
        if (duplicate) tclass[pos / 3] = SLG_AUDIT_TRIANGLE_DUPLICATE;
      }
    }
  }
  wave_count(&hdr->stats[SLG_AUDIT_STAT_EDGES], m > 0);
  wave_count(&hdr->stats[SLG_AUDIT_STAT_BOUNDARY], m == 1);
  wave_count(&hdr->stats[SLG_AUDIT_STAT_MANIFOLD], m == 2);
  wave_count(&hdr->stats[SLG_AUDIT_STAT_NONMANIFOLD], m == 3);
  wave_count(&hdr->stats[SLG_AUDIT_STAT_INCONSISTENT], inconsistent);
  wave_count(&hdr->stats[SLG_AUDIT_STAT_DUPLICATES], duplicate);
}

__global__ __launch_bounds__(256)
void vertex_class_kernel(AuditHdr* hdr, const uint32_t* __restrict__ vbits, int64_t nv, uint8_t* __restrict__ vclass) {
  if (hdr->status) return;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t b = v < nv ? vbits[v] : 0u;
  if (v < nv) vclass[v] = (uint8_t)b;
  wave_count(&hdr->nV, (b & SLG_AUDIT_VERTEX_REFERENCED) != 0);
}

// ---------------------------------------------------------------- components
__global__ __launch_bounds__(256) void iota_kernel(const AuditHdr* hdr, uint32_t* __restrict__ p, int64_t n) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = (uint32_t)i;
}
// Every entry behind its run's first joins its triangle to the first's: m - 1 unions per run.
__global__ __launch_bounds__(256)
void tri_union_kernel(const AuditHdr* hdr, const uint64_t* __restrict__ s, const uint32_t* __restrict__ sval, int64_t n,
                      int64_t nv, uint32_t* parent) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = s[i];
  if (key_src(key) >= (uint64_t)nv) return;
  const int64_t lb = lower_bound(s, n, key);
  if (lb == i) return;
  uf_unite(parent, (sval[i] & ~kDirBit) / 3, (sval[lb] & ~kDirBit) / 3);
}
__global__ __launch_bounds__(256)
void tri_root_kernel(const AuditHdr* hdr, const uint8_t* __restrict__ tclass, int64_t nt, uint32_t* parent,
                     uint32_t* __restrict__ root, uint8_t* __restrict__ flag) {
  if (hdr->status) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  const uint32_t r = (tclass[t] & SLG_AUDIT_TRIANGLE_DEGENERATE) ? kNone : uf_find(parent, (uint32_t)t);
  root[t] = r;
  flag[t] = r == (uint32_t)t ? 1 : 0;
}
__global__ __launch_bounds__(256)
void tri_label_kernel(AuditHdr* hdr, const uint32_t* __restrict__ root, const uint8_t* __restrict__ flag,
                      const uint64_t* __restrict__ pos, int64_t nt, int32_t* __restrict__ labels) {
  if (hdr->status) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  const uint32_t r = root[t];
  labels[t] = r == kNone ? -1 : (int32_t)pos[r];
  if (t == nt - 1) hdr->nC = (int64_t)(pos[t] + flag[t]);
}
// Members per label: integer atomics, one per distinct label of a wave.
__global__ __launch_bounds__(256)
void label_sizes_kernel(const AuditHdr* hdr, const int32_t* __restrict__ labels, int64_t nt, int64_t nc,
                        int64_t* __restrict__ sizes) {
  if (hdr->status) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int32_t l = t < nt ? labels[t] : -1;
  bool todo = l >= 0 && l < nc;
  for (;;) {
    const unsigned long long open = __ballot(todo);
    if (!open) break;
    const int leader = __ffsll((long long)open) - 1;
    const int32_t l0 = __shfl(l, leader, 64);
    const unsigned long long same = __ballot(todo && l == l0);
    if (lane == leader) atomicAdd((unsigned long long*)&sizes[l0], (unsigned long long)__popcll(same));
    if (l == l0) todo = false;
  }
}
__global__ __launch_bounds__(256) void label_best_kernel(AuditHdr* hdr, const int64_t* __restrict__ sizes, int64_t nc) {
  if (hdr->status) return;
  const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (l >= nc) return;
  atomicMax(&hdr->best, ((unsigned long long)(uint32_t)sizes[l] << 32) | (uint32_t)~(uint32_t)l);
}
__global__ void label_largest_kernel(AuditHdr* hdr) {
  if (hdr->status) return;
  hdr->largest = (int64_t)(hdr->best >> 32);
}

// ---------------------------------------------------------------- vertex fans
// The corner 3 t + j of the entry's triangle at the edge's smaller (which = 0) or larger vertex.
__device__ inline uint32_t edge_corner(uint32_t v, int which) {
  const uint32_t pos = v & ~kDirBit, t = pos / 3, e = pos - 3 * t;
  const bool swapped = (v & kDirBit) != 0;               // the winding goes max -> min: corner e is at max
  const uint32_t at_e = 3 * t + e, at_next = 3 * t + (e + 1) % 3;
  return (which == 0) != swapped ? at_e : at_next;
}
__global__ __launch_bounds__(256)
void corner_union_kernel(const AuditHdr* hdr, const uint64_t* __restrict__ s, const uint32_t* __restrict__ sval, int64_t n,
                         int64_t nv, uint32_t* cparent) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = s[i];
  if (key_src(key) >= (uint64_t)nv) return;
  const int64_t lb = lower_bound(s, n, key);
  if (lb == i) return;
  const uint32_t a = sval[i], b = sval[lb];
  uf_unite(cparent, edge_corner(a, 0), edge_corner(b, 0));
  uf_unite(cparent, edge_corner(a, 1), edge_corner(b, 1));
}
// pass 0: vroot[v] = the smallest root among v's corners; pass 1: a corner with another root marks v.
__global__ __launch_bounds__(256)
void corner_root_kernel(const AuditHdr* hdr, const int32_t* __restrict__ tris, const uint8_t* __restrict__ tclass, int64_t n,
                        uint32_t* cparent, uint32_t* __restrict__ vroot, uint8_t* __restrict__ vbad, int pass) {
  if (hdr->status) return;
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n || (tclass[c / 3] & SLG_AUDIT_TRIANGLE_DEGENERATE)) return;
  const uint32_t r = uf_find(cparent, (uint32_t)c);
  const int32_t v = tris[c];
  if (pass == 0) atomicMin(&vroot[v], r);
  else if (vroot[v] != r) vbad[v] = 1;
}
__global__ __launch_bounds__(256)
void fan_class_kernel(AuditHdr* hdr, const uint8_t* __restrict__ vbad, int64_t nv, uint8_t* __restrict__ vclass) {
  if (hdr->status) return;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool bad = v < nv && vbad[v] != 0;
  if (v < nv) vclass[v] = (uint8_t)((vclass[v] & ~SLG_AUDIT_VERTEX_NONMANIFOLD) | (bad ? SLG_AUDIT_VERTEX_NONMANIFOLD : 0));
  wave_count(&hdr->stats[SLG_AUDIT_STAT_NONMANIFOLD_VERTICES], bad);
}

// ---------------------------------------------------------------- measures
// A triangle's two terms, every product and sum as tests/audit_ref.py names them.
__device__ inline void measure_terms(const double* a, const double* b, const double* c, double* vol, double* area) {
  const double cx = b[1] * c[2] - b[2] * c[1], cy = b[2] * c[0] - b[0] * c[2], cz = b[0] * c[1] - b[1] * c[0];
  *vol = ((a[0] * cx + a[1] * cy) + a[2] * cz) / 6.0;
  const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const double nx = u[1] * v[2] - u[2] * v[1], ny = u[2] * v[0] - u[0] * v[2], nz = u[0] * v[1] - u[1] * v[0];
  *area = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
}
// kChunk triangles per workgroup: 8 consecutive per thread, the workgroup's tree (the shape of
// cloud_normals.hip's axis sums).
__global__ __launch_bounds__(256)
void measure_partial_kernel(AuditHdr* hdr, const double* __restrict__ vert, int64_t nv, const int32_t* __restrict__ tris,
                            int64_t nt, double* __restrict__ part) {
  __shared__ double sm[256];
  const int64_t base = (int64_t)blockIdx.x * kChunk + threadIdx.x * (kChunk / 256);
  double sv = 0.0, sa = 0.0;
  for (int j = 0; j < kChunk / 256; ++j) {
    const int64_t t = base + j;
    if (t >= nt) break;
    const int32_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) {
      atomicOr(&hdr->status, SLG_FILTER_BAD_INDEX);
      continue;
    }
    if (i0 == i1 || i1 == i2 || i2 == i0) continue;
    const double a[3] = {vert[3 * (int64_t)i0], vert[3 * (int64_t)i0 + 1], vert[3 * (int64_t)i0 + 2]};
    const double b[3] = {vert[3 * (int64_t)i1], vert[3 * (int64_t)i1 + 1], vert[3 * (int64_t)i1 + 2]};
    const double c[3] = {vert[3 * (int64_t)i2], vert[3 * (int64_t)i2 + 1], vert[3 * (int64_t)i2 + 2]};
    double vol, area;
    measure_terms(a, b, c, &vol, &area);
    sv = sv + vol;
    sa = sa + area;
  }
  sv = block_tree_sum(sv, sm);
  __syncthreads();                           // sm[0] has been read before the next sum overwrites it
  sa = block_tree_sum(sa, sm);
  if (threadIdx.x == 0) {
    part[2 * (int64_t)blockIdx.x] = sv;
    part[2 * (int64_t)blockIdx.x + 1] = sa;
  }
}
__global__ __launch_bounds__(256)
void measure_final_kernel(const AuditHdr* hdr, const double* __restrict__ part, int nb, double* __restrict__ out) {
  __shared__ double sm[256];
  if (hdr->status) return;
  for (int a = 0; a < 2; ++a) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) s = s + part[2 * (int64_t)b + a];
    s = block_tree_sum(s, sm);
    if (threadIdx.x == 0) out[a] = s;
    __syncthreads();
  }
}

// ---------------------------------------------------------------- keep and select
__global__ __launch_bounds__(256)
void keep_kernel(const uint8_t* __restrict__ tclass, const int32_t* __restrict__ labels, int64_t nt,
                 const uint8_t* __restrict__ table, int64_t nc, int drop_bits, uint8_t* __restrict__ keep) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  bool on = !(tclass && (tclass[t] & drop_bits));
  if (on && table) {
    const int32_t l = labels[t];
    on = l >= 0 && l < nc && table[l] != 0;
  }
  keep[t] = on ? 1 : 0;
}
__global__ __launch_bounds__(256)
void select_flag_kernel(AuditHdr* hdr, const int32_t* __restrict__ tris, int64_t nt, int64_t nv, const uint8_t* __restrict__ keep,
                        uint8_t* __restrict__ tflag, uint8_t* __restrict__ vref) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  const int32_t a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
  const bool bad = a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv;
  if (bad) atomicOr(&hdr->status, SLG_FILTER_BAD_INDEX);
  const bool on = !bad && keep[t] != 0;
  tflag[t] = on ? 1 : 0;
  if (on) vref[a] = vref[b] = vref[c] = 1;   // the same byte from every lane that writes it
}
__global__ __launch_bounds__(256)
void select_vertices_kernel(const AuditHdr* hdr, const double* __restrict__ vert, const double* __restrict__ dens, int64_t nv,
                            const uint8_t* __restrict__ vref, const uint64_t* __restrict__ vpos, double* __restrict__ vert_out,
                            double* __restrict__ dens_out) {
  if (hdr->status) return;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv || !vref[v]) return;
  const uint64_t o = vpos[v];
  for (int a = 0; a < 3; ++a) vert_out[3 * o + a] = vert[3 * v + a];
  if (dens) dens_out[o] = dens[v];
}
__global__ __launch_bounds__(256)
void select_triangles_kernel(AuditHdr* hdr, const int32_t* __restrict__ tris, int64_t nt, int64_t nv,
                             const uint8_t* __restrict__ tflag, const uint64_t* __restrict__ tpos,
                             const uint8_t* __restrict__ vref, const uint64_t* __restrict__ vpos, int32_t* __restrict__ tris_out) {
  if (hdr->status) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  if (tflag[t]) {
    const uint64_t o = tpos[t];
    for (int a = 0; a < 3; ++a) tris_out[3 * o + a] = (int32_t)vpos[tris[3 * t + a]];
  }
  if (t == nt - 1) {
    hdr->nT = (int64_t)(tpos[t] + tflag[t]);
    hdr->nV = (int64_t)(vpos[nv - 1] + vref[nv - 1]);
  }
}

}  // namespace
}  // namespace slgaudit

using namespace slgaudit;

static const char* kSizer = "slg_audit_ws_bytes";

extern "C" int64_t slg_audit_ws_bytes(int32_t stage, int64_t n_vertices, int64_t n_triangles) {
  if (stage < SLG_AUDIT_WS_AUDIT || stage > SLG_AUDIT_WS_SELECT || !counts_ok(n_vertices, n_triangles))
    return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_audit_ws_bytes: unknown stage, no vertices or triangles, 2^31 "
                                                         "vertices or more, or more than 2^30 triangle edges");
  return (int64_t)stage_bytes(stage, n_vertices, n_triangles);
}

extern "C" int32_t slg_audit_edges(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* ws, int64_t ws_bytes,
                                   uint8_t* vertex_class_out, uint8_t* triangle_class_out, void* stream) {
  const char* who = "slg_audit_edges";
  if (!triangles || !vertex_class_out || !triangle_class_out || !counts_ok(n_vertices, n_triangles))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL buffer or counts out of range", who);
  if (int rc = bind(who, kSizer, ws, ws_bytes, stage_bytes(SLG_AUDIT_WS_AUDIT, n_vertices, n_triangles))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const AuditWs w = audit_ws(b, n_vertices, n_triangles);
  AuditHdr* hdr = (AuditHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n3 = 3 * n_triangles;
  if (hipMemsetAsync(hdr, 0, SLG_MESH_HDR_BYTES, st) != hipSuccess ||
      hipMemsetAsync(w.vbits, 0, (size_t)n_vertices * 4, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  edge_keys_kernel<<<grid_of(n_triangles, 256), 256, 0, st>>>(hdr, triangles, n_triangles, n_vertices, w.k, w.val,
                                                              triangle_class_out, w.vbits);
  if (int rc = sort_pairs(who, w.k, w.s, w.val, w.sval, (size_t)n3, n_vertices, w.temp, w.tb, st)) return rc;
  edge_class_kernel<<<grid_of(n3, 256), 256, 0, st>>>(hdr, triangles, w.s, w.sval, n3, n_vertices, w.vbits, triangle_class_out);
  vertex_class_kernel<<<grid_of(n_vertices, 256), 256, 0, st>>>(hdr, w.vbits, n_vertices, vertex_class_out);
  return check_launch(who);
}

extern "C" int32_t slg_audit_components_count(int64_t n_triangles, int64_t n_vertices, void* ws, int64_t ws_bytes,
                                              const uint8_t* triangle_class, int32_t* labels_out, void* stream) {
  const char* who = "slg_audit_components_count";
  if (!triangle_class || !labels_out || !counts_ok(n_vertices, n_triangles))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL buffer or counts out of range", who);
  if (int rc = bind(who, kSizer, ws, ws_bytes, stage_bytes(SLG_AUDIT_WS_AUDIT, n_vertices, n_triangles))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const AuditWs w = audit_ws(b, n_vertices, n_triangles);
  AuditHdr* hdr = (AuditHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n3 = 3 * n_triangles;
  const int gt = grid_of(n_triangles, 256);
  iota_kernel<<<gt, 256, 0, st>>>(hdr, w.parent, n_triangles);
  tri_union_kernel<<<grid_of(n3, 256), 256, 0, st>>>(hdr, w.s, w.sval, n3, n_vertices, w.parent);
  tri_root_kernel<<<gt, 256, 0, st>>>(hdr, triangle_class, n_triangles, w.parent, w.root, w.tflag);
  if (int rc = scan_u8(who, w.tflag, w.tpos, (size_t)n_triangles, w.temp, w.tb, st)) return rc;
  tri_label_kernel<<<gt, 256, 0, st>>>(hdr, w.root, w.tflag, w.tpos, n_triangles, labels_out);
  return check_launch(who);
}

extern "C" int32_t slg_audit_components_emit(int64_t n_triangles, int64_t n_vertices, void* ws, int64_t ws_bytes,
                                             const int32_t* labels, int64_t n_components, int64_t* sizes_out, void* stream) {
  const char* who = "slg_audit_components_emit";
  if (!labels || !sizes_out || !counts_ok(n_vertices, n_triangles) || n_components <= 0 || n_components > n_triangles)
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL buffer, counts out of range or no component to emit", who);
  if (int rc = bind(who, kSizer, ws, ws_bytes, stage_bytes(SLG_AUDIT_WS_AUDIT, n_vertices, n_triangles))) return rc;
  AuditHdr* hdr = (AuditHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(sizes_out, 0, (size_t)n_components * 8, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  label_sizes_kernel<<<grid_of(n_triangles, 256), 256, 0, st>>>(hdr, labels, n_triangles, n_components, sizes_out);
  label_best_kernel<<<grid_of(n_components, 256), 256, 0, st>>>(hdr, sizes_out, n_components);
  label_largest_kernel<<<1, 1, 0, st>>>(hdr);
  return check_launch(who);
}

extern "C" int32_t slg_audit_fans(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* ws, int64_t ws_bytes,
                                  const uint8_t* triangle_class, uint8_t* vertex_class, void* stream) {
  const char* who = "slg_audit_fans";
  if (!triangles || !triangle_class || !vertex_class || !counts_ok(n_vertices, n_triangles))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL buffer or counts out of range", who);
  if (int rc = bind(who, kSizer, ws, ws_bytes, stage_bytes(SLG_AUDIT_WS_AUDIT, n_vertices, n_triangles))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const AuditWs w = audit_ws(b, n_vertices, n_triangles);
  AuditHdr* hdr = (AuditHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n3 = 3 * n_triangles;
  const int g3 = grid_of(n3, 256);
  if (hipMemsetAsync(w.vroot, 0xFF, (size_t)n_vertices * 4, st) != hipSuccess ||
      hipMemsetAsync(w.vbad, 0, (size_t)n_vertices, st) != hipSuccess ||
      hipMemsetAsync(&hdr->stats[SLG_AUDIT_STAT_NONMANIFOLD_VERTICES], 0, 8, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  iota_kernel<<<g3, 256, 0, st>>>(hdr, w.cparent, n3);
  corner_union_kernel<<<g3, 256, 0, st>>>(hdr, w.s, w.sval, n3, n_vertices, w.cparent);
  corner_root_kernel<<<g3, 256, 0, st>>>(hdr, triangles, triangle_class, n3, w.cparent, w.vroot, w.vbad, 0);
  corner_root_kernel<<<g3, 256, 0, st>>>(hdr, triangles, triangle_class, n3, w.cparent, w.vroot, w.vbad, 1);
  fan_class_kernel<<<grid_of(n_vertices, 256), 256, 0, st>>>(hdr, w.vbad, n_vertices, vertex_class);
  return check_launch(who);
}

extern "C" int32_t slg_audit_measure(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                     void* ws, int64_t ws_bytes, double* out, void* stream) {
  const char* who = "slg_audit_measure";
  if (!vertices || !triangles || !out || !counts_ok(n_vertices, n_triangles))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL buffer or counts out of range", who);
  if (int rc = bind(who, kSizer, ws, ws_bytes, stage_bytes(SLG_AUDIT_WS_MEASURE, n_vertices, n_triangles))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const MeasureWs w = measure_ws(b, n_triangles);
  AuditHdr* hdr = (AuditHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(n_triangles, kChunk);
  if (hipMemsetAsync(hdr, 0, SLG_MESH_HDR_BYTES, st) != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  measure_partial_kernel<<<nb, 256, 0, st>>>(hdr, vertices, n_vertices, triangles, n_triangles, w.part);
  measure_final_kernel<<<1, 256, 0, st>>>(hdr, w.part, nb, out);
  return check_launch(who);
}

extern "C" int32_t slg_audit_keep(const uint8_t* triangle_class, const int32_t* labels, int64_t n_triangles, const uint8_t* table,
                                  int64_t n_components, int32_t drop_bits, uint8_t* keep_out, void* stream) {
  const char* who = "slg_audit_keep";
  if (!keep_out || n_triangles <= 0 || n_triangles > (1ll << 30) / 3 || (drop_bits && !triangle_class) || drop_bits < 0 ||
      drop_bits > 255 || (table && (!labels || n_components <= 0)) || (!table && n_components != 0))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL buffer, counts out of range, or a table without labels", who);
  keep_kernel<<<grid_of(n_triangles, 256), 256, 0, (hipStream_t)stream>>>(triangle_class, labels, n_triangles, table,
                                                                          n_components, drop_bits, keep_out);
  return check_launch(who);
}

extern "C" int32_t slg_audit_select(const double* vertices, const double* densities, int64_t n_vertices, const int32_t* triangles,
                                    int64_t n_triangles, const uint8_t* keep, int32_t drop_unreferenced, void* ws,
                                    int64_t ws_bytes, double* vertices_out, double* densities_out, int32_t* triangles_out,
                                    void* stream) {
  const char* who = "slg_audit_select";
  if (!vertices || !triangles || !keep || !vertices_out || !triangles_out || (densities && !densities_out) ||
      !counts_ok(n_vertices, n_triangles))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL buffer or counts out of range", who);
  if (int rc = bind(who, kSizer, ws, ws_bytes, stage_bytes(SLG_AUDIT_WS_SELECT, n_vertices, n_triangles))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const SelectWs w = select_ws(b, n_vertices, n_triangles);
  AuditHdr* hdr = (AuditHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const int gt = grid_of(n_triangles, 256);
  if (hipMemsetAsync(hdr, 0, SLG_MESH_HDR_BYTES, st) != hipSuccess ||
      hipMemsetAsync(w.vref, drop_unreferenced ? 0 : 1, (size_t)n_vertices, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  select_flag_kernel<<<gt, 256, 0, st>>>(hdr, triangles, n_triangles, n_vertices, keep, w.tflag, w.vref);
  if (int rc = scan_u8(who, w.tflag, w.tpos, (size_t)n_triangles, w.temp, w.tb, st)) return rc;
  if (int rc = scan_u8(who, w.vref, w.vpos, (size_t)n_vertices, w.temp, w.tb, st)) return rc;
  select_vertices_kernel<<<grid_of(n_vertices, 256), 256, 0, st>>>(hdr, vertices, densities, n_vertices, w.vref, w.vpos,
                                                                   vertices_out, densities_out);
  select_triangles_kernel<<<gt, 256, 0, st>>>(hdr, triangles, n_triangles, n_vertices, w.tflag, w.tpos, w.vref, w.vpos,
                                              triangles_out);
  return check_launch(who);
}
