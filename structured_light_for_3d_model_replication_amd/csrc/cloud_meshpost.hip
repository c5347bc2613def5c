// cloud_meshpost.hip -- post-processing of an indexed triangle mesh in HBM: the
// vertex adjacency and boundary CSRs, umbrella smoothing (Laplacian and Taubin) and the closing of
// small holes by ear clipping.  Our rules, MeshLab / VCGlib parity unpinned.  Every rule is
// restated in tests/meshpost_ref.py; fp64 under -ffp-contract=off and integer atomics only, so the
// same input gives the same bits.
//
// A directed pair (src, dst) is the 64-bit key src << 32 | dst; everything about connectivity is a
// radix sort of such keys, a flag pass, a scan and binary searches in the sorted keys
// (mesh_keys.h, shared with cloud_decimate.hip).  Every call takes a workspace whose first 256
// bytes are the mesh header (status at byte 0, nV at 8, nT at 16; here also int64 stats[8] at
// byte 128).
#include "mesh_keys.h"

namespace slgmeshpost {

constexpr uint32_t kNoEdge = 0xFFFFFFFFu;
constexpr int kMaxLoop = SLG_MESH_HOLES_MAX_SIZE;
constexpr int kStateClosable = 0, kStateLong = 1, kStateBlocked = 2, kStateNone = 3;

// ---------------------------------------------------------------- workspace
struct AdjWs { uint64_t *k6, *s6, *k3, *d3, *sb, *pos6, *posb; uint8_t *f6, *fb; void* temp; size_t tb; };
static AdjWs adj_ws(Bump& b, int64_t nt) {
  AdjWs w;
  const size_t n3 = 3 * (size_t)nt, n6 = 6 * (size_t)nt;
  w.k6 = b.take<uint64_t>(n6);          // the six directed pairs; afterwards the boundary pairs
  w.s6 = b.take<uint64_t>(n6);
  w.k3 = b.take<uint64_t>(n3);
  w.d3 = b.take<uint64_t>(n3);
  w.sb = b.take<uint64_t>(n6);
  w.pos6 = b.take<uint64_t>(n6);
  w.posb = b.take<uint64_t>(n6);
  w.f6 = b.take<uint8_t>(n6);
  w.fb = b.take<uint8_t>(n6);
  w.tb = sort_temp(n6);
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
struct HoleWs { uint64_t *k3, *d3, *B, *bpos, *tbase; uint32_t* next; int32_t *indeg, *outdeg; uint8_t *bf, *lcnt, *blocked;
                void* temp; size_t tb; };
static HoleWs hole_ws(Bump& b, int64_t nv, int64_t nt) {
  HoleWs w;
  const size_t n3 = 3 * (size_t)nt;
  w.k3 = b.take<uint64_t>(n3);
  w.d3 = b.take<uint64_t>(n3);
  w.B = b.take<uint64_t>(n3);
  w.bpos = b.take<uint64_t>(n3);
  w.tbase = b.take<uint64_t>(n3);
  w.next = b.take<uint32_t>(n3);
  w.indeg = b.take<int32_t>(nv);
  w.outdeg = b.take<int32_t>(nv);
  w.bf = b.take<uint8_t>(n3);
  w.lcnt = b.take<uint8_t>(n3);
  w.blocked = b.take<uint8_t>(nv);
  w.tb = sort_temp(n3);
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
static size_t stage_bytes(int stage, int64_t nv, int64_t nt) {
  Bump b(nullptr, SLG_MESH_HDR_BYTES);
  if (stage == SLG_MESH_WS_ADJACENCY) adj_ws(b, nt); else hole_ws(b, nv, nt);
  return b.off;
}
namespace {

// Both directions of every boundary edge (the sentinel otherwise), for the boundary CSR.
__global__ __launch_bounds__(256)
void boundary_pairs_kernel(const PostHdr* hdr, const uint64_t* __restrict__ d3, int64_t n, int64_t nv,
                           uint64_t* __restrict__ bk) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t none = edge_key((uint32_t)nv, 0u);
  const bool bnd = !hdr->status && boundary_rule(d3, n, nv, i);
  const uint64_t k = d3[i];
  bk[2 * i] = bnd ? k : none;
  bk[2 * i + 1] = bnd ? edge_key(key_dst(k), key_src(k)) : none;
}

__global__ void adj_totals_kernel(PostHdr* hdr, const uint8_t* f6, const uint64_t* pos6, const uint8_t* fb,
                                  const uint64_t* posb, int64_t n6) {
  hdr->nV = (int64_t)(pos6[n6 - 1] + f6[n6 - 1]);
  hdr->nT = (int64_t)(posb[n6 - 1] + fb[n6 - 1]);
}

// offsets[v], v = 0 .. V: the entries of sources below v.
__global__ __launch_bounds__(256)
void csr_offsets_kernel(const PostHdr* hdr, const uint64_t* __restrict__ s, const uint64_t* __restrict__ pos, int64_t n,
                        int64_t nv, int64_t total, int64_t* __restrict__ off) {
  if (hdr->status) return;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v > nv) return;
  const int64_t lb = lower_bound(s, n, edge_key((uint32_t)v, 0u));
  off[v] = lb < n ? (int64_t)pos[lb] : total;
}
__global__ __launch_bounds__(256)
void boundary_flag_kernel(const PostHdr* hdr, const int64_t* __restrict__ boff, int64_t nv, uint8_t* __restrict__ bnd) {
  if (hdr->status) return;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < nv) bnd[v] = boff[v + 1] > boff[v] ? 1 : 0;
}

// ---------------------------------------------------------------- smoothing
// One Jacobi pass, one lane per vertex: a lane walks its own row, so the sum keeps the row's
// ascending order ((q0 + q1) + q2 ...) whatever the degree; a wave's rows are neighbours in the
// vertex order, so its gathers of 24-byte rows fall into shared lines of L2.  mode 0:
// p' = (p + s) / (c + 1); mode 1: m = s / c, p' = p + (m - p) * factor; c == 0 copies p.
__global__ __launch_bounds__(256)
void smooth_pass_kernel(const double* __restrict__ in, double* __restrict__ out, int64_t nv,
                        const int64_t* __restrict__ off, const int32_t* __restrict__ nbr,
                        const uint8_t* __restrict__ bnd, const int64_t* __restrict__ boff,
                        const int32_t* __restrict__ bnbr, int mode, double factor) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const bool b = bnd[v] != 0;
  const int64_t lo = b ? boff[v] : off[v], hi = b ? boff[v + 1] : off[v + 1];
  const int32_t* __restrict__ row = b ? bnbr : nbr;
  const double p[3] = {in[3 * v], in[3 * v + 1], in[3 * v + 2]};
  if (hi <= lo) {
    for (int a = 0; a < 3; ++a) out[3 * v + a] = p[a];
    return;
  }
  const int64_t q0 = row[lo];
  double s[3] = {in[3 * q0], in[3 * q0 + 1], in[3 * q0 + 2]};
  for (int64_t k = lo + 1; k < hi; ++k) {
    const int64_t q = row[k];
    for (int a = 0; a < 3; ++a) s[a] = s[a] + in[3 * q + a];
  }
  const double c = (double)(hi - lo);
  for (int a = 0; a < 3; ++a) {
    if (mode == 0) {
      out[3 * v + a] = (p[a] + s[a]) / (c + 1.0);
    } else {
      const double m = s[a] / c;
      out[3 * v + a] = p[a] + (m - p[a]) * factor;
    }
  }
}

// ---------------------------------------------------------------- holes
// bf: boundary edges among the sorted winding pairs; a pair that occurs twice (a non-manifold or
// inconsistently wound edge) blocks both its vertices.
__global__ __launch_bounds__(256)
void hole_flag_kernel(const PostHdr* hdr, const uint64_t* __restrict__ d3, int64_t n, int64_t nv, uint8_t* __restrict__ bf,
                      uint8_t* __restrict__ blocked) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = d3[i];
  if (key_src(k) < (uint64_t)nv && i > 0 && d3[i - 1] == k) blocked[key_src(k)] = blocked[key_dst(k)] = 1;
  bf[i] = boundary_rule(d3, n, nv, i) ? 1 : 0;
}
// B: the boundary edges in ascending key order, and every vertex's in and out degree along them.
__global__ __launch_bounds__(256)
void hole_compact_kernel(PostHdr* hdr, const uint64_t* __restrict__ d3, int64_t n, const uint8_t* __restrict__ bf,
                         const uint64_t* __restrict__ bpos, uint64_t* __restrict__ B, int32_t* __restrict__ indeg,
                         int32_t* __restrict__ outdeg) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (bf[i]) {
    const uint64_t k = d3[i];
    B[bpos[i]] = k;
    atomicAdd(&outdeg[key_src(k)], 1);
    atomicAdd(&indeg[key_dst(k)], 1);
  }
  if (i == n - 1) hdr->stats[SLG_MESH_HOLES_STAT_EDGES] = (int64_t)(bpos[i] + bf[i]);
}
__global__ __launch_bounds__(256)
void hole_degree_kernel(const PostHdr* hdr, const int32_t* __restrict__ indeg, const int32_t* __restrict__ outdeg,
                        int64_t nv, uint8_t* __restrict__ blocked) {
  if (hdr->status) return;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const int32_t i = indeg[v], o = outdeg[v];
  if ((i | o) && (i != 1 || o != 1)) blocked[v] = 1;
}
// next(e) of e = (a, b): the first boundary edge whose source is b.
__global__ __launch_bounds__(256)
void hole_next_kernel(const PostHdr* hdr, const uint64_t* __restrict__ B, uint32_t* __restrict__ next) {
  if (hdr->status) return;
  const int64_t nb = hdr->stats[SLG_MESH_HOLES_STAT_EDGES];
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nb) return;
  const uint32_t b = key_dst(B[j]);
  const int64_t lb = lower_bound(B, nb, edge_key(b, 0u));
  next[j] = (lb < nb && key_src(B[lb]) == b) ? (uint32_t)lb : kNoEdge;
}
// Every boundary edge walks next for at most max_size steps: closable when it is back at itself
// after 3 <= L <= max_size steps without touching a blocked vertex; the loop's leader (its smallest
// index in B) gets the L - 2 triangles.
__global__ __launch_bounds__(256)
void hole_walk_kernel(PostHdr* hdr, const uint64_t* __restrict__ B, const uint32_t* __restrict__ next,
                      const uint8_t* __restrict__ blocked, int max_size, uint8_t* __restrict__ lcnt) {
  if (hdr->status) return;
  const int64_t nb = hdr->stats[SLG_MESH_HOLES_STAT_EDGES];
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int state = kStateNone, L = 0;
  bool leader = false;
  if (j < nb) {
    uint32_t e = (uint32_t)j, least = (uint32_t)j;
    state = kStateLong;
    for (int step = 1; step <= max_size; ++step) {
      const uint64_t k = B[e];
      if (blocked[key_src(k)] || blocked[key_dst(k)]) { state = kStateBlocked; break; }
      e = next[e];
      if (e == kNoEdge) { state = kStateBlocked; break; }
      if (e == (uint32_t)j) { L = step; state = step >= 3 ? kStateClosable : kStateBlocked; break; }
      least = e < least ? e : least;
    }
    leader = state == kStateClosable && least == (uint32_t)j;
    lcnt[j] = leader ? (uint8_t)(L - 2) : 0;
  }
  const int lane = threadIdx.x & 63;
  const int64_t counts[4] = {(int64_t)__popcll(__ballot(leader)), (int64_t)__popcll(__ballot(state == kStateClosable)),
                             (int64_t)__popcll(__ballot(state == kStateLong)),
                             (int64_t)__popcll(__ballot(state == kStateBlocked))};
  if (lane == 0)
    for (int c = 0; c < 4; ++c)
      if (counts[c]) atomicAdd((unsigned long long*)&hdr->stats[SLG_MESH_HOLES_STAT_LOOPS + c], (unsigned long long)counts[c]);
}
__global__ void hole_totals_kernel(PostHdr* hdr, const uint8_t* lcnt, const uint64_t* tbase, int64_t n) {
  if (hdr->status) return;
  hdr->nT = (int64_t)(tbase[n - 1] + lcnt[n - 1]);
}

// Ear clipping, one wavefront per loop and one lane per ring vertex, the ring in registers.  While
// m > 3: d_i = (dx dx + dy dy) + dz dz between r[i-1] and r[i+1] (NaN counts as +inf), the smallest
// wins, ties to the lowest i (a wave arg-min under the order (d, i)); triangle (r[i+1], r[i],
// r[i-1]); r[i] leaves.  Last (r[2], r[1], r[0]).  A wave takes the 64 edges of its slot and works
// through the leaders among them.
__global__ __launch_bounds__(256)
void hole_fill_kernel(const PostHdr* hdr, const double* __restrict__ vert, const uint64_t* __restrict__ B,
                      const uint32_t* __restrict__ next, const uint8_t* __restrict__ lcnt,
                      const uint64_t* __restrict__ tbase, int32_t* __restrict__ out, int64_t n_out) {
  if (hdr->status) return;
  const int64_t nb = hdr->stats[SLG_MESH_HOLES_STAT_EDGES];
  const int lane = threadIdx.x & 63;
  const int64_t j0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63);
  const int mine = j0 + lane < nb ? lcnt[j0 + lane] : 0;
  unsigned long long todo = __ballot(mine != 0);
  while (todo) {
    const int w = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int64_t j = j0 + w;
    int m = __shfl(mine, w) + 2;
    if (m > kMaxLoop) m = kMaxLoop;
    uint64_t o = tbase[j];
    int32_t r = 0;
    uint32_t e = (uint32_t)j;
    for (int i = 0; i < m; ++i) {            // the ring in walk order from the leader's source
      if (lane == i) r = (int32_t)key_src(B[e]);
      e = next[e];
      if (e >= (uint64_t)nb) e = (uint32_t)j;  // (a leader's walk has closed before, so this does not happen)
    }
    double px = 0.0, py = 0.0, pz = 0.0;
    if (lane < m) { px = vert[3 * (int64_t)r]; py = vert[3 * (int64_t)r + 1]; pz = vert[3 * (int64_t)r + 2]; }
    while (m > 3) {
      const bool in = lane < m;
      const int ip = !in ? lane : lane == 0 ? m - 1 : lane - 1, iq = !in ? lane : lane + 1 == m ? 0 : lane + 1;
      const double ax = __shfl(px, ip), ay = __shfl(py, ip), az = __shfl(pz, ip);
      const double bx = __shfl(px, iq), by = __shfl(py, iq), bz = __shfl(pz, iq);
      const int32_t ra = __shfl(r, ip), rb = __shfl(r, iq);
      const double dx = bx - ax, dy = by - ay, dz = bz - az;
      double bd = (dx * dx + dy * dy) + dz * dz;
      if (!in || !(bd == bd)) bd = slgcloud::kInf;
      int bi = lane;
      for (int s = 32; s; s >>= 1) {
        const double od = __shfl_xor(bd, s);
        const int oi = __shfl_xor(bi, s);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
      }
      if (lane == bi && o < (uint64_t)n_out) {
        out[3 * o] = rb;
        out[3 * o + 1] = r;
        out[3 * o + 2] = ra;
      }
      ++o;
      const int up = lane < 63 ? lane + 1 : lane;
      const int32_t nr = __shfl(r, up);
      const double nx = __shfl(px, up), ny = __shfl(py, up), nz = __shfl(pz, up);
      if (lane >= bi) { r = nr; px = nx; py = ny; pz = nz; }
      --m;
    }
    const int32_t r1 = __shfl(r, 1), r2 = __shfl(r, 2);
    if (lane == 0 && o < (uint64_t)n_out) {
      out[3 * o] = r2;
      out[3 * o + 1] = r1;
      out[3 * o + 2] = r;
    }
  }
}

}  // namespace
}  // namespace slgmeshpost

using namespace slgmeshpost;

extern "C" int64_t slg_mesh_post_ws_bytes(int32_t stage, int64_t n_vertices, int64_t n_triangles) {
  if ((stage != SLG_MESH_WS_ADJACENCY && stage != SLG_MESH_WS_HOLES) || !counts_ok(n_vertices, n_triangles))
    return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_post_ws_bytes: unknown stage, no vertices or triangles, 2^31 "
                                                         "vertices or more, or more than 2^30 winding pairs");
  return (int64_t)stage_bytes(stage, n_vertices, n_triangles);
}

extern "C" int32_t slg_mesh_adjacency_count(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* ws,
                                            int64_t ws_bytes, void* stream) {
  if (!triangles || !counts_ok(n_vertices, n_triangles))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_adjacency_count: a NULL buffer or counts out of range");
  if (int rc = bind("slg_mesh_adjacency_count", "slg_mesh_post_ws_bytes", ws, ws_bytes, stage_bytes(SLG_MESH_WS_ADJACENCY, n_vertices, n_triangles))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const AdjWs w = adj_ws(b, n_triangles);
  PostHdr* hdr = (PostHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n3 = 3 * n_triangles, n6 = 6 * n_triangles;
  const char* who = "slg_mesh_adjacency_count";
  if (hipMemsetAsync(hdr, 0, SLG_MESH_HDR_BYTES, st) != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  pair_keys_kernel<<<grid_of(n_triangles, 256), 256, 0, st>>>(hdr, triangles, n_triangles, n_vertices, w.k3, w.k6);
  if (int rc = sort_keys(who, w.k6, w.s6, (size_t)n6, n_vertices, w.temp, w.tb, st)) return rc;
  if (int rc = sort_keys(who, w.k3, w.d3, (size_t)n3, n_vertices, w.temp, w.tb, st)) return rc;
  unique_flag_kernel<<<grid_of(n6, 256), 256, 0, st>>>(w.s6, n6, n_vertices, w.f6);
  if (int rc = scan_u8(who, w.f6, w.pos6, (size_t)n6, w.temp, w.tb, st)) return rc;
  boundary_pairs_kernel<<<grid_of(n3, 256), 256, 0, st>>>(hdr, w.d3, n3, n_vertices, w.k6);
  if (int rc = sort_keys(who, w.k6, w.sb, (size_t)n6, n_vertices, w.temp, w.tb, st)) return rc;
  unique_flag_kernel<<<grid_of(n6, 256), 256, 0, st>>>(w.sb, n6, n_vertices, w.fb);
  if (int rc = scan_u8(who, w.fb, w.posb, (size_t)n6, w.temp, w.tb, st)) return rc;
  adj_totals_kernel<<<1, 1, 0, st>>>(hdr, w.f6, w.pos6, w.fb, w.posb, n6);
  return check_launch(who);
}

extern "C" int32_t slg_mesh_adjacency_emit(int64_t n_triangles, int64_t n_vertices, void* ws, int64_t ws_bytes,
                                           int64_t* offsets_out, int32_t* neighbours_out, int64_t n_neighbours,
                                           uint8_t* boundary_out, int64_t* boundary_offsets_out,
                                           int32_t* boundary_neighbours_out, int64_t n_boundary_neighbours, void* stream) {
  if (!counts_ok(n_vertices, n_triangles) || !offsets_out || !boundary_out || !boundary_offsets_out || n_neighbours < 0 ||
      n_boundary_neighbours < 0 || (n_neighbours && !neighbours_out) || (n_boundary_neighbours && !boundary_neighbours_out))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_adjacency_emit: a NULL buffer or counts out of range");
  if (int rc = bind("slg_mesh_adjacency_emit", "slg_mesh_post_ws_bytes", ws, ws_bytes, stage_bytes(SLG_MESH_WS_ADJACENCY, n_vertices, n_triangles))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const AdjWs w = adj_ws(b, n_triangles);
  const PostHdr* hdr = (const PostHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n6 = 6 * n_triangles;
  const int gv = grid_of(n_vertices + 1, 256);
  if (n_neighbours)
    csr_neighbours_kernel<<<grid_of(n6, 256), 256, 0, st>>>(hdr, w.s6, w.f6, w.pos6, n6, neighbours_out, n_neighbours);
  csr_offsets_kernel<<<gv, 256, 0, st>>>(hdr, w.s6, w.pos6, n6, n_vertices, n_neighbours, offsets_out);
  if (n_boundary_neighbours)
    csr_neighbours_kernel<<<grid_of(n6, 256), 256, 0, st>>>(hdr, w.sb, w.fb, w.posb, n6, boundary_neighbours_out,
                                                           n_boundary_neighbours);
  csr_offsets_kernel<<<gv, 256, 0, st>>>(hdr, w.sb, w.posb, n6, n_vertices, n_boundary_neighbours, boundary_offsets_out);
  boundary_flag_kernel<<<gv, 256, 0, st>>>(hdr, boundary_offsets_out, n_vertices, boundary_out);
  return check_launch("slg_mesh_adjacency_emit");
}

extern "C" int32_t slg_mesh_smooth_pass(const double* vertices, double* vertices_out, int64_t n_vertices,
                                        const int64_t* offsets, const int32_t* neighbours, const uint8_t* boundary,
                                        const int64_t* boundary_offsets, const int32_t* boundary_neighbours, int32_t mode,
                                        double factor, void* stream) {
  if (n_vertices <= 0 || n_vertices >= (1ll << 31) || !vertices || !vertices_out || vertices == vertices_out || !offsets ||
      !boundary || !boundary_offsets || (mode != SLG_MESH_SMOOTH_LAPLACIAN && mode != SLG_MESH_SMOOTH_STEP) || !isfinite(factor))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_smooth_pass: no vertices, a NULL buffer, out == in, an unknown mode or "
                                              "a factor that is not finite");
  smooth_pass_kernel<<<grid_of(n_vertices, 256), 256, 0, (hipStream_t)stream>>>(
      vertices, vertices_out, n_vertices, offsets, neighbours, boundary, boundary_offsets, boundary_neighbours, mode, factor);
  return check_launch("slg_mesh_smooth_pass");
}

extern "C" int32_t slg_mesh_holes_count(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, int32_t max_size,
                                        void* ws, int64_t ws_bytes, void* stream) {
  if (!triangles || !counts_ok(n_vertices, n_triangles) || max_size < 3 || max_size > kMaxLoop)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_holes_count: a NULL buffer, counts out of range or max_size outside 3..64");
  if (int rc = bind("slg_mesh_holes_count", "slg_mesh_post_ws_bytes", ws, ws_bytes, stage_bytes(SLG_MESH_WS_HOLES, n_vertices, n_triangles))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const HoleWs w = hole_ws(b, n_vertices, n_triangles);
  PostHdr* hdr = (PostHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n3 = 3 * n_triangles;
  const int g3 = grid_of(n3, 256);
  const char* who = "slg_mesh_holes_count";
  if (hipMemsetAsync(hdr, 0, SLG_MESH_HDR_BYTES, st) != hipSuccess || hipMemsetAsync(w.indeg, 0, (size_t)n_vertices * 4, st) != hipSuccess ||
      hipMemsetAsync(w.outdeg, 0, (size_t)n_vertices * 4, st) != hipSuccess ||
      hipMemsetAsync(w.blocked, 0, (size_t)n_vertices, st) != hipSuccess || hipMemsetAsync(w.bf, 0, (size_t)n3, st) != hipSuccess ||
      hipMemsetAsync(w.lcnt, 0, (size_t)n3, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  pair_keys_kernel<<<grid_of(n_triangles, 256), 256, 0, st>>>(hdr, triangles, n_triangles, n_vertices, w.k3, nullptr);
  if (int rc = sort_keys(who, w.k3, w.d3, (size_t)n3, n_vertices, w.temp, w.tb, st)) return rc;
  hole_flag_kernel<<<g3, 256, 0, st>>>(hdr, w.d3, n3, n_vertices, w.bf, w.blocked);
  if (int rc = scan_u8(who, w.bf, w.bpos, (size_t)n3, w.temp, w.tb, st)) return rc;
  hole_compact_kernel<<<g3, 256, 0, st>>>(hdr, w.d3, n3, w.bf, w.bpos, w.B, w.indeg, w.outdeg);
  hole_degree_kernel<<<grid_of(n_vertices, 256), 256, 0, st>>>(hdr, w.indeg, w.outdeg, n_vertices, w.blocked);
  hole_next_kernel<<<g3, 256, 0, st>>>(hdr, w.B, w.next);
  hole_walk_kernel<<<g3, 256, 0, st>>>(hdr, w.B, w.next, w.blocked, max_size, w.lcnt);
  if (int rc = scan_u8(who, w.lcnt, w.tbase, (size_t)n3, w.temp, w.tb, st)) return rc;
  hole_totals_kernel<<<1, 1, 0, st>>>(hdr, w.lcnt, w.tbase, n3);
  return check_launch(who);
}

extern "C" int32_t slg_mesh_holes_emit(const double* vertices, int64_t n_vertices, int64_t n_triangles, void* ws,
                                       int64_t ws_bytes, int32_t* triangles_out, int64_t n_new_triangles, void* stream) {
  if (!vertices || !triangles_out || !counts_ok(n_vertices, n_triangles) || n_new_triangles <= 0)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_holes_emit: a NULL buffer, counts out of range or nothing to emit");
  if (int rc = bind("slg_mesh_holes_emit", "slg_mesh_post_ws_bytes", ws, ws_bytes, stage_bytes(SLG_MESH_WS_HOLES, n_vertices, n_triangles))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const HoleWs w = hole_ws(b, n_vertices, n_triangles);
  hole_fill_kernel<<<grid_of(3 * n_triangles, 256), 256, 0, (hipStream_t)stream>>>(
      (const PostHdr*)ws, vertices, w.B, w.next, w.lcnt, w.tbase, triangles_out, n_new_triangles);
  return check_launch("slg_mesh_holes_emit");
}
