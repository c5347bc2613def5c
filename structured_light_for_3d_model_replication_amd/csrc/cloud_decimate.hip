// cloud_decimate.hip -- quadric edge-collapse decimation of an indexed triangle mesh in HBM, in
// rounds of independent collapses.  Our rule, MeshLab / VCGlib parity unpinned.
// The candidate edges have a total order (cost bits, key), a round collapses a set of edges whose
// closed neighbourhoods do not touch, and every expression is named, so the result is a pure
// function of the mesh and the target; tests/decimate_ref.py restates it and the device equals it
// bit for bit.  fp64 under -ffp-contract=off, no sqrt, integer atomics only (min on the per-vertex
// rank words, add on the counters), quadrics summed through the incidence CSR in ascending
// triangle index.
//
// One workspace per call, sized for the input: the 256-byte header, the state (positions, ten
// quadric components per vertex, remap, the alive triangles) and one round's scratch.  The host
// reads the header after each round and passes the alive triangle count into the next, which
// sizes that round's sorts and launches.
#include "mesh_keys.h"

namespace slgdecimate {

using namespace slgmeshpost;

struct DecHdr {         // PostHdr's layout; what it leaves unused carries the round's counts
  int32_t status;       // SLG_FILTER_BAD_INDEX
  int32_t R;            // unused
  int64_t nV, nT;       // alive vertices and triangles
  int64_t nC;           // candidate edges of the last round
  int64_t applied;      // collapses applied in the last round
  int64_t total;        // collapses applied since init
  double unused[10];
  int64_t stats[8];     // SLG_MESH_DECIMATE_STAT_* of the last round
};
static_assert(sizeof(DecHdr) <= SLG_MESH_HDR_BYTES, "header");
static_assert(offsetof(DecHdr, nV) == 8 && offsetof(DecHdr, nT) == 16 && offsetof(DecHdr, nC) == 24 &&
              offsetof(DecHdr, applied) == 32 && offsetof(DecHdr, total) == 40 && offsetof(DecHdr, stats) == 128, "mesh.py's offsets");

constexpr uint64_t kRefused = ~0ull;           // the cost word of a refused candidate: behind every cost
constexpr int kReasonNone = -1;                // else SLG_MESH_DECIMATE_STAT_BOUNDARY .. _NAN

struct DecWs {
  double *P, *Q, *pp;
  int32_t *remap, *tri, *tri2, *nbr;
  int64_t *off, *ioff;
  uint8_t *dead, *bnd, *claimed, *f6, *fc, *live, *sel, *selsorted, *keep;
  uint32_t *word, *idx, *idx_s, *rank;
  uint64_t *k6, *s6, *k3, *d3, *ik, *is, *pos6, *posc, *E, *cost, *cost_s, *spos, *kpos;
  void* temp;
  size_t tb;
};
static DecWs dec_ws(Bump& b, int64_t nv, int64_t nt) {
  DecWs w;
  const size_t V = (size_t)nv, n3 = 3 * (size_t)nt, n6 = 6 * (size_t)nt;
  w.P = b.take<double>(3 * V);
  w.Q = b.take<double>(10 * V);
  w.remap = b.take<int32_t>(V);
  w.dead = b.take<uint8_t>(V);
  w.bnd = b.take<uint8_t>(V);
  w.claimed = b.take<uint8_t>(V);
  w.word = b.take<uint32_t>(V);
  w.off = b.take<int64_t>(V + 1);
  w.ioff = b.take<int64_t>(V + 1);
  w.tri = b.take<int32_t>(n3);
  w.tri2 = b.take<int32_t>(n3);
  w.k6 = b.take<uint64_t>(n6);
  w.s6 = b.take<uint64_t>(n6);
  w.pos6 = b.take<uint64_t>(n6);
  w.posc = b.take<uint64_t>(n6 > V ? n6 : V);   // also the emit's scan over the vertices
  w.f6 = b.take<uint8_t>(n6);
  w.fc = b.take<uint8_t>(n6);
  w.nbr = b.take<int32_t>(n6);
  w.k3 = b.take<uint64_t>(n3);
  w.d3 = b.take<uint64_t>(n3);
  w.ik = b.take<uint64_t>(n3);
  w.is = b.take<uint64_t>(n3);
  w.E = b.take<uint64_t>(n3);
  w.cost = b.take<uint64_t>(n3);
  w.cost_s = b.take<uint64_t>(n3);
  w.spos = b.take<uint64_t>(n3);
  w.kpos = b.take<uint64_t>(nt);
  w.idx = b.take<uint32_t>(n3);
  w.idx_s = b.take<uint32_t>(n3);
  w.rank = b.take<uint32_t>(n3);
  w.pp = b.take<double>(3 * n3);
  w.live = b.take<uint8_t>(n3);
  w.sel = b.take<uint8_t>(n3);
  w.selsorted = b.take<uint8_t>(n3);
  w.keep = b.take<uint8_t>(nt);
  w.tb = sort_temp(n6 > V ? n6 : V);      // the (cost, index) pairs of 3 T candidates need 12 * 3 T + lookback
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
static size_t ws_bytes_of(int64_t nv, int64_t nt) {
  Bump b(nullptr, SLG_MESH_HDR_BYTES);
  dec_ws(b, nv, nt);
  return b.off;
}
static int sort_by_cost(const char* who, const DecWs& w, size_t n, hipStream_t st) {
  size_t need = 0;
  const hipError_t e = rocprim::radix_sort_pairs(nullptr, need, w.cost, w.cost_s, w.idx, w.idx_s, n, 0u, 64u, st);
  if (int rc = fits(who, e, need, w.tb)) return rc;
  size_t tb = w.tb;
  if (rocprim::radix_sort_pairs(w.temp, tb, w.cost, w.cost_s, w.idx, w.idx_s, n, 0u, 64u, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: radix sort failed", who);
  return SLG_OK;
}

namespace {

// ---------------------------------------------------------------- the named expressions
// n = e1 x e2 of corners A, B, C in winding order, not normalised.
__device__ inline void cross_rule(const double* A, const double* B, const double* C, double* n) {
  const double e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
  const double e2x = C[0] - A[0], e2y = C[1] - A[1], e2z = C[2] - A[2];
  n[0] = e1y * e2z - e1z * e2y;
  n[1] = e1z * e2x - e1x * e2z;
  n[2] = e1x * e2y - e1y * e2x;
}
// K = (a², ab, ac, ad, b², bc, bd, c², cd, d²) of the plane (n, d) through A; the weight is (2 area)².
__device__ inline void triangle_quadric_rule(const double* A, const double* B, const double* C, double* K) {
  double n[3];
  cross_rule(A, B, C, n);
  const double d = -((n[0] * A[0] + n[1] * A[1]) + n[2] * A[2]);
  K[0] = n[0] * n[0]; K[1] = n[0] * n[1]; K[2] = n[0] * n[2]; K[3] = n[0] * d;
  K[4] = n[1] * n[1]; K[5] = n[1] * n[2]; K[6] = n[1] * d;
  K[7] = n[2] * n[2]; K[8] = n[2] * d;
  K[9] = d * d;
}
// The quadric's value at (x, y, z); in the choice a non-finite cost counts as +inf, anything not
// above zero (a negative rounding residue, -0) as 0.0.
__device__ inline double cost_rule(const double* q, double x, double y, double z) {
  const double r0 = ((q[0] * x + q[1] * y) + q[2] * z) + q[3];
  const double r1 = ((q[1] * x + q[4] * y) + q[5] * z) + q[6];
  const double r2 = ((q[2] * x + q[5] * y) + q[7] * z) + q[8];
  const double r3 = ((q[3] * x + q[6] * y) + q[8] * z) + q[9];
  const double c = ((r0 * x + r1 * y) + r2 * z) + r3;
  if (!(fabs(c) < slgcloud::kInf)) return slgcloud::kInf;
  return c > 0.0 ? c : 0.0;
}
__device__ inline bool finite3(const double* p) {
  return fabs(p[0]) < slgcloud::kInf && fabs(p[1]) < slgcloud::kInf && fabs(p[2]) < slgcloud::kInf;
}

// ---------------------------------------------------------------- init
__global__ __launch_bounds__(256)
void init_vertices_kernel(DecHdr* hdr, int64_t nv, int64_t nt, int32_t* __restrict__ remap, uint8_t* __restrict__ dead) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v == 0) { hdr->nV = nv; hdr->nT = nt; }
  if (v >= nv) return;
  remap[v] = (int32_t)v;
  dead[v] = 0;
}
// The incidence keys vertex << 32 | triangle of the three corners; sorted, a vertex's row lists
// its triangles in ascending index.  A triangle with a bad index gives sentinels and sets the status.
__global__ __launch_bounds__(256)
void incidence_keys_kernel(DecHdr* hdr, const int32_t* __restrict__ tris, int64_t nt, int64_t nv, uint64_t* __restrict__ ik) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  const int32_t a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
  const bool bad = a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv;
  if (bad) atomicOr(&hdr->status, SLG_FILTER_BAD_INDEX);
  const uint64_t none = edge_key((uint32_t)nv, 0u);
  ik[3 * t] = bad ? none : edge_key((uint32_t)a, (uint32_t)t);
  ik[3 * t + 1] = bad ? none : edge_key((uint32_t)b, (uint32_t)t);
  ik[3 * t + 2] = bad ? none : edge_key((uint32_t)c, (uint32_t)t);
}
// first[v], v = 0 .. V: the first sorted key whose source is v or above.
__global__ __launch_bounds__(256)
void row_starts_kernel(const uint64_t* __restrict__ s, int64_t n, int64_t nv, int64_t* __restrict__ first) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v > nv) return;
  first[v] = lower_bound(s, n, edge_key((uint32_t)v, 0u));
}
// Q[v] = ((K0 + K1) + K2) + .. over the incident triangles in ascending index; zeros without any.
__global__ __launch_bounds__(256)
void quadric_sum_kernel(const DecHdr* hdr, const double* __restrict__ P, const int32_t* __restrict__ tris,
                        const uint64_t* __restrict__ is, const int64_t* __restrict__ ioff, int64_t nv, double* __restrict__ Q) {
  if (hdr->status) return;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  double acc[10];
  for (int c = 0; c < 10; ++c) acc[c] = 0.0;
  const int64_t lo = ioff[v], hi = ioff[v + 1];
  for (int64_t k = lo; k < hi; ++k) {
    const int64_t t = key_dst(is[k]);
    const int64_t a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    double K[10];
    triangle_quadric_rule(P + 3 * a, P + 3 * b, P + 3 * c, K);
    for (int j = 0; j < 10; ++j) acc[j] = k == lo ? K[j] : acc[j] + K[j];
  }
  for (int j = 0; j < 10; ++j) Q[10 * v + j] = acc[j];
}

// ---------------------------------------------------------------- a round: connectivity
__global__ void round_begin_kernel(DecHdr* hdr) {
  hdr->nC = 0;
  hdr->applied = 0;
  for (int c = 0; c < 8; ++c) hdr->stats[c] = 0;
}
// off[v] = the CSR entries of sources below v, from the scan over the sorted six-pair keys.
__global__ __launch_bounds__(256)
void neighbour_offsets_kernel(const uint64_t* __restrict__ s, const uint8_t* __restrict__ f, const uint64_t* __restrict__ pos,
                              int64_t n, int64_t nv, int64_t* __restrict__ off) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v > nv) return;
  const int64_t lb = lower_bound(s, n, edge_key((uint32_t)v, 0u));
  off[v] = lb < n ? (int64_t)pos[lb] : (int64_t)(pos[n - 1] + f[n - 1]);
}
__global__ __launch_bounds__(256)
void boundary_mark_kernel(const uint64_t* __restrict__ d3, int64_t n, int64_t nv, uint8_t* __restrict__ bnd) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !boundary_rule(d3, n, nv, i)) return;
  bnd[key_src(d3[i])] = 1;               // (every writer stores the same 1)
  bnd[key_dst(d3[i])] = 1;
}
// A candidate: a CSR entry (u, v) with u < v; compacted they are the undirected edges in ascending key.
__global__ __launch_bounds__(256)
void candidate_flag_kernel(const uint64_t* __restrict__ s, const uint8_t* __restrict__ f, int64_t n, uint8_t* __restrict__ fc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  fc[i] = (f[i] && key_src(s[i]) < key_dst(s[i])) ? 1 : 0;
}
__global__ __launch_bounds__(256)
void candidate_compact_kernel(DecHdr* hdr, const uint64_t* __restrict__ s, const uint8_t* __restrict__ fc,
                              const uint64_t* __restrict__ posc, int64_t n, uint64_t* __restrict__ E, int64_t n_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (fc[i] && posc[i] < (uint64_t)n_out) E[posc[i]] = s[i];
  if (i == n - 1) {
    const int64_t total = (int64_t)(posc[i] + fc[i]);
    hdr->nC = total < n_out ? total : n_out;
  }
}

// ---------------------------------------------------------------- a round: the candidate evaluation
// One lane per candidate edge; candidates in key order are neighbours in the mesh, so a wave's rows
// fall into shared lines of L2.  A candidate is refused at the first test it fails (boundary,
// nonmanifold, link, valence, nan, flip); the survivors get their placement and its cost's bits.
__global__ __launch_bounds__(256)
void evaluate_kernel(DecHdr* hdr, int64_t n, int64_t nv, const uint64_t* __restrict__ E, const double* __restrict__ P,
                     const double* __restrict__ Q, const int32_t* __restrict__ tris, const int64_t* __restrict__ off,
                     const int32_t* __restrict__ nbr, const uint8_t* __restrict__ bnd, const uint64_t* __restrict__ d3,
                     int64_t n3, const uint64_t* __restrict__ is, const int64_t* __restrict__ ioff,
                     uint64_t* __restrict__ cost, uint32_t* __restrict__ idx, double* __restrict__ pp) {
  if (hdr->status) return;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in = e < hdr->nC;
  int reason = kReasonNone;
  bool valid = false;
  double p[3] = {0.0, 0.0, 0.0}, best = 0.0;
  if (in) {
    const uint64_t key = E[e];
    const uint32_t u = key_src(key), v = key_dst(key);
    const bool bu = bnd[u] != 0, bv = bnd[v] != 0;
    if (bu && bv) reason = SLG_MESH_DECIMATE_STAT_BOUNDARY;
    if (reason == kReasonNone) {           // (u, v) and (v, u) exactly once each among the winding pairs
      for (int dir = 0; dir < 2; ++dir) {
        const uint64_t k = dir ? edge_key(v, u) : key;
        const int64_t lb = lower_bound(d3, n3, k);
        const bool once = lb < n3 && d3[lb] == k && !(lb + 1 < n3 && d3[lb + 1] == k);
        if (!once) reason = SLG_MESH_DECIMATE_STAT_NONMANIFOLD;
      }
    }
    if (reason == kReasonNone) {           // the rows are ascending: a merge finds the common neighbours
      int64_t i = off[u], j = off[v];
      const int64_t iu = off[u + 1], jv = off[v + 1];
      int common = 0;
      bool thin = false;
      while (i < iu && j < jv) {
        const int32_t a = nbr[i], b = nbr[j];
        if (a == b) {
          ++common;
          if (off[a + 1] - off[a] < 4) thin = true;
          ++i; ++j;
        } else if (a < b) ++i; else ++j;
      }
      if (common != 2) reason = SLG_MESH_DECIMATE_STAT_LINK;
      else if (thin) reason = SLG_MESH_DECIMATE_STAT_VALENCE;
    }
    if (reason == kReasonNone) {
      double q[10];
      for (int c = 0; c < 10; ++c) q[c] = Q[10 * (int64_t)u + c] + Q[10 * (int64_t)v + c];
      const double* pu = P + 3 * (int64_t)u;
      const double* pv = P + 3 * (int64_t)v;
      if (bu || bv) {
        const double* keep = bu ? pu : pv;
        for (int a = 0; a < 3; ++a) p[a] = keep[a];
        best = cost_rule(q, p[0], p[1], p[2]);
      } else {
        const double mid[3] = {(pu[0] + pv[0]) * 0.5, (pu[1] + pv[1]) * 0.5, (pu[2] + pv[2]) * 0.5};
        const double c00 = q[4] * q[7] - q[5] * q[5], c01 = q[2] * q[5] - q[1] * q[7], c02 = q[1] * q[5] - q[2] * q[4];
        const double c11 = q[0] * q[7] - q[2] * q[2], c12 = q[1] * q[2] - q[0] * q[5], c22 = q[0] * q[4] - q[1] * q[1];
        const double det = (q[0] * c00 + q[1] * c01) + q[2] * c02;
        const double r0 = -q[3], r1 = -q[6], r2 = -q[8];
        const double s[3] = {((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                             ((c02 * r0 + c12 * r1) + c22 * r2) / det};
        const double sx = s[0] - mid[0], sy = s[1] - mid[1], sz = s[2] - mid[2];
        const double ex = pv[0] - pu[0], ey = pv[1] - pu[1], ez = pv[2] - pu[2];
        const bool admitted = det != 0.0 && finite3(s) && slgcloud::d2_rule(sx, sy, sz) <= 4.0 * slgcloud::d2_rule(ex, ey, ez);
        const double* cand[4] = {s, pu, pv, mid};
        bool first = true;
        for (int c = admitted ? 0 : 1; c < 4; ++c) {
          const double cc = cost_rule(q, cand[c][0], cand[c][1], cand[c][2]);
          if (first || cc < best) {
            best = cc;
            for (int a = 0; a < 3; ++a) p[a] = cand[c][a];
            first = false;
          }
        }
      }
      if (!(best < slgcloud::kInf)) reason = SLG_MESH_DECIMATE_STAT_NAN;
    }
    if (reason == kReasonNone) {           // no triangle around the edge may turn over
      for (int side = 0; side < 2 && reason == kReasonNone; ++side) {
        const uint32_t w = side ? v : u, other = side ? u : v;
        for (int64_t k = ioff[w]; k < ioff[w + 1]; ++k) {
          const int64_t t = key_dst(is[k]);
          const int32_t c3[3] = {tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]};
          if ((uint32_t)c3[0] == other || (uint32_t)c3[1] == other || (uint32_t)c3[2] == other) continue;
          double A[3][3], Bm[3][3], n0[3], n1[3];
          for (int c = 0; c < 3; ++c)
            for (int a = 0; a < 3; ++a) {
              A[c][a] = P[3 * (int64_t)c3[c] + a];
              Bm[c][a] = (uint32_t)c3[c] == w ? p[a] : A[c][a];
            }
          cross_rule(A[0], A[1], A[2], n0);
          cross_rule(Bm[0], Bm[1], Bm[2], n1);
          if (!((n0[0] * n1[0] + n0[1] * n1[1]) + n0[2] * n1[2] > 0.0)) { reason = SLG_MESH_DECIMATE_STAT_FLIP; break; }
        }
      }
    }
    valid = reason == kReasonNone;
  }
  if (e < n) {
    cost[e] = valid ? (uint64_t)__double_as_longlong(best) : kRefused;
    idx[e] = (uint32_t)e;
    for (int a = 0; a < 3; ++a) pp[3 * e + a] = p[a];
  }
  const int lane = threadIdx.x & 63;
  for (int c = 0; c <= SLG_MESH_DECIMATE_STAT_VALID; ++c) {
    const bool mine = c == SLG_MESH_DECIMATE_STAT_VALID ? valid : reason == c;
    const unsigned long long cnt = (unsigned long long)__popcll(__ballot(mine));
    if (lane == 0 && cnt) atomicAdd((unsigned long long*)&hdr->stats[c], cnt);
  }
}

// ---------------------------------------------------------------- a round: rank and selection
__global__ __launch_bounds__(256)
void rank_kernel(const DecHdr* hdr, const uint32_t* __restrict__ idx_s, int64_t n, uint32_t* __restrict__ rank) {
  if (hdr->status) return;
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < n) rank[idx_s[r]] = (uint32_t)r;
}
// f(x) for every vertex x of the closed neighbourhood C(e) = N(u) u N(v) u {u, v}; the edge exists,
// so u is in N(v) and v in N(u) and the two rows are all of it.  Stops when f returns false.
template <class F>
__device__ inline bool over_closed_neighbourhood(uint64_t key, const int64_t* __restrict__ off, const int32_t* __restrict__ nbr, F f) {
  for (int side = 0; side < 2; ++side) {
    const uint32_t w = side ? key_dst(key) : key_src(key);
    for (int64_t k = off[w]; k < off[w + 1]; ++k)
      if (!f(nbr[k])) return false;
  }
  return true;
}
// A candidate is live iff no vertex of C(e) is claimed; every live one offers its rank to the
// words of C(e) by an integer min, which does not depend on the order of arrival.
__global__ __launch_bounds__(256)
void sweep_offer_kernel(const DecHdr* hdr, const uint64_t* __restrict__ E, const uint64_t* __restrict__ cost,
                        const uint32_t* __restrict__ rank, const int64_t* __restrict__ off, const int32_t* __restrict__ nbr,
                        const uint8_t* __restrict__ claimed, const uint8_t* __restrict__ sel, uint8_t* __restrict__ live,
                        uint32_t* __restrict__ word) {
  if (hdr->status) return;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= hdr->nC) return;
  bool is_live = cost[e] != kRefused && !sel[e];
  if (is_live) is_live = over_closed_neighbourhood(E[e], off, nbr, [&](int32_t x) { return claimed[x] == 0; });
  live[e] = is_live ? 1 : 0;
  if (!is_live) return;
  const uint32_t r = rank[e];
  // a word only falls, so a plain read that already shows a rank at or below r cannot be undone by
  // anything later: the atomic is left out then (most offers lose), and the minimum is the same
  over_closed_neighbourhood(E[e], off, nbr, [&](int32_t x) {
    if (word[x] > r) atomicMin(&word[x], r);
    return true;
  });
}
// A live candidate is selected iff it holds the minimum on every vertex of C(e); it claims C(e).
__global__ __launch_bounds__(256)
void sweep_pick_kernel(const DecHdr* hdr, const uint64_t* __restrict__ E, const uint32_t* __restrict__ rank,
                       const int64_t* __restrict__ off, const int32_t* __restrict__ nbr, const uint8_t* __restrict__ live,
                       const uint32_t* __restrict__ word, uint8_t* __restrict__ claimed, uint8_t* __restrict__ sel) {
  if (hdr->status) return;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= hdr->nC || !live[e]) return;
  const uint32_t r = rank[e];
  if (!over_closed_neighbourhood(E[e], off, nbr, [&](int32_t x) { return word[x] == r; })) return;
  sel[e] = 1;
  over_closed_neighbourhood(E[e], off, nbr, [&](int32_t x) { claimed[x] = 1; return true; });
}
__global__ __launch_bounds__(256)
void selected_in_rank_order_kernel(const DecHdr* hdr, const uint32_t* __restrict__ idx_s, const uint8_t* __restrict__ sel,
                                   int64_t n, uint8_t* __restrict__ selsorted) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const uint32_t e = idx_s[r];
  selsorted[r] = (!hdr->status && (int64_t)e < hdr->nC && sel[e]) ? 1 : 0;
}

// ---------------------------------------------------------------- a round: apply
// The first `need` selected candidates in rank order: P[u] = p, Q[u] = Q[u] + Q[v], remap[v] = u.
// Their closed neighbourhoods are disjoint, so no two lanes touch the same vertex.
__global__ __launch_bounds__(256)
void apply_kernel(DecHdr* hdr, const uint64_t* __restrict__ E, const uint32_t* __restrict__ idx_s,
                  const uint8_t* __restrict__ selsorted, const uint64_t* __restrict__ spos, int64_t n, int64_t need,
                  const double* __restrict__ pp, double* __restrict__ P, double* __restrict__ Q, int32_t* __restrict__ remap,
                  uint8_t* __restrict__ dead) {
  if (hdr->status) return;
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  if (r == n - 1) {
    const int64_t selected = (int64_t)(spos[r] + selsorted[r]), applied = selected < need ? selected : need;
    hdr->stats[SLG_MESH_DECIMATE_STAT_SELECTED] = selected;
    hdr->applied = applied;
    hdr->total += applied;
    hdr->nV -= applied;
  }
  if (!selsorted[r] || spos[r] >= (uint64_t)need) return;
  const int64_t e = idx_s[r];
  const int64_t u = key_src(E[e]), v = key_dst(E[e]);
  for (int a = 0; a < 3; ++a) P[3 * u + a] = pp[3 * e + a];
  for (int c = 0; c < 10; ++c) Q[10 * u + c] = Q[10 * u + c] + Q[10 * v + c];
  remap[v] = (int32_t)u;
  dead[v] = 1;
}
__global__ __launch_bounds__(256)
void remap_triangles_kernel(const DecHdr* hdr, int32_t* __restrict__ tris, int64_t nt, const int32_t* __restrict__ remap,
                            uint8_t* __restrict__ keep) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  if (hdr->status) { keep[t] = 0; return; }
  const int32_t a = remap[tris[3 * t]], b = remap[tris[3 * t + 1]], c = remap[tris[3 * t + 2]];
  tris[3 * t] = a; tris[3 * t + 1] = b; tris[3 * t + 2] = c;
  keep[t] = (a != b && b != c && c != a) ? 1 : 0;
}
__global__ __launch_bounds__(256)
void compact_triangles_kernel(DecHdr* hdr, const int32_t* __restrict__ tris, int64_t nt, const uint8_t* __restrict__ keep,
                              const uint64_t* __restrict__ kpos, int32_t* __restrict__ out) {
  if (hdr->status) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  const int64_t total = (int64_t)(kpos[nt - 1] + keep[nt - 1]);
  if (keep[t]) {
    const int64_t o = (int64_t)kpos[t];    // o <= t < nt
    for (int c = 0; c < 3; ++c) out[3 * o + c] = tris[3 * t + c];
  }
  if (t >= total)                          // the tail holds defined indices, whatever is read of it
    for (int c = 0; c < 3; ++c) out[3 * t + c] = 0;
  if (t == nt - 1) hdr->nT = total;
}

// ---------------------------------------------------------------- emit
__global__ __launch_bounds__(256)
void alive_flag_kernel(const uint8_t* __restrict__ dead, int64_t nv, uint8_t* __restrict__ f) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < nv) f[v] = dead[v] ? 0 : 1;
}
__global__ __launch_bounds__(256)
void emit_vertices_kernel(const DecHdr* hdr, const double* __restrict__ P, const double* __restrict__ dens,
                          const uint8_t* __restrict__ f, const uint64_t* __restrict__ vpos, int64_t nv,
                          double* __restrict__ vert_out, double* __restrict__ dens_out, int64_t n_out) {
  if (hdr->status) return;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv || !f[v] || vpos[v] >= (uint64_t)n_out) return;
  const int64_t o = (int64_t)vpos[v];
  for (int a = 0; a < 3; ++a) vert_out[3 * o + a] = P[3 * v + a];
  if (dens_out) dens_out[o] = dens[v];
}
__global__ __launch_bounds__(256)
void emit_triangles_kernel(const DecHdr* hdr, const int32_t* __restrict__ tris, const uint64_t* __restrict__ vpos,
                           int64_t n_out, int32_t* __restrict__ out) {
  if (hdr->status) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_out || t >= hdr->nT) return;
  for (int c = 0; c < 3; ++c) out[3 * t + c] = (int32_t)vpos[tris[3 * t + c]];
}

}  // namespace
}  // namespace slgdecimate

using namespace slgdecimate;

extern "C" int64_t slg_mesh_decimate_ws_bytes(int64_t n_vertices, int64_t n_triangles) {
  if (!counts_ok(n_vertices, n_triangles))
    return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_mesh_decimate_ws_bytes: no vertices or triangles, 2^31 vertices or "
                                                         "more, or more than 2^30 winding pairs");
  return (int64_t)ws_bytes_of(n_vertices, n_triangles);
}

extern "C" int32_t slg_mesh_decimate_init(const double* vertices, int64_t n_vertices, const int32_t* triangles,
                                          int64_t n_triangles, void* ws, int64_t ws_bytes, void* stream) {
  const char* who = "slg_mesh_decimate_init";
  if (!vertices || !triangles || !counts_ok(n_vertices, n_triangles))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL buffer or counts out of range", who);
  if (int rc = bind(who, "slg_mesh_decimate_ws_bytes", ws, ws_bytes, ws_bytes_of(n_vertices, n_triangles))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const DecWs w = dec_ws(b, n_vertices, n_triangles);
  DecHdr* hdr = (DecHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nv = n_vertices, nt = n_triangles, n3 = 3 * nt;
  if (hipMemsetAsync(hdr, 0, SLG_MESH_HDR_BYTES, st) != hipSuccess ||
      hipMemcpyAsync(w.P, vertices, (size_t)nv * 24, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(w.tri, triangles, (size_t)nt * 12, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: memset or copy failed", who);
  init_vertices_kernel<<<grid_of(nv, 256), 256, 0, st>>>(hdr, nv, nt, w.remap, w.dead);
  incidence_keys_kernel<<<grid_of(nt, 256), 256, 0, st>>>(hdr, w.tri, nt, nv, w.ik);
  if (int rc = sort_keys(who, w.ik, w.is, (size_t)n3, nv, w.temp, w.tb, st)) return rc;
  row_starts_kernel<<<grid_of(nv + 1, 256), 256, 0, st>>>(w.is, n3, nv, w.ioff);
  quadric_sum_kernel<<<grid_of(nv, 256), 256, 0, st>>>(hdr, w.P, w.tri, w.is, w.ioff, nv, w.Q);
  return check_launch(who);
}

extern "C" int32_t slg_mesh_decimate_round(void* ws, int64_t ws_bytes, int64_t n_vertices, int64_t n_triangles,
                                           int64_t n_alive, int64_t target, void* stream) {
  const char* who = "slg_mesh_decimate_round";
  if (!counts_ok(n_vertices, n_triangles) || n_alive <= 0 || n_alive > n_triangles || target < 0 || target >= n_alive)
    return slg_internal_fail(SLG_ERR_INVALID, "%s: counts out of range, or a target that is negative or already reached", who);
  if (int rc = bind(who, "slg_mesh_decimate_ws_bytes", ws, ws_bytes, ws_bytes_of(n_vertices, n_triangles))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const DecWs w = dec_ws(b, n_vertices, n_triangles);
  DecHdr* hdr = (DecHdr*)ws;
  PostHdr* phdr = (PostHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nv = n_vertices, ta = n_alive, n3 = 3 * ta, n6 = 6 * ta, need = (ta - target + 1) / 2;
  const int gv = grid_of(nv + 1, 256), g3 = grid_of(n3, 256), g6 = grid_of(n6, 256), gt = grid_of(ta, 256);
  round_begin_kernel<<<1, 1, 0, st>>>(hdr);
  // connectivity of the alive triangles: neighbour rows, boundary flags, winding pairs, incidence rows
  pair_keys_kernel<<<gt, 256, 0, st>>>(phdr, w.tri, ta, nv, w.k3, w.k6);
  if (int rc = sort_keys(who, w.k6, w.s6, (size_t)n6, nv, w.temp, w.tb, st)) return rc;
  if (int rc = sort_keys(who, w.k3, w.d3, (size_t)n3, nv, w.temp, w.tb, st)) return rc;
  unique_flag_kernel<<<g6, 256, 0, st>>>(w.s6, n6, nv, w.f6);
  if (int rc = scan_u8(who, w.f6, w.pos6, (size_t)n6, w.temp, w.tb, st)) return rc;
  csr_neighbours_kernel<<<g6, 256, 0, st>>>(phdr, w.s6, w.f6, w.pos6, n6, w.nbr, n6);
  neighbour_offsets_kernel<<<gv, 256, 0, st>>>(w.s6, w.f6, w.pos6, n6, nv, w.off);
  if (hipMemsetAsync(w.bnd, 0, (size_t)nv, st) != hipSuccess || hipMemsetAsync(w.claimed, 0, (size_t)nv, st) != hipSuccess ||
      hipMemsetAsync(w.sel, 0, (size_t)n3, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  boundary_mark_kernel<<<g3, 256, 0, st>>>(w.d3, n3, nv, w.bnd);
  incidence_keys_kernel<<<gt, 256, 0, st>>>(hdr, w.tri, ta, nv, w.ik);
  if (int rc = sort_keys(who, w.ik, w.is, (size_t)n3, nv, w.temp, w.tb, st)) return rc;
  row_starts_kernel<<<gv, 256, 0, st>>>(w.is, n3, nv, w.ioff);
  // the candidates in ascending key, their tests, placements and costs
  candidate_flag_kernel<<<g6, 256, 0, st>>>(w.s6, w.f6, n6, w.fc);
  if (int rc = scan_u8(who, w.fc, w.posc, (size_t)n6, w.temp, w.tb, st)) return rc;
  candidate_compact_kernel<<<g6, 256, 0, st>>>(hdr, w.s6, w.fc, w.posc, n6, w.E, n3);
  evaluate_kernel<<<g3, 256, 0, st>>>(hdr, n3, nv, w.E, w.P, w.Q, w.tri, w.off, w.nbr, w.bnd, w.d3, n3, w.is, w.ioff, w.cost,
                                      w.idx, w.pp);
  // rank by (cost bits, key): a stable sort of the key-ordered list by cost
  if (int rc = sort_by_cost(who, w, (size_t)n3, st)) return rc;
  rank_kernel<<<g3, 256, 0, st>>>(hdr, w.idx_s, n3, w.rank);
  for (int sweep = 0; sweep < SLG_MESH_DECIMATE_SWEEPS; ++sweep) {
    if (hipMemsetAsync(w.word, 0xFF, (size_t)nv * 4, st) != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
    sweep_offer_kernel<<<g3, 256, 0, st>>>(hdr, w.E, w.cost, w.rank, w.off, w.nbr, w.claimed, w.sel, w.live, w.word);
    sweep_pick_kernel<<<g3, 256, 0, st>>>(hdr, w.E, w.rank, w.off, w.nbr, w.live, w.word, w.claimed, w.sel);
  }
  // the budget's prefix of the selected in rank order, applied; the triangles rewritten and compacted
  selected_in_rank_order_kernel<<<g3, 256, 0, st>>>(hdr, w.idx_s, w.sel, n3, w.selsorted);
  if (int rc = scan_u8(who, w.selsorted, w.spos, (size_t)n3, w.temp, w.tb, st)) return rc;
  apply_kernel<<<g3, 256, 0, st>>>(hdr, w.E, w.idx_s, w.selsorted, w.spos, n3, need, w.pp, w.P, w.Q, w.remap, w.dead);
  remap_triangles_kernel<<<gt, 256, 0, st>>>(hdr, w.tri, ta, w.remap, w.keep);
  if (int rc = scan_u8(who, w.keep, w.kpos, (size_t)ta, w.temp, w.tb, st)) return rc;
  compact_triangles_kernel<<<gt, 256, 0, st>>>(hdr, w.tri, ta, w.keep, w.kpos, w.tri2);
  if (hipMemcpyAsync(w.tri, w.tri2, (size_t)ta * 12, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: copy failed", who);
  return check_launch(who);
}

extern "C" int32_t slg_mesh_decimate_emit(void* ws, int64_t ws_bytes, int64_t n_vertices, int64_t n_triangles,
                                          const double* densities, double* vertices_out, double* densities_out,
                                          int64_t n_vertices_out, int32_t* triangles_out, int64_t n_triangles_out, void* stream) {
  const char* who = "slg_mesh_decimate_emit";
  if (!counts_ok(n_vertices, n_triangles) || !vertices_out || n_vertices_out <= 0 || n_vertices_out > n_vertices ||
      n_triangles_out < 0 || n_triangles_out > n_triangles || (n_triangles_out && !triangles_out) || (!densities != !densities_out))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL buffer or counts out of range", who);
  if (int rc = bind(who, "slg_mesh_decimate_ws_bytes", ws, ws_bytes, ws_bytes_of(n_vertices, n_triangles))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const DecWs w = dec_ws(b, n_vertices, n_triangles);
  const DecHdr* hdr = (const DecHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nv = n_vertices;
  uint8_t* alive = w.claimed;               // idle between rounds
  uint64_t* vpos = w.posc;
  alive_flag_kernel<<<grid_of(nv, 256), 256, 0, st>>>(w.dead, nv, alive);
  if (int rc = scan_u8(who, alive, vpos, (size_t)nv, w.temp, w.tb, st)) return rc;
  emit_vertices_kernel<<<grid_of(nv, 256), 256, 0, st>>>(hdr, w.P, densities, alive, vpos, nv, vertices_out, densities_out,
                                                        n_vertices_out);
  if (n_triangles_out)
    emit_triangles_kernel<<<grid_of(n_triangles_out, 256), 256, 0, st>>>(hdr, w.tri, vpos, n_triangles_out, triangles_out);
  return check_launch(who);
}
