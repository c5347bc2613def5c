// cloud_orient.hip -- tangent-plane normal orientation of a device cloud with normals
// (PointCloud.orient_normals_consistent_tangent_plane(k) of mesh_360 and reconstruct_stl,
// server/processing.py:675, :685, :823), with the two things it is built from as entry points of
// their own: the k-nearest-neighbour index lists and the Euclidean minimum spanning tree.  Rules:
// DESIGN.md §15 and tests/orient_ref.py; each is one __device__ function here.
//
// Three stages, all separate launches on the caller's stream with no host wait:
//   lists    the kNN grid's ring walk with a (d2, index) TopKI list per point in global memory
//            (64 queries to a block of kk x 64 entries, as cloud_feature.hip), the whole-cloud
//            kernel for the points still open after kMaxRing rings.
//   EMST     Boruvka.  Per round every point offers its nearest point of another component: the
//            first foreign entry of its list, or, when the whole list is its own component and the
//            list's last distance does not exceed the component's best so far, a ring walk that
//            skips its own component; a walk that reaches the ring limit goes to a far list (one
//            wave per point over the occupied cells the walk did not search), except that the
//            largest component then sits the round out; a point walled in by its own component
//            is marked and does not walk again.  The minimum is two passes of 64-bit atomicMin:
//            the distance's order key, then (a << 32 | b) among the edges attaining it.
//   tree     Boruvka over the explicit Riemannian graph (lists + EMST edges) with the weight
//            1 - |na . nb|, the same two passes; a list edge is offered to both end components.
// Components are a union-find of packed words (ancestor << 1 | parity to that ancestor): a root
// that chose an edge hooks onto the other root with the parity of the edge's sign, a mutual pair
// keeps the lower label, and a flatten kernel chases every vertex to its root.  Both edge orders
// are total, so both trees are unique and do not depend on which components act in a round.
// Every round of ceil(log2 n) + 1 is enqueued; once one component is left the rest return at once.
#include "cloud_grid.h"

using namespace slgcloud;

namespace {

constexpr int kOrientMaxK = 128;       // SLG_ORIENT_MAX_K
constexpr int kStatsLen = 128;         // SLG_ORIENT_STATS_LEN
constexpr int kMaxRounds = 32;         // ceil(log2 2^30) + 1 = 31 rounds at most
constexpr int kFarBlocks = 256;        // workgroups of the whole-cloud list kernel (each with scratch)
constexpr int kEmstFarBlocks = 16384;  // waves of emst_far_kernel (no scratch): far lists reach half a view
constexpr uint32_t kWalled = 0x80000000u;   // in cur: everything within the ring limit is the point's own component
constexpr uint64_t kNoEdge = ~0ull;    // no offer yet: above every order key of a finite double

// stats (SLG_ORIENT_STAT_*): rounds of the two Boruvkas, the lists' far count, totals, per round.
constexpr int kStatEmstRounds = 0, kStatTreeRounds = 1, kStatListFar = 2, kStatWalked = 3, kStatFar = 4,
              kStatSatOut = 5, kStatRoundWalked = 16, kStatRoundFar = 48, kStatRoundSatOut = 80;

struct OHdr {           // 1024 bytes behind the grid's workspace
  int32_t ncomp;        // components left
  int32_t active;       // this round runs (set by its reset kernel)
  int32_t sits_out;     // the largest component met the ring limit this round
  int32_t n_far;
  int32_t round;
  int32_t n_emst, n_tree;   // edges appended
  uint32_t root;
  unsigned long long best[2];   // (size << 32) | ~label by atomicMax, by round parity
  unsigned long long zmax;
  int32_t stats[kStatsLen];
};
static_assert(sizeof(OHdr) <= 1024, "header");

struct OrientWs {
  Ws grid;
  OHdr* oh;
  double* lst_d;        // [blocks of 64][kk][64]: d2 ascending by (d2, index); later the weights
  uint32_t* lst_i;
  double* far_d;        // [kFarBlocks][kk][64] scratch of the whole-cloud list kernel
  uint32_t* far_i;
  uint32_t *link, *hook, *scomp, *cur, *cand_j;
  int32_t* sizes;
  double* cand_d;
  unsigned long long *best_w, *best_e, *emst_e, *tree_e;
};

void orient_layout(Bump& b, int64_t n, int kk, OrientWs* w) {
  const size_t N = (size_t)n, entries = (size_t)grid_of(n, 64) * kk * 64;
  w->oh = (OHdr*)b.take<uint8_t>(1024);
  w->lst_d = b.take<double>(entries);
  w->lst_i = b.take<uint32_t>(entries);
  w->far_d = b.take<double>((size_t)kFarBlocks * kk * 64);
  w->far_i = b.take<uint32_t>((size_t)kFarBlocks * kk * 64);
  w->link = b.take<uint32_t>(N);
  w->hook = b.take<uint32_t>(N);
  w->scomp = b.take<uint32_t>(N);
  w->cur = b.take<uint32_t>(N);
  w->cand_j = b.take<uint32_t>(N);
  w->sizes = b.take<int32_t>(N);
  w->cand_d = b.take<double>(N);
  w->best_w = b.take<unsigned long long>(N);
  w->best_e = b.take<unsigned long long>(N);
  w->emst_e = b.take<unsigned long long>(N);
  w->tree_e = b.take<unsigned long long>(N);
}

// ---------------------------------------------------------------- the rules (one place each)
// A double's bits as an unsigned integer with the same order (finite values; -0 never occurs).
__device__ inline unsigned long long order_key_rule(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double order_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}
// The undirected edge (a, b), a < b, as one word: ascending words are ascending (a, b).
__device__ inline unsigned long long edge_rule(uint32_t i, uint32_t j) {
  return i < j ? ((unsigned long long)i << 32) | j : ((unsigned long long)j << 32) | i;
}
__device__ inline double normal_dot_rule(const double* __restrict__ nrm, uint32_t a, uint32_t b) {
  return (nrm[3 * (size_t)a] * nrm[3 * (size_t)b] + nrm[3 * (size_t)a + 1] * nrm[3 * (size_t)b + 1]) +
         nrm[3 * (size_t)a + 2] * nrm[3 * (size_t)b + 2];
}
// The Riemannian weight of an edge.
__device__ inline double tangent_weight_rule(const double* __restrict__ nrm, uint32_t a, uint32_t b) {
  return 1.0 - fabs(normal_dot_rule(nrm, a, b));
}
// The sign an edge carries: 1 (negate) when the input normals' dot product is negative; sgn(0) = +1.
__device__ inline uint32_t edge_parity_rule(const double* __restrict__ nrm, uint32_t a, uint32_t b) {
  return normal_dot_rule(nrm, a, b) < 0.0 ? 1u : 0u;
}

__device__ inline unsigned long long load_u64(const unsigned long long* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// ---------------------------------------------------------------- lists
// Plain kNN lists: cloud_grid.h's list kernels without the radius and without a count (kk <= n:
// every list is full).
__global__ __launch_bounds__(64)
void orient_lists_kernel(Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                         const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ustart, int64_t n, int kk,
                         double* lst_d, uint32_t* lst_i, uint32_t* __restrict__ far) {
  lists_body<false>(hdr, sxyz, sidx, ukeys, ustart, n, kk, 0.0, lst_d, lst_i, nullptr, far);
}

__global__ __launch_bounds__(64)
void orient_lists_far_kernel(const Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                             int64_t n, int kk, double* far_d, uint32_t* far_i, double* lst_d, uint32_t* lst_i,
                             const uint32_t* __restrict__ far) {
  lists_far_body<false>(hdr, sxyz, sidx, n, kk, 0.0, far_d, far_i, lst_d, lst_i, nullptr, far);
}

// The lists by input index, row-major [n][kk].
__global__ __launch_bounds__(64)
void orient_lists_out_kernel(const Hdr* hdr, const uint32_t* __restrict__ sidx, int64_t n, int kk,
                             const double* __restrict__ lst_d, const uint32_t* __restrict__ lst_i,
                             uint32_t* __restrict__ idx_out, double* __restrict__ d2_out) {
  if (hdr->status) return;
  const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (q >= n) return;
  const size_t base = (size_t)blockIdx.x * kk * 64 + threadIdx.x, row = (size_t)sidx[q] * kk;
  for (int e = 0; e < kk; ++e) {
    idx_out[row + e] = lst_i[base + (size_t)e * 64];
    d2_out[row + e] = lst_d[base + (size_t)e * 64];
  }
}

// ---------------------------------------------------------------- the union-find rounds
// Every vertex its own component.  Thread per sorted position q.
__global__ __launch_bounds__(256)
void boruvka_init_kernel(const Hdr* hdr, OHdr* oh, const uint32_t* __restrict__ sidx, int64_t n,
                         uint32_t* __restrict__ link, uint32_t* __restrict__ scomp, uint32_t* __restrict__ cur,
                         int32_t* __restrict__ sizes, int first) {
  if (hdr->status) return;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const uint32_t o = sidx[q];
  link[o] = o << 1;
  scomp[q] = o;
  cur[q] = 0u;
  sizes[o] = 1;
  if (q == 0) {
    oh->ncomp = (int32_t)n;
    oh->active = 0;
    oh->sits_out = 0;
    oh->n_far = 0;
    oh->round = 0;
    oh->best[0] = 0ull;
    oh->best[1] = 0ull;
    if (first) oh->stats[kStatListFar] = hdr->n_far;
  }
}

// Start of a round: nothing offered, every root its own parent; with kSizes the component sizes
// counted by the flatten before go into this round's (size, ~label) maximum.
template <bool kSizes>
__global__ __launch_bounds__(256)
void boruvka_reset_kernel(const Hdr* hdr, OHdr* oh, int64_t n, unsigned long long* __restrict__ best_w,
                          unsigned long long* __restrict__ best_e, uint32_t* __restrict__ hook,
                          uint32_t* __restrict__ cand_j, int32_t* __restrict__ sizes) {
  if (hdr->status) return;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool run = oh->ncomp > 1;                      // ncomp changes in the hook kernel only
  if (v == 0) {
    oh->active = run ? 1 : 0;
    oh->sits_out = 0;
    oh->n_far = 0;
  }
  if (!run || v >= n) return;
  best_w[v] = kNoEdge;
  best_e[v] = kNoEdge;
  hook[v] = (uint32_t)v << 1;
  cand_j[v] = kNone;
  if (kSizes) {
    const int32_t s = sizes[v];
    if (s > 0) atomicMax(&oh->best[oh->round & 1], ((unsigned long long)(uint32_t)s << 32) | (uint32_t)~(uint32_t)v);
    sizes[v] = 0;
  }
}

// The label of the component that contributes no edge this round, or kNone.
__device__ inline uint32_t sitting_out(const OHdr* oh) {
  return oh->sits_out ? ~(uint32_t)oh->best[oh->round & 1] : kNone;
}

// The smallest edge among those attaining the component's smallest key (pass 2 of the minimum).
__global__ __launch_bounds__(256)
void emst_pick_kernel(const Hdr* hdr, const OHdr* oh, int64_t n, const uint32_t* __restrict__ link,
                      const uint32_t* __restrict__ cand_j, const double* __restrict__ cand_d,
                      const unsigned long long* __restrict__ best_w, unsigned long long* __restrict__ best_e) {
  if (hdr->status || !oh->active) return;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const uint32_t j = cand_j[v];
  if (j == kNone) return;
  const uint32_t c = link[v] >> 1;
  if (order_key_rule(cand_d[v]) == best_w[c]) atomicMin(&best_e[c], edge_rule((uint32_t)v, j));
}

// Every root that chose an edge hooks onto the other end's root; a mutual pair keeps the lower
// label as root and appends the edge once.  link is only read here (hook is what is written), so
// the parities read are those of the round's start.  nrm == nullptr: no parity (the EMST).
__global__ __launch_bounds__(256)
void boruvka_hook_kernel(const Hdr* hdr, OHdr* oh, int64_t n, const double* __restrict__ nrm,
                         const uint32_t* __restrict__ link, const unsigned long long* __restrict__ best_e,
                         uint32_t* __restrict__ hook, unsigned long long* __restrict__ edges, int32_t* n_edges) {
  if (hdr->status || !oh->active) return;
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const uint32_t r = (uint32_t)v;
  if ((link[r] >> 1) != r) return;                     // not a root
  const unsigned long long e = best_e[r];
  const uint32_t out = sitting_out(oh);
  if (e == kNoEdge || r == out) return;
  const uint32_t a = (uint32_t)(e >> 32), b = (uint32_t)e;
  const uint32_t la = link[a], lb = link[b];
  const uint32_t other = (la >> 1) == r ? lb >> 1 : la >> 1;
  if (other == r) return;                              // cannot happen: an offered edge joins two components
  const bool mutual = other != out && best_e[other] == e;
  if (mutual && r < other) return;
  const uint32_t par = nrm ? (la & 1u) ^ (lb & 1u) ^ edge_parity_rule(nrm, a, b) : 0u;
  hook[r] = (other << 1) | par;
  atomicSub(&oh->ncomp, 1);
  const int32_t slot = atomicAdd(n_edges, 1);
  if (slot < n - 1) edges[slot] = e;                   // a forest: n - 1 edges at most
}

// Chases every vertex to its root through this round's hooks (at most one per component, so fewer
// than n steps), accumulating the parity.  Thread per sorted position q; with kSizes the new
// components are counted.
template <bool kSizes>
__global__ __launch_bounds__(256)
void boruvka_flatten_kernel(const Hdr* hdr, OHdr* oh, const uint32_t* __restrict__ sidx, int64_t n,
                            const uint32_t* __restrict__ hook, uint32_t* __restrict__ link,
                            uint32_t* __restrict__ scomp, int32_t* __restrict__ sizes, int stat) {
  if (hdr->status || !oh->active) return;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const uint32_t o = sidx[q];
  uint32_t r = link[o] >> 1, p = link[o] & 1u;
  for (int64_t it = 0; it < n; ++it) {
    const uint32_t h = hook[r];
    if ((h >> 1) == r) break;
    p ^= h & 1u;
    r = h >> 1;
  }
  link[o] = (r << 1) | p;
  scomp[q] = r;
  if (kSizes) atomicAdd(&sizes[r], 1);
  if (q == 0) {
    const int32_t rd = oh->round;
    if (kSizes && rd < kMaxRounds) oh->stats[kStatRoundSatOut + rd] = oh->sits_out;
    if (kSizes) oh->stats[kStatSatOut] += oh->sits_out;
    oh->best[(rd + 1) & 1] = 0ull;
    oh->round = rd + 1;
    oh->stats[stat] += 1;
  }
}

// ---------------------------------------------------------------- EMST: the offers of a round
// Pass 1a: the first foreign entry of a point's list is its nearest point of another component
// (smallest (d2, index), which for a fixed end is the smallest (d2, a, b)).  cur remembers the
// entries already seen to be of the point's own component: components only grow.
__global__ __launch_bounds__(64)
void emst_list_kernel(const Hdr* hdr, const OHdr* oh, const uint32_t* __restrict__ sidx, int64_t n, int kk,
                      const double* __restrict__ lst_d, const uint32_t* __restrict__ lst_i,
                      const uint32_t* __restrict__ link, uint32_t* __restrict__ cur, uint32_t* __restrict__ cand_j,
                      double* __restrict__ cand_d, unsigned long long* __restrict__ best_w) {
  if (hdr->status || !oh->active) return;
  const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (q >= n) return;
  const size_t base = (size_t)blockIdx.x * kk * 64 + threadIdx.x;
  const uint32_t o = sidx[q], c = link[o] >> 1;
  uint32_t e = cur[q], j = kNone;
  if (e & kWalled) return;                             // its list is its own component's for good
  for (; e < (uint32_t)kk; ++e) {
    j = lst_i[base + (size_t)e * 64];
    if (j != o && (link[j] >> 1) != c) break;
  }
  cur[q] = e;
  if (e >= (uint32_t)kk) return;
  const double d = lst_d[base + (size_t)e * 64];
  cand_d[o] = d;
  cand_j[o] = j;
  atomicMin(&best_w[c], order_key_rule(d));
}

// The nearest point of another component, as a list the ring walk can fill: kk = 1, curmax its
// distance.  Members of the query's own component (the query among them) never enter.
struct ForeignBest {
  int kk, cnt;
  double curmax;
  uint32_t idx;
  const uint32_t* scomp;
  uint32_t comp;
  __device__ inline void offer(double d, const uint32_t* __restrict__ sidx, size_t j) {
    if (cnt && d > curmax) return;
    if (scomp[j] == comp) return;
    const uint32_t i = sidx[j];
    if (!cnt || pair_before_rule(d, i, curmax, idx)) { curmax = d; idx = i; cnt = 1; }
  }
};

// Pass 1b: a point whose whole list is its own component.  Everything outside the list is at
// least as far as the list's last entry, so the point can only improve on the component's best so
// far (U, any earlier value of which is an upper bound too) when that entry is <= U.  The walk
// takes only d2 <= U (the radius walk with r2 = the next double after U) and ends when the block
// searched covers that ball or the best found.  At the ring limit the point goes to the far list;
// a point of the largest component makes that component sit the round out instead.  A walk that
// took every distance (U infinite) and met only its own component need never be repeated, since
// components only grow: the point is marked (kWalled) and goes straight to the far list from then on.
// (Without the mark both halves of a view in two pieces walked six rings again in every late round.)
__global__ __launch_bounds__(64)
void emst_walk_kernel(const Hdr* hdr, OHdr* oh, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                      const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ustart, int64_t n, int kk,
                      const double* __restrict__ lst_d, const uint32_t* __restrict__ link,
                      const uint32_t* __restrict__ scomp, uint32_t* __restrict__ cur, uint32_t* __restrict__ cand_j,
                      double* __restrict__ cand_d, unsigned long long* __restrict__ best_w, uint32_t* __restrict__ far) {
  if (hdr->status || !oh->active) return;
  const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (q >= n || kk >= n) return;                       // a list of the whole cloud leaves nothing to walk to
  const uint32_t o = sidx[q];
  if (cand_j[o] != kNone) return;
  const uint32_t c = link[o] >> 1;
  const unsigned long long bw = load_u64(&best_w[c]);
  const double U = bw == kNoEdge ? kInf : order_unkey(bw);
  if (lst_d[(size_t)blockIdx.x * kk * 64 + threadIdx.x + (size_t)(kk - 1) * 64] > U) return;
  const int32_t rd = oh->round;
  if (!(cur[q] & kWalled)) {
    if (rd < kMaxRounds) atomicAdd(&oh->stats[kStatRoundWalked + rd], 1);
    atomicAdd(&oh->stats[kStatWalked], 1);
    ForeignBest fb{1, 0, 0.0, kNone, scomp, c};
    const double r2 = U == kInf ? kInf : nextafter(U, kInf);
    const bool done = ring_walk<true>(hdr, sxyz, sidx, ukeys, ustart, q, r2, fb);
    if (fb.cnt) {                                      // a real edge out of the component, proven minimal or not
      cand_d[o] = fb.curmax;
      cand_j[o] = fb.idx;
      atomicMin(&best_w[c], order_key_rule(fb.curmax));
    }
    if (done) return;
    if (U == kInf && !fb.cnt) cur[q] |= kWalled;
  }
  if (c == ~(uint32_t)oh->best[rd & 1]) atomicExch(&oh->sits_out, 1);
  else far[atomicAdd(&oh->n_far, 1)] = (uint32_t)q;    // at most one entry per point: n entries
}

// Pass 1c: one wave per far-list point over the whole cloud, by occupied cell.  The cells within
// the ring limit were searched by the walk (its find, if any, is the point's candidate and seeds
// lane 0), so they are skipped; any other cell is scanned only when the distance to its box, less
// the header's slack per axis and a relative 1e-12 as in the ring walk's face bound, does not
// exceed the component's best so far or the lane's own.  (A scan of every point for every entry
// took 47 s on a 1.2 M-point view in two pieces; the cell table is 25 to 50 times shorter and the
// bound leaves few cells.)
__global__ __launch_bounds__(64)
void emst_far_kernel(const Hdr* hdr, OHdr* oh, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                     const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ustart,
                     const uint32_t* __restrict__ link, const uint32_t* __restrict__ scomp,
                     uint32_t* __restrict__ cand_j, double* __restrict__ cand_d, unsigned long long* __restrict__ best_w,
                     const uint32_t* __restrict__ far) {
  if (hdr->status || !oh->active) return;
  const int lane = threadIdx.x;
  const int nf = oh->n_far, nu = hdr->n_unique;
  const double h = hdr->cell, slack = hdr->slack;
  const double mn[3] = {hdr->mn[0], hdr->mn[1], hdr->mn[2]};
  for (int f = blockIdx.x; f < nf; f += gridDim.x) {
    const int64_t q = far[f];
    const uint32_t o = sidx[q], c = link[o] >> 1;
    unsigned long long bw = lane == 0 ? load_u64(&best_w[c]) : 0ull;
    bw = (unsigned long long)__shfl((long long)bw, 0, 64);
    const double U = bw == kNoEdge ? kInf : order_unkey(bw);
    const double p[3] = {sxyz[3 * q], sxyz[3 * q + 1], sxyz[3 * q + 2]};
    int64_t cq[3];
    for (int a = 0; a < 3; ++a) cq[a] = cell_coord(p[a], mn[a], h);      // the walk's centre cell
    double bd = kInf;
    uint32_t bi = kNone;
    if (lane == 0 && cand_j[o] != kNone) { bd = cand_d[o]; bi = cand_j[o]; }
    for (int u = lane; u < nu; u += 64) {
      int64_t cc[3];
      unpack_key(ukeys[u], cc);
      bool searched = true;
      double lb2 = 0.0;
      for (int a = 0; a < 3; ++a) {
        const int64_t dc = cc[a] - cq[a];
        searched = searched && dc >= -kMaxRing && dc <= kMaxRing;
        const double lo = mn[a] + (double)cc[a] * h, hi = mn[a] + (double)(cc[a] + 1) * h;
        const double g = fmax(fmax(fmax(lo - p[a], p[a] - hi), 0.0) - slack, 0.0);
        lb2 += g * g;
      }
      if (searched || lb2 * (1.0 - 1e-12) > (bi == kNone ? U : fmin(U, bd))) continue;
      for (uint32_t j = ustart[u]; j < ustart[u + 1]; ++j) {
        if (scomp[j] == c) continue;
        const double d = d2_rule(sxyz[3 * (size_t)j] - p[0], sxyz[3 * (size_t)j + 1] - p[1], sxyz[3 * (size_t)j + 2] - p[2]);
        if (d > U) continue;
        const uint32_t i = sidx[j];
        if (bi == kNone || pair_before_rule(d, i, bd, bi)) { bd = d; bi = i; }
      }
    }
    const double best = wave_min(bd);
    uint32_t wi = bd == best ? bi : kNone;
    for (int s = 32; s > 0; s >>= 1) {
      const uint32_t other = (uint32_t)__shfl_xor((int)wi, s, 64);
      wi = other < wi ? other : wi;
    }
    if (lane == 0) {
      const int32_t rd = oh->round;
      if (rd < kMaxRounds) atomicAdd(&oh->stats[kStatRoundFar + rd], 1);
      atomicAdd(&oh->stats[kStatFar], 1);
      if (wi != kNone) {
        cand_d[o] = best;
        cand_j[o] = wi;
        atomicMin(&best_w[c], order_key_rule(best));
      }
    }
  }
}

// ---------------------------------------------------------------- the Riemannian tree's offers
__global__ __launch_bounds__(256)
void orient_check_normals_kernel(Hdr* hdr, const double* __restrict__ nrm, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (!(isfinite(nrm[3 * i]) && isfinite(nrm[3 * i + 1]) && isfinite(nrm[3 * i + 2])))
    atomicOr(&hdr->status, SLG_FILTER_BAD_NONFINITE);
}

// The lists' distances are no longer needed: each entry's weight takes its place.
__global__ __launch_bounds__(64)
void tree_weights_kernel(const Hdr* hdr, const double* __restrict__ nrm, const uint32_t* __restrict__ sidx, int64_t n,
                         int kk, const uint32_t* __restrict__ lst_i, double* __restrict__ lst_w) {
  if (hdr->status) return;
  const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (q >= n) return;
  const size_t base = (size_t)blockIdx.x * kk * 64 + threadIdx.x;
  const uint32_t o = sidx[q];
  for (int e = 0; e < kk; ++e) lst_w[base + (size_t)e * 64] = tangent_weight_rule(nrm, o, lst_i[base + (size_t)e * 64]);
}

// One end's component takes the offer.  PASS 0: the smallest key (read first: the minimum only
// falls, so a key that is not below it cannot change it).  PASS 1: the smallest edge attaining it.
template <int PASS>
__device__ inline void tree_offer(unsigned long long* __restrict__ best_w, unsigned long long* __restrict__ best_e,
                                  uint32_t c, unsigned long long key, unsigned long long edge) {
  if (PASS == 0) {
    if (key < load_u64(&best_w[c])) atomicMin(&best_w[c], key);
  } else if (key == best_w[c]) {
    atomicMin(&best_e[c], edge);
  }
}

// A list edge (o, j) joins o's component to j's whether or not o is in j's list, so it is offered
// to both.  A point none of whose entries is foreign never has one again: cur = kk.
template <int PASS>
__global__ __launch_bounds__(64)
void tree_list_kernel(const Hdr* hdr, const OHdr* oh, const uint32_t* __restrict__ sidx, int64_t n, int kk,
                      const double* __restrict__ lst_w, const uint32_t* __restrict__ lst_i,
                      const uint32_t* __restrict__ link, uint32_t* __restrict__ cur,
                      unsigned long long* __restrict__ best_w, unsigned long long* __restrict__ best_e) {
  if (hdr->status || !oh->active) return;
  const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (q >= n) return;
  const size_t base = (size_t)blockIdx.x * kk * 64 + threadIdx.x;
  const uint32_t o = sidx[q], c = link[o] >> 1;
  bool any = false;
  for (uint32_t e = cur[q]; e < (uint32_t)kk; ++e) {
    const uint32_t j = lst_i[base + (size_t)e * 64];
    if (j == o) continue;
    const uint32_t cj = link[j] >> 1;
    if (cj == c) continue;
    any = true;
    const unsigned long long key = order_key_rule(lst_w[base + (size_t)e * 64]), edge = edge_rule(o, j);
    tree_offer<PASS>(best_w, best_e, c, key, edge);
    tree_offer<PASS>(best_w, best_e, cj, key, edge);
  }
  if (PASS == 0 && !any) cur[q] = (uint32_t)kk;
}

template <int PASS>
__global__ __launch_bounds__(256)
void tree_edges_kernel(const Hdr* hdr, const OHdr* oh, const double* __restrict__ nrm, int64_t n, int64_t m,
                       const unsigned long long* __restrict__ emst_e, const uint32_t* __restrict__ link,
                       unsigned long long* __restrict__ best_w, unsigned long long* __restrict__ best_e) {
  if (hdr->status || !oh->active) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= m) return;
  const unsigned long long edge = emst_e[t];
  const uint32_t a = (uint32_t)(edge >> 32), b = (uint32_t)edge;
  if (a >= n || b >= n) return;                        // only a complete EMST fills all n - 1 slots
  const uint32_t ca = link[a] >> 1, cb = link[b] >> 1;
  if (ca == cb) return;
  const unsigned long long key = order_key_rule(tangent_weight_rule(nrm, a, b));
  tree_offer<PASS>(best_w, best_e, ca, key, edge);
  tree_offer<PASS>(best_w, best_e, cb, key, edge);
}

// ---------------------------------------------------------------- root and signs
// PASS 0: the largest z.  PASS 1: the lowest index attaining it.
template <int PASS>
__global__ __launch_bounds__(256)
void orient_root_kernel(const Hdr* hdr, OHdr* oh, const double* __restrict__ xyz, int64_t n) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = order_key_rule(xyz[3 * i + 2]);
  if (PASS == 0) {
    if (key > load_u64(&oh->zmax)) atomicMax(&oh->zmax, key);
  } else if (key == oh->zmax) {
    atomicMin(&oh->root, (uint32_t)i);
  }
}

// The root's normal is negated iff its z is negative; every other sign is the product of the
// edge signs along the tree path, which is the two parities to the common ancestor.  out must
// not alias nrm.
__global__ __launch_bounds__(256)
void orient_apply_kernel(const Hdr* hdr, const OHdr* oh, const double* __restrict__ nrm, int64_t n,
                         const uint32_t* __restrict__ link, double* __restrict__ out, int64_t* __restrict__ root_out) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t root = oh->root;
  if (root >= n) return;
  const uint32_t s = (nrm[3 * (size_t)root + 2] < 0.0 ? 1u : 0u) ^ (link[root] & 1u) ^ (link[i] & 1u);
  for (int a = 0; a < 3; ++a) out[3 * i + a] = s ? -nrm[3 * i + a] : nrm[3 * i + a];
  if (i == 0 && root_out) *root_out = (int64_t)root;
}

__global__ __launch_bounds__(256)
void orient_edges_out_kernel(const Hdr* hdr, const unsigned long long* __restrict__ edges, int64_t m,
                             int64_t* __restrict__ out) {
  if (hdr->status) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= m) return;
  out[2 * t] = (int64_t)(edges[t] >> 32);
  out[2 * t + 1] = (int64_t)(edges[t] & 0xFFFFFFFFull);
}

__global__ __launch_bounds__(kStatsLen)
void orient_stats_out_kernel(const OHdr* oh, int32_t* __restrict__ out) { out[threadIdx.x] = oh->stats[threadIdx.x]; }

// ---------------------------------------------------------------- host side
int rounds_for(int64_t n) {                            // ceil(log2 n) + 1; none for a single point
  if (n < 2) return 0;
  int r = 0;
  while (((int64_t)1 << r) < n) ++r;
  return r + 1;
}

int refuse(const char* who, const double* xyz, int64_t n, int32_t k) {
  if (n <= 0 || k <= 0 || !xyz || ((uintptr_t)xyz & 7))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: n <= 0, k <= 0, or xyz NULL or not 8-byte aligned", who);
  if (n > kMaxPoints || k > kOrientMaxK)
    return slg_internal_fail(SLG_ERR_UNSUPPORTED, "%s: more than 2^30 points or k > %d", who, kOrientMaxK);
  return SLG_OK;
}

int orient_bind(const char* who, int64_t n, int kk, void* ws, int64_t ws_bytes, OrientWs* w) {
  return begin_ext_call(who, "slg_orient_ws_bytes", n, 0, ws, ws_bytes, &w->grid,
                        [&](Bump& b) { orient_layout(b, n, kk, w); });
}

// Stage 1: the grid and the sorted lists.
int lists_stage(const double* xyz, int64_t n, int k, int kk, const OrientWs& w, hipStream_t st) {
  if (hipMemsetAsync(w.oh, 0, 1024, st) != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "orient: memset failed");
  if (int rc = knn_grid(xyz, n, w.grid, k, st)) return rc;
  const Ws& g = w.grid;
  orient_lists_kernel<<<grid_of(n, 64), 64, 0, st>>>(g.hdr, g.sxyz, g.idx_s, g.ukeys, g.ustart, n, kk, w.lst_d, w.lst_i, g.far);
  orient_lists_far_kernel<<<(int)(n < kFarBlocks ? n : kFarBlocks), 64, 0, st>>>(g.hdr, g.sxyz, g.idx_s, n, kk, w.far_d,
                                                                                w.far_i, w.lst_d, w.lst_i, g.far);
  return check_launch("orient lists");
}

// Stage 2: the Euclidean minimum spanning tree into emst_e.
int emst_stage(int64_t n, int kk, const OrientWs& w, hipStream_t st) {
  const Ws& g = w.grid;
  const int g256 = grid_of(n, 256), g64 = grid_of(n, 64);
  boruvka_init_kernel<<<g256, 256, 0, st>>>(g.hdr, w.oh, g.idx_s, n, w.link, w.scomp, w.cur, w.sizes, 1);
  for (int r = 0; r < rounds_for(n); ++r) {
    boruvka_reset_kernel<true><<<g256, 256, 0, st>>>(g.hdr, w.oh, n, w.best_w, w.best_e, w.hook, w.cand_j, w.sizes);
    emst_list_kernel<<<g64, 64, 0, st>>>(g.hdr, w.oh, g.idx_s, n, kk, w.lst_d, w.lst_i, w.link, w.cur, w.cand_j, w.cand_d,
                                        w.best_w);
    emst_walk_kernel<<<g64, 64, 0, st>>>(g.hdr, w.oh, g.sxyz, g.idx_s, g.ukeys, g.ustart, n, kk, w.lst_d, w.link, w.scomp,
                                        w.cur, w.cand_j, w.cand_d, w.best_w, g.far);
    emst_far_kernel<<<(int)(n < kEmstFarBlocks ? n : kEmstFarBlocks), 64, 0, st>>>(
        g.hdr, w.oh, g.sxyz, g.idx_s, g.ukeys, g.ustart, w.link, w.scomp, w.cand_j, w.cand_d, w.best_w, g.far);
    emst_pick_kernel<<<g256, 256, 0, st>>>(g.hdr, w.oh, n, w.link, w.cand_j, w.cand_d, w.best_w, w.best_e);
    boruvka_hook_kernel<<<g256, 256, 0, st>>>(g.hdr, w.oh, n, nullptr, w.link, w.best_e, w.hook, w.emst_e, &w.oh->n_emst);
    boruvka_flatten_kernel<true><<<g256, 256, 0, st>>>(g.hdr, w.oh, g.idx_s, n, w.hook, w.link, w.scomp, w.sizes,
                                                      kStatEmstRounds);
  }
  return check_launch("orient EMST");
}

// Stage 3: the Riemannian tree into tree_e, the root, the signs.
int tree_stage(const double* xyz, const double* nrm, int64_t n, int kk, const OrientWs& w, double* normals_out,
               int64_t* root_out, hipStream_t st) {
  const Ws& g = w.grid;
  const int g256 = grid_of(n, 256), g64 = grid_of(n, 64), ge = grid_of(n > 1 ? n - 1 : 1, 256);
  tree_weights_kernel<<<g64, 64, 0, st>>>(g.hdr, nrm, g.idx_s, n, kk, w.lst_i, w.lst_d);
  boruvka_init_kernel<<<g256, 256, 0, st>>>(g.hdr, w.oh, g.idx_s, n, w.link, w.scomp, w.cur, w.sizes, 0);
  for (int r = 0; r < rounds_for(n); ++r) {
    boruvka_reset_kernel<false><<<g256, 256, 0, st>>>(g.hdr, w.oh, n, w.best_w, w.best_e, w.hook, w.cand_j, w.sizes);
    tree_list_kernel<0><<<g64, 64, 0, st>>>(g.hdr, w.oh, g.idx_s, n, kk, w.lst_d, w.lst_i, w.link, w.cur, w.best_w, w.best_e);
    tree_edges_kernel<0><<<ge, 256, 0, st>>>(g.hdr, w.oh, nrm, n, n - 1, w.emst_e, w.link, w.best_w, w.best_e);
    tree_list_kernel<1><<<g64, 64, 0, st>>>(g.hdr, w.oh, g.idx_s, n, kk, w.lst_d, w.lst_i, w.link, w.cur, w.best_w, w.best_e);
    tree_edges_kernel<1><<<ge, 256, 0, st>>>(g.hdr, w.oh, nrm, n, n - 1, w.emst_e, w.link, w.best_w, w.best_e);
    boruvka_hook_kernel<<<g256, 256, 0, st>>>(g.hdr, w.oh, n, nrm, w.link, w.best_e, w.hook, w.tree_e, &w.oh->n_tree);
    boruvka_flatten_kernel<false><<<g256, 256, 0, st>>>(g.hdr, w.oh, g.idx_s, n, w.hook, w.link, w.scomp, w.sizes,
                                                       kStatTreeRounds);
  }
  if (hipMemsetAsync(&w.oh->root, 0xFF, 4, st) != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "orient: memset failed");
  orient_root_kernel<0><<<g256, 256, 0, st>>>(g.hdr, w.oh, xyz, n);
  orient_root_kernel<1><<<g256, 256, 0, st>>>(g.hdr, w.oh, xyz, n);
  orient_apply_kernel<<<g256, 256, 0, st>>>(g.hdr, w.oh, nrm, n, w.link, normals_out, root_out);
  return check_launch("orient tree");
}

void edges_out(const OrientWs& w, const unsigned long long* edges, int64_t n, int64_t* out, hipStream_t st) {
  if (out && n > 1) orient_edges_out_kernel<<<grid_of(n - 1, 256), 256, 0, st>>>(w.grid.hdr, edges, n - 1, out);
}

}  // namespace

static_assert(kOrientMaxK == SLG_ORIENT_MAX_K && kStatsLen == SLG_ORIENT_STATS_LEN, "slgpu.h");
static_assert(kStatEmstRounds == SLG_ORIENT_STAT_EMST_ROUNDS && kStatTreeRounds == SLG_ORIENT_STAT_TREE_ROUNDS &&
              kStatListFar == SLG_ORIENT_STAT_LIST_FAR && kStatWalked == SLG_ORIENT_STAT_WALKED &&
              kStatFar == SLG_ORIENT_STAT_FAR && kStatSatOut == SLG_ORIENT_STAT_SAT_OUT &&
              kStatRoundWalked == SLG_ORIENT_STAT_ROUND_WALKED && kStatRoundFar == SLG_ORIENT_STAT_ROUND_FAR &&
              kStatRoundSatOut == SLG_ORIENT_STAT_ROUND_SAT_OUT, "slgpu.h");

extern "C" int64_t slg_orient_ws_bytes(int64_t n, int32_t k) {
  if (n <= 0 || k <= 0) return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_orient_ws_bytes: n <= 0 or k <= 0");
  if (n > kMaxPoints || k > kOrientMaxK)
    return -(int64_t)slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_orient_ws_bytes: more than 2^30 points or k > %d",
                                       kOrientMaxK);
  OrientWs w;
  return ext_ws_bytes(n, 0, [&](Bump& b) { orient_layout(b, n, (int)(n < k ? n : k), &w); });
}

extern "C" int32_t slg_knn_lists(const double* xyz, int64_t n, int32_t k, void* ws, int64_t ws_bytes, uint32_t* idx_out,
                                 double* d2_out, void* stream) {
  if (int rc = refuse("slg_knn_lists", xyz, n, k)) return rc;
  if (!idx_out || !d2_out) return slg_internal_fail(SLG_ERR_INVALID, "slg_knn_lists: a NULL buffer");
  const int kk = (int)(n < k ? n : k);
  OrientWs w;
  if (int rc = orient_bind("slg_knn_lists", n, kk, ws, ws_bytes, &w)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = lists_stage(xyz, n, k, kk, w, st)) return rc;
  orient_lists_out_kernel<<<grid_of(n, 64), 64, 0, st>>>(w.grid.hdr, w.grid.idx_s, n, kk, w.lst_d, w.lst_i, idx_out, d2_out);
  return check_launch("slg_knn_lists");
}

extern "C" int32_t slg_emst(const double* xyz, int64_t n, int32_t k, void* ws, int64_t ws_bytes, int64_t* edges_out_,
                            int32_t* stats_out, void* stream) {
  if (int rc = refuse("slg_emst", xyz, n, k)) return rc;
  if (!edges_out_) return slg_internal_fail(SLG_ERR_INVALID, "slg_emst: a NULL buffer");
  const int kk = (int)(n < k ? n : k);
  OrientWs w;
  if (int rc = orient_bind("slg_emst", n, kk, ws, ws_bytes, &w)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = lists_stage(xyz, n, k, kk, w, st)) return rc;
  if (int rc = emst_stage(n, kk, w, st)) return rc;
  edges_out(w, w.emst_e, n, edges_out_, st);
  if (stats_out) orient_stats_out_kernel<<<1, kStatsLen, 0, st>>>(w.oh, stats_out);
  return check_launch("slg_emst");
}

extern "C" int32_t slg_orient_tangent(const double* xyz, const double* normals, int64_t n, int32_t k, void* ws,
                                      int64_t ws_bytes, double* normals_out, int64_t* emst_out, int64_t* tree_out,
                                      int64_t* root_out, int32_t* stats_out, void* stream) {
  if (int rc = refuse("slg_orient_tangent", xyz, n, k)) return rc;
  if (!normals || !normals_out || normals == normals_out || ((uintptr_t)normals & 7) || ((uintptr_t)normals_out & 7))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_orient_tangent: normals or normals_out NULL, not 8-byte aligned, or the "
                                              "same buffer (the cloud needs normals)");
  const int kk = (int)(n < k ? n : k);
  OrientWs w;
  if (int rc = orient_bind("slg_orient_tangent", n, kk, ws, ws_bytes, &w)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = lists_stage(xyz, n, k, kk, w, st)) return rc;
  orient_check_normals_kernel<<<grid_of(n, 256), 256, 0, st>>>(w.grid.hdr, normals, n);
  if (int rc = emst_stage(n, kk, w, st)) return rc;
  if (int rc = tree_stage(xyz, normals, n, kk, w, normals_out, root_out, st)) return rc;
  edges_out(w, w.emst_e, n, emst_out, st);
  edges_out(w, w.tree_e, n, tree_out, st);
  if (stats_out) orient_stats_out_kernel<<<1, kStatsLen, 0, st>>>(w.oh, stats_out);
  return check_launch("slg_orient_tangent");
}
