// cloud_cluster.hip -- device DBSCAN for gfx950 (ProcessingLogic.keep_largest_cluster,
// server/processing.py:391-427), on the radius filter's grid, count and block walk
// (cloud_grid.h, cloud_filter.hip).
//
// Open3D's ClusterDBSCAN in closed form (tests/cluster_ref.py): core = count >=
// min_points; a cluster's core set is a connected component of the core-core neighbour graph;
// components are ranked by their smallest original core index; a non-core point takes the lowest
// label among its core neighbours, or -1.
//
// The components come from a lock-free union-find over parent[n], indexed by original index.
// Invariant: parent[x] <= x, and an entry only ever decreases (every write is an atomic min), so
// the structure is acyclic, every find ends, and a component's root is its smallest index.  A
// failed link means another lane linked first; the loop goes on from what that lane wrote and
// never waits for anything another workgroup has yet to publish.  Inside the union kernel every
// access to parent is an agent-scope atomic: a plain load could be served from a stale line.
#include "cloud_grid.h"

using namespace slgcloud;

namespace {

// A point is core when its radius count (itself included) reaches min_points.
__device__ inline bool core_rule(int32_t count, int32_t min_points) { return count >= min_points; }

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

// Per sorted position q: scidx[q] = the point's original index when it is core, else kNone (the
// word the later walks stage beside the coordinates); parent[i] = i; sizes[i] = 0.
__global__ __launch_bounds__(256)
void dbscan_core_kernel(const Hdr* hdr, int64_t n, const uint32_t* __restrict__ sidx, const int32_t* __restrict__ cnt,
                        int32_t min_points, uint32_t* __restrict__ scidx, uint32_t* __restrict__ parent,
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
__global__ __launch_bounds__(256)
void dbscan_subcell_kernel(const Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ scidx,
                           const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ustart,
                           uint32_t* __restrict__ parent) {
  __shared__ uint32_t submin[8];
  if (hdr->status) return;
  const int nu = hdr->n_unique;
  const int t = threadIdx.x;
  const double half = 0.5 * hdr->cell;
  for (int u = blockIdx.x; u < nu; u += gridDim.x) {
    int64_t c[3];
    unpack_key(ukeys[u], c);
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

// The block walk, one workgroup per occupied cell: core queries against core candidates.  A pair
// is seen from both ends, so only the end with the larger index unites.  tpar holds the
// candidate's root as it stood when the tile was staged.  A candidate whose staged root is the
// query's current root, or the staged root of the candidate last united with (that set is the
// query's by now), is in the query's set already and costs no global access: a lane unites
// about once per distinct set among its neighbours, not once per neighbour.  Without that the
// kernel is bound by the latency of one lane's atomics while its wave waits (20 ms on a 1080p
// view at eps 5).  A batch of queries without a core point skips the walk.
__global__ __launch_bounds__(256)
void dbscan_union_kernel(const Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ scidx,
                         const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ustart, double r2,
                         uint32_t* parent) {
  __shared__ double tile[3 * kTile];
  __shared__ uint32_t tci[kTile], tpar[kTile];
  __shared__ uint32_t rng[9][2];
  cell_batches(hdr, ukeys, ustart, rng, [&](uint32_t qb, uint32_t qe) {
    const uint32_t q = qb + threadIdx.x;
    const uint32_t me = q < qe ? scidx[q] : kNone;
    const bool core = me != kNone;
    if (!__syncthreads_or(core ? 1 : 0)) return;
    const bool wave_active = __ballot(core) != 0;
    const uint32_t lim = core ? me : 0u;     // candidates below lim are this lane's to unite
    double px = 0.0, py = 0.0, pz = 0.0;
    if (core) { px = sxyz[3 * (size_t)q]; py = sxyz[3 * (size_t)q + 1]; pz = sxyz[3 * (size_t)q + 2]; }
    uint32_t hint = core ? uf_find(parent, me) : kNone;   // the root of this lane's set, as last seen
    uint32_t last = kNone;                   // the staged root of the last candidate united with
    block_walk<false>(
        rng, sxyz, tile, wave_active, px, py, pz,
        [&](int w, uint32_t j) {
          const uint32_t c = scidx[j];
          tci[w] = c;
          tpar[w] = c == kNone ? kNone : uf_find(parent, c);
        },
        [&](int j, double d2) {
          const uint32_t c = tci[j], cr = tpar[j];
          if (c < lim && radius_neighbour_rule(d2, r2) && cr != hint && cr != last) {
            hint = uf_unite(parent, hint, c);
            last = cr;
            par_min(parent, c, hint);        // a later staging of c then finds the root at once
            tpar[j] = hint;                  // and the other waves of this workgroup see it now
          }
        });
  });
}

// root[i] = the root of core point i (kNone for a non-core point); flags[i] = i is a root.  The
// exclusive scan of flags over the original order is then the label of every root.
__global__ __launch_bounds__(256)
void dbscan_flatten_kernel(const Hdr* hdr, int64_t n, const int32_t* __restrict__ cnt, int32_t min_points,
                           uint32_t* parent, uint32_t* __restrict__ root, uint32_t* __restrict__ flags) {
  if (hdr->status) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = core_rule(cnt[i], min_points) ? uf_find(parent, (uint32_t)i) : kNone;
  root[i] = r;
  flags[i] = r == (uint32_t)i ? 1u : 0u;
}

// sroot[q] = root of the point at sorted position q, for the border walk to stage; the cluster
// count from the end of the scan.
__global__ __launch_bounds__(256)
void dbscan_sroot_kernel(Hdr* hdr, int64_t n, const uint32_t* __restrict__ sidx, const uint32_t* __restrict__ root,
                         const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos,
                         uint32_t* __restrict__ sroot) {
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
__global__ __launch_bounds__(256)
void dbscan_border_kernel(const Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                          const uint32_t* __restrict__ sroot, const int32_t* __restrict__ cnt,
                          const uint32_t* __restrict__ pos, const uint64_t* __restrict__ ukeys,
                          const uint32_t* __restrict__ ustart, double r2, int32_t* __restrict__ labels) {
  __shared__ double tile[3 * kTile];
  __shared__ uint32_t tsr[kTile];
  __shared__ uint32_t rng[9][2];
  cell_batches(hdr, ukeys, ustart, rng, [&](uint32_t qb, uint32_t qe) {
    const uint32_t q = qb + threadIdx.x;
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
      block_walk<true>(rng, sxyz, tile, wave_need, px, py, pz, [&](int w, uint32_t j) { tsr[w] = sroot[j]; },
                       [&](int j, double d2) {
                         const uint32_t sr = tsr[j];
                         best = (need && radius_neighbour_rule(d2, r2) && sr < best) ? sr : best;
                       });
    }
    if (active) labels[o] = best == kNone ? -1 : (int32_t)pos[best];
  });
}

// Members per label and the noise count.  Integer atomics (order-independent), one per distinct
// label of a wave: neighbours in the input order mostly share a label.
__global__ __launch_bounds__(256)
void dbscan_sizes_kernel(Hdr* hdr, int64_t n, const int32_t* __restrict__ labels, int32_t* __restrict__ sizes) {
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

__global__ __launch_bounds__(256)
void dbscan_keep_kernel(const Hdr* hdr, int64_t n, const int32_t* __restrict__ labels, uint8_t* __restrict__ keep,
                        int32_t* __restrict__ info) {
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

}  // namespace

extern "C" int32_t slg_dbscan(const double* xyz, int64_t n, double eps, int32_t min_points, void* ws, int64_t ws_bytes,
                              int32_t* labels_out, uint8_t* largest_keep_out, int32_t* info_out, void* stream) {
  if (n <= 0 || !(eps > 0.0) || min_points < 0 || !xyz || !labels_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_dbscan: n <= 0, eps <= 0, min_points < 0 or a NULL buffer");
  Ws w;
  int rc = begin_call("slg_dbscan", n, ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const DbscanScratch s = dbscan_scratch(w, n);
  if ((rc = bbox(xyz, n, w, eps * (1.0 + 0x1p-20), 0, st))) return rc;     // the radius filter's cell
  if ((rc = build_grid(xyz, n, w, st))) return rc;
  const double r2 = eps * eps;
  const int cells = (int)(n < 8192 ? n : 8192);
  const int g = grid_of(n, 256);
  radius_count(w, n, r2, 0, s.keep, s.cnt, st);
  dbscan_core_kernel<<<g, 256, 0, st>>>(w.hdr, n, w.idx_s, s.cnt, min_points, s.scidx, s.parent, s.sizes);
  dbscan_subcell_kernel<<<cells, 256, 0, st>>>(w.hdr, w.sxyz, s.scidx, w.ukeys, w.ustart, s.parent);
  dbscan_union_kernel<<<cells, 256, 0, st>>>(w.hdr, w.sxyz, s.scidx, w.ukeys, w.ustart, r2, s.parent);
  dbscan_flatten_kernel<<<g, 256, 0, st>>>(w.hdr, n, s.cnt, min_points, s.parent, s.root, s.flags);
  if ((rc = scan_u32("slg_dbscan", w, s.flags, w.pos, n, st))) return rc;
  dbscan_sroot_kernel<<<g, 256, 0, st>>>(w.hdr, n, w.idx_s, s.root, s.flags, w.pos, s.sroot);
  dbscan_border_kernel<<<cells, 256, 0, st>>>(w.hdr, w.sxyz, w.idx_s, s.sroot, s.cnt, w.pos, w.ukeys, w.ustart, r2,
                                              labels_out);
  dbscan_sizes_kernel<<<g, 256, 0, st>>>(w.hdr, n, labels_out, s.sizes);
  dbscan_argmax_kernel<<<g, 256, 0, st>>>(w.hdr, s.sizes);
  dbscan_keep_kernel<<<g, 256, 0, st>>>(w.hdr, n, labels_out, largest_keep_out, info_out);
  return check_launch("slg_dbscan");
}
