// cloud_surface.hip -- the surface mesh of an oriented cloud in HBM: the empty-ball triangles,
// radius by radius.  Our rule, Open3D parity unpinned: ball pivoting as Open3D runs
// it is a sequential front, what it converges to is not.  Its triangles are those on which a ball
// of radius r rests, on the normals' side, with no point inside; that set is a pure function of the
// cloud and every triple is tested on its own.  Where two such triangles would use one directed
// edge, the total order (bits of the squared circumradius, a, b, c) decides, in rounds of integer
// minima.  tests/surface_ref.py restates it and the device equals it bit for bit: fp64 under
// -ffp-contract=off, every expression named, integer atomics only.
//
// A pass (one radius) is five calls.  begin builds the sparse grid of cloud_grid.h with cell 2 r, so
// the 3x3x3 block of an anchor's cell holds everything within 2 r of it, and with that everything
// within r of a ball that rests on it.  count and emit run the same kernel, one wavefront per
// anchor: the anchor's open neighbours of higher index within 2 r go to a list in LDS, the lanes
// take the pairs of the list.  The host reads the count in between and sizes the pass workspace.
// emit ranks the candidates (stable radix sorts) and finds their directed-edge slots; round is one
// round of the selection, the host reads the live count after each; commit appends the accepted
// triangles, merges their edges into the sorted taken keys and recomputes the closed flags.
// Everything is separate launches on the caller's stream; no workgroup waits for another.
#include "mesh_keys.h"

#include "../../include/slgpu_surface.h"

namespace slgsurface {

using namespace slgmeshpost;
using slgcloud::Hdr;
using slgcloud::Ws;
using slgcloud::d2_rule;
using slgcloud::up256;

constexpr int kMaxPartners = SLG_SURFACE_MAX_NEIGHBOURS;   // the list in LDS: 32 bytes an entry
constexpr int64_t kMaxCandidates = (1ll << 30) / 3;        // 3 C directed edges in 32-bit slots

struct PassHdr {        // 256 bytes at the front of the pass workspace; mesh.py reads the first 32
  int32_t status;       // always 0: the cloud's conditions are in the grid workspace's status word
  int32_t pad;
  int64_t live;         // candidates still live after the last round
  int64_t accepted;     // candidates accepted since emit
  unsigned long long cursor;   // emit: the slots handed out
};
static_assert(sizeof(PassHdr) <= SLG_MESH_HDR_BYTES, "header");
static_assert(offsetof(PassHdr, live) == 8 && offsetof(PassHdr, accepted) == 16, "mesh.py's offsets");

struct GridExt { uint32_t* cnt; };            // behind the grid: the candidates of every anchor (sorted position)
static GridExt grid_ext(Bump& b, int64_t n) { return GridExt{b.take<uint32_t>((size_t)n)}; }

struct PassWs {
  uint64_t *rho, *key, *key2, *ek, *es, *apos, *mk;
  int32_t *tri, *tri_r;
  uint32_t *idx, *idx2, *slot, *word;
  uint8_t *mark, *live, *acc, *has, *open;
  void* temp;
  size_t tb;
};
static PassWs pass_ws(Bump& b, int64_t n, int64_t nc, int64_t nt) {
  PassWs w;
  const size_t C = (size_t)nc, C3 = 3 * C, M = (size_t)nt + C3;
  w.rho = b.take<uint64_t>(C);
  w.tri = b.take<int32_t>(C3);
  w.tri_r = b.take<int32_t>(C3);
  w.idx = b.take<uint32_t>(C);
  w.idx2 = b.take<uint32_t>(C);
  w.key = b.take<uint64_t>(C);
  w.key2 = b.take<uint64_t>(C);
  w.ek = b.take<uint64_t>(C3);
  w.es = b.take<uint64_t>(C3);
  w.slot = b.take<uint32_t>(C3);
  w.word = b.take<uint32_t>(C3);
  w.mark = b.take<uint8_t>(C3);
  w.live = b.take<uint8_t>(C);
  w.acc = b.take<uint8_t>(C);
  w.apos = b.take<uint64_t>(C);
  w.mk = b.take<uint64_t>(M);
  w.has = b.take<uint8_t>((size_t)n);
  w.open = b.take<uint8_t>((size_t)n);
  w.tb = sort_temp(M);
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
static size_t pass_bytes_of(int64_t n, int64_t nc, int64_t nt) {
  Bump b(nullptr, SLG_MESH_HDR_BYTES);
  pass_ws(b, n, nc, nt);
  return b.off;
}
static bool pass_counts_ok(int64_t n, int64_t nc, int64_t nt) {
  return n >= 3 && n <= slgcloud::kMaxPoints && nc > 0 && nc <= kMaxCandidates && nt >= 0 && nt <= (1ll << 40);
}
static bool radius_ok(double r) { return r > 0.0 && r < slgcloud::kInf; }

static int sort_pairs(const char* who, const PassWs& w, const uint64_t* kin, uint64_t* kout, const uint32_t* vin, uint32_t* vout,
                      size_t n, unsigned bits, hipStream_t st) {
  size_t need = 0;
  const hipError_t e = rocprim::radix_sort_pairs(nullptr, need, kin, kout, vin, vout, n, 0u, bits, st);
  if (int rc = fits(who, e, need, w.tb)) return rc;
  size_t tb = w.tb;
  if (rocprim::radix_sort_pairs(w.temp, tb, kin, kout, vin, vout, n, 0u, bits, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: radix sort failed", who);
  return SLG_OK;
}

namespace {

// ---------------------------------------------------------------- the named expressions
__device__ inline double dot_rule(const double* x, const double* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }
__device__ inline void cross_rule(const double* x, const double* y, double* o) {
  o[0] = x[1] * y[2] - x[2] * y[1];
  o[1] = x[2] * y[0] - x[0] * y[2];
  o[2] = x[0] * y[1] - x[1] * y[0];
}
// The triple a < b < c at pa, pb, pc with the normals na, nb, nc: false when it is flat (this also
// refuses duplicates and NaN), when its circumradius exceeds r, or when the normals do not lie on
// one side of its plane.  Else sign (+1: the triangle (a, b, c), -1: (a, c, b)), the squared
// circumradius and the centre o of the ball of radius r that rests on it on the normals' side.
__device__ inline bool triple_rule(const double* pa, const double* pb, const double* pc, const double* na, const double* nb,
                                   const double* nc, double r2, int* sign, double* rho2, double* o) {
  const double u[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]};
  const double v[3] = {pc[0] - pa[0], pc[1] - pa[1], pc[2] - pa[2]};
  double w[3], wu[3], vw[3];
  cross_rule(u, v, w);
  const double w2 = dot_rule(w, w);
  if (!(w2 > 0.0)) return false;
  const double uu = dot_rule(u, u), vv = dot_rule(v, v);
  cross_rule(w, u, wu);
  cross_rule(v, w, vw);
  const double den = 2.0 * w2;
  const double cc[3] = {(wu[0] * vv + vw[0] * uu) / den, (wu[1] * vv + vw[1] * uu) / den, (wu[2] * vv + vw[2] * uu) / den};
  *rho2 = dot_rule(cc, cc);
  const double h2 = r2 - *rho2;
  if (!(h2 >= 0.0)) return false;
  const double sa = dot_rule(w, na), sb = dot_rule(w, nb), sc = dot_rule(w, nc);
  const bool pos = sa > 0.0 && sb > 0.0 && sc > 0.0, neg = sa < 0.0 && sb < 0.0 && sc < 0.0;
  if (!pos && !neg) return false;
  double t = sqrt(h2 / w2);
  if (neg) t = -t;
  *sign = neg ? -1 : 1;
  for (int a = 0; a < 3; ++a) o[a] = (pa[a] + cc[a]) + t * w[a];
  return true;
}

// ---------------------------------------------------------------- the candidates
// One wavefront per anchor (sorted position q, input index a), grid-stride.  The list: the points of
// the anchor's block with a higher input index that are not closed and lie within 2 r.  More than
// kMaxPartners of them set SLG_FILTER_BAD_NEIGHBOURS: the list is never cut short.  The lanes take
// the pairs of the list; b is the lower input index of a pair.  The tests come in the order of the
// rule, the walk over the block for a point inside the ball last, and it stops at the first.
// kEmit false: cnt[q] = the anchor's candidates, *total += them.  kEmit true: lane 0 reserves
// cnt[q] slots at the cursor and the lanes fill them in the order they arrive; the ranking sorts
// by a total order, so that order does not reach the result.
template <bool kEmit>
__global__ __launch_bounds__(64)
void candidates_kernel(Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                       const uint64_t* __restrict__ keys_s, const uint64_t* __restrict__ ukeys,
                       const uint32_t* __restrict__ ustart, const double* __restrict__ nrm, const uint8_t* __restrict__ closed,
                       int64_t n, double r2, uint32_t* __restrict__ cnt, long long* __restrict__ total, PassHdr* ph,
                       uint64_t* __restrict__ rho, int32_t* __restrict__ tri, int64_t n_out) {
  __shared__ uint32_t rng[9][2];
  __shared__ double lp[3 * kMaxPartners];
  __shared__ uint32_t li[kMaxPartners], ls[kMaxPartners];
  __shared__ int m_sh, out_sh;
  __shared__ unsigned long long base_sh;
  if (hdr->status) return;
  const int t = threadIdx.x;
  const int nu = hdr->n_unique;
  const double r2x4 = 4.0 * r2, r2s = r2 * (1.0 - 0x1p-30);
  for (int64_t q = blockIdx.x; q < n; q += gridDim.x) {
    __syncthreads();                           // the previous anchor's list and ranges are no longer read
    const uint32_t a = sidx[q];
    if (closed[a]) {                           // (uniform over the wavefront)
      if (!kEmit && t == 0) cnt[q] = 0;
      continue;
    }
    if (t == 0) { m_sh = 0; out_sh = 0; }
    slgcloud::block_ranges(hdr, ukeys, ustart, nu, keys_s[q], rng);
    __syncthreads();
    const double pa[3] = {sxyz[3 * q], sxyz[3 * q + 1], sxyz[3 * q + 2]};
    for (int r = 0; r < 9; ++r)
      for (uint32_t j = rng[r][0] + t; j < rng[r][1]; j += 64) {
        const uint32_t b = sidx[j];
        if (b <= a || closed[b]) continue;
        const double x = sxyz[3 * (size_t)j], y = sxyz[3 * (size_t)j + 1], z = sxyz[3 * (size_t)j + 2];
        if (!(d2_rule(x - pa[0], y - pa[1], z - pa[2]) < r2x4)) continue;
        const int s = atomicAdd(&m_sh, 1);
        if (s < kMaxPartners) { lp[3 * s] = x; lp[3 * s + 1] = y; lp[3 * s + 2] = z; li[s] = b; ls[s] = j; }
      }
    __syncthreads();
    const int m = m_sh;
    if (m > kMaxPartners) {
      if (t == 0) {
        atomicOr(&hdr->status, SLG_FILTER_BAD_NEIGHBOURS);
        if (!kEmit) cnt[q] = 0;
      }
      continue;
    }
    uint32_t quota = 0;
    if (kEmit) {
      quota = cnt[q];
      if (quota == 0) continue;                // (uniform)
      if (t == 0) base_sh = atomicAdd(&ph->cursor, (unsigned long long)quota);
      __syncthreads();
    }
    const double* na = nrm + 3 * (size_t)a;
    const int np = m * (m - 1) / 2;
    uint32_t mine = 0;
    for (int p = t; p < np; p += 64) {
      // pair p = j (j - 1) / 2 + i with i < j
      int j = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
      while (j * (j - 1) / 2 > p) --j;
      while ((j + 1) * j / 2 <= p) ++j;
      int i = p - j * (j - 1) / 2;
      if (li[i] > li[j]) { const int x = i; i = j; j = x; }
      const uint32_t b = li[i], c = li[j];
      const double pb[3] = {lp[3 * i], lp[3 * i + 1], lp[3 * i + 2]}, pc[3] = {lp[3 * j], lp[3 * j + 1], lp[3 * j + 2]};
      if (!(d2_rule(pc[0] - pb[0], pc[1] - pb[1], pc[2] - pb[2]) < r2x4)) continue;
      int sign;
      double rho2, o[3];
      if (!triple_rule(pa, pb, pc, na, nrm + 3 * (size_t)b, nrm + 3 * (size_t)c, r2, &sign, &rho2, o)) continue;
      const uint32_t sb = ls[i], sc = ls[j];
      bool empty = true;
      for (int r = 0; r < 9 && empty; ++r)
        for (uint32_t k = rng[r][0]; k < rng[r][1]; ++k) {
          if (k == (uint32_t)q || k == sb || k == sc) continue;
          if (d2_rule(sxyz[3 * (size_t)k] - o[0], sxyz[3 * (size_t)k + 1] - o[1], sxyz[3 * (size_t)k + 2] - o[2]) < r2s) {
            empty = false;
            break;
          }
        }
      if (!empty) continue;
      if (kEmit) {
        const uint32_t s = (uint32_t)atomicAdd(&out_sh, 1);
        const int64_t at = (int64_t)base_sh + s;
        if (s < quota && at < n_out) {
          rho[at] = (uint64_t)__double_as_longlong(rho2);
          tri[3 * at] = (int32_t)a;
          tri[3 * at + 1] = (int32_t)(sign > 0 ? b : c);
          tri[3 * at + 2] = (int32_t)(sign > 0 ? c : b);
        }
      } else {
        ++mine;
      }
    }
    if (!kEmit) {
      for (int s = 32; s > 0; s >>= 1) mine += (uint32_t)__shfl_xor((int)mine, s, 64);
      if (t == 0) {
        cnt[q] = mine;
        if (mine) atomicAdd((unsigned long long*)total, (unsigned long long)mine);
      }
    }
  }
}

// ---------------------------------------------------------------- the ranking
__global__ __launch_bounds__(256)
void iota_bc_kernel(const int32_t* __restrict__ tri, int64_t nc, uint32_t* __restrict__ idx, uint64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nc) return;
  idx[i] = (uint32_t)i;
  const uint32_t x = (uint32_t)tri[3 * i + 1], y = (uint32_t)tri[3 * i + 2];
  key[i] = x < y ? edge_key(x, y) : edge_key(y, x);
}
__global__ __launch_bounds__(256)
void key_a_kernel(const int32_t* __restrict__ tri, const uint32_t* __restrict__ idx, int64_t nc, uint64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nc) key[i] = (uint64_t)(uint32_t)tri[3 * (size_t)idx[i]];
}
__global__ __launch_bounds__(256)
void key_rho_kernel(const uint64_t* __restrict__ rho, const uint32_t* __restrict__ idx, int64_t nc, uint64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nc) key[i] = rho[idx[i]];
}
// The candidates in rank order and their three directed edges in winding order.
__global__ __launch_bounds__(256)
void ranked_kernel(const int32_t* __restrict__ tri, const uint32_t* __restrict__ order, int64_t nc, int32_t* __restrict__ tri_r,
                   uint64_t* __restrict__ ek) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= nc) return;
  const size_t e = order[r];
  const uint32_t v0 = (uint32_t)tri[3 * e], v1 = (uint32_t)tri[3 * e + 1], v2 = (uint32_t)tri[3 * e + 2];
  tri_r[3 * r] = (int32_t)v0; tri_r[3 * r + 1] = (int32_t)v1; tri_r[3 * r + 2] = (int32_t)v2;
  ek[3 * r] = edge_key(v0, v1);
  ek[3 * r + 1] = edge_key(v1, v2);
  ek[3 * r + 2] = edge_key(v2, v0);
}
// An edge's slot is the first of its equal keys among the sorted ones; a candidate starts live iff
// none of its edges was taken by an earlier pass.
__global__ __launch_bounds__(256)
void slots_kernel(const uint64_t* __restrict__ ek, const uint64_t* __restrict__ es, int64_t nc, const uint64_t* __restrict__ taken,
                  int64_t nt, uint32_t* __restrict__ slot, uint8_t* __restrict__ live) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= nc) return;
  bool free_ = true;
  for (int e = 0; e < 3; ++e) {
    const uint64_t k = ek[3 * r + e];
    slot[3 * r + e] = (uint32_t)lower_bound(es, 3 * nc, k);
    const int64_t lb = lower_bound(taken, nt, k);
    if (lb < nt && taken[lb] == k) free_ = false;
  }
  live[r] = free_ ? 1 : 0;
}

// ---------------------------------------------------------------- a round
// Every live candidate offers its rank to its three slots by an integer min, which does not depend
// on the order of arrival.
__global__ __launch_bounds__(256)
void offer_kernel(const uint8_t* __restrict__ live, const uint32_t* __restrict__ slot, int64_t nc, uint32_t* __restrict__ word) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= nc || !live[r]) return;
  for (int e = 0; e < 3; ++e) {
    uint32_t* w = word + slot[3 * r + e];
    if (*w > (uint32_t)r) atomicMin(w, (uint32_t)r);   // a word only falls: a read at or below r settles it
  }
}
// A live candidate that holds the minimum on its three slots is accepted and marks them.
__global__ __launch_bounds__(256)
void pick_kernel(PassHdr* ph, uint8_t* __restrict__ live, const uint32_t* __restrict__ slot, const uint32_t* __restrict__ word,
                 int64_t nc, uint8_t* __restrict__ acc, uint8_t* __restrict__ mark) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool win = r < nc && live[r];
  if (win)
    for (int e = 0; e < 3; ++e) win = win && word[slot[3 * r + e]] == (uint32_t)r;
  if (win) {
    acc[r] = 1;
    live[r] = 0;
    for (int e = 0; e < 3; ++e) mark[slot[3 * r + e]] = 1;
  }
  const unsigned long long won = (unsigned long long)__popcll(__ballot(win));
  if ((threadIdx.x & 63) == 0 && won) atomicAdd((unsigned long long*)&ph->accepted, won);
}
// The live candidates on a marked slot leave; the rest are counted for the host.
__global__ __launch_bounds__(256)
void drop_kernel(PassHdr* ph, uint8_t* __restrict__ live, const uint32_t* __restrict__ slot, const uint8_t* __restrict__ mark,
                 int64_t nc) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool stays = r < nc && live[r];
  if (stays) {
    for (int e = 0; e < 3; ++e) stays = stays && !mark[slot[3 * r + e]];
    if (!stays) live[r] = 0;
  }
  const unsigned long long left = (unsigned long long)__popcll(__ballot(stays));
  if ((threadIdx.x & 63) == 0 && left) atomicAdd((unsigned long long*)&ph->live, left);
}

// ---------------------------------------------------------------- commit
__global__ __launch_bounds__(256)
void append_kernel(const int32_t* __restrict__ tri_r, const uint64_t* __restrict__ ek, const uint8_t* __restrict__ acc,
                   const uint64_t* __restrict__ apos, int64_t nc, int64_t n_acc, int32_t* __restrict__ out, uint64_t* __restrict__ mk) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= nc || !acc[r] || apos[r] >= (uint64_t)n_acc) return;
  const size_t o = (size_t)apos[r];
  for (int e = 0; e < 3; ++e) {
    out[3 * o + e] = tri_r[3 * r + e];
    mk[3 * o + e] = ek[3 * r + e];
  }
}
// has[v]: a taken edge at v; open[v]: one without its reverse (every writer stores the same 1).
__global__ __launch_bounds__(256)
void edge_ends_kernel(const uint64_t* __restrict__ taken, int64_t nt, int64_t n, uint8_t* __restrict__ has, uint8_t* __restrict__ open) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nt) return;
  const uint64_t k = taken[i];
  const uint32_t s = key_src(k), d = key_dst(k);
  if ((int64_t)s >= n || (int64_t)d >= n) return;
  has[s] = 1;
  has[d] = 1;
  if (boundary_rule(taken, nt, n, i)) { open[s] = 1; open[d] = 1; }
}
__global__ __launch_bounds__(256)
void closed_kernel(const uint8_t* __restrict__ has, const uint8_t* __restrict__ open, int64_t n, uint8_t* __restrict__ closed) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < n) closed[v] = (has[v] && !open[v]) ? 1 : 0;
}

}  // namespace

static int64_t grid_bytes_of(int64_t n) {
  return slgcloud::ext_ws_bytes(n, 0, [&](Bump& b) { grid_ext(b, n); });
}
static int bind_grid(const char* who, int64_t n, void* ws, int64_t ws_bytes, Ws* w, GridExt* x) {
  return slgcloud::begin_ext_call(who, "slg_surface_ws_bytes", n, 0, ws, ws_bytes, w, [&](Bump& b) { *x = grid_ext(b, n); });
}
static int bind_pass(const char* who, int64_t n, int64_t nc, int64_t nt, void* ws, int64_t ws_bytes, PassWs* w) {
  if (!pass_counts_ok(n, nc, nt)) return slg_internal_fail(SLG_ERR_INVALID, "%s: counts out of range", who);
  if (int rc = bind(who, "slg_surface_ws_bytes", ws, ws_bytes, pass_bytes_of(n, nc, nt))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  *w = pass_ws(b, n, nc, nt);
  return SLG_OK;
}
static int anchors_grid(int64_t n) { return (int)(n < (1 << 20) ? n : (1 << 20)); }

}  // namespace slgsurface

using namespace slgsurface;

extern "C" int64_t slg_surface_ws_bytes(int32_t stage, int64_t n, int64_t n_candidates, int64_t n_taken) {
  const char* who = "slg_surface_ws_bytes";
  if (stage == SLG_SURFACE_WS_GRID) {
    if (n < 3) return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "%s: fewer than 3 points", who);
    return grid_bytes_of(n);
  }
  if (stage != SLG_SURFACE_WS_PASS) return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "%s: unknown stage %d", who, stage);
  if (!pass_counts_ok(n, n_candidates, n_taken))
    return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "%s: fewer than 3 or more than 2^30 points, no candidates or more than "
                                                         "2^30 / 3, or a negative count of taken edges", who);
  return (int64_t)pass_bytes_of(n, n_candidates, n_taken);
}

extern "C" int32_t slg_surface_begin(const double* xyz, int64_t n, double radius, void* grid_ws, int64_t grid_ws_bytes,
                                     void* stream) {
  const char* who = "slg_surface_begin";
  if (!xyz || n < 3 || !radius_ok(radius))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL cloud, fewer than 3 points, or a radius that is not finite and > 0", who);
  Ws w;
  GridExt x;
  if (int rc = bind_grid(who, n, grid_ws, grid_ws_bytes, &w, &x)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = slgcloud::bbox(xyz, n, w, 2.0 * radius, 0, st)) return rc;
  return slgcloud::build_grid(xyz, n, w, st);
}

extern "C" int32_t slg_surface_count(const double* normals, const uint8_t* closed, int64_t n, double radius, void* grid_ws,
                                     int64_t grid_ws_bytes, int64_t* total_out, void* stream) {
  const char* who = "slg_surface_count";
  if (!normals || !closed || !total_out || n < 3 || !radius_ok(radius))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL buffer, fewer than 3 points, or a radius that is not finite and > 0", who);
  Ws w;
  GridExt x;
  if (int rc = bind_grid(who, n, grid_ws, grid_ws_bytes, &w, &x)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(total_out, 0, 8, st) != hipSuccess || hipMemsetAsync(x.cnt, 0, (size_t)n * 4, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  candidates_kernel<false><<<anchors_grid(n), 64, 0, st>>>(w.hdr, w.sxyz, w.idx_s, w.keys_s, w.ukeys, w.ustart, normals, closed, n,
                                                          radius * radius, x.cnt, (long long*)total_out, nullptr, nullptr,
                                                          nullptr, 0);
  return check_launch(who);
}

extern "C" int32_t slg_surface_emit(const double* normals, const uint8_t* closed, int64_t n, double radius, void* grid_ws,
                                    int64_t grid_ws_bytes, const uint64_t* taken, int64_t n_taken, void* pass_ws_,
                                    int64_t pass_ws_bytes, int64_t n_candidates, void* stream) {
  const char* who = "slg_surface_emit";
  if (!normals || !closed || !taken || n < 3 || !radius_ok(radius))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL buffer, fewer than 3 points, or a radius that is not finite and > 0", who);
  Ws w;
  GridExt x;
  PassWs p;
  if (int rc = bind_pass(who, n, n_candidates, n_taken, pass_ws_, pass_ws_bytes, &p)) return rc;
  if (int rc = bind_grid(who, n, grid_ws, grid_ws_bytes, &w, &x)) return rc;
  PassHdr* ph = (PassHdr*)pass_ws_;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nc = n_candidates, c3 = 3 * nc;
  const int gc = grid_of(nc, 256);
  // a cloud refused since the count leaves slots unfilled: every word of them is defined first
  if (hipMemsetAsync(ph, 0, SLG_MESH_HDR_BYTES, st) != hipSuccess || hipMemsetAsync(p.tri, 0, (size_t)c3 * 4, st) != hipSuccess ||
      hipMemsetAsync(p.rho, 0xFF, (size_t)nc * 8, st) != hipSuccess || hipMemsetAsync(p.acc, 0, (size_t)nc, st) != hipSuccess ||
      hipMemsetAsync(p.mark, 0, (size_t)c3, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  candidates_kernel<true><<<anchors_grid(n), 64, 0, st>>>(w.hdr, w.sxyz, w.idx_s, w.keys_s, w.ukeys, w.ustart, normals, closed, n,
                                                         radius * radius, x.cnt, nullptr, ph, p.rho, p.tri, nc);
  // rank = the position after stable sorts on (b, c), a and the bits of rho^2
  unsigned abits = 1;
  while (abits < 32 && ((uint64_t)n >> abits)) ++abits;
  iota_bc_kernel<<<gc, 256, 0, st>>>(p.tri, nc, p.idx, p.key);
  if (int rc = sort_pairs(who, p, p.key, p.key2, p.idx, p.idx2, (size_t)nc, 32 + abits, st)) return rc;
  key_a_kernel<<<gc, 256, 0, st>>>(p.tri, p.idx2, nc, p.key);
  if (int rc = sort_pairs(who, p, p.key, p.key2, p.idx2, p.idx, (size_t)nc, abits, st)) return rc;
  key_rho_kernel<<<gc, 256, 0, st>>>(p.rho, p.idx, nc, p.key);
  if (int rc = sort_pairs(who, p, p.key, p.key2, p.idx, p.idx2, (size_t)nc, 64u, st)) return rc;
  ranked_kernel<<<gc, 256, 0, st>>>(p.tri, p.idx2, nc, p.tri_r, p.ek);
  if (int rc = sort_keys(who, p.ek, p.es, (size_t)c3, n, p.temp, p.tb, st)) return rc;
  slots_kernel<<<gc, 256, 0, st>>>(p.ek, p.es, nc, taken, n_taken, p.slot, p.live);
  return check_launch(who);
}

extern "C" int32_t slg_surface_round(void* pass_ws_, int64_t pass_ws_bytes, int64_t n, int64_t n_candidates, int64_t n_taken,
                                     void* stream) {
  const char* who = "slg_surface_round";
  PassWs p;
  if (int rc = bind_pass(who, n, n_candidates, n_taken, pass_ws_, pass_ws_bytes, &p)) return rc;
  PassHdr* ph = (PassHdr*)pass_ws_;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nc = n_candidates;
  const int gc = grid_of(nc, 256);
  if (hipMemsetAsync(&ph->live, 0, 8, st) != hipSuccess || hipMemsetAsync(p.word, 0xFF, (size_t)nc * 12, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  offer_kernel<<<gc, 256, 0, st>>>(p.live, p.slot, nc, p.word);
  pick_kernel<<<gc, 256, 0, st>>>(ph, p.live, p.slot, p.word, nc, p.acc, p.mark);
  drop_kernel<<<gc, 256, 0, st>>>(ph, p.live, p.slot, p.mark, nc);
  return check_launch(who);
}

extern "C" int32_t slg_surface_commit(void* pass_ws_, int64_t pass_ws_bytes, int64_t n, int64_t n_candidates,
                                      const uint64_t* taken, int64_t n_taken, int64_t n_accepted, int32_t* triangles_out,
                                      uint64_t* taken_out, uint8_t* closed, void* stream) {
  const char* who = "slg_surface_commit";
  if (!taken || !triangles_out || !taken_out || !closed || n_accepted <= 0 || n_accepted > n_candidates)
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL buffer, or no or more accepted triangles than candidates", who);
  PassWs p;
  if (int rc = bind_pass(who, n, n_candidates, n_taken, pass_ws_, pass_ws_bytes, &p)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nc = n_candidates, nm = n_taken + 3 * n_accepted;
  if (int rc = scan_u8(who, p.acc, p.apos, (size_t)nc, p.temp, p.tb, st)) return rc;
  if (n_taken && hipMemcpyAsync(p.mk + 3 * n_accepted, taken, (size_t)n_taken * 8, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: copy failed", who);
  append_kernel<<<grid_of(nc, 256), 256, 0, st>>>(p.tri_r, p.ek, p.acc, p.apos, nc, n_accepted, triangles_out, p.mk);
  if (int rc = sort_keys(who, p.mk, taken_out, (size_t)nm, n, p.temp, p.tb, st)) return rc;
  if (hipMemsetAsync(p.has, 0, (size_t)n, st) != hipSuccess || hipMemsetAsync(p.open, 0, (size_t)n, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  edge_ends_kernel<<<grid_of(nm, 256), 256, 0, st>>>(taken_out, nm, n, p.has, p.open);
  closed_kernel<<<grid_of(n, 256), 256, 0, st>>>(p.has, p.open, n, closed);
  return check_launch(who);
}
