// triangulate.h -- the ray-plane intersection of one valid pixel (fp64, NumPy's operation order)
// and the phase-B schedules of main3_kernel that run it over a tile's items.  Device only; every
// name is TU-local.
#pragma once
#include "decode.h"

namespace {

struct TriOut {
  double x, y, z;      // column-stream point (row_mode 0/1), or column point (row_mode 2)
  double rx, ry, rz;   // row-stream point (row_mode 2)
  double t, tr;        // their ray parameters: (x, y, z) = Oc + r * t, (rx, ry, rz) = Oc + r * tr
  uint32_t keep;       // bit 0 column stream, bit 1 row stream
};

// Ray-plane intersection of one valid pixel (processing.py:143-234), fp64 in NumPy's order, in
// three parts so phase B can issue an item's plane gathers, compute its ray while they are in
// flight, and only then combine (tri_item chains them for the other callers).
struct TriPlanes {
  double2 pc01, pc23;  // column plane: (n0, n1), (n2, d or numer)
  double2 pr01, pr23;  // row plane (row_mode 1/2)
};

// Plane rows: (n0, n1, n2, d) row-major, or -- with the precomputed-numerator tables -- split
// in pair planes [0][c] = (n0, n1), [1][c] = (n2, numer): a wave's consecutive column codes
// then read consecutive 16-byte pairs (8 per cache line) instead of every other 16 bytes of
// 32-byte rows.
// NP: 0 reads p.num_pre at run time, 1 / 2 take it as set / clear (phase B picks per workgroup).
template <int NP = 0>
__device__ inline void tri_planes_col(const MainParams& p, uint32_t code, double2& pc01, double2& pc23) {
  if (NP == 1 || (NP == 0 && p.num_pre)) {
    const double2* qc = reinterpret_cast<const double2*>(p.pcol);
    const uint32_t cc = code & 0xffffu;
    pc01 = qc[cc];
    pc23 = qc[p.n_pcol + cc];
  } else {
    const double2* qc = reinterpret_cast<const double2*>(p.pcol + 4 * int64_t(code & 0xffffu));
    pc01 = qc[0];
    pc23 = qc[1];
  }
}

template <int ROW_MODE, int NP = 0>
__device__ inline void tri_planes_row(const MainParams& p, uint32_t code, double2& pr01, double2& pr23) {
  pr01 = make_double2(0, 0);
  pr23 = make_double2(0, 0);
  if constexpr (ROW_MODE == 2) {
    if (NP == 1 || (NP == 0 && p.num_pre)) {
      const double2* qr = reinterpret_cast<const double2*>(p.prow);
      pr01 = qr[code >> 16];
      pr23 = qr[p.n_prow + (code >> 16)];
    } else {
      const double2* qr = reinterpret_cast<const double2*>(p.prow + 4 * int64_t(code >> 16));
      pr01 = qr[0];
      pr23 = qr[1];
    }
  } else if constexpr (ROW_MODE != 0) {
    const double2* qr = reinterpret_cast<const double2*>(p.prow + 4 * int64_t(code >> 16));
    pr01 = qr[0];
    pr23 = qr[1];
  }
}

template <int ROW_MODE, int NP = 0>
__device__ inline TriPlanes tri_planes(const MainParams& p, uint32_t code) {
  TriPlanes t;
  tri_planes_col<NP>(p, code, t.pc01, t.pc23);
  tri_planes_row<ROW_MODE, NP>(p, code, t.pr01, t.pr23);
  return t;
}

// sqrt and 1/x of a double in [1, 2^900): the same fma sequences the compiler's IEEE-correct
// expansions run (v_rsq_f64 + two Newton/correction rounds; v_rcp_f64 + two Newton rounds +
// one correction, as v_div_scale/v_div_fmas/v_div_fixup compute them when nothing needs
// scaling), without the range scaling and special-case selects that cannot trigger here: the
// same bits, 11 fewer VALU instructions per pixel.
__device__ inline double sqrt_ge1(double x) {
  const double g = __builtin_amdgcn_rsq(x);
  double s = x * g, h = g * 0.5;
  const double r = __builtin_fma(-h, s, 0.5);
  s = __builtin_fma(s, r, s);
  double d = __builtin_fma(-s, s, x);
  h = __builtin_fma(h, r, h);
  s = __builtin_fma(d, h, s);
  d = __builtin_fma(-s, s, x);
  return __builtin_fma(d, h, s);
}

__device__ inline double rcp_ge1(double n) {
  double y = __builtin_amdgcn_rcp(n);
  y = __builtin_fma(y, __builtin_fma(-n, y, 1.0), y);
  y = __builtin_fma(y, __builtin_fma(-n, y, 1.0), y);
  return __builtin_fma(__builtin_fma(-n, y, 1.0), y, y);
}

// The pixel's unit ray (processing.py:143-156).  FAST (p.rays_fast, checked on the host for
// every column and row of the image): the Markstein conditions hold for every pixel, so the
// code is one straight-line block with no per-lane fallback branches -- the same values.
template <int RAYS, bool FAST = false>
__device__ inline void tri_ray(const MainParams& p, int u, int v, double& r0, double& r1, double& r2) {
  if (RAYS == SLG_RAYS_PINHOLE) {
    // The same IEEE quotients as the reference, with the divisions by fx, fy (per camera)
    // and by the norm (three per pixel) done as Markstein corrections of one reciprocal.
    // (Per-column / per-row tables of x and y measured 8 % slower: two more L2 gathers per
    // point cost more than the fp64 they replace.)
    const double ax = double(u) - p.cx, ay = double(v) - p.cy;
    double x, y;
    if constexpr (FAST) {
      x = div_rn(ax, p.fx, p.rfx);                         // processing.py:150
      y = div_rn(ay, p.fy, p.rfy);                         // processing.py:151
    } else {
      x = p.div_fast && div_rn_ok(ax) ? div_rn(ax, p.fx, p.rfx) : ax / p.fx;
      y = p.div_fast && div_rn_ok(ay) ? div_rn(ay, p.fy, p.rfy) : ay / p.fy;
    }
    // np.linalg.norm(rays, axis=0), then rays /= norms; FAST: n in [1, 2^450) (host check)
    const double s2 = (x * x + y * y) + 1.0;
    const double n = FAST ? sqrt_ge1(s2) : sqrt(s2);
    r2 = FAST ? rcp_ge1(n) : 1.0 / n;
    if (FAST || (n < 0x1p900 && div_rn_ok(x) && div_rn_ok(y))) {   // n >= 1: its reciprocal is normal
      r0 = div_rn(x, n, r2); r1 = div_rn(y, n, r2);
    } else {
      r0 = x / n; r1 = y / n;
    }
  } else {
    const int64_t px = int64_t(v) * p.width + u;
    r0 = p.rays[px]; r1 = p.rays[p.n_px + px]; r2 = p.rays[2 * p.n_px + px];
  }
}

template <int ROW_MODE, bool FAST = false, int NP = 0>
__device__ inline TriOut tri_combine(const MainParams& p, const TriPlanes& pl, double r0, double r1, double r2) {
  const bool num_pre = NP == 1 || (NP == 0 && p.num_pre);
  const double2 pc01 = pl.pc01, pc23 = pl.pc23, pr01 = pl.pr01, pr23 = pl.pr23;
  TriOut o;
  const double den = (pc01.x * r0 + pc01.y * r1) + pc23.x * r2;          // np.sum(N*rays, 0)
  // numer = n.Oc + d (processing.py:163-165): precomputed per plane by the caller (column 3 of
  // the table) or computed here
  const double num = num_pre ? pc23.y : ((pc01.x * p.o0 + pc01.y * p.o1) + pc23.x * p.o2) + pc23.y;
  const bool okc = fabs(den) > 1e-6;
  double t;
  if constexpr (FAST) {
    const double q = (-num) / den;                         // unconditional: a select, not a branch
    t = okc ? q : 0.0;
  } else {
    t = okc ? (-num) / den : 0.0;
  }
  o.x = p.o0 + r0 * t; o.y = p.o1 + r1 * t; o.z = p.o2 + r2 * t;
  o.t = t;
  o.tr = 0.0;
  o.keep = okc;
  o.rx = o.ry = o.rz = 0.0;
  if constexpr (ROW_MODE == 1) {                          // epipolar filter, processing.py:197-201
    const double dist = fabs(((pr01.x * o.x + pr01.y * o.y) + pr23.x * o.z) + pr23.y);
    o.keep = okc && (dist < p.tol);
  }
  if constexpr (ROW_MODE == 2) {                          // independent row cloud, :218-228
    const double dr = (pr01.x * r0 + pr01.y * r1) + pr23.x * r2;
    const double nr = num_pre ? pr23.y : ((pr01.x * p.o0 + pr01.y * p.o1) + pr23.x * p.o2) + pr23.y;
    const bool okr = fabs(dr) > 1e-6;
    double tr;
    if constexpr (FAST) {
      const double q = (-nr) / dr;
      tr = okr ? q : 0.0;
    } else {
      tr = okr ? (-nr) / dr : 0.0;
    }
    o.rx = p.o0 + r0 * tr; o.ry = p.o1 + r1 * tr; o.rz = p.o2 + r2 * tr;
    o.tr = tr;
    o.keep |= uint32_t(okr) << 1;
  }
  return o;
}

template <int ROW_MODE, int RAYS, bool FAST = false>
__device__ inline TriOut tri_item(const MainParams& p, uint32_t code, int u, int v) {
  const TriPlanes pl = tri_planes<ROW_MODE>(p, code);
  double r0, r1, r2;
  tri_ray<RAYS, FAST>(p, u, v, r0, r1, r2);
  return tri_combine<ROW_MODE, FAST>(p, pl, r0, r1, r2);
}

#ifndef SLG_TRI_GROUP
#define SLG_TRI_GROUP 4                    // phase B: rounds (items per lane) whose gathers are in flight together
#endif

// LDS slots of compacted item m: phase A writes lane L's items at m = prefix(L) + j, a stride of
// up to 8 items between neighbouring lanes (16 words for the 8-byte records: 16 lanes per
// bank); one pad slot per 16 records (per 8 BGR words) makes that stride odd in words.
#ifndef SLG_ITEM_PAD
#define SLG_ITEM_PAD 4                     // one pad record per 2^SLG_ITEM_PAD items
#endif
#ifndef SLG_BGR_PAD
#define SLG_BGR_PAD 3                      // one pad word per 2^SLG_BGR_PAD BGR words
#endif
constexpr int kItemSlots = kTilePx + (kTilePx >> SLG_ITEM_PAD), kBgrSlots = kTilePx + (kTilePx >> SLG_BGR_PAD);
__device__ inline int item_slot(int m) { return m + (m >> SLG_ITEM_PAD); }
__device__ inline int bgr_slot(int m) { return m + (m >> SLG_BGR_PAD); }

// Round r of a lane's items: its point into the register arrays (NC == 1: the ray parameters
// only, x64_keep_t; NS == 2: row_mode 2's row point too) and one ballot per stream of `keep`.
template <typename XT, int NS, int kIt, int NC>
__device__ __forceinline__ void tri_store(const TriOut& o, uint32_t keep, int r, XT (&pts)[NS][kIt][NC],
                                          uint64_t (&km)[NS][kIt]) {
  if constexpr (NC == 1) {
    pts[0][r][0] = o.t;
    if constexpr (NS == 2) pts[NS - 1][r][0] = o.tr;
  } else {
    pts[0][r][0] = XT(o.x); pts[0][r][1] = XT(o.y); pts[0][r][2] = XT(o.z);
    if constexpr (NS == 2) {
      pts[NS - 1][r][0] = XT(o.rx); pts[NS - 1][r][1] = XT(o.ry); pts[NS - 1][r][2] = XT(o.rz);
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) km[s][r] = __ballot((keep >> s) & 1u);
}

// Phase B of main3 for rounds [i, i + G) (item m = tid + kTileBlock * round), FAST path: the G
// items' loads and fp64 chains are independent, so their plane gathers are in flight together.
// i is any round (the unrolled group loop passes compile-time multiples of G).  This is the grouped schedule (SLG_TRI_GROUP): the instances without static schedules run it
// (row_mode 2 with f32 XYZ, or every instance of a -DSLG_TRI_STATIC=0 build); the others take
// tri_rounds_static below.
template <int G, int ROW_MODE, int RAYS, typename XT, int NS, int kIt, int NP = 0, int NC = 3>
__device__ inline void tri_rounds_at(const MainParams& p, int i, int n_items, const uint2* s_item,
                                     XT (&pts)[NS][kIt][NC], uint64_t (&km)[NS][kIt]) {
  const int tid = threadIdx.x;
  TriOut o[G];
  TriPlanes pl[G];
  double ra[G][3];
  bool in[G];
  uint32_t uvs[G];
#pragma unroll
  for (int h = 0; h < G; ++h) {                    // the G items' plane gathers, all in flight ...
    const int m = tid + kTileBlock * (i + h);
    in[h] = m < n_items;
    const uint2 it = s_item[item_slot(m)];          // m < kTilePx; garbage past n_items masked
    const uint32_t sc = it.x, suv = it.y;
    const uint32_t code = in[h] ? sc : 0u;
    uvs[h] = in[h] ? suv : 0u;
    pl[h] = tri_planes<ROW_MODE, NP>(p, code);
  }
#pragma unroll
  for (int h = 0; h < G; ++h)                      // ... while the rays are computed
    tri_ray<RAYS, true>(p, int(uvs[h] & 0xffffu), int(uvs[h] >> 16), ra[h][0], ra[h][1], ra[h][2]);
  __builtin_amdgcn_sched_barrier(0);               // keep the combine (first use of the planes) after them
#pragma unroll
  for (int h = 0; h < G; ++h) o[h] = tri_combine<ROW_MODE, true, NP>(p, pl[h], ra[h][0], ra[h][1], ra[h][2]);
#pragma unroll
  for (int h = 0; h < G; ++h) {
    const uint32_t keep = in[h] ? o[h].keep : 0u;
    // runtime round index: select into the register arrays (unrolled compares, no scratch)
#pragma unroll
    for (int r = 0; r < kIt; ++r)
      if (r == i + h) tri_store(o[h], keep, r, pts, km);
  }
}

// Phase B of main3 for rounds [I0, I0 + R), both compile-time (a tile of R <= SLG_TRI_STATIC
// rounds: I0 = 0; a longer one: rounds 0..3, then the rest), FAST path: ONE gather round trip.
// tri_rounds_at's groups are serial -- the next group's gathers leave only after the previous
// combine -- so a tile of 5 or 6 rounds (86 % of the C2 views' tiles) paid two loaded L2 round
// trips, the second for one or two rounds.  Here every round index is a compile-time constant
// (the caller dispatches on the block-uniform round count), so there are no r == i + h select
// chains, and the schedule is:
//   1. the R codes from LDS (one address, immediate round offsets), then item by item its
//      column plane's and its row plane's gathers, the code dead once they are out (8 VGPRs a
//      plane: at most 96 VGPRs of planes in flight at R = 6, when phase A's frame registers
//      are dead);
//   2. the items consumed in issue order, singly while SLG_TRI_WIDE or more other items'
//      planes are held, then SLG_TRI_ILP at a time: each item's pixel is read from LDS one
//      item ahead and its ray computed just before its combine, so at most SLG_TRI_ILP rays
//      are live while the later planes land (the compiler's vmcnt waits count down with the
//      issue order), and every consumed item frees 16 VGPRs of planes for 3 (f32), 6 (f64)
//      or 2 (keep-t) of point.
// The scheduling barriers keep the max-ilp scheduler from hoisting the later rays over the
// earlier combines (which would hold R rays beside R planes).  Per item the fp64 operations,
// their order, the ballots and the ranks are tri_rounds_at's: the same bits.
// Register budget (4 waves per SIMD: 128 VGPRs): the f32 two-axis instances sit at 128 and the
// f64 keep-t ones at 126, none with scratch.  What had to go to get there: the six rounds' (u, v)
// and in-range flags held from the start (re-read / recomputed per item), one LDS address per
// round (item_slot is linear in the round), and an out-of-line call (forced inline: MainParams
// lived in scratch otherwise).  A plane spilled while the gathers are issued costs a vmcnt wait
// between them, i.e. the second round trip back.  The profiling instance, which carries the
// phase stamps too, did not fit (32 bytes of scratch, and slower as a whole for it): it defers
// the last two items' row gathers (LATE) and has none.
#ifndef SLG_TRI_STATIC
#define SLG_TRI_STATIC 6                   // tiles of up to this many rounds take tri_rounds_static (0: none)
#endif
#ifndef SLG_TRI_ILP
#define SLG_TRI_ILP 2                      // items whose ray + combine chains are interleaved
#endif
#ifndef SLG_TRI_WIDE
#define SLG_TRI_WIDE 4                     // ... once fewer than this many other items' planes are held
#endif
template <int I0, int R, int ROW_MODE, int RAYS, typename XT, int NS, int kIt, int NP = 0, int NC = 3, int LATE = 0>
__device__ __forceinline__ void tri_rounds_static(const MainParams& p, int n_items, const uint2* s_item,
                                         XT (&pts)[NS][kIt][NC], uint64_t (&km)[NS][kIt]) {
  static_assert(I0 >= 0 && R >= 1 && I0 + R <= kIt, "rounds of one tile");
  const int tid = threadIdx.x;
  TriPlanes pl[R];
  uint32_t codes[R];
  // LATE (the profiling instance, whose phase stamps take the registers): the last LATE items'
  // row planes, needed last of all, are gathered once item 0 has freed its planes
  constexpr int kLate = R >= 6 ? LATE : 0;
  // m < kTilePx: items past n_items are read and masked (code 0, pixel (0, 0), kept by no stream)
  const int m0 = tid + kTileBlock * I0;             // item of round I0 + h: m0 + kTileBlock * h
  // ... in slot sl0[kRound * h]: one LDS address and immediate offsets, not one address per round
  static_assert(kTileBlock % (1 << SLG_ITEM_PAD) == 0, "item_slot is linear in the round");
  constexpr int kRound = kTileBlock + (kTileBlock >> SLG_ITEM_PAD);
  const uint2* sl0 = s_item + item_slot(m0);
#pragma unroll
  for (int h = 0; h < R; ++h) codes[h] = sl0[kRound * h].x;
#pragma unroll
  for (int h = 0; h < R; ++h) {                    // an item's code is dead once its gathers are out
    const uint32_t code = m0 + kTileBlock * h < n_items ? codes[h] : 0u;
    tri_planes_col<NP>(p, code, pl[h].pc01, pl[h].pc23);
    if (h < R - kLate) tri_planes_row<ROW_MODE, NP>(p, code, pl[h].pr01, pl[h].pr23);
    else codes[h] = code;
  }
  // the pixel of an item is read from LDS one item ahead of its ray, not held for all R
  uint32_t uv_next = sl0[0].y;
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int h = 0; h < R; ++h) {
    {
      const bool in = m0 + kTileBlock * h < n_items;
      const uint32_t uv = in ? uv_next : 0u;
      if (h + 1 < R) uv_next = sl0[kRound * (h + 1)].y;
      double r0, r1, r2;
      tri_ray<RAYS, true>(p, int(uv & 0xffffu), int(uv >> 16), r0, r1, r2);
      const TriOut o = tri_combine<ROW_MODE, true, NP>(p, pl[h], r0, r1, r2);
      tri_store(o, in ? o.keep : 0u, I0 + h, pts, km);
    }
    if (kLate > 0 && h == 0) {
#pragma unroll
      for (int g = R - kLate; g < R; ++g) tri_planes_row<ROW_MODE, NP>(p, codes[g], pl[g].pr01, pl[g].pr23);
    }
    // a group ends here: items go singly while SLG_TRI_WIDE or more others' planes are still
    // held, then SLG_TRI_ILP at a time (counted from the last item)
    const int left = R - 1 - h;
    if (left >= SLG_TRI_WIDE || left % SLG_TRI_ILP == 0) __builtin_amdgcn_sched_barrier(0);
  }
}

}  // namespace
