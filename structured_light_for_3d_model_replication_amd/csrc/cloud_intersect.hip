// cloud_intersect.hip -- which pairs of triangles of an indexed mesh in HBM cross.
// The rule is tests/intersect_ref.py: candidates are the pairs of triangles whose closed boxes
// overlap, classed by the vertex indices they share, and every sign is one fp64 determinant
// (Shewchuk's orient3dfast with its permanent and stage-A bound) under -ffp-contract=off in one
// fixed order of operations.  Our rule, Open3D parity unpinned.
//
// The uniform grid only finds the candidates and no result depends on it: a triangle's integer cell
// range is computed once, a pair of listed triangles is taken in its home cell alone (the per-axis
// maximum of the two low cells, compared on integers), a triangle that spans more than
// SLG_ISECT_SPAN_CAP cells is scanned against all triangles by one workgroup, and two such belong to
// the lower index.  Counts are integer adds (one per wave), class bits are ORed, the candidate keys
// land in whatever order the waves emit them and nothing reads that order: the lists are sorted.
#include "mesh_keys.h"

#include "../../include/slgpu_intersect.h"

namespace slgisect {

using namespace slgmeshpost;

constexpr int kSideBits = 24;                 // the default cell: box sides in 2^-24 of the widest side
constexpr int kTile = SLG_ISECT_TILE;
constexpr int kMaxCells = SLG_ISECT_MAX_CELLS;
constexpr int kSpanCap = SLG_ISECT_SPAN_CAP;
constexpr double kBound = SLG_ISECT_BOUND;
constexpr int64_t kMaxItems = 1ll << 40;
constexpr uint8_t kSkip = 0, kListed = 1, kLarge = 2;

struct IsectHdr {
  int32_t status;       // SLG_FILTER_BAD_INDEX
  int32_t R;            // unused
  int64_t n_entries, n_large, n_part, n_runs, n_cand;
  unsigned long long cursor;                 // the emit walk's next key
  int32_t dims[3];
  int32_t pad;
  double origin[3], cell;
  double unused[3];
  int64_t stats[8];     // SLG_ISECT_STAT_*
  unsigned long long ext[6];                 // ordered(): -low corner, high corner of the mesh's box; 0 none
  int64_t side_sum;                          // the longest box sides in 2^-kSideBits of the widest side
};
static_assert(sizeof(IsectHdr) <= SLG_MESH_HDR_BYTES, "header");
static_assert(offsetof(IsectHdr, n_entries) == 8 && offsetof(IsectHdr, n_large) == 16 && offsetof(IsectHdr, n_part) == 24 &&
              offsetof(IsectHdr, n_runs) == 32 && offsetof(IsectHdr, n_cand) == 40 && offsetof(IsectHdr, dims) == 56 &&
              offsetof(IsectHdr, origin) == 72 && offsetof(IsectHdr, cell) == 96 && offsetof(IsectHdr, stats) == 128 &&
              offsetof(IsectHdr, ext) == 192 && offsetof(IsectHdr, side_sum) == 240,
              "mesh.py's offsets");

// ---------------------------------------------------------------- workspaces
static inline size_t scan_temp(size_t n) { return n + (4u << 20); }
struct BoxWs { double* box; int32_t *clo, *chi; uint8_t *tinfo, *cnt, *lflag; uint64_t *off, *lpos; uint32_t *large, *tword;
               void* temp; size_t tb; };
static BoxWs box_ws(Bump& b, int64_t nt) {
  BoxWs w;
  w.box = b.take<double>(6 * (size_t)nt);
  w.clo = b.take<int32_t>(3 * (size_t)nt);
  w.chi = b.take<int32_t>(3 * (size_t)nt);
  w.tinfo = b.take<uint8_t>(nt);
  w.cnt = b.take<uint8_t>(nt);
  w.lflag = b.take<uint8_t>(nt);
  w.off = b.take<uint64_t>(nt);
  w.lpos = b.take<uint64_t>(nt);
  w.large = b.take<uint32_t>(nt);
  w.tword = b.take<uint32_t>(nt);
  w.tb = scan_temp((size_t)nt);
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
struct EntryWs { uint64_t *k, *s, *hpos, *runs; uint8_t* head; void* temp; size_t tb; };
static EntryWs entry_ws(Bump& b, int64_t n) {
  EntryWs w;
  w.k = b.take<uint64_t>(n);
  w.s = b.take<uint64_t>(n);
  w.hpos = b.take<uint64_t>(n);
  w.runs = b.take<uint64_t>(n);
  w.head = b.take<uint8_t>(n);
  w.tb = sort_temp((size_t)n);
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
struct PairWs { uint64_t *keys, *pos; uint8_t *verdict, *flag; void* temp; size_t tb; };
static PairWs pair_ws(Bump& b, int64_t n) {
  PairWs w;
  w.keys = b.take<uint64_t>(n);
  w.pos = b.take<uint64_t>(n);
  w.verdict = b.take<uint8_t>(n);
  w.flag = b.take<uint8_t>(n);
  w.tb = scan_temp((size_t)n);
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
struct ListWs { uint64_t *comp, *sorted; void* temp; size_t tb; };
static ListWs list_ws(Bump& b, int64_t n) {
  ListWs w;
  w.comp = b.take<uint64_t>(n);
  w.sorted = b.take<uint64_t>(n);
  w.tb = sort_temp((size_t)n);
  w.temp = b.take<uint8_t>(w.tb);
  return w;
}
static size_t stage_bytes(int stage, int64_t nt, int64_t n_items) {
  Bump b(nullptr, stage == SLG_ISECT_WS_BOXES ? SLG_MESH_HDR_BYTES : 0);
  if (stage == SLG_ISECT_WS_BOXES) box_ws(b, nt);
  else if (stage == SLG_ISECT_WS_ENTRIES) entry_ws(b, n_items);
  else if (stage == SLG_ISECT_WS_PAIRS) pair_ws(b, n_items);
  else list_ws(b, n_items);
  return b.off;
}
static inline bool items_ok(int64_t n) { return n > 0 && n <= kMaxItems; }
static inline bool entries_ok(int64_t n, int64_t nt) { return n <= (int64_t)kSpanCap * nt && n < (1ll << 31); }   // one workgroup each

namespace {

// One add per wave of the lanes where `on` holds.
__device__ inline void wave_count(int64_t* dst, bool on) {
  const unsigned long long m = __ballot(on);
  if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd((unsigned long long*)dst, (unsigned long long)__popcll(m));
}
// One add per wave of the lanes' values; every lane of the wave calls it.
__device__ inline void wave_add(int64_t* dst, uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long*)dst, (unsigned long long)v);
}
__device__ inline double min3(double a, double b, double c) { const double m = a < b ? a : b; return m < c ? m : c; }
__device__ inline double max3(double a, double b, double c) { const double m = a > b ? a : b; return m > c ? m : c; }

// ---------------------------------------------------------------- boxes and the grid
// A finite double as an integer that orders the same way: the mesh's box is six integer maxima
// (of the negated low corner and of the high corner), zero standing for none.
__device__ inline unsigned long long ordered(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : b | (1ull << 63);
}
__device__ inline double unordered(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? k & ~(1ull << 63) : ~k));
}
// One lane per triangle.  A triangle that takes no part (a bad index, which sets the status word,
// two equal indices, a coordinate that is not finite) gets a zero box and kSkip.
__global__ __launch_bounds__(256)
void box_kernel(IsectHdr* hdr, const double* __restrict__ vert, int64_t nv, const int32_t* __restrict__ tris, int64_t nt,
                double* __restrict__ box, uint8_t* __restrict__ tinfo) {
  __shared__ unsigned long long sext[6];
  if (threadIdx.x < 6) sext[threadIdx.x] = 0ull;
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool on = false;
  if (t < nt) {
    const int32_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    const bool bad = i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv;
    if (bad) atomicOr(&hdr->status, SLG_FILTER_BAD_INDEX);
    on = !bad && !(i0 == i1 || i1 == i2 || i2 == i0);
    double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
    if (on) {
      for (int a = 0; a < 3; ++a) {
        const double x = vert[3 * (int64_t)i0 + a], y = vert[3 * (int64_t)i1 + a], z = vert[3 * (int64_t)i2 + a];
        on = on && isfinite(x) && isfinite(y) && isfinite(z);
        lo[a] = min3(x, y, z);
        hi[a] = max3(x, y, z);
      }
    }
    for (int a = 0; a < 3; ++a) {
      box[6 * t + a] = on ? lo[a] : 0.0;
      box[6 * t + 3 + a] = on ? hi[a] : 0.0;
    }
    tinfo[t] = on ? kListed : kSkip;
    if (on)
      for (int a = 0; a < 3; ++a) {
        atomicMax(&sext[a], ordered(-lo[a]));
        atomicMax(&sext[3 + a], ordered(hi[a]));
      }
  }
  wave_count(&hdr->n_part, on);
  __syncthreads();
  if (threadIdx.x < 6 && sext[threadIdx.x]) atomicMax(&hdr->ext[threadIdx.x], sext[threadIdx.x]);
}
__device__ inline double widest_side(const IsectHdr* hdr) {
  double w = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double d = unordered(hdr->ext[3 + a]) + unordered(hdr->ext[a]);
    w = w > d ? w : d;
  }
  return w;
}
// The sum of the longest box sides in units of 2^-kSideBits of the mesh's widest side: integer adds,
// one per wave, so the default cell does not depend on their order.
__global__ __launch_bounds__(256)
void side_kernel(IsectHdr* hdr, const double* __restrict__ box, const uint8_t* __restrict__ tinfo, int64_t nt) {
  if (hdr->status || hdr->n_part == 0) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const double widest = widest_side(hdr);
  uint32_t q = 0;
  if (t < nt && tinfo[t] != kSkip && widest > 0.0) {
    const double side = max3(box[6 * t + 3] - box[6 * t], box[6 * t + 4] - box[6 * t + 1], box[6 * t + 5] - box[6 * t + 2]);
    const double f = side / widest * (double)(1u << kSideBits);
    q = f >= (double)(1u << kSideBits) ? (1u << kSideBits) : (f > 0.0 ? (uint32_t)f : 0u);
  }
  wave_add(&hdr->side_sum, q);
}
// The grid.  The cell side is the override when positive, else twice the mean longest side; it
// grows until kMaxCells cells cover the widest axis.
__global__ void grid_kernel(IsectHdr* hdr, double cell_override) {
  if (hdr->status) return;
  const int64_t n = hdr->n_part;
  const double widest = n > 0 ? widest_side(hdr) : 0.0;
  double cell = 1.0;
  if (n > 0) {
    cell = cell_override > 0.0 ? cell_override : 2.0 * ((double)hdr->side_sum / (double)n) * widest / (double)(1u << kSideBits);
    if (!(cell > 0.0) || !isfinite(cell)) cell = widest > 0.0 && isfinite(widest) ? widest : 1.0;
    if (cell * (double)kMaxCells < widest) cell = widest / (double)kMaxCells;
  }
  hdr->cell = cell;
  for (int a = 0; a < 3; ++a) {
    const double lo = n > 0 ? -unordered(hdr->ext[a]) : 0.0, hi = n > 0 ? unordered(hdr->ext[3 + a]) : 0.0;
    hdr->origin[a] = lo;
    double q = floor((hi - lo) / cell) + 1.0;
    if (!(q >= 1.0)) q = 1.0;
    hdr->dims[a] = q > (double)kMaxCells ? kMaxCells : (int32_t)q;
  }
}
// A coordinate's cell on one axis: monotone in x, inside 0 .. dim - 1 whatever the rounding.
__device__ inline int32_t cell_of(double x, double origin, double cell, int32_t dim) {
  double q = floor((x - origin) / cell);
  if (!(q >= 0.0)) q = 0.0;
  return q > (double)(dim - 1) ? dim - 1 : (int32_t)q;
}
// Per triangle: the integer cell range, the number of its entries (0 for one that takes no part
// and for a large one) and whether it goes to the large list.
__global__ __launch_bounds__(256)
void cells_kernel(IsectHdr* hdr, const double* __restrict__ box, int64_t nt, uint8_t* __restrict__ tinfo, int32_t* __restrict__ clo,
                  int32_t* __restrict__ chi, uint8_t* __restrict__ cnt, uint8_t* __restrict__ lflag) {
  if (hdr->status) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t entries = 0;
  bool large = false;
  if (t < nt) {
    int64_t span = 0;
    int32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    if (tinfo[t] != kSkip) {
      span = 1;
      for (int a = 0; a < 3; ++a) {
        lo[a] = cell_of(box[6 * t + a], hdr->origin[a], hdr->cell, hdr->dims[a]);
        hi[a] = cell_of(box[6 * t + 3 + a], hdr->origin[a], hdr->cell, hdr->dims[a]);
        if (hi[a] < lo[a]) hi[a] = lo[a];
        span *= (int64_t)(hi[a] - lo[a] + 1);
      }
      large = span > kSpanCap;
      entries = large ? 0u : (uint32_t)span;
      tinfo[t] = large ? kLarge : kListed;
    }
    for (int a = 0; a < 3; ++a) {
      clo[3 * t + a] = lo[a];
      chi[3 * t + a] = hi[a];
    }
    cnt[t] = (uint8_t)entries;
    lflag[t] = large ? 1 : 0;
  }
  wave_add(&hdr->n_entries, entries);
  wave_count(&hdr->n_large, large);
}
__global__ __launch_bounds__(256)
void large_list_kernel(const IsectHdr* hdr, const uint8_t* __restrict__ lflag, const uint64_t* __restrict__ lpos, int64_t nt,
                       uint32_t* __restrict__ large) {
  if (hdr->status) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < nt && lflag[t] && lpos[t] < (uint64_t)nt) large[lpos[t]] = (uint32_t)t;
}

// ---------------------------------------------------------------- entries and runs
__global__ __launch_bounds__(256)
void entry_kernel(const IsectHdr* hdr, const uint8_t* __restrict__ cnt, const uint64_t* __restrict__ off, const int32_t* __restrict__ clo,
                  const int32_t* __restrict__ chi, int64_t nt, uint64_t* __restrict__ k, int64_t n_entries) {
  if (hdr->status || hdr->n_entries != n_entries) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt || !cnt[t]) return;
  uint64_t o = off[t];
  const int64_t dx = hdr->dims[0], dy = hdr->dims[1];
  for (int32_t z = clo[3 * t + 2]; z <= chi[3 * t + 2]; ++z)
    for (int32_t y = clo[3 * t + 1]; y <= chi[3 * t + 1]; ++y)
      for (int32_t x = clo[3 * t]; x <= chi[3 * t]; ++x, ++o)
        if (o < (uint64_t)n_entries) k[o] = edge_key((uint32_t)(((int64_t)z * dy + y) * dx + x), (uint32_t)t);
}
// The first entry of every cell.
__global__ __launch_bounds__(256)
void head_kernel(const IsectHdr* hdr, const uint64_t* __restrict__ s, int64_t n, uint8_t* __restrict__ head) {
  if (hdr->status || hdr->n_entries != n) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) head[i] = (i == 0 || key_src(s[i]) != key_src(s[i - 1])) ? 1 : 0;
}
__global__ __launch_bounds__(256)
void run_kernel(IsectHdr* hdr, const uint8_t* __restrict__ head, const uint64_t* __restrict__ hpos, int64_t n,
                uint64_t* __restrict__ runs) {
  if (hdr->status || hdr->n_entries != n) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (head[i] && hpos[i] < (uint64_t)n) runs[hpos[i]] = (uint64_t)i;
  if (i == n - 1) hdr->n_runs = (int64_t)(hpos[i] + head[i]);
}

// ---------------------------------------------------------------- candidates
__device__ inline bool boxes_overlap(const double* a, const double* b) {
  return a[0] <= b[3] && b[0] <= a[3] && a[1] <= b[4] && b[1] <= a[4] && a[2] <= b[5] && b[2] <= a[5];
}
// The lanes of a wave where `on` holds take consecutive places behind the cursor.
__device__ inline void wave_emit(IsectHdr* hdr, bool on, uint64_t key, uint64_t* __restrict__ out, int64_t cap) {
  const unsigned long long m = __ballot(on);
  if (!m) return;
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(&hdr->cursor, (unsigned long long)__popcll(m));
  const uint32_t lo = __shfl((uint32_t)base, leader, 64), hi = __shfl((uint32_t)(base >> 32), leader, 64);
  const uint64_t at = (((uint64_t)hi << 32) | lo) + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
  if (on && at < (uint64_t)cap) out[at] = key;
}
// One wavefront per cell run (a workgroup past the last run returns).  The lanes hold kTile boxes of
// the run, every later box of the run passes through LDS in tiles of kTile, and a pair is taken
// when the boxes overlap and this cell is its home.  A run's entries ascend by triangle.
template <bool EMIT>
__global__ __launch_bounds__(kTile)
void run_pairs_kernel(IsectHdr* hdr, const uint64_t* __restrict__ s, const uint64_t* __restrict__ runs, int64_t n_entries,
                      const double* __restrict__ box, const int32_t* __restrict__ clo, uint64_t* __restrict__ out, int64_t cap) {
  __shared__ double sbox[kTile][6];
  __shared__ int32_t slo[kTile][3];
  __shared__ uint32_t stri[kTile];
  if (hdr->status || hdr->n_entries != n_entries || (EMIT && hdr->n_cand != cap)) return;
  const int lane = threadIdx.x;
  const int64_t n_runs = hdr->n_runs;
  const int64_t dx = hdr->dims[0], dy = hdr->dims[1];
  uint32_t found = 0;
  const int64_t r = blockIdx.x;
  if (r < n_runs) {
    const int64_t b = (int64_t)runs[r], e = r + 1 < n_runs ? (int64_t)runs[r + 1] : n_entries;
    const int64_t cell = (int64_t)key_src(s[b]);
    const int32_t home[3] = {(int32_t)(cell % dx), (int32_t)((cell / dx) % dy), (int32_t)(cell / (dx * dy))};
    for (int64_t ta = b; ta < e; ta += kTile) {
      const int64_t ia = ta + lane;
      const bool have = ia < e;
      const uint32_t mine = have ? key_dst(s[ia]) : 0u;
      double mb[6];
      int32_t ml[3];
      for (int a = 0; a < 6; ++a) mb[a] = have ? box[6 * (int64_t)mine + a] : 0.0;
      for (int a = 0; a < 3; ++a) ml[a] = have ? clo[3 * (int64_t)mine + a] : 0;
      for (int64_t tb = ta; tb < e; tb += kTile) {
        __syncthreads();                         // the tile before has been read by every lane
        if (tb + lane < e) {
          const uint32_t t = key_dst(s[tb + lane]);
          stri[lane] = t;
          for (int a = 0; a < 6; ++a) sbox[lane][a] = box[6 * (int64_t)t + a];
          for (int a = 0; a < 3; ++a) slo[lane][a] = clo[3 * (int64_t)t + a];
        }
        __syncthreads();
        const int m = e - tb < kTile ? (int)(e - tb) : kTile;
        for (int k = 0; k < m; ++k) {
          bool take = have && tb + k > ia && boxes_overlap(mb, sbox[k]);
          if (take)
            for (int a = 0; a < 3; ++a) take = take && (ml[a] > slo[k][a] ? ml[a] : slo[k][a]) == home[a];
          if (EMIT) wave_emit(hdr, take, edge_key(mine, stri[k]), out, cap);
          else found += take ? 1u : 0u;
        }
      }
    }
  }
  if (!EMIT) wave_add(&hdr->n_cand, found);
}
// One workgroup per large triangle against all triangles; two large ones belong to the lower index.
template <bool EMIT>
__global__ __launch_bounds__(256)
void large_pairs_kernel(IsectHdr* hdr, const uint32_t* __restrict__ large, int64_t nt, const double* __restrict__ box,
                        const uint8_t* __restrict__ tinfo, uint64_t* __restrict__ out, int64_t cap) {
  if (hdr->status || hdr->n_large != (int64_t)gridDim.x || (EMIT && hdr->n_cand != cap)) return;
  const uint32_t L = large[blockIdx.x];
  double mb[6];
  for (int a = 0; a < 6; ++a) mb[a] = box[6 * (int64_t)L + a];
  uint32_t found = 0;
  for (int64_t base = 0; base < nt; base += 256) {
    const int64_t t = base + threadIdx.x;
    bool take = false;
    if (t < nt && t != (int64_t)L) {
      const uint8_t info = tinfo[t];
      if (info == kListed || (info == kLarge && t > (int64_t)L)) {
        double ob[6];
        for (int a = 0; a < 6; ++a) ob[a] = box[6 * t + a];
        take = boxes_overlap(mb, ob);
      }
    }
    const uint32_t lo = t < (int64_t)L ? (uint32_t)t : L, hi = t < (int64_t)L ? L : (uint32_t)t;
    if (EMIT) wave_emit(hdr, take, edge_key(lo, hi), out, cap);
    else found += take ? 1u : 0u;
  }
  if (!EMIT) wave_add(&hdr->n_cand, found);
}

// ---------------------------------------------------------------- the test
struct P3 { double x, y, z; };
struct Signs { uint32_t pos, neg, cer; };      // one bit per determinant: > 0, < 0, certain
__device__ inline P3 load_point(const double* __restrict__ vert, int32_t i) {
  return P3{vert[3 * (int64_t)i], vert[3 * (int64_t)i + 1], vert[3 * (int64_t)i + 2]};
}
// orient3dfast of (a, b, c, d) with its permanent, every operation as tests/intersect_ref.py's o3
// names it, into bit `bit`.
__device__ inline void o3(const P3& a, const P3& b, const P3& c, const P3& d, int bit, Signs& g) {
  const double adx = a.x - d.x, ady = a.y - d.y, adz = a.z - d.z;
  const double bdx = b.x - d.x, bdy = b.y - d.y, bdz = b.z - d.z;
  const double cdx = c.x - d.x, cdy = c.y - d.y, cdz = c.z - d.z;
  const double m1 = bdy * cdz, m2 = bdz * cdy, m3 = cdy * adz, m4 = cdz * ady, m5 = ady * bdz, m6 = adz * bdy;
  const double det = (adx * (m1 - m2) + bdx * (m3 - m4)) + cdx * (m5 - m6);
  const double perm = ((fabs(m1) + fabs(m2)) * fabs(adx) + (fabs(m3) + fabs(m4)) * fabs(bdx)) + (fabs(m5) + fabs(m6)) * fabs(cdx);
  g.pos |= (det > 0.0 ? 1u : 0u) << bit;
  g.neg |= (det < 0.0 ? 1u : 0u) << bit;
  g.cer |= (fabs(det) > kBound * perm ? 1u : 0u) << bit;
}
__device__ inline bool opposite(const Signs& g, int p, int q) {
  return (((g.pos >> p) & (g.neg >> q)) | ((g.neg >> p) & (g.pos >> q))) & 1u;
}
// One edge against one triangle: the plane sides p1, p2 of its ends, its sides e0, e1, e2 of the
// triangle's edges.
__device__ inline void edge_test(const Signs& g, int p1, int p2, int e0, int e1, int e2, bool on, bool& hit, bool& sure, bool& open) {
  const uint32_t em = (1u << e0) | (1u << e1) | (1u << e2), all = em | (1u << p1) | (1u << p2);
  const bool pierces = opposite(g, p1, p2) && ((g.pos & em) == em || (g.neg & em) == em);
  const bool same = (((g.pos >> p1) & (g.pos >> p2)) | ((g.neg >> p1) & (g.neg >> p2))) & (g.cer >> p1) & (g.cer >> p2) & 1u;
  const bool split = (((g.cer >> e0) & (g.cer >> e1) & 1u) && opposite(g, e0, e1)) ||
                     (((g.cer >> e0) & (g.cer >> e2) & 1u) && opposite(g, e0, e2)) ||
                     (((g.cer >> e1) & (g.cer >> e2) & 1u) && opposite(g, e1, e2));
  const bool piercing = pierces && (g.cer & all) == all;
  hit = hit || (on && pierces);
  sure = sure || (on && piercing);
  open = open || (on && !(same || split) && !piercing);
}
// Determinant bits: alpha_j = j, beta_i = 3 + i, eps_ij = 6 + 3 i + j.
__global__ __launch_bounds__(256)
void test_kernel(IsectHdr* hdr, const double* __restrict__ vert, const int32_t* __restrict__ tris, const uint64_t* __restrict__ keys,
                 int64_t n, int64_t nt, uint8_t* __restrict__ verdict, uint32_t* tword) {
  if (hdr->status || hdr->n_cand != n) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool adjacent = false, tested = false, hit = false, uncertain = false;
  if (i < n) {
    const uint64_t key = keys[i];
    const uint32_t s = key_src(key), t = key_dst(key);
    uint8_t v = 0;
    if (s < (uint64_t)nt && t < (uint64_t)nt) {
      int32_t a0 = tris[3 * (int64_t)s], a1 = tris[3 * (int64_t)s + 1], a2 = tris[3 * (int64_t)s + 2];
      int32_t b0 = tris[3 * (int64_t)t], b1 = tris[3 * (int64_t)t + 1], b2 = tris[3 * (int64_t)t + 2];
      const bool m0 = a0 == b0 || a0 == b1 || a0 == b2, m1 = a1 == b0 || a1 == b1 || a1 == b2,
                 m2 = a2 == b0 || a2 == b1 || a2 == b2;
      const int shared = (int)m0 + (int)m1 + (int)m2;
      adjacent = shared >= 2;
      tested = !adjacent;
      if (tested) {
        if (shared == 1) {                       // rotate both so that a0 == b0
          const int32_t sv = m0 ? a0 : (m1 ? a1 : a2);
          if (m1) { const int32_t x = a0; a0 = a1; a1 = a2; a2 = x; }
          else if (m2) { const int32_t x = a0; a0 = a2; a2 = a1; a1 = x; }
          if (b1 == sv) { const int32_t x = b0; b0 = b1; b1 = b2; b2 = x; }
          else if (b2 == sv) { const int32_t x = b0; b0 = b2; b2 = b1; b1 = x; }
        }
        const P3 A0 = load_point(vert, a0), A1 = load_point(vert, a1), A2 = load_point(vert, a2);
        const P3 B0 = load_point(vert, b0), B1 = load_point(vert, b1), B2 = load_point(vert, b2);
        Signs g{0u, 0u, 0u};
        o3(A0, A1, A2, B0, 0, g);
        o3(A0, A1, A2, B1, 1, g);
        o3(A0, A1, A2, B2, 2, g);
        o3(B0, B1, B2, A0, 3, g);
        o3(B0, B1, B2, A1, 4, g);
        o3(B0, B1, B2, A2, 5, g);
        o3(A0, A1, B0, B1, 6, g);
        o3(A0, A1, B1, B2, 7, g);
        o3(A0, A1, B2, B0, 8, g);
        o3(A1, A2, B0, B1, 9, g);
        o3(A1, A2, B1, B2, 10, g);
        o3(A1, A2, B2, B0, 11, g);
        o3(A2, A0, B0, B1, 12, g);
        o3(A2, A0, B1, B2, 13, g);
        o3(A2, A0, B2, B0, 14, g);
        const bool six = shared == 0;
        bool sure = false, open = false;
        edge_test(g, 3, 4, 6, 7, 8, six, hit, sure, open);          // a0 a1 against B
        edge_test(g, 4, 5, 9, 10, 11, true, hit, sure, open);       // a1 a2
        edge_test(g, 5, 3, 12, 13, 14, six, hit, sure, open);       // a2 a0
        edge_test(g, 0, 1, 6, 9, 12, six, hit, sure, open);         // b0 b1 against A
        edge_test(g, 1, 2, 7, 10, 13, true, hit, sure, open);       // b1 b2
        edge_test(g, 2, 0, 8, 11, 14, six, hit, sure, open);        // b2 b0
        uncertain = !sure && open;
        v = (uint8_t)((hit ? SLG_ISECT_INTERSECTING : 0) | (uncertain ? SLG_ISECT_UNCERTAIN : 0));
        if (v) {
          atomicOr(&tword[s], (uint32_t)v);
          atomicOr(&tword[t], (uint32_t)v);
        }
      }
    }
    verdict[i] = v;
  }
  wave_count(&hdr->stats[SLG_ISECT_STAT_ADJACENT], adjacent);
  wave_count(&hdr->stats[SLG_ISECT_STAT_TESTED], tested);
  wave_count(&hdr->stats[SLG_ISECT_STAT_INTERSECTING], hit);
  wave_count(&hdr->stats[SLG_ISECT_STAT_UNCERTAIN], uncertain);
}
__global__ __launch_bounds__(256)
void class_kernel(IsectHdr* hdr, const uint32_t* __restrict__ tword, int64_t nt, uint8_t* __restrict__ tclass) {
  if (hdr->status) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t w = t < nt ? tword[t] : 0u;
  if (t < nt) tclass[t] = (uint8_t)w;
  wave_count(&hdr->stats[SLG_ISECT_STAT_INTERSECTING_TRIANGLES], (w & SLG_ISECT_INTERSECTING) != 0);
  wave_count(&hdr->stats[SLG_ISECT_STAT_UNCERTAIN_TRIANGLES], (w & SLG_ISECT_UNCERTAIN) != 0);
}

// ---------------------------------------------------------------- the lists
__global__ __launch_bounds__(256)
void flag_kernel(const uint8_t* __restrict__ verdict, int64_t n, int which, uint8_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) flag[i] = (verdict[i] & which) ? 1 : 0;
}
__global__ __launch_bounds__(256)
void compact_kernel(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ flag, const uint64_t* __restrict__ pos, int64_t n,
                    uint64_t* __restrict__ comp, int64_t n_list) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && flag[i] && pos[i] < (uint64_t)n_list) comp[pos[i]] = keys[i];
}
__global__ __launch_bounds__(256)
void unpack_kernel(const uint64_t* __restrict__ sorted, int64_t n_list, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_list) return;
  out[2 * i] = (int32_t)key_src(sorted[i]);
  out[2 * i + 1] = (int32_t)key_dst(sorted[i]);
}

}  // namespace
}  // namespace slgisect

using namespace slgisect;

static const char* kSizer = "slg_isect_ws_bytes";

extern "C" int64_t slg_isect_ws_bytes(int32_t stage, int64_t n_vertices, int64_t n_triangles, int64_t n_items) {
  if (stage < SLG_ISECT_WS_BOXES || stage > SLG_ISECT_WS_LIST || !counts_ok(n_vertices, n_triangles) ||
      (stage == SLG_ISECT_WS_BOXES ? n_items < 0 : !items_ok(n_items)))
    return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_isect_ws_bytes: unknown stage, no vertices, triangles or items, 2^31 "
                                                         "vertices or more, more than 2^30 triangle edges or 2^40 items");
  return (int64_t)stage_bytes(stage, n_triangles, n_items);
}

extern "C" int32_t slg_isect_boxes(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                   double cell, void* ws, int64_t ws_bytes, void* stream) {
  const char* who = "slg_isect_boxes";
  if (!vertices || !triangles || !counts_ok(n_vertices, n_triangles) || cell != cell)
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL buffer, counts out of range or a cell that is no number", who);
  if (int rc = bind(who, kSizer, ws, ws_bytes, stage_bytes(SLG_ISECT_WS_BOXES, n_triangles, 0))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES);
  const BoxWs w = box_ws(b, n_triangles);
  IsectHdr* hdr = (IsectHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const int gt = grid_of(n_triangles, 256);
  if (hipMemsetAsync(hdr, 0, SLG_MESH_HDR_BYTES, st) != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  box_kernel<<<gt, 256, 0, st>>>(hdr, vertices, n_vertices, triangles, n_triangles, w.box, w.tinfo);
  side_kernel<<<gt, 256, 0, st>>>(hdr, w.box, w.tinfo, n_triangles);
  grid_kernel<<<1, 1, 0, st>>>(hdr, cell);
  cells_kernel<<<gt, 256, 0, st>>>(hdr, w.box, n_triangles, w.tinfo, w.clo, w.chi, w.cnt, w.lflag);
  if (int rc = scan_u8(who, w.cnt, w.off, (size_t)n_triangles, w.temp, w.tb, st)) return rc;
  if (int rc = scan_u8(who, w.lflag, w.lpos, (size_t)n_triangles, w.temp, w.tb, st)) return rc;
  large_list_kernel<<<gt, 256, 0, st>>>(hdr, w.lflag, w.lpos, n_triangles, w.large);
  return check_launch(who);
}

extern "C" int32_t slg_isect_entries(int64_t n_triangles, int64_t n_vertices, void* ws, int64_t ws_bytes, int64_t n_entries,
                                     void* entries_ws, int64_t entries_ws_bytes, void* stream) {
  const char* who = "slg_isect_entries";
  if (!counts_ok(n_vertices, n_triangles) || !items_ok(n_entries) || !entries_ok(n_entries, n_triangles))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: counts out of range", who);
  if (int rc = bind(who, kSizer, ws, ws_bytes, stage_bytes(SLG_ISECT_WS_BOXES, n_triangles, 0))) return rc;
  if (int rc = bind(who, kSizer, entries_ws, entries_ws_bytes, stage_bytes(SLG_ISECT_WS_ENTRIES, n_triangles, n_entries))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES), be(entries_ws, 0);
  const BoxWs w = box_ws(b, n_triangles);
  const EntryWs ew = entry_ws(be, n_entries);
  IsectHdr* hdr = (IsectHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  const int ge = grid_of(n_entries, 256);
  entry_kernel<<<grid_of(n_triangles, 256), 256, 0, st>>>(hdr, w.cnt, w.off, w.clo, w.chi, n_triangles, ew.k, n_entries);
  if (int rc = sort_keys(who, ew.k, ew.s, (size_t)n_entries, (int64_t)1 << 31, ew.temp, ew.tb, st)) return rc;
  head_kernel<<<ge, 256, 0, st>>>(hdr, ew.s, n_entries, ew.head);
  if (int rc = scan_u8(who, ew.head, ew.hpos, (size_t)n_entries, ew.temp, ew.tb, st)) return rc;
  run_kernel<<<ge, 256, 0, st>>>(hdr, ew.head, ew.hpos, n_entries, ew.runs);
  return check_launch(who);
}

// The walk of both candidate entries: keys NULL counts.
static int32_t candidates(const char* who, int64_t n_triangles, int64_t n_vertices, void* ws, int64_t ws_bytes, int64_t n_entries,
                          void* entries_ws, int64_t entries_ws_bytes, int64_t n_large, bool emit, int64_t n_candidates, void* pairs_ws,
                          int64_t pairs_ws_bytes, void* stream) {
  if (!counts_ok(n_vertices, n_triangles) || n_entries < 0 || !entries_ok(n_entries, n_triangles) || n_large < 0 ||
      n_large > n_triangles || (emit && !items_ok(n_candidates)))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: counts out of range", who);
  if (int rc = bind(who, kSizer, ws, ws_bytes, stage_bytes(SLG_ISECT_WS_BOXES, n_triangles, 0))) return rc;
  if (n_entries)
    if (int rc = bind(who, kSizer, entries_ws, entries_ws_bytes, stage_bytes(SLG_ISECT_WS_ENTRIES, n_triangles, n_entries))) return rc;
  if (emit)
    if (int rc = bind(who, kSizer, pairs_ws, pairs_ws_bytes, stage_bytes(SLG_ISECT_WS_PAIRS, n_triangles, n_candidates))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES), be(entries_ws, 0), bp(pairs_ws, 0);
  const BoxWs w = box_ws(b, n_triangles);
  IsectHdr* hdr = (IsectHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  uint64_t* out = nullptr;
  if (emit) {
    const PairWs pw = pair_ws(bp, n_candidates);
    out = pw.keys;
  }
  if (hipMemsetAsync(emit ? (void*)&hdr->cursor : (void*)&hdr->n_cand, 0, 8, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  if (n_entries) {
    const EntryWs ew = entry_ws(be, n_entries);
    const int g = (int)n_entries;                // an upper bound of the runs, which only the device knows
    if (emit) run_pairs_kernel<true><<<g, kTile, 0, st>>>(hdr, ew.s, ew.runs, n_entries, w.box, w.clo, out, n_candidates);
    else run_pairs_kernel<false><<<g, kTile, 0, st>>>(hdr, ew.s, ew.runs, n_entries, w.box, w.clo, out, 0);
  }
  if (n_large) {
    if (emit) large_pairs_kernel<true><<<(int)n_large, 256, 0, st>>>(hdr, w.large, n_triangles, w.box, w.tinfo, out, n_candidates);
    else large_pairs_kernel<false><<<(int)n_large, 256, 0, st>>>(hdr, w.large, n_triangles, w.box, w.tinfo, out, 0);
  }
  return check_launch(who);
}

extern "C" int32_t slg_isect_candidates_count(int64_t n_triangles, int64_t n_vertices, void* ws, int64_t ws_bytes, int64_t n_entries,
                                              void* entries_ws, int64_t entries_ws_bytes, int64_t n_large, void* stream) {
  return candidates("slg_isect_candidates_count", n_triangles, n_vertices, ws, ws_bytes, n_entries, entries_ws, entries_ws_bytes,
                    n_large, false, 0, nullptr, 0, stream);
}

extern "C" int32_t slg_isect_candidates_emit(int64_t n_triangles, int64_t n_vertices, void* ws, int64_t ws_bytes, int64_t n_entries,
                                             void* entries_ws, int64_t entries_ws_bytes, int64_t n_large, int64_t n_candidates,
                                             void* pairs_ws, int64_t pairs_ws_bytes, void* stream) {
  return candidates("slg_isect_candidates_emit", n_triangles, n_vertices, ws, ws_bytes, n_entries, entries_ws, entries_ws_bytes,
                    n_large, true, n_candidates, pairs_ws, pairs_ws_bytes, stream);
}

extern "C" int32_t slg_isect_test(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, void* ws,
                                  int64_t ws_bytes, int64_t n_candidates, void* pairs_ws, int64_t pairs_ws_bytes,
                                  uint8_t* triangle_class_out, void* stream) {
  const char* who = "slg_isect_test";
  if (!vertices || !triangles || !triangle_class_out || !counts_ok(n_vertices, n_triangles) || !items_ok(n_candidates))
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL buffer or counts out of range", who);
  if (int rc = bind(who, kSizer, ws, ws_bytes, stage_bytes(SLG_ISECT_WS_BOXES, n_triangles, 0))) return rc;
  if (int rc = bind(who, kSizer, pairs_ws, pairs_ws_bytes, stage_bytes(SLG_ISECT_WS_PAIRS, n_triangles, n_candidates))) return rc;
  Bump b(ws, SLG_MESH_HDR_BYTES), bp(pairs_ws, 0);
  const BoxWs w = box_ws(b, n_triangles);
  const PairWs pw = pair_ws(bp, n_candidates);
  IsectHdr* hdr = (IsectHdr*)ws;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(hdr->stats, 0, sizeof(hdr->stats), st) != hipSuccess ||
      hipMemsetAsync(w.tword, 0, (size_t)n_triangles * 4, st) != hipSuccess)
    return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  test_kernel<<<grid_of(n_candidates, 256), 256, 0, st>>>(hdr, vertices, triangles, pw.keys, n_candidates, n_triangles, pw.verdict,
                                                          w.tword);
  class_kernel<<<grid_of(n_triangles, 256), 256, 0, st>>>(hdr, w.tword, n_triangles, triangle_class_out);
  return check_launch(who);
}

extern "C" int32_t slg_isect_list(int32_t which, int64_t n_triangles, int64_t n_candidates, void* pairs_ws, int64_t pairs_ws_bytes,
                                  int64_t n_list, void* list_ws, int64_t list_ws_bytes, int32_t* pairs_out, void* stream) {
  const char* who = "slg_isect_list";
  if ((which != SLG_ISECT_INTERSECTING && which != SLG_ISECT_UNCERTAIN) || !pairs_out || n_triangles <= 0 ||
      n_triangles > (1ll << 30) / 3 || !items_ok(n_candidates) || !items_ok(n_list) || n_list > n_candidates)
    return slg_internal_fail(SLG_ERR_INVALID, "%s: a NULL buffer, counts out of range or an unknown list", who);
  if (int rc = bind(who, kSizer, pairs_ws, pairs_ws_bytes, stage_bytes(SLG_ISECT_WS_PAIRS, n_triangles, n_candidates))) return rc;
  if (int rc = bind(who, kSizer, list_ws, list_ws_bytes, stage_bytes(SLG_ISECT_WS_LIST, n_triangles, n_list))) return rc;
  Bump bp(pairs_ws, 0), bl(list_ws, 0);
  const PairWs pw = pair_ws(bp, n_candidates);
  const ListWs lw = slgisect::list_ws(bl, n_list);
  hipStream_t st = (hipStream_t)stream;
  const int gc = grid_of(n_candidates, 256);
  // a place the compaction does not fill (a count that is not the header's) sorts last
  if (hipMemsetAsync(lw.comp, 0xFF, (size_t)n_list * 8, st) != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "%s: memset failed", who);
  flag_kernel<<<gc, 256, 0, st>>>(pw.verdict, n_candidates, which, pw.flag);
  if (int rc = scan_u8(who, pw.flag, pw.pos, (size_t)n_candidates, pw.temp, pw.tb, st)) return rc;
  compact_kernel<<<gc, 256, 0, st>>>(pw.keys, pw.flag, pw.pos, n_candidates, lw.comp, n_list);
  if (int rc = sort_keys(who, lw.comp, lw.sorted, (size_t)n_list, (int64_t)1 << 31, lw.temp, lw.tb, st)) return rc;
  unpack_kernel<<<grid_of(n_list, 256), 256, 0, st>>>(lw.sorted, n_list, pairs_out);
  return check_launch(who);
}
