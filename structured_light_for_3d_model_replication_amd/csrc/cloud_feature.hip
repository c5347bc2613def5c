// cloud_feature.hip -- FPFH features of a device cloud with normals and the brute-force feature
// matching that global registration starts from (server/processing.py:462-466, :477-478:
// compute_fpfh_feature(KDTreeSearchParamHybrid(radius, max_nn)) and the correspondence search of
// registration_ransac_based_on_feature_matching).  Open3D's ComputePairFeatures,
// ComputeSPFHFeature and ComputeFPFHFeature as published, restated (parity with an
// installed Open3D is unpinned); each rule is one __device__ function here and one function of
// tests/feature_ref.py.
//
// The neighbour lists are the hybrid search of cloud_normals.hip with a limit of their own
// (kFpfhMaxK) and with their storage in global memory: both passes read them, so they are
// built once, sorted in place and kept in the workspace, 64 queries to a block of kk x 64 entries
// (entry j of lane l at j * 64 + l, the layout TopKI walks).  The per-thread histograms live in
// LDS columns (bin * 64 + lane), so no kernel indexes a register array by a bin.
#include "cloud_grid.h"

using namespace slgcloud;

namespace {

constexpr int kFpfhMaxK = 128;         // max_nn of slg_fpfh (SLG_FPFH_MAX_NN)
constexpr int kFeat = 33;              // three histograms of 11 bins (SLG_FPFH_DIM)
constexpr int kBins = 11;
constexpr int kFarBlocks = 256;        // workgroups of fpfh_far_kernel, each with kk x 64 entries of scratch
constexpr int kMatchTile = 128;        // target rows staged in LDS per tile (33 KB)
constexpr double kPi = 3.14159265358979323846;

struct FpfhWs {
  Ws grid;
  double* lst_d;        // [blocks of 64][kk][64]  d2 of the list entries, ascending (d2, index)
  uint32_t* lst_i;      // the same shape: their input indices
  int32_t* cnt;         // [n] entries of the list of sorted position q
  double* far_d;        // [kFarBlocks][kk][64] scratch of the whole-cloud kernel
  uint32_t* far_i;
  double* spfh;         // [n][33], by input index
};

void fpfh_layout(Bump& b, int64_t n, int kk, FpfhWs* w) {
  const size_t entries = (size_t)grid_of(n, 64) * kk * 64;
  w->lst_d = b.take<double>(entries);
  w->lst_i = b.take<uint32_t>(entries);
  w->cnt = b.take<int32_t>((size_t)n);
  w->far_d = b.take<double>((size_t)kFarBlocks * kk * 64);
  w->far_i = b.take<uint32_t>((size_t)kFarBlocks * kk * 64);
  w->spfh = b.take<double>((size_t)n * kFeat);
}

// ---------------------------------------------------------------- the rules (one place each)
struct Triple { double theta, alpha, phi; };

// Open3D's ComputePairFeatures for the pair (p1, n1), (p2, n2); every dot product summed x, y, z.
// Ours: the roles swap when |a1| < |a2| (Open3D compares the acos of the two).
__device__ inline Triple pair_rule(const double* p1, const double* n1, const double* p2, const double* n2) {
  Triple r = {0.0, 0.0, 0.0};
  double dx = p2[0] - p1[0], dy = p2[1] - p1[1], dz = p2[2] - p1[2];
  const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
  if (dist == 0.0) return r;
  const double a1 = ((n1[0] * dx + n1[1] * dy) + n1[2] * dz) / dist;
  const double a2 = ((n2[0] * dx + n2[1] * dy) + n2[2] * dz) / dist;
  const bool swap = fabs(a1) < fabs(a2);
  const double ax = swap ? n2[0] : n1[0], ay = swap ? n2[1] : n1[1], az = swap ? n2[2] : n1[2];   // n1 after the swap
  const double bx = swap ? n1[0] : n2[0], by = swap ? n1[1] : n2[1], bz = swap ? n1[2] : n2[2];   // n2 after the swap
  if (swap) { dx = -dx; dy = -dy; dz = -dz; }
  const double phi = swap ? -a2 : a1;
  double vx = dy * az - dz * ay, vy = dz * ax - dx * az, vz = dx * ay - dy * ax;                  // dp x n1
  const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
  if (vn == 0.0) return r;
  vx = vx / vn; vy = vy / vn; vz = vz / vn;
  const double wx = ay * vz - az * vy, wy = az * vx - ax * vz, wz = ax * vy - ay * vx;            // n1 x v
  r.alpha = (vx * bx + vy * by) + vz * bz;
  r.theta = atan2((wx * bx + wy * by) + wz * bz, (ax * bx + ay * by) + az * bz);
  r.phi = phi;
  return r;
}

// The bin of a coordinate already mapped to [0, 11]: floor, clamped to 0..10.
__device__ inline int bin_rule(double c) {
  int h = (int)floor(c);
  h = h < 0 ? 0 : h;
  return h >= kBins ? kBins - 1 : h;
}
__device__ inline double theta_coord_rule(double theta) { return 11.0 * (theta + kPi) / (2.0 * kPi); }
__device__ inline double unit_coord_rule(double v) { return 11.0 * (v + 1.0) * 0.5; }
__device__ inline double spfh_increment_rule(int m) { return 100.0 / (double)(m - 1); }

// ---------------------------------------------------------------- neighbour lists
// The hybrid search's lists: cloud_grid.h's list kernels with the radius and the count.
__global__ __launch_bounds__(64)
void fpfh_lists_kernel(Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                       const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ustart, int64_t n, int kk,
                       double r2, double* lst_d, uint32_t* lst_i, int32_t* __restrict__ cnt,
                       uint32_t* __restrict__ far) {
  lists_body<true>(hdr, sxyz, sidx, ukeys, ustart, n, kk, r2, lst_d, lst_i, cnt, far);
}

__global__ __launch_bounds__(64)
void fpfh_far_kernel(const Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx, int64_t n,
                     int kk, double r2, double* far_d, uint32_t* far_i, double* lst_d, uint32_t* lst_i,
                     int32_t* __restrict__ cnt, const uint32_t* __restrict__ far) {
  lists_far_body<true>(hdr, sxyz, sidx, n, kk, r2, far_d, far_i, lst_d, lst_i, cnt, far);
}

// ---------------------------------------------------------------- SPFH and FPFH
// One point per thread: the pair features against every list entry but the point itself (left out
// by index), each adding 100 / (m - 1) to one bin of each third, in list order.
__global__ __launch_bounds__(64)
void spfh_kernel(const Hdr* hdr, const double* __restrict__ xyz, const double* __restrict__ normals,
                 const uint32_t* __restrict__ sidx, int64_t n, int kk, const uint32_t* __restrict__ lst_i,
                 const int32_t* __restrict__ cnt, double* __restrict__ spfh, int32_t* __restrict__ m_out) {
  __shared__ double hist[kFeat * 64];
  if (hdr->status) return;
  const int lane = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x * 64 + lane;
  if (q >= n) return;
  for (int j = 0; j < kFeat; ++j) hist[j * 64 + lane] = 0.0;
  const uint32_t o = sidx[q];
  const int m = cnt[q];
  if (m > 1) {
    const size_t base = (size_t)blockIdx.x * kk * 64 + lane;
    const double p1[3] = {xyz[3 * (size_t)o], xyz[3 * (size_t)o + 1], xyz[3 * (size_t)o + 2]};
    const double n1[3] = {normals[3 * (size_t)o], normals[3 * (size_t)o + 1], normals[3 * (size_t)o + 2]};
    const double inc = spfh_increment_rule(m);
    for (int j = 0; j < m; ++j) {
      const uint32_t nb = lst_i[base + (size_t)j * 64];
      if (nb == o) continue;
      const double p2[3] = {xyz[3 * (size_t)nb], xyz[3 * (size_t)nb + 1], xyz[3 * (size_t)nb + 2]};
      const double n2[3] = {normals[3 * (size_t)nb], normals[3 * (size_t)nb + 1], normals[3 * (size_t)nb + 2]};
      const Triple t = pair_rule(p1, n1, p2, n2);
      hist[bin_rule(theta_coord_rule(t.theta)) * 64 + lane] += inc;
      hist[(kBins + bin_rule(unit_coord_rule(t.alpha))) * 64 + lane] += inc;
      hist[(2 * kBins + bin_rule(unit_coord_rule(t.phi))) * 64 + lane] += inc;
    }
  }
  for (int j = 0; j < kFeat; ++j) spfh[(size_t)o * kFeat + j] = hist[j * 64 + lane];
  if (m_out) m_out[o] = m;
}

// One point per thread: over the same list in order, skipping entries with d2 == 0, the
// neighbour's SPFH divided by the squared distance, added to the feature and to its third's sum;
// each third scaled by 100 / sum where the sum is not zero; then the point's own SPFH.
__global__ __launch_bounds__(64)
void fpfh_kernel(const Hdr* hdr, const uint32_t* __restrict__ sidx, int64_t n, int kk,
                 const double* __restrict__ lst_d, const uint32_t* __restrict__ lst_i, const int32_t* __restrict__ cnt,
                 const double* __restrict__ spfh, double* __restrict__ fpfh) {
  __shared__ double acc[kFeat * 64];
  if (hdr->status) return;
  const int lane = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x * 64 + lane;
  if (q >= n) return;
  for (int j = 0; j < kFeat; ++j) acc[j * 64 + lane] = 0.0;
  const uint32_t o = sidx[q];
  const int m = cnt[q];
  double sum0 = 0.0, sum1 = 0.0, sum2 = 0.0;
  if (m > 1) {
    const size_t base = (size_t)blockIdx.x * kk * 64 + lane;
    for (int e = 0; e < m; ++e) {
      const double dd = lst_d[base + (size_t)e * 64];
      if (dd == 0.0) continue;
      const double* s = spfh + (size_t)lst_i[base + (size_t)e * 64] * kFeat;
      for (int j = 0; j < kBins; ++j) {
        const double v0 = s[j] / dd, v1 = s[kBins + j] / dd, v2 = s[2 * kBins + j] / dd;
        acc[j * 64 + lane] += v0;
        acc[(kBins + j) * 64 + lane] += v1;
        acc[(2 * kBins + j) * 64 + lane] += v2;
        sum0 += v0; sum1 += v1; sum2 += v2;
      }
    }
  }
  const double sc0 = sum0 != 0.0 ? 100.0 / sum0 : 1.0;
  const double sc1 = sum1 != 0.0 ? 100.0 / sum1 : 1.0;
  const double sc2 = sum2 != 0.0 ? 100.0 / sum2 : 1.0;
  const double* own = spfh + (size_t)o * kFeat;
  for (int j = 0; j < kFeat; ++j) {
    const double sc = j < kBins ? sc0 : (j < 2 * kBins ? sc1 : sc2);
    fpfh[(size_t)o * kFeat + j] = acc[j * 64 + lane] * sc + own[j];      // sc = 1 leaves the zeros alone
  }
}

// ---------------------------------------------------------------- matching
// Squared feature distance of two rows, summed j = 0..32 left to right.
__device__ inline double feature_d2_rule(const double* a, const double* b) {
  double d = 0.0;
#pragma unroll
  for (int j = 0; j < kFeat; ++j) {
    const double x = a[j] - b[j];
    d += x * x;
  }
  return d;
}

// One query row per lane (held in registers), the rows of b staged through LDS kMatchTile at a
// time and read back as broadcasts.  The rows come in ascending index and only a strictly smaller
// distance replaces the best, so the smallest (d2, index) wins.
__global__ __launch_bounds__(256)
void match_kernel(const double* __restrict__ a, int64_t na, const double* __restrict__ b, int64_t nb,
                  int32_t* __restrict__ nn) {
  __shared__ double tile[kMatchTile * kFeat];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + t;
  const bool have = i < na;
  double f[kFeat];
#pragma unroll
  for (int j = 0; j < kFeat; ++j) f[j] = have ? a[(size_t)i * kFeat + j] : 0.0;
  double bestd = kInf;
  int32_t besti = 0;
  for (int64_t tb = 0; tb < nb; tb += kMatchTile) {
    const int m = (int)(nb - tb < kMatchTile ? nb - tb : kMatchTile);
    __syncthreads();                           // the previous tile has been consumed
    for (int w = t; w < m * kFeat; w += 256) tile[w] = b[(size_t)tb * kFeat + w];
    __syncthreads();
    if (!have) continue;
    for (int r = 0; r < m; ++r) {
      const double d = feature_d2_rule(f, tile + r * kFeat);
      if (d < bestd) { bestd = d; besti = (int32_t)(tb + r); }
    }
  }
  if (have) nn[i] = besti;
}

__global__ __launch_bounds__(256)
void match_flags_kernel(const int32_t* __restrict__ nn_s, int64_t ns, const int32_t* __restrict__ nn_t, int mutual,
                        uint32_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ns) return;
  flags[i] = (!mutual || nn_t[nn_s[i]] == (int32_t)i) ? 1u : 0u;
}

// pos = exclusive scan of flags: the kept pairs in source order.
__global__ __launch_bounds__(256)
void match_pairs_kernel(const int32_t* __restrict__ nn_s, int64_t ns, const uint32_t* __restrict__ flags,
                        const uint32_t* __restrict__ pos, int64_t* __restrict__ pairs, int64_t* __restrict__ m_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ns) return;
  if (flags[i]) {
    pairs[2 * (size_t)pos[i]] = i;
    pairs[2 * (size_t)pos[i] + 1] = nn_s[i];
  }
  if (i == ns - 1) *m_out = (int64_t)pos[i] + flags[i];
}

void match_layout(Bump& b, int64_t ns, int64_t nt, int32_t** nn_s, int32_t** nn_t) {
  *nn_s = b.take<int32_t>((size_t)ns);
  *nn_t = b.take<int32_t>((size_t)nt);
}

}  // namespace

static_assert(kFpfhMaxK == SLG_FPFH_MAX_NN && kFeat == SLG_FPFH_DIM, "slgpu.h");

extern "C" int64_t slg_fpfh_ws_bytes(int64_t n, int32_t max_nn) {
  if (n <= 0 || max_nn < 2)
    return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_fpfh_ws_bytes: n <= 0 or max_nn < 2");
  if (n > kMaxPoints || max_nn > kFpfhMaxK)
    return -(int64_t)slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_fpfh_ws_bytes: more than 2^30 points or max_nn > %d",
                                       kFpfhMaxK);
  FpfhWs w;
  return ext_ws_bytes(n, 0, [&](Bump& b) { fpfh_layout(b, n, (int)(n < max_nn ? n : max_nn), &w); });
}

extern "C" int32_t slg_fpfh(const double* xyz, const double* normals, int64_t n, double radius, int32_t max_nn,
                            void* ws, int64_t ws_bytes, double* fpfh_out, double* spfh_out, int32_t* m_out,
                            void* stream) {
  if (n <= 0 || !(radius > 0.0) || !isfinite(radius) || max_nn < 2 || !xyz || !normals || !fpfh_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_fpfh: n <= 0, radius not finite and > 0, max_nn < 2 or a NULL buffer "
                                              "(the cloud needs normals)");
  if (max_nn > kFpfhMaxK) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_fpfh: max_nn > %d", kFpfhMaxK);
  // begin_call's own refusal, kept ahead of the grid's size query (which would name slg_filter_ws_bytes)
  if (n > kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_fpfh: more than 2^30 points");
  FpfhWs w;
  const int kk = (int)(n < max_nn ? n : max_nn);
  int rc = begin_ext_call("slg_fpfh", "slg_fpfh_ws_bytes", n, 0, ws, ws_bytes, &w.grid,
                          [&](Bump& b) { fpfh_layout(b, n, kk, &w); });
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = knn_grid(xyz, n, w.grid, max_nn, st))) return rc;
  const Ws& g = w.grid;
  const double r2 = radius * radius;
  const int nb = grid_of(n, 64);
  double* spfh = spfh_out ? spfh_out : w.spfh;
  fpfh_lists_kernel<<<nb, 64, 0, st>>>(g.hdr, g.sxyz, g.idx_s, g.ukeys, g.ustart, n, kk, r2, w.lst_d, w.lst_i, w.cnt, g.far);
  fpfh_far_kernel<<<(int)(n < kFarBlocks ? n : kFarBlocks), 64, 0, st>>>(g.hdr, g.sxyz, g.idx_s, n, kk, r2, w.far_d,
                                                                        w.far_i, w.lst_d, w.lst_i, w.cnt, g.far);
  spfh_kernel<<<nb, 64, 0, st>>>(g.hdr, xyz, normals, g.idx_s, n, kk, w.lst_i, w.cnt, spfh, m_out);
  fpfh_kernel<<<nb, 64, 0, st>>>(g.hdr, g.idx_s, n, kk, w.lst_d, w.lst_i, w.cnt, spfh, fpfh_out);
  return check_launch("slg_fpfh");
}

extern "C" int64_t slg_feature_match_ws_bytes(int64_t n_source, int64_t n_target) {
  if (n_source <= 0 || n_target <= 0)
    return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_feature_match_ws_bytes: n_source <= 0 or n_target <= 0");
  if (n_source > kMaxPoints || n_target > kMaxPoints)
    return -(int64_t)slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_feature_match_ws_bytes: more than 2^30 rows");
  int32_t *nn_s, *nn_t;
  return ext_ws_bytes(n_source, 0, [&](Bump& b) { match_layout(b, n_source, n_target, &nn_s, &nn_t); });
}

extern "C" int32_t slg_feature_match(const double* source_feature, int64_t n_source, const double* target_feature,
                                     int64_t n_target, int32_t mutual_filter, void* ws, int64_t ws_bytes,
                                     int32_t* nn_source_out, int32_t* nn_target_out, int64_t* pairs_out, int64_t* m_out,
                                     void* stream) {
  if (n_source <= 0 || n_target <= 0 || !source_feature || !target_feature || !pairs_out || !m_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_feature_match: n_source <= 0, n_target <= 0 or a NULL buffer");
  if (n_target > kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_feature_match: more than 2^30 rows");
  // begin_call's own refusal, kept ahead of the grid's size query (which would name slg_filter_ws_bytes)
  if (n_source > kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_feature_match: more than 2^30 points");
  Ws w;
  int32_t *nn_s, *nn_t;
  int rc = begin_ext_call("slg_feature_match", "slg_feature_match_ws_bytes", n_source, 0, ws, ws_bytes, &w,
                          [&](Bump& b) { match_layout(b, n_source, n_target, &nn_s, &nn_t); });
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (nn_source_out) nn_s = nn_source_out;
  if (nn_target_out) nn_t = nn_target_out;
  const int gs = grid_of(n_source, 256);
  match_kernel<<<gs, 256, 0, st>>>(source_feature, n_source, target_feature, n_target, nn_s);
  if (mutual_filter)
    match_kernel<<<grid_of(n_target, 256), 256, 0, st>>>(target_feature, n_target, source_feature, n_source, nn_t);
  match_flags_kernel<<<gs, 256, 0, st>>>(nn_s, n_source, nn_t, mutual_filter ? 1 : 0, w.idx);
  if ((rc = scan_u32("slg_feature_match", w, w.idx, w.pos, n_source, st))) return rc;
  match_pairs_kernel<<<gs, 256, 0, st>>>(nn_s, n_source, w.idx, w.pos, pairs_out, m_out);
  return check_launch("slg_feature_match");
}
