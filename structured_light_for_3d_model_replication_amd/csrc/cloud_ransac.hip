// cloud_ransac.hip -- the device side of the seeded RANSAC global registration
// (server/processing.py:470-486: registration_ransac_based_on_feature_matching with ransac_n = 3,
// TransformationEstimationPointToPoint(False), the edge-length and distance checkers).  Rules:
// DESIGN.md §13 and tests/feature_ref.py; each is one __device__ function here.
//
// A registration is slg_ransac_prepare (the target's grid, once) and then one slg_ransac_batch per
// batch of trials.  A batch is four launches with no host wait between them: one trial per lane
// (draws from a counter-based hash of (seed, trial, k), the checkers, the estimate), the
// order-preserving compaction of the passing trials, the evaluation of every passing trial over
// the whole source against the shared grid (the hypothesis index in the launch grid), and the
// fold of its sums into one record per passing trial.  The choice among the records is the
// host's: it is sequential in the trial number (cloud.py).
#include "cloud_grid.h"

using namespace slgcloud;

namespace {

constexpr int kRansacGridK = 1;        // the ICP's target grid: 2 points per occupied cell
constexpr int kMaxBatch = 16384;       // trials per slg_ransac_batch (SLG_RANSAC_MAX_BATCH)
constexpr int kTrialStride = 20;       // doubles per trial record (SLG_RANSAC_TRIAL_STRIDE)
constexpr int kRecordStride = 32;      // doubles per evaluation record (SLG_RANSAC_RECORD_STRIDE)
constexpr int kEvalRows = 32;          // hypotheses evaluated side by side (grid.y); the rest by stride
constexpr int kHornSweeps = 6;         // cyclic Jacobi sweeps on Horn's 4x4 (DESIGN.md §13 says why)
constexpr int kFlagEdge = 1, kFlagDistance = 2;
constexpr int kDrawStride = 4;         // draw k of trial t hashes t * 4 + k

struct RansacState {    // 256 bytes behind the target grid's workspace
  int32_t n_pass;       // passing trials of the batch in flight
};
static_assert(sizeof(RansacState) <= 256, "state");

struct RansacWs {
  Ws grid;              // the target's grid; its header carries the status word and far_count
  RansacState* st;
  uint32_t* flags;      // [batch] both checkers passed
  uint32_t* pass;       // [batch] the passing trials' offsets in the batch, ascending
  int32_t* picks;       // [batch][3]
  double* T;            // [batch][12] rows 0..2 of each trial's estimate
  double* part;         // [batch][blocks of kChunk source points][2] n_corr, err2
};

void ransac_layout(Bump& b, int64_t ns, int32_t batch, RansacWs* w) {
  w->st = b.take<RansacState>(1);
  w->flags = b.take<uint32_t>((size_t)batch);
  w->pass = b.take<uint32_t>((size_t)batch);
  w->picks = b.take<int32_t>((size_t)batch * 3);
  w->T = b.take<double>((size_t)batch * 12);
  w->part = b.take<double>((size_t)batch * grid_of(ns, kChunk) * 2);
}

// ---------------------------------------------------------------- the rules (one place each)
// (mix64_rule and draw_rule, which cloud_plane.hip shares, are in cloud_grid.h; a trial here
// reserves kDrawStride draws.)
// CorrespondenceCheckerBasedOnEdgeLength on squares (ours: Open3D compares the lengths).
__device__ inline bool edge_rule(const double* sa, const double* sb, const double* ta, const double* tb, double e2) {
  const double ds2 = d2_rule(sa[0] - sb[0], sa[1] - sb[1], sa[2] - sb[2]);
  const double dt2 = d2_rule(ta[0] - tb[0], ta[1] - tb[1], ta[2] - tb[2]);
  return ds2 >= dt2 * e2 && dt2 >= ds2 * e2;
}

// One Jacobi rotation in the (P, Q) plane of the symmetric 4x4 A (both halves kept); V holds the
// eigenvectors as columns.  The 3x3 rotation of cloud_normals.hip, for any size.
template <int P, int Q>
__device__ __forceinline__ void jacobi4_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  A[P][P] = A[P][P] - t * apq;
  A[Q][Q] = A[Q][Q] + t * apq;
  A[P][Q] = 0.0;
  A[Q][P] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r == P || r == Q) continue;
    const double arp = A[r][P], arq = A[r][Q];
    const double np = c * arp - s * arq, nq = s * arp + c * arq;
    A[r][P] = np; A[P][r] = np;
    A[r][Q] = nq; A[Q][r] = nq;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double vp = V[k][P], vq = V[k][Q];
    V[k][P] = c * vp - s * vq;
    V[k][Q] = s * vp + c * vq;
  }
}

// TransformationEstimationPointToPoint(False) for three pairs: Horn's quaternion.  Centroids
// ((p0 + p1) + p2) / 3; M[i][j] = sum over the pairs of a[i] * b[j], left to right, with a, b the
// centred source and target points; Horn's symmetric 4x4 of M; kHornSweeps sweeps of cyclic Jacobi
// in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); the column of the first largest diagonal entry,
// normalised, is (w, x, y, z); R from the unit quaternion, so it is a proper rotation whatever the
// three points are; t = ct - R cs.  T: rows 0..2 of the 4x4, row-major.
__device__ inline void estimate_rule(const double (*s)[3], const double (*t)[3], double* T) {
  double cs[3], ct[3], M[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cs[a] = ((s[0][a] + s[1][a]) + s[2][a]) / 3.0;
    ct[a] = ((t[0][a] + t[1][a]) + t[2][a]) / 3.0;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      M[i][j] = ((s[0][i] - cs[i]) * (t[0][j] - ct[j]) + (s[1][i] - cs[i]) * (t[1][j] - ct[j])) +
                (s[2][i] - cs[i]) * (t[2][j] - ct[j]);
  }
  double A[4][4], V[4][4];
  A[0][0] = (M[0][0] + M[1][1]) + M[2][2];
  A[1][1] = (M[0][0] - M[1][1]) - M[2][2];
  A[2][2] = (M[1][1] - M[0][0]) - M[2][2];
  A[3][3] = (M[2][2] - M[0][0]) - M[1][1];
  A[0][1] = A[1][0] = M[1][2] - M[2][1];
  A[0][2] = A[2][0] = M[2][0] - M[0][2];
  A[0][3] = A[3][0] = M[0][1] - M[1][0];
  A[1][2] = A[2][1] = M[0][1] + M[1][0];
  A[1][3] = A[3][1] = M[2][0] + M[0][2];
  A[2][3] = A[3][2] = M[1][2] + M[2][1];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  }
#pragma unroll 1
  for (int sweep = 0; sweep < kHornSweeps; ++sweep) {
    jacobi4_rotate<0, 1>(A, V);
    jacobi4_rotate<0, 2>(A, V);
    jacobi4_rotate<0, 3>(A, V);
    jacobi4_rotate<1, 2>(A, V);
    jacobi4_rotate<1, 3>(A, V);
    jacobi4_rotate<2, 3>(A, V);
  }
  // the column of the first largest diagonal entry, as selects (no lookup by index)
  double lam = A[0][0], qw = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
  bool b = A[1][1] > lam;
  lam = b ? A[1][1] : lam; qw = b ? V[0][1] : qw; qx = b ? V[1][1] : qx; qy = b ? V[2][1] : qy; qz = b ? V[3][1] : qz;
  b = A[2][2] > lam;
  lam = b ? A[2][2] : lam; qw = b ? V[0][2] : qw; qx = b ? V[1][2] : qx; qy = b ? V[2][2] : qy; qz = b ? V[3][2] : qz;
  b = A[3][3] > lam;
  qw = b ? V[0][3] : qw; qx = b ? V[1][3] : qx; qy = b ? V[2][3] : qy; qz = b ? V[3][3] : qz;
  const double len = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
  qw = qw / len; qx = qx / len; qy = qy / len; qz = qz / len;
  const double R[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                       2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                       2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    T[4 * a] = R[3 * a];
    T[4 * a + 1] = R[3 * a + 1];
    T[4 * a + 2] = R[3 * a + 2];
    T[4 * a + 3] = ct[a] - ((R[3 * a] * cs[0] + R[3 * a + 1] * cs[1]) + R[3 * a + 2] * cs[2]);
  }
}

// d2(T s - t) of one pair, T being rows 0..2.
__device__ inline double pair_d2_rule(const double* T, const double* s, const double* t) {
  double q[3];
  transform_point_rule(T, s, q);
  return d2_rule(q[0] - t[0], q[1] - t[1], q[2] - t[2]);
}

// ---------------------------------------------------------------- kernels
// One trial per lane.  A trial whose three draws are not distinct fails the edge checker (ours).
__global__ __launch_bounds__(256)
void ransac_trials_kernel(Hdr* hdr, const double* __restrict__ src, int64_t ns, const double* __restrict__ tgt,
                          int64_t nt, const int64_t* __restrict__ pairs, int64_t m, double e2, double dist2,
                          uint64_t seed, int64_t t0, int batch, uint32_t* __restrict__ flags,
                          int32_t* __restrict__ picks, double* __restrict__ Tout, double* __restrict__ trials) {
  if (hdr->status) return;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= batch) return;
  const uint64_t t = (uint64_t)(t0 + g);
  uint32_t c[3];
  double s[3][3], d[3][3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c[k] = draw_rule<kDrawStride>(seed, t, (uint32_t)k, (uint32_t)m);
    const int64_t si = pairs[2 * (size_t)c[k]], ti = pairs[2 * (size_t)c[k] + 1];
    const bool in = si >= 0 && si < ns && ti >= 0 && ti < nt;
    if (!in) atomicOr(&hdr->status, SLG_FILTER_BAD_INDEX);
    ok = ok && in;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s[k][a] = in ? src[3 * si + a] : 0.0;
      d[k][a] = in ? tgt[3 * ti + a] : 0.0;
    }
  }
  const bool distinct = c[0] != c[1] && c[0] != c[2] && c[1] != c[2];
  const bool edge = ok && distinct && edge_rule(s[0], s[1], d[0], d[1], e2) && edge_rule(s[0], s[2], d[0], d[2], e2) &&
                    edge_rule(s[1], s[2], d[1], d[2], e2);
  double T[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  bool near = false;
  if (edge) {
    estimate_rule(s, d, T);
    near = pair_d2_rule(T, s[0], d[0]) <= dist2 && pair_d2_rule(T, s[1], d[1]) <= dist2 &&
           pair_d2_rule(T, s[2], d[2]) <= dist2;
  }
  flags[g] = near ? 1u : 0u;
#pragma unroll
  for (int k = 0; k < 3; ++k) picks[3 * g + k] = (int32_t)c[k];
#pragma unroll
  for (int k = 0; k < 12; ++k) Tout[12 * (size_t)g + k] = T[k];
  if (trials) {
    double* rec = trials + (size_t)g * kTrialStride;
#pragma unroll
    for (int k = 0; k < 3; ++k) rec[k] = (double)c[k];
    rec[3] = (double)((edge ? kFlagEdge : 0) | (near ? kFlagDistance : 0));
#pragma unroll
    for (int k = 0; k < 12; ++k) rec[4 + k] = T[k];
    rec[16] = 0.0; rec[17] = 0.0; rec[18] = 0.0; rec[19] = 1.0;
  }
}

// One workgroup: the passing trials' offsets in ascending order (each thread counts a run of
// consecutive trials, the counts are scanned, each thread writes its run).  At most max_eval of
// them are kept; out[0] = their number, out[1] = the trials the batch has then dealt with: all of
// them, or those up to and including the last one kept, so that the caller's next batch starts
// behind it and no trial is skipped.
__global__ __launch_bounds__(256)
void ransac_compact_kernel(const Hdr* hdr, RansacState* st, const uint32_t* __restrict__ flags, int batch, int max_eval,
                           uint32_t* __restrict__ pass, int32_t* __restrict__ out) {
  __shared__ uint32_t cnt[256];
  if (hdr->status) {                             // uniform: set before this launch
    if (threadIdx.x == 0) { st->n_pass = 0; out[0] = 0; out[1] = batch; }
    return;
  }
  const int t = threadIdx.x;
  const int per = (batch + 255) / 256;
  const int lo = t * per, hi = lo + per < batch ? lo + per : batch;
  uint32_t c = 0;
  for (int g = lo; g < hi; ++g) c += flags[g];
  cnt[t] = c;
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0;
    for (int k = 0; k < 256; ++k) { const uint32_t v = cnt[k]; cnt[k] = run; run += v; }
    const int32_t kept = run < (uint32_t)max_eval ? (int32_t)run : max_eval;
    st->n_pass = kept;
    out[0] = kept;
    out[1] = batch;
  }
  __syncthreads();
  uint32_t o = cnt[t];
  for (int g = lo; g < hi; ++g)
    if (flags[g]) {
      if (o < (uint32_t)max_eval) pass[o] = (uint32_t)g;
      if (o == (uint32_t)max_eval) out[1] = g;     // the first trial left out starts the next batch (after thread 0's write)
      ++o;
    }
}

// The ICP's evaluation (§12) for every passing trial: blockIdx.y strides over the hypotheses,
// blockIdx.x is a chunk of kChunk source points, 8 consecutive points per thread.  Per point
// p' = T p and the radius walk with the best (d2, index) in registers; a query still open after
// kMaxRing rings scans the whole target itself.  n_corr and err2: the thread's points in order,
// the tree over the workgroup, one partial pair per chunk.
__global__ __launch_bounds__(256)
void ransac_eval_kernel(Hdr* hdr, const RansacState* st, const double* __restrict__ src, int64_t ns,
                        const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                        const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ustart, int64_t nt, double r2,
                        const uint32_t* __restrict__ pass, const double* __restrict__ Tin, double* __restrict__ part,
                        int32_t* __restrict__ corr, int corr_cap) {
  __shared__ double sm[256];
  __shared__ int32_t bad;
  if (threadIdx.x == 0) bad = hdr->status;
  __syncthreads();
  if (bad) return;                               // the same answer for every thread of the workgroup
  const int n_pass = st->n_pass;
  const int64_t base = (int64_t)blockIdx.x * kChunk + threadIdx.x * (kChunk / 256);
  for (int h = blockIdx.y; h < n_pass; h += gridDim.y) {
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = Tin[12 * (size_t)pass[h] + k];
    double cnt = 0.0, err = 0.0;
    for (int j = 0; j < kChunk / 256; ++j) {
      const int64_t i = base + j;
      if (i >= ns) break;
      const double p[3] = {src[3 * i], src[3 * i + 1], src[3 * i + 2]};
      Best1 best{1, 0, kInf, kNone};
      if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) {
        atomicOr(&hdr->status, SLG_FILTER_BAD_NONFINITE);
      } else {
        double q[3];
        transform_point_rule(T, p, q);
        if (!ring_walk_at<true, true>(hdr, sxyz, sidx, ukeys, ustart, q, r2, best)) {
          best = Best1{1, 0, kInf, kNone};
          scan_range<true>(best, sxyz, sidx, 0u, (uint32_t)nt, 1u, q, r2);
          atomicAdd(&hdr->n_far, 1);
        }
      }
      if (best.cnt) { cnt += 1.0; err += best.curmax; }
      if (corr && h < corr_cap) corr[(size_t)h * ns + i] = best.cnt ? (int32_t)best.idx : -1;
    }
    const double c = block_tree_sum(cnt, sm);
    __syncthreads();                             // sm[0] has been read before the next sum overwrites it
    const double e = block_tree_sum(err, sm);
    __syncthreads();
    if (threadIdx.x == 0) {
      double* o = part + ((size_t)h * gridDim.x + blockIdx.x) * 2;
      o[0] = c;
      o[1] = e;
    }
  }
}

// One workgroup per passing trial (strided): the tree over the chunks' partials, the count of the
// pairs of C with d2(T s - t) < d * d (integers: order-free), and the record.
__global__ __launch_bounds__(256)
void ransac_records_kernel(const Hdr* hdr, const RansacState* st, const double* __restrict__ src, int64_t ns,
                           const double* __restrict__ tgt, int64_t nt, const int64_t* __restrict__ pairs, int64_t m,
                           double dist2, int64_t t0, const uint32_t* __restrict__ pass, const int32_t* __restrict__ picks,
                           const double* __restrict__ Tin, const double* __restrict__ part, int nb,
                           double* __restrict__ records) {
  __shared__ double sm[256];
  __shared__ unsigned long long ism[256];
  if (hdr->status) return;                       // a non-finite source point, seen by the launch before
  const int n_pass = st->n_pass;
  const int t = threadIdx.x;
  for (int h = blockIdx.x; h < n_pass; h += gridDim.x) {
    const uint32_t g = pass[h];
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = Tin[12 * (size_t)g + k];
    double cnt = 0.0, err = 0.0;
    for (int b = t; b < nb; b += 256) {
      cnt += part[((size_t)h * nb + b) * 2];
      err += part[((size_t)h * nb + b) * 2 + 1];
    }
    const double n_corr = block_tree_sum(cnt, sm);
    __syncthreads();
    const double err2 = block_tree_sum(err, sm);
    __syncthreads();
    unsigned long long in = 0;
    for (int64_t k = t; k < m; k += 256) {
      const int64_t si = pairs[2 * k], ti = pairs[2 * k + 1];
      if (si < 0 || si >= ns || ti < 0 || ti >= nt) continue;   // flagged by the trials kernel when drawn
      const double s[3] = {src[3 * si], src[3 * si + 1], src[3 * si + 2]};
      const double d[3] = {tgt[3 * ti], tgt[3 * ti + 1], tgt[3 * ti + 2]};
      if (pair_d2_rule(T, s, d) < dist2) ++in;
    }
    ism[t] = in;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s) ism[t] += ism[t + s];
      __syncthreads();
    }
    if (t == 0) {
      double* rec = records + (size_t)h * kRecordStride;
      rec[0] = (double)(t0 + g);
      for (int k = 0; k < 3; ++k) rec[1 + k] = (double)picks[3 * g + k];
      for (int k = 0; k < 12; ++k) rec[4 + k] = T[k];
      rec[16] = 0.0; rec[17] = 0.0; rec[18] = 0.0; rec[19] = 1.0;
      rec[20] = n_corr;
      rec[21] = err2;
      rec[22] = n_corr / (double)ns;
      rec[23] = n_corr > 0.0 ? sqrt(err2 / n_corr) : 0.0;
      rec[24] = (double)ism[0];
      for (int k = 25; k < kRecordStride; ++k) rec[k] = 0.0;
    }
    __syncthreads();                             // ism[0] has been read before the next trial's count
  }
}

}  // namespace

static_assert(kMaxBatch == SLG_RANSAC_MAX_BATCH && kTrialStride == SLG_RANSAC_TRIAL_STRIDE &&
              kRecordStride == SLG_RANSAC_RECORD_STRIDE, "slgpu.h");

extern "C" int64_t slg_ransac_ws_bytes(int64_t n_source, int64_t n_target, int32_t batch) {
  if (n_source <= 0 || n_target <= 0 || batch <= 0)
    return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_ransac_ws_bytes: n_source <= 0, n_target <= 0 or batch <= 0");
  if (n_source > kMaxPoints || n_target > kMaxPoints || batch > kMaxBatch)
    return -(int64_t)slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_ransac_ws_bytes: more than 2^30 points or batch > %d",
                                       kMaxBatch);
  RansacWs w;
  return ext_ws_bytes(n_target, kRansacGridK, [&](Bump& b) { ransac_layout(b, n_source, batch, &w); });
}

extern "C" int32_t slg_ransac_prepare(const double* tgt_xyz, int64_t n_target, void* ws, int64_t ws_bytes,
                                      void* stream) {
  if (n_target <= 0 || !tgt_xyz)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_ransac_prepare: n_target <= 0 or a NULL buffer");
  Ws w;
  int rc = begin_call("slg_ransac_prepare", n_target, ws, ws_bytes, &w);
  if (rc) return rc;
  return knn_grid(tgt_xyz, n_target, w, kRansacGridK, (hipStream_t)stream);
}

extern "C" int32_t slg_ransac_batch(const double* src_xyz, int64_t n_source, const double* tgt_xyz, int64_t n_target,
                                    const int64_t* pairs, int64_t n_pairs, int32_t ransac_n, double edge_length,
                                    double max_dist, double confidence, int64_t seed, int64_t first_trial, int32_t batch, void* ws,
                                    int64_t ws_bytes, int32_t max_eval, double* records_out, int32_t* n_eval_out,
                                    double* trials_out, int32_t* corr_out, int32_t corr_cap, void* stream) {
  if (n_source <= 0 || n_target <= 0 || n_pairs <= 0 || batch <= 0 || first_trial < 0 || corr_cap < 0 || max_eval <= 0 ||
      !(max_dist > 0.0) || !isfinite(max_dist) || !(edge_length >= 0.0) || !(edge_length <= 1.0) || !(confidence >= 0.0) || !(confidence <= 1.0) ||
      !src_xyz || !tgt_xyz || !pairs || !records_out || !n_eval_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_ransac_batch: n <= 0, batch <= 0, max_eval <= 0, first_trial < 0, max_dist not finite "
                                              "and > 0, edge_length or confidence outside [0, 1] or a NULL buffer");
  if (ransac_n != 3) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_ransac_batch: ransac_n must be 3");
  if (n_source > kMaxPoints || n_pairs > kMaxPoints || batch > kMaxBatch)
    return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_ransac_batch: more than 2^30 points or pairs, or batch > %d",
                             kMaxBatch);
  RansacWs w;
  int rc = begin_ext_call("slg_ransac_batch", "slg_ransac_ws_bytes", n_target, kRansacGridK, ws, ws_bytes, &w.grid,
                          [&](Bump& b) { ransac_layout(b, n_source, batch, &w); });
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const Ws& g = w.grid;
  const double e2 = edge_length * edge_length, dist2 = max_dist * max_dist;
  const int nb = grid_of(n_source, kChunk);
  ransac_trials_kernel<<<grid_of(batch, 256), 256, 0, st>>>(g.hdr, src_xyz, n_source, tgt_xyz, n_target, pairs, n_pairs, e2,
                                                           dist2, (uint64_t)seed, first_trial, batch, w.flags, w.picks,
                                                           w.T, trials_out);
  ransac_compact_kernel<<<1, 256, 0, st>>>(g.hdr, w.st, w.flags, batch, max_eval, w.pass, n_eval_out);
  ransac_eval_kernel<<<dim3(nb, batch < kEvalRows ? batch : kEvalRows), 256, 0, st>>>(
      g.hdr, w.st, src_xyz, n_source, g.sxyz, g.idx_s, g.ukeys, g.ustart, n_target, dist2, w.pass, w.T, w.part,
      corr_out, corr_cap);
  ransac_records_kernel<<<batch < 256 ? batch : 256, 256, 0, st>>>(g.hdr, w.st, src_xyz, n_source, tgt_xyz, n_target, pairs,
                                                                  n_pairs, dist2, first_trial, w.pass, w.picks, w.T,
                                                                  w.part, nb, records_out);
  return check_launch("slg_ransac_batch");
}
