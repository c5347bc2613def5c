// cloud_icp.hip -- point-to-plane ICP, rigid transform and what the 360-degree merge's loop body
// needs beside them (server/processing.py:549-603: registration_icp with
// TransformationEstimationPointToPlane, PointCloud.transform), on the device cloud.  Open3D's
// published rules restated (parity with an installed Open3D is unpinned); each
// rule is one __device__ function here and one function of tests/icp_ref.py.  The 1-NN search is
// the ring walk of cloud_grid.h over the kNN grid of the target; the sums are the fixed tree of
// the statistical filter, so the same input gives the same bits.
//
// A registration is max_iteration + 1 evaluations (correspondences, far list, sums, solve), all
// enqueued at once on the caller's stream.  Nothing synchronises with the host: the solve kernel
// sets a `done` word in the ICP state once the loop has stopped, and every kernel of the
// evaluations still queued reads it and returns.
#include "cloud_grid.h"

using namespace slgcloud;

namespace {

constexpr int kIcpGridK = 1;           // sizes the target grid's cells: knn_target(1) = 2 points per occupied cell
constexpr int kTerms = 29;             // 21 of JTJ's upper triangle, 6 of JTr, n_corr, err2
constexpr int kLogStride = 56;         // doubles per log record (SLG_ICP_LOG_STRIDE)
constexpr int kResultLen = 24;         // doubles of result_out (SLG_ICP_RESULT_LEN)
constexpr int kMaxIterations = 1000;   // every iteration is enqueued up front

struct Mat4 { double m[16]; };         // row-major, by value in kernel arguments

struct IcpState {       // 256 bytes behind the target grid's workspace
  double T[16];         // the accumulated transform the next evaluation uses
  double prev_fitness, prev_rmse;
  int32_t done;         // the loop has stopped: every later kernel of the call returns
  int32_t n_far;        // this evaluation's far list
};
static_assert(sizeof(IcpState) <= 256, "state");

struct IcpWs {
  Ws grid;              // the target's kNN grid; its header carries the status word and far_count
  IcpState* st;
  double* part;
  int32_t* corr;
  uint32_t* far;
  double* log;
};

// The regions behind the target grid's workspace.
void icp_layout(Bump& b, int64_t ns, int32_t max_iteration, IcpWs* w) {
  w->st = b.take<IcpState>(1);
  w->part = b.take<double>((size_t)grid_of(ns, kChunk) * kTerms);
  w->corr = b.take<int32_t>((size_t)ns);
  w->far = b.take<uint32_t>((size_t)ns);
  w->log = b.take<double>(((size_t)max_iteration + 1) * kLogStride);
}

// ---------------------------------------------------------------- the rules (one place each)
// (transform_point_rule and Best1, which cloud_ransac.hip shares, are in cloud_grid.h.)
// Normals: the 3x3 block, no translation.
template <class M>
__device__ inline void transform_normal_rule(const M& T, const double* v, double* o) {
#pragma unroll
  for (int a = 0; a < 3; ++a) o[a] = (T[4 * a] * v[0] + T[4 * a + 1] * v[1]) + T[4 * a + 2] * v[2];
}

// Index of entry (a, b), a <= b, of a 6x6 upper triangle stored row by row.
__host__ __device__ constexpr int ut(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }

// One correspondence's 29 terms added to acc: s the transformed source point, t and n the
// target's point and normal.  r = ((s - t) . n) summed x, y, z; J = [s x n, n].
__device__ inline void terms_rule(const double* s, const double* t, const double* n, double* acc) {
  const double dx = s[0] - t[0], dy = s[1] - t[1], dz = s[2] - t[2];
  const double r = (dx * n[0] + dy * n[1]) + dz * n[2];
  const double J[6] = {s[1] * n[2] - s[2] * n[1], s[2] * n[0] - s[0] * n[2], s[0] * n[1] - s[1] * n[0],
                       n[0], n[1], n[2]};
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int b = a; b < 6; ++b) acc[ut(a, b)] += J[a] * J[b];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * r;
  acc[27] += 1.0;
  acc[28] += d2_rule(t[0] - s[0], t[1] - s[1], t[2] - s[2]);
}

// JTJ x = -JTr by LDL' without pivoting, in this operation order (tests/icp_ref.py:ldlt_solve
// repeats it).  S: the 27 sums.  False (x = 0) when a pivot is <= 0 or not finite.
__device__ inline bool ldlt_solve_rule(const double* S, double* x) {
  double L[6][6], D[6], y[6];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = S[ut(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) d = d - (L[j][k] * L[j][k]) * D[k];
    ok = ok && d > 0.0 && isfinite(d);
    D[j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = S[ut(j, i)];
#pragma unroll
      for (int k = 0; k < j; ++k) v = v - (L[i][k] * L[j][k]) * D[k];
      L[i][j] = v / d;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {              // L y = -JTr
    double v = -S[21 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
    y[i] = v;
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {             // L' x = y / D
    double v = y[i] / D[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * x[k];
    x[i] = v;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = ok ? x[i] : 0.0;
  return ok;
}

// TransformVector6dToMatrix4d and T <- U T: R = Rz(x[2]) Ry(x[1]) Rx(x[0]) multiplied out,
// t = x[3:6]; each entry of the product summed left to right; the last row stays 0 0 0 1.
__device__ inline void update_rule(const double* x, double* T) {
  const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
  const double U[12] = {cg * cb, (cg * sb) * sa - sg * ca, (cg * sb) * ca + sg * sa, x[3],
                        sg * cb, (sg * sb) * sa + cg * ca, (sg * sb) * ca - cg * sa, x[4],
                        -sb,     cb * sa,                  cb * ca,                  x[5]};
  double o[12];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 4; ++b)
      o[4 * a + b] = ((U[4 * a] * T[b] + U[4 * a + 1] * T[4 + b]) + U[4 * a + 2] * T[8 + b]) + U[4 * a + 3] * T[12 + b];
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = o[k];
}

__device__ inline bool stop_rule(double fitness, double prev_fitness, double rmse, double prev_rmse, double rel_fitness,
                                 double rel_rmse) {
  return fabs(fitness - prev_fitness) < rel_fitness && fabs(rmse - prev_rmse) < rel_rmse;
}

// ---------------------------------------------------------------- fixed-order tree over kTerms sums
// block_tree_sum (cloud_grid.h) for kTerms values at once: the same additions per value.
__device__ inline void block_tree_sum_terms(const double* v, double (*sm)[256]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < kTerms; ++k) sm[k][t] = v[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < kTerms; ++k) sm[k][t] = sm[k][t] + sm[k][t + s];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- kernels
__global__ void icp_init_kernel(IcpState* st, Mat4 T) {
#pragma unroll
  for (int k = 0; k < 16; ++k) st->T[k] = T.m[k];
  st->prev_fitness = 0.0;
  st->prev_rmse = 0.0;
  st->done = 0;
  st->n_far = 0;
}

// One source point per lane, in input order: p' = T p, then the radius walk with the best
// (d2, index) in registers.  A query still open after kMaxRing rings goes to the far list.
__global__ __launch_bounds__(256)
void icp_corr_kernel(Hdr* hdr, IcpState* st, const double* __restrict__ src, int64_t ns,
                     const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                     const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ustart, double r2,
                     int32_t* __restrict__ corr, uint32_t* __restrict__ far) {
  if (hdr->status || st->done) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ns) return;
  const double p[3] = {src[3 * i], src[3 * i + 1], src[3 * i + 2]};
  if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) {
    atomicOr(&hdr->status, SLG_FILTER_BAD_NONFINITE);
    return;
  }
  double q[3];
  transform_point_rule(st->T, p, q);
  Best1 best{1, 0, kInf, kNone};
  if (!ring_walk_at<true, true>(hdr, sxyz, sidx, ukeys, ustart, q, r2, best)) {
    far[atomicAdd(&st->n_far, 1)] = (uint32_t)i;      // list order is free: each entry is independent
    return;
  }
  corr[i] = best.cnt ? (int32_t)best.idx : -1;
}

// One wave per listed query over the whole target: each lane keeps the best of its stride, then
// the wave reduces the (d2, index) pairs.
__global__ __launch_bounds__(64)
void icp_far_kernel(const Hdr* hdr, const IcpState* st, const double* __restrict__ src,
                    const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx, int64_t nt, double r2,
                    int32_t* __restrict__ corr, const uint32_t* __restrict__ far) {
  if (hdr->status || st->done) return;
  const int lane = threadIdx.x;
  const int nf = st->n_far;
  for (int f = blockIdx.x; f < nf; f += gridDim.x) {
    const int64_t i = far[f];
    const double p[3] = {src[3 * i], src[3 * i + 1], src[3 * i + 2]};
    double q[3];
    transform_point_rule(st->T, p, q);
    Best1 best{1, 0, kInf, kNone};
    scan_range<true>(best, sxyz, sidx, (uint32_t)lane, (uint32_t)nt, 64, q, r2);
    double d = best.curmax;
    uint32_t id = best.idx;
    for (int s = 32; s > 0; s >>= 1) {
      const double od = __shfl_xor(d, s, 64);
      const uint32_t oi = (uint32_t)__shfl_xor((int)id, s, 64);
      if (pair_before_rule(od, oi, d, id)) { d = od; id = oi; }
    }
    if (lane == 0) corr[i] = id != kNone ? (int32_t)id : -1;
  }
}

// The 29 terms of every source point from corr[i] (zeros without a correspondence; without target
// normals the normal is taken as zero, which leaves n_corr and err2), summed over the input
// order: 8 consecutive points per thread, the tree over the workgroup, one partial set per kChunk
// points.
__global__ __launch_bounds__(256)
void icp_sums_kernel(const Hdr* hdr, const IcpState* st, const double* __restrict__ src, int64_t ns,
                     const double* __restrict__ tgt, const double* __restrict__ nrm, int64_t nt,
                     const int32_t* __restrict__ corr, double* __restrict__ part) {
  __shared__ double sm[kTerms][256];
  if (hdr->status || st->done) return;
  double acc[kTerms];
#pragma unroll
  for (int k = 0; k < kTerms; ++k) acc[k] = 0.0;
  const int64_t base = (int64_t)blockIdx.x * kChunk + threadIdx.x * (kChunk / 256);
  for (int j = 0; j < kChunk / 256; ++j) {
    const int64_t i = base + j;
    if (i >= ns) break;
    const int64_t c = corr[i];
    if (c < 0 || c >= nt) continue;
    const double p[3] = {src[3 * i], src[3 * i + 1], src[3 * i + 2]};
    double s[3];
    transform_point_rule(st->T, p, s);
    const double t[3] = {tgt[3 * c], tgt[3 * c + 1], tgt[3 * c + 2]};
    double n[3] = {0.0, 0.0, 0.0};
    if (nrm) { n[0] = nrm[3 * c]; n[1] = nrm[3 * c + 1]; n[2] = nrm[3 * c + 2]; }
    terms_rule(s, t, n, acc);
  }
  block_tree_sum_terms(acc, sm);
  if (threadIdx.x < kTerms) part[(int64_t)blockIdx.x * kTerms + threadIdx.x] = sm[threadIdx.x][0];
}

// One workgroup: the tree over the partials, then in one lane this evaluation's fitness and rmse,
// the stop test, the result, the log record, and (unless the loop ends here) the solve and
// T <- U T.  step = the number of updates made before this evaluation.
__global__ __launch_bounds__(256)
void icp_solve_kernel(Hdr* hdr, IcpState* st, const double* __restrict__ part, int nb, int64_t ns, int step,
                      int max_iteration, double rel_fitness, double rel_rmse, int have_normals,
                      double* __restrict__ result, double* __restrict__ log) {
  __shared__ double sm[kTerms][256];
  if (hdr->status || st->done) return;
  double acc[kTerms];
#pragma unroll
  for (int k = 0; k < kTerms; ++k) acc[k] = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) {
#pragma unroll
    for (int k = 0; k < kTerms; ++k) acc[k] += part[(int64_t)b * kTerms + k];
  }
  block_tree_sum_terms(acc, sm);
  if (threadIdx.x != 0) return;
  double S[kTerms];
#pragma unroll
  for (int k = 0; k < kTerms; ++k) S[k] = sm[k][0];
  const double n_corr = S[27], err2 = S[28];
  const double fitness = n_corr / (double)ns;
  const double rmse = n_corr > 0.0 ? sqrt(err2 / n_corr) : 0.0;
  const bool stop = step > 0 && stop_rule(fitness, st->prev_fitness, rmse, st->prev_rmse, rel_fitness, rel_rmse);
  const bool last = stop || step == max_iteration;
  st->prev_fitness = fitness;
  st->prev_rmse = rmse;
  hdr->n_far += st->n_far;                   // byte 8 of the workspace: the call's total
  st->n_far = 0;
  double T[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) T[k] = st->T[k];
  double* rec = log + (size_t)step * kLogStride;
#pragma unroll
  for (int k = 0; k < 16; ++k) { result[k] = T[k]; rec[k] = T[k]; }   // the T this evaluation was made at
  result[16] = fitness;
  result[17] = rmse;
  result[18] = n_corr;
  result[19] = (double)step;
  result[20] = stop ? 1.0 : 0.0;
  result[21] = 0.0;                          // reserved: written, so result_out needs no clearing by the caller
  result[22] = 0.0;
  result[23] = 0.0;
  double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int flags = (stop ? SLG_ICP_LOG_STOP : 0) | (last && !stop ? SLG_ICP_LOG_LAST : 0);
  if (last) {
    st->done = 1;
  } else {
    const bool ok = have_normals && n_corr > 0.0 && ldlt_solve_rule(S, x);
    if (ok) {
      update_rule(x, T);
#pragma unroll
      for (int k = 0; k < 12; ++k) st->T[k] = T[k];
    } else {
#pragma unroll
      for (int k = 0; k < 6; ++k) x[k] = 0.0;
    }
    flags |= ok ? SLG_ICP_LOG_SOLVED : SLG_ICP_LOG_SINGULAR;
  }
  rec[16] = n_corr;
  rec[17] = err2;
  rec[18] = fitness;
  rec[19] = rmse;
#pragma unroll
  for (int k = 0; k < 27; ++k) rec[20 + k] = S[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) rec[47 + k] = x[k];
  rec[53] = (double)flags;
  rec[54] = 0.0;
  rec[55] = 0.0;
}

__global__ __launch_bounds__(256)
void transform_kernel(const double* xyz, const double* normals, int64_t n, Mat4 T, double* xyz_out,
                      double* normals_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  double o[3];
  transform_point_rule(T.m, p, o);
  for (int a = 0; a < 3; ++a) xyz_out[3 * i + a] = o[a];
  if (normals) {
    const double v[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
    transform_normal_rule(T.m, v, o);
    for (int a = 0; a < 3; ++a) normals_out[3 * i + a] = o[a];
  }
}

// A rigid or affine 4x4: every entry finite, the last row exactly 0 0 0 1.
bool matrix_ok(const double* T) {
  for (int k = 0; k < 16; ++k)
    if (!isfinite(T[k])) return false;
  return T[12] == 0.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 1.0;
}

}  // namespace

static_assert(kLogStride == SLG_ICP_LOG_STRIDE && kResultLen == SLG_ICP_RESULT_LEN, "slgpu.h");

extern "C" int64_t slg_icp_ws_bytes(int64_t n_source, int64_t n_target, int32_t max_iteration) {
  if (n_source <= 0 || n_target <= 0 || max_iteration < 0)
    return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_icp_ws_bytes: n_source <= 0, n_target <= 0 or max_iteration < 0");
  if (n_source > kMaxPoints || n_target > kMaxPoints || max_iteration > kMaxIterations)
    return -(int64_t)slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_icp_ws_bytes: more than 2^30 points or max_iteration > %d",
                                       kMaxIterations);
  IcpWs w;
  return ext_ws_bytes(n_target, kIcpGridK, [&](Bump& b) { icp_layout(b, n_source, max_iteration, &w); });
}

extern "C" int32_t slg_icp_point_to_plane(const double* src_xyz, int64_t n_source, const double* tgt_xyz,
                                          const double* tgt_normals, int64_t n_target, double max_dist,
                                          const double* init_T, double rel_fitness, double rel_rmse,
                                          int32_t max_iteration, void* ws, int64_t ws_bytes, double* result_out,
                                          int32_t* corr_out, double* log_out, void* stream) {
  if (n_source <= 0 || n_target <= 0 || !(max_dist > 0.0) || max_iteration < 0 || !(rel_fitness >= 0.0) ||
      !(rel_rmse >= 0.0) || !src_xyz || !tgt_xyz || !init_T || !result_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_icp_point_to_plane: n <= 0, max_dist <= 0 or NaN, max_iteration < 0, "
                                              "a negative or NaN criterion, or a NULL buffer");
  if (!matrix_ok(init_T))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_icp_point_to_plane: init_T needs finite entries and a last row of 0 0 0 1");
  if (n_source > kMaxPoints || max_iteration > kMaxIterations)
    return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_icp_point_to_plane: more than 2^30 points or max_iteration > %d",
                             kMaxIterations);
  IcpWs w;
  int rc = begin_ext_call("slg_icp_point_to_plane", "slg_icp_ws_bytes", n_target, kIcpGridK, ws, ws_bytes, &w.grid,
                          [&](Bump& b) { icp_layout(b, n_source, max_iteration, &w); });
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  Mat4 T;
  for (int k = 0; k < 16; ++k) T.m[k] = init_T[k];
  icp_init_kernel<<<1, 1, 0, st>>>(w.st, T);
  if ((rc = knn_grid(tgt_xyz, n_target, w.grid, kIcpGridK, st))) return rc;
  int32_t* corr = corr_out ? corr_out : w.corr;
  double* log = log_out ? log_out : w.log;
  const double r2 = max_dist * max_dist;
  const int nb = grid_of(n_source, kChunk);
  for (int step = 0; step <= max_iteration; ++step) {
    icp_corr_kernel<<<grid_of(n_source, 256), 256, 0, st>>>(w.grid.hdr, w.st, src_xyz, n_source, w.grid.sxyz, w.grid.idx_s,
                                                           w.grid.ukeys, w.grid.ustart, r2, corr, w.far);
    icp_far_kernel<<<(int)(n_source < 1024 ? n_source : 1024), 64, 0, st>>>(w.grid.hdr, w.st, src_xyz, w.grid.sxyz,
                                                                           w.grid.idx_s, n_target, r2, corr, w.far);
    icp_sums_kernel<<<nb, 256, 0, st>>>(w.grid.hdr, w.st, src_xyz, n_source, tgt_xyz, tgt_normals, n_target, corr, w.part);
    icp_solve_kernel<<<1, 256, 0, st>>>(w.grid.hdr, w.st, w.part, nb, n_source, step, max_iteration, rel_fitness, rel_rmse,
                                        tgt_normals ? 1 : 0, result_out, log);
  }
  return check_launch("slg_icp_point_to_plane");
}

extern "C" int32_t slg_cloud_transform(const double* xyz, const double* normals, int64_t n, const double* T,
                                       double* xyz_out, double* normals_out, void* stream) {
  if (n <= 0 || !xyz || !xyz_out || !T || (normals && !normals_out))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_cloud_transform: n <= 0 or a NULL buffer");
  if (!matrix_ok(T))
    return slg_internal_fail(SLG_ERR_INVALID, "slg_cloud_transform: T needs finite entries and a last row of 0 0 0 1");
  if (n > kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_cloud_transform: more than 2^30 points");
  Mat4 M;
  for (int k = 0; k < 16; ++k) M.m[k] = T[k];
  transform_kernel<<<grid_of(n, 256), 256, 0, (hipStream_t)stream>>>(xyz, normals, n, M, xyz_out, normals_out);
  return check_launch("transform_kernel");
}
