// cloud_plane.hip -- seeded RANSAC plane segmentation on the device cloud
// (ProcessingLogic.remove_background, server/processing.py:337-364: Open3D segment_plane, then
// select_by_index(inliers, invert=True)).  Rules: DESIGN.md §14 and tests/plane_ref.py; each is
// one __device__ function here.
//
// A segmentation is one slg_plane_batch per batch of trials and one slg_plane_finish.  A batch is
// three launches with no host wait between them: one trial per lane (draws from the counter-based
// hash of (seed, trial, k), the model), the evaluation of every trial of the batch over the whole
// cloud (one plane per lane, one chunk of kChunk points per workgroup, staged in LDS and read back
// as broadcasts in index order, so each lane holds its chunk's count and err with no cross-lane
// step), and one wave per trial whose first lane sums the chunks' partials in chunk order into the
// record.
// The choice among the records is the host's: it is sequential in the trial number (cloud.py).
// The finish takes the winning plane: inlier flags, their scan, the ascending indices, and the
// refit over the inliers by the fixed tree of cloud_grid.h.
#include "cloud_grid.h"

using namespace slgcloud;

namespace {

constexpr int kMaxBatch = 4096;        // trials per slg_plane_batch (SLG_PLANE_MAX_BATCH)
constexpr int kRecordStride = 16;      // doubles per record (SLG_PLANE_RECORD_STRIDE)
constexpr int kSumsLen = 16;           // doubles of slg_plane_finish's sums_out (SLG_PLANE_SUMS_LEN)
constexpr int kMinN = 3, kMaxN = 8;    // ransac_n (SLG_PLANE_MAX_RANSAC_N)
constexpr int kEvalTile = 1024;        // points plane_eval_kernel stages in LDS at a time (24 KB)
constexpr int kRecordsTile = 1024;     // chunk partials plane_records_kernel stages in LDS at a time

struct PlaneWs {
  Ws grid;              // the filter workspace: the status word, the scan's scratch, flags, pos, part
  double* planes;       // [batch][4]
  uint32_t* valid;      // [batch]
  int32_t* cnt;         // [batch][chunks]
  double* err;          // [batch][chunks]
};

void plane_layout(Bump& b, int64_t n, int32_t batch, PlaneWs* w) {
  const size_t nb = (size_t)grid_of(n, kChunk);
  w->planes = b.take<double>((size_t)batch * 4);
  w->valid = b.take<uint32_t>((size_t)batch);
  w->cnt = b.take<int32_t>(nb * (size_t)batch);
  w->err = b.take<double>(nb * (size_t)batch);
}

// ---------------------------------------------------------------- the rules (one place each)
// (mix64_rule and draw_rule, which cloud_ransac.hip shares, are in cloud_grid.h; a trial here
// reserves kMaxN draws: draw k of trial t hashes t * 8 + k.)
// abc / norm and d from a point of the plane; false (the zero plane) when the norm is zero.
__device__ inline bool plane_normalise_rule(double x, double y, double z, const double* at, double* pl) {
  const double norm = sqrt((x * x + y * y) + z * z);
  const bool ok = !(norm == 0.0);
  pl[0] = ok ? x / norm : 0.0;
  pl[1] = ok ? y / norm : 0.0;
  pl[2] = ok ? z / norm : 0.0;
  pl[3] = ok ? -((pl[0] * at[0] + pl[1] * at[1]) + pl[2] * at[2]) : 0.0;
  return ok;
}

// ComputeTrianglePlane.
__device__ inline bool triangle_plane_rule(const double* p0, const double* p1, const double* p2, double* pl) {
  const double e0[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  const double e1[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  return plane_normalise_rule(e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2],
                              e0[0] * e1[1] - e0[1] * e1[0], p0, pl);
}

// GetPlaneFromPoints from the centroid and the six centred sums S = xx xy xz yy yz zz.
__device__ inline bool plane_from_sums_rule(const double* c, const double* S, double* pl) {
  const double xx = S[0], xy = S[1], xz = S[2], yy = S[3], yz = S[4], zz = S[5];
  const double det_x = yy * zz - yz * yz, det_y = xx * zz - xz * xz, det_z = xx * yy - xy * xy;
  double a, b, d;
  if (det_x > det_y && det_x > det_z) {
    a = det_x; b = xz * yz - xy * zz; d = xy * yz - xz * yy;
  } else if (det_y > det_z) {
    a = xz * yz - xy * zz; b = det_y; d = xy * xz - yz * xx;
  } else {
    a = xy * yz - xz * yy; b = xy * xz - yz * xx; d = det_z;
  }
  return plane_normalise_rule(a, b, d, c, pl);
}

__device__ inline double plane_distance_rule(double a, double b, double c, double d, double x, double y, double z) {
  return fabs(((a * x + b * y) + c * z) + d);
}
__device__ inline bool plane_inlier_rule(double dist, double thr) { return dist < thr; }

// ---------------------------------------------------------------- kernels
// One trial per lane.  A trial with two equal draws, or a zero norm, is invalid: the zero plane.
__global__ __launch_bounds__(256)
void plane_trials_kernel(const double* __restrict__ xyz, int64_t n, int rn, uint64_t seed, int64_t t0, int batch,
                         double* __restrict__ planes, uint32_t* __restrict__ valid) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= batch) return;
  const uint64_t t = (uint64_t)(t0 + g);
  uint32_t c[kMaxN];
  double p[kMaxN][3];
  bool distinct = true;
#pragma unroll
  for (int k = 0; k < kMaxN; ++k) {
    const bool use = k < rn;
    c[k] = use ? draw_rule<kMaxN>(seed, t, (uint32_t)k, (uint32_t)n) : 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a) p[k][a] = use ? xyz[3 * (size_t)c[k] + a] : 0.0;
#pragma unroll
    for (int j = 0; j < k; ++j) distinct = distinct && !(use && c[j] == c[k]);
  }
  double pl[4];
  bool ok;
  if (rn == 3) {
    ok = triangle_plane_rule(p[0], p[1], p[2], pl);
  } else {
    double cen[3] = {0.0, 0.0, 0.0}, S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kMaxN; ++k)
      if (k < rn) { cen[0] += p[k][0]; cen[1] += p[k][1]; cen[2] += p[k][2]; }
#pragma unroll
    for (int a = 0; a < 3; ++a) cen[a] = cen[a] / (double)rn;
#pragma unroll
    for (int k = 0; k < kMaxN; ++k)
      if (k < rn) {
        const double rx = p[k][0] - cen[0], ry = p[k][1] - cen[1], rz = p[k][2] - cen[2];
        S[0] += rx * rx; S[1] += rx * ry; S[2] += rx * rz; S[3] += ry * ry; S[4] += ry * rz; S[5] += rz * rz;
      }
    ok = plane_from_sums_rule(cen, S, pl);
  }
  ok = ok && distinct;
#pragma unroll
  for (int k = 0; k < 4; ++k) planes[4 * (size_t)g + k] = ok ? pl[k] : 0.0;
  valid[g] = ok ? 1u : 0u;
}

// blockIdx.x: a chunk of kChunk consecutive points; blockIdx.y * 256 + lane: the trial.  The
// chunk goes through LDS kEvalTile points at a time, by 16-byte loads (an odd last double alone),
// and comes back as broadcasts in index order; a lane without a trial, or with an invalid one,
// runs the zero plane and is ignored later, so no wave diverges inside the loop.  count and err
// per (trial, chunk).  Two tiles per chunk, not one: 24 KB of LDS lets six workgroups share a CU,
// and the order of the sum does not depend on the tile.
__global__ __launch_bounds__(256)
void plane_eval_kernel(Hdr* hdr, const double* __restrict__ xyz, int64_t n, const double* __restrict__ planes, int batch,
                       double thr, int nb, int32_t* __restrict__ cnt_part, double* __restrict__ err_part) {
  __shared__ double2 tile2[3 * kEvalTile / 2];
  const int t = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * kChunk;
  const int m = (int)(n - p0 < kChunk ? n - p0 : kChunk);
  const int g = blockIdx.y * 256 + t;
  const bool have = g < batch;
  const double a = have ? planes[4 * (size_t)g] : 0.0, b = have ? planes[4 * (size_t)g + 1] : 0.0;
  const double c = have ? planes[4 * (size_t)g + 2] : 0.0, d = have ? planes[4 * (size_t)g + 3] : 0.0;
  const double* tile = (const double*)tile2;
  int32_t cnt = 0;
  double err = 0.0;
  bool bad = false;
  for (int tb = 0; tb < m; tb += kEvalTile) {
    const int mm = m - tb < kEvalTile ? m - tb : kEvalTile;
    const int words = 3 * mm;
    const double* src = xyz + 3 * (p0 + tb);     // 16-byte aligned: xyz is, and 3 * kEvalTile * 8 is a multiple of 16
    __syncthreads();                             // the previous tile has been consumed
    for (int w = t; 2 * w < words; w += 256) {
      double2 v;
      if (2 * w + 1 < words) {
        v = ((const double2*)src)[w];
      } else {
        v.x = src[2 * w];
        v.y = 0.0;
      }
      bad = bad || !(isfinite(v.x) && isfinite(v.y));
      tile2[w] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < mm; ++j) {
      const double dist = plane_distance_rule(a, b, c, d, tile[3 * j], tile[3 * j + 1], tile[3 * j + 2]);
      const bool in = plane_inlier_rule(dist, thr);
      cnt += in ? 1 : 0;
      err += in ? dist : 0.0;
    }
  }
  if (bad) atomicOr(&hdr->status, SLG_FILTER_BAD_NONFINITE);
  if (have) {
    cnt_part[(size_t)g * nb + blockIdx.x] = cnt;
    err_part[(size_t)g * nb + blockIdx.x] = err;
  }
}

// One wave per trial: the trial's partials come into LDS kRecordsTile chunks at a time (one
// contiguous row, so many loads are in flight), lane 0 adds them in chunk order and writes the
// record.  (One lane per trial over [chunk][trial] partials was one workgroup waiting for one
// load after another: 0.33 ms for 1,196 chunks, more than the evaluation itself.)
__global__ __launch_bounds__(64)
void plane_records_kernel(const Hdr* hdr, const double* __restrict__ planes, const uint32_t* __restrict__ valid,
                          const int32_t* __restrict__ cnt_part, const double* __restrict__ err_part, int nb,
                          int64_t n, int64_t t0, double* __restrict__ records) {
  __shared__ double es[kRecordsTile];
  __shared__ int32_t cs[kRecordsTile];
  if (hdr->status) return;                       // a non-finite point, seen by the launch before; the same for every lane
  const int g = blockIdx.x, lane = threadIdx.x;
  int64_t cnt = 0;
  double err = 0.0;
  for (int b0 = 0; b0 < nb; b0 += kRecordsTile) {
    const int mm = nb - b0 < kRecordsTile ? nb - b0 : kRecordsTile;
    __syncthreads();                             // the previous tile has been consumed
    for (int w = lane; w < mm; w += 64) {
      es[w] = err_part[(size_t)g * nb + b0 + w];
      cs[w] = cnt_part[(size_t)g * nb + b0 + w];
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll 8
      for (int k = 0; k < mm; ++k) {
        cnt += cs[k];
        err += es[k];
      }
    }
  }
  if (lane != 0) return;
  const bool ok = valid[g] != 0;
  const double count = ok ? (double)cnt : 0.0;
  err = ok ? err : 0.0;
  double* rec = records + (size_t)g * kRecordStride;
  rec[0] = (double)(t0 + g);
  rec[1] = ok ? 1.0 : 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) rec[2 + k] = planes[4 * (size_t)g + k];
  rec[6] = count;
  rec[7] = err;
  rec[8] = count / (double)n;
  rec[9] = count > 0.0 ? err / sqrt(count) : 0.0;
#pragma unroll
  for (int k = 10; k < kRecordStride; ++k) rec[k] = 0.0;
}

struct Plane4 { double v[4]; };

__global__ __launch_bounds__(256)
void plane_inliers_kernel(Hdr* hdr, const double* __restrict__ xyz, int64_t n, Plane4 pl, double thr,
                          uint32_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) atomicOr(&hdr->status, SLG_FILTER_BAD_NONFINITE);
  flags[i] = plane_inlier_rule(plane_distance_rule(pl.v[0], pl.v[1], pl.v[2], pl.v[3], x, y, z), thr) ? 1u : 0u;
}

// pos = exclusive scan of flags: the inliers' indices in ascending order, and their number.
__global__ __launch_bounds__(256)
void plane_indices_kernel(int64_t n, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos,
                          int64_t* __restrict__ index_out, int64_t* __restrict__ count_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (flags[i]) index_out[pos[i]] = i;
  if (i == n - 1) *count_out = (int64_t)pos[i] + flags[i];
}

// The refit's sums over the input order with the fixed tree of cloud_grid.h (8 consecutive points
// per thread, the workgroup's tree, one partial set per kChunk points); a point that is no inlier
// adds nothing.  PASS 0: x y z.  PASS 1: the six centred sums about sums[9..11].
template <int PASS>
__global__ __launch_bounds__(256)
void plane_refit_partial_kernel(const Hdr* hdr, const double* __restrict__ xyz, int64_t n,
                                const uint32_t* __restrict__ flags, const double* __restrict__ sums,
                                double* __restrict__ part) {
  __shared__ double sm[256];
  if (hdr->status) return;
  constexpr int kT = PASS == 0 ? 3 : 6;
  double cen[3] = {0.0, 0.0, 0.0};
  if (PASS == 1) { cen[0] = sums[9]; cen[1] = sums[10]; cen[2] = sums[11]; }
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int64_t base = (int64_t)blockIdx.x * kChunk + threadIdx.x * (kChunk / 256);
  for (int j = 0; j < kChunk / 256; ++j) {
    const int64_t i = base + j;
    if (i >= n) break;
    if (!flags[i]) continue;
    const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (PASS == 0) {
      acc[0] += x; acc[1] += y; acc[2] += z;
    } else {
      const double rx = x - cen[0], ry = y - cen[1], rz = z - cen[2];
      acc[0] += rx * rx; acc[1] += rx * ry; acc[2] += rx * rz; acc[3] += ry * ry; acc[4] += ry * rz; acc[5] += rz * rz;
    }
  }
#pragma unroll
  for (int k = 0; k < kT; ++k) {
    const double s = block_tree_sum(acc[k], sm);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.x * 6 + k] = s;
    __syncthreads();                             // sm[0] has been read before the next sum overwrites it
  }
}

// One workgroup: the tree over the partials.  PASS 0 leaves the sums, the centroid and the count;
// PASS 1 the six centred sums and the refitted plane.
template <int PASS>
__global__ __launch_bounds__(256)
void plane_refit_final_kernel(const Hdr* hdr, const double* __restrict__ part, int nb, const int64_t* __restrict__ count,
                              double* __restrict__ sums, double* __restrict__ plane_out) {
  __shared__ double sm[256];
  __shared__ double res[6];
  if (hdr->status) return;
  constexpr int kT = PASS == 0 ? 3 : 6;
#pragma unroll
  for (int k = 0; k < kT; ++k) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) s += part[(int64_t)b * 6 + k];
    s = block_tree_sum(s, sm);
    if (threadIdx.x == 0) res[k] = s;
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double m = (double)*count;
  if (PASS == 0) {
    for (int k = 0; k < 3; ++k) { sums[k] = res[k]; sums[9 + k] = m > 0.0 ? res[k] / m : 0.0; }
    sums[12] = m;
    for (int k = 13; k < kSumsLen; ++k) sums[k] = 0.0;
  } else {
    for (int k = 0; k < 6; ++k) sums[3 + k] = res[k];
    const double cen[3] = {sums[9], sums[10], sums[11]};
    double pl[4];
    plane_from_sums_rule(cen, res, pl);          // no inlier: zero sums, a zero norm, the zero plane
    for (int k = 0; k < 4; ++k) plane_out[k] = pl[k];
  }
}

int plane_bind(const char* who, int64_t n, int32_t batch, void* ws, int64_t ws_bytes, PlaneWs* w) {
  return begin_ext_call(who, "slg_plane_ws_bytes", n, 0, ws, ws_bytes, &w->grid,
                        [&](Bump& b) { plane_layout(b, n, batch, w); });
}

}  // namespace

static_assert(kMaxBatch == SLG_PLANE_MAX_BATCH && kRecordStride == SLG_PLANE_RECORD_STRIDE &&
              kSumsLen == SLG_PLANE_SUMS_LEN && kMaxN == SLG_PLANE_MAX_RANSAC_N, "slgpu.h");

extern "C" int64_t slg_plane_ws_bytes(int64_t n, int32_t batch) {
  if (n <= 0 || batch <= 0) return -(int64_t)slg_internal_fail(SLG_ERR_INVALID, "slg_plane_ws_bytes: n <= 0 or batch <= 0");
  if (n > kMaxPoints || batch > kMaxBatch)
    return -(int64_t)slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_plane_ws_bytes: more than 2^30 points or batch > %d",
                                       kMaxBatch);
  PlaneWs w;
  return ext_ws_bytes(n, 0, [&](Bump& b) { plane_layout(b, n, batch, &w); });
}

extern "C" int32_t slg_plane_batch(const double* xyz, int64_t n, double distance_threshold, int32_t ransac_n, int64_t seed,
                                   int64_t first_trial, int32_t batch, void* ws, int64_t ws_bytes, double* records_out,
                                   void* stream) {
  if (n <= 0 || batch <= 0 || first_trial < 0 || ransac_n < kMinN || !(distance_threshold > 0.0) ||
      !isfinite(distance_threshold) || !xyz || ((uintptr_t)xyz & 15) || !records_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_plane_batch: n <= 0, batch <= 0, first_trial < 0, ransac_n < 3, a threshold "
                                              "that is not finite and > 0, a NULL buffer or xyz not 16-byte aligned");
  if (ransac_n > kMaxN) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_plane_batch: ransac_n > %d", kMaxN);
  if (n > kMaxPoints || batch > kMaxBatch)
    return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_plane_batch: more than 2^30 points or batch > %d", kMaxBatch);
  if (n < ransac_n) return slg_internal_fail(SLG_ERR_INVALID, "slg_plane_batch: fewer points than ransac_n");
  PlaneWs w;
  int rc = plane_bind("slg_plane_batch", n, batch, ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(w.grid.hdr, 0, 256, st) != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "slg_plane_batch: memset failed");
  const int nb = grid_of(n, kChunk), gb = grid_of(batch, 256);
  plane_trials_kernel<<<gb, 256, 0, st>>>(xyz, n, ransac_n, (uint64_t)seed, first_trial, batch, w.planes, w.valid);
  plane_eval_kernel<<<dim3(nb, gb), 256, 0, st>>>(w.grid.hdr, xyz, n, w.planes, batch, distance_threshold, nb, w.cnt,
                                                  w.err);
  plane_records_kernel<<<batch, 64, 0, st>>>(w.grid.hdr, w.planes, w.valid, w.cnt, w.err, nb, n, first_trial, records_out);
  return check_launch("slg_plane_batch");
}

extern "C" int32_t slg_plane_finish(const double* xyz, int64_t n, const double* plane, double distance_threshold, void* ws,
                                    int64_t ws_bytes, int64_t* index_out, int64_t* count_out, double* sums_out,
                                    double* plane_out, void* stream) {
  if (n <= 0 || !(distance_threshold > 0.0) || !isfinite(distance_threshold) || !xyz || !plane || !index_out || !count_out ||
      !sums_out || !plane_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_plane_finish: n <= 0, a threshold that is not finite and > 0, or a NULL buffer");
  Plane4 pl;
  for (int k = 0; k < 4; ++k) {
    if (!isfinite(plane[k])) return slg_internal_fail(SLG_ERR_INVALID, "slg_plane_finish: the plane is not finite");
    pl.v[k] = plane[k];
  }
  if (n > kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_plane_finish: more than 2^30 points");
  PlaneWs w;
  int rc = plane_bind("slg_plane_finish", n, 1, ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(w.grid.hdr, 0, 256, st) != hipSuccess) return slg_internal_fail(SLG_ERR_HIP, "slg_plane_finish: memset failed");
  const Ws& g = w.grid;
  const int nb = grid_of(n, kChunk), gn = grid_of(n, 256);
  plane_inliers_kernel<<<gn, 256, 0, st>>>(g.hdr, xyz, n, pl, distance_threshold, g.idx);      // idx: the flags
  if ((rc = scan_u32("slg_plane_finish", g, g.idx, g.pos, n, st))) return rc;
  plane_indices_kernel<<<gn, 256, 0, st>>>(n, g.idx, g.pos, index_out, count_out);
  plane_refit_partial_kernel<0><<<nb, 256, 0, st>>>(g.hdr, xyz, n, g.idx, sums_out, g.part);
  plane_refit_final_kernel<0><<<1, 256, 0, st>>>(g.hdr, g.part, nb, count_out, sums_out, plane_out);
  plane_refit_partial_kernel<1><<<nb, 256, 0, st>>>(g.hdr, xyz, n, g.idx, sums_out, g.part);
  plane_refit_final_kernel<1><<<1, 256, 0, st>>>(g.hdr, g.part, nb, count_out, sums_out, plane_out);
  return check_launch("slg_plane_finish");
}
