// cloud_normals.hip -- the Open3D steps of the merge tail and of the front of both meshing
// methods on the device (server/processing.py:605-628, :653-670, :804-837): voxel down-sample (a
// per-voxel ordered reduction over the grid of cloud_grid.h), normal estimation (the ring walk
// with the neighbours' indices kept), orientation and centroid.  Rules: DESIGN.md §10 and
// tests/normals_ref.py.
#include "cloud_grid.h"

using namespace slgcloud;

namespace {

// ---------------------------------------------------------------- voxel down-sample
// Open3D's VoxelDownSample, restated.  The grid is the shared one with the origin
// at min - voxel/2 and the cell exactly `voxel`: cell_coord is then floor((p - vmin) / voxel) in
// IEEE subtraction and division, NumPy's own result.  The stable (key, index) sort delivers each
// voxel's members in ascending original index, which is the order of the sums.
constexpr int kVoxelLong = 64;     // members above which a voxel goes to the wave kernel

__device__ inline double voxel_origin_rule(double mn, double voxel) { return mn - voxel * 0.5; }
__device__ inline double voxel_mean_rule(double sum, uint32_t count) { return sum / (double)count; }
// exact mean of a colour channel, rounded half up, in integers
__device__ inline uint8_t colour_mean_rule(unsigned long long sum, uint32_t count) {
  return (uint8_t)((2ull * sum + count) / (2ull * count));
}

__global__ void voxel_setup_kernel(Hdr* hdr, double voxel) {
  if (hdr->status) return;
  double vmin[3], c[3];
  for (int a = 0; a < 3; ++a) {
    vmin[a] = voxel_origin_rule(hdr->mn[a], voxel);
    c[a] = floor((hdr->mx[a] - vmin[a]) / voxel);
    if (!(c[a] <= (double)kCellMax)) { atomicOr(&hdr->status, SLG_FILTER_BAD_EXTENT); return; }
  }
  for (int a = 0; a < 3; ++a) { hdr->mn[a] = vmin[a]; hdr->cmax[a] = (int32_t)c[a]; }
  hdr->cell = voxel;
}

// head[i] = 1 when original point i is the first (smallest-index) member of its voxel.  The
// exclusive scan of head over the original order is the voxel's place in the output.
__global__ __launch_bounds__(256)
void voxel_heads_kernel(const Hdr* hdr, int64_t n, const uint64_t* __restrict__ keys_s,
                        const uint32_t* __restrict__ sidx, uint32_t* __restrict__ head) {
  if (hdr->status) return;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  head[sidx[q]] = (q == 0 || keys_s[q] != keys_s[q - 1]) ? 1u : 0u;
}

struct VoxelOut {
  double* xyz;
  uint8_t* bgr;
  int64_t* first;
  int32_t* count;
};

__device__ inline void voxel_write(const VoxelOut& o, uint32_t slot, uint32_t first, uint32_t count, double sx,
                                   double sy, double sz, const unsigned long long* cs) {
  o.xyz[3 * (size_t)slot] = voxel_mean_rule(sx, count);
  o.xyz[3 * (size_t)slot + 1] = voxel_mean_rule(sy, count);
  o.xyz[3 * (size_t)slot + 2] = voxel_mean_rule(sz, count);
  if (o.bgr)
    for (int a = 0; a < 3; ++a) o.bgr[3 * (size_t)slot + a] = colour_mean_rule(cs[a], count);
  if (o.first) o.first[slot] = (int64_t)first;
  if (o.count) o.count[slot] = (int32_t)count;
}

// One lane per voxel: the left-to-right sum of its members.  A voxel of more than kVoxelLong
// members goes to the list of voxel_long_kernel (list order is free).
__global__ __launch_bounds__(256)
void voxel_reduce_kernel(Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                         const uint8_t* __restrict__ bgr, const uint32_t* __restrict__ ustart,
                         const uint32_t* __restrict__ place, uint32_t* __restrict__ longlist, VoxelOut out,
                         int64_t* __restrict__ m_out) {
  if (hdr->status) return;
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int nu = hdr->n_unique;
  if (u == 0) *m_out = nu;
  if (u >= nu) return;
  const uint32_t s = ustart[u], e = ustart[u + 1];
  if (e - s > (uint32_t)kVoxelLong) {
    longlist[atomicAdd(&hdr->n_far, 1)] = (uint32_t)u;
    return;
  }
  double sx = sxyz[3 * (size_t)s], sy = sxyz[3 * (size_t)s + 1], sz = sxyz[3 * (size_t)s + 2];
  unsigned long long cs[3] = {0, 0, 0};
  const uint32_t first = sidx[s];
  if (bgr)
    for (int a = 0; a < 3; ++a) cs[a] = bgr[3 * (size_t)first + a];
  for (uint32_t j = s + 1; j < e; ++j) {
    sx += sxyz[3 * (size_t)j];
    sy += sxyz[3 * (size_t)j + 1];
    sz += sxyz[3 * (size_t)j + 2];
    if (bgr) {
      const size_t o = 3 * (size_t)sidx[j];
      for (int a = 0; a < 3; ++a) cs[a] += bgr[o + a];
    }
  }
  voxel_write(out, place[first], first, e - s, sx, sy, sz, cs);
}

// One wave per listed voxel: 64 members are loaded at a time, one per lane, and every lane then
// adds them in lane order from broadcasts, so the additions are the same sequence as the
// left-to-right sum while the loads run side by side.  Colour sums are integers (order-free).
__global__ __launch_bounds__(64)
void voxel_long_kernel(const Hdr* hdr, const double* __restrict__ sxyz, const uint32_t* __restrict__ sidx,
                       const uint8_t* __restrict__ bgr, const uint32_t* __restrict__ ustart,
                       const uint32_t* __restrict__ place, const uint32_t* __restrict__ longlist, VoxelOut out) {
  if (hdr->status) return;
  const int lane = threadIdx.x;
  const int nl = hdr->n_far;
  for (int f = blockIdx.x; f < nl; f += gridDim.x) {
    const uint32_t u = longlist[f];
    const uint32_t s = ustart[u], e = ustart[u + 1];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    unsigned long long cs[3] = {0, 0, 0};
    for (uint32_t base = s; base < e; base += 64) {
      const uint32_t j = base + lane;
      const int m = (int)(e - base < 64u ? e - base : 64u);
      double vx = 0.0, vy = 0.0, vz = 0.0;
      if (j < e) {
        vx = sxyz[3 * (size_t)j]; vy = sxyz[3 * (size_t)j + 1]; vz = sxyz[3 * (size_t)j + 2];
        if (bgr) {
          const size_t o = 3 * (size_t)sidx[j];
          for (int a = 0; a < 3; ++a) cs[a] += bgr[o + a];
        }
      }
      for (int t = 0; t < m; ++t) {
        const double bx = __shfl(vx, t, 64), by = __shfl(vy, t, 64), bz = __shfl(vz, t, 64);
        if (base == s && t == 0) { sx = bx; sy = by; sz = bz; }     // the sum starts at the first member
        else { sx += bx; sy += by; sz += bz; }
      }
    }
    for (int a = 0; a < 3; ++a)
      for (int sh = 32; sh > 0; sh >>= 1) cs[a] += __shfl_xor(cs[a], sh, 64);
    const uint32_t first = sidx[s];
    if (lane == 0) voxel_write(out, place[first], first, e - s, sx, sy, sz, cs);
  }
}

// ---------------------------------------------------------------- normals
// Open3D's EstimateNormals with KDTreeSearchParamHybrid, restated: the neighbours
// of a point are the first max_nn of all points in (d2, original index) order (TopKI,
// pair_before_rule) that have d2 < radius^2; nine raw moments summed in that order; cov = E[ab] -
// E[a]E[b]; the normal is the unit eigenvector of the smallest eigenvalue (cyclic Jacobi,
// kJacobiSweeps sweeps), signed so that the first non-zero of (nz, ny, nx) is positive.
constexpr int kJacobiSweeps = 5;

struct Moments {        // the nine running sums
  double x, y, z, xx, xy, xz, yy, yz, zz;
  __device__ inline void clear() { x = y = z = xx = xy = xz = yy = yz = zz = 0.0; }
  __device__ inline void add(double px, double py, double pz) {
    x += px; y += py; z += pz;
    xx += px * px; xy += px * py; xz += px * pz;
    yy += py * py; yz += py * pz; zz += pz * pz;
  }
};
struct Cov { double xx, xy, xz, yy, yz, zz; };
struct Vec3 { double x, y, z; };

// cov from the nine sums over m neighbours: each sum / m, then E[ab] - E[a] E[b].
__device__ __forceinline__ Cov covariance_rule(const Moments& M, int m) {
  const double d = (double)m;
  const double ex = M.x / d, ey = M.y / d, ez = M.z / d;
  Cov c;
  c.xx = M.xx / d - ex * ex;
  c.xy = M.xy / d - ex * ey;
  c.xz = M.xz / d - ex * ez;
  c.yy = M.yy / d - ey * ey;
  c.yz = M.yz / d - ey * ez;
  c.zz = M.zz / d - ez * ez;
  return c;
}

// One Jacobi rotation in the (p, q) plane of a symmetric 3x3 matrix (r is the third index):
// app, aqq, apq the plane's entries, arp, arq the third row's; v?p, v?q the eigenvector columns.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                     double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp; arq = rq;
  const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
  v0p = a0; v0q = b0;
  const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
  v1p = a1; v1q = b1;
  const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
  v2p = a2; v2q = b2;
}

// The normal of a covariance: (0, 0, 1) with fewer than 3 neighbours or a zero matrix.
__device__ __forceinline__ Vec3 normal_rule(const Cov& c, int m) {
  const bool none = m < 3 || (c.xx == 0.0 && c.xy == 0.0 && c.xz == 0.0 && c.yy == 0.0 && c.yz == 0.0 && c.zz == 0.0);
  double a00 = c.xx, a01 = c.xy, a02 = c.xz, a11 = c.yy, a12 = c.yz, a22 = c.zz;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  if (!none)
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
      jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1), third 2
      jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), third 1
      jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), third 0
    }
  // the column of the first smallest diagonal entry, as two selects (a lookup by index would put
  // the columns into scratch)
  const bool s1 = a11 < a00;
  const double lam = s1 ? a11 : a00;
  double x = s1 ? v01 : v00, y = s1 ? v11 : v10, z = s1 ? v21 : v20;
  const bool s2 = a22 < lam;
  x = s2 ? v02 : x; y = s2 ? v12 : y; z = s2 ? v22 : z;
  const double len = sqrt((x * x + y * y) + z * z);
  x = x / len; y = y / len; z = z / len;
  const bool flip = z != 0.0 ? z < 0.0 : (y != 0.0 ? y < 0.0 : x < 0.0);   // the sign rule
  Vec3 n;
  n.x = none ? 0.0 : (flip ? -x : x);
  n.y = none ? 0.0 : (flip ? -y : y);
  n.z = none ? 1.0 : (flip ? -z : z);
  return n;
}

__device__ __forceinline__ void normals_write(const Moments& M, int m, uint32_t o, double* __restrict__ normals,
                                     double* __restrict__ cov_out, int32_t* __restrict__ m_out) {
  Cov c = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (m > 0) c = covariance_rule(M, m);
  const Vec3 nrm = normal_rule(c, m);
  normals[3 * (size_t)o] = nrm.x;
  normals[3 * (size_t)o + 1] = nrm.y;
  normals[3 * (size_t)o + 2] = nrm.z;
  if (cov_out) {
    double* co = cov_out + 6 * (size_t)o;
    co[0] = c.xx; co[1] = c.xy; co[2] = c.xz; co[3] = c.yy; co[4] = c.yz; co[5] = c.zz;
  }
  if (m_out) m_out[o] = m;
}

// One point per thread: the ring walk with the (d2, index) list and the radius, then the moments
// in list order.  Points open after kMaxRing rings (a radius of many cells around a point with few
// neighbours) go to normals_far_kernel.
__global__ __launch_bounds__(64)
void normals_kernel(Hdr* hdr, const double* __restrict__ xyz, const double* __restrict__ sxyz,
                    const uint32_t* __restrict__ sidx, const uint64_t* __restrict__ ukeys,
                    const uint32_t* __restrict__ ustart, int64_t n, int k, double r2, double* __restrict__ normals,
                    double* __restrict__ cov_out, int32_t* __restrict__ m_out, uint32_t* __restrict__ far) {
  extern __shared__ double lds[];
  if (hdr->status) return;
  const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (q >= n) return;
  const int kk = (int)(n < k ? n : k);
  TopKI tk{lds + threadIdx.x, (uint32_t*)(lds + (size_t)kk * 64) + threadIdx.x, kk, 0, 0, -1.0, 0u};
  if (!ring_walk<true>(hdr, sxyz, sidx, ukeys, ustart, q, r2, tk)) {
    far[atomicAdd(&hdr->n_far, 1)] = (uint32_t)q;
    return;
  }
  tk.sort();
  Moments M;
  M.clear();
  for (int j = 0; j < tk.cnt; ++j) {
    const size_t o = 3 * (size_t)tk.idx[j * 64];
    M.add(xyz[o], xyz[o + 1], xyz[o + 2]);
  }
  normals_write(M, tk.cnt, sidx[q], normals, cov_out, m_out);
}

// knn_far_kernel (cloud_filter.hip) with the (d2, index) order: the wave merges its 64 sorted
// lists (wave_merge: the smallest (d2, index) head until kk are taken or none is left); every
// lane adds the same moments.
__global__ __launch_bounds__(64)
void normals_far_kernel(const Hdr* hdr, const double* __restrict__ xyz, const double* __restrict__ sxyz,
                        const uint32_t* __restrict__ sidx, int64_t n, int k, double r2, double* __restrict__ normals,
                        double* __restrict__ cov_out, int32_t* __restrict__ m_out, const uint32_t* __restrict__ far) {
  extern __shared__ double lds[];
  if (hdr->status) return;
  const int lane = threadIdx.x;
  const int nf = hdr->n_far;
  const int kk = (int)(n < k ? n : k);
  for (int f = blockIdx.x; f < nf; f += gridDim.x) {
    const int64_t q = far[f];
    const double p[3] = {sxyz[3 * q], sxyz[3 * q + 1], sxyz[3 * q + 2]};
    TopKI tk{lds + lane, (uint32_t*)(lds + (size_t)kk * 64) + lane, kk, 0, 0, -1.0, 0u};
    scan_range<true>(tk, sxyz, sidx, lane, (uint32_t)n, 64, p, r2);
    tk.sort();
    Moments M;
    M.clear();
    const int m = wave_merge<true>(tk, kk, [&](int, double, uint32_t bi) {
      const size_t o = 3 * (size_t)bi;
      M.add(xyz[o], xyz[o + 1], xyz[o + 2]);
    });
    if (lane == 0) normals_write(M, m, sidx[q], normals, cov_out, m_out);
  }
}

// Open3D's OrientNormalsTowardsCameraLocation: negated when normal . (loc - p) < 0; `outward`
// then negates every normal (the reference's `* -1.0`).
__device__ inline bool orient_flip_rule(const double* nrm, const double* p, const double* loc) {
  const double rx = loc[0] - p[0], ry = loc[1] - p[1], rz = loc[2] - p[2];
  return (nrm[0] * rx + nrm[1] * ry) + nrm[2] * rz < 0.0;
}

__global__ __launch_bounds__(256)
void orient_kernel(const double* __restrict__ xyz, double* __restrict__ normals, int64_t n,
                   const double* __restrict__ loc, int outward) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  const double l[3] = {loc[0], loc[1], loc[2]};
  double v[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
  const bool flip = orient_flip_rule(v, p, l) != (outward != 0);
  if (flip)
    for (int a = 0; a < 3; ++a) normals[3 * i + a] = -v[a];
}

// Per-axis sums over the input order with the fixed tree of the statistical filter's sums
// (cloud_filter.hip): 8 consecutive points per thread, the workgroup's tree, then the partials.
__global__ __launch_bounds__(256)
void axis_sum_partial_kernel(const double* __restrict__ xyz, int64_t n, double* __restrict__ part) {
  __shared__ double sm[256];
  const int64_t base = (int64_t)blockIdx.x * kChunk + threadIdx.x * (kChunk / 256);
  for (int a = 0; a < 3; ++a) {
    double s = 0.0;
    for (int j = 0; j < kChunk / 256; ++j)
      if (base + j < n) s += xyz[3 * (base + j) + a];
    s = block_tree_sum(s, sm);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.x * 3 + a] = s;
    __syncthreads();                         // sm[0] has been read before the next axis overwrites it
  }
}

__global__ __launch_bounds__(256)
void axis_sum_final_kernel(const double* __restrict__ part, int nb, int64_t n, double* __restrict__ out) {
  __shared__ double sm[256];
  for (int a = 0; a < 3; ++a) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) s += part[(int64_t)b * 3 + a];
    s = block_tree_sum(s, sm);
    if (threadIdx.x == 0) out[a] = s / (double)n;
    __syncthreads();
  }
}

}  // namespace

extern "C" int32_t slg_voxel_downsample(const double* xyz, const uint8_t* bgr, int64_t n, double voxel_size, void* ws,
                                        int64_t ws_bytes, double* xyz_out, uint8_t* bgr_out, int64_t* first_index_out,
                                        int32_t* count_out, int64_t* m_out, void* stream) {
  if (n <= 0 || !(voxel_size > 0.0) || !isfinite(voxel_size) || !xyz || !xyz_out || !m_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_voxel_downsample: n <= 0, voxel_size not finite and > 0, or a NULL buffer");
  Ws w;
  int rc = begin_call("slg_voxel_downsample", n, ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = bbox(xyz, n, w, 0.0, 0, st))) return rc;       // the box; voxel_setup_kernel fixes origin and cell
  voxel_setup_kernel<<<1, 1, 0, st>>>(w.hdr, voxel_size);
  if ((rc = build_grid(xyz, n, w, st))) return rc;
  const VoxelScratch s = voxel_scratch(w, n);
  const int g = grid_of(n, 256);
  voxel_heads_kernel<<<g, 256, 0, st>>>(w.hdr, n, w.keys_s, w.idx_s, s.head);
  if ((rc = scan_u32("slg_voxel_downsample", w, s.head, s.place, n, st))) return rc;
  const VoxelOut out{xyz_out, bgr ? bgr_out : nullptr, first_index_out, count_out};
  voxel_reduce_kernel<<<g, 256, 0, st>>>(w.hdr, w.sxyz, w.idx_s, bgr, w.ustart, s.place, w.far, out, m_out);
  voxel_long_kernel<<<(int)(n < 1024 ? n : 1024), 64, 0, st>>>(w.hdr, w.sxyz, w.idx_s, bgr, w.ustart, s.place, w.far, out);
  return check_launch("slg_voxel_downsample");
}

extern "C" int32_t slg_estimate_normals(const double* xyz, int64_t n, double radius, int32_t max_nn, void* ws,
                                        int64_t ws_bytes, double* normals_out, double* cov_out, int32_t* m_out,
                                        void* stream) {
  if (n <= 0 || !(radius > 0.0) || !isfinite(radius) || max_nn < 3 || !xyz || !normals_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_estimate_normals: n <= 0, radius not finite and > 0, max_nn < 3 or a NULL buffer");
  if (max_nn > kMaxK) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_estimate_normals: max_nn > %d", kMaxK);
  Ws w;
  int rc = begin_call("slg_estimate_normals", n, ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int k = max_nn;
  if ((rc = knn_grid(xyz, n, w, k, st))) return rc;        // the grid slg_statistical_outlier builds
  const size_t lds = (size_t)(n < k ? n : k) * 64 * (sizeof(double) + sizeof(uint32_t));
  const double r2 = radius * radius;
  normals_kernel<<<grid_of(n, 64), 64, lds, st>>>(w.hdr, xyz, w.sxyz, w.idx_s, w.ukeys, w.ustart, n, k, r2, normals_out,
                                                  cov_out, m_out, w.far);
  normals_far_kernel<<<(int)(n < 1024 ? n : 1024), 64, lds, st>>>(w.hdr, xyz, w.sxyz, w.idx_s, n, k, r2, normals_out,
                                                                  cov_out, m_out, w.far);
  return check_launch("slg_estimate_normals");
}

extern "C" int32_t slg_orient_normals(const double* xyz, double* normals, int64_t n, const double* location,
                                      int32_t outward, void* stream) {
  if (n <= 0 || !xyz || !normals || !location)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_orient_normals: n <= 0 or a NULL buffer");
  if (n > kMaxPoints) return slg_internal_fail(SLG_ERR_UNSUPPORTED, "slg_orient_normals: more than 2^30 points");
  orient_kernel<<<grid_of(n, 256), 256, 0, (hipStream_t)stream>>>(xyz, normals, n, location, outward);
  return check_launch("orient_kernel");
}

extern "C" int32_t slg_cloud_centroid(const double* xyz, int64_t n, void* ws, int64_t ws_bytes, double* centroid_out,
                                      void* stream) {
  if (n <= 0 || !xyz || !centroid_out)
    return slg_internal_fail(SLG_ERR_INVALID, "slg_cloud_centroid: n <= 0 or a NULL buffer");
  Ws w;
  int rc = begin_call("slg_cloud_centroid", n, ws, ws_bytes, &w);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int nb = grid_of(n, kChunk);
  axis_sum_partial_kernel<<<nb, 256, 0, st>>>(xyz, n, w.part);
  axis_sum_final_kernel<<<1, 256, 0, st>>>(w.part, nb, n, centroid_out);
  return check_launch("slg_cloud_centroid");
}
