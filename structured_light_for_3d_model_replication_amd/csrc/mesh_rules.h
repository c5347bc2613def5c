// mesh_rules.h -- the rules the two watertight meshers share (included, never compiled alone):
// cloud_mesh.hip (the dense grid) and cloud_band.hip (the banded cascade; §21).  One
// __device__ function per rule, each restated in tests/mesh_ref.py; fp64 under -ffp-contract=off.
#pragma once
#include "cloud_grid.h"

namespace slgmesh {

struct MeshHdr {        // 256 bytes at the front of the workspace; mesh.py reads it by these offsets
  int32_t status;       // SLG_FILTER_BAD_* bits
  int32_t R;
  int64_t nV, nT;
  double origin[3];
  double h, iso, thr;
};
static_assert(sizeof(MeshHdr) <= SLG_MESH_HDR_BYTES, "header");
static_assert(offsetof(MeshHdr, status) == 0 && offsetof(MeshHdr, R) == 4 && offsetof(MeshHdr, nV) == 8 &&
              offsetof(MeshHdr, nT) == 16 && offsetof(MeshHdr, origin) == 24 && offsetof(MeshHdr, h) == 48 &&
              offsetof(MeshHdr, iso) == 56 && offsetof(MeshHdr, thr) == 64, "mesh.py's offsets");

constexpr double kOmega = 6.0 / 7.0;
// the Kuhn tetrahedra: corner codes (dx + 2 dy + 4 dz) along the six axis-order paths 000 -> 111
__device__ constexpr int kTetCode[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
__device__ constexpr int kTetOdd[6] = {0, 1, 1, 0, 0, 1};
// owned edge types +x +y +z +xy +xz +yz +xyz as corner codes, and back
__device__ constexpr int kEdgeCode[7] = {1, 2, 4, 3, 5, 6, 7};
__device__ constexpr int kTypeOfCode[8] = {-1, 0, 1, 3, 2, 4, 5, 6};

// u = (p - origin) / h, i = floor(u) clamped to 0 .. R - 1 (also for NaN), t = u - i.
__device__ inline void cell_rule(double p, double o, double h, int R, int* i, double* t) {
  const double u = (p - o) / h;
  double c = floor(u);
  if (!(c > 0.0)) c = 0.0;
  if (c > (double)(R - 1)) c = (double)(R - 1);
  *i = (int)c;
  *t = u - c;
}
// The trilinear weight of corner (dx, dy, dz) of the cell.
__device__ inline double corner_weight_rule(const double* t, int dx, int dy, int dz) {
  const double wx = dx ? t[0] : 1.0 - t[0], wy = dy ? t[1] : 1.0 - t[1], wz = dz ? t[2] : 1.0 - t[2];
  return (wx * wy) * wz;
}
__device__ inline double jacobi_rule(double uc, double S, double f, double h2) {
  return uc + kOmega * ((S - h2 * f) / 6.0 - uc);
}
__device__ inline bool inside_rule(double chi, double iso) { return chi < iso; }
// The triangles of a tetrahedron whose inside corners are the bits of m (tests/mesh_ref.py:
// tet_case): tri[j][e] = (p, q), p < q, local corner numbers of the edge carrying vertex e.
__device__ inline int tet_case_rule(int m, int odd, int (*tri)[3][2]) {
  int ins[4], outs[4], ni = 0, no = 0;
  for (int v = 0; v < 4; ++v) {
    if ((m >> v) & 1) ins[ni++] = v; else outs[no++] = v;
  }
  if (ni == 0 || ni == 4) return 0;
  int nt;
  if (ni == 2) {
    const int A = ins[0], B = ins[1];
    int C = outs[0], D = outs[1];
    if (((A > C) + (A > D) + (B > C) + (B > D)) & 1) { const int s = C; C = D; D = s; }
    const int q[2][3][2] = {{{A, C}, {A, D}, {B, D}}, {{A, C}, {B, D}, {B, C}}};
    for (int j = 0; j < 2; ++j)
      for (int e = 0; e < 3; ++e) { tri[j][e][0] = q[j][e][0]; tri[j][e][1] = q[j][e][1]; }
    nt = 2;
  } else {
    const int A = ni == 1 ? ins[0] : outs[0];
    int o[3], k = 0;
    for (int v = 0; v < 4; ++v)
      if (v != A) o[k++] = v;
    if (A & 1) { const int s = o[1]; o[1] = o[2]; o[2] = s; }
    if (ni == 3) { const int s = o[1]; o[1] = o[2]; o[2] = s; }
    for (int e = 0; e < 3; ++e) { tri[0][e][0] = A; tri[0][e][1] = o[e]; }
    nt = 1;
  }
  for (int j = 0; j < nt; ++j) {
    if (odd)
      for (int c = 0; c < 2; ++c) { const int s = tri[j][1][c]; tri[j][1][c] = tri[j][2][c]; tri[j][2][c] = s; }
    for (int e = 0; e < 3; ++e)
      if (tri[j][e][0] > tri[j][e][1]) { const int s = tri[j][e][0]; tri[j][e][0] = tri[j][e][1]; tri[j][e][1] = s; }
  }
  return nt;
}

}  // namespace slgmesh
