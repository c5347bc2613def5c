/* slgpu_surface.h -- the surface mesher's entry points of libslgpu.so (csrc/cloud_surface.hip;
 * DESIGN.md §20): the empty-ball triangles of an oriented cloud, radius by radius, what the device
 * takes of reconstruct_stl(mode="surface") (server/processing.py:711-728).  Our rule, Open3D parity
 * unpinned; a pure function of the cloud, its normals and the radii, restated in
 * tests/surface_ref.py.  Asynchronous on `stream`.
 *
 * A second table beside slgpu.h (whose codes, types and conventions hold here): the same library,
 * bound by the same _native.lib() from _native.SURFACE_EXPORTS.
 *
 * The caller keeps the state across the passes (one per radius, ascending): `closed`, uint8 [n],
 * zero at the start, and `taken`, the directed edges src << 32 | dst of the accepted triangles,
 * sorted ascending (never NULL, also when n_taken is 0).  Two workspaces, 256-byte aligned: the
 * grid's, slg_surface_ws_bytes(SLG_SURFACE_WS_GRID, n, 0, 0) bytes, whose first int32 is the status
 * word of the cloud steps (SLG_FILTER_BAD_NONFINITE, SLG_FILTER_BAD_EXTENT: 2^21 or more cells of
 * 2 r on an axis, SLG_FILTER_BAD_NEIGHBOURS; every later kernel of the pass then returns), and the
 * pass's, slg_surface_ws_bytes(SLG_SURFACE_WS_PASS, n, C, n_taken) bytes for C candidates, which
 * begins with int32 0 at byte 0, int64 live candidates at 8 and int64 accepted candidates at 16.
 *
 *   slg_surface_begin   the sparse grid with cell 2 r over the cloud.
 *   slg_surface_count   *total_out = C, the candidate triples a < b < c of the pass: no vertex
 *                       closed, squared sides < 4 r^2 (d2_rule), not flat, circumradius <= r, the
 *                       three normals on one side, no other point j with
 *                       d2(P[j], o) < r^2 (1 - 2^-30) for the centre o of the ball resting on it.
 *                       An anchor a with more than SLG_SURFACE_MAX_NEIGHBOURS open neighbours of
 *                       higher index within 2 r sets SLG_FILTER_BAD_NEIGHBOURS.  The caller reads
 *                       the status word and C, and sizes the pass workspace.
 *   slg_surface_emit    the candidates again, into the pass workspace; their rank (ascending bits
 *                       of rho^2, a, b, c); the slots of their directed edges; live = no edge in
 *                       `taken`.
 *   slg_surface_round   one round of the selection: integer atomicMin of the rank on the three
 *                       slots of every live candidate, those that hold all three are accepted and
 *                       mark them, the live candidates on a marked slot leave.  The caller reads
 *                       live and accepted after every round and stops at live == 0.
 *   slg_surface_commit  the n_accepted triangles in rank order into triangles_out, `taken` and
 *                       their edges merged into taken_out (n_taken + 3 n_accepted keys), and
 *                       closed[v] = v has a taken edge and every taken edge at v has its reverse.
 *
 * SLG_ERR_INVALID for a NULL or misaligned buffer, n < 3, a radius that is not finite and > 0,
 * C <= 0 or 3 C > 2^30, n_accepted outside 1..C, or a workspace that is too small. */
#ifndef SLGPU_SURFACE_H
#define SLGPU_SURFACE_H

#include "slgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLG_FILTER_BAD_NEIGHBOURS 8         /* beside slgpu.h's SLG_FILTER_BAD_* bits */
#define SLG_SURFACE_MAX_NEIGHBOURS 512
#define SLG_SURFACE_MAX_RADII 8
#define SLG_SURFACE_WS_GRID 0
#define SLG_SURFACE_WS_PASS 1
int64_t slg_surface_ws_bytes(int32_t stage, int64_t n, int64_t n_candidates, int64_t n_taken);
int32_t slg_surface_begin(const double *xyz, int64_t n, double radius, void *grid_ws, int64_t grid_ws_bytes,
                          void *stream);
int32_t slg_surface_count(const double *normals, const uint8_t *closed, int64_t n, double radius, void *grid_ws,
                          int64_t grid_ws_bytes, int64_t *total_out, void *stream);
int32_t slg_surface_emit(const double *normals, const uint8_t *closed, int64_t n, double radius, void *grid_ws,
                         int64_t grid_ws_bytes, const uint64_t *taken, int64_t n_taken, void *pass_ws,
                         int64_t pass_ws_bytes, int64_t n_candidates, void *stream);
int32_t slg_surface_round(void *pass_ws, int64_t pass_ws_bytes, int64_t n, int64_t n_candidates, int64_t n_taken,
                          void *stream);
int32_t slg_surface_commit(void *pass_ws, int64_t pass_ws_bytes, int64_t n, int64_t n_candidates,
                           const uint64_t *taken, int64_t n_taken, int64_t n_accepted, int32_t *triangles_out,
                           uint64_t *taken_out, uint8_t *closed, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SLGPU_SURFACE_H */
