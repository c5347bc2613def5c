/* slgpu_intersect.h -- the mesh self-intersection test's entry points of libslgpu.so
 * (csrc/cloud_intersect.hip): which pairs of triangles of an indexed mesh in HBM cross.
 * Our rule, Open3D parity (is_self_intersecting) unpinned; a pure function of the mesh, restated in
 * tests/intersect_ref.py, which is its definition.  Asynchronous on `stream`.
 *
 * A fifth table beside slgpu.h (whose codes, types and conventions hold here): the same library,
 * bound by the same _native.lib() from _native.INTERSECT_EXPORTS.
 *
 * Vertices double [V * 3], triangles int32 [T * 3]; 0 < V < 2^31, 0 < 3 T <= 2^30.  A triangle with
 * two equal indices or with a coordinate that is not finite takes part in nothing.  A candidate is a
 * pair s < t of the others whose closed boxes overlap on all three axes.  By the indices they share a
 * candidate is adjacent (2 or 3: counted, not tested), or tested on two edges (1, after rotating both
 * so that a0 == b0) or on six (0).  Every sign is the fp64 determinant orient3dfast in one fixed
 * order of operations, certain when |det| > SLG_ISECT_BOUND * permanent; an edge pierces the other
 * triangle iff its ends lie strictly on both sides of its plane and it passes the three edges on one
 * strict side.  A pair is intersecting iff an edge pierces; uncertain iff no edge test is certainly
 * piercing and one is neither certainly excluded nor certainly piercing.
 *
 * How the candidates are found is no part of the answer: a uniform grid of at most
 * SLG_ISECT_MAX_CELLS cells per axis, cell side `cell` (<= 0: twice the mean longest box side, an
 * integer sum), one entry cell << 32 | t per cell of a triangle that spans at most
 * SLG_ISECT_SPAN_CAP cells, the others on the large list; a pair of two listed triangles is taken in
 * the one cell that is the per-axis maximum of their low cells, a pair with a large triangle by the
 * scan of that triangle (two large ones: of the lower index).
 *
 * The workspace of stage SLG_ISECT_WS_BOXES holds the header in its first 256 bytes: int32 status
 * at 0 (SLG_FILTER_BAD_INDEX), int64 entries at 8, large triangles at 16, triangles that take part at
 * 24, cell runs at 32, candidates at 40, int32 dims[3] at 56, double origin[3] at 72, cell at 96, and
 * at byte 128 int64 stats[8] indexed by SLG_ISECT_STAT_*.  The stages ENTRIES (n_items entries, fewer
 * than 2^31), PAIRS (n_items candidates) and LIST (n_items listed pairs) are arrays without a header.
 * The counts a call takes are the header's as read back; with another count its kernels return.
 *
 *   slg_isect_boxes             boxes, the grid, cell ranges, the large list; entries and large
 *                               triangles in the header for one read-back.
 *   slg_isect_entries           the entries, sorted, and the starts of their cell runs.  n_entries
 *                               as read back.
 *   slg_isect_candidates_count  candidates into the header: one wavefront per cell run over tiles
 *                               of SLG_ISECT_TILE boxes in LDS, one workgroup per large triangle.
 *                               With n_entries == 0 the entries workspace is not looked at.
 *   slg_isect_candidates_emit   the same walk writing the keys s << 32 | t, in no particular order.
 *   slg_isect_test              one lane per candidate: the verdict byte (SLG_ISECT_INTERSECTING,
 *                               SLG_ISECT_UNCERTAIN), the stats, triangle_class_out uint8 [T] with the
 *                               same bits.
 *   slg_isect_list              the pairs whose verdict has `which`, ascending, int32 [n_list * 2].
 *
 * Every kernel returns when the header's status is set.  SLG_ERR_INVALID for a NULL buffer, counts
 * out of range, an unknown stage, or a workspace that is NULL, misaligned or too small. */
#ifndef SLGPU_INTERSECT_H
#define SLGPU_INTERSECT_H

#include "slgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLG_ISECT_WS_BOXES 0
#define SLG_ISECT_WS_ENTRIES 1
#define SLG_ISECT_WS_PAIRS 2
#define SLG_ISECT_WS_LIST 3
#define SLG_ISECT_SPAN_CAP 64
#define SLG_ISECT_MAX_CELLS 1024
#define SLG_ISECT_TILE 64
#define SLG_ISECT_BOUND 0x1.c000000000007p-51
#define SLG_ISECT_INTERSECTING 1
#define SLG_ISECT_UNCERTAIN 2
#define SLG_ISECT_STAT_ADJACENT 0
#define SLG_ISECT_STAT_TESTED 1
#define SLG_ISECT_STAT_INTERSECTING 2
#define SLG_ISECT_STAT_UNCERTAIN 3
#define SLG_ISECT_STAT_INTERSECTING_TRIANGLES 4
#define SLG_ISECT_STAT_UNCERTAIN_TRIANGLES 5
int64_t slg_isect_ws_bytes(int32_t stage, int64_t n_vertices, int64_t n_triangles, int64_t n_items);
int32_t slg_isect_boxes(const double *vertices, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, double cell,
                        void *ws, int64_t ws_bytes, void *stream);
int32_t slg_isect_entries(int64_t n_triangles, int64_t n_vertices, void *ws, int64_t ws_bytes, int64_t n_entries, void *entries_ws,
                          int64_t entries_ws_bytes, void *stream);
int32_t slg_isect_candidates_count(int64_t n_triangles, int64_t n_vertices, void *ws, int64_t ws_bytes, int64_t n_entries,
                                   void *entries_ws, int64_t entries_ws_bytes, int64_t n_large, void *stream);
int32_t slg_isect_candidates_emit(int64_t n_triangles, int64_t n_vertices, void *ws, int64_t ws_bytes, int64_t n_entries,
                                  void *entries_ws, int64_t entries_ws_bytes, int64_t n_large, int64_t n_candidates, void *pairs_ws,
                                  int64_t pairs_ws_bytes, void *stream);
int32_t slg_isect_test(const double *vertices, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, void *ws,
                       int64_t ws_bytes, int64_t n_candidates, void *pairs_ws, int64_t pairs_ws_bytes, uint8_t *triangle_class_out,
                       void *stream);
int32_t slg_isect_list(int32_t which, int64_t n_triangles, int64_t n_candidates, void *pairs_ws, int64_t pairs_ws_bytes,
                       int64_t n_list, void *list_ws, int64_t list_ws_bytes, int32_t *pairs_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SLGPU_INTERSECT_H */
