/* slgpu_audit.h -- the mesh audit's entry points of libslgpu.so (csrc/cloud_audit.hip; DESIGN.md
 * §22): whether an indexed triangle mesh in HBM is closed, manifold, oriented and one piece, its
 * signed volume and area, and the selection that keeps chosen triangles and the vertices they use.
 * Our rules, Open3D / MeshLab parity unpinned; pure functions of the mesh, restated in
 * tests/audit_ref.py.  Self-intersection is not tested.  Asynchronous on `stream`.
 *
 * A fourth table beside slgpu.h (whose codes, types and conventions hold here): the same library,
 * bound by the same _native.lib() from _native.AUDIT_EXPORTS.
 *
 * Vertices double [V * 3], triangles int32 [T * 3]; 0 < V < 2^31, 0 < 3 T <= 2^30.  A triangle with
 * two equal indices is degenerate and takes no part in anything below.  Every other triangle gives
 * its three undirected edges (min, max) as keys min << 32 | max, each with its position 3 t + e and a
 * direction bit (set when the winding goes max -> min); a stable radix sort puts equal keys into a
 * run with ascending positions.  A run of 1 is a boundary edge, of 2 a manifold edge (inconsistent
 * when both entries carry the same direction bit), of 3 or more a non-manifold edge.
 *
 * The workspace of stage SLG_AUDIT_WS_AUDIT serves slg_audit_edges, _components_count,
 * _components_emit and _fans, in that order or with steps left out, edges first.  Its first 256 bytes
 * are the header: int32 status at 0 (SLG_FILTER_BAD_INDEX: a triangle index outside 0 .. V - 1),
 * int64 nV at 8 (the referenced vertices), int64 nC at 24 (the components), int64 largest at 32 (the
 * triangles of the largest component) and, at byte 128, int64 stats[8] indexed by SLG_AUDIT_STAT_*.
 * The stages SLG_AUDIT_WS_MEASURE and SLG_AUDIT_WS_SELECT are workspaces of their own with the status
 * word at 0; slg_audit_select leaves the new nV at 8 and nT at 16.
 *
 *   slg_audit_edges        keys, sort, classes.  stats EDGES .. DUPLICATES; nV.  vertex_class_out
 *                          uint8 [V]: SLG_AUDIT_VERTEX_* bits (REFERENCED: by a triangle that is not
 *                          degenerate).  triangle_class_out uint8 [T]: SLG_AUDIT_TRIANGLE_* bits.
 *                          Triangle t with sorted indices (a, b, c) is a duplicate iff the run of
 *                          (a, b) holds, before t's own entry, a triangle whose third vertex is c.
 *   slg_audit_components_count   all triangles of a run are joined (a lock-free union-find whose
 *                          root is the smallest index); labels_out int32 [T]: the rank of the root
 *                          among roots, -1 for a degenerate triangle; nC.
 *   slg_audit_components_emit    sizes_out int64 [n_components] and the header's largest.
 *   slg_audit_fans         over the 3 T corners, per run the corners at min of its triangles are
 *                          joined and those at max; a vertex whose corners have more than one root
 *                          gets SLG_AUDIT_VERTEX_NONMANIFOLD in vertex_class (the array of
 *                          slg_audit_edges); stat NONMANIFOLD_VERTICES.
 *   slg_audit_measure      out[0] = sum of a . (b x c) / 6, out[1] = sum of 0.5 |(b - a) x (c - a)|
 *                          over the triangles that are not degenerate: SLG_AUDIT_CHUNK triangles per
 *                          workgroup, 8 consecutive per thread, the workgroup's binary tree, then the
 *                          partials the same way.  No floating atomics.
 *   slg_audit_keep         keep_out uint8 [T]: no bit of drop_bits in triangle_class[t] (NULL: none)
 *                          and, with a table uint8 [n_components], labels[t] >= 0 and table[labels[t]].
 *   slg_audit_select       the triangles with keep[t] != 0 in input order; with drop_unreferenced the
 *                          vertices they use in input order, else all; renumbered; densities (may be
 *                          NULL) carried.  Outputs are sized as the inputs; the header has the counts.
 *
 * Every kernel returns when the header's status is set.  SLG_ERR_INVALID for a NULL buffer, counts
 * out of range, an unknown stage, or a workspace that is NULL, misaligned or too small. */
#ifndef SLGPU_AUDIT_H
#define SLGPU_AUDIT_H

#include "slgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLG_AUDIT_WS_AUDIT 0
#define SLG_AUDIT_WS_MEASURE 1
#define SLG_AUDIT_WS_SELECT 2
#define SLG_AUDIT_CHUNK 2048
#define SLG_AUDIT_STAT_EDGES 0
#define SLG_AUDIT_STAT_BOUNDARY 1
#define SLG_AUDIT_STAT_MANIFOLD 2
#define SLG_AUDIT_STAT_NONMANIFOLD 3
#define SLG_AUDIT_STAT_INCONSISTENT 4
#define SLG_AUDIT_STAT_DEGENERATE 5
#define SLG_AUDIT_STAT_DUPLICATES 6
#define SLG_AUDIT_STAT_NONMANIFOLD_VERTICES 7
#define SLG_AUDIT_VERTEX_REFERENCED 1
#define SLG_AUDIT_VERTEX_BOUNDARY 2
#define SLG_AUDIT_VERTEX_NONMANIFOLD_EDGE 4
#define SLG_AUDIT_VERTEX_INCONSISTENT 8
#define SLG_AUDIT_VERTEX_NONMANIFOLD 16
#define SLG_AUDIT_TRIANGLE_DEGENERATE 1
#define SLG_AUDIT_TRIANGLE_DUPLICATE 2
int64_t slg_audit_ws_bytes(int32_t stage, int64_t n_vertices, int64_t n_triangles);
int32_t slg_audit_edges(const int32_t *triangles, int64_t n_triangles, int64_t n_vertices, void *ws, int64_t ws_bytes,
                        uint8_t *vertex_class_out, uint8_t *triangle_class_out, void *stream);
int32_t slg_audit_components_count(int64_t n_triangles, int64_t n_vertices, void *ws, int64_t ws_bytes,
                                   const uint8_t *triangle_class, int32_t *labels_out, void *stream);
int32_t slg_audit_components_emit(int64_t n_triangles, int64_t n_vertices, void *ws, int64_t ws_bytes,
                                  const int32_t *labels, int64_t n_components, int64_t *sizes_out, void *stream);
int32_t slg_audit_fans(const int32_t *triangles, int64_t n_triangles, int64_t n_vertices, void *ws, int64_t ws_bytes,
                       const uint8_t *triangle_class, uint8_t *vertex_class, void *stream);
int32_t slg_audit_measure(const double *vertices, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles,
                          void *ws, int64_t ws_bytes, double *out, void *stream);
int32_t slg_audit_keep(const uint8_t *triangle_class, const int32_t *labels, int64_t n_triangles, const uint8_t *table,
                       int64_t n_components, int32_t drop_bits, uint8_t *keep_out, void *stream);
int32_t slg_audit_select(const double *vertices, const double *densities, int64_t n_vertices, const int32_t *triangles,
                         int64_t n_triangles, const uint8_t *keep, int32_t drop_unreferenced, void *ws, int64_t ws_bytes,
                         double *vertices_out, double *densities_out, int32_t *triangles_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SLGPU_AUDIT_H */
