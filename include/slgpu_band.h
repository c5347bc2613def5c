/* slgpu_band.h -- the banded cascadic mesher's entry points of libslgpu.so (csrc/cloud_band.hip;
 * DESIGN.md §21): the watertight rule for depth 3..12.  A dense solve at a base depth carries the far
 * field (slgpu.h's slg_mesh_* calls); every finer level exists only in blocks of 8^3 cells near the
 * points, starts from the prolonged coarser solution and is smoothed by a fixed number of Jacobi
 * sweeps; the surface is extracted inside the finest band.  Our rule, Open3D parity unpinned; a pure
 * function of the cloud and its normals, restated in tests/band_ref.py.  Asynchronous on `stream`.
 *
 * A third table beside slgpu.h (whose codes, types and conventions hold here): the same library,
 * bound by the same _native.lib() from _native.BAND_EXPORTS.
 *
 * A level of R = 2^l cells per axis (8 <= R <= 4096) has nb = R / 8 blocks per axis.  Block b owns
 * the cells and the nodes [8 b, 8 b + 8) per axis, so the nodes 0 .. R fall into (nb + 1)^3 node
 * blocks, id (bz (nb + 1) + by) (nb + 1) + bx.  The caller holds per level:
 *
 *   hdr      256 bytes, 256-byte aligned: slgpu.h's mesh header (int32 status at 0, int32 R at 4,
 *            int64 nV at 8, nT at 16, double origin[3] at 24, h at 48, iso at 56) and, at byte 128,
 *            int64 stats[8] indexed by SLG_BAND_STAT_*.
 *   seed, active   uint8 [(nb+1)^3]: a point's cell lies in the block; it or one of its 26 neighbours
 *            is seeded (a cell is active when its block is).
 *   table    int32 [(nb+1)^3]: the rank, in ascending id, of a node block that holds a band node
 *            (one of the cell blocks b - {0,1}^3 is active), else -1.  The ranks number the stored
 *            blocks; a node field is double [n_blocks * 512], entry rank * 512 + (lz 8 + ly) 8 + lx.
 *   block_ids int32 [n_blocks], incident uint8 [n_blocks * 512]: a stored block's id; per node, bit
 *            ex + 2 ey + 4 ez is set when the cell at node - 1 + e is active.  A node is a band node
 *            when a bit is set and interior when all 8 are.
 *
 *   slg_band_level      the level's header from the base workspace's (slg_mesh_grid at the base
 *                       depth): status and origin copied, h = h_base / (R / base_R), counts 0.
 *   slg_band_blocks     seed, active and table; stats SEEDED, ACTIVE and NODE_BLOCKS.  The caller
 *                       reads the header (status, n_blocks) and sizes everything that follows.
 *   slg_band_nodes      block_ids and incident; stats BAND_NODES and INTERIOR_NODES.
 *   slg_band_splat      W and V (double [n_blocks * 512 (* 3)]) by §16's gather: per node its active
 *                       incident cells in ascending cell id, each cell's points in ascending input
 *                       index (a stable 64-bit radix sort by cell id, binary searches).
 *   slg_band_divergence f: §16's central differences at interior nodes, 0 elsewhere.
 *   slg_band_prolong    u = 0.125 * (0 + P(parent)) at band nodes off the box boundary, 0 elsewhere;
 *                       P is §16's prolongation.  parent_table NULL: the parent is the dense base
 *                       level [R/2+1]^3; else it is a banded level and parent_blocks its n_blocks.
 *   slg_band_smooth     `sweeps` Jacobi sweeps (omega = 6/7) over u and tmp in turn, one workgroup
 *                       per stored block through LDS: interior nodes update, every other stored
 *                       node keeps its value.  The result is in u when sweeps is even, else in tmp.
 *   slg_band_iso        hdr.iso = §16's tree sum of the trilinear chi at the points / n.
 *   slg_band_count      per stored node the 7-bit mask of its crossing owned edges that lie in an
 *                       active cell, per active cell its triangle count; two scans; hdr.nV, hdr.nT.
 *   slg_band_emit       vertices in ascending (block, local node, edge type) with the trilinear W
 *                       as density (a node outside the band reads as 0), triangles in ascending
 *                       (block, local cell, tetrahedron, triangle).
 *
 * Every kernel returns when hdr.status is set or n_blocks is not the header's count.
 * SLG_ERR_INVALID for a NULL or misaligned buffer, R no power of two in 8..4096, n <= 0, a count
 * outside its range or a workspace that is too small; SLG_ERR_UNSUPPORTED for more than 2^30 points
 * or 2^31 vertices or more. */
#ifndef SLGPU_BAND_H
#define SLGPU_BAND_H

#include "slgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLG_BAND_MIN_DEPTH 3
#define SLG_BAND_MAX_DEPTH 12
#define SLG_BAND_MAX_BASE_DEPTH 10
#define SLG_BAND_BLOCK 8
#define SLG_BAND_WS_BLOCKS 0
#define SLG_BAND_WS_SPLAT 1
#define SLG_BAND_WS_ISO 2
#define SLG_BAND_WS_EXTRACT 3
#define SLG_BAND_STAT_SEEDED 0
#define SLG_BAND_STAT_ACTIVE 1
#define SLG_BAND_STAT_NODE_BLOCKS 2
#define SLG_BAND_STAT_BAND_NODES 3
#define SLG_BAND_STAT_INTERIOR_NODES 4
int64_t slg_band_ws_bytes(int32_t stage, int32_t R, int64_t n, int64_t n_blocks);
int32_t slg_band_level(const void *base_ws, int32_t base_R, int32_t R, void *hdr, void *stream);
int32_t slg_band_blocks(const double *xyz, int64_t n, int32_t R, void *hdr, uint8_t *seed, uint8_t *active,
                        int32_t *table, void *ws, int64_t ws_bytes, void *stream);
int32_t slg_band_nodes(int32_t R, void *hdr, const uint8_t *active, const int32_t *table, int64_t n_blocks,
                       int32_t *block_ids, uint8_t *incident, void *stream);
int32_t slg_band_splat(const double *xyz, const double *normals, int64_t n, int32_t R, void *hdr, const uint8_t *seed,
                       const int32_t *table, const int32_t *block_ids, const uint8_t *incident, int64_t n_blocks,
                       void *ws, int64_t ws_bytes, double *W_out, double *V_out, void *stream);
int32_t slg_band_divergence(const double *V, int32_t R, const void *hdr, const int32_t *table, const int32_t *block_ids,
                            const uint8_t *incident, int64_t n_blocks, double *f_out, void *stream);
int32_t slg_band_prolong(const double *parent, const int32_t *parent_table, int64_t parent_blocks, int32_t R,
                         const void *hdr, const int32_t *block_ids, const uint8_t *incident, int64_t n_blocks,
                         double *u_out, void *stream);
int32_t slg_band_smooth(const double *f, int32_t R, const void *hdr, const int32_t *table, const int32_t *block_ids,
                        const uint8_t *incident, int64_t n_blocks, int32_t sweeps, double *u, double *tmp, void *stream);
int32_t slg_band_iso(const double *chi, const double *xyz, int64_t n, int32_t R, void *hdr, const int32_t *table,
                     int64_t n_blocks, void *ws, int64_t ws_bytes, void *stream);
int32_t slg_band_count(const double *chi, int32_t R, void *hdr, const int32_t *table, const int32_t *block_ids,
                       const uint8_t *incident, int64_t n_blocks, void *ws, int64_t ws_bytes, void *stream);
int32_t slg_band_emit(const double *chi, const double *W, int32_t R, const void *hdr, const int32_t *table,
                      const int32_t *block_ids, const uint8_t *incident, int64_t n_blocks, void *ws, int64_t ws_bytes,
                      double *vertices_out, int64_t n_vertices, double *densities_out, int32_t *triangles_out,
                      int64_t n_triangles, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SLGPU_BAND_H */
