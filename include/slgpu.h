/*
 * slgpu.h — C ABI of the MI355X (gfx950) structured-light reconstruction library.
 *
 * Drop-in boundary for the hot path of TtT609/Structured_Light_for_3D_Model_Replication.
 * The reference has no FFI: its boundary is the Python call surface, so each export below
 * replaces one reference function (cited), and the Python package
 * `structured_light_for_3d_model_replication_amd` binds these symbols with ctypes and keeps
 * the reference's signatures.
 *
 *   slg_decode_stats       <- mask thresholds of ProcessingLogic._gray_decode
 *                             (server/processing.py:59-78; Otsu / manual) and of
 *                             SLSystem.generate_cloud.gray_decode (server/sl_system.py:527-543;
 *                             95th-percentile / dynamic range)
 *   slg_decode             <- ProcessingLogic._gray_decode (server/processing.py:28-124) and
 *                             generate_cloud.gray_decode (server/sl_system.py:516-588)
 *   slg_triangulate        <- ProcessingLogic._reconstruct_point_cloud
 *                             (server/processing.py:127-234) and
 *                             generate_cloud.reconstruct_point_cloud (server/sl_system.py:592-661)
 *   slg_reconstruct        <- decode + triangulate of one view as run by
 *                             process_multi_ply._process_source (server/processing.py:286-298)
 *                             without materialising the correspondence maps
 *   slg_decode_triangulate <- the same without the stats launch (after slg_decode_stats)
 *   slg_reconstruct_batch  <- process_multi_ply(mode='batch') over view folders
 *                             (server/processing.py:314-334): many views, one stream
 *   slg_ply_write          <- ProcessingLogic._save_ply (server/processing.py:236-248), host side
 *   slg_ply_format         <- the same lines formatted on the device (batch pipeline)
 *   slg_png_gray8_size /   <- cv2.imread(f, 0) of an 8-bit grayscale capture frame
 *   slg_png_gray8_decode      (server/processing.py:59-60,98-99), host side fast path
 *   slg_rays_match_pinhole <- the `Nc.shape[1] == h*w` ray source test
 *                             (server/processing.py:143-156): tells whether the calibration's
 *                             Nc table equals the cam_K pinhole rays bit for bit, in which case
 *                             the kernels recompute rays instead of gathering 24 B/pixel.
 *
 * Conventions
 *   - All buffer pointers are DEVICE pointers owned by the caller (the library never
 *     allocates or frees caller memory); scratch lives in a caller-provided workspace of
 *     slg_workspace_bytes() bytes, zeroed once with slg_workspace_init().
 *   - No call depends on what its memory held before.  Every other workspace (the cloud steps'
 *     `ws`, the mesher's, the post-processing, decimation, PLY and PNG ones, the PNG `raw` scratch)
 *     and every output buffer is NOT initialised by the caller: a call writes what it later reads,
 *     clears on its own stream what its kernels accumulate into, and writes every entry of an
 *     output it documents (a prefix of `count` entries where it says so; what lies behind the
 *     prefix is unspecified).  The result is a pure function of the inputs whatever the bytes
 *     were: zeros, 0xFF, or another call's leftovers at another size.  The two exceptions: the
 *     per-view fused workspace above (zeroed once by slg_workspace_init, never by a call), and
 *     the arena cursor of slg_workspace_set_arena (the caller's counter, which the launches
 *     advance).  A step made of several calls (slg_ransac_prepare -> slg_ransac_batch,
 *     slg_plane_batch -> slg_plane_finish, the mesher's stages, count -> emit of the adjacency
 *     and of the holes, decimate init -> round -> emit) keeps its state in the workspace between
 *     its own calls: the workspace is free only before the first of them.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Every export only
 *     enqueues work (no host synchronisation), so calls can be captured into a hipGraph.
 *   - Return value: SLG_OK (0) or an SLG_ERR_* code; slg_last_error() returns a thread-local
 *     message for the last failing call on the calling thread.
 *   - Frames: uint8 [n_frames][frame_stride] planar stack in capture order (index 0 white,
 *     1 black, then (pattern, inverse) per column bit MSB-first, then per row bit starting
 *     at 2 + 2*ceil(log2(proj_cols))).  frame_stride % 8 == 0 and >= round_up(H*W, 8)
 *     (every frame row is readable in whole 8-byte words), base 8-byte aligned.
 *   - Points are written in ascending pixel order (np.where(mask) order); row_mode 2 writes
 *     the column cloud then the row cloud, like np.hstack((P_col, P_row)).
 */
#ifndef SLGPU_H
#define SLGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLG_ABI_VERSION 2

#define SLG_OK 0
#define SLG_ERR_INVALID 1      /* bad argument (message in slg_last_error) */
#define SLG_ERR_HIP 2          /* HIP runtime / launch error */
#define SLG_ERR_UNSUPPORTED 3  /* e.g. more than 15 code bits per axis */
#define SLG_ERR_NOT_ENOUGH 4   /* fewer than 4 frames (reference: ValueError) */
#define SLG_ERR_INDEX 5        /* odd trailing frame in the sl_system variant (IndexError) */

/* thresh_mode */
#define SLG_THRESH_OTSU 0        /* processing.py:63-72 */
#define SLG_THRESH_MANUAL 1      /* processing.py:73-76 */
#define SLG_THRESH_PERCENTILE 2  /* sl_system.py:534-540 */

/* variant */
#define SLG_VARIANT_PROCESSING 0 /* ProcessingLogic._gray_decode: first-n bits, rescaled */
#define SLG_VARIANT_SLSYSTEM 1   /* generate_cloud.gray_decode: all bits, break on missing */

/* ray_mode */
#define SLG_RAYS_TABLE 0         /* gather Nc[:, idx] (processing.py:143-144) */
#define SLG_RAYS_PINHOLE 1       /* recompute from cam_K (processing.py:145-156) */

/* Limits (SLG_ERR_UNSUPPORTED otherwise): height*width < 1.43e9 and n_frames*frame_stride
 * < 4 GiB -- the kernels address frames and texture with 32-bit buffer offsets. */
typedef struct slg_capture {
  const uint8_t *frames;   /* device, [n_frames][frame_stride] */
  int64_t frame_stride;    /* bytes between frames (>= round_up(height*width, 8), % 8 == 0) */
  int32_t n_frames;        /* frames present (len(files)) */
  int32_t height;
  int32_t width;
  int32_t reserved;
  const uint8_t *texture;  /* device, [height*width][3] BGR (cv2.imread(files[0])), or NULL for a
                              gray capture: BGR = frame 0 replicated, what cv2.imread(files[0])
                              returns for an 8-bit gray PNG (no texture bytes are then read) */
} slg_capture;

typedef struct slg_decode_params {
  int32_t proj_cols;       /* n_cols  (processing.py:28) */
  int32_t proj_rows;       /* n_rows */
  int32_t n_sets_col;      /* processing variant only (processing.py:83) */
  int32_t n_sets_row;
  int32_t variant;         /* SLG_VARIANT_* */
  int32_t thresh_mode;     /* SLG_THRESH_* */
  double shadow_val;       /* manual: compared as double; pass float32-rounded values for */
  double contrast_val;     /* NumPy-2 weak-scalar semantics (the Python layer does this) */
} slg_decode_params;

typedef struct slg_calib {
  const double *rays;      /* device (3, height*width) C-contiguous, or NULL (SLG_RAYS_PINHOLE) */
  int32_t ray_mode;        /* SLG_RAYS_* */
  int32_t reserved;
  double fx, fy, cx, cy;   /* cam_K[0,0], cam_K[1,1], cam_K[0,2], cam_K[1,2] */
  double oc[3];            /* Oc (always 0 from calibrate_final, sl_system.py:355) */
  const double *col_planes;/* device (n_col_planes, 4) row-major = wPlaneCol.T */
  int32_t n_col_planes;
  int32_t reserved2;
  const double *row_planes;/* device (n_row_planes, 4) row-major = wPlaneRow.T */
  int32_t n_row_planes;
  int32_t reserved3;
  /* Optional (NULL: the kernels compute numer per point; same values either way): */
  const double *col_planes_num; /* device (2, n_col_planes, 2) "pair planes": [0][c] = (n0, n1),
                                 * [1][c] = (n2, numer), numer = ((n0*Oc0 + n1*Oc1) + n2*Oc2) + d
                                 * (processing.py:163-166), so a wave's neighbouring column codes
                                 * gather neighbouring 16-byte pairs */
  const double *row_planes_num; /* the same for the row planes (read by row_mode 2 only) */
} slg_calib;

typedef struct slg_tri_params {
  int32_t row_mode;        /* 0 col only, 1 epipolar filter, 2 col+row clouds (processing.py:174-234) */
  int32_t xyz_f64;         /* 1: XYZ float64 (bit-exact with the reference); 0: float32 */
  double epipolar_tol;     /* processing.py:199 */
} slg_tri_params;

typedef struct slg_maps {
  const int32_t *col;      /* device [height*width] */
  const int32_t *row;      /* device [height*width] (may be NULL for row_mode 0) */
  const uint8_t *mask;     /* device [height*width] bool */
  const uint8_t *texture;  /* device [height*width][3] BGR */
  int32_t height;
  int32_t width;
} slg_maps;

typedef struct slg_cloud {
  void *xyz;               /* device [capacity][3] float or double */
  uint8_t *bgr;            /* device [capacity][3] */
  int64_t *count;          /* device, 1 element: number of points written */
  int64_t capacity;        /* >= height*width (row_mode 0/1) or 2*height*width (row_mode 2) */
} slg_cloud;

int32_t slg_version(void);
const char *slg_last_error(void);
/* Digest of the sources and flags this library was built from (build.py: sha256 of every
 * source, the header and the compile flags); _native.lib() refuses a library whose digest does
 * not match the sources beside it. */
const char *slg_build_id(void);
/* The fused kernel's instance table, one line per instance ("<symbol>\t<0|1>\n", 1 = its device
 * code is in the library's gfx950 code object) into buf (cap bytes, NUL-terminated; truncated
 * lines are dropped).  Returns the number of instances missing, or -SLG_ERR_INVALID.  Launches
 * of a missing instance return SLG_ERR_UNSUPPORTED instead of reaching the HIP runtime, which
 * aborts on them.  Reads the library file only (no HIP call). */
int32_t slg_kernel_table(char *buf, int64_t cap);
/* The symbol of the fused kernel instance that the calling thread's last fused launch picked from
 * that table, into buf (cap bytes, NUL-terminated); "" when the thread has picked none, or its last
 * pick found no instance.  A test hook: the GPU suite checks that every instance of the table runs and
 * matches the oracle.  Host only (no HIP call). */
int32_t slg_last_kernel(char *buf, int64_t cap);

/* Workspace size for images of n_pixels (covers every mode). */
int64_t slg_workspace_bytes(int64_t n_pixels);
/* Zero a freshly allocated workspace (once; the kernels keep it consistent afterwards). */
int32_t slg_workspace_init(void *workspace, int64_t workspace_bytes, void *stream);

/* Resident jobs (jobs.ResidentJob): bind n_slices workspace slices (ws_stride apart) to one
 * packed output arena of capacity_points points.  From then on, whichever kernel sets a slice's
 * thresholds (stats, partials, a fused launch's finishing workgroups) also reserves the view's
 * region: atomicAdd(*cursor, need) with need = min(#white >= smin, #(white - black) >= cmin) x
 * points_per_valid (1: row_mode 0/1, 2: row_mode 2) -- an upper bound of the view's points -- so
 * no view can write past its region; no room left: the view stores nothing.  The fused launches
 * then take every bound slice's cloud (slg_cloud) as: xyz / bgr = the arena's base, capacity =
 * the arena's, count -> int64[2] = {points, first point index in the arena or -1 (no room: re-run
 * the view)}.  The caller zeroes *cursor (device int64) before each job; cursor NULL unbinds.
 * Asynchronous on `stream`. */
int32_t slg_workspace_set_arena(void *workspace, int64_t ws_stride, int32_t n_slices, int64_t *cursor,
                                int64_t capacity_points, int32_t points_per_valid, void *stream);

/* Histograms + thresholds of the valid mask into the workspace; also arms the workspace for
 * the next slg_decode / slg_reconstruct on the same stream. */
int32_t slg_decode_stats(const slg_capture *cap, const slg_decode_params *dp, void *workspace,
                         void *stream);

/* One view split over ranks by bands of rows ("single huge view"; its one exchange
 * step).  slg_decode_histograms writes the band's mask histograms, summed over the band, to
 * hist_out (device uint32[513]): Otsu -> [0..255] white, [256..511] clip(white - black, 0, 255)
 * (processing.py:63-72); percentile -> [0..255] black, [512] = max(white - black) + 256
 * (sl_system.py:534-540).  The ranks add [0..511] and take the max of [512] (RCCL all-reduce);
 * slg_thresholds_from_histograms then sets this band's workspace thresholds from the view's
 * totals (n_pixels = the whole view's, so the thresholds are the unsplit view's, bit for bit) and
 * arms it for slg_decode_triangulate of the band (n_band_pixels).  Manual thresholds need no
 * exchange: slg_decode_stats on the band.  Each band's cloud is its rows' points in pixel order,
 * so rank-ordered concatenation is the view's cloud (row_mode 2: every band's column cloud, then
 * every band's row cloud). */
int32_t slg_decode_histograms(const slg_capture *cap, const slg_decode_params *dp, void *workspace,
                              uint32_t *hist_out, void *stream);
int32_t slg_thresholds_from_histograms(const uint32_t *hist, int64_t n_pixels, const slg_decode_params *dp,
                                       void *workspace, int64_t n_band_pixels, void *stream);

/* Gray decode to correspondence maps (after slg_decode_stats on the same workspace). */
int32_t slg_decode(const slg_capture *cap, const slg_decode_params *dp, void *workspace,
                   int32_t *col_out, int32_t *row_out, uint8_t *mask_out, void *stream);

/* Ray-plane triangulation + ordered compaction from maps.  Arms the workspace itself. */
int32_t slg_triangulate(const slg_maps *maps, const slg_calib *calib, const slg_tri_params *tp,
                        void *workspace, const slg_cloud *out, void *stream);

/* Fused: stats + decode + triangulate + compaction of one view (maps never hit HBM). */
int32_t slg_reconstruct(const slg_capture *cap, const slg_decode_params *dp,
                        const slg_calib *calib, const slg_tri_params *tp, void *workspace,
                        const slg_cloud *out, void *stream);

/* The fused decode+triangulate launch alone (slg_reconstruct minus the stats launch): call
 * after slg_decode_stats on the same workspace and stream. */
int32_t slg_decode_triangulate(const slg_capture *cap, const slg_decode_params *dp,
                               const slg_calib *calib, const slg_tri_params *tp, void *workspace,
                               const slg_cloud *out, void *stream);

/* A batch of views of one geometry (turntable scan, scan farm; frame counts may differ):
 * per group of up to 16 views, one batched stats launch and ONE fused decode+triangulate launch
 * covering every view of the group (no host sync).  `workspace` holds n_views slices of
 * `ws_stride` bytes (>= slg_workspace_bytes, % 256 == 0), each initialised once; outs[v]
 * receives view v.  timing_events (optional: NULL, or 2 hipEvent_t / NULL entries per group of
 * 16 views) are recorded around each fused launch. */
int32_t slg_reconstruct_batch(const slg_capture *caps, int32_t n_views, const slg_decode_params *dp,
                              const slg_calib *calib, const slg_tri_params *tp, void *workspace,
                              int64_t ws_stride, const slg_cloud *outs, void *const *timing_events,
                              void *stream);

/* The two halves of slg_reconstruct_batch, so a caller can run the stats of the next batch on a
 * second stream while this batch's fused launch runs (each view's workspace slice must not be
 * shared between the two batches in flight). */
int32_t slg_decode_stats_batch(const slg_capture *caps, int32_t n_views, const slg_decode_params *dp,
                               void *workspace, int64_t ws_stride, void *stream);
int32_t slg_decode_triangulate_batch(const slg_capture *caps, int32_t n_views, const slg_decode_params *dp,
                                     const slg_calib *calib, const slg_tri_params *tp, void *workspace,
                                     int64_t ws_stride, const slg_cloud *outs, void *const *timing_events,
                                     void *stream);

/* Streaming turntable batches (thresh_mode OTSU only): the fused launch of batch k also
 * computes the Otsu histograms of batch k+2 (`next`, n_next <= n_views views, same geometry),
 * one 1 KB partial per 2048-pixel tile in each view's workspace slice; no separate pass over
 * the white/black frames of batch k+2 is needed.  Batch k+2 must then use the SAME workspace
 * slices as batch k, and slg_decode_stats_partials_batch on them (after this launch, before
 * batch k+2's fused launch; it may overlap batch k+1's) turns the partials into thresholds and
 * arms the slices for batch k+2.  Results are identical to slg_decode_stats_batch. */
int32_t slg_decode_triangulate_batch_next(const slg_capture *caps, int32_t n_views,
                                          const slg_decode_params *dp, const slg_calib *calib,
                                          const slg_tri_params *tp, void *workspace, int64_t ws_stride,
                                          const slg_cloud *outs, const slg_capture *next,
                                          int32_t n_next, void *const *timing_events, void *stream);
int32_t slg_decode_stats_partials_batch(int32_t n_views, int32_t height, int32_t width,
                                        const slg_decode_params *dp, void *workspace,
                                        int64_t ws_stride, void *stream);

/* The streaming turntable pipeline on ONE stream (what BatchReconstructor.run_pipelined
 * "fused" issues): slg_decode_triangulate_batch_next, plus `n_fin` views whose partials an
 * EARLIER launch on this stream carried (slices at fin_workspace + v * ws_stride) turned into
 * thresholds by finishing workgroups at the front of this launch's grid -- the work of
 * slg_decode_stats_partials_batch without its kernel or a second stream.  Batch k's launch
 * carries batch k+2 and finishes batch k+1; fin_workspace must not be this launch's own
 * workspace.  The finished batch must share this launch's geometry (height, width) and decode
 * parameters `dp` (its slices are read with them; nothing else identifies it).  ws_stride must
 * be >= slg_workspace_bytes and 256-aligned whenever n_views, n_next or n_fin exceeds 1.
 * Results are identical to slg_decode_stats_batch. */
int32_t slg_decode_triangulate_batch_carry(const slg_capture *caps, int32_t n_views,
                                           const slg_decode_params *dp, const slg_calib *calib,
                                           const slg_tri_params *tp, void *workspace, int64_t ws_stride,
                                           const slg_cloud *outs, const slg_capture *next,
                                           int32_t n_next, void *fin_workspace, int32_t n_fin,
                                           void *const *timing_events, void *stream);

/* Count (into *mismatches, device int64) the Nc entries that differ bitwise from the cam_K
 * pinhole rays; 0 means SLG_RAYS_PINHOLE reproduces the table exactly. */
int32_t slg_rays_match_pinhole(const double *rays, int32_t height, int32_t width, double fx,
                               double fy, double cx, double cy, int64_t *mismatches,
                               void *stream);

/* Colour captures (the phone path: canvas PNGs uploaded by frontend/App.tsx:234-247 and saved
 * as-is by server/server.py:86) on the device, from ONE upload of the decoded frames:
 * gray[f][i] = cv2.imread(f, 0) of rgb frame f (RGB or RGBA bytes, `channels` 3|4, frame f at
 * rgb + f * src_stride) into a frame stack of gray_stride, and, when bgr0 is not NULL, frame 0
 * as the BGR texture cv2.imread(files[0]) returns.  weights: libpng's rgb_to_gray fixed point
 * (PNG) or OpenCV's BGR2GRAY weights (BMP) -- restated from the libraries' published formulas,
 * parity unpinned (no OpenCV here).  Replaces the host conversion of frames.py. */
#define SLG_GRAY_PNG 0
#define SLG_GRAY_BMP 1
int32_t slg_rgb_to_gray(const uint8_t *rgb, int32_t channels, int64_t n_pixels, int64_t src_stride,
                        int32_t n_frames, uint8_t *gray, int64_t gray_stride, uint8_t *bgr0,
                        int32_t weights, void *stream);
/* Texture of a gray capture (cv2.imread(files[0]) of an 8-bit gray PNG: frame 0 replicated to
 * B, G, R) built on the device from the uploaded frame 0: no host replication, no extra upload. */
int32_t slg_gray_texture(const uint8_t *frame0, int64_t n_pixels, uint8_t *bgr, void *stream);

/* Host: write an ASCII PLY exactly as ProcessingLogic._save_ply does (processing.py:236-248):
 * header, then "%.4f %.4f %.4f R G B" per point (Python's correctly rounded formatting, BGR
 * swapped to RGB).  xyz/bgr are HOST arrays [n][3].  Formats on n_threads host threads
 * (<= 0: all cores).  Returns bytes written, or -SLG_ERR_* on failure. */
int64_t slg_ply_write(const char *path, const double *xyz, const uint8_t *bgr, int64_t n,
                      int32_t n_threads);

/* Device: the BODY of the same PLY (the lines after end_header), formatted on the GPU from a
 * DEVICE cloud (xyz float64 [n][3], bgr uint8 [n][3]) into DEVICE `text`, so a batch's clouds
 * leave HBM as the bytes to write (processing.py:245-248; byte-identical with slg_ply_write).
 * `text` holds slg_ply_format_bound(n) bytes, `ws` slg_ply_format_ws_bytes(n) bytes (device).
 * Asynchronous on `stream`; afterwards ws holds {int64 body_bytes; int32 bad; int32 pad}: bad
 * != 0 means a coordinate is NaN, infinite or >= 9.2e14 in magnitude, the body is not written,
 * and the caller formats on the host (slg_ply_write).  Returns 0 or SLG_ERR_*. */
int64_t slg_ply_format_bound(int64_t n);
int64_t slg_ply_format_ws_bytes(int64_t n);
int32_t slg_ply_format(const double *xyz, const uint8_t *bgr, int64_t n, char *text, void *ws, void *stream);

/* Host: frame ingest fast path for cv2.imread(f, 0) (processing.py:59-60,98-99) on 8-bit
 * grayscale, non-interlaced PNGs, where it is the identity on the stored samples.
 * slg_png_gray8_size returns 0 and the size for such a file, non-zero for any other file
 * (decode it the general way).  slg_png_gray8_decode fills out[height][width]; non-zero on a
 * CRC error, a truncated stream or a size mismatch.  Thread-safe (one call per decode thread). */
int32_t slg_png_gray8_size(const char *path, int32_t *width, int32_t *height);
int32_t slg_png_gray8_decode(const char *path, uint8_t *out, int64_t cap, int32_t width,
                             int32_t height);

/* Host: any other PNG (colour, gray + alpha, palette, 1-16 bits, Adam7) decoded to exactly what
 * OpenCV's PNG decoder returns: cv2.imread(f, 0) into gray[height][width] and / or cv2.imread(f)
 * into bgr[height][width][3] (either may be NULL; caps in bytes).  OpenCV converts through libpng
 * (png_set_strip_16, png_set_strip_alpha, png_set_palette_to_rgb, png_set_expand_gray_1_2_4_to_8,
 * then png_set_bgr / png_set_gray_to_rgb / png_set_rgb_to_gray(png, 1, 0.299, 0.587)); that
 * arithmetic -- gamma tables of gAMA / sRGB files included -- is restated, pinned byte for byte
 * to libpng 1.6.37 (tests/test_png_color.py), and the files whose colour handling libpng decides
 * from data not restated (iCCP profiles, duplicate / invalid / disagreeing gAMA and sRGB) go
 * through the system libpng itself.  info[7]: {width, height, colour type, bit depth, interlace,
 * restated (1) or libpng (0), decoded by libpng (1)}.  slg_png_info fills info[0..5] only.
 * Return 0, else non-zero (unreadable, corrupt or unsupported: cv2.imread would return None).
 * Thread-safe. */
int32_t slg_png_info(const char *path, int32_t *info /* [6] */);
int32_t slg_png_read(const char *path, uint8_t *gray, int64_t gray_cap, uint8_t *bgr, int64_t bgr_cap,
                     int32_t *info /* [7] */);

/* PNG decode on the device (the same cv2.imread of every used frame, for the batch file path):
 * the host only reads the file and checks its chunks, the GPU inflates and un-filters.
 * slg_png_zstream (host): for an 8-bit, non-interlaced PNG of colour type 0 (gray), 2 (RGB),
 * 4 (gray + alpha) or 6 (RGBA) -- a colour one only without gAMA / sRGB / iCCP chunks, whose
 * gray conversion (libpng's gamma path) is slg_png_read's -- copies the concatenated IDAT payload (the zlib stream) into
 * buf (cap bytes; needs zlen + 8, the file size + 8 always suffices) and fills info[4] =
 * {width, height, channels, zlen}; returns 0, else non-zero (any other file, a CRC error, cap
 * too small: decode it the general way).  Thread-safe.
 * slg_png_decode_device: decodes n frames (DEVICE descriptors `frames`, each naming DEVICE
 * buffers: z = the zlib stream as read by slg_png_zstream, 4-byte aligned and readable for
 * zlen + 8 bytes; raw = scratch of slg_png_raw_bytes(w, h, ch) bytes; out = the samples,
 * [height][out_pitch] rows of width * channels bytes).  status is DEVICE int32 [2 * n]:
 * status[2f] = 0 or SLG_PNG_E_* (a frame with a non-zero status is left unspecified and must
 * be decoded on the host), status[2f + 1] internal.  Asynchronous on `stream`; returns 0 or SLG_ERR_*. */
#define SLG_PNG_E_STREAM 1     /* not a valid zlib/deflate stream (or reads past zlen); also a stored
                                  block longer than what is left of the image (its LEN is refused
                                  before any of its bytes is taken) */
#define SLG_PNG_E_SIZE 2       /* inflated size differs from height * (1 + width * channels): the
                                  stream ends short, or a literal or a copy would pass the end */
#define SLG_PNG_E_ADLER 3      /* Adler-32 of the inflated bytes differs from the stream's */
#define SLG_PNG_E_FILTER 4     /* a scanline filter type byte > 4 */
#define SLG_PNG_E_UNSUPPORTED 5 /* rows wider than the device un-filter takes (width * channels > 24576) */
typedef struct slg_png_frame {
  const uint8_t *z;        /* zlib stream (device) */
  int64_t zlen;
  uint8_t *raw;            /* scratch (device), slg_png_raw_bytes() */
  uint8_t *out;            /* samples (device) */
  int64_t out_pitch;       /* bytes between output rows (>= width * channels) */
  int32_t width, height, channels, reserved;
} slg_png_frame;
int32_t slg_png_zstream(const char *path, uint8_t *buf, int64_t cap, int32_t *info /* [4] */);
int64_t slg_png_raw_bytes(int32_t width, int32_t height, int32_t channels);
int32_t slg_png_decode_device(const slg_png_frame *frames, int32_t n, int32_t *status, void *stream);
/* A stream for the device PNG decode that leaves CUs free (hipExtStreamCreateWithCUMask): every
 * `reserve_every`-th CU of the current device is left out of its mask, so a long inflate launch
 * (one 50 KB-LDS wave per stream, ~225 ms) cannot occupy every CU and the batch pipeline's fused
 * launches of host-decoded views keep running beside it.  *stream = the hipStream_t; returns 0
 * or SLG_ERR_*.  slg_stream_destroy releases it. */
int32_t slg_stream_create_reserving(int32_t reserve_every, void **stream);
int32_t slg_stream_destroy(void *stream);

/* ---- Multi-GPU: the final point-cloud gather of a view-sharded scan.
 * Replaces nothing in the reference (its batch loop is serial, server/processing.py:314-334);
 * it is the one collective of the sharded path: after every rank has reconstructed its block
 * of turntable views, the clouds move to one rank over RCCL (xGMI), exact sizes only.
 * RCCL is resolved at run time (the librccl.so.1 already in the process, e.g. torch's).
 *   1. rank 0: slg_gather_unique_id(id); the caller distributes the 128 bytes (e.g. a
 *      torch.distributed broadcast);  every rank: slg_gather_init(&comm, n_ranks, rank, id),
 *      with its HIP device current;
 *   2. slg_gather_counts: all-gather of n_per_rank int64 counts per rank (device buffers,
 *      all_counts = [n_ranks][n_per_rank]); the caller reads them to size the root's buffer;
 *   3. slg_gatherv: rank r's send_bytes land at root's recv + sum(recv_bytes[:r]) (recv and the
 *      HOST array recv_bytes[n_ranks] are read on the root only); grouped point-to-point;
 *   4. slg_gather_destroy.  All calls enqueue on `stream` (hipStream_t). */
#define SLG_GATHER_ID_BYTES 128
typedef struct slg_gather_comm slg_gather_comm;
int32_t slg_gather_unique_id(uint8_t *id /* [SLG_GATHER_ID_BYTES] */);
int32_t slg_gather_init(slg_gather_comm **comm, int32_t n_ranks, int32_t rank, const uint8_t *id);
int32_t slg_gather_counts(slg_gather_comm *comm, const int64_t *counts, int32_t n_per_rank,
                          int64_t *all_counts, void *stream);
int32_t slg_gatherv(slg_gather_comm *comm, const void *send, int64_t send_bytes, void *recv,
                    const int64_t *recv_bytes, int32_t root, void *stream);
int32_t slg_gather_destroy(slg_gather_comm *comm);
/* Host only, no RCCL: the plan slg_gatherv follows.  On the root (rank == root): checks
 * recv_bytes (non-negative, recv_bytes[root] == send_bytes), writes offsets[n_ranks + 1] (rank
 * r lands at recv + offsets[r], offsets[n_ranks] = total) and recv_from[n_ranks] (1 = a
 * point-to-point receive from that peer; 0 for the root, whose own part is a device copy, and
 * for zero-byte peers).  On other ranks: recv_from[0] = 1 when the rank sends (send_bytes > 0),
 * offsets untouched.  Returns the number of point-to-point operations this rank issues, or a
 * negative SLG_ERR_* code (slg_last_error() says why). */
int32_t slg_gatherv_plan(int32_t n_ranks, int32_t rank, int32_t root, int64_t send_bytes,
                         const int64_t *recv_bytes, int64_t *offsets, int32_t *recv_from);

/* ---- Point-cloud cleanup on the device (csrc/cloud_grid.hip, cloud_filter.hip,
 * cloud_cluster.hip): the three deterministic neighbour steps of the reference's cleanup tab (two filters, and DBSCAN with the largest-cluster
 * pick: slg_dbscan, below), on a packed DEVICE cloud (xyz float64 [n][3]), so a reconstructed view
 * is cleaned without leaving HBM.
 *   slg_radius_outlier      <- ProcessingLogic.remove_radius_outlier (server/processing.py:430-448)
 *   slg_statistical_outlier <- ProcessingLogic.remove_outliers (server/processing.py:367-388,620)
 *   slg_cloud_select        <- the select_by_index that follows either (ascending indices)
 * Semantics (Open3D's RemoveRadiusOutliers / RemoveStatisticalOutliers as published, restated;
 * parity with an installed Open3D is unpinned), all in fp64 with d2 = (dx*dx + dy*dy) + dz*dz:
 *   radius:      counts[i] = #{j : d2(i, j) < radius*radius} (i included, strict);
 *                keep[i] = counts[i] > nb_points.
 *   statistical: avg[i] = (sum of sqrt of the min(k, n) smallest d2(i, j), i included, ascending)
 *                / min(k, n);  mean = (sum of avg > 0) / n;  std = sqrt(sum over avg > 0 of
 *                (avg - mean)^2 / (n - 1));  thr = mean + std_ratio * std;
 *                keep[i] = avg[i] > 0 && avg[i] < thr.  The two sums are fixed trees over the input
 *                order (no atomics): the same input gives the same bits.  k <= 64
 *                (SLG_ERR_UNSUPPORTED above).
 * `ws` is DEVICE scratch of slg_filter_ws_bytes(n, k) bytes (k = 0 when only the radius filter
 * and the select use it), 8-byte aligned, not initialised by the caller.  keep_out is uint8 [n]
 * in input order; counts_out (int32 [n]) and avg_out (float64 [n]) may be NULL; stats_out is
 * float64 [3] = {mean, std, thr} or NULL.  Asynchronous on `stream`, no host synchronisation.
 * Afterwards the int32 at the front of ws is 0, or SLG_FILTER_BAD_* bits: a coordinate is NaN or
 * infinite, or the cloud spans 2^21 or more cells of `radius` on an axis; the outputs are then
 * unspecified (nothing faults), as with slg_ply_format's `bad`.  After slg_statistical_outlier
 * the int32 at byte 8 of ws is the number of points whose neighbour search left the grid walk
 * (isolated points) for the whole-cloud kernel.
 * slg_cloud_select packs the points with keep != 0, in input order, into out (xyz float64, bgr;
 * bgr / out->bgr may be NULL; *out->count = points written, at most out->capacity) and their
 * input indices into index_out (int64 [n] or NULL).  It uses ws but leaves the status word.
 *
 *   slg_dbscan              <- PointCloud.cluster_dbscan + the largest-label pick of
 *                              ProcessingLogic.keep_largest_cluster (server/processing.py:391-427)
 * Semantics (Open3D's ClusterDBSCAN as published, restated in closed form; the labels are a pure
 * function of the input): with the radius filter's counts at radius = eps,
 *   core[i] = counts[i] >= min_points;  two core points are linked when d2 < eps*eps;  a cluster's
 *   core set is a connected component of that graph;  components are numbered 0..n_clusters-1 in
 *   ascending order of their smallest input index;  a non-core point takes the lowest label among
 *   its core neighbours, or -1 (noise) when it has none.
 *   Largest cluster: the label with the most members (core and border), the lowest label among
 *   equals, -1 when there is no cluster;  largest_keep[i] = labels[i] == that label (all 0 when
 *   there is none).
 * ws is slg_filter_ws_bytes(n, 0) bytes; labels_out is int32 [n] in input order;
 * largest_keep_out (uint8 [n]) and info_out (int32 [4] = n_clusters, largest_label,
 * largest_count, n_noise) may be NULL.  Asynchronous on `stream`, no host synchronisation; the
 * status word at the front of ws as for slg_radius_outlier (radius = eps).  SLG_ERR_INVALID for
 * n <= 0, eps <= 0 or NaN, min_points < 0, or a NULL xyz, labels_out or ws; SLG_ERR_UNSUPPORTED
 * above 2^30 points. */
#define SLG_FILTER_BAD_NONFINITE 1
#define SLG_FILTER_BAD_EXTENT 2
#define SLG_FILTER_BAD_INDEX 4      /* slg_ransac_batch: a correspondence names a point outside its cloud */
int64_t slg_filter_ws_bytes(int64_t n, int32_t k);
int32_t slg_radius_outlier(const double *xyz, int64_t n, double radius, int32_t nb_points, void *ws,
                           int64_t ws_bytes, uint8_t *keep_out, int32_t *counts_out, void *stream);
int32_t slg_statistical_outlier(const double *xyz, int64_t n, int32_t nb_neighbors, double std_ratio,
                                void *ws, int64_t ws_bytes, uint8_t *keep_out, double *avg_out,
                                double *stats_out, void *stream);
int32_t slg_cloud_select(const double *xyz, const uint8_t *bgr, int64_t n, const uint8_t *keep,
                         const slg_cloud *out, int64_t *index_out, void *ws, void *stream);
int32_t slg_dbscan(const double *xyz, int64_t n, double eps, int32_t min_points,
                   void *ws, int64_t ws_bytes,
                   int32_t *labels_out,          /* [n]: -1 noise, else 0..n_clusters-1 */
                   uint8_t *largest_keep_out,    /* [n] or NULL */
                   int32_t *info_out,            /* [4] or NULL: n_clusters, largest_label, largest_count, n_noise */
                   void *stream);

/* ---- Voxel down-sample, normals, orientation and centroid on the device cloud
 * (csrc/cloud_normals.hip): the Open3D operations of the tail of merge_pro_360
 * (server/processing.py:605-628) and of the front of both meshing methods (:653-670, :804-837).
 * Open3D's published rules restated, fp64, no floating-point atomics: the same input gives the
 * same bits.  ws, where a function takes one, is slg_filter_ws_bytes(n, 0) bytes; asynchronous on
 * `stream`, no host synchronisation; the status word at the front of ws as for the filters
 * (slg_voxel_downsample and slg_estimate_normals set it).
 *
 *   slg_voxel_downsample    <- PointCloud.voxel_down_sample(voxel_size)
 * vmin = min_bound - voxel_size * 0.5 per axis; a point's voxel is floor((p - vmin) / voxel_size)
 * (IEEE subtraction and division).  A voxel's point is, per axis, the sum of its members'
 * coordinates taken left to right in ascending input index, divided by their number; its colour
 * is per channel (2 * sum + count) / (2 * count) in integers (the exact mean, half up).  Voxels
 * come out in ascending order of their smallest member index (our rule: Open3D's order is that of
 * a hash map).  xyz_out float64 [n][3]; bgr / bgr_out uint8 [n][3] or NULL; first_index_out
 * int64 [n] (the smallest member index) and count_out int32 [n] or NULL; *m_out (DEVICE int64) =
 * the number of voxels, which is how many entries of each output are written.  A span of 2^21 or
 * more voxels on an axis sets SLG_FILTER_BAD_EXTENT.
 *
 *   slg_estimate_normals    <- PointCloud.estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))
 * Neighbours of i: all points in ascending (d2, input index) order, i included; the first
 * min(max_nn, n) of them; of those the ones with d2 < radius * radius (strict).  m = their number.
 * Nine sums over them in that order (x, y, z, xx, xy, xz, yy, yz, zz), each divided by m, then
 * cov_ab = E[ab] - E[a] * E[b].  The normal is the unit eigenvector of cov's smallest eigenvalue,
 * signed so that the first non-zero of (nz, ny, nx) is positive; (0, 0, 1) when m < 3 or cov is
 * identically zero.  normals_out float64 [n][3]; cov_out float64 [n][6] (xx, xy, xz, yy, yz, zz)
 * and m_out int32 [n] may be NULL.  3 <= max_nn <= 64 (SLG_ERR_UNSUPPORTED above).  Afterwards the
 * int32 at byte 8 of ws counts the points that left the grid walk for the whole-cloud kernel.
 *
 *   slg_orient_normals      <- orient_normals_towards_camera_location(location) [then * -1.0]
 * normals[i] is negated when normals[i] . (location - xyz[i]) < 0; with outward != 0 every normal
 * is negated afterwards.  `location` is DEVICE float64 [3].  In place.
 *
 *   slg_cloud_centroid      <- PointCloud.get_center() / points.mean(axis=0)
 * centroid_out (DEVICE float64 [3]) = per-axis sum / n, the sum a fixed tree over the input order.
 *
 * SLG_ERR_INVALID for n <= 0, a size that is not finite and > 0, max_nn < 3 or a NULL required
 * buffer; SLG_ERR_UNSUPPORTED above 2^30 points. */
int32_t slg_voxel_downsample(const double *xyz, const uint8_t *bgr, int64_t n, double voxel_size,
                             void *ws, int64_t ws_bytes, double *xyz_out, uint8_t *bgr_out,
                             int64_t *first_index_out, int32_t *count_out, int64_t *m_out, void *stream);
int32_t slg_estimate_normals(const double *xyz, int64_t n, double radius, int32_t max_nn,
                             void *ws, int64_t ws_bytes, double *normals_out, double *cov_out,
                             int32_t *m_out, void *stream);
int32_t slg_orient_normals(const double *xyz, double *normals, int64_t n, const double *location,
                           int32_t outward, void *stream);
int32_t slg_cloud_centroid(const double *xyz, int64_t n, void *ws, int64_t ws_bytes,
                           double *centroid_out, void *stream);

/* ---- Point-to-plane ICP and rigid transform on the device cloud (csrc/cloud_icp.hip; DESIGN.md
 * §12): the deterministic part of the loop body of merge_pro_360 (server/processing.py:549-603).
 * Open3D's published rules restated, fp64, no floating-point atomics: the same input gives the
 * same bits.  Asynchronous on `stream`, no host synchronisation: every iteration is enqueued at
 * once, and a `done` word on the device ends the ones that are left.
 *
 *   slg_cloud_transform     <- PointCloud.transform(T)
 * p'[a] = ((T[a][0]*x + T[a][1]*y) + T[a][2]*z) + T[a][3]; normals the same with the 3x3 block and
 * no translation.  T is HOST float64 [16], row-major; its last row must be exactly 0 0 0 1 and
 * every entry finite.  normals / normals_out may be NULL; the outputs may be the inputs.
 *
 *   slg_icp_point_to_plane  <- registration_icp(source, target, max_dist, init,
 *                              TransformationEstimationPointToPlane(),
 *                              ICPConvergenceCriteria(rel_fitness, rel_rmse, max_iteration))
 * Evaluation at a transform T (the accumulated one, applied to the original source each time):
 *   p' = T p as above;  corr[i] = the target point with the smallest (d2, target input index),
 *   d2 = d2(target - p'), among those with d2 < max_dist * max_dist (strict), or -1;
 *   n_corr = their number; err2 = sum of their d2; fitness = n_corr / n_source;
 *   inlier_rmse = sqrt(err2 / n_corr), 0 when n_corr = 0.
 * Step: per correspondence r = ((p' - t) . n_t) summed x, y, z and J = [p' x n_t, n_t]; the 21
 *   upper-triangle entries of sum J J', the 6 of sum J r, n_corr and err2 are fixed trees over the
 *   source input order; JTJ x = -JTr by LDL' without pivoting in a fixed operation order; a pivot
 *   <= 0 or not finite, n_corr = 0 or tgt_normals = NULL make the update the identity; else
 *   R = Rz(x[2]) Ry(x[1]) Rx(x[0]), t = x[3:6], T <- U T.
 * Loop: evaluate at init_T; then up to max_iteration times step and evaluate, stopping after an
 *   evaluation with |fitness - previous| < rel_fitness and |rmse - previous| < rel_rmse.
 *   max_iteration = 0 is evaluate_registration.
 * ws is DEVICE scratch of slg_icp_ws_bytes(n_source, n_target, max_iteration) bytes, 8-byte
 * aligned; the status word at its front as for the filters (a NaN or infinite source or target
 * coordinate sets SLG_FILTER_BAD_NONFINITE; the outputs are then unspecified), and the int32 at
 * byte 8 counts the queries, over all evaluations, that left the grid walk for the whole-target
 * kernel.  init_T is HOST float64 [16] like T above.  result_out is DEVICE float64
 * [SLG_ICP_RESULT_LEN]: T (16), fitness, inlier_rmse, n_corr, iterations (updates made),
 * converged (1 when the stop test ended the loop), 3 unused (written as 0).  corr_out is DEVICE int32 [n_source]
 * or NULL: the last evaluation's correspondences.  log_out is DEVICE float64
 * [max_iteration + 1][SLG_ICP_LOG_STRIDE] or NULL, one record per evaluation (iterations + 1 are
 * written): the T it was made at (16), n_corr, err2, fitness, rmse, the 21 + 6 sums, the x of the
 * step that followed (6, zeros when none), SLG_ICP_LOG_* flags, 2 unused.
 *
 * SLG_ERR_INVALID for n <= 0, max_dist <= 0 or NaN, max_iteration < 0, a negative or NaN
 * criterion, a NULL required pointer, a bad T or a workspace that is too small;
 * SLG_ERR_UNSUPPORTED above 2^30 points or 1000 iterations. */
#define SLG_ICP_RESULT_LEN 24
#define SLG_ICP_LOG_STRIDE 56
#define SLG_ICP_LOG_STOP 1       /* the stop test held at this evaluation */
#define SLG_ICP_LOG_SOLVED 2     /* a step followed: x was applied */
#define SLG_ICP_LOG_SINGULAR 4   /* a step followed with the identity (pivot, n_corr = 0, no normals) */
#define SLG_ICP_LOG_LAST 8       /* max_iteration updates were made */
int64_t slg_icp_ws_bytes(int64_t n_source, int64_t n_target, int32_t max_iteration);
int32_t slg_icp_point_to_plane(const double *src_xyz, int64_t n_source, const double *tgt_xyz,
                               const double *tgt_normals, int64_t n_target, double max_dist,
                               const double *init_T, double rel_fitness, double rel_rmse,
                               int32_t max_iteration, void *ws, int64_t ws_bytes, double *result_out,
                               int32_t *corr_out, double *log_out, void *stream);
int32_t slg_cloud_transform(const double *xyz, const double *normals, int64_t n, const double *T,
                            double *xyz_out, double *normals_out, void *stream);

/* ---- FPFH features, feature matching and seeded RANSAC global registration on the device cloud
 * (csrc/cloud_feature.hip, csrc/cloud_ransac.hip): what merge_pro_360 needs to find
 * a scan's initial pose itself (server/processing.py:451-486).  Open3D's published rules restated
 * (places where the rule is ours are marked so in DESIGN.md), fp64, no floating-point atomics: the
 * same input, and the same seed, give the same bits.  Asynchronous on `stream`; the status word at
 * the front of ws as for the filters.
 *
 *   slg_fpfh                <- compute_fpfh_feature(pcd, KDTreeSearchParamHybrid(radius, max_nn))
 * Neighbours of i: slg_estimate_normals' hybrid search (the first min(max_nn, n) of all points in
 * (d2, input index) order, of those the ones with d2 < radius * radius), m of them, i included.
 * SPFH of i: for every neighbour but i itself (left out by index), Open3D's pair feature of
 * (p_i, n_i), (p_j, n_j) with the roles swapped when |a1| < |a2|; each of the three features adds
 * 100 / (m - 1) to the bin floor(11 * (theta + pi) / (2 pi)), floor(11 * (alpha + 1) * 0.5),
 * floor(11 * (phi + 1) * 0.5) (clamped to 0..10) of its third, in list order.  FPFH of i: over the
 * same list, skipping d2 = 0, spfh[j] / d2 added to the feature and to its third's sum; each third
 * scaled by 100 / sum where the sum is not zero; plus spfh[i].  m <= 1 gives a zero row.
 * fpfh_out float64 [n][SLG_FPFH_DIM]; spfh_out (the same shape) and m_out int32 [n] may be NULL.
 * 2 <= max_nn <= SLG_FPFH_MAX_NN.  ws: slg_fpfh_ws_bytes(n, max_nn) bytes; afterwards the int32 at
 * byte 8 counts the points that left the grid walk for the whole-cloud kernel.
 *
 *   slg_feature_match       <- the correspondence search of registration_ransac_based_on_feature_matching
 * nn_source[i] = the target row with the smallest (d2, target index), d2 = sum over j = 0..32 of
 * (a_j - b_j)^2 left to right, by exact brute force.  With mutual_filter the pair (i, nn_source[i])
 * is kept only when the reverse search from nn_source[i] returns i.  pairs_out int64 [n_source][2]
 * gets the kept pairs in source order, *m_out (DEVICE int64) their number.  nn_source_out int32
 * [n_source] and nn_target_out int32 [n_target] (written with mutual_filter only) may be NULL.
 *
 *   slg_ransac_prepare / slg_ransac_batch
 * prepare builds the target's grid in ws once per registration.  batch runs the trials
 * first_trial .. first_trial + batch - 1 on it: trial t draws three indices into `pairs`
 * (((h >> 32) * n_pairs) >> 32 with h = mix(mix(seed + 0x9E3779B97F4A7C15) + 4 t + k), mix the
 * finaliser of SplitMix64); the draws must be distinct and every pair of the three must satisfy
 * ds2 >= dt2 * e^2 and dt2 >= ds2 * e^2 on the squared edge lengths; T is the rigid least-squares
 * transform of the three pairs (Horn's quaternion, a proper rotation, last row 0 0 0 1); all three
 * must satisfy d2(T s - t) <= max_dist^2.  Every trial that passes is evaluated as
 * slg_icp_point_to_plane evaluates a transform (n_corr, err2, fitness, rmse against the whole
 * target) and gets the number of pairs with d2(T s - t) < max_dist^2, up to max_eval trials per
 * call: a batch in which more pass ends before the first one left out.  records_out float64
 * [batch][SLG_RANSAC_RECORD_STRIDE] holds one record per evaluated trial in ascending trial order;
 * n_eval_out (DEVICE int32 [2]) their number and the number of trials the call dealt with (batch,
 * or fewer: the next call's first_trial is this call's plus that).  A record: trial, the three draws, T (16), n_corr, err2, fitness,
 * rmse, inliers, 7 unused.  trials_out float64 [batch][SLG_RANSAC_TRIAL_STRIDE] or NULL: per trial
 * the draws, SLG_RANSAC_EDGE_OK | SLG_RANSAC_DISTANCE_OK, and T (16; the identity when the edge
 * checker failed).  corr_out int32 [corr_cap][n_source] or NULL: the correspondences (-1: none) of
 * the first corr_cap records.  The choice among the records is sequential in the trial number and
 * is the host's (cloud.py); `confidence` belongs to it and is only validated here.
 *
 * SLG_ERR_INVALID for n <= 0, a radius or distance that is not finite and > 0, max_nn < 2,
 * edge_length or confidence outside [0, 1], a NULL required buffer (slg_fpfh needs normals) or a
 * workspace that is too small; SLG_ERR_UNSUPPORTED above 2^30 points, max_nn > SLG_FPFH_MAX_NN,
 * ransac_n != 3 or batch > SLG_RANSAC_MAX_BATCH. */
#define SLG_FPFH_DIM 33
#define SLG_FPFH_MAX_NN 128
#define SLG_RANSAC_MAX_BATCH 16384
#define SLG_RANSAC_TRIAL_STRIDE 20
#define SLG_RANSAC_RECORD_STRIDE 32
#define SLG_RANSAC_EDGE_OK 1
#define SLG_RANSAC_DISTANCE_OK 2
int64_t slg_fpfh_ws_bytes(int64_t n, int32_t max_nn);
int32_t slg_fpfh(const double *xyz, const double *normals, int64_t n, double radius, int32_t max_nn,
                 void *ws, int64_t ws_bytes, double *fpfh_out, double *spfh_out, int32_t *m_out,
                 void *stream);
int64_t slg_feature_match_ws_bytes(int64_t n_source, int64_t n_target);
int32_t slg_feature_match(const double *source_feature, int64_t n_source, const double *target_feature,
                          int64_t n_target, int32_t mutual_filter, void *ws, int64_t ws_bytes,
                          int32_t *nn_source_out, int32_t *nn_target_out, int64_t *pairs_out,
                          int64_t *m_out, void *stream);
int64_t slg_ransac_ws_bytes(int64_t n_source, int64_t n_target, int32_t batch);
int32_t slg_ransac_prepare(const double *tgt_xyz, int64_t n_target, void *ws, int64_t ws_bytes,
                           void *stream);
int32_t slg_ransac_batch(const double *src_xyz, int64_t n_source, const double *tgt_xyz,
                         int64_t n_target, const int64_t *pairs, int64_t n_pairs, int32_t ransac_n,
                         double edge_length, double max_dist, double confidence, int64_t seed,
                         int64_t first_trial, int32_t batch, void *ws, int64_t ws_bytes, int32_t max_eval,
                         double *records_out, int32_t *n_eval_out, double *trials_out,
                         int32_t *corr_out, int32_t corr_cap, void *stream);

/* ---- Seeded RANSAC plane segmentation on the device cloud (csrc/cloud_plane.hip):
 * PointCloud.segment_plane of ProcessingLogic.remove_background (server/processing.py:337-364).
 * Open3D's published rules restated (places where the rule is ours are marked so in DESIGN.md),
 * fp64, no floating-point atomics: the same cloud and seed give the same bits.  Asynchronous on
 * `stream`; the status word at the front of ws as for the filters (a NaN or infinite coordinate
 * sets SLG_FILTER_BAD_NONFINITE; the outputs are then unspecified).  xyz must be 16-byte aligned.
 *
 *   slg_plane_batch
 * runs the trials first_trial .. first_trial + batch - 1.  Trial t draws ransac_n indices
 * (((h >> 32) * n) >> 32 with h = mix(mix(seed + 0x9E3779B97F4A7C15) + 8 t + k), mix the finaliser
 * of SplitMix64); two equal draws make the trial invalid.  ransac_n = 3: abc = (p1 - p0) x (p2 - p0),
 * norm = sqrt((x^2 + y^2) + z^2), invalid when 0, else abc / norm and d = -((a p0x + b p0y) + c p0z).
 * ransac_n > 3: the centroid (sum in draw order / ransac_n), the six centred sums xx xy xz yy yz zz
 * in draw order, det_x = yy zz - yz yz, det_y = xx zz - xz xz, det_z = xx yy - xy xy; abc =
 * (det_x, xz yz - xy zz, xy yz - xz yy) when det_x is strictly the largest, else
 * (xz yz - xy zz, det_y, xy xz - yz xx) when det_y > det_z, else (xy yz - xz yy, xy xz - yz xx,
 * det_z); normalised as above with d from the centroid.  Every trial is evaluated over the whole
 * cloud: dist = |((a x + b y) + c z) + d|, an inlier when dist < distance_threshold (strict),
 * count their number, err the sum of their dist: left to right within each chunk of 2048
 * consecutive points (a point that is no inlier adds +0.0), then the chunks left to right.
 * records_out float64 [batch][SLG_PLANE_RECORD_STRIDE], one record per trial in trial order:
 * trial, valid, a, b, c, d, count, err, fitness = count / n, rmse = err / sqrt(count) (0 without
 * inliers), 6 unused; an invalid trial has the zero plane and zeros.  The choice among the records
 * is sequential in the trial number and is the host's (cloud.py).
 *
 *   slg_plane_finish
 * takes a plane (HOST float64 [4]): index_out int64 [n] gets the indices with dist <
 * distance_threshold in ascending order, *count_out (DEVICE int64) their number m; sums_out
 * (DEVICE float64 [SLG_PLANE_SUMS_LEN]): the sums of x, y, z over those points, the six centred
 * sums xx xy xz yy yz zz about centroid = sums / m, the centroid (3), m, 3 unused, each sum the
 * fixed tree of slg_cloud_centroid over the input order in which other points add nothing;
 * plane_out (DEVICE float64 [4]): the ransac_n > 3 rule applied to that centroid and those sums.
 *
 * ws: slg_plane_ws_bytes(n, batch) bytes (slg_plane_finish needs batch = 1).  SLG_ERR_INVALID for
 * n <= 0, n < ransac_n, ransac_n < 3, batch <= 0, first_trial < 0, a threshold or plane that is not
 * finite (and > 0), a NULL or misaligned buffer or a workspace that is too small;
 * SLG_ERR_UNSUPPORTED above 2^30 points, ransac_n > SLG_PLANE_MAX_RANSAC_N or batch >
 * SLG_PLANE_MAX_BATCH. */
#define SLG_PLANE_MAX_BATCH 4096
#define SLG_PLANE_RECORD_STRIDE 16
#define SLG_PLANE_SUMS_LEN 16
#define SLG_PLANE_MAX_RANSAC_N 8
int64_t slg_plane_ws_bytes(int64_t n, int32_t batch);
int32_t slg_plane_batch(const double *xyz, int64_t n, double distance_threshold, int32_t ransac_n,
                        int64_t seed, int64_t first_trial, int32_t batch, void *ws, int64_t ws_bytes,
                        double *records_out, void *stream);
int32_t slg_plane_finish(const double *xyz, int64_t n, const double *plane, double distance_threshold,
                         void *ws, int64_t ws_bytes, int64_t *index_out, int64_t *count_out,
                         double *sums_out, double *plane_out, void *stream);

/* ---- Tangent-plane normal orientation on the device cloud (csrc/cloud_orient.hip):
 * PointCloud.orient_normals_consistent_tangent_plane(k) of mesh_360 and reconstruct_stl
 * (server/processing.py:675, :685, :823), with the neighbour lists and the Euclidean minimum
 * spanning tree it is built from as calls of their own.  Open3D's procedure in closed form (its
 * sort leaves ties open; the total orders below are ours), fp64, integer atomics only: the same
 * input gives the same bits.  Asynchronous on `stream`; the status word at the front of ws as for
 * the filters (a NaN or infinite coordinate or normal sets SLG_FILTER_BAD_NONFINITE; the outputs
 * are then unspecified).
 *
 *   slg_knn_lists
 * kk = min(k, n) entries per point: all points in ascending (d2, input index) order, d2 =
 * (dx^2 + dy^2) + dz^2, the point itself included (it is first unless a duplicate with a lower
 * index precedes it).  idx_out uint32 [n][kk], d2_out float64 [n][kk], rows by input index.
 *
 *   slg_emst
 * the minimum spanning tree of the complete graph under the total order (d2, a, b) on the
 * undirected edges (a, b), a < b: unique, duplicates are ordinary edges with d2 = 0.  edges_out
 * int64 [n - 1][2] gets its edges (a, b) in no particular order.  k is the length of the lists
 * the Boruvka rounds start from (any k >= 1 gives the same tree).
 *
 *   slg_orient_tangent
 * the Riemannian graph is the EMST's edges and, for every point, the edges to its list entries
 * other than itself; its minimum spanning tree under (w, a, b), w = 1 - |(na.x nb.x + na.y nb.y)
 * + na.z nb.z|, is unique.  The root is the lowest index among the points of largest z; its normal
 * is negated iff its z component is negative.  Every other point's sign is the root's times the
 * product over its tree path of sgn(na . nb) on the input normals, sgn(0) = +1.  normals_out
 * float64 [n][3] (not the input buffer) gets the normals, negated as a whole or left alone;
 * optional: emst_out and tree_out int64 [n - 1][2] as above, root_out int64 [1].
 *
 * stats_out (optional, DEVICE int32 [SLG_ORIENT_STATS_LEN]): SLG_ORIENT_STAT_*: the rounds of the
 * two Boruvkas, the points the lists sent to the whole-cloud kernel, the points that walked the
 * grid for a foreign neighbour and the far-list entries (totals, then per EMST round from
 * SLG_ORIENT_STAT_ROUND_*), and the rounds the largest component sat out.  These depend on the
 * schedule, the results do not.
 *
 * ws: slg_orient_ws_bytes(n, k) bytes.  SLG_ERR_INVALID for n <= 0, k <= 0, a NULL or misaligned
 * (8 bytes) buffer, normals_out == normals or a workspace that is too small; SLG_ERR_UNSUPPORTED
 * above 2^30 points or k > SLG_ORIENT_MAX_K. */
#define SLG_ORIENT_MAX_K 128
#define SLG_ORIENT_STATS_LEN 128
#define SLG_ORIENT_STAT_EMST_ROUNDS 0
#define SLG_ORIENT_STAT_TREE_ROUNDS 1
#define SLG_ORIENT_STAT_LIST_FAR 2
#define SLG_ORIENT_STAT_WALKED 3
#define SLG_ORIENT_STAT_FAR 4
#define SLG_ORIENT_STAT_SAT_OUT 5
#define SLG_ORIENT_STAT_ROUND_WALKED 16
#define SLG_ORIENT_STAT_ROUND_FAR 48
#define SLG_ORIENT_STAT_ROUND_SAT_OUT 80
int64_t slg_orient_ws_bytes(int64_t n, int32_t k);
int32_t slg_knn_lists(const double *xyz, int64_t n, int32_t k, void *ws, int64_t ws_bytes,
                      uint32_t *idx_out, double *d2_out, void *stream);
int32_t slg_emst(const double *xyz, int64_t n, int32_t k, void *ws, int64_t ws_bytes,
                 int64_t *edges_out, int32_t *stats_out, void *stream);
int32_t slg_orient_tangent(const double *xyz, const double *normals, int64_t n, int32_t k, void *ws,
                           int64_t ws_bytes, double *normals_out, int64_t *emst_out, int64_t *tree_out,
                           int64_t *root_out, int32_t *stats_out, void *stream);

/* ---- Watertight meshing of an oriented device cloud on a dense uniform grid (csrc/cloud_mesh.hip;
 * DESIGN.md §16): the last call of mesh_360 and reconstruct_stl(mode="watertight")
 * (server/processing.py:703, :842).  Our rule, Open3D parity unpinned: the idea of Poisson surface
 * reconstruction on a uniform grid of R = 2^depth cells per axis instead of Kazhdan's adaptive
 * octree.  fp64, integer atomics only (the status word): the same input gives the same bits.
 * Asynchronous on `stream`.  Node arrays are float64 [R+1]^3, x fastest.
 *
 * Every call takes a workspace, 256-byte aligned, whose first SLG_MESH_HDR_BYTES bytes are the
 * header: int32 status (SLG_FILTER_BAD_* as for the filters) at byte 0, int32 R at 4, int64 nV at 8,
 * int64 nT at 16, float64 origin[3] at 24, h at 48, iso at 56, thr at 64.  The rest is the stage's
 * scratch, slg_mesh_ws_bytes(stage, R, n, m) bytes in all (n points or values, m triangles);
 * SLG_MESH_WS_ALL: the largest of the stages GRID..EXTRACT plus the six node arrays W, V, f, chi
 * (48 (R+1)^3 bytes), what a whole reconstruction holds.  Once the status word is set, later
 * kernels return at once.
 *
 *   slg_mesh_grid        side = scale * largest extent of the box, origin = (min + max) / 2 -
 *                        side / 2, h = side / R into the header; a non-finite coordinate or a zero
 *                        extent sets the status word.
 *   slg_mesh_set_header  the header from host values instead (the stages as calls of their own).
 *   slg_mesh_splat       u = (p - origin) / h, i = floor(u) clamped to 0..R-1, t = u - i; per node
 *                        its 8 incident cells in ascending cell id, each cell's points in
 *                        ascending input index: W += w, V += w * normal, w the trilinear weight.
 *                        V_out float64 [R+1]^3 x 3.  A non-finite normal sets the status word.
 *   slg_mesh_divergence  f = (dVx / 2h + dVy / 2h) + dVz / 2h by central differences, 0 on the boundary.
 *   slg_mesh_solve       the 7-point Laplacian of chi = f, chi = 0 on the boundary: `cycles` V(2,2)
 *                        cycles from 0 of a vertex-centred multigrid R, R/2, .., 2; damped Jacobi
 *                        (6/7), full weighting, trilinear prolongation, the R = 2 level directly.
 *   slg_mesh_sample      out[j] = trilinear field at xyz[j].
 *   slg_mesh_iso         header iso = mean of trilinear chi at the points (slg_cloud_centroid's tree).
 *   slg_mesh_count       marching tetrahedra over Kuhn's six tetrahedra per cell, inside = chi < iso:
 *                        crossing masks, triangle counts and their scans into the scratch; header
 *                        nV, nT.  slg_mesh_emit (same workspace, untouched in between) then writes
 *                        vertices float64 [nV][3] in ascending (owner node, edge type), densities
 *                        (trilinear W at the vertex; W may be NULL) and triangles int32 [nT][3] in
 *                        ascending (cell, tetrahedron, triangle), wound so that (b - a) x (c - a)
 *                        points from inside to outside.
 *   slg_mesh_quantile    header thr = numpy's linear quantile(values, q).
 *   slg_mesh_remove      drops the vertices with mask != 0 and every triangle with such a corner,
 *                        renumbers, keeps the order; header nV, nT are the new counts.
 *   slg_mesh_triangle_normals  unit (b - a) x (c - a), (0, 0, 0) for a zero-area triangle.
 *   slg_mesh_stl_pack    50 bytes per triangle: float32 normal, three float32 vertices, uint16 0.
 *
 * SLG_ERR_INVALID for a NULL or misaligned buffer, a count <= 0, depth outside 2..10, R no power
 * of two in range, scale < 1, q outside [0, 1] or a workspace that is too small;
 * SLG_ERR_UNSUPPORTED above 2^30 points or from 2^31 vertices. */
#define SLG_MESH_HDR_BYTES 256
#define SLG_MESH_WS_GRID 0
#define SLG_MESH_WS_SPLAT 1
#define SLG_MESH_WS_SOLVE 2
#define SLG_MESH_WS_ISO 3
#define SLG_MESH_WS_EXTRACT 4
#define SLG_MESH_WS_QUANTILE 5
#define SLG_MESH_WS_REMOVE 6
#define SLG_MESH_WS_ALL 7
int64_t slg_mesh_ws_bytes(int32_t stage, int32_t R, int64_t n, int64_t m);
int32_t slg_mesh_set_header(void *ws, int32_t R, const double *origin, double h, double iso, void *stream);
int32_t slg_mesh_grid(const double *xyz, int64_t n, int32_t depth, double scale, void *ws, int64_t ws_bytes,
                      void *stream);
int32_t slg_mesh_splat(const double *xyz, const double *normals, int64_t n, int32_t R, void *ws,
                       int64_t ws_bytes, double *W_out, double *V_out, void *stream);
int32_t slg_mesh_divergence(const double *V, int32_t R, void *ws, double *f_out, void *stream);
int32_t slg_mesh_solve(const double *f, int32_t R, int32_t cycles, void *ws, int64_t ws_bytes,
                       double *chi_out, void *stream);
int32_t slg_mesh_sample(const double *field, const double *xyz, int64_t n, void *ws, double *out, void *stream);
int32_t slg_mesh_iso(const double *chi, const double *xyz, int64_t n, void *ws, int64_t ws_bytes, void *stream);
int32_t slg_mesh_count(const double *chi, int32_t R, void *ws, int64_t ws_bytes, void *stream);
int32_t slg_mesh_emit(const double *chi, const double *W, int32_t R, void *ws, int64_t ws_bytes,
                      double *vertices_out, int64_t n_vertices, double *densities_out, int32_t *triangles_out,
                      int64_t n_triangles, void *stream);
int32_t slg_mesh_quantile(const double *values, int64_t n, double q, void *ws, int64_t ws_bytes, void *stream);
int32_t slg_mesh_remove(const double *vertices, const double *densities, int64_t n_vertices,
                        const int32_t *triangles, int64_t n_triangles, const uint8_t *mask, void *ws,
                        int64_t ws_bytes, double *vertices_out, double *densities_out, int32_t *triangles_out,
                        void *stream);
int32_t slg_mesh_triangle_normals(const double *vertices, const int32_t *triangles, int64_t n_triangles,
                                  double *normals_out, void *stream);
int32_t slg_mesh_stl_pack(const double *vertices, const int32_t *triangles, const double *normals,
                          int64_t n_triangles, uint8_t *records_out, void *stream);

/* ---- Mesh post-processing (csrc/cloud_meshpost.hip): what the device takes of the
 * reference's MeshLab step (server/processing.py:742-787): vertex adjacency, Laplacian and Taubin
 * smoothing, the closing of small holes.  Our rules, MeshLab / VCGlib parity unpinned; the same
 * input gives the same bits.  Asynchronous on `stream`.  triangles int32 [T][3] with indices in
 * 0..V-1 (any other sets SLG_FILTER_BAD_INDEX in the status word; later kernels then return).
 *
 * The workspaces, slg_mesh_post_ws_bytes(stage, V, T) bytes and 256-byte aligned, begin with the
 * mesh header: int32 status at byte 0, int64 nV at 8, int64 nT at 16, and int64 stats[8] at 128.
 * The stage numbers continue those of slg_mesh_ws_bytes.  A directed pair is the key src << 32 | dst.
 *
 *   slg_mesh_adjacency_count  the six directed pairs of every triangle, sorted, unique, no
 *                        self-pair: header nV = entries of the adjacency CSR.  The winding pairs
 *                        a->b, b->c, c->a alone: (a, b) is a boundary edge iff (b, a) is not
 *                        among them; header nT = entries of the boundary CSR (both directions of
 *                        every boundary edge, unique).
 *   slg_mesh_adjacency_emit   (same workspace, untouched in between) offsets int64 [V+1] and
 *                        neighbours int32 ascending per row; boundary uint8 [V] (1: an endpoint
 *                        of a boundary edge) and the boundary CSR likewise.
 *   slg_mesh_smooth_pass one Jacobi pass out = f(in), out != in.  N(v) is the boundary row of a
 *                        boundary vertex, the adjacency row otherwise; s = ((q0 + q1) + q2) + ..
 *                        per component in row order, c = |N(v)|; c == 0 copies p.
 *                        SLG_MESH_SMOOTH_LAPLACIAN: p' = (p + s) / (c + 1).  SLG_MESH_SMOOTH_STEP:
 *                        m = s / c, p' = p + (m - p) * factor (Taubin: factor lam, then mu).
 *   slg_mesh_holes_count B = the boundary edges in ascending key order; next(a, b) = the first
 *                        edge of B with source b.  A vertex is blocked when its in or out degree
 *                        along B is not 1 while it has any, or when a winding pair through it
 *                        occurs twice.  Every edge walks next for at most max_size (3..64) steps:
 *                        closable when back at itself after 3 <= L <= max_size steps without
 *                        touching a blocked vertex; the loop's leader is its smallest index in B.
 *                        Header nT = new triangles (L - 2 per loop), stats[SLG_MESH_HOLES_STAT_*].
 *   slg_mesh_holes_emit  (same workspace) the new triangles in ascending (leader, clip step) into
 *                        triangles_out [nT][3]: ring r[0..m-1] from the leader's source in walk
 *                        order; while m > 3 the i with the smallest squared diagonal
 *                        (dx dx + dy dy) + dz dz between r[i-1] and r[i+1] (ties: lowest i) gives
 *                        (r[i+1], r[i], r[i-1]) and leaves; last (r[2], r[1], r[0]).  No
 *                        self-intersection or existing-edge check.
 *
 * SLG_ERR_INVALID for a NULL or misaligned buffer, V or T <= 0, V >= 2^31, 3 T > 2^30, max_size
 * outside 3..64, an unknown stage or mode, or a workspace that is too small. */
#define SLG_MESH_WS_ADJACENCY 8
#define SLG_MESH_WS_HOLES 9
#define SLG_MESH_SMOOTH_LAPLACIAN 0
#define SLG_MESH_SMOOTH_STEP 1
#define SLG_MESH_HOLES_MAX_SIZE 64
#define SLG_MESH_HOLES_STAT_EDGES 0          /* boundary edges */
#define SLG_MESH_HOLES_STAT_LOOPS 1          /* closable loops */
#define SLG_MESH_HOLES_STAT_CLOSABLE_EDGES 2 /* edges on closable loops */
#define SLG_MESH_HOLES_STAT_LONG_EDGES 3     /* edges whose walk ran max_size steps: loops left open by size */
#define SLG_MESH_HOLES_STAT_BLOCKED_EDGES 4  /* edges whose walk touched a blocked vertex */
int64_t slg_mesh_post_ws_bytes(int32_t stage, int64_t n_vertices, int64_t n_triangles);
int32_t slg_mesh_adjacency_count(const int32_t *triangles, int64_t n_triangles, int64_t n_vertices, void *ws,
                                 int64_t ws_bytes, void *stream);
int32_t slg_mesh_adjacency_emit(int64_t n_triangles, int64_t n_vertices, void *ws, int64_t ws_bytes,
                                int64_t *offsets_out, int32_t *neighbours_out, int64_t n_neighbours,
                                uint8_t *boundary_out, int64_t *boundary_offsets_out,
                                int32_t *boundary_neighbours_out, int64_t n_boundary_neighbours, void *stream);
int32_t slg_mesh_smooth_pass(const double *vertices, double *vertices_out, int64_t n_vertices,
                             const int64_t *offsets, const int32_t *neighbours, const uint8_t *boundary,
                             const int64_t *boundary_offsets, const int32_t *boundary_neighbours, int32_t mode,
                             double factor, void *stream);
int32_t slg_mesh_holes_count(const int32_t *triangles, int64_t n_triangles, int64_t n_vertices, int32_t max_size,
                             void *ws, int64_t ws_bytes, void *stream);
int32_t slg_mesh_holes_emit(const double *vertices, int64_t n_vertices, int64_t n_triangles, void *ws,
                            int64_t ws_bytes, int32_t *triangles_out, int64_t n_new_triangles, void *stream);

/* ---- Mesh decimation (csrc/cloud_decimate.hip): quadric edge collapse in rounds of
 * independent collapses, what the device takes of meshlab_params["simplify"]
 * (server/processing.py:778-781).  Our rule, MeshLab / VCGlib parity unpinned; a pure function of
 * the mesh and the target, restated in tests/decimate_ref.py.  Asynchronous on `stream`.
 *
 * One workspace of slg_mesh_decimate_ws_bytes(V, T) bytes, 256-byte aligned, carries the state
 * from init through the rounds to emit.  It begins with the mesh header: int32 status at byte 0
 * (SLG_FILTER_BAD_INDEX: a triangle index outside 0..V-1; every later kernel then returns), int64
 * alive vertices at 8, alive triangles at 16, the last round's candidate edges at 24 and applied
 * collapses at 32, all collapses since init at 40, and int64 stats[8] at 128
 * (SLG_MESH_DECIMATE_STAT_* of the last round).
 *
 *   slg_mesh_decimate_init   copies positions and triangles into the workspace, builds the
 *                        incidence CSR and sums every vertex's quadric over its triangles in
 *                        ascending index: K = (a2, ab, ac, ad, b2, bc, bd, c2, cd, d2) of
 *                        n = (B - A) x (C - A), not normalised, d = -((nx Ax + ny Ay) + nz Az).
 *   slg_mesh_decimate_round  one round on the n_alive triangles the header reports (the caller
 *                        reads it after every round): adjacency, the candidate edges u < v in
 *                        ascending key, their refusals (boundary, nonmanifold, link, valence, nan,
 *                        flip), placement and cost, the rank by (cost bits, key),
 *                        SLG_MESH_DECIMATE_SWEEPS selection sweeps by integer atomicMin over the
 *                        closed neighbourhoods, and the first ceil((n_alive - target) / 2) selected
 *                        in rank order applied: P[u] = p, Q[u] += Q[v], v -> u, triangles with two
 *                        equal corners dropped, the rest compacted in order.
 *   slg_mesh_decimate_emit   the surviving vertices (and densities, when given) in their order
 *                        and the alive triangles renumbered: n_vertices_out = header's alive
 *                        vertices, n_triangles_out = alive triangles.
 *
 * SLG_ERR_INVALID for a NULL or misaligned buffer, V or T <= 0, V >= 2^31, 3 T > 2^30, n_alive
 * outside 1..T, a target below 0 or not below n_alive, or a workspace that is too small. */
#define SLG_MESH_DECIMATE_SWEEPS 4
#define SLG_MESH_DECIMATE_STAT_BOUNDARY 0    /* both endpoints on the boundary */
#define SLG_MESH_DECIMATE_STAT_NONMANIFOLD 1 /* (u, v) or (v, u) not exactly once among the winding pairs */
#define SLG_MESH_DECIMATE_STAT_LINK 2        /* the endpoints share other than two neighbours */
#define SLG_MESH_DECIMATE_STAT_VALENCE 3     /* a shared neighbour of valence below 4 */
#define SLG_MESH_DECIMATE_STAT_FLIP 4        /* a triangle around the edge would turn over */
#define SLG_MESH_DECIMATE_STAT_NAN 5         /* the placement's cost is not finite */
#define SLG_MESH_DECIMATE_STAT_VALID 6       /* candidates that passed every test */
#define SLG_MESH_DECIMATE_STAT_SELECTED 7    /* selected by the sweeps (the budget may apply fewer) */
int64_t slg_mesh_decimate_ws_bytes(int64_t n_vertices, int64_t n_triangles);
int32_t slg_mesh_decimate_init(const double *vertices, int64_t n_vertices, const int32_t *triangles,
                               int64_t n_triangles, void *ws, int64_t ws_bytes, void *stream);
int32_t slg_mesh_decimate_round(void *ws, int64_t ws_bytes, int64_t n_vertices, int64_t n_triangles,
                                int64_t n_alive, int64_t target, void *stream);
int32_t slg_mesh_decimate_emit(void *ws, int64_t ws_bytes, int64_t n_vertices, int64_t n_triangles,
                               const double *densities, double *vertices_out, double *densities_out,
                               int64_t n_vertices_out, int32_t *triangles_out, int64_t n_triangles_out,
                               void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SLGPU_H */
