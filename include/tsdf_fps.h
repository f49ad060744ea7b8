/*
 * tsdf_fps.h — C ABI of libtsdf_fps.so: farthest-point sampled clouds, the input of a point network (HandPointNet,
 * Point-to-Point Regression PointNet and their family): a fixed number M of points of a frame's cloud, each the point
 * farthest from all chosen before it.
 *
 * One more library next to libtsdf_hip.so (include/tsdf.h, v7, frozen), the eleven of csrc/Makefile's EXTS line,
 * libtsdf_heatmap.so, libtsdf_heatloss.so and libtsdf_occupancy.so (all v1, frozen): its own translation unit
 * (csrc/tsdf_fps.hip), its own binary and its own version number.  It shares the status codes of tsdf.h and nothing
 * else; the camera's five constants come by value.  Conventions:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - a call is asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronises;
 *   - it allocates nothing, uses no global atomics and no device-side state, never prints, has no CPU fallback and may
 *     be captured into a hipGraph (a captured launch is self-contained; with d_work the workspace belongs to the launch
 *     until it has run);
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.  Arguments are checked first, then the device
 *     (TSDF_ERR_NO_DEVICE unless the current device is a gfx950), then the kernel is launched.
 */
#ifndef TSDF_FPS_H_
#define TSDF_FPS_H_

#include <stdint.h>

#include "tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_FPS_VERSION 1

/* a batch position with more candidates than the call can hold; next to enum tsdf_frame_status's 0, 1, 2 */
#define TSDF_FPS_FRAME_OVER_CAPACITY 3

#define TSDF_FPS_MAX_POINTS 65536   /* M is in 1..TSDF_FPS_MAX_POINTS */

/* the element type of tsdf_fps_points_hip's d_points */
#define TSDF_FPS_F32 0
#define TSDF_FPS_F64 1

/* 1 */
int tsdf_fps_version(void);

/*
 * THE RULE, the same for both entries.  Per batch position a loader (below) gives `count` CANDIDATES in RANK order, each
 * three float32 coordinates, all finite.  All arithmetic is float32, every operation rounded on its own, no fma.
 *     sample 0 is the candidate of lowest rank
 *     every candidate i keeps a running dist_i, initially +inf
 *     after sample j-1 = s is chosen:   dx = p_i.x - s.x,  dy = p_i.y - s.y,  dz = p_i.z - s.z
 *                                       dist_i = min(dist_i, (dx*dx + dy*dy) + dz*dz)
 *     sample j is the candidate of greatest dist, ties to the LOWEST rank
 * dist is never a NaN: a difference of two finite numbers is finite or an infinity, never a NaN; its square is in
 * [+0, +inf]; a sum of two numbers of [+0, +inf] is in [+0, +inf] (no inf - inf arises); and the minimum of two such
 * numbers is one of them.  So dist is in [+0, +inf], its bit pattern orders as an unsigned integer, and "greatest" is
 * well defined.  (A sample's own dist is +0: dx = dy = dz = +0.)
 * Nothing special happens when the candidates run out: once the greatest dist is 0 every dist is +0, the tie goes to the
 * lowest rank, which is sample 0, and choosing it changes nothing.  So for count < M, or a cloud of few distinct points,
 * the trailing rows equal row 0 (with radius2 +0).
 * CONSEQUENCE: sample j depends on samples 0..j-1 alone, so the first k rows of an M-point result are the k-point
 * result: the 1024 / 512 / 128 hierarchy of a point network costs one call.
 *
 * OUTPUTS per batch position, every byte written by the launch:
 *   d_out_points   float32[n][M][3]  the very float32 points the selection measured
 *   d_out_pixel    int32[n][M]       the rank of each sample (crop index or row): gather anything else with it
 *   d_out_radius2  float32[n][M] or NULL: row 0 is +inf, row j the dist at which sample j was chosen — the squared
 *                  covering radius of samples 0..j-1, non-increasing in j
 *   d_out_count    int32[n]          the number of candidates
 *   d_out_status   int32[n]          per-position status, which never fails the call:
 *       TSDF_FRAME_BAD_HEADER (2)         see the loaders
 *       TSDF_FRAME_DEGENERATE (1)         count == 0
 *       TSDF_FPS_FRAME_OVER_CAPACITY (3)  count exceeds what the call can hold (below); count is still the true count
 *       all three give zero points, pixel = -1 and radius2 = +0 in every row.  Otherwise TSDF_FRAME_OK (0).
 *
 * CAPACITY AND FORMS.  The result never depends on the form.
 *   resident   one workgroup per position holds the candidates' coordinates in LDS and, with their running dist, in
 *              registers: up to *resident_cap candidates (tsdf_fps_plan), nothing in memory.
 *   streaming  the same rule with the state in the caller's workspace d_work, float32[n][capacity][4] (x, y, z, dist),
 *              16-byte aligned: up to `capacity` candidates per position.  Used for a position above the resident cap,
 *              and, with form_hint 1, for every position (so that small frames can test it).  Written for correctness;
 *              each iteration goes through the cache hierarchy and it is several times slower per candidate.
 *   A position holds iff  count <= resident_cap (form_hint 0)  or  d_work and count <= capacity.
 *   form_hint  0 the library's choice, 1 streaming wherever a workspace allows.
 */

/*
 * The plan, host code only: *resident_cap candidates fit the resident form, the workspace of the streaming form is
 * *work_bytes = 16 * capacity bytes per batch position, and a workgroup uses *lds_bytes of LDS.
 * TSDF_ERR_INVALID_ARG for M outside 1..65536, capacity outside 0..2^31-1, a form_hint that is not 0 or 1 or a NULL
 * result pointer.
 */
int tsdf_fps_plan(int M, int64_t capacity, int form_hint, int *resident_cap, int64_t *work_bytes, int *lds_bytes);

/*
 * Candidates FROM A PACKED CROP.
 *   d_depth, depth_len, d_offsets, d_headers, n_src, d_index, n, focal .. trunc_voxels, d_xforms
 *              exactly as for tsdf_occupancy_hip (include/tsdf_occupancy.h): source tables indexed by source frame,
 *              batch position i takes g = d_index ? d_index[i] : i, a g outside [0, n_src) or a header that fails the
 *              voxelizer's rule gives TSDF_FRAME_BAD_HEADER and nothing of the frame is read; the camera by value;
 *              d_xforms float64[n][24] or NULL, one map per BATCH POSITION, forward rows only.  A crop of 2^31 pixels
 *              or more is a bad header here: its ranks would not fit int32.
 *   M          samples per position, 1..65536
 *   capacity, d_work   the streaming form's workspace (above); d_work NULL means capacity must be 0
 * Per pixel of column x and row y of the image with depth d (float32), in float64, one rounding per operation, no fma:
 *     a candidate iff |d| >= invalid_eps                               a NaN is not
 *     q = (double)d / F
 *     p = ( q * (x - cx),  -(q * (y - cy)),  -(double)d )
 *     o = p                                                            without a map
 *     o_i = (A_i0 * p_x + A_i1 * p_y) + (A_i2 * p_z + b_i)             with one, in this grouping.  Under identity rows
 *                                                                      o == p, hence the same samples; a zero loses
 *                                                                      its sign (p_y = -0 on the row of cy gives +0)
 *     the candidate's point is ( (float)o_x, (float)o_y, (float)o_z ): ONE rounding to float32
 *     a candidate whose three float32 coordinates are not all finite is dropped
 *     rank = the pixel's index in the crop, row-major in the bbox: (y - top) * (right - left) + (x - left)
 *
 * TSDF_ERR_INVALID_ARG, checked in this order before the device is looked at: n < 0; M outside 1..65536; a form_hint
 * that is not 0 or 1; capacity outside 0..2^31-1; (n == 0 returns TSDF_OK here;) a NULL d_depth, d_offsets, d_headers,
 * d_out_points, d_out_pixel, d_out_count or d_out_status; depth_len < 0; n_src < 1; d_index == NULL with n_src != n;
 * d_work NULL with capacity != 0 or d_work given with capacity == 0; a d_xforms that is not 8-byte aligned or a d_work
 * that is not 16-byte aligned; a focal, invalid_eps or trunc_voxels that is not > 0; a batch whose n workgroups do not
 * fit one launch (2^32 work-items or more).
 */
int tsdf_fps_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                 int64_t n_src, const int64_t *d_index, int n, int M, double focal, double cx, double cy,
                 float invalid_eps, float trunc_voxels, int64_t capacity, int form_hint, void *hip_stream,
                 const double *d_xforms, float *d_work, float *d_out_points, int32_t *d_out_pixel, float *d_out_radius2,
                 int32_t *d_out_count, int32_t *d_out_status);

/*
 * Candidates FROM A CLOUD: point_clouds' output, or a network's own set-abstraction level.
 *   d_points   float32[n][P][3] (dtype TSDF_FPS_F32) or float64[n][P][3] (TSDF_FPS_F64), aligned to its element
 *   P          rows per position, 1..2^31-1
 * A float64 coordinate is rounded once to float32.  A row is a candidate iff its three float32 coordinates are finite;
 * rank = row number.  There is no header: TSDF_FRAME_BAD_HEADER does not occur.
 *
 * TSDF_ERR_INVALID_ARG, in this order: n < 0; M outside 1..65536; a form_hint that is not 0 or 1; capacity outside
 * 0..2^31-1; a dtype that is not TSDF_FPS_F32 or TSDF_FPS_F64; P outside 1..2^31-1; (n == 0 returns TSDF_OK here;) a
 * NULL d_points, d_out_points, d_out_pixel, d_out_count or d_out_status; d_work NULL with capacity != 0 or d_work given
 * with capacity == 0; a d_points off its element's alignment or a d_work that is not 16-byte aligned; too many
 * workgroups for one launch.
 */
int tsdf_fps_points_hip(const void *d_points, int dtype, int n, int64_t P, int M, int64_t capacity, int form_hint,
                        void *hip_stream, float *d_work, float *d_out_points, int32_t *d_out_pixel,
                        float *d_out_radius2, int32_t *d_out_count, int32_t *d_out_status);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_FPS_H_ */
