/*
 * tsdf_locate.h — C ABI of libtsdf_locate.so: the hand located in raw depth frames on the GPU — the nearest object's
 * centre of mass, a fixed cube cut around it, and the crops packed as the depth / offsets / headers triple every
 * voxelizer here reads.
 *
 * One more extension library next to libtsdf_hip.so (include/tsdf.h, v7, frozen) and libtsdf_augment.so,
 * libtsdf_augstep.so, libtsdf_auggrid.so, libtsdf_depth16.so, libtsdf_obb.so, libtsdf_lowp.so, libtsdf_maplowp.so,
 * libtsdf_mapstep.so (all v1, frozen): its own translation unit (csrc/tsdf_locate.hip), its own binary and its own
 * version number.  It shares the status codes of tsdf.h and nothing else.  Conventions:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - the calls are asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronise;
 *   - they allocate nothing, use no atomics and no device-side state, never print, have no CPU fallback, are
 *     deterministic (two calls give identical bits; a frame gives the same bits alone and at any position of any batch)
 *     and may be captured into a hipGraph (the captured launches are self-contained);
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.  Arguments are checked first, then the device
 *     (TSDF_ERR_NO_DEVICE unless the current device is a gfx950), then the kernels are launched.
 *
 * What it is for: every entry of the other headers starts from a hand that somebody has already cut out of the image
 * (MSRA ships that box in each file).  NYU, ICVL, BigHand and a live sensor ship whole frames.  This library is the
 * step every hand-pose code base has in front of its network — centre of mass of the nearest object, a cube of
 * 250-300 mm around it — with the frames read on the GPU as the sensor wrote them.
 */
#ifndef TSDF_LOCATE_H_
#define TSDF_LOCATE_H_

#include <stdint.h>

#include "tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_LOCATE_VERSION 1

/* enum of `frame_type` */
#define TSDF_LOCATE_F32 0 /* float32 millimetres */
#define TSDF_LOCATE_U16 1 /* uint16 u with a shift k in 0..7: the depth is u * 2^-k, the encoding of tsdf_depth16.h */

/* 1 */
int tsdf_locate_version(void);

/*
 * The capacity rule.  *per_frame = min(W, s) * min(H, s) with s = floor(cube * focal / near) + 2 (float64, cube and
 * near widened from float32 first): no located crop is larger, because the cube's depth is a mean of depths >= near,
 * so a side is at most floor(cube * focal / near) + 2 pixels, and step 5 below holds a side to min(W, s) (or min(H, s))
 * outright.  A d_out_depth of n * *per_frame floats can therefore never overflow.  Host code, no device.
 *
 * TSDF_ERR_INVALID_ARG: per_frame == NULL, H <= 0, W <= 0, or cube, near or focal not > 0 (a NaN is not).
 */
int tsdf_locate_capacity(int H, int W, float cube, float near_mm, double focal, int64_t *per_frame);

/*
 * Locate the hand in n frames and pack the crops.
 *
 *   d_frames    [n_src][H][W], contiguous, aligned to its element: float32 mm (TSDF_LOCATE_F32) or uint16
 *               (TSDF_LOCATE_U16, depth = float32(u) * 2^-shift, exact)
 *   shift       0..7 with TSDF_LOCATE_U16, otherwise unused
 *   n_src, H, W the source frames and their size
 *   d_index     int64[n] or NULL.  With NULL, n_src must equal n.  Batch position i reads source frame
 *               g = d_index ? d_index[i] : i; a g outside [0, n_src) gives that position status 2
 *   n           batch positions; 0 is a no-op (TSDF_OK) whatever else is passed
 *   near_mm, far_mm   float32, 0 < near <= far: the depth range in which the hand is looked for
 *   cube        float32 > 0: the edge of the crop cube, mm
 *   seed_band   float32 >= 0, mm
 *   refine      0..8
 *   R           the grid resolution (a multiple of 4 in 4..128); it enters d_out_grid alone but is checked always
 *   focal, cx, cy, invalid_eps, trunc_voxels
 *               the camera constants BY VALUE, the five fields of the camera struct of tsdf.h in its order (the MSRA
 *               constants are 241.42, 160, 120, 1, 3).  They go through the one camera rule of every entry: focal,
 *               invalid_eps and trunc_voxels each > 0, a NaN is not
 *   depth_capacity    floats in d_out_depth: at least n times tsdf_locate_capacity's *per_frame
 *   d_out_depth   float32[depth_capacity]: the crops packed back to back; nothing at or beyond offsets[n] is written
 *   d_out_offsets int64[n + 1]: the exclusive prefix sums of (right - left) * (bottom - top), exact
 *   d_out_headers int32[n][6]: W, H, left, top, right, bottom — a header the voxelizers' header rule accepts
 *   d_out_com     float64[n][3], 8-byte aligned: the centre c
 *   d_out_count   int32[n]: the pixels kept in the crop
 *   d_out_status  int32[n]: 0, 1 (no valid pixel) or 2 (index outside the source frames)
 *   d_out_grid    float32[n][8] or NULL: the CUBE grid row, vox_ori[3], voxel_len, trunc_dis, 0, 0, 0 (what
 *                 tsdf_voxelize_grid_hip takes)
 *   d_out_max_l   float32[n] or NULL, d_out_mid_p float32[n][3] or NULL: they need d_out_grid
 *
 * Contract, per batch position.  Everything is float64 unless it says float32; every product, quotient and sum is
 * rounded on its own (no fma).  F = focal, h = float64(cube) / 2, x the column and y the row of a pixel, d its depth.
 *
 *   1. A pixel is VALID iff d is finite, |d| >= invalid_eps and near <= d <= far (float32 compares; a NaN is invalid).
 *   2. No valid pixel: the position is degenerate (status 1), see below.
 *   3. d_min is the smallest valid depth (float32).  The seed set S is every valid pixel with
 *      float64(d) <= float64(d_min) + float64(seed_band); with seed_band == 0, S is every valid pixel.
 *   4. The centre of a set S — there is no division per pixel.  N = |S|, sd = sum d, sx = sum d * (x - cx),
 *      sy = sum d * (y - cy) (each product rounded, then added):
 *          c_x = (sx / F) / N        c_y = -((sy / F) / N)        c_z = -(sd / N)
 *      The sums run over a reduction tree that is a function of H, W and the rectangle summed over alone — not of n, of
 *      the batch position or of timing; there are no atomics.  Another order moves c by parts in 1e-11.
 *   5. The rectangle of the cube about c, cd = -c_z:
 *          u0 = ((c_x - h) * F) / cd + cx          u1 = ((c_x + h) * F) / cd + cx
 *          v0 = ((-(c_y + h)) * F) / cd + cy       v1 = ((-(c_y - h)) * F) / cd + cy
 *          left  = clamp(floor(u0), 0, W - 1)      right  = clamp(floor(u1) + 1, left + 1, W)
 *          top   = clamp(floor(v0), 0, H - 1)      bottom = clamp(floor(v1) + 1, top + 1, H)
 *      and then right = min(right, left + min(W, s)), bottom = min(bottom, top + min(H, s)) with the s of
 *      tsdf_locate_capacity — which changes nothing unless rounding put a side one pixel over what exact arithmetic
 *      allows; it is what makes the capacity rule a guarantee.
 *   6. `refine` times: S becomes the valid pixels inside the rectangle with |float64(d) - cd| <= h.  If S is not empty,
 *      c becomes its centre (4) and the rectangle is recomputed (5); if it is empty, c and the rectangle stay and the
 *      remaining rounds are skipped (they would find the same).
 *   7. The crop: for the final c and rectangle, row by row, the pixel's depth — copied exactly, or widened exactly —
 *      if it is valid and |float64(d) - cd| <= h, else +0.  d_out_count is the number of pixels kept.
 *   8. The cube grid, float32, one rounding per operation (the reference's glue, pre/tsdf_numba.py:142-147, with
 *      max_l := cube and mid_p := float32(c)):  voxel_len = cube / R, trunc_dis = voxel_len * trunc_voxels,
 *      vox_ori = (mid_p - cube / 2) + voxel_len / 2;  d_out_max_l = cube, d_out_mid_p = float32(c).
 *
 * A degenerate position (status 1) and one whose index is outside the source frames (status 2) write the header
 * [W, H, 0, 0, 1, 1], ONE pixel of +0, c = 0, count 0, a zero grid row, max_l 0 and mid_p 0; the voxelizers then report
 * their own status 1 for it and write a zero volume.
 *
 * Launches: the locating kernel (one workgroup per position), a one-workgroup scan of the sizes into d_out_offsets, and
 * the masked copy (one workgroup per position) — three kernels on hip_stream, nothing handed between workgroups inside
 * a launch.
 *
 * TSDF_ERR_INVALID_ARG, before the device is looked at: n < 0; with n > 0: a frame_type that is neither of the two; a
 * shift outside 0..7 with TSDF_LOCATE_U16; H <= 0 or W <= 0; n_src < 1; d_index == NULL with n_src != n; near not > 0,
 * far not >= near, cube not > 0, seed_band not >= 0 (a NaN fails each); refine outside 0..8; an R that is not a
 * multiple of 4 in 4..128; camera constants that the camera rule refuses; a NULL d_frames, d_out_depth, d_out_offsets,
 * d_out_headers, d_out_com, d_out_count or d_out_status; a d_out_max_l or d_out_mid_p without d_out_grid; a d_frames or
 * d_out_depth not aligned to its element, a d_out_com or d_out_offsets not 8-byte aligned; a depth_capacity below n
 * times the capacity rule's *per_frame.
 */
int tsdf_locate_hip(const void *d_frames, int frame_type, int shift, int64_t n_src, int H, int W, const int64_t *d_index,
                    int n, float near_mm, float far_mm, float cube, float seed_band, int refine, int R, double focal,
                    double cx, double cy, float invalid_eps, float trunc_voxels, int64_t depth_capacity, void *hip_stream,
                    float *d_out_depth, int64_t *d_out_offsets, int32_t *d_out_headers, double *d_out_com,
                    int32_t *d_out_count, int32_t *d_out_status, float *d_out_grid, float *d_out_max_l,
                    float *d_out_mid_p);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_LOCATE_H_ */
