/*
 * tsdf_patch.h — C ABI of libtsdf_patch.so: what the 2-D CNNs that read a depth image take (DeepPrior++, A2J, DenseReg,
 * Pose-REN and most NYU / ICVL / BigHand baselines).  From the cube tsdf_locate.h places about the hand: a fixed-size
 * patch [n][S][S] resampled from the cube's image rectangle, its depth normalised by the cube to [-1, 1] with the
 * background at +1, optionally under the in-plane augmentation those networks train with (rotation, scale, shift — a 2x3
 * map per position); the joints in the patch's own normalised (u, v, d) coordinates; and the way back to the camera frame.
 *
 * One more library next to libtsdf_hip.so (include/tsdf.h, v7, frozen), the eleven of csrc/Makefile's EXTS line,
 * libtsdf_heatmap.so, libtsdf_heatloss.so, libtsdf_occupancy.so, libtsdf_fps.so, libtsdf_group.so and
 * libtsdf_pointfield.so (all v1, frozen): its own translation unit (csrc/tsdf_patch.hip), its own binary and its own
 * version number.  It shares the status codes of tsdf.h, the frame encodings of tsdf_locate.h and the 2-byte element
 * codes of tsdf_lowp.h, and nothing else.  Conventions, those of tsdf_locate.h:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - a call is asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronises;
 *   - it allocates nothing, uses no atomics and no device-side state, never prints, has no CPU fallback, is deterministic
 *     (two calls give identical bits; a position gives the same bits alone and at any place of any batch) and may be
 *     captured into a hipGraph (a captured launch is self-contained);
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.  Arguments are checked first, then the device
 *     (TSDF_ERR_NO_DEVICE unless the current device is a gfx950), then the kernel is launched;
 *   - n == 0 is a no-op (TSDF_OK) once the scalar arguments have passed.
 * The camera comes BY VALUE in every entry — focal, cx, cy, invalid_eps, trunc_voxels, the five fields of the camera
 * struct of tsdf.h in its order, as tsdf_locate_hip takes them (the MSRA constants are 241.42, 160, 120, 1, 3) — and goes
 * through the one camera rule of every entry here: focal, invalid_eps and trunc_voxels each > 0, a NaN is not.
 */
#ifndef TSDF_PATCH_H_
#define TSDF_PATCH_H_

#include <stdint.h>

#include "tsdf.h"
#include "tsdf_locate.h" /* TSDF_LOCATE_F32 / TSDF_LOCATE_U16: `frame_type` */
#include "tsdf_lowp.h"   /* TSDF_LOWP_F16 / TSDF_LOWP_BF16: the 2-byte `dtype` codes */

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_PATCH_VERSION 1

#define TSDF_PATCH_F32 0 /* dtype: float32 patches; the 2-byte ones are TSDF_LOWP_F16 (1) and TSDF_LOWP_BF16 (2) */

#define TSDF_PATCH_MIN_SIZE 8   /* S is a multiple of 8 in TSDF_PATCH_MIN_SIZE..TSDF_PATCH_MAX_SIZE */
#define TSDF_PATCH_MAX_SIZE 512
#define TSDF_PATCH_MAX_JOINTS 65536 /* J is in 1..TSDF_PATCH_MAX_JOINTS */

#define TSDF_PATCH_NEAREST 0 /* interp */
#define TSDF_PATCH_BILINEAR 1

/* 1 */
int tsdf_patch_version(void);

/*
 * ARGUMENTS COMMON TO ENTRIES 3 TO 6.
 *   d_com        float64[n][3], 8-byte aligned: the cube centre c of batch position i in the camera frame, mm, c_z = -depth
 *                (tsdf_locate_hip's d_out_com).
 *   cube         float32, the cube's edge in mm; d_cube float32[n] or NULL: where it is non-NULL, d_cube[i] replaces the
 *                scalar for position i (scale augmentation of the cube is per frame) and the scalar is not looked at.
 *                Without d_cube the scalar must be finite and > 0.
 *   d_affine     float64[n][6] or NULL, 8-byte aligned: the row a00 a01 a02 a10 a11 a12 maps PATCH coordinates to SOURCE
 *                coordinates (rule 3).  NULL is the identity.
 *   d_status_in  int32[n] or NULL.  A position with a non-zero entry is not read (status 1).  tsdf_locate_hip's
 *                d_out_status chains.
 *   focal, cx, cy, invalid_eps, trunc_voxels   the camera by value (above).
 *
 * CONTRACT OF A PATCH, per batch position i.  Everything is float64 unless it says otherwise; every product, quotient,
 * sum and difference is rounded on its own (no fma).
 *     F = focal,  h = float64(cube_i) / 2,  rh = 1.0 / h,  cd = -c_z,  rS = 1.0 / float64(S)
 *   1. STATUS.  The position has status 1 (TSDF_FRAME_DEGENERATE) if d_status_in[i] != 0, a component of c is not finite,
 *      cd is not > 0, cube_i is not finite and > 0, or an entry of its affine row is not finite.  Otherwise it has status
 *      2 (TSDF_FRAME_BAD_HEADER) if its source index g = d_index ? d_index[i] : i is outside [0, n_src), or (entry 4) the
 *      header rule of the voxelizers refuses header g: a crop [left, right) x [top, bottom) with right > left,
 *      bottom > top and (right - left) * (bottom - top) == offsets[g + 1] - offsets[g], offsets[g] >= 0 and
 *      offsets[g + 1] <= depth_len is accepted.  Either way every pixel of its patch is `background` and nothing of the
 *      source is read.  Otherwise the status is 0.
 *   2. THE CUBE'S RECTANGLE in continuous image coordinates — tsdf_locate.h step 5 before its floor; a pixel's centre is
 *      at its integer column and row, as there:
 *          u0 = ((c_x - h) * F) / cd + cx          u1 = ((c_x + h) * F) / cd + cx
 *          v0 = ((-(c_y + h)) * F) / cd + cy       v1 = ((-(c_y - h)) * F) / cd + cy
 *          du = u1 - u0                            dv = v1 - v0
 *   3. OUTPUT PIXEL (row i, column j):
 *          a = float64(2j + 1) * rS - 1.0          b = float64(2i + 1) * rS - 1.0
 *          a' = (a00 * a + a01 * b) + a02          b' = (a10 * a + a11 * b) + a12      (NULL affine: a' = a, b' = b)
 *          u = u0 + ((a' + 1.0) * 0.5) * du        v = v0 + ((b' + 1.0) * 0.5) * dv
 *   4. A TAP (x, y), two float64 whole numbers, is VALID iff x and y are finite; left <= x < right and top <= y < bottom,
 *      compared in float64 BEFORE any conversion to an integer (coordinates of 1e30 cannot wrap); its depth d (float32,
 *      or the uint16 widened exactly: float32(u) * 2^-shift) is finite with |d| >= invalid_eps (float32 compares); and
 *      |float64(d) - cd| <= h, the cube's depth test of tsdf_locate.h step 7.  The source rectangle is the whole frame
 *      (left = top = 0, right = W, bottom = H, base = g * H * W) in entry 3 and the header's in entry 4
 *      (base = offsets[g]); the element read is base + (y - top) * (right - left) + (x - left) in 64-bit integers.
 *   5. NEAREST: the one tap is (floor(u + 0.5), floor(v + 0.5)).  Valid: z = (float64(d) - cd) * rh; otherwise the pixel
 *      is `background`.
 *   6. BILINEAR: x0 = floor(u), fx = u - x0, y0 = floor(v), fy = v - y0; the taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1),
 *      (x0 + 1, y0 + 1), in that order, with the weights (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy.
 *      s is the sum of w_k * float64(d_k) and w the sum of w_k over the VALID taps in that order, each starting from +0;
 *      invalid taps are skipped.  With no valid tap, or w == 0, the pixel is `background`.  Otherwise dbar = s if all
 *      four taps are valid, else s / w, and z = (dbar - cd) * rh.  The hand is never blended with the background.
 *   7. z is rounded ONCE to float32; for a 2-byte dtype it is then narrowed by round-to-nearest-even (float16 with
 *      subnormals), and so is `background`.
 * Nothing divides per pixel but s / w at silhouette pixels of the bilinear form.
 */

/*
 * 2. The plan, host code only: a workgroup of 256 lanes serves one ITEM at a time, a band of *rows_per_group consecutive
 * rows of one position's patch; a lane owns *px_per_lane adjacent pixels of one row — 4 (float32) or 8 (2-byte), one
 * 16-byte store —, so a row takes S / *px_per_lane lanes, *rows_per_group = min(S, floor(256 / (S / *px_per_lane))) and
 * a position takes *items_per_position = ceil(S / *rows_per_group) items.  The items of a batch, n * *items_per_position,
 * are walked by a grid-stride loop of at most 4096 workgroups.
 * TSDF_ERR_INVALID_ARG for an S that is not a multiple of 8 in 8..512, a dtype that is not 0, 1 or 2 or a NULL result.
 */
int tsdf_patch_plan(int S, int dtype, int *px_per_lane, int *rows_per_group, int *items_per_position);

/*
 * 3. Patches from raw frames.
 *   d_frames     [n_src][H][W], contiguous, aligned to its element: float32 mm (TSDF_LOCATE_F32) or uint16
 *                (TSDF_LOCATE_U16 with shift 0..7), tsdf_locate.h's encodings
 *   d_index      int64[n] or NULL; with NULL, n_src must equal n
 *   S, interp, dtype, background    the patch's edge, TSDF_PATCH_NEAREST / TSDF_PATCH_BILINEAR, the element type, the
 *                value of a pixel without a valid tap (any float32)
 *   d_out_patch  [n][S][S] of dtype, 16-byte aligned; every byte is written
 *   d_out_status int32[n]
 *
 * TSDF_ERR_INVALID_ARG, in this order, before the device is looked at: n < 0; an S that is not a multiple of 8 in
 * 8..512; an interp that is not 0 or 1; a dtype that is not 0, 1 or 2; a frame_type that is neither of the two; a shift
 * outside 0..7 with TSDF_LOCATE_U16; H <= 0 or W <= 0; n_src < 0; no d_cube and a cube that is not finite and > 0;
 * camera constants the camera rule refuses; (n == 0 returns TSDF_OK here;) n_src < 1; d_index == NULL with n_src != n; a
 * NULL d_frames, d_com, d_out_patch or d_out_status; a d_frames not aligned to its element, a d_com, d_affine or d_index
 * not 8-byte aligned, a d_cube, d_status_in or d_out_status not 4-byte aligned, a d_out_patch not 16-byte aligned.
 */
int tsdf_patch_frames_hip(const void *d_frames, int frame_type, int shift, int64_t n_src, int H, int W,
                          const int64_t *d_index, const double *d_com, float cube, const float *d_cube,
                          const double *d_affine, const int32_t *d_status_in, int n, int S, int interp, int dtype,
                          float background, double focal, double cx, double cy, float invalid_eps, float trunc_voxels,
                          void *hip_stream, void *d_out_patch, int32_t *d_out_status);

/*
 * 4. Patches from a pack: d_depth float32[depth_len], d_offsets int64[n_src + 1], d_headers int32[n_src][6] (W, H, left,
 * top, right, bottom) — the triple every voxelizer here reads and tsdf_locate_hip writes.  The same kernel template and
 * the same contract as entry 3; the source rectangle is the header's.  A tap outside the crop is invalid even where the
 * frame the crop was cut from had a pixel there, so at the crop's right and bottom edge — floor(u + 0.5) can reach the
 * crop's exclusive bound — and under an affine map this entry on tsdf_locate_hip's pack and entry 3 on the frames
 * themselves need NOT agree.
 *
 * TSDF_ERR_INVALID_ARG, in this order: n < 0; S; interp; dtype; depth_len < 0; n_src < 0; cube; the camera; (n == 0
 * returns TSDF_OK here;) n_src < 1; d_index == NULL with n_src != n; a NULL d_depth, d_offsets, d_headers, d_com,
 * d_out_patch or d_out_status; the alignments of entry 3, d_depth and d_headers to 4 bytes, d_offsets to 8.
 */
int tsdf_patch_crops_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                         int64_t n_src, const int64_t *d_index, const double *d_com, float cube, const float *d_cube,
                         const double *d_affine, const int32_t *d_status_in, int n, int S, int interp, int dtype,
                         float background, double focal, double cx, double cy, float invalid_eps, float trunc_voxels,
                         void *hip_stream, void *d_out_patch, int32_t *d_out_status);

/*
 * 5. The labels: camera-frame joints d_joints float32[n][J][3] in the patch's coordinates.  One thread per joint.  With
 * the quantities of the patch contract, for a joint (X, Y, Z):
 *          dj = -Z          u = (X * F) / dj + cx          v = ((-Y) * F) / dj + cy
 *          a' = ((u - u0) / du) * 2.0 - 1.0                b' = ((v - v0) / dv) * 2.0 - 1.0
 *          det = a00 * a11 - a01 * a10
 *          a = (a11 * (a' - a02) - a01 * (b' - a12)) / det
 *          b = (a00 * (b' - a12) - a10 * (a' - a02)) / det
 *          w = (dj - cd) * rh
 *   d_out_uvd float32[n][J][3] = float32(a, b, w), each rounded once; with a NULL affine a = a', b = b'.  A joint inside
 *   the cube and inside the patch is in [-1, 1]^3; nothing is clamped.
 *   d_out_valid int32[n][J]: a joint with a non-finite coordinate or with dj not > 0, and every joint of a position with
 *   status 1, gets uvd = +0 and valid 0; every other joint valid 1.
 *   d_out_status int32[n]: 1 for a position that is status 1 by rule 1 of the patch contract or whose det is 0 or not
 *   finite, else 0.  (There is no source here, so no status 2.)
 *
 * TSDF_ERR_INVALID_ARG, in this order: n < 0; J outside 1..65536; cube; the camera; (n == 0 returns TSDF_OK here;) a NULL
 * d_joints, d_com, d_out_uvd, d_out_valid or d_out_status; a d_com or d_affine not 8-byte aligned, any other pointer
 * not 4-byte aligned; n * J of 2^31 or more.
 */
int tsdf_patch_uvd_hip(const float *d_joints, const double *d_com, float cube, const float *d_cube,
                       const double *d_affine, const int32_t *d_status_in, int n, int J, double focal, double cx,
                       double cy, float invalid_eps, float trunc_voxels, void *hip_stream, float *d_out_uvd,
                       int32_t *d_out_valid, int32_t *d_out_status);

/*
 * 6. The way back: d_uvd float32[n][J][3] (a, b, w) to camera-frame joints.
 *          depth = w * h + cd
 *          a' = (a00 * a + a01 * b) + a02      b' = (a10 * a + a11 * b) + a12      (the forward map of rule 3)
 *          u = u0 + ((a' + 1.0) * 0.5) * du    v = v0 + ((b' + 1.0) * 0.5) * dv
 *          X = ((u - cx) * depth) / F          Y = -(((v - cy) * depth) / F)          Z = -depth
 *   d_out_joints float32[n][J][3] = float32(X, Y, Z), each rounded once.  Every joint of a position that is status 1 by
 *   rule 1 of the patch contract is a row of +0.  Entry 5 followed by this entry returns a joint to within the two
 *   float32 roundings (DESIGN.md has the measured figure).
 *
 * TSDF_ERR_INVALID_ARG: as entry 5, with d_uvd and d_out_joints as the required float32 pointers.
 */
int tsdf_patch_joints_hip(const float *d_uvd, const double *d_com, float cube, const float *d_cube,
                          const double *d_affine, const int32_t *d_status_in, int n, int J, double focal, double cx,
                          double cy, float invalid_eps, float trunc_voxels, void *hip_stream, float *d_out_joints);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_PATCH_H_ */
