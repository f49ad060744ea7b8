/*
 * tsdf_auggrid.h — C ABI of libtsdf_auggrid.so: the augmented voxelization on a grid the CALLER supplies, and the
 * augmented labels on their own.
 *
 * A third extension library next to libtsdf_hip.so (include/tsdf.h, v7, frozen), libtsdf_augment.so and
 * libtsdf_augstep.so (both v1, frozen): its own translation unit (csrc/tsdf_auggrid.hip), its own binary and its own
 * version number.  It shares the status codes, tsdf_cam and the layout enum of tsdf.h and nothing else.  Conventions:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - the calls are asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronise;
 *   - they allocate nothing, use no atomics and no device-side state, never print, have no CPU fallback, are
 *     deterministic and may be captured into a hipGraph (a captured launch is self-contained);
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.  Arguments are checked first, then the device
 *     (TSDF_ERR_NO_DEVICE unless the current device is a gfx950), then the kernel is launched.
 *
 * What it is for: every augmented entry of tsdf.h places its own grid on ALL mapped valid pixels.  The reference's
 * DataProcess.process() (pre/process.py:19-24) does data_aug, then set_length, then tsdf_f on the augmented RESAMPLED
 * cloud.  tsdf_point_clouds_hip(d_xforms) -> tsdf_cloud_grid_hip -> tsdf_voxelize_aug_grid_hip is that pipeline with
 * nothing on the host in between, as tsdf_point_clouds_hip -> tsdf_cloud_grid_hip -> tsdf_voxelize_grid_hip is the plain
 * one.
 */
#ifndef TSDF_AUGGRID_H_
#define TSDF_AUGGRID_H_

#include <stdint.h>

#include "tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_AUGGRID_VERSION 1

/* 1 */
int tsdf_auggrid_version(void);

/*
 * tsdf_voxelize_aug_hip (include/tsdf.h) with the grid placement handed in instead of derived from the mapped pixels —
 * the augmented twin of tsdf_voxelize_grid_hip.
 *
 *   d_depth, depth_len, d_offsets, d_headers, layout   as for tsdf_voxelize_grid_hip
 *   n          number of frames; 0 is a no-op (TSDF_OK), whatever else is passed
 *   R          grid resolution: a multiple of 4 in 4..128
 *   cam        constants, or NULL for the MSRA defaults (focal 241.42, principal point (160, 120), invalid_eps 1),
 *              restated in this library; trunc_voxels is unused (the truncation distance comes with the grid).
 *              A non-NULL cam whose focal, invalid_eps or trunc_voxels is not > 0 (a NaN is not) is
 *              TSDF_ERR_INVALID_ARG when n > 0, whichever fields the entry reads.
 *   d_xforms   float64[n][24], 8-byte aligned: per frame the forward affine map T(p) = A p + b as three rows
 *              {A_i0, A_i1, A_i2, b_i}, then its inverse in the same form (the d_xforms of tsdf_voxelize_aug_hip)
 *   d_grid     float32[n][8]: vox_ori[3], voxel_len, trunc_dis, then 3 pad words per frame — exactly what
 *              tsdf_cloud_grid_hip writes and tsdf_voxelize_grid_hip reads; the grid lives in the MAPPED frame
 *   d_out_tsdf   float32[n][3][R][R][R] in `layout`, 16-byte aligned.  Every byte of it is written by the launch: the
 *                caller need not clear it
 *   d_out_status int32[n] or NULL: enum tsdf_frame_status per frame
 *
 * Arithmetic: that of oracle/tsdf_oracle.c::tsdf_oracle_voxels_aug, operation for operation, float64 with one rounding
 * per operation (fma only where written), for the voxel of index (x, y, z):
 *     v'_a = (double)ori_a + (double)idx_a * (double)voxel_len          product and sum rounded separately
 *     it   = 1.0 / (double)trunc_dis,  iF = 1.0 / F                     per frame
 *     v_i  = (A'_i0 v'_x + A'_i1 v'_y) + (A'_i2 v'_z + b'_i)            T^-1, the inverse rows, in this grouping
 *     q    = -F / v_z                                                   IEEE division
 *     pix_x = trunc_i32(v_x * q + cx),  pix_y = trunc_i32(-v_y * q + cy)   unfused; truncation toward zero, out-of-
 *                                                                       range values saturate and NaN gives 0
 *     the voxel is rejected (0 in all three channels) when the pixel lies outside the bounding box of the header, or
 *     when the depth pd gathered there is not valid: valid iff |pd| >= invalid_eps, so a NaN is invalid
 *     dxi = pix_x - cx,  dyi = pix_y - cy
 *     g_i0 = -(A_i0 * iF),  g_i1 = A_i1 * iF                            per frame, the forward rows
 *     c_i  = fma(g_i0, dxi, fma(g_i1, dyi, A_i2))
 *     u_i  = fma(pd, c_i, v'_i - b_i)
 *     t_i  = u_i * it ;  near iff fma(t_z, t_z, fma(t_y, t_y, t_x * t_x)) <= 1     (no square root)
 *     value_i = near ? min(|t_i|, 1) : 1, negated iff u_z < 0 ; stored as float32
 * With the identity map and the same grid the pixel every voxel gathers, the zero mask, the sign and the z channel equal
 * tsdf_voxelize_grid_hip bit for bit, and x / y agree with it to the float32 rounding.
 *
 * Per-frame status (never fails the call):
 *   TSDF_FRAME_BAD_HEADER (2)  the voxelizer's header rule: right <= left, bottom <= top, an extent overflowing int32,
 *                              bbox area != offsets[i+1] - offsets[i], or the payload not inside [0, depth_len).  The
 *                              depth of such a frame is never read.
 *   TSDF_FRAME_DEGENERATE (1)  the grid row is unusable: !(trunc_dis > 0), or a non-finite voxel_len, trunc_dis or
 *                              vox_ori.  The all-zero row tsdf_cloud_grid_hip writes for a degenerate cloud is one.
 *   Both give an all-zero volume.  Otherwise TSDF_FRAME_OK (0).
 * THIS ENTRY DOES NOT SCAN THE CROP: a frame without any valid pixel simply gets a zero volume with status 0 (every
 * voxel is rejected).  In the pipeline above the cloud stages flag such frames (their cloud is all zero, its grid row
 * all zero, and the volume stage then reports 1 for it as well).
 *
 * TSDF_ERR_INVALID_ARG, before the device is looked at: n < 0; with n > 0 a NULL d_depth, d_offsets, d_headers,
 * d_xforms, d_grid or d_out_tsdf, depth_len < 0, an R that is not a multiple of 4 in 4..128, a layout that is not of
 * enum tsdf_layout, a d_xforms that is not 8-byte aligned, a d_out_tsdf that is not 16-byte aligned, or a batch whose
 * n * ceil(R / slab) workgroups of 256 lanes do not fit one launch (2^32 work-items: more frames than their volumes fit
 * any memory).
 */
int tsdf_voxelize_aug_grid_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets,
                               const int32_t *d_headers, int n, int R, const tsdf_cam *cam, int layout,
                               void *hip_stream, const double *d_xforms, const float *d_grid,
                               float *d_out_tsdf, int32_t *d_out_status);

/*
 * The augmented labels on their own — the reference's data_aug for the joints (pre/process.py:232-249), re-specified
 * like tsdf_labels.d_out_gt_aug of tsdf.h: each joint is mapped with its frame's FORWARD rows,
 *     o_i = fma(A_i0, x, fma(A_i1, y, fma(A_i2, z, b_i)))   in float64, then rounded to float32
 * (oracle/tsdf_oracle.c::tsdf_oracle_transform_joints).  Bit-identical to the d_out_gt_aug tsdf_voxelize_aug_labels_hip
 * writes for the same inputs.
 *
 *   d_gt          float32[n][3*n_joints]  x, y, z per joint, camera frame, mm
 *   d_xforms      float64[n][24], 8-byte aligned (only the forward rows are read)
 *   n_joints      1..170
 *   d_out_gt_aug  float32[n][3*n_joints]
 *
 * n == 0 is a no-op.  n < 0, and with n > 0 a NULL pointer, an n_joints outside 1..170, a misaligned d_xforms or
 * n * n_joints >= 2^32 return TSDF_ERR_INVALID_ARG before any device work.
 */
int tsdf_transform_joints_hip(const float *d_gt, const double *d_xforms, int n, int n_joints, void *hip_stream,
                              float *d_out_gt_aug);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_AUGGRID_H_ */
