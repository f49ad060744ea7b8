/*
 * tsdf_heatmap.h — C ABI of libtsdf_heatmap.so: the voxel heatmap labels of a voxel-to-voxel network — one Gaussian
 * volume per joint, aligned voxel for voxel with the TSDF volume the network reads — and the way back, per joint the
 * peak of a predicted volume as normalised coordinates.
 *
 * One more extension library next to libtsdf_hip.so (include/tsdf.h, v7, frozen) and the eleven of csrc/Makefile's EXTS
 * line (all v1, frozen): its own translation unit (csrc/tsdf_heatmap.hip), its own binary and its own version number.  It
 * shares the status codes and the layout enum of tsdf.h and the 2-byte dtype enum of tsdf_lowp.h, and nothing else; no
 * entry takes a camera.  Conventions:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - the calls are asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronise;
 *   - they allocate nothing, use no atomics and no device-side state, never print, have no CPU fallback, are
 *     deterministic and may be captured into a hipGraph (a captured launch is self-contained);
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.  Arguments are checked first, then the device
 *     (TSDF_ERR_NO_DEVICE unless the current device is a gfx950), then the kernel is launched.
 *
 * Both directions depend on nothing but the normalised label u = (gt - mid_p) / max_l + 0.5 (gt_nor of every entry that
 * writes labels).  Voxel i of a grid has its centre at mid_p - max_l / 2 + (i + 0.5) * max_l / R, so a joint sits at the
 * voxel coordinate c = u * R - 0.5 under every placement and every per-frame map: the grid itself is not an argument.
 *
 * Argument rules of both entries, checked in this order, each TSDF_ERR_INVALID_ARG, before the device is looked at:
 *   n == 0 is a no-op (TSDF_OK) whatever else is passed; n < 0; an R that is not a multiple of 4 in 4..128; n_joints
 *   outside 1..170; a layout not of enum tsdf_layout; a dtype that is not 0 (float32), TSDF_LOWP_F16 or TSDF_LOWP_BF16;
 *   (encode) a sigma that is not finite and > 0, (decode) a radius outside 0..3; a NULL pointer that is not optional; a
 *   volume that is not 16-byte aligned or any other array that is not 4-byte aligned; n * n_joints >= 2^24 (one
 *   workgroup of 256 lanes per joint at least: the launch would not fit 2^32 work-items).
 */
#ifndef TSDF_HEATMAP_H_
#define TSDF_HEATMAP_H_

#include <stdint.h>

#include "tsdf.h"
#include "tsdf_lowp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_HEATMAP_VERSION 1

/* the float32 element type of a volume here; the 2-byte ones are enum tsdf_lowp_dtype's */
#define TSDF_HEATMAP_F32 0

/* 1 */
int tsdf_heatmap_version(void);

/*
 * Encode: one Gaussian volume per (frame, joint).
 *
 *   d_u          float32[n][n_joints][3], columns x, y, z: the normalised labels (the layout of gt_nor)
 *   d_status     int32[n] or NULL: enum tsdf_frame_status per frame, as the voxelizer wrote it
 *   sigma        the Gaussian's standard deviation in voxels of THIS grid
 *   layout       enum tsdf_layout: the last three axes of the output are z, y, x (czyx) or x, y, z (cxyz), the TSDF
 *                volume's own two orders
 *   dtype        0 (float32), TSDF_LOWP_F16 or TSDF_LOWP_BF16
 *   d_out_heat   dtype[n][n_joints][R][R][R], 16-byte aligned.  Every byte of it is written by the launch
 *   d_out_valid  int32[n][n_joints] or NULL
 *
 * Arithmetic, float64 with every operation rounded on its own (no fma).  Per (frame, joint), axis a and index i:
 *     c_a    = (double)u_a * R - 0.5                   exact: a 24-bit significand times an integer <= 128
 *     t      = i - c_a
 *     k      = 1 / (2 * ((double)sigma * (double)sigma))
 *     g_a[i] = exp(-((t * t) * k))
 * and the voxel (ix, iy, iz) is p = (g_z[iz] * g_y[iy]) * g_x[ix], in that order in both layouts, written as
 * (float)p — or +0 when p < 2^-126, so that the result does not depend on a subnormal mode.  A 2-byte dtype stores
 * that float32 narrowed by round-to-nearest-even (two roundings on purpose: the result is the cast of the float32 volume).
 * The peak is 1 where a joint sits on a voxel centre; there is no truncation window.
 *
 * A joint with a non-finite coordinate, or of a frame whose d_status is not 0, gets an all-zero volume (+0) and
 * valid = 0; every other joint gets valid = 1.  A joint outside the cube is valid and gets its tail (which the flush
 * rule may make all zero).
 */
int tsdf_joint_heatmaps_hip(const float *d_u, const int32_t *d_status, int n, int n_joints, int R, float sigma,
                            int layout, int dtype, void *hip_stream, void *d_out_heat, int32_t *d_out_valid);

/*
 * Decode: per (frame, joint) the maximum of a volume and, optionally, a centre of mass about it.
 *
 *   d_heat       dtype[n][n_joints][R][R][R] in `layout`, 16-byte aligned
 *   radius       0..3
 *   d_out_u      float32[n][n_joints][3], columns x, y, z whatever the layout
 *   d_out_peak   float32[n][n_joints] or NULL: the maximum itself (a 2-byte input is widened exactly)
 *   d_out_arg    int32[n][n_joints] or NULL: its linear index within the joint's volume, in memory order
 *
 * The maximum is taken over values compared with `>`: a NaN is never the maximum, and ties (+0 and -0 tie) go to the
 * lowest linear index.  If no element compares (every value is a NaN): arg = -1, peak = NaN, u = 0.5 on every axis.
 *   radius 0:      u_a = (float)((i*_a + 0.5) / R), i* the argmax voxel, the division in float64
 *   radius r > 0:  w = max(h, 0) over the (2r+1)^3 window about the argmax, clipped to the grid (a NaN counts as 0);
 *                  c^_a = sum(w * i_a) / sum(w) in float64, u_a = (float)((c^_a + 0.5) / R).  When sum(w) is not a
 *                  finite number > 0 the radius-0 result is written.
 * One workgroup reads one joint's volume: a batch of few joints at a large R does not fill the device.
 */
int tsdf_heatmap_joints_hip(const void *d_heat, int dtype, int n, int n_joints, int R, int layout, int radius,
                            void *hip_stream, float *d_out_u, float *d_out_peak, int32_t *d_out_arg);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_HEATMAP_H_ */
