/*
 * tsdf_heatloss.h — C ABI of libtsdf_heatloss.so: the training side of the voxel heatmaps of tsdf_heatmap.h.  The squared
 * error of a predicted volume against the Gaussian target of tsdf_joint_heatmaps_hip WITHOUT that target in memory (the
 * kernels regenerate every target voxel from the label, bit for bit the encode's float32), a soft-argmax over the softmax
 * of a whole volume (integral regression, the differentiable counterpart of tsdf_heatmap_joints_hip), and the gradient of
 * each with respect to the prediction.
 *
 * One more extension library next to libtsdf_hip.so (include/tsdf.h, v7, frozen), the eleven of csrc/Makefile's EXTS line
 * and libtsdf_heatmap.so (all v1, frozen): its own translation unit (csrc/tsdf_heatloss.hip), its own binary and its own
 * version number.  It shares the status codes and the layout enum of tsdf.h, the 2-byte dtype enum of tsdf_lowp.h and the
 * float32 dtype code of tsdf_heatmap.h, and nothing else; no entry takes a camera.  Conventions, those of tsdf_heatmap.h:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - the calls are asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronise;
 *   - they allocate nothing, use no atomics and no device-side state, never print, have no CPU fallback, are
 *     deterministic and may be captured into a hipGraph (a captured launch is self-contained);
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.  Arguments are checked first, then the device
 *     (TSDF_ERR_NO_DEVICE unless the current device is a gfx950), then the kernel is launched.
 *
 * A (frame, joint) pair is a "unit"; unit = frame * n_joints + joint.  A volume is dtype[n][n_joints][R][R][R] whose last
 * three axes are z, y, x (czyx) or x, y, z (cxyz); a 2-byte element is widened to float32 exactly before it is used.
 * All arithmetic is float64 with every operation rounded on its own (no fma).
 *
 * Argument rules of the four entries, checked in this order, each TSDF_ERR_INVALID_ARG, before the device is looked at:
 *   n == 0 is a no-op (TSDF_OK) whatever else is passed; n < 0; an R that is not a multiple of 4 in 4..128; n_joints
 *   outside 1..170; a layout not of enum tsdf_layout; a dtype that is not 0 (float32), TSDF_LOWP_F16 or TSDF_LOWP_BF16;
 *   a sigma / beta that is not finite and > 0; a NULL pointer that is not optional; a volume that is not 16-byte
 *   aligned, an array of doubles that is not 8-byte aligned or any other array that is not 4-byte aligned;
 *   n * n_joints >= 2^24.
 *
 * Summation order.  The forward entries sum R^3 terms per unit in an order that is a function of R, dtype and layout
 * alone: a unit's result is the same bits alone and in any batch, and from call to call.
 */
#ifndef TSDF_HEATLOSS_H_
#define TSDF_HEATLOSS_H_

#include <stdint.h>

#include "tsdf.h"
#include "tsdf_heatmap.h"
#include "tsdf_lowp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_HEATLOSS_VERSION 1

/* 1 */
int tsdf_heatloss_version(void);

/*
 * Loss, forward: per unit the sum of squared differences between a prediction and the Gaussian target of its label.
 *
 *   d_pred       dtype[n][n_joints][R][R][R] in `layout`, 16-byte aligned
 *   d_u          float32[n][n_joints][3], columns x, y, z: the normalised labels (gt_nor), as the encode takes them
 *   d_status     int32[n] or NULL: enum tsdf_frame_status per frame
 *   sigma        the Gaussian's standard deviation in voxels of this grid
 *   d_out_sse    float64[n][n_joints], 8-byte aligned
 *   d_out_valid  int32[n][n_joints] or NULL
 *
 * The target of voxel (ix, iy, iz) is the float32 tsdf_joint_heatmaps_hip writes, bit for bit: with the float64 tables
 * g_a[i] = exp(-((t * t) * k)), t = i - ((double)u_a * R - 0.5), k = 1 / (2 * ((double)sigma * (double)sigma)),
 *     p = (g_z[iz] * g_y[iy]) * g_x[ix]      in that order in both layouts
 *     t32 = p < 2^-126 ? +0 : (float)p
 * Per voxel d = (double)pred - (double)t32, and sse[unit] is the float64 sum of d * d over the volume.  A NaN or an
 * infinity in the prediction propagates by IEEE rules into its own unit's sum and no other.
 *
 * A unit with a non-finite label coordinate, or of a frame whose d_status is not 0, is invalid (exactly the encode's
 * rule): sse = 0, valid = 0, and its prediction is not read.  Every other unit gets valid = 1.
 * One workgroup reads one unit's volume: a batch of few units at a large R does not fill the device.
 */
int tsdf_heat_sse_hip(const void *d_pred, int dtype, const float *d_u, const int32_t *d_status, int n, int n_joints, int R,
                      float sigma, int layout, void *hip_stream, double *d_out_sse, int32_t *d_out_valid);

/*
 * Loss, gradient: grad = (float)((double)w[unit] * d) per voxel, d as above.
 *
 *   d_w          float32[n][n_joints]: per unit the upstream gradient times the reduction's factor (2 / count for a mean)
 *   d_out_grad   dtype[n][n_joints][R][R][R] in `layout`, 16-byte aligned: the type and shape of d_pred.  Every byte of it
 *                is written.  d_out_grad == d_pred (in place) is allowed: a voxel is read before it is written, by the
 *                lane that writes it.  Any other overlap of the two is not.
 *
 * For a 2-byte dtype the float32 is narrowed by round-to-nearest-even.  An invalid unit gets +0 in every voxel, whatever
 * w holds (a NaN included), and its prediction is not read.
 */
int tsdf_heat_sse_grad_hip(const void *d_pred, int dtype, const float *d_u, const int32_t *d_status, const float *d_w, int n,
                           int n_joints, int R, float sigma, int layout, void *hip_stream, void *d_out_grad);

/*
 * Soft-argmax, forward: per unit the expectation of the voxel index under softmax(beta * h) over the whole volume.
 *
 *   d_heat       dtype[n][n_joints][R][R][R] in `layout`, 16-byte aligned
 *   beta         the softmax's inverse temperature, finite and > 0
 *   d_out_u      float32[n][n_joints][3], columns x, y, z whatever the layout
 *   d_out_stats  float64[n][n_joints][5], 8-byte aligned, required: (m, Z, c_x, c_y, c_z), what the gradient reads
 *
 *     m    the maximum of the volume under `>` starting from -inf: a NaN is never it (a volume of NaNs alone has m = -inf)
 *     z_i  = exp((double)beta * ((double)h_i - m))
 *     Z    = sum of z_i
 *     c_a  = (sum of z_i * i_a) / Z          for a = x, y, z, i_a the voxel's index on that axis
 *     u_a  = (float)((c_a + 0.5) / R)
 * IEEE propagation does the rest: a volume that holds a NaN, or whose maximum is not finite (all -inf, or a +inf), has
 * NaN in Z, c_a and u_a, and that unit alone.
 * One workgroup reads one unit's volume (twice: the maximum has a sweep of its own).
 */
int tsdf_soft_argmax_hip(const void *d_heat, int dtype, int n, int n_joints, int R, float beta, int layout, void *hip_stream,
                         float *d_out_u, double *d_out_stats);

/*
 * Soft-argmax, gradient with respect to the volume.
 *
 *   d_stats      float64[n][n_joints][5]: the forward's, of the same d_heat and beta
 *   d_grad_u     float32[n][n_joints][3]: the upstream gradient of u, columns x, y, z
 *   d_out_grad   the type and shape of d_heat, 16-byte aligned; every byte is written; d_out_grad == d_heat is allowed
 *
 * grad_i = beta * (z_i / Z) * (sum over a of (double)gu_a * (i_a - c_a)) / R, formed as
 *     s_i = (gu_x * (i_x - c_x) + gu_y * (i_y - c_y)) + gu_z * (i_z - c_z)
 *     k   = (double)beta / (Z * R)           once per unit
 *     grad_i = (float)((z_i * k) * s_i)      z_i recomputed from h_i, m and beta as above
 * narrowed by round-to-nearest-even for a 2-byte dtype.
 */
int tsdf_soft_argmax_grad_hip(const void *d_heat, int dtype, const double *d_stats, const float *d_grad_u, int n,
                              int n_joints, int R, float beta, int layout, void *hip_stream, void *d_out_grad);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_HEATLOSS_H_ */
