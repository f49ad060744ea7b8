/*
 * tsdf_obb.h — C ABI of libtsdf_obb.so: per-frame principal-axis (oriented-bounding-box) maps computed on the GPU.
 *
 * A sixth library next to libtsdf_hip.so (include/tsdf.h, v7, frozen) and the four extensions libtsdf_augment.so,
 * libtsdf_augstep.so, libtsdf_auggrid.so and libtsdf_depth16.so (all v1, frozen): its own translation unit
 * (csrc/tsdf_obb.hip), its own binary and its own version number.  It shares the status codes and tsdf_cam of tsdf.h and
 * nothing else.  Conventions:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - the call is asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronises;
 *   - it allocates nothing, uses no atomics and no device-side state, never prints, has no CPU fallback, is deterministic
 *     and may be captured into a hipGraph (a captured launch is self-contained);
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.  Arguments are checked first, then the device
 *     (TSDF_ERR_NO_DEVICE unless the current device is a gfx950), then the kernel is launched.
 *
 * What it is for: every voxelizer entry cuts its volume in the camera's axes, so the same hand turned in the image plane
 * gives another volume and other normalised labels.  The standard alternative of hand-pose pipelines (HandPointNet) is the
 * oriented bounding box: turn each cloud into its own principal axes first.  tsdf_voxelize_aug_hip (include/tsdf.h) takes
 * any per-frame affine map float64[n][24], places the grid on the mapped cloud and maps the joints; this library writes
 * that map from the depth alone: the cloud's mean and covariance over all valid pixels, a 3x3 symmetric eigen-
 * decomposition and a deterministic choice of signs.  The map is a rigid motion, so distances between joints, and pose
 * error, are the same in the mapped frame as in the camera's.
 */
#ifndef TSDF_OBB_H_
#define TSDF_OBB_H_

#include <stdint.h>

#include "tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_OBB_VERSION 1

/* 1 */
int tsdf_obb_version(void);

/*
 * The principal-axis map of every frame of a packed batch.
 *
 *   d_depth, depth_len, d_offsets, d_headers   the packed frames, as for tsdf_voxelize_hip: float32[depth_len] crops back
 *              to back, int64[n+1] element offsets, int32[n][6] = W, H, left, top, right, bottom
 *   n          number of frames; 0 is a no-op (TSDF_OK), whatever else is passed
 *   cam        constants, or NULL for the MSRA defaults (focal 241.42, principal point (160, 120), invalid_eps 1),
 *              restated in this library; trunc_voxels is unused.
 *              A non-NULL cam whose focal, invalid_eps or trunc_voxels is not > 0 (a NaN is not) is
 *              TSDF_ERR_INVALID_ARG when n > 0, whichever fields the entry reads.
 *   d_out_xforms   float64[n][24], 8-byte aligned: per frame the forward map T(p) = A p + b as three rows
 *                  {A_i0, A_i1, A_i2, b_i}, then its inverse in the same form — the d_xforms of tsdf_voxelize_aug_hip
 *   d_out_moments  float64[n][16], 8-byte aligned, or NULL: N, mu[3], C as xx xy xz yy yz zz, lambda[3] descending,
 *                  3 pad words (written 0)
 *   d_out_status   int32[n] or NULL: enum tsdf_frame_status per frame
 *
 * Arithmetic, all of it float64 with one rounding per operation (fma only where written):
 *
 *   Valid pixel   |d| >= cam->invalid_eps, so a NaN is invalid — the voxelizer's rule, because the map feeds the
 *                 voxelizer.
 *   Point of pixel (row i, column j) of the crop:
 *       s = (double)d / F                 IEEE division
 *       x = ((left + j) - cx) * s         left + j exact in int32, converted, cx subtracted
 *       y = -(((top + i) - cy) * s)
 *       z = -(double)d
 *   Moments       N = number of valid pixels, mu = (sum p) / N, C = (sum (p - mu)(p - mu)^T) / N (divisor N), in two
 *                 passes over the crop: the first sums p, the second sums the six products of q = p - mu as
 *                 acc = fma(q_a, q_b, acc).  Never sum p p^T - N mu mu^T.
 *       Summation order (fixed; it is a function of the crop's width and height alone, NOT of where the frame lies in
 *       d_depth, of n, or of any other frame — two calls give identical bits, and a frame alone gives the bits it gives
 *       in any batch):  the workgroup has 16 waves of 64 lanes.  Wave w takes rows w, w + 16, ... in ascending order; in a
 *       row, lane l takes the column groups 4(l + 64v) .. 4(l + 64v) + 3 for v = 0, 1, ... (columns ascending inside a
 *       group), and after the groups lane l < W mod 4 takes the one remaining column 4 floor(W / 4) + l.  Each lane adds its
 *       pixels to its own accumulators in that order.  The lanes of a wave are then added by a butterfly, partner lane
 *       l xor 32, 16, 8, 4, 2, 1 in this order (v = v + partner's v), and the 16 wave sums are added in wave order
 *       starting from wave 0's.
 *   Eigen-decomposition   cyclic Jacobi on C, eigenvector matrix V starting from the identity; a sweep visits the pairs
 *                 (p, q) = (0,1), (0,2), (1,2).  Before every sweep: stop when
 *                 C01^2 + C02^2 + C12^2 (summed left to right) <= (2^-53 * trace)^2, trace = (Cxx + Cyy) + Czz of the
 *                 moments; at most 12 sweeps.  A pair with C_pq == 0 is skipped; otherwise
 *                     theta = (C_qq - C_pp) / (2 * C_pq)
 *                     t = 1 / (|theta| + sqrt(theta * theta + 1)), negated iff theta < 0
 *                     c = 1 / sqrt(t * t + 1),  s = t * c
 *                     C_pp = C_pp - t * C_pq,  C_qq = C_qq + t * C_pq,  C_pq = 0
 *                     with r the third index:  C_rp' = c * C_rp - s * C_rq,  C_rq' = s * C_rp + c * C_rq
 *                     for every row k of V:    V_kp' = c * V_kp - s * V_kq,  V_kq' = s * V_kp + c * V_kq
 *                 The eigenvalues are the diagonal, sorted descending with their columns of V by the exchanges
 *                 (0,1), (1,2), (0,1), each made only when the later one is strictly larger: ties keep their order.
 *   Axes and signs (HandPointNet's convention)
 *                 e1 = the column of the largest eigenvalue, negated iff e1.y < 0
 *                 e3 = the column of the smallest, negated iff e3.z < 0
 *                 e2 = e3 x e1 (products and differences rounded separately): right-handed, det +1
 *                 A component that is exactly 0 leaves the sign alone.
 *   Map           a rotation about the centroid: A has the rows e1, e2, e3,
 *                     b_i = mu_i - fma(A_i0, mu_x, fma(A_i1, mu_y, A_i2 * mu_z))
 *                 and the inverse rows are A^T and mu - A^T mu, formed the same way: T(p) = A (p - mu) + mu, the form of
 *                 augment.py with the centroid for centre.
 *
 * Per-frame status (never fails the call):
 *   TSDF_FRAME_BAD_HEADER (2)  the voxelizer's header rule, checked in 64 bits: right <= left, bottom <= top, an extent
 *                              overflowing int32, bbox area != offsets[i+1] - offsets[i], or the payload not inside
 *                              [0, depth_len).  The depth of such a frame is never read; its N is 0.
 *   TSDF_FRAME_DEGENERATE (1)  N < 3, a non-finite mean or covariance, or trace == 0.
 *   Both give the identity map (A = A^-1 = I, b = 0) and zero moments, N kept.
 *   Otherwise TSDF_FRAME_OK (0).  A rank-deficient covariance (a line, a plane) is OK: the result is still a rotation.
 *
 * TSDF_ERR_INVALID_ARG, before the device is looked at: n < 0; with n > 0 a NULL d_depth, d_offsets, d_headers or
 * d_out_xforms, depth_len < 0, a d_out_xforms or d_out_moments that is not 8-byte aligned, or a d_out_status that is not
 * 4-byte aligned.
 */
int tsdf_obb_xforms_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets,
                        const int32_t *d_headers, int n, const tsdf_cam *cam, void *hip_stream,
                        double *d_out_xforms, double *d_out_moments, int32_t *d_out_status);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_OBB_H_ */
