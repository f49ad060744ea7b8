/*
 * tsdf_augment.h — C ABI of libtsdf_augment.so: the 3-D augmentation's draws and maps, produced on the GPU.
 *
 * An extension library next to libtsdf_hip.so (include/tsdf.h), whose v7 ABI is frozen: it has its own translation unit
 * (csrc/tsdf_augment.hip), its own binary and its own version number, and shares with the product only the status codes
 * of `enum tsdf_status` and the calling conventions:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - the call is asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronises;
 *   - no global state, never prints, no CPU fallback;
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.
 */
#ifndef TSDF_AUGMENT_H_
#define TSDF_AUGMENT_H_

#include <stdint.h>

#include "tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_AUGMENT_VERSION 1

/* 1 */
int tsdf_augment_version(void);

/*
 * One augmentation per batch position, drawn from a counter: the reference's distributions (pre/process.py:209-216:
 * stretch ~ U(2/3, 3/2) for x and y, two integer angles in [-30, 30) degrees), not its legacy generator's stream.
 *
 *   d_centres      float32[n_src][3]  each frame's un-augmented grid centre (mid_p as tsdf_aabb_hip writes it)
 *   d_index        int64[n] or NULL   batch position i uses frame g = d_index ? d_index[i] : i
 *   key, counter0  the draw of position i depends on (key, counter0 + i) alone: not on n, not on how a range of
 *                  counters is cut into launches, not on d_index
 *   d_out_xforms   float64[n][24]     what tsdf_voxelize_aug_hip reads: forward rows {A_i0, A_i1, A_i2, b_i}, then the
 *                                     rows of the inverse map
 *   d_out_stretch  float64[n] or NULL the stretch drawn
 *   d_out_rot      int32[n][2] or NULL  (rot_xy, rot_z) in degrees
 *
 * Draws.  All integer work is mod 2^64; mix is splitmix64 (add 0x9E3779B97F4A7C15, xor-shift 30, multiply by
 * 0xBF58476D1CE4E5B9, xor-shift 27, multiply by 0x94D049BB133111EB, xor-shift 31).  With c = counter0 + i and
 * h = mix(key + c):
 *     u       = (mix(h + 0) >> 11) * 2^-53
 *     stretch = lo + u * span,  lo = 2.0/3.0, span = 1.5 - lo  (float64; multiply, round, add, round)
 *     rot_xy  = -30 + (((mix(h + 1) >> 32) * 60) >> 32)
 *     rot_z   = -30 + (((mix(h + 2) >> 32) * 60) >> 32)
 *
 * Maps, in float64.  R = Rx(rot_xy) * Ry(rot_xy) * Rz(rot_z) with
 *     Rx(a) = [1 0 0; 0 c s; 0 -s c]   Ry(a) = [c 0 -s; 0 1 0; s 0 c]   Rz(a) = [c s 0; -s c 0; 0 0 1],
 * angles deg * (pi / 180); A = R^T * diag(s, s, 1); m = float64(centre); b = m - A*m.  The inverse is analytic:
 * A^-1 = diag(1/s, 1/s, 1) * R, b^-1 = m - A^-1 * m.  m is a fixed point of both maps.
 *
 * An index outside [0, n_src) gives that row the identity map, stretch = NaN and angles (0, 0); no other row is
 * affected and nothing is read out of bounds.
 *
 * n < 0, n_src < 1 with n > 0, a NULL d_centres or d_out_xforms with n > 0, or a d_out_xforms that is not 8-byte
 * aligned return TSDF_ERR_INVALID_ARG before any device work; n == 0 is a no-op (TSDF_OK).
 */
int tsdf_aug_draw_hip(const float *d_centres, int64_t n_src, const int64_t *d_index, int n,
                      uint64_t key, uint64_t counter0, void *hip_stream,
                      double *d_out_xforms, double *d_out_stretch, int32_t *d_out_rot);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_AUGMENT_H_ */
