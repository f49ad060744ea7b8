/*
 * tsdf_augstep.h — C ABI of libtsdf_augstep.so: the augmentation's draws and maps from a key and counters that live in
 * DEVICE memory.
 *
 * A second extension library next to libtsdf_hip.so (include/tsdf.h, v7, frozen) and libtsdf_augment.so
 * (include/tsdf_augment.h, v1, frozen at two exports): its own translation unit (csrc/tsdf_augstep.hip), its own binary
 * and its own version number.  The conventions are those of tsdf_augment.h:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - the call is asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronises;
 *   - no global state, never prints, no CPU fallback;
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.
 */
#ifndef TSDF_AUGSTEP_H_
#define TSDF_AUGSTEP_H_

#include <stdint.h>

#include "tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_AUGSTEP_VERSION 1

/* 1 */
int tsdf_augstep_version(void);

/*
 * tsdf_aug_draw_hip (include/tsdf_augment.h) with the key and the counters read by the KERNEL instead of passed by the
 * host: the same draws and the same float64[n][24] maps for the same (key, c), centre and index — the same splitmix64
 * chain, stretch and angle formulas, float64 operation order and analytic inverse; that header defines them.
 *
 *   d_centres      float32[n_src][3]  each frame's un-augmented grid centre
 *   d_index        int64[n] or NULL   batch position i uses frame g = d_index ? d_index[i] : i
 *   d_state        uint64[2]          {key, counter0}, read by the launch when it RUNS: whatever was written there
 *                                     earlier on the same stream is what it uses.  A launch captured into a graph
 *                                     therefore draws anew at every replay whose state was rewritten before it.
 *   d_counters     int64[n] or NULL   position i draws from (key, c), c = counter0 + (d_counters ? (uint64_t)d_counters[i]
 *                                     : i) mod 2^64 — with d_counters the counters of a batch need not be contiguous
 *                                     (a frame's own number under a shuffling loader); negative values wrap
 *   d_out_xforms   float64[n][24]     forward rows {A_i0, A_i1, A_i2, b_i}, then the rows of the inverse map
 *   d_out_stretch  float64[n] or NULL the stretch drawn
 *   d_out_rot      int32[n][2] or NULL  (rot_xy, rot_z) in degrees
 *
 * An index outside [0, n_src) gives that row the identity map, stretch = NaN and angles (0, 0); no other row is
 * affected and nothing is read out of bounds.
 *
 * n < 0 returns TSDF_ERR_INVALID_ARG.  With n > 0: a NULL d_centres, d_state or d_out_xforms, n_src < 1, or a d_state or
 * d_out_xforms that is not 8-byte aligned return TSDF_ERR_INVALID_ARG.  All of this before any device work; n == 0 is a
 * no-op (TSDF_OK), whatever else is passed.
 */
int tsdf_aug_draw_at_hip(const float *d_centres, int64_t n_src, const int64_t *d_index, int n,
                         const uint64_t *d_state, const int64_t *d_counters, void *hip_stream,
                         double *d_out_xforms, double *d_out_stretch, int32_t *d_out_rot);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_AUGSTEP_H_ */
