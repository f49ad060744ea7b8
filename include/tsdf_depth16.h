/*
 * tsdf_depth16.h — C ABI of libtsdf_depth16.so: depth held as 16-bit integers, widened to the float32 buffer the
 * voxelizer reads.
 *
 * A fifth small library next to libtsdf_hip.so (include/tsdf.h, v7, frozen), libtsdf_augment.so, libtsdf_augstep.so and
 * libtsdf_auggrid.so (all frozen): its own translation unit (csrc/tsdf_depth16.hip), its own binary and its own version
 * number.  It shares the status codes of include/tsdf.h and nothing else.
 *
 * The encoding (packing.py, pack magic TSDFPK02): a pack stores q = depth * 2^k as uint16 with one shift k in 0..7 per
 * pack; the depth is float32(q) * float32(2^-k).  Both steps are exact in float32 (q < 2^16 has at most 16 significant
 * bits, the factor is a power of two and the product is far from the subnormal range), so the widened value IS the
 * float32 depth the pack was encoded from, bit for bit — the encoder refuses any value for which that would not hold.
 *
 * Conventions, as in the other extension headers:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - the device call is asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream), never synchronises;
 *   - no global state, never prints, no CPU fallback;
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.
 */
#ifndef TSDF_DEPTH16_H_
#define TSDF_DEPTH16_H_

#include <stdint.h>

#include "tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_DEPTH16_VERSION 1
#define TSDF_DEPTH16_MAX_SHIFT 7

/* 1 */
int tsdf_depth16_version(void);

/*
 * d_dst[i] = (float)d_src[i] * 2^-shift for 0 <= i < n_px, by one launch on `hip_stream`.  Nothing outside
 * d_dst[0, n_px) is written and nothing outside d_src[0, n_px) is read.
 *
 *   d_src   uint16[n_px]   2-byte aligned; no more is asked (a loader passes slices that start at a frame boundary)
 *   d_dst   float32[n_px]  4-byte aligned; no more is asked.  Must not overlap d_src.
 *   shift   0..TSDF_DEPTH16_MAX_SHIFT
 *
 * Checked before any device call, in this order: n_px < 0 or a shift outside 0..7 return TSDF_ERR_INVALID_ARG;
 * n_px == 0 returns TSDF_OK without a launch, whatever the pointers are; a NULL d_src or d_dst, a d_src that is not
 * 2-byte aligned or a d_dst that is not 4-byte aligned return TSDF_ERR_INVALID_ARG.  A current device that is not a
 * gfx950 returns TSDF_ERR_NO_DEVICE, a launch the runtime rejects TSDF_ERR_LAUNCH.
 */
int tsdf_depth16_widen_hip(const uint16_t *d_src, int64_t n_px, int shift, float *d_dst, void *hip_stream);

/*
 * tsdf_host_gather_frames_n (include/tsdf.h) for a 16-bit payload: frames index[0..n) of the packed HOST buffer src
 * (frame f is src[src_offsets[f], src_offsets[f+1])) are copied back to back into dst, and dst_offsets[n+1] is filled
 * in.  Host memory only; n_threads workers (1..64, clamped) split the bytes, small gathers run on the calling thread.
 *
 * Everything is validated before the first byte is copied, and any violation returns TSDF_ERR_INVALID_ARG with dst
 * untouched: src_len, n_src or n negative; with n > 0 a NULL src, src_offsets, index, dst or dst_offsets; an index
 * outside [0, n_src); offsets that are negative, run backwards or leave [0, src_len] (a damaged pack); a total that
 * exceeds dst_len.  n == 0 writes dst_offsets[0] = 0 when dst_offsets is given and returns TSDF_OK.
 */
int tsdf_depth16_host_gather(const uint16_t *src, int64_t src_len, const int64_t *src_offsets, int64_t n_src,
                             const int64_t *index, int64_t n, uint16_t *dst, int64_t dst_len, int64_t *dst_offsets,
                             int n_threads);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_DEPTH16_H_ */
