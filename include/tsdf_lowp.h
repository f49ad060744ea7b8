/*
 * tsdf_lowp.h — C ABI of libtsdf_lowp.so: the plain voxel pass on a grid the CALLER supplies, written as float16 or
 * bfloat16 voxels, and the same narrowing for float32 values the caller already has.
 *
 * One more extension library next to libtsdf_hip.so (include/tsdf.h, v7, frozen) and libtsdf_augment.so,
 * libtsdf_augstep.so, libtsdf_auggrid.so, libtsdf_depth16.so, libtsdf_obb.so (all v1, frozen): its own translation unit
 * (csrc/tsdf_lowp.hip), its own binary and its own version number.  It shares the status codes, tsdf_cam and the layout
 * enum of tsdf.h and nothing else.  Conventions:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - the calls are asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronise;
 *   - they allocate nothing, use no atomics and no device-side state, never print, have no CPU fallback, are
 *     deterministic and may be captured into a hipGraph (a captured launch is self-contained);
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.  Arguments are checked first, then the device
 *     (TSDF_ERR_NO_DEVICE unless the current device is a gfx950), then the kernel is launched.
 *
 * What it is for: the consumer of the volumes is a 3-D CNN trained under float16 / bfloat16 autocast.  Every other entry
 * writes float32[n][3][R][R][R], which the caller then casts: one full write, one full re-read and one half write of the
 * volume.  This library narrows in registers and writes the half-size volume once.
 */
#ifndef TSDF_LOWP_H_
#define TSDF_LOWP_H_

#include <stdint.h>

#include "tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_LOWP_VERSION 1

/* the 2-byte element type of an output */
enum tsdf_lowp_dtype {
  TSDF_LOWP_F16 = 1,  /* IEEE binary16 */
  TSDF_LOWP_BF16 = 2  /* bfloat16: the upper half of a binary32 */
};

/* 1 */
int tsdf_lowp_version(void);

/*
 * The plain voxel pass of tsdf_voxelize_grid_hip (include/tsdf.h), written as 2-byte voxels.
 *
 *   d_depth, depth_len   as for tsdf_voxelize_grid_hip: float32 crops packed back to back
 *   d_offsets  int64[n_src+1]    element offsets into d_depth            }
 *   d_headers  int32[n_src][6]   W, H, left, top, right, bottom          }  SOURCE tables, indexed by source frame
 *   d_grid     float32[n_src][8] vox_ori[3], voxel_len, trunc_dis, then  }
 *                                3 pad words: the rows of tsdf_voxelize_grid_hip
 *   n_src      number of source frames
 *   d_index    int64[n] or NULL: batch position i voxelizes source frame g = d_index ? d_index[i] : i.  With NULL,
 *              n_src must equal n.  A g outside [0, n_src) gives that position TSDF_FRAME_BAD_HEADER and a zero volume,
 *              and nothing is read out of bounds (the rule of tsdf_voxelize_indexed_hip)
 *   n          number of batch positions; 0 is a no-op (TSDF_OK)
 *   R          grid resolution: a multiple of 4 in 4..128
 *   cam        constants, or NULL for the MSRA defaults (focal 241.42, principal point (160, 120), invalid_eps 1),
 *              restated in this library; trunc_voxels is unused (the truncation distance comes with the grid).
 *              A non-NULL cam whose focal, invalid_eps or trunc_voxels is not > 0 (a NaN is not) is
 *              TSDF_ERR_INVALID_ARG when n > 0, whichever fields the entry reads.
 *   layout     enum tsdf_layout
 *   dtype      enum tsdf_lowp_dtype
 *   d_out_tsdf   2-byte elements [n][3][R][R][R] in `layout`, 16-byte aligned.  Every byte of it is written by the
 *                launch: the caller need not clear it
 *   d_out_status int32[n] or NULL: enum tsdf_frame_status per batch position
 *
 * Value of a voxel: the float32 value of the plain contract (include/tsdf.h, tsdf_voxelize_hip "Arithmetic"), then
 * narrowed to `dtype` by round-to-nearest-even.  Two roundings on purpose, float64 -> float32 -> 2 bytes: the result is
 * the cast of a float32 volume, not a third number system.
 *
 * The float32 value, operation for operation — the order of the product's plain pass (csrc/phase2.inc::voxel_values4
 * and the tables that feed it), float64 with one rounding per operation, fma only where written, for the voxel of index
 * (x, y, z); float32 parameters are widened to float64 first:
 *     v_a   = ori_a + idx_a * voxel_len                      product and sum rounded separately
 *     it    = 1 / trunc_dis,  kq = (1 / F) * it              per frame
 *     vs_a  = v_a * it                                       the centre pre-scaled by 1 / trunc_dis
 *     q     = -F / v_z                                       IEEE division
 *     pix_x = trunc_i32(v_x * q + cx),  pix_y = trunc_i32((-v_y) * q + cy)
 *                                                            unfused; truncation toward zero, out-of-range values
 *                                                            saturate and NaN gives 0 (v_cvt_i32_f64)
 *     the voxel is rejected (+0 in all three channels) when the pixel lies outside the bounding box of the header, or
 *     when the depth pd gathered there is not valid: valid iff |pd| >= invalid_eps, so a NaN is invalid
 *     dxi = pix_x - cx,  dyi = pix_y - cy
 *     tz  = fma(pd, it, vs_z)                                (v_z - w_z) / trunc_dis, w_z = -pd
 *     a   = pd * kq
 *     tx  = fma(-dxi, a, vs_x),  ty = fma(dyi, a, vs_y)
 *     near iff fma(tz, tz, fma(ty, ty, tx * tx)) <= 1        (no square root)
 *     value_c = near ? min(|(float)t_c|, 1) : 1, negated iff w_z > v_z, i.e. iff pd < the smallest float32 >= -v_z
 * (The product forms dxi as (first column of its gather rectangle - cx) + relative column; with a principal point for
 * which both are exact — any cx, cy with a short binary fraction, the defaults among them — the two are the same
 * number.)  The sign survives the narrowing, also on a zero; float16 subnormal results are produced, not flushed.
 * NaN and infinity cannot occur in a volume.
 *
 * Per-position status (never fails the call), from the header rule and the grid row alone:
 *   TSDF_FRAME_BAD_HEADER (2)  g outside [0, n_src), or the voxelizer's header rule, checked in 64 bits: right <= left,
 *                              bottom <= top, an extent overflowing int32, bbox area != offsets[g+1] - offsets[g], or
 *                              the payload not inside [0, depth_len).  The depth of such a frame is never read.
 *   TSDF_FRAME_DEGENERATE (1)  the grid row is unusable: !(trunc_dis > 0), or a non-finite voxel_len, trunc_dis or
 *                              vox_ori.
 *   Both give an all-zero volume (+0 in every voxel).  Otherwise TSDF_FRAME_OK (0).
 * THIS ENTRY DOES NOT SCAN THE CROP: a frame without any valid pixel gets a zero volume with status 0 (every voxel is
 * rejected) where tsdf_voxelize_grid_hip reports 1 for it.
 *
 * TSDF_ERR_INVALID_ARG, before the device is looked at: n < 0; an R that is not a multiple of 4 in 4..128, a layout that
 * is not of enum tsdf_layout, a dtype that is not of enum tsdf_lowp_dtype; with n > 0 a NULL d_depth, d_offsets,
 * d_headers, d_grid or d_out_tsdf, depth_len < 0, n_src < 1, d_index == NULL with n_src != n, a d_out_tsdf that is not
 * 16-byte aligned, or a batch whose n * ceil(R / slab) workgroups of 256 lanes do not fit one launch (2^32 work-items).
 */
int tsdf_voxelize_grid_lowp_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets,
                                const int32_t *d_headers, int64_t n_src, const int64_t *d_index, int n, int R,
                                const tsdf_cam *cam, int layout, int dtype, void *hip_stream,
                                const float *d_grid, void *d_out_tsdf, int32_t *d_out_status);

/*
 * The same narrowing applied to float32 values the caller already has: d_out[k] = round-to-nearest-even of d_in[k] in
 * `dtype`, for k in [0, count).  Ties go to the even 2-byte pattern, the sign survives (also on a zero), float16
 * subnormals are produced, a magnitude beyond the type's largest finite value rounds to infinity as IEEE says, infinity
 * stays infinity and a NaN stays a quiet NaN.  It is the cast for volumes that are already float32, and it is how the
 * narrowing is tested on chosen bit patterns.
 *
 *   d_in    float32[count], 16-byte aligned
 *   count   any number >= 0; 0 is a no-op (TSDF_OK)
 *   d_out   2-byte elements [count], 16-byte aligned
 * A lane takes 8 elements (two 16-byte loads, one 16-byte store); the last count % 8 elements are converted one by one.
 *
 * count < 0, a dtype not of enum tsdf_lowp_dtype, and with count > 0 a NULL or misaligned d_in or d_out return
 * TSDF_ERR_INVALID_ARG before any device work.
 */
int tsdf_lowp_narrow_hip(const float *d_in, int64_t count, int dtype, void *hip_stream, void *d_out);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_LOWP_H_ */
