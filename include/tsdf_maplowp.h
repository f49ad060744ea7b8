/*
 * tsdf_maplowp.h — C ABI of libtsdf_maplowp.so: the grid placement under a per-frame map on its own, and the augmented
 * voxel pass on a grid the CALLER supplies written as float16 or bfloat16 voxels.
 *
 * One more extension library next to libtsdf_hip.so (include/tsdf.h, v7, frozen) and libtsdf_augment.so,
 * libtsdf_augstep.so, libtsdf_auggrid.so, libtsdf_depth16.so, libtsdf_obb.so, libtsdf_lowp.so (all v1, frozen): its own
 * translation unit (csrc/tsdf_maplowp.hip), its own binary and its own version number.  It shares the status codes,
 * tsdf_cam and the layout enum of tsdf.h, enum tsdf_lowp_dtype of tsdf_lowp.h and nothing else.  Conventions:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - the calls are asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronise;
 *   - they allocate nothing, use no atomics and no device-side state, never print, have no CPU fallback, are
 *     deterministic and may be captured into a hipGraph (a captured launch is self-contained);
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.  Arguments are checked first, then the device
 *     (TSDF_ERR_NO_DEVICE unless the current device is a gfx950), then the kernel is launched.
 *
 * What it is for: frames are voxelized under a per-frame map (the 3-D augmentation, the principal-axis frame) and the
 * network runs under float16 / bfloat16 autocast.  libtsdf_lowp.so writes 2-byte volumes for the plain path only; the
 * only thing that places a grid on the MAPPED valid pixels is the fused float32 kernel of tsdf_voxelize_aug_hip.
 * tsdf_map_place_hip -> tsdf_voxelize_map_grid_lowp_hip is that entry as two launches with a 2-byte volume: the map's
 * placement, then the augmented voxel pass narrowed in registers.  Both entries draw a batch by index from resident
 * source tables; the maps, the grid rows and every output belong to BATCH POSITIONS.
 */
#ifndef TSDF_MAPLOWP_H_
#define TSDF_MAPLOWP_H_

#include <stdint.h>

#include "tsdf.h"
#include "tsdf_lowp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_MAPLOWP_VERSION 1

/* 1 */
int tsdf_maplowp_version(void);

/*
 * The grid placement of tsdf_voxelize_aug_hip (include/tsdf.h) on its own: the float32 AABB of every valid pixel's
 * back-projected point under the frame's forward map, then the float32 glue and the degenerate-frame rule.
 *
 *   d_depth, depth_len   float32 crops packed back to back, as for tsdf_voxelize_hip
 *   d_offsets  int64[n_src+1]    element offsets into d_depth            }  SOURCE tables, indexed by source frame
 *   d_headers  int32[n_src][6]   W, H, left, top, right, bottom          }
 *   n_src      number of source frames
 *   d_index    int64[n] or NULL: batch position i places the grid of source frame g = d_index ? d_index[i] : i.  With
 *              NULL, n_src must equal n.  A g outside [0, n_src) gives that position TSDF_FRAME_BAD_HEADER, and nothing
 *              is read out of bounds (the rule of tsdf_voxelize_indexed_hip)
 *   n          number of batch positions; 0 is a no-op (TSDF_OK)
 *   R          grid resolution: a multiple of 4 in 4..128
 *   cam        constants, or NULL for the MSRA defaults (focal 241.42, principal point (160, 120), invalid_eps 1,
 *              trunc_voxels 3), restated in this library.
 *              A non-NULL cam whose focal, invalid_eps or trunc_voxels is not > 0 (a NaN is not) is
 *              TSDF_ERR_INVALID_ARG when n > 0, whichever fields the entry reads.
 *   d_xforms   float64[n][24], 8-byte aligned: ONE MAP PER BATCH POSITION (as for tsdf_voxelize_indexed_aug_hip), the
 *              forward rows {A_i0, A_i1, A_i2, b_i} then the inverse rows; only the forward rows are read
 *   d_out_grid   float32[n][8], required: vox_ori[3], voxel_len, trunc_dis, 0, 0, 0 per batch position — the row
 *                tsdf_voxelize_grid_hip, tsdf_voxelize_aug_grid_hip and tsdf_voxelize_map_grid_lowp_hip read.  A position
 *                that is not TSDF_FRAME_OK gets an all-zero row, which every voxel pass answers with a zero volume
 *   d_out_max_l  float32[n] or NULL      }  in the MAPPED frame; 0 for a position that is not OK, except that a
 *   d_out_mid_p  float32[n][3] or NULL   }  zero extent keeps its finite centre
 *   d_out_status int32[n] or NULL: enum tsdf_frame_status per batch position
 *
 * Arithmetic, operation for operation that of oracle/tsdf_oracle.c (tsdf_oracle_aabb_aug, tsdf_oracle_glue and the
 * degenerate rule, chained as in tsdf_oracle_voxelize_aug), for the pixel of column x and row y of the image with
 * depth d (float32):
 *     valid iff |d| >= invalid_eps                             a NaN is invalid
 *     q = (double)d / F                                        the IEEE quotient
 *     p = ( q * (x - cx),  -q * (y - cy),  -(double)d )        one rounding per operation
 *     o_i = fma(A_i0, p_x, fma(A_i1, p_y, fma(A_i2, p_z, b_i)))   the fused chain, then rounded to float32
 *     min_i / max_i over all valid pixels; a NaN o_i moves neither extreme
 *     mid_i = (min_i + max_i) / 2,  len_i = max_i - min_i,  max_l = the largest len_i (a len_i is taken when it is
 *     greater than the running value, which starts as len_x), voxel_len = max_l / R, trunc_dis = voxel_len *
 *     trunc_voxels, vox_ori_i = (mid_i - max_l / 2) + voxel_len / 2          float32, one rounding per operation
 * Minimum and maximum do not depend on the order of their operands, so the result does not depend on how the pixels
 * are split among lanes: a frame's outputs are the same bits wherever it lies in the batch.
 *
 * Per-position status (never fails the call):
 *   TSDF_FRAME_BAD_HEADER (2)  g outside [0, n_src), or the voxelizer's header rule, checked in 64 bits: right <= left,
 *                              bottom <= top, an extent overflowing int32, bbox area != offsets[g+1] - offsets[g], or
 *                              the payload not inside [0, depth_len).  The depth of such a frame is never read.
 *   TSDF_FRAME_DEGENERATE (1)  no valid pixel, or max_l not positive and finite, or a non-finite mid_p.
 *   Otherwise TSDF_FRAME_OK (0).
 * max_l, mid_p and status equal those of tsdf_voxelize_aug_hip for the same frame and map bit for bit.
 *
 * TSDF_ERR_INVALID_ARG, before the device is looked at: n < 0; an R that is not a multiple of 4 in 4..128; with n > 0 a
 * NULL d_depth, d_offsets, d_headers, d_xforms or d_out_grid, depth_len < 0, n_src < 1, d_index == NULL with
 * n_src != n, or a d_xforms that is not 8-byte aligned.
 */
int tsdf_map_place_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                       int64_t n_src, const int64_t *d_index, int n, int R, const tsdf_cam *cam, void *hip_stream,
                       const double *d_xforms, float *d_out_grid, float *d_out_max_l, float *d_out_mid_p,
                       int32_t *d_out_status);

/*
 * The augmented voxel pass of tsdf_voxelize_aug_grid_hip (include/tsdf_auggrid.h), written as 2-byte voxels.
 *
 *   d_depth, depth_len, d_offsets, d_headers, n_src, d_index, n, cam   as for tsdf_map_place_hip (trunc_voxels is
 *              unused: the truncation distance comes with the grid)
 *   R          grid resolution: a multiple of 4 in 4..128
 *   layout     enum tsdf_layout
 *   dtype      enum tsdf_lowp_dtype (include/tsdf_lowp.h)
 *   d_xforms   float64[n][24], 8-byte aligned  }  PER BATCH POSITION, whatever d_index says: position i voxelizes
 *   d_grid     float32[n][8]                   }  source frame g under map i on grid row i (vox_ori[3], voxel_len,
 *                                                 trunc_dis, 3 pad words: what tsdf_map_place_hip writes)
 *   d_out_tsdf   2-byte elements [n][3][R][R][R] in `layout`, 16-byte aligned.  Every byte of it is written by the
 *                launch: the caller need not clear it
 *   d_out_status int32[n] or NULL: enum tsdf_frame_status per batch position
 *
 * Value of a voxel: the float32 value of tsdf_voxelize_aug_grid_hip's contract (include/tsdf_auggrid.h "Arithmetic",
 * == oracle/tsdf_oracle.c::tsdf_oracle_voxels_aug, operation for operation), then narrowed to `dtype` by
 * round-to-nearest-even — the two roundings of include/tsdf_lowp.h: the result is the cast of a float32 volume.  The
 * sign survives the narrowing, also on a zero; float16 subnormal results are produced, not flushed.  A rejected voxel
 * is +0 in all three channels.  NaN and infinity cannot occur in a volume.
 *
 * Per-position status (never fails the call), from the header rule and the grid row alone:
 *   TSDF_FRAME_BAD_HEADER (2)  g outside [0, n_src), or the header rule as above.  The depth is never read.
 *   TSDF_FRAME_DEGENERATE (1)  the grid row is unusable: !(trunc_dis > 0), or a non-finite voxel_len, trunc_dis or
 *                              vox_ori.  The all-zero row tsdf_map_place_hip writes for a position that is not OK is one.
 *   Both give an all-zero volume (+0 in every voxel).  Otherwise TSDF_FRAME_OK (0).
 * THIS ENTRY DOES NOT SCAN THE CROP: a frame without any valid pixel gets a zero volume with status 0 when its grid row
 * is usable.  After tsdf_map_place_hip the placement's status is the one to keep.
 *
 * TSDF_ERR_INVALID_ARG, before the device is looked at: n < 0; an R that is not a multiple of 4 in 4..128, a layout that
 * is not of enum tsdf_layout, a dtype that is not of enum tsdf_lowp_dtype; with n > 0 a NULL d_depth, d_offsets,
 * d_headers, d_xforms, d_grid or d_out_tsdf, depth_len < 0, n_src < 1, d_index == NULL with n_src != n, a d_xforms that
 * is not 8-byte aligned, a d_out_tsdf that is not 16-byte aligned, or a batch whose n * ceil(R / slab) workgroups of 256
 * lanes do not fit one launch (2^32 work-items).
 */
int tsdf_voxelize_map_grid_lowp_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets,
                                    const int32_t *d_headers, int64_t n_src, const int64_t *d_index, int n, int R,
                                    const tsdf_cam *cam, int layout, int dtype, void *hip_stream,
                                    const double *d_xforms, const float *d_grid, void *d_out_tsdf,
                                    int32_t *d_out_status);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_MAPLOWP_H_ */
