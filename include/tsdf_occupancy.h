/*
 * tsdf_occupancy.h — C ABI of libtsdf_occupancy.so: one-channel occupancy volumes, the input of a voxel-to-voxel network
 * (V2V-PoseNet and its family): a voxel is 1 if a point of the frame's back-projected cloud falls inside it, else 0.
 *
 * One more library next to libtsdf_hip.so (include/tsdf.h, v7, frozen), the eleven of csrc/Makefile's EXTS line,
 * libtsdf_heatmap.so and libtsdf_heatloss.so (all v1, frozen): its own translation unit (csrc/tsdf_occupancy.hip), its
 * own binary and its own version number.  It shares the status codes and the layout enum of tsdf.h and the element
 * types of tsdf_heatmap.h (0 for float32, the two of tsdf_lowp.h), and nothing else; the camera's five constants come
 * by value.  Conventions:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - the call is asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronises;
 *   - it allocates nothing, uses no GLOBAL atomics and no device-side state, never prints, has no CPU fallback and may
 *     be captured into a hipGraph (a captured launch is self-contained).  Every volume the other libraries write is a
 *     gather; this one is a scatter, and a workgroup sets the bits of its own LDS mask with an atomic OR.  OR is
 *     commutative and idempotent, so the mask, and with it every output byte, does not depend on the order in which the
 *     lanes arrive: the result is deterministic although an atomic is used;
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.  Arguments are checked first, then the device
 *     (TSDF_ERR_NO_DEVICE unless the current device is a gfx950), then the kernel is launched.
 */
#ifndef TSDF_OCCUPANCY_H_
#define TSDF_OCCUPANCY_H_

#include <stdint.h>

#include "tsdf.h"
#include "tsdf_heatmap.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_OCCUPANCY_VERSION 1

/* 1 */
int tsdf_occupancy_version(void);

/*
 * The launch plan of tsdf_occupancy_hip at resolution R, host code only.  A batch position's R slices of the output's
 * slowest axis are cut into *nslab slabs of *slab slices, the last one shorter when *slab does not divide R; one
 * workgroup per slab holds the slab's voxels as a bit mask of *lds_bytes = 4 * ceil(*slab * R * R / 32) bytes of LDS,
 * at most 64 KiB (two workgroups then share a CU).
 *   slab_hint 0   the library's plan: the fewest slabs the cap allows, of equal size up to rounding (R <= 80: one)
 *   slab_hint > 0 that many slices per workgroup, clamped to what the cap allows and to R
 * TSDF_ERR_INVALID_ARG for an R that is not a multiple of 4 in 4..128, a negative hint or a NULL result pointer.
 */
int tsdf_occupancy_plan(int R, int slab_hint, int *slab, int *nslab, int *lds_bytes);

/*
 * Occupancy volumes of n batch positions on grids the CALLER places.
 *
 *   d_depth, depth_len   float32 crops packed back to back, as for tsdf_voxelize_hip
 *   d_offsets  int64[n_src+1]    element offsets into d_depth            }  SOURCE tables, indexed by source frame
 *   d_headers  int32[n_src][6]   W, H, left, top, right, bottom          }
 *   n_src      number of source frames
 *   d_index    int64[n] or NULL: batch position i takes source frame g = d_index ? d_index[i] : i.  With NULL, n_src
 *              must equal n.  A g outside [0, n_src) gives that position TSDF_FRAME_BAD_HEADER, and nothing is read out
 *              of bounds
 *   n          number of batch positions; 0 is a no-op (TSDF_OK) once R, layout, dtype and slab_hint have passed
 *   R          THIS grid's resolution: a multiple of 4 in 4..128
 *   focal, cx, cy, invalid_eps, trunc_voxels   the camera by value (the MSRA defaults are 241.42, 160, 120, 1, 3).
 *              focal, invalid_eps and trunc_voxels must each be > 0 (a NaN is not); trunc_voxels is otherwise unused
 *   layout     enum tsdf_layout: the last three axes of the output are z, y, x (czyx) or x, y, z (cxyz)
 *   dtype      TSDF_HEATMAP_F32 (0), TSDF_LOWP_F16 or TSDF_LOWP_BF16
 *   slab_hint  0, or slices per workgroup as for tsdf_occupancy_plan.  The result never depends on it
 *   d_xforms   float64[n][24] or NULL, 8-byte aligned: one map per BATCH POSITION, the forward rows {A_i0, A_i1, A_i2,
 *              b_i} then the inverse rows; only the forward rows are read.  NULL: no map
 *   d_max_l    float32[n]      }  per BATCH POSITION: the cube's edge and centre of ANY placement (an AABB, a mapped
 *   d_mid_p    float32[n][3]   }  AABB, a cloud's, a fixed cube), in the mapped frame.  The resolution is this call's R:
 *                                 an 88^3 occupancy goes with a 32^3 TSDF of the same frame
 *   d_out_occ    dtype[n][1][R][R][R] in `layout`, 16-byte aligned.  Every byte of it is written by the launch
 *   d_out_status int32[n] or NULL: enum tsdf_frame_status per batch position
 *
 * Arithmetic.  Float64 unless marked, every operation rounded on its own, no fma anywhere.
 * Per batch position, in float32, one rounding per operation (the glue of every placement here):
 *     voxel_len = max_l / R
 *     ori_a     = (mid_p_a - max_l / 2) + voxel_len / 2                for a = x, y, z
 *     iv        = 1.0 / (double)voxel_len                              float64
 * Per pixel of column x and row y of the image with depth d (float32):
 *     valid iff |d| >= invalid_eps                                     a NaN is invalid
 *     q = (double)d / F
 *     p = ( q * (x - cx),  -(q * (y - cy)),  -(double)d )
 *     o = p                                                            without a map
 *     o_i = (A_i0 * p_x + A_i1 * p_y) + (A_i2 * p_z + b_i)             with one, in this grouping; under identity rows
 *                                                                      this is p bit for bit for a finite point
 *     s_a = (o_a - (double)ori_a) * iv + 0.5
 *     k_a = floor(s_a)
 *     the skin rule:  k_a == -1 and s_a >= -2^-10      ->  k_a = 0
 *                     k_a ==  R and s_a <= R + 2^-10   ->  k_a = R - 1
 *     the point sets voxel (k_x, k_y, k_z) iff 0 <= k_a < R on all three axes; a NaN s_a is outside.  The comparison
 *     is made on the float64 k_a, before any conversion to an integer.
 * The skin rule is there because under a placement derived from the cloud's own extent the extreme point of each axis
 * sits exactly on the grid's face (s = R or s = 0 in exact arithmetic) and the float32 glue moves it by parts in 10^-5
 * of a voxel to either side: without the rule the hand's outermost pixel would be kept or lost by rounding.
 * A voxel is 1.0 in `dtype` if some valid pixel sets it and +0 otherwise.  Voxel (x, y, z) is the voxel of that index in
 * the TSDF volume and in tsdf_joint_heatmaps_hip's volumes of the same frame: a joint whose normalised label is u sits
 * at the voxel coordinate u * R - 0.5, so a point's voxel is floor(u * R) up to the roundings above.
 *
 * Per-position status (never fails the call):
 *   TSDF_FRAME_BAD_HEADER (2)  g outside [0, n_src), or the voxelizer's header rule, checked in 64 bits: right <= left,
 *                              bottom <= top, an extent overflowing int32, bbox area != offsets[g+1] - offsets[g], or
 *                              the payload not inside [0, depth_len).  The depth of such a frame is never read.
 *   TSDF_FRAME_DEGENERATE (1)  otherwise, an unusable row: !(max_l > 0), or a max_l, mid_p_a, voxel_len or ori_a that is
 *                              not finite, or !(voxel_len > 0).
 *   Both give an all-zero volume (+0 in every voxel).  Otherwise TSDF_FRAME_OK (0).
 * THIS ENTRY DOES NOT LOOK FOR "no valid pixel": such a frame gets an all-zero volume with status 0, as from the other
 * entries that voxelize on a caller's grid.  After a placement entry the placement's status is the one to keep.
 *
 * TSDF_ERR_INVALID_ARG, checked in this order before the device is looked at: n < 0; an R that is not a multiple of 4
 * in 4..128; a layout not of enum tsdf_layout; a dtype that is not 0, TSDF_LOWP_F16 or TSDF_LOWP_BF16; slab_hint < 0;
 * (n == 0 returns TSDF_OK here;) a NULL d_depth, d_offsets, d_headers, d_max_l, d_mid_p or d_out_occ; depth_len < 0;
 * n_src < 1; d_index == NULL with n_src != n; a d_xforms that is not 8-byte aligned or a d_out_occ that is not 16-byte
 * aligned; a focal, invalid_eps or trunc_voxels that is not > 0; a batch whose n * nslab workgroups of 512 lanes do not
 * fit one launch (2^32 work-items or more).
 */
int tsdf_occupancy_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                       int64_t n_src, const int64_t *d_index, int n, int R, double focal, double cx, double cy,
                       float invalid_eps, float trunc_voxels, int layout, int dtype, int slab_hint, void *hip_stream,
                       const double *d_xforms, const float *d_max_l, const float *d_mid_p, void *d_out_occ,
                       int32_t *d_out_status);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_OCCUPANCY_H_ */
