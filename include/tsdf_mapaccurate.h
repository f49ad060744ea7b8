/*
 * tsdf_mapaccurate.h — C ABI of libtsdf_mapaccurate.so: the ACCURATE directional TSDF under a per-frame map, on a grid the
 * caller supplies — per voxel the nearest MAPPED surface point among all valid pixels of the crop, where
 * tsdf_voxelize_aug_grid_hip (include/tsdf_auggrid.h) takes the one pixel the voxel projects to.
 *
 * One more extension library next to libtsdf_hip.so (include/tsdf.h, v7, frozen) and the ten of csrc/Makefile's EXTS line
 * (all v1, frozen), libtsdf_accurate.so among them: its own translation unit (csrc/tsdf_mapaccurate.hip), its own binary
 * and its own version number.  It shares the status codes and the layout enum of tsdf.h and nothing else; the camera's
 * constants come by value.  It combines two contracts and restates neither more than it must: the MAP, the voxel centre,
 * the projected pixel and the distance terms are include/tsdf_auggrid.h's ("Arithmetic"), the SEARCH, the `nearest` output
 * and the status rules are include/tsdf_accurate.h's.  Conventions:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - the calls are asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronise;
 *   - they allocate nothing, use no atomics and no device-side state, never print, have no CPU fallback, are
 *     deterministic and may be captured into a hipGraph (a captured launch is self-contained);
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.  Arguments are checked first, then the device
 *     (TSDF_ERR_NO_DEVICE unless the current device is a gfx950), then the kernel is launched.
 *
 * What it is for: training runs under a per-frame map (the 3-D augmentation, the principal-axis frame), and there the only
 * volume was the projective one.  tsdf_map_place_hip (include/tsdf_maplowp.h) -> this entry is the accurate volume of the
 * augmented step; tsdf_lowp_narrow_hip (include/tsdf_lowp.h) follows it where 2-byte voxels are wanted.
 */
#ifndef TSDF_MAPACCURATE_H_
#define TSDF_MAPACCURATE_H_

#include <stdint.h>

#include "tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_MAPACCURATE_VERSION 1

/* 1 */
int tsdf_mapaccurate_version(void);

/*
 * The accurate voxel pass under per-position maps, on caller-supplied grid rows.
 *
 *   d_depth, depth_len   as for tsdf_voxelize_grid_hip: float32 crops packed back to back
 *   d_offsets  int64[n_src+1]    element offsets into d_depth            }  SOURCE tables, indexed by source frame
 *   d_headers  int32[n_src][6]   W, H, left, top, right, bottom          }  (as tsdf_voxelize_map_grid_lowp_hip)
 *   n_src      number of source frames
 *   d_index    int64[n] or NULL: batch position i voxelizes source frame g = d_index ? d_index[i] : i.  With NULL,
 *              n_src must equal n.  A g outside [0, n_src) gives that position TSDF_FRAME_BAD_HEADER and a zero volume,
 *              and nothing is read out of bounds
 *   n          number of batch positions; 0 is a no-op (TSDF_OK) whatever the camera
 *   R          grid resolution: a multiple of 4 in 4..128
 *   focal, cx, cy, invalid_eps, trunc_voxels
 *              the camera's constants BY VALUE (the MSRA defaults are 241.42, 160, 120, 1, 3).  When n > 0, a focal,
 *              invalid_eps or trunc_voxels that is not > 0 (a NaN is not) is TSDF_ERR_INVALID_ARG; cx and cy are not
 *              judged.  trunc_voxels is otherwise unused: the truncation distance comes with the grid.
 *   layout     enum tsdf_layout
 *   d_xforms   float64[n][24], 8-byte aligned, per BATCH POSITION: the forward affine map T(p) = A p + b as three rows
 *              {A_i0, A_i1, A_i2, b_i}, then its inverse T^-1 = A' p + b' in the same form
 *   d_grid     float32[n][8] per BATCH POSITION: vox_ori[3], voxel_len, trunc_dis, then 3 pad words — what
 *              tsdf_map_place_hip writes; the grid lives in the MAPPED frame
 *   d_out_tsdf    float32[n][3][R][R][R] in `layout`, 16-byte aligned
 *   d_out_nearest int32[n][R][R][R] or NULL, in the index order of ONE channel of the volume in `layout`; 16-byte aligned
 *                 when given
 *   d_out_status  int32[n] or NULL: enum tsdf_frame_status per batch position
 * Every byte of every output that is given is written by the launch: the caller need not clear anything.
 *
 * Value of the voxel of index (x, y, z) of a position whose status is 0.  Float32 parameters are widened to float64 first;
 * float64 with one rounding per operation, fma only where written.
 *   Voxel centre    v'_a = (double)ori_a + (double)idx_a * (double)voxel_len, product and sum rounded separately.
 *   Per position    it = 1.0 / (double)trunc_dis,  iF = 1.0 / F,  g_i0 = -(A_i0 * iF),  g_i1 = A_i1 * iF   (forward rows)
 *   Visibility      include/tsdf_auggrid.h "Arithmetic", operation for operation:
 *                       v_i = (A'_i0 v'_x + A'_i1 v'_y) + (A'_i2 v'_z + b'_i)      the INVERSE rows, in this grouping
 *                       q = -F / v_z (IEEE division), pix_x = trunc_i32(v_x * q + cx), pix_y = trunc_i32((-v_y) * q + cy)
 *                       (unfused; truncation toward zero, saturating, NaN gives 0)
 *                   `rejected` iff that pixel lies outside the bounding box of the header or the depth there is not
 *                   valid;  `negative` iff not rejected and u_z < 0, u_z the third distance term below evaluated at
 *                   (pix_x, pix_y) with the depth gathered there.  The inverse rows serve this projection ONLY.
 *   Candidates      every VALID pixel p of the crop: |d_p| >= invalid_eps (a NaN is invalid, negative depths are valid),
 *                   at image coordinates col = left + (column in the crop), row = top + (row in the crop).  Its scaled
 *                   squared distance s(p) is evaluated by the mapped pass's own sequence with (col, row) in place of
 *                   (pix_x, pix_y):
 *                       dxi = col - cx,  dyi = row - cy
 *                       c_i = fma(g_i0, dxi, fma(g_i1, dyi, A_i2))
 *                       u_i = fma(d_p, c_i, v'_i - b_i)                            v'_i - T(w(p))_i, mm
 *                       t_i = u_i * it
 *                       s   = fma(t_z, t_z, fma(t_y, t_y, t_x * t_x))
 *                   Only the FORWARD rows enter s.  For the pixel a voxel projects to this is
 *                   tsdf_voxelize_aug_grid_hip's own number, so a voxel that is near projectively is near accurately.
 *   Nearest pixel   p* = argmin s(p), ties to the LOWEST row-major crop index.  A NaN s wins no comparison.  Whatever
 *                   cheaper test the kernel places in front of the evaluation discards only candidates whose evaluated s
 *                   provably exceeds min(1, best so far) (csrc/tsdf_mapaccurate.hip and DESIGN.md have the argument).
 *   Near voxel      s(p*) <= 1:  m_i = |t_i(p*)| in float64, set to 1 unless m_i < 1, negated iff `negative` (also on a
 *                   zero), then rounded to float32 — tsdf_voxelize_aug_grid_hip's order, so a voxel whose p* is its
 *                   projected pixel has that entry's bits;  nearest = p*'s row-major crop index (for a crop of 2^31
 *                   pixels or more: that index modulo 2^32).
 *   Far voxel       otherwise, or no valid pixel at all: the mapped projective value, +0 in all three channels if
 *                   rejected, else +1 or -1 in all three by `negative`;  nearest = -1.
 * There is NO special case for the map: a singular or non-finite forward part is just arithmetic — it yields far voxels,
 * or whatever s says.
 *
 * Per-position status (never fails the call), from the header rule and the grid row alone, as
 * tsdf_voxelize_grid_accurate_hip has them:
 *   TSDF_FRAME_BAD_HEADER (2)  g outside [0, n_src), or the voxelizer's header rule, checked in 64 bits.  The depth of
 *                              such a frame is never read.
 *   TSDF_FRAME_DEGENERATE (1)  the POSITION's grid row is unusable: !(trunc_dis > 0), or a non-finite voxel_len,
 *                              trunc_dis or vox_ori.  The all-zero row tsdf_map_place_hip writes for a bad position is one.
 *   Both give an all-zero volume (+0 in every voxel) and nearest = -1 everywhere.  Otherwise TSDF_FRAME_OK (0).
 * A frame without any valid pixel gets a zero volume with status 0: every voxel is rejected and far.
 *
 * Cost: the kernel inverts the forward 3x3 itself and searches, per voxel, the pixel rectangle that can hold a point within
 * trunc_dis of it.  Where that inverse cannot be trusted (a singular, non-finite or badly conditioned forward part) or the
 * voxel lies within the truncation distance of the camera plane, there is no rectangle and the WHOLE crop is searched.
 *
 * TSDF_ERR_INVALID_ARG, before the device is looked at: n < 0; an R that is not a multiple of 4 in 4..128, a layout that
 * is not of enum tsdf_layout; with n > 0 a NULL d_depth, d_offsets, d_headers, d_xforms, d_grid or d_out_tsdf,
 * depth_len < 0, n_src < 1, d_index == NULL with n_src != n, a d_xforms that is not 8-byte aligned, a d_out_tsdf or a
 * non-NULL d_out_nearest that is not 16-byte aligned, a focal, invalid_eps or trunc_voxels that is not > 0, or a batch
 * whose n * ceil(R / slab) workgroups of 256 lanes do not fit one launch (2^32 work-items).
 */
int tsdf_voxelize_map_grid_accurate_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets,
                                        const int32_t *d_headers, int64_t n_src, const int64_t *d_index, int n, int R,
                                        double focal, double cx, double cy, float invalid_eps, float trunc_voxels,
                                        int layout, void *hip_stream, const double *d_xforms, const float *d_grid,
                                        float *d_out_tsdf, int32_t *d_out_nearest, int32_t *d_out_status);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_MAPACCURATE_H_ */
