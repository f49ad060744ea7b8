/*
 * tsdf_accurate.h — C ABI of libtsdf_accurate.so: the ACCURATE directional TSDF on a grid the caller supplies — per voxel
 * the nearest surface point among ALL valid pixels of the crop, not the one pixel the voxel projects to.
 *
 * One more extension library next to libtsdf_hip.so (include/tsdf.h, v7, frozen) and libtsdf_augment.so,
 * libtsdf_augstep.so, libtsdf_auggrid.so, libtsdf_depth16.so, libtsdf_obb.so, libtsdf_lowp.so, libtsdf_maplowp.so,
 * libtsdf_mapstep.so, libtsdf_locate.so (all v1, frozen): its own translation unit (csrc/tsdf_accurate.hip), its own binary
 * and its own version number.  It shares the status codes and the layout enum of tsdf.h and nothing else; the camera's
 * constants come by value.  Conventions:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - the calls are asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronise;
 *   - they allocate nothing, use no atomics and no device-side state, never print, have no CPU fallback, are
 *     deterministic and may be captured into a hipGraph (a captured launch is self-contained);
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.  Arguments are checked first, then the device
 *     (TSDF_ERR_NO_DEVICE unless the current device is a gfx950), then the kernel is launched.
 *
 * What it is for: every other voxelizer here computes the PROJECTIVE directional TSDF (pre/tsdf_numba.py:15-72): a voxel
 * is projected into the image, the pixel it lands on supplies "the closest surface point", and a voxel whose pixel is
 * empty is rejected.  Ge et al. (CVPR 2017, section 3.1) define that as the cheap approximation of the accurate D-TSDF —
 * the nearest point of the whole cloud — and report the latter as the better input.  The voxels beside the silhouette,
 * which the projective pass rejects although a surface point lies within the truncation distance, get their value here.
 */
#ifndef TSDF_ACCURATE_H_
#define TSDF_ACCURATE_H_

#include <stdint.h>

#include "tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_ACCURATE_VERSION 1

/* 1 */
int tsdf_accurate_version(void);

/*
 * The accurate voxel pass on caller-supplied grid rows.
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
 *   n          number of batch positions; 0 is a no-op (TSDF_OK) whatever the camera
 *   R          grid resolution: a multiple of 4 in 4..128
 *   focal, cx, cy, invalid_eps, trunc_voxels
 *              the camera's constants BY VALUE (the MSRA defaults are 241.42, 160, 120, 1, 3).  When n > 0, a focal,
 *              invalid_eps or trunc_voxels that is not > 0 (a NaN is not) is TSDF_ERR_INVALID_ARG; cx and cy are not
 *              judged.  trunc_voxels is otherwise unused: the truncation distance comes with the grid.
 *   layout     enum tsdf_layout
 *   d_out_tsdf    float32[n][3][R][R][R] in `layout`, 16-byte aligned
 *   d_out_nearest int32[n][R][R][R] or NULL, in the index order of ONE channel of the volume in `layout`; 16-byte aligned
 *                 when given
 *   d_out_status  int32[n] or NULL: enum tsdf_frame_status per batch position
 * Every byte of every output that is given is written by the launch: the caller need not clear anything.
 *
 * Value of the voxel of index (x, y, z) of a frame whose status is 0.  Float32 parameters are widened to float64 first.
 *   Voxel centre    v_a = ori_a + idx_a * voxel_len, float64, product and sum rounded separately: the plain contract's
 *                   centre (include/tsdf.h, tsdf_voxelize_hip "Arithmetic"; include/tsdf_lowp.h).
 *   Candidates      every VALID pixel p of the crop: |d_p| >= invalid_eps (a NaN is invalid; negative depths are valid,
 *                   as everywhere here).  With col = left + (column in the crop), row = top + (row in the crop) — image
 *                   coordinates — its point is
 *                       w(p) = ((col - cx) * d_p / F, -(row - cy) * d_p / F, -d_p)
 *                   and its scaled squared distance s(p) = |v - w(p)|^2 / trunc_dis^2, both defined over the reals on
 *                   the float32 inputs.
 *   Nearest pixel   p* = argmin s(p), ties to the LOWEST row-major crop index.  The kernel evaluates s in float64 with
 *                   an absolute error of at most 2^-40 for s <= 2 (coordinates and depths below 2^24 truncation
 *                   distances), as
 *                       it = 1 / trunc_dis,  kq = (1 / F) * it,  vs_a = v_a * it,  a = d_p * kq
 *                       tz = fma(d_p, it, vs_z),  tx = fma(-(col - cx), a, vs_x),  ty = fma(row - cy, a, vs_y)
 *                       s  = fma(tz, tz, fma(ty, ty, tx * tx))
 *                   — for the pixel a voxel projects to this is the plain contract's own sequence, number for number.
 *                   Whatever cheaper test the kernel places in front of that evaluation discards only candidates that
 *                   provably have s > min(1, best so far) (csrc/tsdf_accurate.hip and DESIGN.md have the argument).
 *   Visibility      `projected`, `rejected` and `negative` are the plain contract's pixel of this voxel, its rejection
 *                   and its sign rule, evaluated operation for operation as include/tsdf_lowp.h writes them:
 *                       q = -F / v_z (IEEE division), pix_x = trunc_i32(v_x * q + cx), pix_y = trunc_i32((-v_y) * q + cy)
 *                       (unfused; truncation toward zero, saturating, NaN gives 0)
 *                       rejected iff the pixel lies outside the bounding box of the header or the depth pd there is
 *                       not valid;  negative iff w_z > v_z, i.e. iff pd < the smallest float32 >= -v_z (defined only
 *                       when not rejected).
 *                   A voxel whose ray meets no surface lies in free space: positive.
 *   Near voxel      s(p*) <= 1:  value_c = min(|(float)t_c(p*)|, 1) as float32, negated (also on a zero) iff the voxel
 *                   is not rejected and `negative`;  nearest = p*'s row-major crop index (for a crop of 2^31 pixels or
 *                   more: that index modulo 2^32).
 *   Far voxel       otherwise, or no valid pixel at all: THE PLAIN CONTRACT'S VALUE, +0 in all three channels if
 *                   rejected, else +1 or -1 in all three by the sign rule;  nearest = -1.  (A voxel that is near
 *                   projectively is near accurately, its projected pixel being a candidate evaluated by the same
 *                   sequence: a far voxel's plain value is only ever 0 or +-1.)
 *
 * Per-position status (never fails the call), from the header rule and the grid row alone:
 *   TSDF_FRAME_BAD_HEADER (2)  g outside [0, n_src), or the voxelizer's header rule, checked in 64 bits: right <= left,
 *                              bottom <= top, an extent overflowing int32, bbox area != offsets[g+1] - offsets[g], or
 *                              the payload not inside [0, depth_len).  The depth of such a frame is never read.
 *   TSDF_FRAME_DEGENERATE (1)  the grid row is unusable: !(trunc_dis > 0), or a non-finite voxel_len, trunc_dis or
 *                              vox_ori.
 *   Both give an all-zero volume (+0 in every voxel) and nearest = -1 everywhere.  Otherwise TSDF_FRAME_OK (0).
 * A frame without any valid pixel gets a zero volume with status 0, as in tsdf_voxelize_grid_lowp_hip: every voxel is
 * rejected and far.
 *
 * Cost: a voxel whose depth interval [-v_z - trunc_dis, -v_z + trunc_dis] stays on one side of zero by invalid_eps has a
 * finite pixel window and the kernel searches that; a voxel within the truncation distance of the camera plane has none
 * and the WHOLE crop is searched for it (76,800 candidates per voxel on a full 320 x 240 frame).
 *
 * TSDF_ERR_INVALID_ARG, before the device is looked at: n < 0; an R that is not a multiple of 4 in 4..128, a layout that
 * is not of enum tsdf_layout; with n > 0 a NULL d_depth, d_offsets, d_headers, d_grid or d_out_tsdf, depth_len < 0,
 * n_src < 1, d_index == NULL with n_src != n, a d_out_tsdf or a non-NULL d_out_nearest that is not 16-byte aligned, a
 * focal, invalid_eps or trunc_voxels that is not > 0, or a batch whose n * ceil(R / slab) workgroups of 256 lanes do not
 * fit one launch (2^32 work-items).
 */
int tsdf_voxelize_grid_accurate_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets,
                                    const int32_t *d_headers, int64_t n_src, const int64_t *d_index, int n, int R,
                                    double focal, double cx, double cy, float invalid_eps, float trunc_voxels,
                                    int layout, void *hip_stream, const float *d_grid,
                                    float *d_out_tsdf, int32_t *d_out_nearest, int32_t *d_out_status);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_ACCURATE_H_ */
