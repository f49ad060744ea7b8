/*
 * tsdf_mapstep.h — C ABI of libtsdf_mapstep.so: two per-frame maps composed into one, and the augmented step's whole head
 * — draw, compose, grid placement, labels — as ONE launch.
 *
 * One more extension library next to libtsdf_hip.so (include/tsdf.h, v7, frozen) and libtsdf_augment.so,
 * libtsdf_augstep.so, libtsdf_auggrid.so, libtsdf_depth16.so, libtsdf_obb.so, libtsdf_lowp.so, libtsdf_maplowp.so (all
 * v1, frozen): its own translation unit (csrc/tsdf_mapstep.hip), its own binary and its own version number.  It shares
 * the status codes of tsdf.h and nothing else.  Conventions:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - the calls are asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronise;
 *   - they allocate nothing, use no atomics and no device-side state, never print, have no CPU fallback, are
 *     deterministic and may be captured into a hipGraph (a captured launch is self-contained);
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.  Arguments are checked first, then the device
 *     (TSDF_ERR_NO_DEVICE unless the current device is a gfx950), then the kernel is launched.
 *
 * What it is for: a frame is voxelized under ONE map.  The principal-axis map of include/tsdf_obb.h removes the hand's
 * in-plane pose, the augmentation of include/tsdf_augstep.h perturbs a pose; training wants the second about the first.
 * tsdf_compose_xforms_hip makes one map of two.  tsdf_map_step_head_hip is everything the augmented step does before
 * its voxel pass — tsdf_aug_draw_at_hip, the composition, tsdf_map_place_hip, tsdf_transform_joints_hip on the batch's
 * joints, tsdf_normalize_joints_hip — in one launch instead of five or six dependent ones, bit for bit.
 */
#ifndef TSDF_MAPSTEP_H_
#define TSDF_MAPSTEP_H_

#include <stdint.h>

#include "tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_MAPSTEP_VERSION 1

/* 1 */
int tsdf_mapstep_version(void);

/*
 * out[i] = outer[i] o inner[g], g = d_index ? d_index[i] : i: the map that applies inner[g] first and outer[i] second.
 *
 *   d_outer   float64[n][24], 8-byte aligned        }  the layout of tsdf_voxelize_aug_hip (include/tsdf.h): the forward
 *   d_inner   float64[n_inner][24], 8-byte aligned  }  rows {A_i0, A_i1, A_i2, b_i}, i = 0..2, then the inverse rows
 *   n_inner   number of inner maps
 *   d_index   int64[n] or NULL.  With NULL, n_inner must equal n.  A g outside [0, n_inner) reads nothing of d_inner and
 *             gives out[i] = outer[i], every bit of it: inner is then the identity
 *   n         number of maps written; 0 is a no-op (TSDF_OK)
 *   d_out     float64[n][24], 8-byte aligned.  It may be d_outer (a lane reads its row before it writes it)
 *
 * Arithmetic: float64, every product and every sum rounded on its own, no fma.  With P and Q two sets of 3 x 4 rows,
 * (A_ij | b_i) the rows of the result:
 *     A_ij = (P_i0 Q_0j + P_i1 Q_1j) + P_i2 Q_2j
 *     b_i  = ((P_i0 q_0 + P_i1 q_1) + P_i2 q_2) + p_i
 * forward half: P = outer's forward rows, Q = inner's forward rows; inverse half: P = inner's INVERSE rows, Q = outer's
 * inverse rows (the inverse of a composition is the inverses composed the other way round; no 3 x 3 is inverted).
 *
 * TSDF_ERR_INVALID_ARG, before the device is looked at: n < 0; with n > 0 a NULL d_outer, d_inner or d_out, n_inner < 1,
 * d_index == NULL with n_inner != n, or a d_outer, d_inner or d_out that is not 8-byte aligned.
 */
int tsdf_compose_xforms_hip(const double *d_outer, const double *d_inner, int64_t n_inner, const int64_t *d_index, int n,
                            void *hip_stream, double *d_out);

/*
 * The head of the augmented step: per batch position, everything before the voxel pass, in one launch.
 *
 *   d_depth, depth_len, d_offsets, d_headers, n_src, d_index, n, R
 *                as for tsdf_map_place_hip (include/tsdf_maplowp.h): the SOURCE tables and the batch drawn from them
 *   focal, cx, cy, invalid_eps, trunc_voxels
 *                the camera constants BY VALUE — the five fields of the camera struct of tsdf.h in its order; there is no
 *                default here (the MSRA constants are 241.42, 160, 120, 1, 3).  They are put through the one camera rule of
 *                every entry: focal, invalid_eps and trunc_voxels must each be > 0 (a NaN is not), whether or not
 *                d_out_grid is given
 *   d_centres    float32[n_src][3]: the centre each source frame's augmentation turns about, as for tsdf_aug_draw_at_hip
 *   d_base       float64[n_src][24], 8-byte aligned, or NULL: one base map per SOURCE FRAME (tsdf_obb_xforms_hip's, say)
 *   d_state      uint64[2], 8-byte aligned: {key, counter0}, read BY THE KERNEL when it runs (include/tsdf_augstep.h)
 *   d_counters   int64[n] or NULL, as for tsdf_aug_draw_at_hip
 *   d_gt         float32[n_src][3 * n_joints] or NULL: the joints of every SOURCE frame
 *   n_joints     1..170 with d_gt, otherwise unused;  clamp: as for tsdf_normalize_joints_hip
 *   d_out_xforms float64[n][24], 8-byte aligned, required: the map T of every batch position
 *   d_out_grid   float32[n][8] or NULL.  With NULL the crop is NOT read — d_depth, d_offsets and d_headers may be NULL —
 *                and the launch is the draw and the composition alone
 *   d_out_max_l float32[n], d_out_mid_p float32[n][3], d_out_status int32[n]: each may be NULL; they need d_out_grid
 *   d_out_gt_aug float32[n][3 * n_joints] or NULL, d_out_gt_nor float32[n][3 * n_joints]: with d_gt, which needs
 *                d_out_grid and d_out_gt_nor
 *   d_out_stretch float64[n] or NULL, d_out_rot int32[n][2] or NULL: the draws, as for tsdf_aug_draw_at_hip
 *
 * Contract: every output equals, bit for bit, what this chain of existing entries writes (their headers state the
 * arithmetic; it is not restated here):
 *     U = tsdf_aug_draw_at_hip(d_centres, n_src, d_index, n, d_state, d_counters) -> U, stretch, rot
 *                                                                            (include/tsdf_augstep.h, tsdf_augment.h)
 *     T = d_base ? tsdf_compose_xforms_hip(U, d_base, n_src, d_index, n) : U   -> d_out_xforms            (above)
 *     tsdf_map_place_hip(..., d_index, n, R, the camera, d_xforms = T)   -> d_out_grid, max_l, mid_p, status
 *                                                                            (include/tsdf_maplowp.h)
 *     tsdf_transform_joints_hip(joints of source frame min(max(g, 0), n_src - 1), T)   -> d_out_gt_aug
 *                                                                            (include/tsdf_auggrid.h)
 *     tsdf_normalize_joints_hip(gt_aug, max_l, mid_p, clamp)   -> d_out_gt_nor   (include/tsdf.h)
 * including what the chain does with an index outside [0, n_src) (the identity map, a NaN stretch, status 2, labels
 * 0.5), a bad header, a frame without a valid pixel, a degenerate extent and a map that holds a NaN.
 *
 * TSDF_ERR_INVALID_ARG, before the device is looked at: n < 0; an R that is not a multiple of 4 in 4..128; with n > 0 a
 * NULL d_centres, d_state or d_out_xforms, n_src < 1, d_index == NULL with n_src != n, a d_out_xforms, d_state or d_base
 * that is not 8-byte aligned, camera constants that the camera rule refuses; with d_out_grid a NULL d_depth, d_offsets
 * or d_headers or depth_len < 0; without d_out_grid a d_out_max_l, d_out_mid_p, d_out_status or d_gt; with d_gt a NULL
 * d_out_gt_nor or n_joints outside 1..170; without d_gt a d_out_gt_aug or d_out_gt_nor.
 */
int tsdf_map_step_head_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                           int64_t n_src, const int64_t *d_index, int n, int R, double focal, double cx, double cy,
                           float invalid_eps, float trunc_voxels, const float *d_centres, const double *d_base, const uint64_t *d_state,
                           const int64_t *d_counters, const float *d_gt, int n_joints, int clamp, void *hip_stream,
                           double *d_out_xforms, float *d_out_grid, float *d_out_max_l, float *d_out_mid_p,
                           int32_t *d_out_status, float *d_out_gt_aug, float *d_out_gt_nor, double *d_out_stretch,
                           int32_t *d_out_rot);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_MAPSTEP_H_ */
