/*
 * tsdf_group.h — C ABI of libtsdf_group.so: what a point network (HandPointNet, Point-to-Point Regression PointNet and
 * their family) reads next to its sampled cloud — for every centre of a set-abstraction level its K nearest neighbours
 * in the cloud (kNN grouping), and for every point a surface normal by PCA over its nearest neighbours.
 *
 * One more library next to libtsdf_hip.so (include/tsdf.h, v7, frozen), the eleven of csrc/Makefile's EXTS line,
 * libtsdf_heatmap.so, libtsdf_heatloss.so, libtsdf_occupancy.so and libtsdf_fps.so (all v1, frozen): its own
 * translation unit (csrc/tsdf_group.hip), its own binary and its own version number.  It shares the status codes of
 * tsdf.h and nothing else.  Conventions, those of tsdf_fps.h:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - a call is asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronises;
 *   - it allocates nothing, uses no global atomics and no device-side state, never prints, has no CPU fallback and may
 *     be captured into a hipGraph (a captured launch is self-contained);
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.  Arguments are checked first, then the device
 *     (TSDF_ERR_NO_DEVICE unless the current device is a gfx950), then the kernel is launched.
 */
#ifndef TSDF_GROUP_H_
#define TSDF_GROUP_H_

#include <stdint.h>

#include "tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_GROUP_VERSION 1

#define TSDF_GROUP_MAX_CLOUD 12288   /* P is in 1..TSDF_GROUP_MAX_CLOUD: the resident cap of tsdf_fps.h's sampler */
#define TSDF_GROUP_MAX_K 128         /* K is in 1..TSDF_GROUP_MAX_K */
#define TSDF_GROUP_SWEEPS 8          /* the FIXED number of Jacobi sweeps of tsdf_normals_hip */

/* 1 */
int tsdf_group_version(void);

/*
 * CANDIDATES AND QUERIES, the same for both entries.
 *   d_points     float32[n][pitch][3], 4-byte aligned: the cloud of batch position i is the first P rows of its `pitch`
 *                rows, P in 1..TSDF_GROUP_MAX_CLOUD, pitch >= P.  (pitch == P is a dense [n][P][3]; pitch > P reads the
 *                prefix of a larger cloud in place — with tsdf_fps.h's "the first k rows of an M-point result are the
 *                k-point result", the cloud of the next set-abstraction level.)
 *                A row is a CANDIDATE iff its three coordinates are finite; its RANK is its row number.  A ragged cloud
 *                padded with NaN rows therefore needs no count.  m is the number of candidates.
 *   d_query      float32[n][C][3] or NULL, C >= 1.  With NULL the queries are rows 0..C-1 of the position's cloud
 *                itself, which requires C <= P: the FPS prefix, no separate centre tensor.
 *   K            neighbours per query, 1..TSDF_GROUP_MAX_K
 *   d_status_in  int32[n] or NULL.  A position with a non-zero input status is not read: its status is copied through
 *                and all its rows are "no result" rows (below).  tsdf_fps.h's d_out_status chains.
 *
 * THE RULE.  All arithmetic is float32, every operation rounded on its own, no fma.  For query q and candidate p
 *     dx = p.x - q.x,  dy = p.y - q.y,  dz = p.z - q.z,  dist = (dx*dx + dy*dy) + dz*dz
 * which is tsdf_fps.h's expression.  For finite p and q dist is in [+0, +inf] and never a NaN (the argument is in
 * tsdf_fps.h), so its bit pattern orders as an unsigned integer.  The KEY of a candidate is (dist bits) << 32 | rank.
 * The neighbours of q are the K smallest keys in ascending key order: nearest first, ties to the LOWEST rank, +inf
 * distances included.  With m < K, slots m..K-1 repeat slot 0, index and distance (and offset): a gather through the
 * result is always valid.
 * With d_query == NULL a query is a candidate of its own cloud: its slot 0 is itself at +0, or a duplicate of it of
 * lower rank.
 * A query with a non-finite coordinate gives a "NO RESULT" row: index -1, dist2 +0, offsets +0 (normal +0, curvature
 * +0); the position's status stays 0.  m == 0 gives the position TSDF_FRAME_DEGENERATE (1) and all its rows are "no
 * result" rows.  Otherwise d_out_status int32[n] is d_status_in's value, or TSDF_FRAME_OK (0).
 * Every byte of every given output is written by the launch.
 */

/*
 * The plan, host code only: one workgroup of 256 lanes holds its position's cloud in *lds_bytes of (dynamic) LDS and
 * answers *queries_per_group queries, so a position takes *groups_per_position = ceil(C / *queries_per_group)
 * workgroups.  TSDF_ERR_INVALID_ARG for P outside 1..TSDF_GROUP_MAX_CLOUD, C < 1, K outside 1..TSDF_GROUP_MAX_K or a
 * NULL result pointer.
 */
int tsdf_group_plan(int P, int C, int K, int *lds_bytes, int *queries_per_group, int *groups_per_position);

/*
 * kNN GROUPING.
 *   d_out_index   int32[n][C][K]       the neighbours' ranks
 *   d_out_dist2   float32[n][C][K] or NULL: their dist
 *   d_out_offset  float32[n][C][K][3] or NULL: the very dx, dy, dz of each neighbour — what a set-abstraction layer reads
 *   d_out_status  int32[n]
 *
 * TSDF_ERR_INVALID_ARG, checked in this order before the device is looked at: n < 0; P outside 1..12288; C < 1; K
 * outside 1..128; pitch < P; (n == 0 returns TSDF_OK here;) a NULL d_points, d_out_index or d_out_status; d_query NULL
 * with C > P; a d_points, d_query, d_out_dist2 or d_out_offset that is not 4-byte aligned; a batch whose
 * n * ceil(C / queries_per_group) workgroups do not fit one launch (2^32 work-items or more).
 */
int tsdf_knn_hip(const float *d_points, int64_t pitch, const float *d_query, const int32_t *d_status_in, int n, int P,
                 int C, int K, void *hip_stream, int32_t *d_out_index, float *d_out_dist2, float *d_out_offset,
                 int32_t *d_out_status);

/*
 * SURFACE NORMALS by PCA over the neighbours.  The neighbour set of a query is tsdf_knn_hip's: m' = min(K, m) distinct
 * slots, in slot order.  Everything below is float64, one rounding per operation, no fma.
 *   slot j's value lives in lane j % 64.  A lane adds its slot j and its slot j + 64; a slot >= m' contributes +0.0.
 *   Then six butterfly steps, v = v + v[lane ^ s] for s = 1, 2, 4, 8, 16, 32.  Addition commutes, so every lane ends
 *   with the same bits: the TREE SUM.
 *     S      = the three tree sums of the neighbours' coordinates, each widened to double
 *     mean   = S / m'
 *     e      = p - mean                                            per neighbour
 *     cov_ab = (the tree sum of e_a * e_b) / m'                    ab in xx, xy, xz, yy, yz, zz
 *   The eigenvectors by cyclic Jacobi on cov with V = I: TSDF_GROUP_SWEEPS (8) sweeps, a FIXED count, each the pairs
 *   (0,1), (0,2), (1,2) in this order; a rotation whose off-diagonal element a_pq is exactly 0 is skipped, else
 *     theta = (a_qq - a_pp) / (2 * a_pq),  t = 1 / (|theta| + sqrt(theta*theta + 1)), negated if theta < 0,
 *     c = 1 / sqrt(t*t + 1),  s = t * c,  a_pp -= t * a_pq,  a_qq += t * a_pq,  a_pq = 0,
 *     (a_rp, a_rq) = (c*a_rp - s*a_rq, s*a_rp + c*a_rq),  and the same for each row of (V_p, V_q).
 *   The normal n is the column of V of the smallest diagonal element, ties to the lowest column.
 *   Orientation: w = view - q (q widened; view is d_view's row, or the origin), d = (n_x*w_x + n_y*w_y) + n_z*w_z, and
 *   n is negated iff d < 0.
 *   Curvature: l0 / ((l0 + l1) + l2) with the diagonal ascending, and 0 when that sum is 0.
 *   Normal and curvature are rounded ONCE to float32.  m' < 3 gives a zero normal and zero curvature (+0).
 *
 *   d_view           float64[n][3] or NULL, 8-byte aligned: the viewpoint of each batch position
 *   d_out_normals    float32[n][C][3]
 *   d_out_curvature  float32[n][C] or NULL
 *   d_out_status     int32[n]
 *
 * TSDF_ERR_INVALID_ARG, in this order: n < 0; P outside 1..12288; C < 1; K outside 1..128; pitch < P; (n == 0 returns
 * TSDF_OK here;) a NULL d_points, d_out_normals or d_out_status; d_query NULL with C > P; a d_points, d_query or
 * d_out_curvature that is not 4-byte aligned or a d_view that is not 8-byte aligned; too many workgroups for one launch.
 */
int tsdf_normals_hip(const float *d_points, int64_t pitch, const float *d_query, const int32_t *d_status_in,
                     const double *d_view, int n, int P, int C, int K, void *hip_stream, float *d_out_normals,
                     float *d_out_curvature, int32_t *d_out_status);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_GROUP_H_ */
