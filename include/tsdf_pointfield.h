/*
 * tsdf_pointfield.h — C ABI of libtsdf_pointfield.so: the label side of a point-wise regression network (Point-to-Point
 * Regression PointNet, Ge, Ren, Yuan, ECCV 2018) and the way back.  For every point of a sampled cloud and every joint
 * the network predicts a heat value and a unit vector towards the joint; ENCODE writes that offset field from the joints,
 * DECODE recovers each joint from a (predicted) field by a weighted vote of the points of greatest heat.
 *
 * One more library next to libtsdf_hip.so (include/tsdf.h, v7, frozen), the eleven of csrc/Makefile's EXTS line,
 * libtsdf_heatmap.so, libtsdf_heatloss.so, libtsdf_occupancy.so, libtsdf_fps.so and libtsdf_group.so (all v1, frozen):
 * its own translation unit (csrc/tsdf_pointfield.hip), its own binary and its own version number.  It shares the status
 * codes of tsdf.h, the cloud rules of tsdf_group.h and the dtype codes of tsdf_heatmap.h, and nothing else.
 * Conventions, those of tsdf_group.h:
 *   - every pointer named d_* is device-accessible memory (device memory, or page-locked host memory);
 *   - a call is asynchronous on `hip_stream` (a hipStream_t; NULL is the default stream) and never synchronises;
 *   - it allocates nothing, uses no global atomics and no device-side state, never prints, has no CPU fallback and may
 *     be captured into a hipGraph (a captured launch is self-contained);
 *   - the return value is TSDF_OK (0) or a negative tsdf_status.  Arguments are checked first, then the device
 *     (TSDF_ERR_NO_DEVICE unless the current device is a gfx950), then the kernel is launched.
 */
#ifndef TSDF_POINTFIELD_H_
#define TSDF_POINTFIELD_H_

#include <stdint.h>

#include "tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_POINTFIELD_VERSION 1

#define TSDF_POINTFIELD_MAX_CLOUD 12288    /* P is in 1..TSDF_POINTFIELD_MAX_CLOUD: TSDF_GROUP_MAX_CLOUD */
#define TSDF_POINTFIELD_MAX_K 12288        /* ENCODE: K is in 1..TSDF_POINTFIELD_MAX_K */
#define TSDF_POINTFIELD_MAX_VOTES 128      /* DECODE: M is in 1..TSDF_POINTFIELD_MAX_VOTES */
#define TSDF_POINTFIELD_MAX_JOINTS 65536   /* J is in 1..TSDF_POINTFIELD_MAX_JOINTS */

#define TSDF_POINTFIELD_CP 0   /* layout "cp": [n][4J][P], what a Conv1d head emits */
#define TSDF_POINTFIELD_PC 1   /* layout "pc": [n][P][4J] */

#define TSDF_POINTFIELD_F32 0    /* dtype: the codes of tsdf_heatmap.h / tsdf_lowp.h */
#define TSDF_POINTFIELD_F16 1
#define TSDF_POINTFIELD_BF16 2

/* 1 */
int tsdf_pointfield_version(void);

/*
 * INPUTS OF BOTH ENTRIES.
 *   d_points     float32[n][pitch][3], 4-byte aligned: the cloud of batch position i is the first P rows of its `pitch`
 *                rows, P in 1..TSDF_POINTFIELD_MAX_CLOUD, pitch >= P — exactly tsdf_group.h's cloud.  A row is a
 *                CANDIDATE iff its three coordinates are finite; its RANK is its row number; m is the number of
 *                candidates of the position.
 *   d_status_in  int32[n] or NULL.  A position with a non-zero input status is not read: its status is copied through
 *                and all its outputs are zero (+0).  tsdf_fps.h's d_out_status chains.
 *   radius       a double, finite and > 0, in the cloud's units: the ball about a joint.
 *   layout       TSDF_POINTFIELD_CP: the field is [n][4J][P];  TSDF_POINTFIELD_PC: [n][P][4J].
 *                Channel j (0 <= j < J) is joint j's heat; channel J + 3j + a is component a of its vector.
 *   dtype        the field's element type: float32, float16 or bfloat16.  A 2-byte value is the float32 value narrowed
 *                by round-to-nearest-even (float16 with subnormals); a 2-byte value read is widened exactly.
 * d_out_status int32[n] is the input status, else TSDF_FRAME_DEGENERATE (1) when m == 0, else TSDF_FRAME_OK (0).
 * Every byte of every given output is written by the launch.
 */

/*
 * The plan, host code only: one workgroup of 256 lanes holds its position's cloud in *lds_bytes of (dynamic) LDS and
 * serves *joints_per_group joints, one wave a joint at a time, so a position takes *groups_per_position =
 * ceil(J / *joints_per_group) workgroups.  K is ENCODE's K, or DECODE's M.  TSDF_ERR_INVALID_ARG for P outside
 * 1..TSDF_POINTFIELD_MAX_CLOUD, J outside 1..TSDF_POINTFIELD_MAX_JOINTS, K outside 1..TSDF_POINTFIELD_MAX_K or a NULL
 * result pointer.
 */
int tsdf_pointfield_plan(int P, int J, int K, int *lds_bytes, int *joints_per_group, int *groups_per_position);

/*
 * ENCODE.  d_joints float32[n][J][3], 4-byte aligned.  For joint q and candidate p of rank i:
 *   1. float32, every operation rounded on its own, no fma:
 *          dx = q.x - p.x,  dy = q.y - p.y,  dz = q.z - p.z      (the point-to-joint direction)
 *          dist2 = (dx*dx + dy*dy) + dz*dz
 *      Negation is exact, so dist2 is bit for bit the dist2 of tsdf_knn_hip with d_query = d_joints.  For finite p and q
 *      it is in [+0, +inf] and never a NaN.  The KEY of the candidate is (dist2 bits) << 32 | i.
 *   2. p is a MEMBER of q iff
 *        - its key is among the min(K, m) smallest keys of the joint (ties to the LOWEST rank; K >= m is the pure ball
 *          rule), and
 *        - d <= radius, where d = sqrt((double)dist2) (float64, IEEE).  An infinite dist2 is never a member.
 *   3. For a member, in float64:  heat = 1 - d / radius;  vec_a = (double)d_a / d, and +0 when dist2 == 0.  Each is
 *      rounded ONCE to float32 (then narrowed for a 2-byte dtype).  A point on the joint has heat 1 and a zero vector; a
 *      point at d == radius has heat +0 and a unit vector.
 *   4. Every other (point, joint) cell is +0 in all four channels: non-members, non-candidate rows, invalid joints.
 *   5. d_out_valid int32[n][J]: 1 iff the joint's three coordinates are finite, the position's status is 0 and m > 0.
 *   6. m == 0 gives the position TSDF_FRAME_DEGENERATE.
 *
 * TSDF_ERR_INVALID_ARG, checked in this order before the device is looked at: n < 0; P outside 1..12288; J outside
 * 1..65536; K outside 1..12288; pitch < P; a radius that is not finite or not > 0; a layout that is not 0 or 1; a dtype
 * that is not 0, 1 or 2; (n == 0 returns TSDF_OK here;) a NULL d_points, d_joints, d_out_field, d_out_valid or
 * d_out_status; a d_points or d_joints that is not 4-byte aligned, or a d_out_field that is not aligned to its element;
 * a batch whose n * ceil(J / joints_per_group) workgroups do not fit one launch (2^32 work-items or more).
 */
int tsdf_pointfield_encode_hip(const float *d_points, int64_t pitch, const float *d_joints, const int32_t *d_status_in,
                               int n, int P, int J, int K, double radius, int layout, int dtype, void *hip_stream,
                               void *d_out_field, int32_t *d_out_valid, int32_t *d_out_status);

/*
 * DECODE.  d_field is a field in `layout` and `dtype`, usually a network's prediction; every value is widened exactly
 * to float32.  Per joint:
 *   1. The min(M, m) candidates of GREATEST heat are selected, ties to the LOWEST rank.  A NaN heat never wins over a
 *      number (it orders below -inf), but is selected when numbers run out.  Heats are compared by the order-preserving
 *      integer image of their bits, so -0 orders below +0 (both vote with weight 0).
 *   2. Per selected candidate, in float64, every operation rounded on its own, no fma:
 *          w  = min(max(h, 0), 1), and 0 for a NaN heat
 *          nv = sqrt((vx*vx + vy*vy) + vz*vz)
 *          u_a = v_a / nv, and 0 when nv is 0 or not finite
 *          e_a = p_a + (radius * (1 - w)) * u_a
 *   3. W = sum of w and S_a = sum of w * e_a, each as the TREE SUM of tsdf_group.h: the candidate of compact index c
 *      (its number among the candidates, in rank order) belongs to lane c % 64; a lane adds its selected candidates in
 *      ascending c, starting from +0.0; then six butterfly additions v + v[lane ^ s], s = 1, 2, 4, 8, 16, 32.
 *   4. joint_a = S_a / W and weight = W, each rounded ONCE to float32.
 *   5. W == 0, m == 0 or a position with a status: a zero row and weight +0.
 *   d_out_joints float32[n][J][3];  d_out_weight float32[n][J].
 *
 * TSDF_ERR_INVALID_ARG, in this order: n < 0; P outside 1..12288; J outside 1..65536; M outside 1..128; pitch < P; a
 * radius that is not finite or not > 0; a bad layout; a bad dtype; (n == 0 returns TSDF_OK here;) a NULL d_points,
 * d_field, d_out_joints, d_out_weight or d_out_status; a d_points, d_out_joints or d_out_weight that is not 4-byte
 * aligned or a d_field that is not aligned to its element; too many workgroups for one launch.
 */
int tsdf_pointfield_decode_hip(const float *d_points, int64_t pitch, const void *d_field, const int32_t *d_status_in,
                               int n, int P, int J, int M, double radius, int layout, int dtype, void *hip_stream,
                               float *d_out_joints, float *d_out_weight, int32_t *d_out_status);

#ifdef __cplusplus
}
#endif

#endif /* TSDF_POINTFIELD_H_ */
