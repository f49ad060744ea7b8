// tsdf_auggrid.hip — libtsdf_auggrid.so: the augmented voxelization on a caller-supplied grid and the augmented labels on
// their own (include/tsdf_auggrid.h).
//
// A translation unit and a library of its own, next to libtsdf_hip.so, libtsdf_augment.so and libtsdf_augstep.so (all
// frozen).  It takes the status codes, tsdf_cam and the layout enum from include/tsdf.h and the host preamble every library
// here has from device.inc, the device primitives from prim.inc and the slab scaffold it shares with tsdf_lowp.hip from
// slab.inc; nothing else of the product's .inc files is included, and there is no device global: every launch is
// self-contained.
//
// tsdf_aug_grid_kernel: n x ceil(R / slab) workgroups of 256 threads; a workgroup owns `slab` consecutive slices (indices
// of the slowest output axis) of one frame, so a batch of 16 frames at 32^3 is 256 workgroups.  It
//   1. checks the frame's header and grid row (both uniform); a frame that is not OK has its slab zero-filled and
//      workgroup 0 of the frame writes the status;
//   2. tabulates, per axis and grid index, the three products of the inverse map with the voxel centre's coordinate (the z
//      axis with b' added: the contract groups T^-1 as (A'_i0 x + A'_i1 y) + (A'_i2 z + b'_i), both brackets depend on grid
//      indices only) and v' - b of the distance terms: 3 x R entries of 32 bytes in LDS (3 KiB at R = 32);
//   3. walks its slab in items of 4 consecutive voxels of the fastest axis, one item per lane and pass: two additions
//      per row of the map, the IEEE division, the unfused pixel index, a plain global load of the gathered pixel (a crop
//      is at most 300 KB and is re-read by every slab of the frame: it is expected to be served by L2), the distance
//      terms, and three 16-byte stores, one per channel (items are numbered in output order, so a wave writes one
//      contiguous KiB per channel).
// No LDS staging of the crop, no work queue, no communication between workgroups, no atomics.
// Arithmetic contract: include/tsdf_auggrid.h (== oracle/tsdf_oracle.c::tsdf_oracle_voxels_aug); compiled with
// -ffp-contract=off, fma only where __builtin_fma is written.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_auggrid.h"

namespace {

#include "device.inc"   // check_device, launched, misaligned: the host preamble of every library here
#include "prim.inc"     // kDefaultCam, trunc_i32, finite32, header_ok
#include "slab.inc"     // workgroup <-> slab, the frame's header and grid row, zero-fill, host sizing

typedef float grid_f4 __attribute__((ext_vector_type(4)));
typedef double grid_d4 __attribute__((ext_vector_type(4)));

struct AugGridArgs {
  const float *depth;
  int64_t depth_len;
  const int64_t *offsets;
  const int32_t *headers;
  int n, R;
  int slab;    // slices per workgroup
  int nslab;   // workgroups per frame
  double focal, cx, cy;
  float eps;
  const double *xforms;   // [n][24]
  const float *grid;      // [n][8]
  float *out;             // [n][3][R][R][R]
  int32_t *status;        // [n] or null
};

template <int LAYOUT>
__global__ __launch_bounds__(kSlabWG) void tsdf_aug_grid_kernel(AugGridArgs a) {
#pragma clang fp contract(off)
  // [axis][index] = {A'_0a v'_a, A'_1a v'_a, A'_2a v'_a, v'_a - b_a}; the z axis carries + b'_i in its first three
  __shared__ grid_d4 s_tab[3][kSlabMaxR];

  const int tid = threadIdx.x;
  const int R = a.R, R4 = R >> 2;
  const Slab blk = slab_of_block(a.nslab, a.slab, R);
  const int64_t i = blk.i;
  const int sb = blk.sb, se = blk.se;
  const int64_t R3 = (int64_t)R * R * R;
  float *__restrict__ out = a.out + i * 3 * R3;

  const int64_t depth_len = a.depth_len;
  const SlabFrame fr = slab_frame(depth_len, a.offsets, a.headers, a.grid, i, true);
  const int left = fr.left, top = fr.top, right = fr.right, bottom = fr.bottom;
  const int64_t bw = fr.bw;
  const float ox = fr.ox, oy = fr.oy, oz = fr.oz, vl = fr.vl, td = fr.td;
  if (blk.first() && tid == 0 && a.status) a.status[i] = fr.status;

  if (fr.status != TSDF_FRAME_OK) {   // (uniform)
    slab_zero_fill<grid_f4>(out, R, sb, (int64_t)(se - sb) * R * R4, tid);
    return;
  }

  const double *__restrict__ xf = a.xforms + 24 * i;
  for (int e = tid; e < 3 * R; e += kSlabWG) {
    const int ax = e / R, idx = e - ax * R;
    const float o = ax == 0 ? ox : ax == 1 ? oy : oz;
    const double prod = (double)idx * (double)vl;
    const double vp = (double)o + prod;                       // v'_a
    grid_d4 t;
    t.x = xf[12 + ax] * vp;                                   // A'_0a v'_a
    t.y = xf[16 + ax] * vp;
    t.z = xf[20 + ax] * vp;
    if (ax == 2) {                                            // (A'_i2 z' + b'_i)
      t.x = t.x + xf[15];
      t.y = t.y + xf[19];
      t.z = t.z + xf[23];
    }
    t.w = vp - xf[4 * ax + 3];                                // v'_a - b_a
    s_tab[ax][idx] = t;
  }

  // per-frame constants of the distance terms
  const double F = a.focal, cx = a.cx, cy = a.cy;
  const double iF = 1.0 / F, it = 1.0 / (double)td;
  const double p00 = xf[0] * iF, p10 = xf[4] * iF, p20 = xf[8] * iF;
  const double g00 = -p00, g10 = -p10, g20 = -p20;                           // g_i0 = -(A_i0 * iF)
  const double g01 = xf[1] * iF, g11 = xf[5] * iF, g21 = xf[9] * iF;         // g_i1 = A_i1 * iF
  const double a02 = xf[2], a12 = xf[6], a22 = xf[10];
  const float eps = a.eps;
  const float *__restrict__ d = a.depth + fr.off0;
  __syncthreads();

  const int nit = (se - sb) * R * R4;
  for (int item = tid; item < nit; item += kSlabWG) {
    const int f4 = (item % R4) * 4;
    const int t1 = item / R4;
    const int y = t1 % R, sl = sb + t1 / R;
    const grid_d4 ty = s_tab[1][y];
    const grid_d4 ts = s_tab[LAYOUT == 0 ? 2 : 0][sl];     // the slice's axis: z (czyx) or x (cxyz)
    grid_f4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0, o2 = o0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const grid_d4 tf = s_tab[LAYOUT == 0 ? 0 : 2][f4 + j];   // the lane's own axis
      const grid_d4 tx = LAYOUT == 0 ? tf : ts, tz = LAYOUT == 0 ? ts : tf;
      // v = T^-1(v') = (A'_i0 x' + A'_i1 y') + (A'_i2 z' + b'_i)
      const double s0 = tx.x + ty.x, s1 = tx.y + ty.y, s2 = tx.z + ty.z;
      const double vx = s0 + tz.x, vy = s1 + tz.y, vz = s2 + tz.z;
      const double q = -F / vz;
      const double mx = vx * q, my = (-vy) * q;
      const int px = trunc_i32(mx + cx), py = trunc_i32(my + cy);
      float v0 = 0.f, v1 = 0.f, v2 = 0.f;
      if (px >= left && px < right && py >= top && py < bottom) {
        const float pd = d[(int64_t)(py - top) * bw + (px - left)];
        if (__builtin_fabsf(pd) >= eps) {                     // NaN is invalid
          const double dxi = (double)px - cx, dyi = (double)py - cy, pd64 = (double)pd;
          const double c0 = __builtin_fma(g00, dxi, __builtin_fma(g01, dyi, a02));
          const double c1 = __builtin_fma(g10, dxi, __builtin_fma(g11, dyi, a12));
          const double c2 = __builtin_fma(g20, dxi, __builtin_fma(g21, dyi, a22));
          const double u0 = __builtin_fma(pd64, c0, tx.w);    // v'_i - w'_i, mm
          const double u1 = __builtin_fma(pd64, c1, ty.w);
          const double u2 = __builtin_fma(pd64, c2, tz.w);
          const double t0 = u0 * it, t1v = u1 * it, t2 = u2 * it;
          const double xx = t0 * t0;
          const double sq = __builtin_fma(t2, t2, __builtin_fma(t1v, t1v, xx));
          const bool nearv = sq <= 1.0;
          double m0 = __builtin_fabs(t0), m1 = __builtin_fabs(t1v), m2 = __builtin_fabs(t2);
          if (!(m0 < 1.0)) m0 = 1.0;                          // min(|t|, 1); a NaN distance counts as far
          if (!(m1 < 1.0)) m1 = 1.0;
          if (!(m2 < 1.0)) m2 = 1.0;
          if (!nearv) m0 = m1 = m2 = 1.0;
          if (u2 < 0.0) {
            m0 = -m0;
            m1 = -m1;
            m2 = -m2;
          }
          v0 = (float)m0;
          v1 = (float)m1;
          v2 = (float)m2;
        }
      }
      o0[j] = v0;
      o1[j] = v1;
      o2[j] = v2;
    }
    const int64_t e = ((int64_t)sl * R + y) * R + f4;   // o[c][slow][y][fast]
    *reinterpret_cast<grid_f4 *>(out + e) = o0;
    *reinterpret_cast<grid_f4 *>(out + R3 + e) = o1;
    *reinterpret_cast<grid_f4 *>(out + 2 * R3 + e) = o2;
  }
}

struct JointArgs {
  const float *gt;        // [n][J][3]
  const double *xforms;   // [n][24]
  int64_t total;          // n * J
  int J;
  float *out;
};

// one lane per coordinate triple: T(joint) with the frame's forward rows, a fused chain in float64 (affine3_fwd)
__global__ __launch_bounds__(kSlabWG) void tsdf_transform_joints_kernel(JointArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kSlabWG + threadIdx.x;
  if (t >= a.total) return;
  const int64_t i = t / a.J;
  const double *__restrict__ m = a.xforms + 24 * i;
  const float *__restrict__ g = a.gt + 3 * t;
  const double x = (double)g[0], y = (double)g[1], z = (double)g[2];
  float *__restrict__ o = a.out + 3 * t;
#pragma unroll
  for (int r = 0; r < 3; ++r)
    o[r] = (float)__builtin_fma(m[4 * r], x, __builtin_fma(m[4 * r + 1], y, __builtin_fma(m[4 * r + 2], z, m[4 * r + 3])));
}

}  // namespace

extern "C" {

int tsdf_auggrid_version(void) { return TSDF_AUGGRID_VERSION; }

int tsdf_voxelize_aug_grid_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                               int n, int R, const tsdf_cam *cam, int layout, void *hip_stream, const double *d_xforms,
                               const float *d_grid, float *d_out_tsdf, int32_t *d_out_status) {
  // arguments first, then the device, then the launch
  if (n < 0) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_depth || !d_offsets || !d_headers || !d_xforms || !d_grid || !d_out_tsdf || depth_len < 0) return TSDF_ERR_INVALID_ARG;
  if (slab_bad_shape(R, layout)) return TSDF_ERR_INVALID_ARG;
  if (misaligned(d_xforms, 7) || misaligned(d_out_tsdf, 15)) return TSDF_ERR_INVALID_ARG;
  if (!cam_ok(cam)) return TSDF_ERR_INVALID_ARG;
  SlabPlan plan;
  if (!slab_plan(n, R, 4, plan)) return TSDF_ERR_INVALID_ARG;   // a launch holds fewer than 2^32 work-items
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  if (!cam) cam = &kDefaultCam;
  AugGridArgs a;
  a.depth = d_depth;
  a.depth_len = depth_len;
  a.offsets = d_offsets;
  a.headers = d_headers;
  a.n = n;
  a.R = R;
  a.slab = plan.slab;
  a.nslab = plan.nslab;
  a.focal = cam->focal;
  a.cx = cam->cx;
  a.cy = cam->cy;
  a.eps = cam->invalid_eps;
  a.xforms = d_xforms;
  a.grid = d_grid;
  a.out = d_out_tsdf;
  a.status = d_out_status;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  if (layout == TSDF_LAYOUT_CZYX)
    hipLaunchKernelGGL(tsdf_aug_grid_kernel<0>, dim3((unsigned)plan.blocks), dim3(kSlabWG), 0, s, a);
  else
    hipLaunchKernelGGL(tsdf_aug_grid_kernel<1>, dim3((unsigned)plan.blocks), dim3(kSlabWG), 0, s, a);
  return launched();
}

int tsdf_transform_joints_hip(const float *d_gt, const double *d_xforms, int n, int n_joints, void *hip_stream,
                              float *d_out_gt_aug) {
  if (n < 0) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_gt || !d_xforms || !d_out_gt_aug || n_joints < 1 || n_joints > 170) return TSDF_ERR_INVALID_ARG;
  if (misaligned(d_xforms, 7)) return TSDF_ERR_INVALID_ARG;
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  JointArgs a;
  a.gt = d_gt;
  a.xforms = d_xforms;
  a.total = (int64_t)n * n_joints;
  a.J = n_joints;
  a.out = d_out_gt_aug;
  const int64_t blocks = (a.total + kSlabWG - 1) / kSlabWG;
  if (blocks * kSlabWG > 0xffffffffll) return TSDF_ERR_INVALID_ARG;
  hipLaunchKernelGGL(tsdf_transform_joints_kernel, dim3((unsigned)blocks), dim3(kSlabWG), 0,
                     static_cast<hipStream_t>(hip_stream), a);
  return launched();
}

}  // extern "C"
