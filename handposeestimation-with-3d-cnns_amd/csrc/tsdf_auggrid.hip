// tsdf_auggrid.hip — libtsdf_auggrid.so: the augmented voxelization on a caller-supplied grid and the augmented labels on
// their own (include/tsdf_auggrid.h).
//
// A translation unit and a library of its own, next to libtsdf_hip.so, libtsdf_augment.so and libtsdf_augstep.so (all
// frozen).  It takes the status codes, tsdf_cam and the layout enum from include/tsdf.h and the host preamble every library
// here has from device.inc, the device primitives from prim.inc, the slab scaffold it shares with tsdf_lowp.hip,
// tsdf_maplowp.hip and tsdf_accurate.hip from slab.inc and the voxel arithmetic under a map — the per-axis table, the
// per-frame constants, the four-voxel chain — from mapvox.inc, which it shares with tsdf_maplowp.hip; nothing else of the
// product's .inc files is included, and there is no device global: every launch is self-contained.
//
// tsdf_aug_grid_kernel: n x ceil(R / slab) workgroups of 256 threads; a workgroup owns `slab` consecutive slices (indices
// of the slowest output axis) of one frame, so a batch of 16 frames at 32^3 is 256 workgroups.  It
//   1. checks the frame's header and grid row (both uniform; slab.inc, with no index: the ABI has none); a frame that is
//      not OK has its slab zero-filled and workgroup 0 of the frame writes the status;
//   2. tabulates, per axis and grid index, the three products of the inverse map with the voxel centre's coordinate and
//      v' - b of the distance terms (mapvox.inc::map_fill_tab): 3 x R entries of 32 bytes in LDS (3 KiB at R = 32);
//   3. walks its slab in items of 4 consecutive voxels of the fastest axis, one item per lane and pass
//      (mapvox.inc::map_quad): two additions per row of the map, the IEEE division, the unfused pixel index and a plain
//      global load of the gathered pixel for each of the four (always in bounds: a rejected voxel reads the crop's first
//      pixel; a crop is at most 300 KB and is re-read by every slab of the frame: it is expected to be served by L2), then
//      the distance terms, and three 16-byte stores, one per channel (items are numbered in output order, so a wave writes
//      one contiguous KiB per channel).
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
#include "mapvox.inc"   // map_fill_tab, map_consts, map_quad: the mapped voxel arithmetic, shared with tsdf_maplowp.hip

typedef float grid_f4 __attribute__((ext_vector_type(4)));

struct AugGridArgs {
  SlabSrc src;            // no index in this ABI: index null, n_src = n
  float eps;
  const double *xforms;   // [n][24]
  const float *grid;      // [n][8]
  float *out;             // [n][3][R][R][R]
  int32_t *status;        // [n] or null
};

template <int LAYOUT>
__global__ __launch_bounds__(kSlabWG) void tsdf_aug_grid_kernel(AugGridArgs a) {
#pragma clang fp contract(off)
  __shared__ map_d4 s_tab[3][kSlabMaxR];

  const int tid = threadIdx.x;
  const int R = a.src.R, R4 = R >> 2;
  const Slab blk = slab_of_block(a.src.nslab, a.src.slab, R);
  const int sb = blk.sb, se = blk.se;
  const int64_t R3 = (int64_t)R * R * R;
  float *__restrict__ out = a.out + blk.i * 3 * R3;

  const SlabFrame fr = slab_head<true>(a.src, blk, a.grid);
  if (slab_bad_frame<grid_f4>(fr, blk, a.status, out, R, (int64_t)(se - sb) * R * R4, tid)) return;

  const double *__restrict__ xf = a.xforms + 24 * blk.i;
  map_fill_tab(s_tab, xf, fr.ox, fr.oy, fr.oz, fr.vl, R, tid);
  const MapK k = map_consts(xf, a.src, a.eps, fr);
  const float *__restrict__ d = a.src.depth + fr.off0;
  __syncthreads();

  const int nit = (se - sb) * R * R4;
  for (int item = tid; item < nit; item += kSlabWG) {
    const int f4 = (item % R4) * 4;
    const int t1 = item / R4;
    const int y = t1 % R, sl = sb + t1 / R;
    const map_d4 ty = s_tab[1][y];
    const map_d4 ts = s_tab[LAYOUT == 0 ? 2 : 0][sl];      // the slice's axis: z (czyx) or x (cxyz)
    float v0[4], v1[4], v2[4];
    map_quad<LAYOUT>(s_tab, k, d, ty, ts, f4, v0, v1, v2);
    const int64_t e = ((int64_t)sl * R + y) * R + f4;   // o[c][slow][y][fast]
    *reinterpret_cast<grid_f4 *>(out + e) = grid_f4{v0[0], v0[1], v0[2], v0[3]};
    *reinterpret_cast<grid_f4 *>(out + R3 + e) = grid_f4{v1[0], v1[1], v1[2], v1[3]};
    *reinterpret_cast<grid_f4 *>(out + 2 * R3 + e) = grid_f4{v2[0], v2[1], v2[2], v2[3]};
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
  if (slab_bad_shape(R, layout)) return TSDF_ERR_INVALID_ARG;   // after n == 0, unlike the later libraries: frozen
  if (!d_xforms || !d_grid || !d_out_tsdf || misaligned(d_xforms, 7) || misaligned(d_out_tsdf, 15))
    return TSDF_ERR_INVALID_ARG;
  SlabPlan plan;
  if (!slab_args_ok(d_depth, depth_len, d_offsets, d_headers, n, nullptr, n, R, 4, cam, plan)) return TSDF_ERR_INVALID_ARG;
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  if (!cam) cam = &kDefaultCam;
  AugGridArgs a;
  a.src = slab_src(d_depth, depth_len, d_offsets, d_headers, n, nullptr, n, R, *cam, plan);
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
