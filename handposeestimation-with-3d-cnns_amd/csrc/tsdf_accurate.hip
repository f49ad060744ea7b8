// tsdf_accurate.hip — libtsdf_accurate.so: the ACCURATE directional TSDF on a caller-supplied grid: per voxel the nearest
// surface point among all valid pixels of the crop (include/tsdf_accurate.h has the contract).
//
// A translation unit and a library of its own, next to libtsdf_hip.so and the other extension libraries (all frozen).  It
// takes the status codes and the layout enum from include/tsdf.h, the host preamble every library here has from
// device.inc, the device primitives from prim.inc, the slab scaffold it shares with tsdf_auggrid.hip, tsdf_lowp.hip and
// tsdf_maplowp.hip from slab.inc and what it shares with tsdf_mapaccurate.hip alone — the search rectangle, the bad-frame
// tail, the item's store, the host's halving and launch — from search.inc; the plain contract's projection and sign rule are RESTATED here operation for operation
// as tsdf_lowp.hip has them, and there is no device global: every launch is self-contained.
//
// tsdf_grid_accurate_kernel: n x ceil(R / slab) workgroups of 256 threads; a workgroup owns `slab` consecutive slices
// (indices of the slowest output axis) of one batch position — slab.inc's slab, halved while the launch would hold fewer
// than kMinBlocks workgroups (search.inc).  It
//   1. resolves its source frame (the index, if any) and checks the frame's header and grid row (all uniform); a position
//      that is not OK has its slab filled with zeros (nearest: -1) and workgroup 0 of the position writes the status;
//   2. walks its slab in items of 4 consecutive voxels of the fastest axis, one item per lane and pass.  Per item:
//      a. the plain contract's projection, gather and sign rule for each of the 4 voxels (`sv`: 0 rejected, else +-1);
//      b. the SEARCH REGION of the item, a pixel rectangle (below; search.inc::search_rect);
//      c. one row-major walk of that rectangle: per valid pixel the z term of each voxel first (one per item in layout
//         czyx, where the 4 voxels share z) and, where some |tz| <= 1, the float64 evaluation of s for those voxels;
//         (best s, row, column) is kept with a strict <, so ties stay with the lowest index;
//      d. per voxel the values from the best pixel, recomputed by the same sequence; three 16-byte stores, one per
//         channel, and one for `nearest` if asked.  Items are numbered in output order.
// No LDS, no work queue, no communication between workgroups, no atomics.  Compiled with -ffp-contract=off, fma only where
// __builtin_fma is written.
//
// THE SEARCH REGION.  search.inc has the argument for what may be discarded before s is evaluated (the z term, the
// corner-quotient rectangle) and the rectangle itself; what is this file's is why its six arguments bound a point w within
// T' of a voxel v.  Here the voxel and the points live in ONE frame, the camera's, so |v - w| <= T' bounds each coordinate
// by itself: w_x in [v_x - T', v_x + T'], w_y likewise, and |w_z - v_z| <= T' puts the depth d = -w_z into
// [-v_z - T', -v_z + T'].  Over the 4 voxels of an item the ranges are united: [xlo - T', xhi + T'] along the fastest axis
// of layout czyx (cxyz: the z range), one y.  The depth interval meets zero by eps where the item lies within T' (+ eps)
// of the camera plane: then the whole crop is walked.
// Tried and not kept ("Accurate directional TSDF"): a per-tile (min, max) depth cull in LDS — on hand crops a
// tile's depth range meets most voxels' interval, and the tile walk cost twice the time of this one.  Not tried: a float32
// screen, the slab's union window staged in LDS, several pixels per loop trip.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_accurate.h"

namespace {

#include "device.inc"   // check_device, launched, misaligned: the host preamble of every library here
#include "prim.inc"     // cam_ok, trunc_i32, finite32, f32_round_up, header_ok
#include "slab.inc"     // workgroup <-> slab, the frame's header and grid row, zero-fill, host sizing
#include "search.inc"   // the item, the search rectangle, the bad-frame tail, the item's store, the host's halving and launch

struct AccArgs {
  SlabSrc src;
  double inv_focal;
  float eps;
  const float *grid;        // [n_src][8]
  float *out;               // [n][3][R][R][R]
  int32_t *nearest;         // [n][R][R][R] or null
  int32_t *status;          // [n] or null
};

template <int LAYOUT>
__global__ __launch_bounds__(kSlabWG) void tsdf_grid_accurate_kernel(AccArgs a) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const int R = a.src.R, RV = R / V;
  const Slab blk = slab_of_block(a.src.nslab, a.src.slab, R);
  const int sb = blk.sb, se = blk.se;
  const int64_t R3 = (int64_t)R * R * R;
  float *__restrict__ out = a.out + blk.i * 3 * R3;
  int32_t *__restrict__ nearest = a.nearest ? a.nearest + blk.i * R3 : nullptr;

  const SlabFrame fr = slab_head<true>(a.src, blk, a.grid);
  const int left = fr.left, top = fr.top, right = fr.right, bottom = fr.bottom;
  const int64_t bw = fr.bw;
  const int64_t per = (int64_t)(se - sb) * R * RV;   // 16-byte pieces of the slab, per channel
  if (search_bad_frame(fr, blk, a.status, out, nearest, R, per, tid)) return;

  // per-frame constants, as tsdf_lowp.hip has them
  const double F = a.src.focal, cx = a.src.cx, cy = a.src.cy;
  const double ox = (double)fr.ox, oy = (double)fr.oy, oz = (double)fr.oz, vl = (double)fr.vl;
  const double T = (double)fr.td;
  const double it = 1.0 / T;
  const double kq = a.inv_focal * it;
  const double Tw = T * (1.0 + 0x1p-20);   // the window's truncation distance T' (search.inc)
  const float eps = a.eps;
  const double epsd = (double)eps;
  const float *__restrict__ d = a.src.depth + fr.off0;

  const int nit = (se - sb) * R * RV;
  for (int item = tid; item < nit; item += kSlabWG) {
    const int fv = (item % RV) * V;
    const int t1 = item / RV;
    const int y = t1 % R, sl = sb + t1 / R;
    const double vy = oy + (double)y * vl;
    const double vys = vy * it;

    // ---- a. the plain contract per voxel: centre, projection, gather, sign ----
    double vxs[V], vzs[V];
    float sv[V];
    double xlo = __builtin_inf(), xhi = -__builtin_inf(), zlo = __builtin_inf(), zhi = -__builtin_inf();
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int xi = LAYOUT == 0 ? fv + j : sl, zi = LAYOUT == 0 ? sl : fv + j;
      const double px_ = (double)xi * vl, pz_ = (double)zi * vl;
      const double vx = ox + px_, vz = oz + pz_;
      vxs[j] = vx * it;
      vzs[j] = vz * it;
      xlo = __builtin_fmin(xlo, vx), xhi = __builtin_fmax(xhi, vx);
      zlo = __builtin_fmin(zlo, vz), zhi = __builtin_fmax(zhi, vz);
      const double q = -F / vz;                                  // IEEE division
      const double mx = vx * q, my = (-vy) * q;
      const int px = trunc_i32(mx + cx), py = trunc_i32(my + cy);
      const bool inb = px >= left && px < right && py >= top && py < bottom;
      const int64_t at = inb ? (int64_t)(py - top) * bw + (px - left) : 0;   // the load is always in bounds
      const float pd = d[at];
      const bool ok = inb & (__builtin_fabsf(pd) >= eps);        // NaN is invalid
      const bool neg = pd < f32_round_up(-vz);                   // w_z > v_z
      sv[j] = ok ? (neg ? -1.0f : 1.0f) : 0.0f;
    }

    // ---- b. the item's search rectangle [c0, c1) x [r0, r1), image coordinates ----
    const SearchRect w = search_rect(xlo - Tw, xhi + Tw, vy - Tw, vy + Tw, -zhi - Tw, -zlo + Tw, epsd, F, cx, cy, left, top,
                                     right, bottom);
    const int c0 = w.c0, c1 = w.c1, r0 = w.r0, r1 = w.r1;

    // ---- c. the walk ----
    double best[V];
    int brow[V], bcol[V];
#pragma unroll
    for (int j = 0; j < V; ++j) best[j] = __builtin_inf(), brow[j] = 0, bcol[j] = -1;
    if (c0 < c1 && r0 < r1) {
      int row = r0, col = c0;
      const float *__restrict__ p = d + (int64_t)(r0 - top) * bw + (c0 - left);
      const int64_t skip = bw - (c1 - c0);
      double dyi = (double)row - cy;
      while (row < r1) {
        const float pd = *p;
        if (__builtin_fabsf(pd) >= eps) {
          const double pd64 = (double)pd;
          double tz[V];
          bool any = false;
#pragma unroll
          for (int j = 0; j < V; ++j) {
            tz[j] = LAYOUT == 0 && j > 0 ? tz[0] : __builtin_fma(pd64, it, vzs[j]);   // czyx: an item has one z
            any |= __builtin_fabs(tz[j]) <= 1.0;
          }
          if (any) {                                             // otherwise the evaluated s exceeds 1 for all four
            const double aq = pd64 * kq;
            const double ndxi = -((double)col - cx);
            const double ty = __builtin_fma(dyi, aq, vys);
#pragma unroll
            for (int j = 0; j < V; ++j) {
              if (__builtin_fabs(tz[j]) <= 1.0) {
                const double tx = LAYOUT == 1 && j > 0 ? __builtin_fma(ndxi, aq, vxs[0]) : __builtin_fma(ndxi, aq, vxs[j]);
                const double xx = tx * tx;
                const double s = __builtin_fma(tz[j], tz[j], __builtin_fma(ty, ty, xx));
                if (s < best[j]) best[j] = s, brow[j] = row, bcol[j] = col;
              }
            }
          }
        }
        ++p, ++col;
        if (col == c1) {
          col = c0, ++row, p += skip;
          dyi = (double)row - cy;
        }
      }
    }

    // ---- d. the values, from the best pixel by the same sequence ----
    acc_f4 o0, o1, o2;
    acc_i4 on;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const bool nearv = best[j] <= 1.0;
      const int64_t at = nearv ? (int64_t)(brow[j] - top) * bw + (bcol[j] - left) : 0;
      const double pd64 = (double)d[at];
      const double aq = pd64 * kq;
      const double tz = __builtin_fma(pd64, it, vzs[j]);
      const double tx = __builtin_fma(-((double)bcol[j] - cx), aq, vxs[j]);
      const double ty = __builtin_fma((double)brow[j] - cy, aq, vys);
      const float sg = sv[j] < 0.0f ? -1.0f : 1.0f;              // a rejected voxel's ray meets no surface: positive
      const float m0 = __builtin_fminf(__builtin_fabsf((float)tx), 1.0f);
      const float m1 = __builtin_fminf(__builtin_fabsf((float)ty), 1.0f);
      const float m2 = __builtin_fminf(__builtin_fabsf((float)tz), 1.0f);
      o0[j] = nearv ? m0 * sg : sv[j];
      o1[j] = nearv ? m1 * sg : sv[j];
      o2[j] = nearv ? m2 * sg : sv[j];
      on[j] = nearv ? (int)(uint32_t)(uint64_t)at : -1;
    }
    const int64_t e = ((int64_t)sl * R + y) * R + fv;   // o[c][slow][y][fast]
    search_store(out, nearest, R3, e, o0, o1, o2, on);
  }
}

}  // namespace

extern "C" {

int tsdf_accurate_version(void) { return TSDF_ACCURATE_VERSION; }

int tsdf_voxelize_grid_accurate_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets,
                                    const int32_t *d_headers, int64_t n_src, const int64_t *d_index, int n, int R,
                                    double focal, double cx, double cy, float invalid_eps, float trunc_voxels,
                                    int layout, void *hip_stream, const float *d_grid, float *d_out_tsdf,
                                    int32_t *d_out_nearest, int32_t *d_out_status) {
  // arguments first, then the device, then the launch
  if (n < 0) return TSDF_ERR_INVALID_ARG;
  if (slab_bad_shape(R, layout)) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_grid || !d_out_tsdf || misaligned(d_out_tsdf, 15) || misaligned(d_out_nearest, 15)) return TSDF_ERR_INVALID_ARG;
  const tsdf_cam cam = {focal, cx, cy, invalid_eps, trunc_voxels};   // by value in the ABI, one rule all the same
  SlabPlan plan;
  if (!slab_args_ok(d_depth, depth_len, d_offsets, d_headers, n_src, d_index, n, R, V, &cam, plan))
    return TSDF_ERR_INVALID_ARG;
  search_halve(plan, n, R);   // bound by its search: below kMinBlocks workgroups the slabs are halved
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  AccArgs a;
  a.src = slab_src(d_depth, depth_len, d_offsets, d_headers, n_src, d_index, n, R, cam, plan);
  a.inv_focal = 1.0 / focal;
  a.eps = invalid_eps;
  a.grid = d_grid;
  a.out = d_out_tsdf;
  a.nearest = d_out_nearest;
  a.status = d_out_status;
  return search_launch(tsdf_grid_accurate_kernel<0>, tsdf_grid_accurate_kernel<1>, layout, plan, hip_stream, a);
}

}  // extern "C"
