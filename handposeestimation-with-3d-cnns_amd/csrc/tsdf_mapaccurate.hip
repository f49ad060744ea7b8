// tsdf_mapaccurate.hip — libtsdf_mapaccurate.so: the ACCURATE directional TSDF under a per-frame map, on a caller-supplied
// grid: per voxel the nearest MAPPED surface point among all valid pixels of the crop (include/tsdf_mapaccurate.h has the
// contract).  tsdf_accurate.hip is the same search without a map, tsdf_auggrid.hip the same map without a search.
//
// A translation unit and a library of its own, next to libtsdf_hip.so and the other extension libraries (all frozen).  It
// takes the status codes and the layout enum from include/tsdf.h, the host preamble every library here has from
// device.inc, the device primitives from prim.inc, the slab scaffold from slab.inc, what the two accurate kernels share
// beyond it (the search rectangle, the bad-frame tail, the item's store, the host's halving and launch) from search.inc
// and, from mapvox.inc, the per-axis
// table and the per-frame constants of the mapped arithmetic (map_fill_tab, map_consts) — the text tsdf_auggrid.hip and
// tsdf_maplowp.hip run.  The projection and the distance terms are restated here operation for operation as
// mapvox.inc::map_quad has them, because here the terms are evaluated per CANDIDATE pixel.  No device global: every launch
// is self-contained.
//
// tsdf_map_grid_accurate_kernel: n x ceil(R / slab) workgroups of 256 threads; a workgroup owns `slab` consecutive slices
// of one batch position — slab.inc's slab, halved while the launch would hold fewer than kMinBlocks workgroups (search.inc).  It
//   1. resolves its source frame (the index, if any) and checks the frame's header and the POSITION's grid row (all
//      uniform); a position that is not OK has its slab filled with zeros (nearest: -1) and workgroup 0 of the position
//      writes the status;
//   2. tabulates the per-axis terms (mapvox.inc::map_fill_tab, 12 KiB of LDS), and thread 0 inverts the FORWARD 3x3 in
//      float64 and judges the inverse (window_consts: 14 doubles in LDS); one barrier; the uniform constants go to
//      scalar registers (uniform64);
//   3. walks its slab in items of 4 consecutive voxels of the fastest axis, one item per lane and pass.  Per item:
//      a. per voxel the mapped contract's projection (the INVERSE rows), gather and sign (`sv`: 0 rejected, else +-1 by
//         the projected pixel's u_z), and the voxel's camera-frame centre B (v' - b), B the kernel's own inverse;
//      b. the SEARCH REGION of the item, a pixel rectangle (below; search.inc::search_rect);
//      c. one row-major walk of that rectangle.  The c_i depend on the pixel only and their fma(g_i1, dyi, A_i2) on the
//         row only; u_i differs between the 4 voxels only in its addend, and only along the fastest axis: in layout czyx
//         the item has ONE t_z and ONE t_y and four t_x, in cxyz one t_x, one t_y and four t_z.  Per valid pixel the z
//         term(s) first and, where some |t_z| <= 1, the rest; (best s, row, column) is kept with a strict <, so ties stay
//         with the lowest index, and a NaN s wins nothing;
//      d. per voxel the values from the best pixel, recomputed by the same sequence, clamped and signed in float64 and
//         rounded once (map_quad's order); three 16-byte stores, one per channel, and one for `nearest` if asked.
// No work queue, no communication between workgroups, no atomics.  Compiled with -ffp-contract=off, fma only where
// __builtin_fma is written.
//
// THE SEARCH REGION.  search.inc has the argument for what may be discarded before s is evaluated (the z term — here
// tz = u_z * it, and the argument does not look at how tz came about — and the corner-quotient rectangle) and the
// rectangle itself; what is this file's is why its six arguments bound, in the CAMERA frame, a point w whose mapped image
// is within T of the voxel.  Over the reals u = (v' - b) - A w for the point w of a pixel.  Let B be ANY 3x3 (the kernel's
// computed inverse, exact as the float64 numbers it holds), Res = B A - I, c = B (v' - b).  Then B u = c - w - Res w, so
//         |w_a - c_a| <= ||row a of B||_2 |u|_2 + rho |w|_2,   rho = ||Res||_F,
//     and from |w| <= |c| + |w - c| and |w - c| <= ||B||_F |u| + rho |w|:  for rho <= 1/4 and |u| <= T
//         |w_a - c_a| <= T h_a + 2 rho (|c|_1 + ||B||_F T),     h_a = ||row a of B||_2.
//     That bounds each CAMERA coordinate of a point within T of the voxel by the half-extent H_a around c_a, whatever B
//     is — a poor inverse only has a large rho.  So w_x is in [c_x - H_x, c_x + H_x], w_y likewise and the depth d = -w_z
//     in [-c_z - H_z, -c_z + H_z]; over the item's 4 voxels the ranges of c are united (clo, chi).  The kernel uses
//     T' = T (1 + 2^-20) for T and rho' = rho + 2^-30 for rho: a pixel outside has a real |u| > T'; 2^-30 covers the
//     float64 roundings of Res, h_a (a square root of three products) and c (relative 2^-50 ||B|| ||A|| each) under the
//     conditions below, and under their magnitudes the sequence's evaluation error is the 2^-40 search.inc counts on.
//     The rectangle is used only where the inverse can be TRUSTED: ||A||_F and ||B||_F both <= 2^20, ||A||_F ||B||_F <=
//     2^16 and rho <= 2^-24, each written so that a NaN fails (a zero or non-finite determinant gives a non-finite B or a
//     rho of sqrt 3).  Otherwise, and where the depth interval does not stay on one side of zero by invalid_eps, there is
//     NO rectangle and the whole crop is walked.  The caller's inverse rows never enter: they may disagree with the
//     forward rows, and s is defined by the forward rows alone.
// REGISTERS.  The per-frame constants (the six g, it, T', the nine entries and three row norms of B, the slack's two
// factors) are the same in every lane; uniform64 moves them into scalar registers, which takes the kernel from 132 / 130
// vector registers (3 waves per SIMD) to 94 / 92 (5 waves) and the 64^3 shape from 7.07 to 5.46 ms.
// Tried and not kept: a cap of 3 or 4 waves per SIMD on top of that (amdgpu_waves_per_eu) — 4 % faster at 1024 crops 32^3
// in layout czyx, 10-35 % slower at every other shape and layout measured.  Not tried: skipping on tz^2 >= best so far
// (the contract allows it), a float32 screen, the slab's union window staged in LDS.  (tsdf_accurate.hip records the
// per-tile depth cull that was tried there and not kept.)

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_mapaccurate.h"

namespace {

#include "device.inc"   // check_device, launched, misaligned: the host preamble of every library here
#include "prim.inc"     // cam_ok, trunc_i32, finite32, header_ok
#include "slab.inc"     // workgroup <-> slab, the frame's header and grid row, zero-fill, host sizing
#include "search.inc"   // the item, the search rectangle, the bad-frame tail, the item's store, the host's halving and launch
#include "mapvox.inc"   // map_fill_tab, MapK, map_consts: the mapped arithmetic's table and constants

struct MapAccArgs {
  SlabSrc src;
  float eps;
  const double *xforms;     // [n][24]
  const float *grid;        // [n][8]
  float *out;               // [n][3][R][R][R]
  int32_t *nearest;         // [n][R][R][R] or null
  int32_t *status;          // [n] or null
};

// A float64 every lane holds the same value of (computed from uniform inputs by the same operations), moved into scalar
// registers: v_fma_f64 and its kin take one scalar operand, and the per-frame constants then cost no vector registers.
__device__ __forceinline__ double uniform64(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// w[0..8]: B, the float64 inverse of the forward 3x3 by cofactors; w[9..11]: h_a = ||row a of B||_2; w[12]: ||B||_F;
// w[13]: 2 rho' where the inverse is trusted, else a NaN (no rectangle).  The head of this file has the conditions.
__device__ __forceinline__ void window_consts(const double *__restrict__ xf, double *w) {
#pragma clang fp contract(off)
  const double a00 = xf[0], a01 = xf[1], a02 = xf[2], a10 = xf[4], a11 = xf[5], a12 = xf[6], a20 = xf[8], a21 = xf[9],
               a22 = xf[10];
  const double k00 = a11 * a22 - a12 * a21, k01 = a12 * a20 - a10 * a22, k02 = a10 * a21 - a11 * a20;
  const double det = (a00 * k00 + a01 * k01) + a02 * k02;
  const double id = 1.0 / det;
  double B[9];
  B[0] = k00 * id, B[1] = (a02 * a21 - a01 * a22) * id, B[2] = (a01 * a12 - a02 * a11) * id;
  B[3] = k01 * id, B[4] = (a00 * a22 - a02 * a20) * id, B[5] = (a02 * a10 - a00 * a12) * id;
  B[6] = k02 * id, B[7] = (a01 * a20 - a00 * a21) * id, B[8] = (a00 * a11 - a01 * a10) * id;
  const double A[9] = {a00, a01, a02, a10, a11, a12, a20, a21, a22};
  double nA = 0.0, nB = 0.0, rr = 0.0;
  for (int i = 0; i < 3; ++i) {
    double hh = 0.0;
    for (int j = 0; j < 3; ++j) {
      nA = nA + A[3 * i + j] * A[3 * i + j];
      hh = hh + B[3 * i + j] * B[3 * i + j];
      const double r = ((B[3 * i] * A[j] + B[3 * i + 1] * A[3 + j]) + B[3 * i + 2] * A[6 + j]) - (i == j ? 1.0 : 0.0);
      rr = rr + r * r;
    }
    nB = nB + hh;
    w[9 + i] = __builtin_sqrt(hh);
  }
  nA = __builtin_sqrt(nA), nB = __builtin_sqrt(nB);
  const double rho = __builtin_sqrt(rr);
  const bool trusted = nA <= 0x1p20 && nB <= 0x1p20 && nA * nB <= 0x1p16 && rho <= 0x1p-24;   // a NaN fails each
  for (int e = 0; e < 9; ++e) w[e] = B[e];
  w[12] = nB;
  w[13] = trusted ? 2.0 * (rho + 0x1p-30) : __builtin_nan("");
}

template <int LAYOUT>
__global__ __launch_bounds__(kSlabWG) void tsdf_map_grid_accurate_kernel(MapAccArgs a) {
#pragma clang fp contract(off)
  __shared__ map_d4 s_tab[3][kSlabMaxR];
  __shared__ double s_win[14];

  const int tid = threadIdx.x;
  const int R = a.src.R, RV = R / V;
  const Slab blk = slab_of_block(a.src.nslab, a.src.slab, R);
  const int sb = blk.sb, se = blk.se;
  const int64_t R3 = (int64_t)R * R * R;
  float *__restrict__ out = a.out + blk.i * 3 * R3;
  int32_t *__restrict__ nearest = a.nearest ? a.nearest + blk.i * R3 : nullptr;

  const SlabFrame fr = slab_head<false>(a.src, blk, a.grid);   // the grid row is the POSITION's
  const int64_t per = (int64_t)(se - sb) * R * RV;   // 16-byte pieces of the slab, per channel
  if (search_bad_frame(fr, blk, a.status, out, nearest, R, per, tid)) return;

  const double *__restrict__ xf = a.xforms + 24 * blk.i;
  map_fill_tab(s_tab, xf, fr.ox, fr.oy, fr.oz, fr.vl, R, tid);
  if (tid == 0) window_consts(xf, s_win);
  MapK k = map_consts(xf, a.src, a.eps, fr);
  k.it = uniform64(k.it);
  k.g00 = uniform64(k.g00), k.g10 = uniform64(k.g10), k.g20 = uniform64(k.g20);
  k.g01 = uniform64(k.g01), k.g11 = uniform64(k.g11), k.g21 = uniform64(k.g21);
  const int left = k.left, top = k.top, right = k.right, bottom = k.bottom;
  const int64_t bw = k.bw;
  const float eps = k.eps;
  const double epsd = (double)eps;
  const double Tw = uniform64((double)fr.td * (1.0 + 0x1p-20));   // the window's truncation distance T' (search.inc)
  const float *__restrict__ d = a.src.depth + fr.off0;
  __syncthreads();
  double B[9], hB[3];                                  // the window's constants, out of LDS once
#pragma unroll
  for (int e = 0; e < 9; ++e) B[e] = uniform64(s_win[e]);
#pragma unroll
  for (int e = 0; e < 3; ++e) hB[e] = uniform64(s_win[9 + e]);
  const double rho2 = uniform64(s_win[13]);
  const bool windowed = rho2 == rho2;                  // (uniform) the inverse is trusted
  const double slack0 = uniform64(rho2 * (s_win[12] * Tw));   // 2 rho' ||B||_F T'

  const int nit = (se - sb) * R * RV;
  for (int item = tid; item < nit; item += kSlabWG) {
    const int fv = (item % RV) * V;
    const int t1 = item / RV;
    const int y = t1 % R, sl = sb + t1 / R;
    const map_d4 ty = s_tab[1][y];
    const map_d4 ts = s_tab[LAYOUT == 0 ? 2 : 0][sl];          // the slice's axis: z (czyx) or x (cxyz)

    // ---- a. the mapped contract per voxel: projection, gather, sign; the camera-frame centre ----
    double wf[V];                                              // v' - b along the fastest axis: x (czyx) or z (cxyz)
    float sv[V];
    double clo[3], chi[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) clo[i] = __builtin_inf(), chi[i] = -__builtin_inf();
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const map_d4 tf = s_tab[LAYOUT == 0 ? 0 : 2][fv + j];
      const map_d4 tx = LAYOUT == 0 ? tf : ts, tz = LAYOUT == 0 ? ts : tf;
      wf[j] = tf.w;
      // v = T^-1(v') = (A'_i0 x' + A'_i1 y') + (A'_i2 z' + b'_i)
      const double s0 = tx.x + ty.x, s1 = tx.y + ty.y, s2 = tx.z + ty.z;
      const double vx = s0 + tz.x, vy = s1 + tz.y, vz = s2 + tz.z;
      const double q = -k.F / vz;                              // IEEE division
      const double mx = vx * q, my = (-vy) * q;
      const int px = trunc_i32(mx + k.cx), py = trunc_i32(my + k.cy);
      const bool inb = px >= left && px < right && py >= top && py < bottom;
      const int64_t at = inb ? (int64_t)(py - top) * bw + (px - left) : 0;   // the load is always in bounds
      const float pd = d[at];
      const bool ok = inb & (__builtin_fabsf(pd) >= eps);      // NaN is invalid
      const double dxi = (double)px - k.cx, dyi = (double)py - k.cy;
      const double c2 = __builtin_fma(k.g20, dxi, __builtin_fma(k.g21, dyi, k.a22));
      const double u2 = __builtin_fma((double)pd, c2, tz.w);
      sv[j] = ok ? (u2 < 0.0 ? -1.0f : 1.0f) : 0.0f;
      if (windowed) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double c = (B[3 * i] * tx.w + B[3 * i + 1] * ty.w) + B[3 * i + 2] * tz.w;   // B (v' - b)
          clo[i] = __builtin_fmin(clo[i], c), chi[i] = __builtin_fmax(chi[i], c);
        }
      }
    }

    // ---- b. the item's search rectangle [c0, c1) x [r0, r1), image coordinates ----
    SearchRect w = {left, right, top, bottom};               // an inverse that is not trusted: the whole crop
    if (windowed) {
      double c1n = 0.0;                                        // the largest |c|_1 of the four
#pragma unroll
      for (int i = 0; i < 3; ++i) c1n = c1n + __builtin_fmax(__builtin_fabs(clo[i]), __builtin_fabs(chi[i]));
      const double slack = __builtin_fma(rho2, c1n, slack0);   // 2 rho' (|c|_1 + ||B||_F T')
      const double Hx = __builtin_fma(Tw, hB[0], slack), Hy = __builtin_fma(Tw, hB[1], slack),
                   Hz = __builtin_fma(Tw, hB[2], slack);
      w = search_rect(clo[0] - Hx, chi[0] + Hx, clo[1] - Hy, chi[1] + Hy, -chi[2] - Hz, -clo[2] + Hz, epsd, k.F, k.cx, k.cy,
                      left, top, right, bottom);
    }
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
      double dyi = (double)row - k.cy;
      double e0 = __builtin_fma(k.g01, dyi, k.a02), e1 = __builtin_fma(k.g11, dyi, k.a12),
             e2 = __builtin_fma(k.g21, dyi, k.a22);
      while (row < r1) {
        const float pd = *p;
        if (__builtin_fabsf(pd) >= eps) {
          const double pd64 = (double)pd;
          const double dxi = (double)col - k.cx;
          const double c2 = __builtin_fma(k.g20, dxi, e2);
          double tz[V];
          bool any = false;
#pragma unroll
          for (int j = 0; j < V; ++j) {
            // czyx: an item has one z
            tz[j] = LAYOUT == 0 ? (j > 0 ? tz[0] : __builtin_fma(pd64, c2, ts.w) * k.it) : __builtin_fma(pd64, c2, wf[j]) * k.it;
            any |= __builtin_fabs(tz[j]) <= 1.0;
          }
          if (any) {                                           // otherwise the evaluated s exceeds 1 for all four
            const double cc0 = __builtin_fma(k.g00, dxi, e0), cc1 = __builtin_fma(k.g10, dxi, e1);
            const double t1v = __builtin_fma(pd64, cc1, ty.w) * k.it;
#pragma unroll
            for (int j = 0; j < V; ++j) {
              if (__builtin_fabs(tz[j]) <= 1.0) {
                const double t0v = __builtin_fma(pd64, cc0, LAYOUT == 0 ? wf[j] : ts.w) * k.it;   // cxyz: an item has one x
                const double xx = t0v * t0v;
                const double s = __builtin_fma(tz[j], tz[j], __builtin_fma(t1v, t1v, xx));
                if (s < best[j]) best[j] = s, brow[j] = row, bcol[j] = col;
              }
            }
          }
        }
        ++p, ++col;
        if (col == c1) {
          col = c0, ++row, p += skip;
          dyi = (double)row - k.cy;
          e0 = __builtin_fma(k.g01, dyi, k.a02), e1 = __builtin_fma(k.g11, dyi, k.a12), e2 = __builtin_fma(k.g21, dyi, k.a22);
        }
      }
    }

    // ---- d. the values, from the best pixel by the same sequence; clamp and sign in float64, one rounding ----
    acc_f4 o0, o1, o2;
    acc_i4 on;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const bool nearv = best[j] <= 1.0;
      const int64_t at = nearv ? (int64_t)(brow[j] - top) * bw + (bcol[j] - left) : 0;
      const double pd64 = (double)d[at];
      const double dxi = (double)bcol[j] - k.cx, dyi = (double)brow[j] - k.cy;
      const double cc0 = __builtin_fma(k.g00, dxi, __builtin_fma(k.g01, dyi, k.a02));
      const double cc1 = __builtin_fma(k.g10, dxi, __builtin_fma(k.g11, dyi, k.a12));
      const double cc2 = __builtin_fma(k.g20, dxi, __builtin_fma(k.g21, dyi, k.a22));
      const double t0v = __builtin_fma(pd64, cc0, LAYOUT == 0 ? wf[j] : ts.w) * k.it;
      const double t1v = __builtin_fma(pd64, cc1, ty.w) * k.it;
      const double t2v = __builtin_fma(pd64, cc2, LAYOUT == 0 ? ts.w : wf[j]) * k.it;
      double m0 = __builtin_fabs(t0v), m1 = __builtin_fabs(t1v), m2 = __builtin_fabs(t2v);
      if (!(m0 < 1.0)) m0 = 1.0;
      if (!(m1 < 1.0)) m1 = 1.0;
      if (!(m2 < 1.0)) m2 = 1.0;
      if (sv[j] < 0.0f) {
        m0 = -m0;
        m1 = -m1;
        m2 = -m2;
      }
      o0[j] = nearv ? (float)m0 : sv[j];
      o1[j] = nearv ? (float)m1 : sv[j];
      o2[j] = nearv ? (float)m2 : sv[j];
      on[j] = nearv ? (int)(uint32_t)(uint64_t)at : -1;
    }
    const int64_t e = ((int64_t)sl * R + y) * R + fv;   // o[c][slow][y][fast]
    search_store(out, nearest, R3, e, o0, o1, o2, on);
  }
}

}  // namespace

extern "C" {

int tsdf_mapaccurate_version(void) { return TSDF_MAPACCURATE_VERSION; }

int tsdf_voxelize_map_grid_accurate_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets,
                                        const int32_t *d_headers, int64_t n_src, const int64_t *d_index, int n, int R,
                                        double focal, double cx, double cy, float invalid_eps, float trunc_voxels,
                                        int layout, void *hip_stream, const double *d_xforms, const float *d_grid,
                                        float *d_out_tsdf, int32_t *d_out_nearest, int32_t *d_out_status) {
  // arguments first, then the device, then the launch
  if (n < 0) return TSDF_ERR_INVALID_ARG;
  if (slab_bad_shape(R, layout)) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_xforms || !d_grid || !d_out_tsdf || misaligned(d_xforms, 7) || misaligned(d_out_tsdf, 15) ||
      misaligned(d_out_nearest, 15))
    return TSDF_ERR_INVALID_ARG;
  const tsdf_cam cam = {focal, cx, cy, invalid_eps, trunc_voxels};   // by value in the ABI, one rule all the same
  SlabPlan plan;
  if (!slab_args_ok(d_depth, depth_len, d_offsets, d_headers, n_src, d_index, n, R, V, &cam, plan))
    return TSDF_ERR_INVALID_ARG;
  search_halve(plan, n, R);   // bound by its search: below kMinBlocks workgroups the slabs are halved
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  MapAccArgs a;
  a.src = slab_src(d_depth, depth_len, d_offsets, d_headers, n_src, d_index, n, R, cam, plan);
  a.eps = invalid_eps;
  a.xforms = d_xforms;
  a.grid = d_grid;
  a.out = d_out_tsdf;
  a.nearest = d_out_nearest;
  a.status = d_out_status;
  return search_launch(tsdf_map_grid_accurate_kernel<0>, tsdf_map_grid_accurate_kernel<1>, layout, plan, hip_stream, a);
}

}  // extern "C"
