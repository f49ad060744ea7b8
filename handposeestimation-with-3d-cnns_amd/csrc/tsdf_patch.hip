// tsdf_patch.hip — libtsdf_patch.so: depth-image patches resampled from the located cube's rectangle, the joints in the
// patch's normalised (u, v, d) coordinates and the way back (include/tsdf_patch.h, which has the contracts operation by
// operation).
//
// A translation unit and a library of its own, next to libtsdf_hip.so and the other libraries (all frozen).  It takes the
// status codes from include/tsdf.h, the host preamble every library here has from device.inc, cam_ok / finite32 /
// header_ok from prim.inc, the 2-byte store side from narrow.inc and its argument rules and its plan from
// patch_host.inc, plain C++ that is also built on its own under the CPU sanitizers.  No device global and no atomic:
// every launch is self-contained.
//
// THE PATCH KERNEL is a gather.  A work ITEM is (batch position, band of rows of its patch); a workgroup of kPatchWG lanes
// walks the items by a grid-stride loop.  Per item:
//   1. PROLOGUE (patch_prologue), lane 0 alone: the position's status, the cube's rectangle u0, v0, du, dv, 1 / h, the
//      affine row, the source rectangle and its base — every division of the contract but s / w — into LDS.  The two
//      entries differ here and nowhere else: frames take the whole frame of their index, crops the header's rectangle once
//      header_ok accepts it.  One barrier, then every lane reads the constants as broadcasts.
//   2. A lane owns V adjacent pixels of one row (V = 4 float32, 8 two-byte): per pixel the contract's u and v, one tap or
//      four as plain global loads (under the identity a row of the patch walks a row of the source), the depth test, the
//      normalisation — and ONE 16-byte store of the V values.
// THE LABEL KERNELS are one thread per joint, each forming its position's constants itself.
// All global indexing is in 64 bits.  Compiled with -ffp-contract=off: no fused multiply-add anywhere in this file.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_patch.h"

namespace {

#include "device.inc"       // check_device, launched, misaligned: the host preamble of every library here
#include "prim.inc"         // cam_ok, finite32, header_ok
#include "narrow.inc"       // narrow2, store_vol, bad_dtype: the 16-byte store of a lane's pixels
#include "patch_host.inc"   // patch_*_defect, patch_plan, patch_groups, kPatchWG

// what fixes the cube of a position: the arguments common to the four launching entries
struct PatchGeo {
  const double *com;          // [n][3]
  float cube;
  const float *cube_n;        // [n] or null
  const double *affine;       // [n][6] or null
  const int32_t *status_in;   // [n] or null
  double focal, cx, cy;
};

// rule 2's rectangle and what else a pixel or a joint needs of its position
struct PatchCube {
  double u0, v0, du, dv, rh, cd, h;
  double a00, a01, a02, a10, a11, a12;   // the affine row; unset without one
};

__device__ __forceinline__ bool finite64(double v) { return __builtin_fabs(v) < __builtin_inf(); }   // false for NaN

// Rule 1's status 1 and, for a position without it, rule 2.  Returns 0 or TSDF_FRAME_DEGENERATE.
__device__ __forceinline__ int patch_cube(const PatchGeo &g, int64_t i, PatchCube &c) {
#pragma clang fp contract(off)
  if (g.status_in && g.status_in[i] != 0) return TSDF_FRAME_DEGENERATE;
  const double *com = g.com + 3 * i;
  const double c_x = com[0], c_y = com[1], cd = -com[2];
  const float cube = g.cube_n ? g.cube_n[i] : g.cube;
  if (!finite64(c_x) || !finite64(c_y) || !finite64(cd) || !(cd > 0.0)) return TSDF_FRAME_DEGENERATE;
  if (!finite32(cube) || !(cube > 0.0f)) return TSDF_FRAME_DEGENERATE;
  if (g.affine) {
    const double *row = g.affine + 6 * i;
    c.a00 = row[0], c.a01 = row[1], c.a02 = row[2], c.a10 = row[3], c.a11 = row[4], c.a12 = row[5];
    if (!finite64(c.a00) || !finite64(c.a01) || !finite64(c.a02) || !finite64(c.a10) || !finite64(c.a11) || !finite64(c.a12))
      return TSDF_FRAME_DEGENERATE;
  }
  const double F = g.focal, h = (double)cube / 2.0;
  c.h = h, c.rh = 1.0 / h, c.cd = cd;
  c.u0 = ((c_x - h) * F) / cd + g.cx;
  const double u1 = ((c_x + h) * F) / cd + g.cx;
  c.v0 = ((-(c_y + h)) * F) / cd + g.cy;
  const double v1 = ((-(c_y - h)) * F) / cd + g.cy;
  c.du = u1 - c.u0, c.dv = v1 - c.v0;
  return TSDF_FRAME_OK;
}

struct PatchArgs {
  PatchGeo g;
  const void *src;            // the frames, or the pack's depth
  const int64_t *offsets;     // crops: [n_src + 1]
  const int32_t *headers;     // crops: [n_src][6]
  int64_t depth_len;          // crops
  int64_t n_src;
  int H, W;                   // frames
  int crops, u16;
  float scale;                // 2^-shift (1 for float32)
  const int64_t *index;       // [n] or null
  int64_t items;              // n * plan.items
  int S;
  PatchPlan plan;
  double rS;                  // 1.0 / S
  float background, eps;
  void *out;                  // [n][S][S]
  int32_t *status;            // [n]
};

// an item's constants, formed once by lane 0
struct PatchPos {
  PatchCube c;
  double left, top, right, bottom;   // the source rectangle, for the float64 compares of rule 4
  int64_t base, width, pos;
  int lefti, topi, band, status, mapped;
};

__device__ __forceinline__ void patch_prologue(const PatchArgs &a, int64_t item, PatchPos &p) {
  const int64_t pos = item / a.plan.items;
  p.pos = pos, p.band = (int)(item - pos * a.plan.items), p.mapped = a.g.affine != nullptr;
  int st = patch_cube(a.g, pos, p.c);
  if (st == TSDF_FRAME_OK) {
    const int64_t g = a.index ? a.index[pos] : pos;
    if (g < 0 || g >= a.n_src) {
      st = TSDF_FRAME_BAD_HEADER;
    } else if (a.crops) {
      const int32_t *hd = a.headers + 6 * g;
      const int left = hd[2], top = hd[3], right = hd[4], bottom = hd[5];
      const int64_t off0 = a.offsets[g], off1 = a.offsets[g + 1], depth_len = a.depth_len;
      if (header_ok(left, top, right, bottom, off0, off1, depth_len)) {
        p.left = (double)left, p.top = (double)top, p.right = (double)right, p.bottom = (double)bottom;
        p.base = off0, p.width = (int64_t)right - left, p.lefti = left, p.topi = top;
      } else {
        st = TSDF_FRAME_BAD_HEADER;
      }
    } else {
      p.left = 0.0, p.top = 0.0, p.right = (double)a.W, p.bottom = (double)a.H;
      p.base = g * a.H * a.W, p.width = a.W, p.lefti = 0, p.topi = 0;
    }
  }
  p.status = st;
  if (p.band == 0) a.status[pos] = st;
}

// Rule 4: the tap (x, y), two float64 whole numbers.  True with its depth in d iff it is valid.  The range compares fail
// for a NaN and for an infinity, and come before the conversion to integers, which is then exact.
__device__ __forceinline__ bool patch_tap(const PatchArgs &a, const PatchPos &p, double x, double y, double &d) {
  if (!(x >= p.left && x < p.right && y >= p.top && y < p.bottom)) return false;
  const int64_t e = p.base + (int64_t)((int)y - p.topi) * p.width + ((int)x - p.lefti);
  const float f = a.u16 ? (float)static_cast<const uint16_t *>(a.src)[e] * a.scale : static_cast<const float *>(a.src)[e];
  if (!finite32(f) || !(__builtin_fabsf(f) >= a.eps)) return false;
  d = (double)f;
  return __builtin_fabs(d - p.c.cd) <= p.c.h;
}

// DT: 0 float32, TSDF_LOWP_F16, TSDF_LOWP_BF16
template <int DT, bool BILINEAR>
__global__ __launch_bounds__(kPatchWG) void tsdf_patch_kernel(PatchArgs a) {
#pragma clang fp contract(off)
  constexpr int V = DT == 0 ? 4 : 8;
  __shared__ PatchPos s_pos;

  const int tid = threadIdx.x, S = a.S;
  const int r_in = tid / a.plan.lanes_per_row, col0 = (tid - r_in * a.plan.lanes_per_row) * V;   // col0 + V <= S
  const bool lane_on = r_in < a.plan.rows;
  char *out = static_cast<char *>(a.out);
  for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x) {   // the bounds are the workgroup's
    __syncthreads();   // the readers of the last item are done
    if (tid == 0) patch_prologue(a, item, s_pos);
    __syncthreads();
    const PatchPos &p = s_pos;
    const int row = p.band * a.plan.rows + r_in;
    if (!lane_on || row >= S) continue;
    float f[V];
#pragma unroll
    for (int j = 0; j < V; ++j) f[j] = a.background;
    if (p.status == TSDF_FRAME_OK) {
      const double b = (double)(2 * row + 1) * a.rS - 1.0;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const double aa = (double)(2 * (col0 + j) + 1) * a.rS - 1.0;
        double ap = aa, bp = b;
        if (p.mapped) {   // uniform
          ap = (p.c.a00 * aa + p.c.a01 * b) + p.c.a02;
          bp = (p.c.a10 * aa + p.c.a11 * b) + p.c.a12;
        }
        const double u = p.c.u0 + ((ap + 1.0) * 0.5) * p.c.du;
        const double v = p.c.v0 + ((bp + 1.0) * 0.5) * p.c.dv;
        if constexpr (!BILINEAR) {
          double d;
          if (patch_tap(a, p, __builtin_floor(u + 0.5), __builtin_floor(v + 0.5), d)) f[j] = (float)((d - p.c.cd) * p.c.rh);
        } else {
          const double x0 = __builtin_floor(u), y0 = __builtin_floor(v);
          const double fx = u - x0, fy = v - y0;
          const double gx = 1.0 - fx, gy = 1.0 - fy;
          const double wk[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
          double s = 0.0, w = 0.0;
          int have = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            double d;
            if (patch_tap(a, p, (k & 1) ? x0 + 1.0 : x0, (k & 2) ? y0 + 1.0 : y0, d)) s = s + wk[k] * d, w = w + wk[k], ++have;
          }
          if (have != 0 && w != 0.0) {
            const double dbar = have == 4 ? s : s / w;
            f[j] = (float)((dbar - p.c.cd) * p.c.rh);
          }
        }
      }
    }
    const int64_t e = (p.pos * S + row) * S + col0;
    if constexpr (DT == 0) {
      const lowp_u4 o = {__builtin_bit_cast(unsigned, f[0]), __builtin_bit_cast(unsigned, f[1]),
                         __builtin_bit_cast(unsigned, f[2]), __builtin_bit_cast(unsigned, f[3])};
      store_vol((GlobalOut)(out + e * 4), o);
    } else {
      lowp_u4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = narrow2<DT == TSDF_LOWP_BF16>(f[2 * j], f[2 * j + 1]);
      store_vol((GlobalOut)(out + e * 2), o);
    }
  }
}

struct PatchLabelArgs {
  PatchGeo g;
  const float *in;        // [n][J][3]: joints (uvd kernel) or uvd (joints kernel)
  int J;
  int64_t total;          // n * J < 2^31
  float *out;             // [n][J][3]
  int32_t *valid;         // uvd kernel: [n][J]
  int32_t *status;        // uvd kernel: [n]
};

__global__ __launch_bounds__(kPatchWG) void tsdf_patch_uvd_kernel(PatchLabelArgs a) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * kPatchWG + threadIdx.x;
  if (t >= a.total) return;
  const int64_t pos = t / a.J;
  PatchCube c;
  int st = patch_cube(a.g, pos, c);
  double det = 1.0;
  if (st == TSDF_FRAME_OK && a.g.affine) {
    det = c.a00 * c.a11 - c.a01 * c.a10;
    if (!(det != 0.0) || !finite64(det)) st = TSDF_FRAME_DEGENERATE;
  }
  if (t - pos * a.J == 0) a.status[pos] = st;
  const float *q = a.in + 3 * t;
  const float X = q[0], Y = q[1], Z = q[2];
  const double dj = -(double)Z;
  float ua = 0.f, ub = 0.f, uw = 0.f;
  const bool ok = st == TSDF_FRAME_OK && finite32(X) && finite32(Y) && finite32(Z) && dj > 0.0;
  if (ok) {
    const double u = ((double)X * a.g.focal) / dj + a.g.cx;
    const double v = ((-(double)Y) * a.g.focal) / dj + a.g.cy;
    const double ap = ((u - c.u0) / c.du) * 2.0 - 1.0;
    const double bp = ((v - c.v0) / c.dv) * 2.0 - 1.0;
    double pa = ap, pb = bp;
    if (a.g.affine) {
      const double ta = ap - c.a02, tb = bp - c.a12;
      pa = (c.a11 * ta - c.a01 * tb) / det;
      pb = (c.a00 * tb - c.a10 * ta) / det;
    }
    ua = (float)pa, ub = (float)pb, uw = (float)((dj - c.cd) * c.rh);
  }
  float *o = a.out + 3 * t;
  o[0] = ua, o[1] = ub, o[2] = uw;
  a.valid[t] = ok ? 1 : 0;
}

__global__ __launch_bounds__(kPatchWG) void tsdf_patch_joints_kernel(PatchLabelArgs a) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * kPatchWG + threadIdx.x;
  if (t >= a.total) return;
  const int64_t pos = t / a.J;
  PatchCube c;
  const int st = patch_cube(a.g, pos, c);
  float X = 0.f, Y = 0.f, Z = 0.f;
  if (st == TSDF_FRAME_OK) {
    const float *q = a.in + 3 * t;
    const double pa = (double)q[0], pb = (double)q[1], w = (double)q[2];
    const double depth = w * c.h + c.cd;
    double ap = pa, bp = pb;
    if (a.g.affine) {
      ap = (c.a00 * pa + c.a01 * pb) + c.a02;
      bp = (c.a10 * pa + c.a11 * pb) + c.a12;
    }
    const double u = c.u0 + ((ap + 1.0) * 0.5) * c.du;
    const double v = c.v0 + ((bp + 1.0) * 0.5) * c.dv;
    X = (float)(((u - a.g.cx) * depth) / a.g.focal);
    Y = (float)(-(((v - a.g.cy) * depth) / a.g.focal));
    Z = (float)(-depth);
  }
  float *o = a.out + 3 * t;
  o[0] = X, o[1] = Y, o[2] = Z;
}

PatchGeo patch_geo(const PatchCommon &c) { return {c.com, c.cube, c.cube_n, c.affine, c.status_in, c.focal, c.cx, c.cy}; }

template <int DT>
void patch_launch_dt(const PatchArgs &a, int interp, unsigned groups, hipStream_t s) {
  if (interp == TSDF_PATCH_BILINEAR) hipLaunchKernelGGL((tsdf_patch_kernel<DT, true>), dim3(groups), dim3(kPatchWG), 0, s, a);
  else hipLaunchKernelGGL((tsdf_patch_kernel<DT, false>), dim3(groups), dim3(kPatchWG), 0, s, a);
}

// the device, then the launch: `a` holds its source; the rest comes from the entries' common arguments
int patch_launch(PatchArgs &a, const PatchCommon &c, const PatchOut &o, float background, void *hip_stream) {
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  a.g = patch_geo(c);
  a.plan = patch_plan(o.S, o.dtype);
  a.items = (int64_t)c.n * a.plan.items;
  a.S = o.S, a.rS = 1.0 / (double)o.S, a.background = background, a.eps = c.eps;
  a.out = const_cast<void *>(o.patch), a.status = const_cast<int32_t *>(o.status);
  const unsigned groups = patch_groups(c.n, a.plan);
  const hipStream_t s = static_cast<hipStream_t>(hip_stream);
  if (o.dtype == TSDF_PATCH_F32) patch_launch_dt<0>(a, o.interp, groups, s);
  else if (o.dtype == TSDF_LOWP_F16) patch_launch_dt<TSDF_LOWP_F16>(a, o.interp, groups, s);
  else patch_launch_dt<TSDF_LOWP_BF16>(a, o.interp, groups, s);
  return launched();
}

template <typename Kernel>
int patch_label_launch(Kernel kernel, const PatchCommon &c, int J, const float *in, float *out, int32_t *valid,
                       int32_t *status, void *hip_stream) {
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  PatchLabelArgs a = {patch_geo(c), in, J, (int64_t)c.n * J, out, valid, status};
  const unsigned groups = (unsigned)((a.total + kPatchWG - 1) / kPatchWG);
  hipLaunchKernelGGL(kernel, dim3(groups), dim3(kPatchWG), 0, static_cast<hipStream_t>(hip_stream), a);
  return launched();
}

}  // namespace

extern "C" {

int tsdf_patch_version(void) { return TSDF_PATCH_VERSION; }

int tsdf_patch_plan(int S, int dtype, int *px_per_lane, int *rows_per_group, int *items_per_position) {
  if (patch_bad_size(S) || patch_bad_elem(dtype) || !px_per_lane || !rows_per_group || !items_per_position)
    return TSDF_ERR_INVALID_ARG;
  const PatchPlan p = patch_plan(S, dtype);
  *px_per_lane = p.px;
  *rows_per_group = p.rows;
  *items_per_position = p.items;
  return TSDF_OK;
}

int tsdf_patch_frames_hip(const void *d_frames, int frame_type, int shift, int64_t n_src, int H, int W,
                          const int64_t *d_index, const double *d_com, float cube, const float *d_cube,
                          const double *d_affine, const int32_t *d_status_in, int n, int S, int interp, int dtype,
                          float background, double focal, double cx, double cy, float invalid_eps, float trunc_voxels,
                          void *hip_stream, void *d_out_patch, int32_t *d_out_status) {
  // arguments first, then the device, then the launch
  const PatchCommon c = {d_com, cube, d_cube, d_affine, d_status_in, n, focal, cx, cy, invalid_eps, trunc_voxels};
  const PatchOut o = {S, interp, dtype, d_out_patch, d_out_status};
  const PatchDefect bad = patch_frames_defect(c, o, d_frames, frame_type, shift, n_src, H, W, d_index);
  if (bad != kPatchGood) return patch_status(bad);
  const bool u16 = frame_type == TSDF_LOCATE_U16;
  PatchArgs a = {};
  a.src = d_frames, a.n_src = n_src, a.H = H, a.W = W, a.crops = 0, a.u16 = u16 ? 1 : 0;
  a.scale = u16 ? 1.0f / (float)(1 << shift) : 1.0f;
  a.index = d_index;
  return patch_launch(a, c, o, background, hip_stream);
}

int tsdf_patch_crops_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                         int64_t n_src, const int64_t *d_index, const double *d_com, float cube, const float *d_cube,
                         const double *d_affine, const int32_t *d_status_in, int n, int S, int interp, int dtype,
                         float background, double focal, double cx, double cy, float invalid_eps, float trunc_voxels,
                         void *hip_stream, void *d_out_patch, int32_t *d_out_status) {
  const PatchCommon c = {d_com, cube, d_cube, d_affine, d_status_in, n, focal, cx, cy, invalid_eps, trunc_voxels};
  const PatchOut o = {S, interp, dtype, d_out_patch, d_out_status};
  const PatchDefect bad = patch_crops_defect(c, o, d_depth, depth_len, d_offsets, d_headers, n_src, d_index);
  if (bad != kPatchGood) return patch_status(bad);
  PatchArgs a = {};
  a.src = d_depth, a.offsets = d_offsets, a.headers = d_headers, a.depth_len = depth_len, a.n_src = n_src;
  a.crops = 1, a.u16 = 0, a.scale = 1.0f, a.index = d_index;
  return patch_launch(a, c, o, background, hip_stream);
}

int tsdf_patch_uvd_hip(const float *d_joints, const double *d_com, float cube, const float *d_cube,
                       const double *d_affine, const int32_t *d_status_in, int n, int J, double focal, double cx,
                       double cy, float invalid_eps, float trunc_voxels, void *hip_stream, float *d_out_uvd,
                       int32_t *d_out_valid, int32_t *d_out_status) {
  const PatchCommon c = {d_com, cube, d_cube, d_affine, d_status_in, n, focal, cx, cy, invalid_eps, trunc_voxels};
  const PatchDefect bad = patch_label_defect(c, J, d_joints, d_out_uvd, d_out_valid, d_out_status);
  if (bad != kPatchGood) return patch_status(bad);
  return patch_label_launch(tsdf_patch_uvd_kernel, c, J, d_joints, d_out_uvd, d_out_valid, d_out_status, hip_stream);
}

int tsdf_patch_joints_hip(const float *d_uvd, const double *d_com, float cube, const float *d_cube,
                          const double *d_affine, const int32_t *d_status_in, int n, int J, double focal, double cx,
                          double cy, float invalid_eps, float trunc_voxels, void *hip_stream, float *d_out_joints) {
  const PatchCommon c = {d_com, cube, d_cube, d_affine, d_status_in, n, focal, cx, cy, invalid_eps, trunc_voxels};
  const PatchDefect bad = patch_label_defect(c, J, d_uvd, d_out_joints, d_out_joints, d_out_joints);
  if (bad != kPatchGood) return patch_status(bad);
  return patch_label_launch(tsdf_patch_joints_kernel, c, J, d_uvd, d_out_joints, nullptr, nullptr, hip_stream);
}

}  // extern "C"
