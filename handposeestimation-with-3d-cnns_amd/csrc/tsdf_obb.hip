// tsdf_obb.hip — libtsdf_obb.so: per-frame principal-axis maps, float64[n][24], from the depth alone
// (include/tsdf_obb.h).
//
// A translation unit and a library of its own, next to libtsdf_hip.so and the four extensions (all frozen).  It takes the
// status codes and tsdf_cam from include/tsdf.h, the host preamble every library here has from device.inc and the header
// rule and default camera from prim.inc; nothing else of the product's .inc files is included, and there is no device global: the launch is self-contained.
//
// tsdf_obb_kernel: one workgroup of 1024 threads (16 wave64) per frame, a grid-stride loop over frames when n exceeds the
// grid.  Per frame:
//   1. the header rule (uniform); a bad frame's depth is not read;
//   2. pass 1 over the crop: wave <-> rows, lane <-> groups of four consecutive columns, one 16-byte load per group
//      through a vector type DECLARED 4-byte aligned (a crop of odd width leaves every later row and frame at 4-byte
//      alignment; gfx950 under HSA serves a global_load_dwordx4 at any 4-byte boundary, as tsdf_depth16_widen_kernel
//      relies on at 2 bytes), the W mod 4 last columns one by one.  The split is by COLUMN, never by address: which lane
//      adds which pixel, and in which order, is a function of the crop's shape alone, so a frame's bits do not depend on
//      where it lies in the batch.  Four accumulators per lane: the count and the sums of x, y, z in float64;
//   3. a butterfly over the wave (__shfl_xor 32, 16, 8, 4, 2, 1), the wave sums through LDS; every lane adds the 16 of
//      them in wave order, so all hold the same mean without a second barrier;
//   4. pass 2 (the crop now comes from L2): six accumulators per lane, the products of p - mu; the same butterfly, the
//      same LDS hand-over, summed in wave order by thread 0;
//   5. thread 0: cyclic Jacobi on the 3x3 covariance (scalars only, no indexed arrays: no scratch), the sort, the signs,
//      the map and its inverse, and 24 + 16 doubles and the status written with plain stores.
// No atomics, no communication between workgroups, two barriers per frame (pass 2's also keeps the next frame's wave sums
// from overwriting s_p1 while a lane still reads it).
// Arithmetic contract: include/tsdf_obb.h; compiled with -ffp-contract=off, fma only where __builtin_fma is written.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_obb.h"

namespace {

#include "device.inc"   // check_device, launched, misaligned: the host preamble of every library here
#include "prim.inc"     // kDefaultCam, header_ok

constexpr int kObbWG = 1024;              // threads per workgroup
constexpr int kObbWaves = kObbWG / 64;    // 16 wave64
constexpr int kObbMaxBlocks = 1 << 16;    // frames beyond the grid are reached by the grid-stride loop
constexpr int kObbSweeps = 12;

typedef float obb_f4 __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes on a 4-byte boundary

struct ObbArgs {
  const float *depth;
  int64_t depth_len;
  const int64_t *offsets;
  const int32_t *headers;
  int n;
  double focal, cx, cy;
  float eps;
  double *xforms;    // [n][24]
  double *moments;   // [n][16] or null
  int32_t *status;   // [n] or null
};

__device__ __forceinline__ bool finite64(double v) { return __builtin_fabs(v) < __builtin_inf(); }   // false for NaN

// the butterfly of the contract: every lane ends with the same sum
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) v = v + __shfl_xor(v, k, 64);
  return v;
}

// One pixel.  PASS 1: acc = {sum x, sum y, sum z}, cnt the count; PASS 2: acc = the six products of p - m.
template <int PASS>
__device__ __forceinline__ void obb_pixel(float d, int col, double yc, double F, double cx, float eps, double mx, double my,
                                          double mz, double (&acc)[6], int &cnt) {
  if (!(__builtin_fabsf(d) >= eps)) return;   // NaN is invalid
  const double d64 = (double)d;
  const double s = d64 / F;
  const double x = ((double)col - cx) * s;
  const double y = -(yc * s);
  const double z = -d64;
  if (PASS == 1) {
    cnt += 1;
    acc[0] = acc[0] + x;
    acc[1] = acc[1] + y;
    acc[2] = acc[2] + z;
  } else {
    const double qx = x - mx, qy = y - my, qz = z - mz;
    acc[0] = __builtin_fma(qx, qx, acc[0]);
    acc[1] = __builtin_fma(qx, qy, acc[1]);
    acc[2] = __builtin_fma(qx, qz, acc[2]);
    acc[3] = __builtin_fma(qy, qy, acc[3]);
    acc[4] = __builtin_fma(qy, qz, acc[4]);
    acc[5] = __builtin_fma(qz, qz, acc[5]);
  }
}

// One pass over a crop of bw x bh pixels at d: wave <-> rows, lane <-> column groups (see the contract's order).
template <int PASS>
__device__ __forceinline__ void obb_scan(const float *__restrict__ d, int bw, int bh, int left, int top, int wave, int lane,
                                         double F, double cx, double cy, float eps, double mx, double my, double mz,
                                         double (&acc)[6], int &cnt) {
  const int ngrp = bw >> 2, tail0 = ngrp << 2, ntail = bw - tail0;
  for (int r = wave; r < bh; r += kObbWaves) {
    const float *__restrict__ row = d + (int64_t)r * bw;
    const double yc = (double)(top + r) - cy;
    for (int g = lane; g < ngrp; g += 64) {
      const obb_f4 q = *reinterpret_cast<const obb_f4 *>(row + 4 * g);
      const int c0 = left + 4 * g;
      obb_pixel<PASS>(q.x, c0, yc, F, cx, eps, mx, my, mz, acc, cnt);
      obb_pixel<PASS>(q.y, c0 + 1, yc, F, cx, eps, mx, my, mz, acc, cnt);
      obb_pixel<PASS>(q.z, c0 + 2, yc, F, cx, eps, mx, my, mz, acc, cnt);
      obb_pixel<PASS>(q.w, c0 + 3, yc, F, cx, eps, mx, my, mz, acc, cnt);
    }
    if (lane < ntail) obb_pixel<PASS>(row[tail0 + lane], left + tail0 + lane, yc, F, cx, eps, mx, my, mz, acc, cnt);
  }
}

// One Jacobi rotation of the pair (p, q); r is the third index.  V's rows k = 0, 1, 2 hold columns p and q.
__device__ __forceinline__ void jacobi_rot(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p,
                                           double &v0q, double &v1p, double &v1q, double &v2p, double &v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double th2 = theta * theta;
  double t = 1.0 / (__builtin_fabs(theta) + __builtin_sqrt(th2 + 1.0));
  if (theta < 0.0) t = -t;
  const double t2 = t * t;
  const double c = 1.0 / __builtin_sqrt(t2 + 1.0);
  const double s = t * c;
  const double tp = t * apq;
  app = app - tp;
  aqq = aqq + tp;
  apq = 0.0;
  const double rp = arp, rq = arq;
  const double crp = c * rp, srq = s * rq, srp = s * rp, crq = c * rq;
  arp = crp - srq;
  arq = srp + crq;
#define OBB_ROT_V(vp, vq)                              \
  {                                                    \
    const double a_ = vp, b_ = vq;                     \
    const double ca_ = c * a_, sb_ = s * b_;           \
    const double sa_ = s * a_, cb_ = c * b_;           \
    vp = ca_ - sb_;                                    \
    vq = sa_ + cb_;                                    \
  }
  OBB_ROT_V(v0p, v0q)
  OBB_ROT_V(v1p, v1q)
  OBB_ROT_V(v2p, v2q)
#undef OBB_ROT_V
}

__device__ __forceinline__ void swap2(double &a, double &b) {
  const double t = a;
  a = b;
  b = t;
}

// {A_i0, A_i1, A_i2, m_i - A_i . m}
__device__ __forceinline__ void obb_row(double *o, double a0, double a1, double a2, double mi, double mx, double my,
                                        double mz) {
  const double p2 = a2 * mz;
  o[0] = a0;
  o[1] = a1;
  o[2] = a2;
  o[3] = mi - __builtin_fma(a0, mx, __builtin_fma(a1, my, p2));
}

__device__ void obb_identity(double *xf, double *mo, double cnt) {
#pragma unroll
  for (int k = 0; k < 24; ++k) xf[k] = (k % 12) % 5 == 0 ? 1.0 : 0.0;   // rows {1,0,0,0}, {0,1,0,0}, {0,0,1,0}, twice
  if (mo) {
    mo[0] = cnt;
#pragma unroll
    for (int k = 1; k < 16; ++k) mo[k] = 0.0;
  }
}

__global__ __launch_bounds__(kObbWG) void tsdf_obb_kernel(ObbArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_p1[kObbWaves][4];   // per wave: N, sum x, sum y, sum z
  __shared__ double s_p2[kObbWaves][6];   // per wave: the six sums of products

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double F = a.focal, cx = a.cx, cy = a.cy;
  const float eps = a.eps;

  for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
    double *xf = a.xforms + 24 * i;
    double *mo = a.moments ? a.moments + 16 * i : nullptr;

    // the voxelizer's header rule; a bad frame's depth is not read
    const int32_t *hd = a.headers + 6 * i;
    const int left = hd[2], top = hd[3], right = hd[4], bottom = hd[5];
    const int64_t off0 = a.offsets[i], off1 = a.offsets[i + 1];
    const int64_t depth_len = a.depth_len;
    if (!header_ok(left, top, right, bottom, off0, off1, depth_len)) {   // (uniform)
      if (tid == 0) {
        obb_identity(xf, mo, 0.0);
        if (a.status) a.status[i] = TSDF_FRAME_BAD_HEADER;
      }
      continue;
    }
    const int bw = right - left, bh = bottom - top;   // header_ok: both are positive ints
    const float *__restrict__ d = a.depth + off0;

    // pass 1: the count and the sum of the points
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int cnt = 0;
    obb_scan<1>(d, bw, bh, left, top, wave, lane, F, cx, cy, eps, 0.0, 0.0, 0.0, acc, cnt);
    {
      const double wn = wave_sum((double)cnt), wx = wave_sum(acc[0]), wy = wave_sum(acc[1]), wz = wave_sum(acc[2]);
      if (lane == 0) {
        s_p1[wave][0] = wn;
        s_p1[wave][1] = wx;
        s_p1[wave][2] = wy;
        s_p1[wave][3] = wz;
      }
    }
    __syncthreads();
    double N = s_p1[0][0], sx = s_p1[0][1], sy = s_p1[0][2], sz = s_p1[0][3];   // every lane: the same bits
#pragma unroll
    for (int w = 1; w < kObbWaves; ++w) {
      N = N + s_p1[w][0];
      sx = sx + s_p1[w][1];
      sy = sy + s_p1[w][2];
      sz = sz + s_p1[w][3];
    }
    const double mx = sx / N, my = sy / N, mz = sz / N;
    if (!(N >= 3.0) || !finite64(mx) || !finite64(my) || !finite64(mz)) {   // (uniform)
      if (tid == 0) {
        obb_identity(xf, mo, N);
        if (a.status) a.status[i] = TSDF_FRAME_DEGENERATE;
      }
      __syncthreads();   // the next frame writes s_p1: not before every lane has read this frame's
      continue;
    }

    // pass 2: the products about the mean
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] = 0.0;
    obb_scan<2>(d, bw, bh, left, top, wave, lane, F, cx, cy, eps, mx, my, mz, acc, cnt);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double wv = wave_sum(acc[k]);
      if (lane == 0) s_p2[wave][k] = wv;
    }
    __syncthreads();
    if (tid != 0) continue;   // (thread 0 reaches the next frame's first barrier only after it has read s_p2)

    double cxx = s_p2[0][0], cxy = s_p2[0][1], cxz = s_p2[0][2], cyy = s_p2[0][3], cyz = s_p2[0][4], czz = s_p2[0][5];
#pragma unroll
    for (int w = 1; w < kObbWaves; ++w) {
      cxx = cxx + s_p2[w][0];
      cxy = cxy + s_p2[w][1];
      cxz = cxz + s_p2[w][2];
      cyy = cyy + s_p2[w][3];
      cyz = cyz + s_p2[w][4];
      czz = czz + s_p2[w][5];
    }
    cxx = cxx / N;
    cxy = cxy / N;
    cxz = cxz / N;
    cyy = cyy / N;
    cyz = cyz / N;
    czz = czz / N;
    const double trace = (cxx + cyy) + czz;
    if (!finite64(cxx) || !finite64(cxy) || !finite64(cxz) || !finite64(cyy) || !finite64(cyz) || !finite64(czz) ||
        trace == 0.0) {
      obb_identity(xf, mo, N);
      if (a.status) a.status[i] = TSDF_FRAME_DEGENERATE;
      continue;
    }

    // cyclic Jacobi: a = the working matrix, v = the eigenvectors as columns
    double a00 = cxx, a01 = cxy, a02 = cxz, a11 = cyy, a12 = cyz, a22 = czz;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    const double lim = 0x1p-53 * trace, lim2 = lim * lim;
    for (int sweep = 0; sweep < kObbSweeps; ++sweep) {
      const double o01 = a01 * a01, o02 = a02 * a02, o12 = a12 * a12;
      const double off = (o01 + o02) + o12;
      if (off <= lim2) break;
      jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0,1), r = 2
      jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0,2), r = 1
      jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1,2), r = 0
    }
    // descending, ties keep their order: exchanges (0,1), (1,2), (0,1)
    if (a11 > a00) {
      swap2(a00, a11);
      swap2(v00, v01);
      swap2(v10, v11);
      swap2(v20, v21);
    }
    if (a22 > a11) {
      swap2(a11, a22);
      swap2(v01, v02);
      swap2(v11, v12);
      swap2(v21, v22);
    }
    if (a11 > a00) {
      swap2(a00, a11);
      swap2(v00, v01);
      swap2(v10, v11);
      swap2(v20, v21);
    }
    // e1 = column 0, e3 = column 2, their signs; e2 = e3 x e1
    double e1x = v00, e1y = v10, e1z = v20, e3x = v02, e3y = v12, e3z = v22;
    if (e1y < 0.0) {
      e1x = -e1x;
      e1y = -e1y;
      e1z = -e1z;
    }
    if (e3z < 0.0) {
      e3x = -e3x;
      e3y = -e3y;
      e3z = -e3z;
    }
    const double p0 = e3y * e1z, p1 = e3z * e1y, p2 = e3z * e1x, p3 = e3x * e1z, p4 = e3x * e1y, p5 = e3y * e1x;
    const double e2x = p0 - p1, e2y = p2 - p3, e2z = p4 - p5;

    obb_row(xf + 0, e1x, e1y, e1z, mx, mx, my, mz);
    obb_row(xf + 4, e2x, e2y, e2z, my, mx, my, mz);
    obb_row(xf + 8, e3x, e3y, e3z, mz, mx, my, mz);
    obb_row(xf + 12, e1x, e2x, e3x, mx, mx, my, mz);   // the inverse: A^T and mu - A^T mu
    obb_row(xf + 16, e1y, e2y, e3y, my, mx, my, mz);
    obb_row(xf + 20, e1z, e2z, e3z, mz, mx, my, mz);
    if (mo) {
      mo[0] = N;
      mo[1] = mx;
      mo[2] = my;
      mo[3] = mz;
      mo[4] = cxx;
      mo[5] = cxy;
      mo[6] = cxz;
      mo[7] = cyy;
      mo[8] = cyz;
      mo[9] = czz;
      mo[10] = a00;
      mo[11] = a11;
      mo[12] = a22;
      mo[13] = 0.0;
      mo[14] = 0.0;
      mo[15] = 0.0;
    }
    if (a.status) a.status[i] = TSDF_FRAME_OK;
  }
}

}  // namespace

extern "C" {

int tsdf_obb_version(void) { return TSDF_OBB_VERSION; }

int tsdf_obb_xforms_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers, int n,
                        const tsdf_cam *cam, void *hip_stream, double *d_out_xforms, double *d_out_moments,
                        int32_t *d_out_status) {
  // arguments first, then the device, then the launch
  if (n < 0) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_depth || !d_offsets || !d_headers || !d_out_xforms || depth_len < 0) return TSDF_ERR_INVALID_ARG;
  if (misaligned(d_out_xforms, 7) || misaligned(d_out_moments, 7) || misaligned(d_out_status, 3)) return TSDF_ERR_INVALID_ARG;
  if (!cam_ok(cam)) return TSDF_ERR_INVALID_ARG;
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  if (!cam) cam = &kDefaultCam;
  ObbArgs a;
  a.depth = d_depth;
  a.depth_len = depth_len;
  a.offsets = d_offsets;
  a.headers = d_headers;
  a.n = n;
  a.focal = cam->focal;
  a.cx = cam->cx;
  a.cy = cam->cy;
  a.eps = cam->invalid_eps;
  a.xforms = d_out_xforms;
  a.moments = d_out_moments;
  a.status = d_out_status;
  const int blocks = n < kObbMaxBlocks ? n : kObbMaxBlocks;
  hipLaunchKernelGGL(tsdf_obb_kernel, dim3((unsigned)blocks), dim3(kObbWG), 0, static_cast<hipStream_t>(hip_stream), a);
  return launched();
}

}  // extern "C"
