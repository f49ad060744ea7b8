// tsdf_heatmap.hip — libtsdf_heatmap.so: per-joint Gaussian heatmap volumes from normalised labels, and per joint the
// peak of a volume back as normalised coordinates (include/tsdf_heatmap.h).
//
// A translation unit and a library of its own, next to libtsdf_hip.so and the other extension libraries (all frozen).  It
// takes the status codes and the layout enum from include/tsdf.h, the 2-byte dtype enum from include/tsdf_lowp.h, the host
// preamble every library here has from device.inc, the store side from narrow.inc (the float32 volume leaves through
// the same 16-byte store) and its argument rules, its plan and its item arithmetic from heatmap_host.inc, plain C++ that
// is also built on its own under the CPU sanitizers.  No device global, no atomics: every launch is self-contained.
//
// tsdf_heat_encode_kernel: store-bound.  units x nslab workgroups of 256 threads; a workgroup owns `slab` consecutive
// slices of the slowest axis of one (frame, joint) volume (heatmap_host.inc::heat_plan).  It
//   1. reads the joint's three coordinates and the frame's status (uniform) and tabulates g_x, g_y, g_z as float64 in LDS
//      (3 x R x 8 bytes): at most two exp per thread.  An invalid joint's tables are zero, so its volume is +0 by the
//      flush rule without a path of its own; workgroup 0 of the pair writes `valid`;
//   2. walks its slab in items of V consecutive voxels of the fastest axis, numbered in output order so that a wave
//      writes contiguous memory: V = 4 for float32, V = 8 for a 2-byte dtype when R % 8 == 0, else 4.  Item -> (slice,
//      row, column) is two multiply-shifts (heat_item).  Per voxel: one float64 multiply with the row's hoisted
//      g_z * g_y under czyx — under cxyz the row shares g_x, which the contract multiplies in LAST, so there it is two —,
//      the flush test, a conversion, and the item leaves as ONE 16-byte store (8 bytes for V = 4 of a 2-byte dtype).
// All output indexing is in 64 bits.
//
// tsdf_heat_decode_kernel: read-bound.  One workgroup of 256 threads per (frame, joint): 16-byte loads, four in flight
// per lane, a running (value, lowest index) per lane, a butterfly over the wave, one combine of the four waves through
// LDS; the first wave then sums the (2r+1)^3 window (at most 343 terms, float64) and lane 0 writes the 3 + 1 + 1 results.
// A lane meets its elements in rising index order and takes a new one only on `>` (a lane that found nothing above -inf
// looks once more for its first -inf), the combine prefers the lower index on equal values: the result is the lowest
// index of the maximum whatever the split.
// Compiled with -ffp-contract=off.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_heatmap.h"

namespace {

#include "device.inc"         // check_device, device_cus, launched, misaligned, bad_res: the host preamble of every library here
#include "narrow.inc"         // narrow2, store_vol, Piece, bad_dtype: the 2-byte store side
#include "heatmap_host.inc"   // heat_defect_*, heat_plan, heat_item: argument rules, plan and item arithmetic

constexpr int kHeatWG = 256;   // threads per workgroup of both kernels (4 wave64)

struct HeatEncArgs {
  const float *u;           // [units][3]
  const int32_t *status;    // [n] or null
  int J, R, slab, nslab;
  unsigned magic_rv, magic_r;
  double k;                 // 1 / (2 sigma^2)
  void *out;                // [units][R][R][R]
  int32_t *valid;           // [units] or null
};

// DT: 0 float32, TSDF_LOWP_F16, TSDF_LOWP_BF16; V voxels per lane and item
template <int LAYOUT, int DT, int V>
__global__ __launch_bounds__(kHeatWG) void tsdf_heat_encode_kernel(HeatEncArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_g[3][kHeatMaxR];   // g_x, g_y, g_z

  const int tid = threadIdx.x;
  const int R = a.R, RV = R / V;
  const unsigned unit = blockIdx.x / (unsigned)a.nslab;
  const int s = (int)(blockIdx.x - unit * (unsigned)a.nslab);
  const int sb = s * a.slab, se = sb + a.slab < R ? sb + a.slab : R;

  const float *uj = a.u + 3 * (int64_t)unit;
  const float u0 = uj[0], u1 = uj[1], u2 = uj[2];
  bool ok = __builtin_isfinite(u0) && __builtin_isfinite(u1) && __builtin_isfinite(u2);   // (uniform)
  if (a.status && a.status[unit / (unsigned)a.J] != 0) ok = false;
  for (int e = tid; e < 3 * R; e += kHeatWG) {
    const int axis = e >= 2 * R ? 2 : e >= R ? 1 : 0, i = e - axis * R;
    double g = 0.0;
    if (ok) {
      const double c = (double)(axis == 0 ? u0 : axis == 1 ? u1 : u2) * (double)R - 0.5;
      const double t = (double)i - c;
      g = exp(-((t * t) * a.k));
    }
    s_g[axis][i] = g;
  }
  if (s == 0 && tid == 0 && a.valid) a.valid[unit] = ok ? 1 : 0;
  __syncthreads();

  constexpr int kSlow = LAYOUT == 0 ? 2 : 0, kFast = LAYOUT == 0 ? 0 : 2;   // czyx: slices of z, x fastest; cxyz: the reverse
  constexpr int kBytes = DT == 0 ? 4 : 2;
  char *out = static_cast<char *>(a.out) + (int64_t)unit * R * R * R * kBytes;
  const unsigned nit = (unsigned)((se - sb) * R * RV);
  for (unsigned item = tid; item < nit; item += kHeatWG) {
    const HeatItem it = heat_item(item, R, RV, V, a.magic_rv, a.magic_r);
    const int sl = sb + it.slice;
    const double gs = s_g[kSlow][sl], gy = s_g[1][it.mid];
    const double zy = gs * gy;   // czyx: g_z * g_y, the row's
    float f[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double gf = s_g[kFast][it.fast + j];
      const double p = LAYOUT == 0 ? zy * gf : (gf * gy) * gs;   // (g_z * g_y) * g_x in both
      f[j] = p < 0x1p-126 ? 0.f : (float)p;
    }
    const int64_t e = ((int64_t)sl * R + it.mid) * R + it.fast;
    if constexpr (DT == 0) {
      static_assert(V == 4, "a float32 item is four voxels");
      const lowp_u4 o = {__builtin_bit_cast(unsigned, f[0]), __builtin_bit_cast(unsigned, f[1]),
                         __builtin_bit_cast(unsigned, f[2]), __builtin_bit_cast(unsigned, f[3])};
      store_vol((GlobalOut)(out + e * 4), o);
    } else {
      typename Piece<V>::type o;
#pragma unroll
      for (int j = 0; j < V / 2; ++j) o[j] = narrow2<DT == TSDF_LOWP_BF16>(f[2 * j], f[2 * j + 1]);
      store_vol((GlobalOut)(out + e * 2), o);
    }
  }
}

template <int LAYOUT>
void launch_encode(const HeatEncArgs &a, int dtype, int64_t blocks, hipStream_t s) {
  const dim3 g((unsigned)blocks), b(kHeatWG);
  if (dtype == TSDF_HEATMAP_F32) {
    hipLaunchKernelGGL((tsdf_heat_encode_kernel<LAYOUT, 0, 4>), g, b, 0, s, a);
  } else if (dtype == TSDF_LOWP_F16) {
    if (a.R % 8 == 0) hipLaunchKernelGGL((tsdf_heat_encode_kernel<LAYOUT, TSDF_LOWP_F16, 8>), g, b, 0, s, a);
    else hipLaunchKernelGGL((tsdf_heat_encode_kernel<LAYOUT, TSDF_LOWP_F16, 4>), g, b, 0, s, a);
  } else {
    if (a.R % 8 == 0) hipLaunchKernelGGL((tsdf_heat_encode_kernel<LAYOUT, TSDF_LOWP_BF16, 8>), g, b, 0, s, a);
    else hipLaunchKernelGGL((tsdf_heat_encode_kernel<LAYOUT, TSDF_LOWP_BF16, 4>), g, b, 0, s, a);
  }
}

struct HeatDecArgs {
  const void *heat;   // [units][R][R][R]
  int R, radius;
  float *u;           // [units][3]
  float *peak;        // [units] or null
  int32_t *arg;       // [units] or null
};

// element e of a 16-byte piece, widened exactly
template <int DT>
__device__ __forceinline__ float heat_widen(const lowp_u4 &q, int e) {
  if constexpr (DT == 0) {
    const unsigned w = q[e];   // (a copy: __builtin_bit_cast of the vector's element itself reads element 0)
    return __builtin_bit_cast(float, w);
  } else {
    const unsigned h = (q[e >> 1] >> (16 * (e & 1))) & 0xffffu;
    if constexpr (DT == TSDF_LOWP_BF16) return __builtin_bit_cast(float, h << 16);
    else return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
  }
}

// one element of the volume, widened exactly
template <int DT>
__device__ __forceinline__ float heat_at(const void *vol, int idx) {
  if constexpr (DT == 0) {
    return static_cast<const float *>(vol)[idx];
  } else {
    const unsigned h = static_cast<const unsigned short *>(vol)[idx];
    if constexpr (DT == TSDF_LOWP_BF16) return __builtin_bit_cast(float, h << 16);
    else return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
  }
}

// (v2, i2) replaces (v1, i1): an index < 0 is "none yet"; a held value is never a NaN
__device__ __forceinline__ bool heat_better(float v1, int i1, float v2, int i2) {
  return i2 >= 0 && (i1 < 0 || v2 > v1 || (v2 == v1 && i2 < i1));
}

template <int LAYOUT, int DT>
__global__ __launch_bounds__(kHeatWG) void tsdf_heat_decode_kernel(HeatDecArgs a) {
#pragma clang fp contract(off)
  constexpr int E = DT == 0 ? 4 : 8;     // elements of a 16-byte load
  constexpr int kDepth = 4;              // loads in flight per lane
  __shared__ float s_v[kHeatWG / 64];
  __shared__ int s_i[kHeatWG / 64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = a.R, R3 = R * R * R, nvec = R3 / E;   // R^3 is a multiple of 64
  const int64_t unit = blockIdx.x;
  const char *vol = static_cast<const char *>(a.heat) + unit * R3 * (DT == 0 ? 4 : 2);
  const lowp_u4 *__restrict__ pieces = reinterpret_cast<const lowp_u4 *>(vol);

  float best = -__builtin_inff();
  int bidx = -1;
  for (int v0 = tid; v0 < nvec; v0 += kDepth * kHeatWG) {
    lowp_u4 q[kDepth];
#pragma unroll
    for (int k = 0; k < kDepth; ++k) {
      const int vi = v0 + k * kHeatWG;
      const lowp_u4 none = {0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u};   // NaNs in all three types: never taken
      q[k] = vi < nvec ? pieces[vi] : none;
    }
#pragma unroll
    for (int k = 0; k < kDepth; ++k) {
      const int i0 = (v0 + k * kHeatWG) * E;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float h = heat_widen<DT>(q[k], e);
        if (h > best) {
          best = h;
          bidx = i0 + e;
        }
      }
    }
  }
  if (bidx < 0) {   // nothing above -inf among this lane's elements: its first -inf, if it has one, is its maximum
    for (int vi = tid; vi < nvec && bidx < 0; vi += kHeatWG) {
      const lowp_u4 q = pieces[vi];
#pragma unroll
      for (int e = E - 1; e >= 0; --e)
        if (heat_widen<DT>(q, e) == -__builtin_inff()) bidx = vi * E + e;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(best, off);
    const int oi = __shfl_xor(bidx, off);
    if (heat_better(best, bidx, ov, oi)) {
      best = ov;
      bidx = oi;
    }
  }
  if (lane == 0) {
    s_v[wave] = best;
    s_i[wave] = bidx;
  }
  __syncthreads();
  if (wave != 0) return;
  best = s_v[0], bidx = s_i[0];
#pragma unroll
  for (int w = 1; w < kHeatWG / 64; ++w) {
    const float ov = s_v[w];
    const int oi = s_i[w];
    if (heat_better(best, bidx, ov, oi)) {
      best = ov;
      bidx = oi;
    }
  }

  float *uo = a.u + 3 * unit;
  if (bidx < 0) {   // every value is a NaN (uniform)
    if (lane == 0) {
      uo[0] = uo[1] = uo[2] = 0.5f;
      if (a.peak) a.peak[unit] = __builtin_nanf("");
      if (a.arg) a.arg[unit] = -1;
    }
    return;
  }
  // the argmax voxel in memory order: slowest, middle, fastest axis
  const int is = bidx / (R * R), im = (bidx / R) % R, ifa = bidx % R;
  double cs = (double)is, cm = (double)im, cf = (double)ifa;
  const int r = a.radius;
  if (r > 0) {   // (uniform)
    const int ls = is - r > 0 ? is - r : 0, lm = im - r > 0 ? im - r : 0, lf = ifa - r > 0 ? ifa - r : 0;
    const int hs = is + r < R - 1 ? is + r : R - 1, hm = im + r < R - 1 ? im + r : R - 1, hf = ifa + r < R - 1 ? ifa + r : R - 1;
    const int nm = hm - lm + 1, nf = hf - lf + 1, total = (hs - ls + 1) * nm * nf;
    double sw = 0.0, ss = 0.0, sm = 0.0, sf = 0.0;
    for (int t = lane; t < total; t += 64) {
      const int ks = t / (nm * nf), km = (t / nf) % nm, kf = t % nf;
      const int js = ls + ks, jm = lm + km, jf = lf + kf;
      const float h = heat_at<DT>(vol, (js * R + jm) * R + jf);
      const double w = h > 0.f ? (double)h : 0.0;   // max(h, 0); a NaN counts as 0
      sw += w;
      ss += w * (double)js;
      sm += w * (double)jm;
      sf += w * (double)jf;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      sw += __shfl_xor(sw, off);
      ss += __shfl_xor(ss, off);
      sm += __shfl_xor(sm, off);
      sf += __shfl_xor(sf, off);
    }
    if (sw > 0.0 && __builtin_isfinite(sw)) {
      cs = ss / sw;
      cm = sm / sw;
      cf = sf / sw;
    }
  }
  if (lane == 0) {
    const double Rd = (double)R;
    const float us = (float)((cs + 0.5) / Rd), um = (float)((cm + 0.5) / Rd), uf = (float)((cf + 0.5) / Rd);
    uo[0] = LAYOUT == 0 ? uf : us;   // x: the fastest axis under czyx, the slowest under cxyz
    uo[1] = um;
    uo[2] = LAYOUT == 0 ? us : uf;
    if (a.peak) a.peak[unit] = best;
    if (a.arg) a.arg[unit] = bidx;
  }
}

template <int LAYOUT>
void launch_decode(const HeatDecArgs &a, int dtype, int64_t units, hipStream_t s) {
  const dim3 g((unsigned)units), b(kHeatWG);
  if (dtype == TSDF_HEATMAP_F32) hipLaunchKernelGGL((tsdf_heat_decode_kernel<LAYOUT, 0>), g, b, 0, s, a);
  else if (dtype == TSDF_LOWP_F16) hipLaunchKernelGGL((tsdf_heat_decode_kernel<LAYOUT, TSDF_LOWP_F16>), g, b, 0, s, a);
  else hipLaunchKernelGGL((tsdf_heat_decode_kernel<LAYOUT, TSDF_LOWP_BF16>), g, b, 0, s, a);
}

}  // namespace

extern "C" {

int tsdf_heatmap_version(void) { return TSDF_HEATMAP_VERSION; }

int tsdf_joint_heatmaps_hip(const float *d_u, const int32_t *d_status, int n, int n_joints, int R, float sigma, int layout,
                            int dtype, void *hip_stream, void *d_out_heat, int32_t *d_out_valid) {
  // arguments first, then the device, then the launch
  const HeatDefect bad = heat_defect_encode(d_u, d_status, n, n_joints, R, sigma, layout, dtype, d_out_heat, d_out_valid);
  if (bad != kHeatGood) return heat_status(bad);
  const int cus = device_cus();
  if (cus < 0) return cus;
  const int64_t units = (int64_t)n * n_joints;
  const HeatPlan plan = heat_plan(units, R, cus);
  const int V = dtype != TSDF_HEATMAP_F32 && R % 8 == 0 ? 8 : 4;
  HeatEncArgs a;
  a.u = d_u;
  a.status = d_status;
  a.J = n_joints;
  a.R = R;
  a.slab = plan.slab;
  a.nslab = plan.nslab;
  a.magic_rv = heat_magic(R / V);
  a.magic_r = heat_magic(R);
  a.k = 1.0 / (2.0 * ((double)sigma * (double)sigma));
  a.out = d_out_heat;
  a.valid = d_out_valid;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  if (layout == TSDF_LAYOUT_CZYX) launch_encode<0>(a, dtype, plan.blocks, s);
  else launch_encode<1>(a, dtype, plan.blocks, s);
  return launched();
}

int tsdf_heatmap_joints_hip(const void *d_heat, int dtype, int n, int n_joints, int R, int layout, int radius,
                            void *hip_stream, float *d_out_u, float *d_out_peak, int32_t *d_out_arg) {
  // arguments first, then the device, then the launch
  const HeatDefect bad = heat_defect_decode(d_heat, dtype, n, n_joints, R, layout, radius, d_out_u, d_out_peak, d_out_arg);
  if (bad != kHeatGood) return heat_status(bad);
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  HeatDecArgs a;
  a.heat = d_heat;
  a.R = R;
  a.radius = radius;
  a.u = d_out_u;
  a.peak = d_out_peak;
  a.arg = d_out_arg;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const int64_t units = (int64_t)n * n_joints;
  if (layout == TSDF_LAYOUT_CZYX) launch_decode<0>(a, dtype, units, s);
  else launch_decode<1>(a, dtype, units, s);
  return launched();
}

}  // extern "C"
