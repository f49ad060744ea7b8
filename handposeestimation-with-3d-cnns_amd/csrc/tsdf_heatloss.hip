// tsdf_heatloss.hip — libtsdf_heatloss.so: the squared error of a predicted heatmap volume against the Gaussian target of
// its label without that target in memory, a soft-argmax over the softmax of a whole volume, and the gradient of each
// (include/tsdf_heatloss.h).
//
// A translation unit and a library of its own, next to libtsdf_hip.so and the other extension libraries (all frozen).  It
// takes the status codes and the layout enum from include/tsdf.h, the dtype codes from include/tsdf_lowp.h and
// include/tsdf_heatmap.h, the host preamble every library here has from device.inc, the store side from narrow.inc, the
// shape rules, the slab plan and the item arithmetic from heatmap_host.inc as they are, and its own argument rules and the
// forward kernels' coordinate arithmetic from heatloss_host.inc, plain C++ that is also built on its own under the CPU
// sanitizers.  heat_widen and the table fill are restated from tsdf_heatmap.hip, which is frozen.  No device global, no
// atomics: every launch is self-contained.
//
// The two forward kernels (tsdf_heat_sse_kernel, tsdf_soft_argmax_kernel) are read-bound reductions after the decode
// kernel: one workgroup of 256 threads per (frame, joint), 16-byte loads, four in flight per lane, float64 accumulators per
// lane (one; four), a __shfl_xor butterfly over the wave, one combine of the four waves through LDS in the order
// ((w0 + w1) + w2) + w3, and thread 0 writes the unit's results.  A lane meets its pieces in rising order and a piece's
// elements in rising order, so the order of every sum is a function of R, dtype and layout alone.  Coordinates are formed
// per group of four elements (heat_quad): an 8-element piece of a 2-byte volume straddles rows when R % 8 != 0.  The
// soft-argmax takes the maximum in a sweep of its own and reads the volume a second time for the sums.
//
// The two gradient kernels (tsdf_heat_sse_grad_kernel, tsdf_soft_argmax_grad_kernel) are elementwise after the encode
// kernel: units x nslab workgroups (heat_plan), items of V voxels of the fastest axis numbered in memory order
// (heat_item), per item ONE 16-byte load and ONE 16-byte store (8 bytes each for V = 4 of a 2-byte dtype).  A lane reads
// its item before it writes it and touches no other, which is what makes out == in legal.  All volume indexing is in 64 bits.
// Compiled with -ffp-contract=off.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_heatloss.h"

namespace {

#include "device.inc"          // check_device, device_cus, launched, misaligned, bad_res: the host preamble of every library here
#include "narrow.inc"          // narrow2, store_vol, Piece, bad_dtype: the 2-byte store side
#include "heatmap_host.inc"    // HeatDefect, heat_defect_shape, heat_status, heat_plan, heat_item, heat_magic, kHeatMaxR
#include "heatloss_host.inc"   // heat_defect_sse ... heat_defect_soft_argmax_grad, heat_quad

constexpr int kLossWG = 256;    // threads per workgroup of all four kernels (4 wave64)
constexpr int kLossDepth = 4;   // 16-byte loads in flight per lane in the forward kernels

// element e of a piece of 32-bit words, widened exactly (tsdf_heatmap.hip's, for a piece of either width)
template <int DT, typename P>
__device__ __forceinline__ float heat_widen(const P &q, int e) {
  if constexpr (DT == 0) {
    const unsigned w = q[e];   // (a copy: __builtin_bit_cast of the vector's element itself reads element 0)
    return __builtin_bit_cast(float, w);
  } else {
    const unsigned h = (q[e >> 1] >> (16 * (e & 1))) & 0xffffu;
    if constexpr (DT == TSDF_LOWP_BF16) return __builtin_bit_cast(float, h << 16);
    else return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
  }
}

// The encode kernel's table fill, operation for operation: g[a][i] = exp(-((t * t) * k)), t = i - ((double)u_a * R - 0.5),
// zero tables for an invalid unit.  Returns the unit's validity (uniform); the caller places the barrier.
__device__ __forceinline__ bool heat_fill_gauss(double (*s_g)[kHeatMaxR], const float *u, const int32_t *status, unsigned unit,
                                                int J, int R, double k, int tid) {
#pragma clang fp contract(off)
  const float *uj = u + 3 * (int64_t)unit;
  const float u0 = uj[0], u1 = uj[1], u2 = uj[2];
  bool ok = __builtin_isfinite(u0) && __builtin_isfinite(u1) && __builtin_isfinite(u2);
  if (status && status[unit / (unsigned)J] != 0) ok = false;
  for (int e = tid; e < 3 * R; e += kLossWG) {
    const int axis = e >= 2 * R ? 2 : e >= R ? 1 : 0, i = e - axis * R;
    double g = 0.0;
    if (ok) {
      const double c = (double)(axis == 0 ? u0 : axis == 1 ? u1 : u2) * (double)R - 0.5;
      const double t = (double)i - c;
      g = exp(-((t * t) * k));
    }
    s_g[axis][i] = g;
  }
  return ok;
}

// the encode's float32 target of one voxel: (g_z * g_y) * g_x in both layouts, flushed below 2^-126.  gs, gy: the slowest
// and the middle axis' factors, zy = gs * gy, gf the fastest axis'
template <int LAYOUT>
__device__ __forceinline__ float heat_target(double gs, double gy, double zy, double gf) {
#pragma clang fp contract(off)
  const double p = LAYOUT == 0 ? zy * gf : (gf * gy) * gs;
  return p < 0x1p-126 ? 0.f : (float)p;
}

// the sum of a per-lane float64 over the wave, the same bits in every lane
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// ---------------------------------------------------------------------------------------------------------- loss, forward
struct SseArgs {
  const void *pred;         // [units][R][R][R]
  const float *u;           // [units][3]
  const int32_t *status;    // [n] or null
  int J, R;
  unsigned magic_rq, magic_r;
  double k;                 // 1 / (2 sigma^2)
  double *sse;              // [units]
  int32_t *valid;           // [units] or null
};

template <int LAYOUT, int DT>
__global__ __launch_bounds__(kLossWG) void tsdf_heat_sse_kernel(SseArgs a) {
#pragma clang fp contract(off)
  constexpr int E = DT == 0 ? 4 : 8;   // elements of a 16-byte load
  constexpr int kSlow = LAYOUT == 0 ? 2 : 0, kFast = LAYOUT == 0 ? 0 : 2;
  __shared__ double s_g[3][kHeatMaxR];   // g_x, g_y, g_z
  __shared__ double s_w[kLossWG / 64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = a.R, R3 = R * R * R, nvec = R3 / E;   // R^3 is a multiple of 64
  const unsigned unit = blockIdx.x;
  const bool ok = heat_fill_gauss(s_g, a.u, a.status, unit, a.J, R, a.k, tid);
  if (!ok) {   // (uniform) the prediction is not read
    if (tid == 0) {
      a.sse[unit] = 0.0;
      if (a.valid) a.valid[unit] = 0;
    }
    return;
  }
  __syncthreads();

  const char *vol = static_cast<const char *>(a.pred) + (int64_t)unit * R3 * (DT == 0 ? 4 : 2);
  const lowp_u4 *__restrict__ pieces = reinterpret_cast<const lowp_u4 *>(vol);
  double acc = 0.0;
  for (int v0 = tid; v0 < nvec; v0 += kLossDepth * kLossWG) {
    lowp_u4 q[kLossDepth];
#pragma unroll
    for (int k = 0; k < kLossDepth; ++k) {
      const int vi = v0 + k * kLossWG;
      const lowp_u4 none = {0u, 0u, 0u, 0u};
      q[k] = vi < nvec ? pieces[vi] : none;
    }
#pragma unroll
    for (int k = 0; k < kLossDepth; ++k) {
      const int vi = v0 + k * kLossWG;
      if (vi >= nvec) break;
#pragma unroll
      for (int h = 0; h < E / 4; ++h) {
        const HeatQuad c = heat_quad((unsigned)(vi * (E / 4) + h), R, a.magic_rq, a.magic_r);
        const double gs = s_g[kSlow][c.slow], gy = s_g[1][c.mid];
        const double zy = gs * gy;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float t32 = heat_target<LAYOUT>(gs, gy, zy, s_g[kFast][c.fast + j]);
          const double d = (double)heat_widen<DT>(q[k], 4 * h + j) - (double)t32;
          acc += d * d;
        }
      }
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) s_w[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    a.sse[unit] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
    if (a.valid) a.valid[unit] = 1;
  }
}

template <int LAYOUT>
void launch_sse(const SseArgs &a, int dtype, int64_t units, hipStream_t s) {
  const dim3 g((unsigned)units), b(kLossWG);
  if (dtype == TSDF_HEATMAP_F32) hipLaunchKernelGGL((tsdf_heat_sse_kernel<LAYOUT, 0>), g, b, 0, s, a);
  else if (dtype == TSDF_LOWP_F16) hipLaunchKernelGGL((tsdf_heat_sse_kernel<LAYOUT, TSDF_LOWP_F16>), g, b, 0, s, a);
  else hipLaunchKernelGGL((tsdf_heat_sse_kernel<LAYOUT, TSDF_LOWP_BF16>), g, b, 0, s, a);
}

// --------------------------------------------------------------------------------------------------------- loss, gradient
// an item of V voxels as it is loaded and stored: 16 bytes, or 8 for four 2-byte voxels
template <int DT, int V>
struct LossPiece {
  typedef typename Piece<DT == 0 ? 8 : V>::type type;
};

// V float32 leave as one item of the output volume at byte address p
template <int DT, int V>
__device__ __forceinline__ void store_item(char *p, const float (&f)[V]) {
  typename LossPiece<DT, V>::type o;
  if constexpr (DT == 0) {
    static_assert(V == 4, "a float32 item is four voxels");
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = __builtin_bit_cast(unsigned, f[j]);
  } else {
#pragma unroll
    for (int j = 0; j < V / 2; ++j) o[j] = narrow2<DT == TSDF_LOWP_BF16>(f[2 * j], f[2 * j + 1]);
  }
  store_vol((GlobalOut)p, o);
}

struct SseGradArgs {
  const void *pred;         // [units][R][R][R]
  const float *u;           // [units][3]
  const int32_t *status;    // [n] or null
  const float *w;           // [units]
  int J, R, slab, nslab;
  unsigned magic_rv, magic_r;
  double k;                 // 1 / (2 sigma^2)
  void *out;                // [units][R][R][R]; may be pred
};

// DT: 0 float32, TSDF_LOWP_F16, TSDF_LOWP_BF16; V voxels per lane and item
template <int LAYOUT, int DT, int V>
__global__ __launch_bounds__(kLossWG) void tsdf_heat_sse_grad_kernel(SseGradArgs a) {
#pragma clang fp contract(off)
  constexpr int kSlow = LAYOUT == 0 ? 2 : 0, kFast = LAYOUT == 0 ? 0 : 2;
  constexpr int kBytes = DT == 0 ? 4 : 2;
  typedef typename LossPiece<DT, V>::type PieceT;
  __shared__ double s_g[3][kHeatMaxR];   // g_x, g_y, g_z

  const int tid = threadIdx.x;
  const int R = a.R, RV = R / V;
  const unsigned unit = blockIdx.x / (unsigned)a.nslab;
  const int s = (int)(blockIdx.x - unit * (unsigned)a.nslab);
  const int sb = s * a.slab, se = sb + a.slab < R ? sb + a.slab : R;
  const bool ok = heat_fill_gauss(s_g, a.u, a.status, unit, a.J, R, a.k, tid);   // (uniform)
  const double wd = ok ? (double)a.w[unit] : 0.0;
  __syncthreads();

  const int64_t base = (int64_t)unit * R * R * R * kBytes;
  const char *in = static_cast<const char *>(a.pred) + base;
  char *out = static_cast<char *>(a.out) + base;
  const unsigned nit = (unsigned)((se - sb) * R * RV);
  for (unsigned item = tid; item < nit; item += kLossWG) {
    const HeatItem it = heat_item(item, R, RV, V, a.magic_rv, a.magic_r);
    const int sl = sb + it.slice;
    const int64_t e = (((int64_t)sl * R + it.mid) * R + it.fast) * kBytes;
    float f[V];
    if (ok) {
      const PieceT q = *reinterpret_cast<const PieceT *>(in + e);
      const double gs = s_g[kSlow][sl], gy = s_g[1][it.mid];
      const double zy = gs * gy;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float t32 = heat_target<LAYOUT>(gs, gy, zy, s_g[kFast][it.fast + j]);
        const double d = (double)heat_widen<DT>(q, j) - (double)t32;
        f[j] = (float)(wd * d);
      }
    } else {   // +0 whatever w holds; the prediction is not read
#pragma unroll
      for (int j = 0; j < V; ++j) f[j] = 0.f;
    }
    store_item<DT, V>(out + e, f);
  }
}

// the ten instantiations of a gradient kernel: 2 layouts x (float32, and 2 dtypes x {8, 4} voxels a lane)
#define TSDF_LOSS_LAUNCH_GRAD(KERNEL, ARGS)                                                                  \
  do {                                                                                                       \
    if (dtype == TSDF_HEATMAP_F32) {                                                                         \
      hipLaunchKernelGGL((KERNEL<LAYOUT, 0, 4>), g, b, 0, s, ARGS);                                          \
    } else if (dtype == TSDF_LOWP_F16) {                                                                     \
      if (ARGS.R % 8 == 0) hipLaunchKernelGGL((KERNEL<LAYOUT, TSDF_LOWP_F16, 8>), g, b, 0, s, ARGS);         \
      else hipLaunchKernelGGL((KERNEL<LAYOUT, TSDF_LOWP_F16, 4>), g, b, 0, s, ARGS);                         \
    } else {                                                                                                 \
      if (ARGS.R % 8 == 0) hipLaunchKernelGGL((KERNEL<LAYOUT, TSDF_LOWP_BF16, 8>), g, b, 0, s, ARGS);        \
      else hipLaunchKernelGGL((KERNEL<LAYOUT, TSDF_LOWP_BF16, 4>), g, b, 0, s, ARGS);                        \
    }                                                                                                        \
  } while (0)

template <int LAYOUT>
void launch_sse_grad(const SseGradArgs &a, int dtype, int64_t blocks, hipStream_t s) {
  const dim3 g((unsigned)blocks), b(kLossWG);
  TSDF_LOSS_LAUNCH_GRAD(tsdf_heat_sse_grad_kernel, a);
}

// --------------------------------------------------------------------------------------------------- soft-argmax, forward
struct SoftArgs {
  const void *heat;   // [units][R][R][R]
  int R;
  unsigned magic_rq, magic_r;
  double beta;
  float *u;           // [units][3]
  double *stats;      // [units][5]: m, Z, c_x, c_y, c_z
};

template <int LAYOUT, int DT>
__global__ __launch_bounds__(kLossWG) void tsdf_soft_argmax_kernel(SoftArgs a) {
#pragma clang fp contract(off)
  constexpr int E = DT == 0 ? 4 : 8;   // elements of a 16-byte load
  __shared__ float s_m[kLossWG / 64];
  __shared__ double s_w[4][kLossWG / 64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = a.R, R3 = R * R * R, nvec = R3 / E;   // R^3 is a multiple of 64
  const int64_t unit = blockIdx.x;
  const char *vol = static_cast<const char *>(a.heat) + unit * R3 * (DT == 0 ? 4 : 2);
  const lowp_u4 *__restrict__ pieces = reinterpret_cast<const lowp_u4 *>(vol);
  const lowp_u4 none = {0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u};   // NaNs in all three types: never taken

  // sweep 1: the maximum under `>` from -inf
  float best = -__builtin_inff();
  for (int v0 = tid; v0 < nvec; v0 += kLossDepth * kLossWG) {
    lowp_u4 q[kLossDepth];
#pragma unroll
    for (int k = 0; k < kLossDepth; ++k) {
      const int vi = v0 + k * kLossWG;
      q[k] = vi < nvec ? pieces[vi] : none;
    }
#pragma unroll
    for (int k = 0; k < kLossDepth; ++k) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float h = heat_widen<DT>(q[k], e);
        if (h > best) best = h;
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float o = __shfl_xor(best, off);
    if (o > best) best = o;
  }
  if (lane == 0) s_m[wave] = best;
  __syncthreads();
  best = s_m[0];
#pragma unroll
  for (int w = 1; w < kLossWG / 64; ++w)
    if (s_m[w] > best) best = s_m[w];
  const double m = (double)best;

  // sweep 2: Z and the three first moments, by the slowest, the middle and the fastest axis
  double sz = 0.0, ss = 0.0, sm = 0.0, sf = 0.0;
  for (int v0 = tid; v0 < nvec; v0 += kLossDepth * kLossWG) {
    lowp_u4 q[kLossDepth];
#pragma unroll
    for (int k = 0; k < kLossDepth; ++k) {
      const int vi = v0 + k * kLossWG;
      q[k] = vi < nvec ? pieces[vi] : none;
    }
#pragma unroll
    for (int k = 0; k < kLossDepth; ++k) {
      const int vi = v0 + k * kLossWG;
      if (vi >= nvec) break;
#pragma unroll
      for (int h = 0; h < E / 4; ++h) {
        const HeatQuad c = heat_quad((unsigned)(vi * (E / 4) + h), R, a.magic_rq, a.magic_r);
        const double ds = (double)c.slow, dm = (double)c.mid;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double z = exp(a.beta * ((double)heat_widen<DT>(q[k], 4 * h + j) - m));
          sz += z;
          ss += z * ds;
          sm += z * dm;
          sf += z * (double)(c.fast + j);
        }
      }
    }
  }
  sz = wave_sum(sz);
  ss = wave_sum(ss);
  sm = wave_sum(sm);
  sf = wave_sum(sf);
  if (lane == 0) {
    s_w[0][wave] = sz;
    s_w[1][wave] = ss;
    s_w[2][wave] = sm;
    s_w[3][wave] = sf;
  }
  __syncthreads();
  if (tid == 0) {
    double t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = ((s_w[i][0] + s_w[i][1]) + s_w[i][2]) + s_w[i][3];
    const double Z = t[0], cs = t[1] / Z, cm = t[2] / Z, cf = t[3] / Z;
    const double cx = LAYOUT == 0 ? cf : cs, cz = LAYOUT == 0 ? cs : cf;   // x: the fastest axis under czyx, the slowest under cxyz
    const double Rd = (double)R;
    float *uo = a.u + 3 * unit;
    uo[0] = (float)((cx + 0.5) / Rd);
    uo[1] = (float)((cm + 0.5) / Rd);
    uo[2] = (float)((cz + 0.5) / Rd);
    double *st = a.stats + 5 * unit;
    st[0] = m;
    st[1] = Z;
    st[2] = cx;
    st[3] = cm;
    st[4] = cz;
  }
}

template <int LAYOUT>
void launch_soft(const SoftArgs &a, int dtype, int64_t units, hipStream_t s) {
  const dim3 g((unsigned)units), b(kLossWG);
  if (dtype == TSDF_HEATMAP_F32) hipLaunchKernelGGL((tsdf_soft_argmax_kernel<LAYOUT, 0>), g, b, 0, s, a);
  else if (dtype == TSDF_LOWP_F16) hipLaunchKernelGGL((tsdf_soft_argmax_kernel<LAYOUT, TSDF_LOWP_F16>), g, b, 0, s, a);
  else hipLaunchKernelGGL((tsdf_soft_argmax_kernel<LAYOUT, TSDF_LOWP_BF16>), g, b, 0, s, a);
}

// -------------------------------------------------------------------------------------------------- soft-argmax, gradient
struct SoftGradArgs {
  const void *heat;       // [units][R][R][R]
  const double *stats;    // [units][5]
  const float *gu;        // [units][3]
  int R, slab, nslab;
  unsigned magic_rv, magic_r;
  double beta;
  void *out;              // [units][R][R][R]; may be heat
};

template <int LAYOUT, int DT, int V>
__global__ __launch_bounds__(kLossWG) void tsdf_soft_argmax_grad_kernel(SoftGradArgs a) {
#pragma clang fp contract(off)
  constexpr int kSlow = LAYOUT == 0 ? 2 : 0, kFast = LAYOUT == 0 ? 0 : 2;
  constexpr int kBytes = DT == 0 ? 4 : 2;
  typedef typename LossPiece<DT, V>::type PieceT;
  __shared__ double s_t[3][kHeatMaxR];   // gu_a * (i - c_a) for a = x, y, z

  const int tid = threadIdx.x;
  const int R = a.R, RV = R / V;
  const unsigned unit = blockIdx.x / (unsigned)a.nslab;
  const int s = (int)(blockIdx.x - unit * (unsigned)a.nslab);
  const int sb = s * a.slab, se = sb + a.slab < R ? sb + a.slab : R;
  const double *st = a.stats + 5 * (int64_t)unit;
  const float *gu = a.gu + 3 * (int64_t)unit;
  const double m = st[0];
  const double kk = a.beta / (st[1] * (double)R);
  for (int e = tid; e < 3 * R; e += kLossWG) {
    const int axis = e >= 2 * R ? 2 : e >= R ? 1 : 0, i = e - axis * R;
    s_t[axis][i] = (double)gu[axis] * ((double)i - st[2 + axis]);
  }
  __syncthreads();

  const int64_t base = (int64_t)unit * R * R * R * kBytes;
  const char *in = static_cast<const char *>(a.heat) + base;
  char *out = static_cast<char *>(a.out) + base;
  const unsigned nit = (unsigned)((se - sb) * R * RV);
  for (unsigned item = tid; item < nit; item += kLossWG) {
    const HeatItem it = heat_item(item, R, RV, V, a.magic_rv, a.magic_r);
    const int sl = sb + it.slice;
    const int64_t e = (((int64_t)sl * R + it.mid) * R + it.fast) * kBytes;
    const PieceT q = *reinterpret_cast<const PieceT *>(in + e);
    const double ts = s_t[kSlow][sl], ty = s_t[1][it.mid];
    float f[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double tf = s_t[kFast][it.fast + j];
      const double sum = LAYOUT == 0 ? (tf + ty) + ts : (ts + ty) + tf;   // (x + y) + z in both
      const double z = exp(a.beta * ((double)heat_widen<DT>(q, j) - m));
      f[j] = (float)((z * kk) * sum);
    }
    store_item<DT, V>(out + e, f);
  }
}

template <int LAYOUT>
void launch_soft_grad(const SoftGradArgs &a, int dtype, int64_t blocks, hipStream_t s) {
  const dim3 g((unsigned)blocks), b(kLossWG);
  TSDF_LOSS_LAUNCH_GRAD(tsdf_soft_argmax_grad_kernel, a);
}

}  // namespace

extern "C" {

int tsdf_heatloss_version(void) { return TSDF_HEATLOSS_VERSION; }

int tsdf_heat_sse_hip(const void *d_pred, int dtype, const float *d_u, const int32_t *d_status, int n, int n_joints, int R,
                      float sigma, int layout, void *hip_stream, double *d_out_sse, int32_t *d_out_valid) {
  // arguments first, then the device, then the launch
  const HeatDefect bad = heat_defect_sse(d_pred, dtype, d_u, d_status, n, n_joints, R, sigma, layout, d_out_sse, d_out_valid);
  if (bad != kHeatGood) return heat_status(bad);
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  SseArgs a;
  a.pred = d_pred;
  a.u = d_u;
  a.status = d_status;
  a.J = n_joints;
  a.R = R;
  a.magic_rq = heat_magic(R / 4);
  a.magic_r = heat_magic(R);
  a.k = 1.0 / (2.0 * ((double)sigma * (double)sigma));
  a.sse = d_out_sse;
  a.valid = d_out_valid;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const int64_t units = (int64_t)n * n_joints;
  if (layout == TSDF_LAYOUT_CZYX) launch_sse<0>(a, dtype, units, s);
  else launch_sse<1>(a, dtype, units, s);
  return launched();
}

int tsdf_heat_sse_grad_hip(const void *d_pred, int dtype, const float *d_u, const int32_t *d_status, const float *d_w, int n,
                           int n_joints, int R, float sigma, int layout, void *hip_stream, void *d_out_grad) {
  const HeatDefect bad = heat_defect_sse_grad(d_pred, dtype, d_u, d_status, d_w, n, n_joints, R, sigma, layout, d_out_grad);
  if (bad != kHeatGood) return heat_status(bad);
  const int cus = device_cus();
  if (cus < 0) return cus;
  const int64_t units = (int64_t)n * n_joints;
  const HeatPlan plan = heat_plan(units, R, cus);
  const int V = dtype != TSDF_HEATMAP_F32 && R % 8 == 0 ? 8 : 4;
  SseGradArgs a;
  a.pred = d_pred;
  a.u = d_u;
  a.status = d_status;
  a.w = d_w;
  a.J = n_joints;
  a.R = R;
  a.slab = plan.slab;
  a.nslab = plan.nslab;
  a.magic_rv = heat_magic(R / V);
  a.magic_r = heat_magic(R);
  a.k = 1.0 / (2.0 * ((double)sigma * (double)sigma));
  a.out = d_out_grad;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  if (layout == TSDF_LAYOUT_CZYX) launch_sse_grad<0>(a, dtype, plan.blocks, s);
  else launch_sse_grad<1>(a, dtype, plan.blocks, s);
  return launched();
}

int tsdf_soft_argmax_hip(const void *d_heat, int dtype, int n, int n_joints, int R, float beta, int layout, void *hip_stream,
                         float *d_out_u, double *d_out_stats) {
  const HeatDefect bad = heat_defect_soft_argmax(d_heat, dtype, n, n_joints, R, beta, layout, d_out_u, d_out_stats);
  if (bad != kHeatGood) return heat_status(bad);
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  SoftArgs a;
  a.heat = d_heat;
  a.R = R;
  a.magic_rq = heat_magic(R / 4);
  a.magic_r = heat_magic(R);
  a.beta = (double)beta;
  a.u = d_out_u;
  a.stats = d_out_stats;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const int64_t units = (int64_t)n * n_joints;
  if (layout == TSDF_LAYOUT_CZYX) launch_soft<0>(a, dtype, units, s);
  else launch_soft<1>(a, dtype, units, s);
  return launched();
}

int tsdf_soft_argmax_grad_hip(const void *d_heat, int dtype, const double *d_stats, const float *d_grad_u, int n,
                              int n_joints, int R, float beta, int layout, void *hip_stream, void *d_out_grad) {
  const HeatDefect bad = heat_defect_soft_argmax_grad(d_heat, dtype, d_stats, d_grad_u, n, n_joints, R, beta, layout, d_out_grad);
  if (bad != kHeatGood) return heat_status(bad);
  const int cus = device_cus();
  if (cus < 0) return cus;
  const int64_t units = (int64_t)n * n_joints;
  const HeatPlan plan = heat_plan(units, R, cus);
  const int V = dtype != TSDF_HEATMAP_F32 && R % 8 == 0 ? 8 : 4;
  SoftGradArgs a;
  a.heat = d_heat;
  a.stats = d_stats;
  a.gu = d_grad_u;
  a.R = R;
  a.slab = plan.slab;
  a.nslab = plan.nslab;
  a.magic_rv = heat_magic(R / V);
  a.magic_r = heat_magic(R);
  a.beta = (double)beta;
  a.out = d_out_grad;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  if (layout == TSDF_LAYOUT_CZYX) launch_soft_grad<0>(a, dtype, plan.blocks, s);
  else launch_soft_grad<1>(a, dtype, plan.blocks, s);
  return launched();
}

}  // extern "C"
