// tsdf_occupancy.hip — libtsdf_occupancy.so: one-channel occupancy volumes on grids the caller places
// (include/tsdf_occupancy.h, which has the contract operation by operation).
//
// A translation unit and a library of its own, next to libtsdf_hip.so and the other libraries (all frozen).  It takes the
// status codes and the layout enum from include/tsdf.h, the element types from include/tsdf_heatmap.h, the host preamble
// every library here has from device.inc, cam_ok and header_ok from prim.inc, the store side from narrow.inc and its
// argument rules and its plan from occupancy_host.inc, plain C++ that is also built on its own under the CPU sanitizers.
// No device global and no global atomic: every launch is self-contained.
//
// tsdf_occupancy_kernel: a SCATTER, where every other volume here is a gather.  n x nslab workgroups of 512 threads; a
// workgroup owns `slab` consecutive slices of the slowest axis of one batch position (occupancy_host.inc::occ_plan) and
//   1. zeroes a bit mask of slab * R * R bits in LDS, bit order = the slab's output order;
//   2. goes over the WHOLE crop — wave <-> rows, lane <-> four consecutive columns as one 16-byte load on a 4-byte
//      boundary, the last bw % 4 columns one by one (the mapping of place.inc) — and per valid pixel runs the contract's
//      float64 arithmetic; a point whose slowest index falls into the slab ORs its bit into the mask's word in LDS
//      (ds_or_b32).  OR is commutative and idempotent: the mask does not depend on the order of arrival;
//   3. barrier;
//   4. expands the mask into 16-byte stores, 4 float32 or 8 two-byte voxels each.  The slab is one contiguous piece of
//      the output and R * R is a multiple of 16, so an item never straddles a mask word and needs no (slice, row,
//      column): item t is bits [V t, V t + V) and elements [V t, V t + V) of the slab.
// Every slab workgroup of a position re-reads its crop (from L2 after the first).  A position that is not OK skips step
// 2, so step 4 writes its zeros; the position's first workgroup writes the status.  All output indexing is in 64 bits.
// Compiled with -ffp-contract=off: no fma anywhere in this file.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_occupancy.h"

namespace {

#include "device.inc"           // check_device, launched, misaligned, bad_res: the host preamble of every library here
#include "prim.inc"             // cam_ok, finite32, header_ok
#include "narrow.inc"           // lowp_u4, store_vol, bad_dtype: the store side
#include "occupancy_host.inc"   // occ_defect, occ_plan, kOccWG: argument rules and plan

constexpr int kOccWaves = kOccWG / 64;

typedef float occ_f4 __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes on a 4-byte boundary

struct OccArgs {
  const float *depth;
  int64_t depth_len;
  const int64_t *offsets;   // [n_src + 1]
  const int32_t *headers;   // [n_src][6]
  int64_t n_src;
  const int64_t *index;     // [n] or null
  int R, slab, nslab;
  double focal, cx, cy;
  float eps;
  const double *xforms;     // [n][24] or null
  const float *max_l;       // [n]
  const float *mid_p;       // [n][3]
  void *out;                // [n][R][R][R]
  int32_t *status;          // [n] or null
};

// what a pixel needs of its position: the map's forward rows, the grid and the slab
struct OccFrame {
  double m[12];
  double ox, oy, oz, iv, Rd;
  int R, sb, se;
};

// one axis: the voxel index as a float64, or -1 when the point is outside
__device__ __forceinline__ double occ_axis(double o, double ori, double iv, double Rd) {
  const double s = (o - ori) * iv + 0.5;
  double k = __builtin_floor(s);
  if (k == -1.0 && s >= -0x1p-10) k = 0.0;            // the skin rule
  if (k == Rd && s <= Rd + 0x1p-10) k = Rd - 1.0;
  return k >= 0.0 && k < Rd ? k : -1.0;               // a NaN is outside
}

template <int LAYOUT, bool MAPPED>
__device__ __forceinline__ void occ_pixel(float d, int col, double yc, double F, double cx, float eps, const OccFrame &f,
                                          unsigned *mask) {
  if (!(__builtin_fabsf(d) >= eps)) return;   // NaN is invalid
  const double d64 = (double)d;
  const double q = d64 / F;                   // IEEE division
  const double px = q * ((double)col - cx);
  const double py = -(q * yc);
  const double pz = -d64;
  double o0 = px, o1 = py, o2 = pz;
  if constexpr (MAPPED) {
    o0 = (f.m[0] * px + f.m[1] * py) + (f.m[2] * pz + f.m[3]);
    o1 = (f.m[4] * px + f.m[5] * py) + (f.m[6] * pz + f.m[7]);
    o2 = (f.m[8] * px + f.m[9] * py) + (f.m[10] * pz + f.m[11]);
  }
  const double k0 = occ_axis(o0, f.ox, f.iv, f.Rd);
  const double k1 = occ_axis(o1, f.oy, f.iv, f.Rd);
  const double k2 = occ_axis(o2, f.oz, f.iv, f.Rd);
  if (k0 < 0.0 || k1 < 0.0 || k2 < 0.0) return;
  const int ix = (int)k0, iy = (int)k1, iz = (int)k2;   // each in [0, R)
  const int slow = LAYOUT == 0 ? iz : ix, fast = LAYOUT == 0 ? ix : iz;
  if (slow < f.sb || slow >= f.se) return;
  const unsigned bit = (unsigned)(((slow - f.sb) * f.R + iy) * f.R + fast);   // < slab * R * R <= 2^19
  atomicOr(&mask[bit >> 5], 1u << (bit & 31u));
}

// DT: 0 float32, TSDF_LOWP_F16, TSDF_LOWP_BF16
template <int LAYOUT, int DT, bool MAPPED>
__global__ __launch_bounds__(kOccWG) void tsdf_occupancy_kernel(OccArgs a) {
#pragma clang fp contract(off)
  extern __shared__ unsigned s_mask[];   // ceil(slab * R * R / 32) words

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = a.R;
  const unsigned i = blockIdx.x / (unsigned)a.nslab;
  const int s = (int)(blockIdx.x - i * (unsigned)a.nslab);
  const int sb = s * a.slab, se = sb + a.slab < R ? sb + a.slab : R;
  const int nbits = (se - sb) * R * R;   // a multiple of 16
  const int nwords = (nbits + 31) >> 5;
  for (int w = tid; w < nwords; w += kOccWG) s_mask[w] = 0u;

  // the source frame; outside the tables it is a bad header and nothing of it is read (everything here is uniform)
  const int64_t g = a.index ? a.index[i] : (int64_t)i;
  bool ok = g >= 0 && g < a.n_src;
  int left = 0, top = 0, right = 0, bottom = 0;
  int64_t off0 = 0;
  if (ok) {
    const int32_t *hd = a.headers + 6 * g;
    left = hd[2], top = hd[3], right = hd[4], bottom = hd[5];
    const int64_t off1 = a.offsets[g + 1], depth_len = a.depth_len;
    off0 = a.offsets[g];
    ok = header_ok(left, top, right, bottom, off0, off1, depth_len);
  }
  int status = ok ? TSDF_FRAME_OK : TSDF_FRAME_BAD_HEADER;
  OccFrame f;
  f.R = R, f.sb = sb, f.se = se, f.Rd = (double)R;
  if (ok) {
    // the glue: float32, one rounding per operation
    const float max_l = a.max_l[i];
    const float m0 = a.mid_p[3 * (int64_t)i], m1 = a.mid_p[3 * (int64_t)i + 1], m2 = a.mid_p[3 * (int64_t)i + 2];
    const float vl = __fdiv_rn(max_l, (float)R);
    const float half_l = __fdiv_rn(max_l, 2.0f), half_v = __fdiv_rn(vl, 2.0f);
    const float ox = __fadd_rn(__fsub_rn(m0, half_l), half_v);
    const float oy = __fadd_rn(__fsub_rn(m1, half_l), half_v);
    const float oz = __fadd_rn(__fsub_rn(m2, half_l), half_v);
    const bool usable = max_l > 0.f && vl > 0.f && finite32(max_l) && finite32(vl) && finite32(m0) && finite32(m1) &&
                        finite32(m2) && finite32(ox) && finite32(oy) && finite32(oz);
    if (!usable) status = TSDF_FRAME_DEGENERATE;
    f.ox = (double)ox, f.oy = (double)oy, f.oz = (double)oz;
    f.iv = 1.0 / (double)vl;
  }
  if (s == 0 && tid == 0 && a.status) a.status[i] = status;
  __syncthreads();   // the mask is zero before the first OR

  if (status == TSDF_FRAME_OK) {
    if constexpr (MAPPED) {
#pragma unroll
      for (int k = 0; k < 12; ++k) f.m[k] = a.xforms[24 * (int64_t)i + k];
    }
    const int bw = right - left, bh = bottom - top;   // header_ok: both are positive ints
    const float *__restrict__ d = a.depth + off0;
    const double F = a.focal, cx = a.cx, cy = a.cy;
    const float eps = a.eps;
    const int ngrp = bw >> 2, tail0 = ngrp << 2, ntail = bw - tail0;
    // gl lanes per row: the smallest power of two that holds the row's groups of four (4..64), so a wave takes 64 / gl
    // rows at a time (uniform)
    int sh = 6;
    while (sh > 2 && (1 << (sh - 1)) >= ngrp) --sh;
    const int gl = 1 << sh, rpw = 64 >> sh;
    const int sub = lane >> sh, gq = lane & (gl - 1);
    for (int r = wave * rpw + sub; r < bh; r += kOccWaves * rpw) {
      const float *__restrict__ row = d + (int64_t)r * bw;
      const double yc = (double)(top + r) - cy;
      for (int q = gq; q < ngrp; q += gl) {
        const occ_f4 v = *reinterpret_cast<const occ_f4 *>(row + 4 * q);
        const int c0 = left + 4 * q;
        occ_pixel<LAYOUT, MAPPED>(v.x, c0, yc, F, cx, eps, f, s_mask);
        occ_pixel<LAYOUT, MAPPED>(v.y, c0 + 1, yc, F, cx, eps, f, s_mask);
        occ_pixel<LAYOUT, MAPPED>(v.z, c0 + 2, yc, F, cx, eps, f, s_mask);
        occ_pixel<LAYOUT, MAPPED>(v.w, c0 + 3, yc, F, cx, eps, f, s_mask);
      }
      if (gq < ntail) occ_pixel<LAYOUT, MAPPED>(row[tail0 + gq], left + tail0 + gq, yc, F, cx, eps, f, s_mask);
    }
  }
  __syncthreads();   // every bit of the slab is in the mask

  constexpr int V = DT == 0 ? 4 : 8;       // voxels of a 16-byte store
  constexpr int kBytes = DT == 0 ? 4 : 2;
  char *out = static_cast<char *>(a.out) + ((int64_t)i * R * R * R + (int64_t)sb * R * R) * kBytes;
  const int nit = nbits / V;
  for (int item = tid; item < nit; item += kOccWG) {
    const unsigned b0 = (unsigned)item * V;
    const unsigned bits = s_mask[b0 >> 5] >> (b0 & 31u);   // V divides 32 and b0: the item's bits are in one word
    lowp_u4 o;
    if constexpr (DT == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (bits >> j) & 1u ? 0x3f800000u : 0u;
    } else {
      constexpr unsigned one = DT == TSDF_LOWP_BF16 ? 0x3f80u : 0x3c00u;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = ((bits >> (2 * j)) & 1u ? one : 0u) | ((bits >> (2 * j + 1)) & 1u ? one << 16 : 0u);
    }
    store_vol((GlobalOut)(out + (int64_t)item * 16), o);
  }
}

template <int LAYOUT, int DT>
void launch_mapped(const OccArgs &a, int64_t blocks, int lds, hipStream_t s) {
  const dim3 g((unsigned)blocks), b(kOccWG);
  if (a.xforms) hipLaunchKernelGGL((tsdf_occupancy_kernel<LAYOUT, DT, true>), g, b, (size_t)lds, s, a);
  else hipLaunchKernelGGL((tsdf_occupancy_kernel<LAYOUT, DT, false>), g, b, (size_t)lds, s, a);
}

template <int LAYOUT>
void launch_dtype(const OccArgs &a, int dtype, int64_t blocks, int lds, hipStream_t s) {
  if (dtype == TSDF_HEATMAP_F32) launch_mapped<LAYOUT, 0>(a, blocks, lds, s);
  else if (dtype == TSDF_LOWP_F16) launch_mapped<LAYOUT, TSDF_LOWP_F16>(a, blocks, lds, s);
  else launch_mapped<LAYOUT, TSDF_LOWP_BF16>(a, blocks, lds, s);
}

}  // namespace

extern "C" {

int tsdf_occupancy_version(void) { return TSDF_OCCUPANCY_VERSION; }

int tsdf_occupancy_plan(int R, int slab_hint, int *slab, int *nslab, int *lds_bytes) {
  if (bad_res(R) || slab_hint < 0 || !slab || !nslab || !lds_bytes) return TSDF_ERR_INVALID_ARG;
  const OccPlan p = occ_plan(R, slab_hint);
  *slab = p.slab;
  *nslab = p.nslab;
  *lds_bytes = p.lds_bytes;
  return TSDF_OK;
}

int tsdf_occupancy_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                       int64_t n_src, const int64_t *d_index, int n, int R, double focal, double cx, double cy,
                       float invalid_eps, float trunc_voxels, int layout, int dtype, int slab_hint, void *hip_stream,
                       const double *d_xforms, const float *d_max_l, const float *d_mid_p, void *d_out_occ,
                       int32_t *d_out_status) {
  // arguments first, then the device, then the launch
  const OccCall c = {d_depth, depth_len, d_offsets, d_headers, n_src, d_index, n, R, focal, cx, cy, invalid_eps,
                     trunc_voxels, layout, dtype, slab_hint, d_xforms, d_max_l, d_mid_p, d_out_occ};
  const OccDefect bad = occ_defect(c);
  if (bad != kOccGood) return occ_status(bad);
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  const OccPlan plan = occ_plan(R, slab_hint);
  OccArgs a;
  a.depth = d_depth;
  a.depth_len = depth_len;
  a.offsets = d_offsets;
  a.headers = d_headers;
  a.n_src = n_src;
  a.index = d_index;
  a.R = R;
  a.slab = plan.slab;
  a.nslab = plan.nslab;
  a.focal = focal;
  a.cx = cx;
  a.cy = cy;
  a.eps = invalid_eps;
  a.xforms = d_xforms;
  a.max_l = d_max_l;
  a.mid_p = d_mid_p;
  a.out = d_out_occ;
  a.status = d_out_status;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const int64_t blocks = (int64_t)n * plan.nslab;
  if (layout == TSDF_LAYOUT_CZYX) launch_dtype<0>(a, dtype, blocks, plan.lds_bytes, s);
  else launch_dtype<1>(a, dtype, blocks, plan.lds_bytes, s);
  return launched();
}

}  // extern "C"
