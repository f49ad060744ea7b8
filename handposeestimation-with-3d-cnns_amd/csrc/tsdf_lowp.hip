// tsdf_lowp.hip — libtsdf_lowp.so: the plain voxel pass on a caller-supplied grid written as float16 / bfloat16 voxels, and
// the same narrowing for float32 values (include/tsdf_lowp.h).
//
// A translation unit and a library of its own, next to libtsdf_hip.so and the other extension libraries (all frozen).  It
// takes the status codes, tsdf_cam and the layout enum from include/tsdf.h, the host preamble every library here has
// from device.inc, the device primitives from prim.inc, the slab scaffold it shares with tsdf_auggrid.hip from
// slab.inc and the narrowing and the stores it shares with tsdf_maplowp.hip from narrow.inc; the product's plain voxel arithmetic (phase2.inc::voxel_values4 and the tables of frame.inc that feed
// it) is RESTATED here operation for operation, nothing else of the product's .inc files is included, and there is no
// device global: every launch is self-contained.
//
// tsdf_grid_lowp_kernel: n x ceil(R / slab) workgroups of 256 threads; a workgroup owns `slab` consecutive slices (indices
// of the slowest output axis) of one batch position.  It
//   1. resolves its source frame (the index, if any) and checks the frame's header and grid row (all uniform); a position
//      that is not OK has its slab zero-filled and workgroup 0 of the position writes the status;
//   2. tabulates per axis and grid index what depends on one grid index alone: the centre's coordinate and its pre-scaled
//      form for x and y, and for z the projection factor q = -F / v_z (the one true division, R per workgroup), the
//      pre-scaled centre and the float32 threshold of the sign test: 6.5 KiB of LDS whatever R is;
//   3. walks its slab in items of V consecutive voxels of the fastest axis (V = 8 when R % 8 == 0, else 4), one item per
//      lane and pass: the unfused pixel index, a plain global load of the gathered pixel (a crop is at most 300 KB and is
//      re-read by every slab of the frame: it is expected to be served by L2), the z distance, and — only in a wave that
//      holds a voxel within the truncation distance along z — the x / y terms; the 3 x V float32 values are narrowed
//      pairwise in registers and leave as ONE 16-byte store per channel (V = 4: one 8-byte store).  Items are numbered in
//      output order, so a wave writes one contiguous KiB per channel, as the float32 kernels do with 4 voxels a lane.
// No LDS staging of the crop, no work queue, no communication between workgroups, no atomics.
// Compiled with -ffp-contract=off, fma only where __builtin_fma is written.
//
// The stores: the volume is written once and never re-read here, so it goes out non-temporal ("nt").  Measured for THIS
// kernel on one MI355X (tools/bench_lowp.py --lib, one build per policy, bfloat16; 1024 crops 32^3 / 16 crops 32^3 / 256
// crops 64^3, us per launch): "nt" 98.2 / 9.5 / 109.6, the product's "sc1 nt" 104.1 / 9.9 / 114.2, "sc0 sc1 nt" 104.0 /
// 9.4 / 112.8, no bits 100.0 / 9.5 / 144.6 — the device scope that pays for the product's float32 stores costs 4-6 %
// here.  -DTSDF_LOWP_STORE_ASM='"..."' selects other bits.  All stores are vector stores.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_lowp.h"

namespace {

#include "device.inc"   // check_device, launched, misaligned: the host preamble of every library here
#include "prim.inc"     // kDefaultCam, trunc_i32, finite32, f32_round_up, header_ok
#include "slab.inc"     // workgroup <-> slab, the frame's header and grid row, zero-fill, host sizing
#include "narrow.inc"   // narrow2, store_vol, Piece, bad_dtype: the 2-byte store side, shared with tsdf_maplowp.hip

constexpr int kNarrowMaxBlocks = 1 << 16;   // the narrowing kernel strides over anything larger

typedef float lowp_f4 __attribute__((ext_vector_type(4)));

struct LowpArgs {
  SlabSrc src;
  double inv_focal;
  float eps;
  const float *grid;        // [n_src][8]
  uint16_t *out;            // [n][3][R][R][R]
  int32_t *status;          // [n] or null
};

// V = voxels per lane and item (8: 16-byte stores, 4: 8-byte stores)
template <int LAYOUT, bool BF16, int V>
__global__ __launch_bounds__(kSlabWG) void tsdf_grid_lowp_kernel(LowpArgs a) {
#pragma clang fp contract(off)
  typedef typename Piece<V>::type piece;
  __shared__ double s_vx[kSlabMaxR], s_vxs[kSlabMaxR];     // v_x, v_x * it
  __shared__ double s_nvy[kSlabMaxR], s_vys[kSlabMaxR];    // -v_y, v_y * it
  __shared__ double s_q[kSlabMaxR], s_vzs[kSlabMaxR];      // -F / v_z, v_z * it
  __shared__ float s_neg[kSlabMaxR];                       // f32_round_up(-v_z)

  const int tid = threadIdx.x;
  const int R = a.src.R, RV = R / V;
  const Slab blk = slab_of_block(a.src.nslab, a.src.slab, R);
  const int sb = blk.sb, se = blk.se;
  const int64_t R3 = (int64_t)R * R * R;
  uint16_t *__restrict__ out = a.out + blk.i * 3 * R3;

  const SlabFrame fr = slab_head<true>(a.src, blk, a.grid);
  const int left = fr.left, top = fr.top, right = fr.right, bottom = fr.bottom;
  const int64_t bw = fr.bw;
  const float ox = fr.ox, oy = fr.oy, oz = fr.oz, vl = fr.vl, td = fr.td;
  // R * R is a multiple of 16
  if (slab_bad_frame<lowp_u4>(fr, blk, a.status, out, R, (int64_t)(se - sb) * R * R / 8, tid)) return;

  // per-frame constants (frame.inc::make_voxk) and per-axis tables (frame.inc::fill_tables)
  const double F = a.src.focal, cx = a.src.cx, cy = a.src.cy;
  const double it = 1.0 / (double)td;
  const double kq = a.inv_focal * it;
  for (int e = tid; e < 3 * R; e += kSlabWG) {
    const int ax = e / R, idx = e - ax * R;
    const float o = ax == 0 ? ox : ax == 1 ? oy : oz;
    const double prod = (double)idx * (double)vl;
    const double v = (double)o + prod;                        // v_a
    const double vs = v * it;
    if (ax == 0) {
      s_vx[idx] = v;
      s_vxs[idx] = vs;
    } else if (ax == 1) {
      s_nvy[idx] = -v;
      s_vys[idx] = vs;
    } else {
      s_q[idx] = -F / v;                                      // IEEE division
      s_vzs[idx] = vs;
      s_neg[idx] = f32_round_up(-v);                          // pd < -v_z  <=>  w_z > v_z
    }
  }
  const float eps = a.eps;
  const float *__restrict__ d = a.src.depth + fr.off0;
  __syncthreads();

  const int nit = (se - sb) * R * RV;
  for (int item = tid; item < nit; item += kSlabWG) {
    const int fv = (item % RV) * V;
    const int t1 = item / RV;
    const int y = t1 % R, sl = sb + t1 / R;
    const double nvy = s_nvy[y], vys = s_vys[y];
    // ---- project the V voxels and gather their depths ----
    int px[V], py[V];
    float pd[V];
    bool inb[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int xi = LAYOUT == 0 ? fv + j : sl, zi = LAYOUT == 0 ? sl : fv + j;
      const double q = s_q[zi];
      const double mx = s_vx[xi] * q, my = nvy * q;
      px[j] = trunc_i32(mx + cx);
      py[j] = trunc_i32(my + cy);
      inb[j] = px[j] >= left && px[j] < right && py[j] >= top && py[j] < bottom;
      const int64_t at = inb[j] ? (int64_t)(py[j] - top) * bw + (px[j] - left) : 0;   // the load is always in bounds
      pd[j] = d[at];
    }
    // ---- z first: rejected voxels are 0, voxels beyond the truncation distance along z alone are +-1 ----
    double pd64[V], tz[V];
    float sv[V];
    bool any_near = false;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int zi = LAYOUT == 0 ? sl : fv + j;
      const bool ok = inb[j] & (__builtin_fabsf(pd[j]) >= eps);   // NaN is invalid
      pd64[j] = (double)pd[j];
      tz[j] = __builtin_fma(pd64[j], it, s_vzs[zi]);
      const bool neg = pd[j] < s_neg[zi];
      any_near |= ok & (__builtin_fabs(tz[j]) <= 1.0);
      sv[j] = ok ? (neg ? -1.0f : 1.0f) : 0.0f;
    }
    float v0[V], v1[V], v2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) v0[j] = v1[j] = v2[j] = sv[j];
    if (__any(any_near)) {
      // otherwise every voxel of this wave is rejected or has |tz| > 1, so dist^2 >= tz^2 > 1: (+-1, +-1, +-1)
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int xi = LAYOUT == 0 ? fv + j : sl;
        const double aq = pd64[j] * kq;
        const double dxi = (double)px[j] - cx, dyi = (double)py[j] - cy;
        const double tx = __builtin_fma(-dxi, aq, s_vxs[xi]);
        const double ty = __builtin_fma(dyi, aq, vys);
        const double xx = tx * tx;
        const double s = __builtin_fma(tz[j], tz[j], __builtin_fma(ty, ty, xx));
        const bool nearv = s <= 1.0;
        // |t| clamped to 1, float32; times sv = +-1 or 0: exact, and the sign lands on a zero too
        const float m0 = __builtin_fminf(__builtin_fabsf((float)tx), 1.0f);
        const float m1 = __builtin_fminf(__builtin_fabsf((float)ty), 1.0f);
        const float m2 = __builtin_fminf(__builtin_fabsf((float)tz[j]), 1.0f);
        v0[j] = nearv ? m0 * sv[j] : sv[j];
        v1[j] = nearv ? m1 * sv[j] : sv[j];
        v2[j] = nearv ? m2 * sv[j] : sv[j];
      }
    }
    // ---- narrow pairwise, one store per channel ----
    piece o0, o1, o2;
#pragma unroll
    for (int j = 0; j < V / 2; ++j) {
      o0[j] = narrow2<BF16>(v0[2 * j], v0[2 * j + 1]);
      o1[j] = narrow2<BF16>(v1[2 * j], v1[2 * j + 1]);
      o2[j] = narrow2<BF16>(v2[2 * j], v2[2 * j + 1]);
    }
    const int64_t e = ((int64_t)sl * R + y) * R + fv;   // o[c][slow][y][fast]
    store_vol((GlobalOut)(out + e), o0);
    store_vol((GlobalOut)(out + R3 + e), o1);
    store_vol((GlobalOut)(out + 2 * R3 + e), o2);
  }
}

struct NarrowArgs {
  const float *in;
  int64_t count;
  uint16_t *out;
};

// 8 elements per lane and step: two 16-byte loads, one 16-byte store; the last count % 8 elements one by one
template <bool BF16>
__global__ __launch_bounds__(kSlabWG) void tsdf_lowp_narrow_kernel(NarrowArgs a) {
  const int64_t n8 = a.count >> 3;
  const int64_t step = (int64_t)gridDim.x * kSlabWG;
  const lowp_f4 *__restrict__ in4 = reinterpret_cast<const lowp_f4 *>(a.in);
  lowp_u4 *__restrict__ out4 = reinterpret_cast<lowp_u4 *>(a.out);
  for (int64_t k = (int64_t)blockIdx.x * kSlabWG + threadIdx.x; k < n8; k += step) {
    const lowp_f4 lo = in4[2 * k], hi = in4[2 * k + 1];
    lowp_u4 o;
    o.x = narrow2<BF16>(lo.x, lo.y);
    o.y = narrow2<BF16>(lo.z, lo.w);
    o.z = narrow2<BF16>(hi.x, hi.y);
    o.w = narrow2<BF16>(hi.z, hi.w);
    out4[k] = o;
  }
  const int64_t t = (n8 << 3) + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 8 && t < a.count) a.out[t] = (uint16_t)narrow2<BF16>(a.in[t], 0.0f);
}

template <int LAYOUT, bool BF16>
void launch_grid(const LowpArgs &a, int64_t blocks, hipStream_t s) {
  if (a.src.R % 8 == 0)
    hipLaunchKernelGGL((tsdf_grid_lowp_kernel<LAYOUT, BF16, 8>), dim3((unsigned)blocks), dim3(kSlabWG), 0, s, a);
  else
    hipLaunchKernelGGL((tsdf_grid_lowp_kernel<LAYOUT, BF16, 4>), dim3((unsigned)blocks), dim3(kSlabWG), 0, s, a);
}

}  // namespace

extern "C" {

int tsdf_lowp_version(void) { return TSDF_LOWP_VERSION; }

int tsdf_voxelize_grid_lowp_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                                int64_t n_src, const int64_t *d_index, int n, int R, const tsdf_cam *cam, int layout,
                                int dtype, void *hip_stream, const float *d_grid, void *d_out_tsdf, int32_t *d_out_status) {
  // arguments first, then the device, then the launch
  if (n < 0) return TSDF_ERR_INVALID_ARG;
  if (slab_bad_shape(R, layout)) return TSDF_ERR_INVALID_ARG;
  if (bad_dtype(dtype)) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_grid || !d_out_tsdf || misaligned(d_out_tsdf, 15)) return TSDF_ERR_INVALID_ARG;
  SlabPlan plan;
  if (!slab_args_ok(d_depth, depth_len, d_offsets, d_headers, n_src, d_index, n, R, R % 8 == 0 ? 8 : 4, cam, plan))
    return TSDF_ERR_INVALID_ARG;
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  if (!cam) cam = &kDefaultCam;
  LowpArgs a;
  a.src = slab_src(d_depth, depth_len, d_offsets, d_headers, n_src, d_index, n, R, *cam, plan);
  a.inv_focal = 1.0 / cam->focal;
  a.eps = cam->invalid_eps;
  a.grid = d_grid;
  a.out = static_cast<uint16_t *>(d_out_tsdf);
  a.status = d_out_status;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const bool bf = dtype == TSDF_LOWP_BF16;
  if (layout == TSDF_LAYOUT_CZYX) {
    if (bf) launch_grid<0, true>(a, plan.blocks, s);
    else launch_grid<0, false>(a, plan.blocks, s);
  } else {
    if (bf) launch_grid<1, true>(a, plan.blocks, s);
    else launch_grid<1, false>(a, plan.blocks, s);
  }
  return launched();
}

int tsdf_lowp_narrow_hip(const float *d_in, int64_t count, int dtype, void *hip_stream, void *d_out) {
  if (count < 0 || bad_dtype(dtype)) return TSDF_ERR_INVALID_ARG;
  if (count == 0) return TSDF_OK;
  if (!d_in || !d_out || misaligned(d_in, 15) || misaligned(d_out, 15)) return TSDF_ERR_INVALID_ARG;
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  NarrowArgs a;
  a.in = d_in;
  a.count = count;
  a.out = static_cast<uint16_t *>(d_out);
  int64_t blocks = ((count >> 3) + kSlabWG - 1) / kSlabWG;
  if (blocks < 1) blocks = 1;
  if (blocks > kNarrowMaxBlocks) blocks = kNarrowMaxBlocks;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  if (dtype == TSDF_LOWP_BF16)
    hipLaunchKernelGGL(tsdf_lowp_narrow_kernel<true>, dim3((unsigned)blocks), dim3(kSlabWG), 0, s, a);
  else
    hipLaunchKernelGGL(tsdf_lowp_narrow_kernel<false>, dim3((unsigned)blocks), dim3(kSlabWG), 0, s, a);
  return launched();
}

}  // extern "C"
