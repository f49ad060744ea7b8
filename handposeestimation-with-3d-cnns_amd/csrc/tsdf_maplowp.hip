// tsdf_maplowp.hip — libtsdf_maplowp.so: the grid placement under a per-frame map on its own, and the augmented voxel
// pass on a caller-supplied grid written as float16 / bfloat16 voxels (include/tsdf_maplowp.h).
//
// A translation unit and a library of its own, next to libtsdf_hip.so and the other extension libraries (all frozen).  It
// takes the status codes, tsdf_cam and the layout enum from include/tsdf.h, the dtype enum from include/tsdf_lowp.h, the
// host preamble every library here has from device.inc, the device primitives from prim.inc, the slab scaffold it shares
// with tsdf_auggrid.hip and tsdf_lowp.hip from slab.inc, the store side it shares with tsdf_lowp.hip from narrow.inc and
// the placement's arithmetic — the crop pass, the wave butterfly, the float32 glue and the degenerate rule — from
// place.inc, which it shares with tsdf_mapstep.hip.  The augmented voxel arithmetic — the per-axis table, the per-frame
// constants and the four-voxel chain — is mapvox.inc's, the text tsdf_auggrid.hip::tsdf_aug_grid_kernel runs too; nothing
// of the product's other .inc files is included, and there is no device global: every launch is self-contained.
//
// tsdf_map_place_kernel: one workgroup of 1024 threads (16 wave64) per batch position, a grid-stride loop over positions
// when n exceeds the grid — the shape of tsdf_obb_kernel.  Per position:
//   1. the source frame (the index, if any) and the header rule (uniform); a bad frame's depth is not read;
//   2. one pass over the crop (place.inc::place_crop): wave <-> rows, lane <-> groups of four consecutive columns, one
//      16-byte load per group through a vector type DECLARED 4-byte aligned, the W mod 4 last columns one by one.  A
//      row narrower than 129 columns needs 32 lanes or fewer, so a wave then takes 2, 4, 8 or 16 rows at a time (the
//      pass is bound by its float64 arithmetic: idle lanes are lost time).  Per valid pixel the IEEE division by the
//      focal length (the compiler's sequence: exact for every F), the back-projection, the three fused
//      rows of the forward map, three roundings to float32 and six running extremes per lane;
//   3. a butterfly over the wave, the wave extremes through LDS, and thread 0 takes the 16 of them, runs the float32 glue
//      and the degenerate rule (place.inc::place_glue) and writes the row, max_l, mid_p and the status with plain stores.
// Minimum and maximum are order-free, so any split of the pixels gives the same bits.  No atomics, no communication
// between workgroups, two barriers per position (the second keeps the next position's wave extremes out of s_red while
// thread 0 still reads it).
//
// tsdf_map_grid_lowp_kernel: n x ceil(R / slab) workgroups of 256 threads; a workgroup owns `slab` consecutive slices of
// one batch position.  It
//   1. resolves its source frame and checks the frame's header and the POSITION's grid row (all uniform); a position that
//      is not OK has its slab zero-filled and workgroup 0 of the position writes the status;
//   2. tabulates the per-axis terms (mapvox.inc::map_fill_tab: 3 x R entries of 32 bytes in LDS);
//   3. walks its slab in items of V consecutive voxels of the fastest axis (V = 8 when R % 8 == 0, else 4), one item per
//      lane and pass, as V / 4 quads: a quad projects its four voxels and issues their four gathers (always in bounds: a
//      rejected voxel reads the crop's first pixel) before the distance terms of the first one, then narrows its 3 x 4
//      float32 values pairwise into 2 dwords per channel.  Only the packed dwords of an earlier quad stay live while
//      the next one is computed; the item leaves as ONE 16-byte store per channel (V = 4: one 8-byte store).
// No LDS staging of the crop, no work queue, no communication between workgroups, no atomics.
// Compiled with -ffp-contract=off, fma only where __builtin_fma is written.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_maplowp.h"

namespace {

#include "device.inc"   // check_device, launched, misaligned: the host preamble of every library here
#include "prim.inc"     // kDefaultCam, trunc_i32, finite32, header_ok
#include "slab.inc"     // workgroup <-> slab, the frame's header and grid row, zero-fill, host sizing
#include "narrow.inc"   // narrow2, store_vol, Piece, bad_dtype: the 2-byte store side
#include "place.inc"    // place_crop, place_glue, Placed: the placement's arithmetic, shared with tsdf_mapstep.hip
#include "mapvox.inc"   // map_fill_tab, map_consts, map_quad: the mapped voxel arithmetic, shared with tsdf_auggrid.hip

constexpr int kPlaceWG = 1024;               // threads per workgroup of the placement
constexpr int kPlaceWaves = kPlaceWG / 64;   // 16 wave64
constexpr int kPlaceMaxBlocks = 1 << 16;     // positions beyond the grid are reached by the grid-stride loop

struct PlaceArgs {
  const float *depth;
  int64_t depth_len;
  const int64_t *offsets;   // [n_src + 1]
  const int32_t *headers;   // [n_src][6]
  int64_t n_src;
  const int64_t *index;     // [n] or null
  int n, R;
  double focal, cx, cy;
  float eps, trunc_vox;
  const double *xforms;     // [n][24]
  float *grid;              // [n][8]
  float *max_l;             // [n] or null
  float *mid_p;             // [n][3] or null
  int32_t *status;          // [n] or null
};

// what thread 0 writes for one position
__device__ __forceinline__ void place_write(const PlaceArgs &a, int64_t i, const Placed &p) {
  float *g = a.grid + 8 * i;
  g[0] = p.ox, g[1] = p.oy, g[2] = p.oz, g[3] = p.vl, g[4] = p.td, g[5] = 0.f, g[6] = 0.f, g[7] = 0.f;
  if (a.max_l) a.max_l[i] = p.max_l;
  if (a.mid_p) {
    float *m = a.mid_p + 3 * i;
    m[0] = p.m0, m[1] = p.m1, m[2] = p.m2;
  }
  if (a.status) a.status[i] = p.status;
}

__global__ __launch_bounds__(kPlaceWG) void tsdf_map_place_kernel(PlaceArgs a) {
#pragma clang fp contract(off)
  __shared__ float s_red[kPlaceWaves][8];   // per wave: min xyz, max xyz, any, pad

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double F = a.focal, cx = a.cx, cy = a.cy;
  const float eps = a.eps;

  for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
    // the source frame; outside the tables it is a bad header and nothing of it is read
    const int64_t g = a.index ? a.index[i] : i;
    bool ok = g >= 0 && g < a.n_src;   // (uniform)
    int left = 0, top = 0, right = 0, bottom = 0;
    int64_t off0 = 0;
    if (ok) {
      const int32_t *hd = a.headers + 6 * g;
      left = hd[2], top = hd[3], right = hd[4], bottom = hd[5];
      const int64_t off1 = a.offsets[g + 1], depth_len = a.depth_len;
      off0 = a.offsets[g];
      ok = header_ok(left, top, right, bottom, off0, off1, depth_len);
    }
    if (!ok) {
      if (tid == 0) place_write(a, i, place_none(TSDF_FRAME_BAD_HEADER));
      continue;
    }
    const int bw = right - left, bh = bottom - top;   // header_ok: both are positive ints
    const float *__restrict__ d = a.depth + off0;
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = a.xforms[24 * i + k];

    place_crop<kPlaceWaves>(d, left, top, bw, bh, F, cx, cy, eps, m, lane, wave, s_red);
    __syncthreads();
    if (tid == 0) place_write(a, i, place_glue<kPlaceWaves>(s_red, a.R, a.trunc_vox));
    __syncthreads();   // the next position writes s_red: not before thread 0 has read this one's
  }
}

struct MapLowpArgs {
  SlabSrc src;
  float eps;
  const double *xforms;     // [n][24]
  const float *grid;        // [n][8]
  uint16_t *out;            // [n][3][R][R][R]
  int32_t *status;          // [n] or null
};

// V = voxels per lane and item (8: 16-byte stores, 4: 8-byte stores)
template <int LAYOUT, bool BF16, int V>
__global__ __launch_bounds__(kSlabWG) void tsdf_map_grid_lowp_kernel(MapLowpArgs a) {
#pragma clang fp contract(off)
  typedef typename Piece<V>::type piece;
  __shared__ map_d4 s_tab[3][kSlabMaxR];

  const int tid = threadIdx.x;
  const int R = a.src.R, RV = R / V;
  const Slab blk = slab_of_block(a.src.nslab, a.src.slab, R);
  const int sb = blk.sb, se = blk.se;
  const int64_t R3 = (int64_t)R * R * R;
  uint16_t *__restrict__ out = a.out + blk.i * 3 * R3;

  const SlabFrame fr = slab_head<false>(a.src, blk, a.grid);   // the grid row is the POSITION's
  // R * R is a multiple of 16
  if (slab_bad_frame<lowp_u4>(fr, blk, a.status, out, R, (int64_t)(se - sb) * R * R / 8, tid)) return;

  const double *__restrict__ xf = a.xforms + 24 * blk.i;
  map_fill_tab(s_tab, xf, fr.ox, fr.oy, fr.oz, fr.vl, R, tid);
  const MapK k = map_consts(xf, a.src, a.eps, fr);
  const float *__restrict__ d = a.src.depth + fr.off0;
  __syncthreads();

  const int nit = (se - sb) * R * RV;
  for (int item = tid; item < nit; item += kSlabWG) {
    const int fv = (item % RV) * V;
    const int t1 = item / RV;
    const int y = t1 % R, sl = sb + t1 / R;
    const map_d4 ty = s_tab[1][y];
    const map_d4 ts = s_tab[LAYOUT == 0 ? 2 : 0][sl];        // the slice's axis: z (czyx) or x (cxyz)
    piece o0, o1, o2;
#pragma unroll
    for (int h = 0; h < V / 4; ++h) {
      float v0[4], v1[4], v2[4];
      map_quad<LAYOUT>(s_tab, k, d, ty, ts, fv + 4 * h, v0, v1, v2);
      o0[2 * h] = narrow2<BF16>(v0[0], v0[1]);
      o0[2 * h + 1] = narrow2<BF16>(v0[2], v0[3]);
      o1[2 * h] = narrow2<BF16>(v1[0], v1[1]);
      o1[2 * h + 1] = narrow2<BF16>(v1[2], v1[3]);
      o2[2 * h] = narrow2<BF16>(v2[0], v2[1]);
      o2[2 * h + 1] = narrow2<BF16>(v2[2], v2[3]);
    }
    const int64_t e = ((int64_t)sl * R + y) * R + fv;        // o[c][slow][y][fast]
    store_vol((GlobalOut)(out + e), o0);
    store_vol((GlobalOut)(out + R3 + e), o1);
    store_vol((GlobalOut)(out + 2 * R3 + e), o2);
  }
}

template <int LAYOUT, bool BF16>
void launch_grid(const MapLowpArgs &a, int64_t blocks, hipStream_t s) {
  if (a.src.R % 8 == 0)
    hipLaunchKernelGGL((tsdf_map_grid_lowp_kernel<LAYOUT, BF16, 8>), dim3((unsigned)blocks), dim3(kSlabWG), 0, s, a);
  else
    hipLaunchKernelGGL((tsdf_map_grid_lowp_kernel<LAYOUT, BF16, 4>), dim3((unsigned)blocks), dim3(kSlabWG), 0, s, a);
}

}  // namespace

extern "C" {

int tsdf_maplowp_version(void) { return TSDF_MAPLOWP_VERSION; }

int tsdf_map_place_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                       int64_t n_src, const int64_t *d_index, int n, int R, const tsdf_cam *cam, void *hip_stream,
                       const double *d_xforms, float *d_out_grid, float *d_out_max_l, float *d_out_mid_p,
                       int32_t *d_out_status) {
  // arguments first, then the device, then the launch
  if (n < 0) return TSDF_ERR_INVALID_ARG;
  if (slab_bad_shape(R, TSDF_LAYOUT_CZYX)) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_depth || !d_offsets || !d_headers || !d_xforms || !d_out_grid || depth_len < 0) return TSDF_ERR_INVALID_ARG;
  if (n_src < 1 || (!d_index && n_src != n)) return TSDF_ERR_INVALID_ARG;
  if (misaligned(d_xforms, 7)) return TSDF_ERR_INVALID_ARG;
  if (!cam_ok(cam)) return TSDF_ERR_INVALID_ARG;
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  if (!cam) cam = &kDefaultCam;
  PlaceArgs a;
  a.depth = d_depth;
  a.depth_len = depth_len;
  a.offsets = d_offsets;
  a.headers = d_headers;
  a.n_src = n_src;
  a.index = d_index;
  a.n = n;
  a.R = R;
  a.focal = cam->focal;
  a.cx = cam->cx;
  a.cy = cam->cy;
  a.eps = cam->invalid_eps;
  a.trunc_vox = cam->trunc_voxels;
  a.xforms = d_xforms;
  a.grid = d_out_grid;
  a.max_l = d_out_max_l;
  a.mid_p = d_out_mid_p;
  a.status = d_out_status;
  const int blocks = n < kPlaceMaxBlocks ? n : kPlaceMaxBlocks;
  hipLaunchKernelGGL(tsdf_map_place_kernel, dim3((unsigned)blocks), dim3(kPlaceWG), 0, static_cast<hipStream_t>(hip_stream),
                     a);
  return launched();
}

int tsdf_voxelize_map_grid_lowp_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets,
                                    const int32_t *d_headers, int64_t n_src, const int64_t *d_index, int n, int R,
                                    const tsdf_cam *cam, int layout, int dtype, void *hip_stream, const double *d_xforms,
                                    const float *d_grid, void *d_out_tsdf, int32_t *d_out_status) {
  // arguments first, then the device, then the launch
  if (n < 0) return TSDF_ERR_INVALID_ARG;
  if (slab_bad_shape(R, layout)) return TSDF_ERR_INVALID_ARG;
  if (bad_dtype(dtype)) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_xforms || !d_grid || !d_out_tsdf || misaligned(d_xforms, 7) || misaligned(d_out_tsdf, 15))
    return TSDF_ERR_INVALID_ARG;
  SlabPlan plan;
  if (!slab_args_ok(d_depth, depth_len, d_offsets, d_headers, n_src, d_index, n, R, R % 8 == 0 ? 8 : 4, cam, plan))
    return TSDF_ERR_INVALID_ARG;
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  if (!cam) cam = &kDefaultCam;
  MapLowpArgs a;
  a.src = slab_src(d_depth, depth_len, d_offsets, d_headers, n_src, d_index, n, R, *cam, plan);
  a.eps = cam->invalid_eps;
  a.xforms = d_xforms;
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

}  // extern "C"
