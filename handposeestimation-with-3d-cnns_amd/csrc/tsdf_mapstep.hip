// tsdf_mapstep.hip — libtsdf_mapstep.so: two per-frame maps composed into one, and the head of the augmented step — draw,
// compose, grid placement, labels — as one launch (include/tsdf_mapstep.h).
//
// A translation unit and a library of its own, next to libtsdf_hip.so and the other extension libraries (all frozen).  It
// takes the status codes from include/tsdf.h, the host preamble every library here has from device.inc, the
// device primitives from prim.inc and the augmentation's draw and map arithmetic from augdraw.inc, which it includes
// UNCHANGED: aug_draw_row writes its row through a generic pointer, and here that pointer is a row in LDS, so the
// draw exists once for the three libraries that use it.  The placement's crop pass, wave butterfly, glue and degenerate
// rule come from place.inc, the text tsdf_maplowp.hip::tsdf_map_place_kernel runs: the head's placement equals that
// kernel's bit for bit because it is the same arithmetic, written once.  The joints' map (tsdf_auggrid.hip::
// tsdf_transform_joints_kernel) and the label normalisation (kernels.inc::tsdf_normalize_kernel) are RESTATED here
// operation for operation; there is no device global: every launch is self-contained.
//
// tsdf_compose_kernel: one lane per map, 256-thread workgroups, no LDS.  The two halves one after the other (a half is 24
// doubles in, 12 out), every row as 16-byte accesses on its 8-byte boundary; the 192-byte result leaves as twelve 16-byte
// stores, as aug_store writes a drawn row.
//
// tsdf_map_step_head_kernel: one workgroup of 1024 threads (16 wave64) per batch position, a grid-stride loop over
// positions when n exceeds the grid — the shape of tsdf_map_place_kernel.  Per position:
//   1. thread 0 draws U into LDS (aug_draw_row), composes it with the source frame's base row when there is one, and
//      leaves T's 24 doubles in LDS and in global memory; meanwhile every lane resolves the source frame and its header;
//   2. a barrier, then every lane takes T's forward rows from LDS;
//   3. the placement's crop pass and wave butterfly (place.inc::place_crop), a barrier, and its glue (place_glue, thread
//      0), which also publishes max_l and mid_p in LDS;
//   4. a barrier, then lanes 0..J-1 map one joint of the source frame each and normalise it.
// No atomics, no communication between workgroups, at most four barriers per position, all under uniform conditions.
// Without d_out_grid there is nothing for a workgroup to do: tsdf_map_step_draw_kernel is step 1 alone, one lane per
// position in 256-thread workgroups (tsdf_aug_draw_at_kernel's shape), the row drawn into d_out_xforms and composed there.
// Compiled with -ffp-contract=off, fma only where __builtin_fma is written.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_mapstep.h"

namespace {

#include "device.inc"    // check_device, launched, misaligned: the host preamble of every library here
#include "prim.inc"      // cam_ok, finite32, header_ok
#include "augdraw.inc"   // kAugWG, aug_d2, aug_store, aug_draw_row: shared with tsdf_augment.hip and tsdf_augstep.hip
#include "place.inc"     // place_crop, place_glue, Placed: the placement's arithmetic, shared with tsdf_maplowp.hip

constexpr int kHeadWG = 1024;              // threads per workgroup of the head
constexpr int kHeadWaves = kHeadWG / 64;   // 16 wave64
constexpr int kHeadMaxBlocks = 1 << 16;    // positions beyond the grid are reached by the grid-stride loop

// One half of a composition: rows (A | b) of P after Q, every product and every sum rounded on its own.
__device__ __forceinline__ void compose_half(const double (&P)[12], const double (&Q)[12], double (&o)[12]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double p0 = P[4 * i], p1 = P[4 * i + 1], p2 = P[4 * i + 2], p3 = P[4 * i + 3];
#pragma unroll
    for (int j = 0; j < 3; ++j) o[4 * i + j] = (p0 * Q[j] + p1 * Q[4 + j]) + p2 * Q[8 + j];
    o[4 * i + 3] = ((p0 * Q[3] + p1 * Q[7]) + p2 * Q[11]) + p3;
  }
}

// twelve doubles as six 16-byte loads / stores on an 8-byte boundary
__device__ __forceinline__ void load12(const double *p, double (&v)[12]) {
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const aug_d2 t = *reinterpret_cast<const aug_d2 *>(p + 2 * k);
    v[2 * k] = t.x;
    v[2 * k + 1] = t.y;
  }
}
__device__ __forceinline__ void store12(double *p, const double (&v)[12]) {
#pragma unroll
  for (int k = 0; k < 6; ++k) aug_store(p, k, v[2 * k], v[2 * k + 1]);
}

// out = outer o inner, or outer itself when there is no inner row; out may be outer (each half is read before it is
// written, and the second half reads nothing the first wrote)
__device__ __forceinline__ void compose_row(const double *outer, const double *inner, double *out) {
  double P[12], Q[12], o[12];
  load12(outer, P);            // forward: outer's rows after inner's
  if (inner) {
    load12(inner, Q);
    compose_half(P, Q, o);
    store12(out, o);
  } else {
    store12(out, P);
  }
  load12(outer + 12, Q);       // inverse: inner's inverse rows after outer's
  if (inner) {
    load12(inner + 12, P);
    compose_half(P, Q, o);
    store12(out + 12, o);
  } else {
    store12(out + 12, Q);
  }
}

struct ComposeArgs {
  const double *outer;    // [n][24]
  const double *inner;    // [n_inner][24]
  int64_t n_inner;
  const int64_t *index;   // [n] or null
  int n;
  double *out;            // [n][24]
};

__global__ __launch_bounds__(kAugWG) void tsdf_compose_kernel(ComposeArgs a) {
  const int i = blockIdx.x * kAugWG + threadIdx.x;
  if (i >= a.n) return;
  const int64_t g = a.index ? a.index[i] : (int64_t)i;
  const bool ok = g >= 0 && g < a.n_inner;
  compose_row(a.outer + 24 * (int64_t)i, ok ? a.inner + 24 * g : nullptr, a.out + 24 * (int64_t)i);
}

struct HeadArgs {
  const float *depth;
  int64_t depth_len;
  const int64_t *offsets;    // [n_src + 1]
  const int32_t *headers;    // [n_src][6]
  int64_t n_src;
  const int64_t *index;      // [n] or null
  int n, R;
  double focal, cx, cy;
  float eps, trunc_vox;
  const float *centres;      // [n_src][3]
  const double *base;        // [n_src][24] or null
  const uint64_t *state;     // {key, counter0}
  const int64_t *counters;   // [n] or null
  const float *gt;           // [n_src][3 J] or null
  int J, clamp;
  double *xforms;            // [n][24]
  float *grid;               // [n][8] or null: no placement, no labels
  float *max_l;              // [n] or null
  float *mid_p;              // [n][3] or null
  int32_t *status;           // [n] or null
  float *gt_aug;             // [n][3 J] or null
  float *gt_nor;             // [n][3 J] (with gt)
  double *stretch;           // [n] or null
  int32_t *rot;              // [n][2] or null
};

// d_out_grid == NULL: the draw and the composition alone, one lane per position — tsdf_aug_draw_at_kernel's shape.  The
// lane draws its row straight into d_out_xforms and composes it in place.
__global__ __launch_bounds__(kAugWG) void tsdf_map_step_draw_kernel(HeadArgs a) {
  const int i = blockIdx.x * kAugWG + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t key = a.state[0], counter0 = a.state[1];
  const int64_t g = a.index ? a.index[i] : (int64_t)i;
  const uint64_t c = counter0 + (a.counters ? (uint64_t)a.counters[i] : (uint64_t)i);
  aug_draw_row(a.centres, a.n_src, g, i, key, c, a.xforms, a.stretch, a.rot);
  if (a.base && g >= 0 && g < a.n_src) {
    double *row = a.xforms + 24 * (int64_t)i;
    compose_row(row, a.base + 24 * g, row);
  }
}

// what thread 0 writes for one position, and what the labels read: s_pl = max_l, mid_p
__device__ __forceinline__ void place_write(const HeadArgs &a, int64_t i, float (&s_pl)[4], const Placed &p) {
  float *g = a.grid + 8 * i;
  g[0] = p.ox, g[1] = p.oy, g[2] = p.oz, g[3] = p.vl, g[4] = p.td, g[5] = 0.f, g[6] = 0.f, g[7] = 0.f;
  if (a.max_l) a.max_l[i] = p.max_l;
  if (a.mid_p) {
    float *m = a.mid_p + 3 * i;
    m[0] = p.m0, m[1] = p.m1, m[2] = p.m2;
  }
  if (a.status) a.status[i] = p.status;
  s_pl[0] = p.max_l, s_pl[1] = p.m0, s_pl[2] = p.m1, s_pl[3] = p.m2;
}

__global__ __launch_bounds__(kHeadWG) void tsdf_map_step_head_kernel(HeadArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double s_T[24];   // the position's map
  __shared__ float s_red[kHeadWaves][8];                    // per wave: min xyz, max xyz, any, pad
  __shared__ float s_pl[4];                                 // max_l, mid_p

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double F = a.focal, cx = a.cx, cy = a.cy;
  const float eps = a.eps;

  for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
    // the source frame; outside the tables the draw is the identity, the base is not read and the header is bad
    const int64_t g = a.index ? a.index[i] : i;
    const bool src_ok = g >= 0 && g < a.n_src;   // (uniform)

    if (tid == 0) {
      const uint64_t key = a.state[0], counter0 = a.state[1];
      const uint64_t c = counter0 + (a.counters ? (uint64_t)a.counters[i] : (uint64_t)i);
      aug_draw_row(a.centres, a.n_src, g, 0, key, c, s_T, a.stretch ? a.stretch + i : nullptr,
                   a.rot ? a.rot + 2 * i : nullptr);
      if (a.base && src_ok) compose_row(s_T, a.base + 24 * g, s_T);
      compose_row(s_T, nullptr, a.xforms + 24 * i);   // (a copy: twelve 16-byte stores)
    }

    bool ok = src_ok;
    int left = 0, top = 0, right = 0, bottom = 0;
    int64_t off0 = 0;
    if (ok) {
      const int32_t *hd = a.headers + 6 * g;
      left = hd[2], top = hd[3], right = hd[4], bottom = hd[5];
      const int64_t off1 = a.offsets[g + 1], depth_len = a.depth_len;
      off0 = a.offsets[g];
      ok = header_ok(left, top, right, bottom, off0, off1, depth_len);
    }
    __syncthreads();   // T is in s_T

    if (!ok) {         // (uniform) the depth is not read
      if (tid == 0) place_write(a, i, s_pl, place_none(TSDF_FRAME_BAD_HEADER));
    } else {
      const int bw = right - left, bh = bottom - top;   // header_ok: both are positive ints
      const float *__restrict__ d = a.depth + off0;
      double m[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) m[k] = s_T[k];

      place_crop<kHeadWaves>(d, left, top, bw, bh, F, cx, cy, eps, m, lane, wave, s_red);
      __syncthreads();
      if (tid == 0) place_write(a, i, s_pl, place_glue<kHeadWaves>(s_red, a.R, a.trunc_vox));
    }

    if (a.gt) {          // (uniform)
      __syncthreads();   // max_l and mid_p are in s_pl
      const int64_t gs = g < 0 ? 0 : g >= a.n_src ? a.n_src - 1 : g;   // the joints of the nearest frame
      const float ml = s_pl[0];
      for (int j = tid; j < a.J; j += kHeadWG) {
        const float *__restrict__ p = a.gt + 3 * (gs * a.J + j);
        const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
        const int64_t at = 3 * (i * a.J + j);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          // tsdf_transform_joints_kernel, then tsdf_normalize_kernel on the float32 it wrote
          const float v = (float)__builtin_fma(s_T[4 * r], x, __builtin_fma(s_T[4 * r + 1], y,
                                                                             __builtin_fma(s_T[4 * r + 2], z, s_T[4 * r + 3])));
          if (a.gt_aug) a.gt_aug[at + r] = v;
          float o = 0.5f;
          if (ml > 0.f) {
            o = __fadd_rn(__fdiv_rn(__fsub_rn(v, s_pl[1 + r]), ml), 0.5f);
            if (a.clamp) {
              o = o < 0.f ? 0.f : o;
              o = o > 1.f ? 1.f : o;
            }
          }
          a.gt_nor[at + r] = o;
        }
      }
    }
    __syncthreads();   // the next position writes s_T, s_red and s_pl: not before this one's readers are done
  }
}

}  // namespace

extern "C" {

int tsdf_mapstep_version(void) { return TSDF_MAPSTEP_VERSION; }

int tsdf_compose_xforms_hip(const double *d_outer, const double *d_inner, int64_t n_inner, const int64_t *d_index, int n,
                            void *hip_stream, double *d_out) {
  // arguments first, then the device, then the launch
  if (n < 0) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_outer || !d_inner || !d_out) return TSDF_ERR_INVALID_ARG;
  if (n_inner < 1 || (!d_index && n_inner != n)) return TSDF_ERR_INVALID_ARG;
  if (misaligned(d_outer, 7) || misaligned(d_inner, 7) || misaligned(d_out, 7)) return TSDF_ERR_INVALID_ARG;
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  ComposeArgs a;
  a.outer = d_outer;
  a.inner = d_inner;
  a.n_inner = n_inner;
  a.index = d_index;
  a.n = n;
  a.out = d_out;
  const unsigned blocks = ((unsigned)n + kAugWG - 1) / kAugWG;
  hipLaunchKernelGGL(tsdf_compose_kernel, dim3(blocks), dim3(kAugWG), 0, static_cast<hipStream_t>(hip_stream), a);
  return launched();
}

int tsdf_map_step_head_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                           int64_t n_src, const int64_t *d_index, int n, int R, double focal, double cx, double cy,
                           float invalid_eps, float trunc_voxels, const float *d_centres, const double *d_base, const uint64_t *d_state,
                           const int64_t *d_counters, const float *d_gt, int n_joints, int clamp, void *hip_stream,
                           double *d_out_xforms, float *d_out_grid, float *d_out_max_l, float *d_out_mid_p,
                           int32_t *d_out_status, float *d_out_gt_aug, float *d_out_gt_nor, double *d_out_stretch,
                           int32_t *d_out_rot) {
  // arguments first, then the device, then the launch
  if (n < 0) return TSDF_ERR_INVALID_ARG;
  if (bad_res(R)) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_centres || !d_state || !d_out_xforms) return TSDF_ERR_INVALID_ARG;
  if (n_src < 1 || (!d_index && n_src != n)) return TSDF_ERR_INVALID_ARG;
  if (misaligned(d_out_xforms, 7) || misaligned(d_state, 7) || misaligned(d_base, 7)) return TSDF_ERR_INVALID_ARG;
  const tsdf_cam cam = {focal, cx, cy, invalid_eps, trunc_voxels};   // by value in the ABI, one rule all the same
  if (!cam_ok(&cam)) return TSDF_ERR_INVALID_ARG;
  if (d_out_grid) {
    if (!d_depth || !d_offsets || !d_headers || depth_len < 0) return TSDF_ERR_INVALID_ARG;
  } else if (d_out_max_l || d_out_mid_p || d_out_status || d_gt) {
    return TSDF_ERR_INVALID_ARG;
  }
  if (d_gt) {
    if (!d_out_gt_nor || n_joints < 1 || n_joints > 170) return TSDF_ERR_INVALID_ARG;
  } else if (d_out_gt_aug || d_out_gt_nor) {
    return TSDF_ERR_INVALID_ARG;
  }
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  HeadArgs a;
  a.depth = d_depth;
  a.depth_len = depth_len;
  a.offsets = d_offsets;
  a.headers = d_headers;
  a.n_src = n_src;
  a.index = d_index;
  a.n = n;
  a.R = R;
  a.focal = cam.focal;
  a.cx = cam.cx;
  a.cy = cam.cy;
  a.eps = cam.invalid_eps;
  a.trunc_vox = cam.trunc_voxels;
  a.centres = d_centres;
  a.base = d_base;
  a.state = d_state;
  a.counters = d_counters;
  a.gt = d_gt;
  a.J = d_gt ? n_joints : 0;
  a.clamp = clamp;
  a.xforms = d_out_xforms;
  a.grid = d_out_grid;
  a.max_l = d_out_max_l;
  a.mid_p = d_out_mid_p;
  a.status = d_out_status;
  a.gt_aug = d_out_gt_aug;
  a.gt_nor = d_out_gt_nor;
  a.stretch = d_out_stretch;
  a.rot = d_out_rot;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  if (!d_out_grid) {
    hipLaunchKernelGGL(tsdf_map_step_draw_kernel, dim3(((unsigned)n + kAugWG - 1) / kAugWG), dim3(kAugWG), 0, s, a);
    return launched();
  }
  const int blocks = n < kHeadMaxBlocks ? n : kHeadMaxBlocks;
  hipLaunchKernelGGL(tsdf_map_step_head_kernel, dim3((unsigned)blocks), dim3(kHeadWG), 0, s, a);
  return launched();
}

}  // extern "C"
