// tsdf_locate.hip — libtsdf_locate.so: the hand located in raw depth frames — the nearest object's centre of mass, a fixed
// cube cut around it, the crops packed as the depth / offsets / headers triple the voxelizers read (include/tsdf_locate.h,
// which has the contract operation by operation).
//
// A translation unit and a library of its own, next to libtsdf_hip.so and the other extension libraries (all frozen).  It
// takes the status codes from include/tsdf.h, the host preamble every library here has from device.inc and cam_ok /
// finite32 from prim.inc; there is no device global: every launch is self-contained.
//
// tsdf_locate_kernel<T>: one workgroup of 1024 threads (16 wave64) per batch position, a grid-stride loop over positions
// when n exceeds the grid — the shape of tsdf_obb_kernel / tsdf_map_place_kernel.  Wave <-> rows, lane <-> four consecutive
// columns as one load through the element-aligned vector type (16 bytes of float32, 8 of uint16), the last W % 4 columns
// one by one; rows narrower than 33 groups are packed several to a wave.  Per position:
//   pass 0   d_min over the whole frame (float32 compares), a __shfl_xor butterfly, sixteen wave results through LDS;
//   pass 1   the seed sums N, sd, sx, sy in float64 over the whole frame, the same butterfly and the sixteen partials
//            summed in wave order by every lane (so the centre and the rectangle are uniform without a second barrier);
//   refine   the same sums over the rectangle's rows and columns alone — by then the frame is in L2 / Infinity Cache.
// Each set is a WINDOW of float32 depths (valid_px, band_top, cube_window: exactly the contract's float64 tests), so a
// pixel that is not summed costs two compares.  The LDS partials are double-buffered by pass parity: one barrier per pass.  Thread 0 writes the header, the centre, the
// status and the cube's grid row.
// tsdf_locate_scan_kernel: ONE workgroup; the sizes (right - left) * (bottom - top) of the headers just written, scanned
// into offsets[n + 1] — a chunk per thread, a __shfl_up scan per wave, sixteen wave totals through LDS.
// tsdf_locate_copy_kernel<T>: one workgroup per position; the rectangle's rows masked and copied (or widened) to
// depth[offsets[i] ...) with the mapping of the passes above, loads and stores through the 4-byte-aligned 16-byte vector type
// (a crop's start is only 4-byte aligned) and single elements at the ragged ends; the kept pixels are counted on the way.
// The pack's offsets depend on every earlier frame's size, which is why the copy is a launch of its own.
// Compiled with -ffp-contract=off: no fma anywhere in this file.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_locate.h"

namespace {

#include "device.inc"    // check_device, launched, misaligned: the host preamble of every library here
#include "prim.inc"      // cam_ok, finite32

constexpr int kLocWG = 1024;              // threads per workgroup
constexpr int kLocWaves = kLocWG / 64;    // 16 wave64
constexpr int kLocMaxBlocks = 1 << 16;    // positions beyond the grid are reached by the grid-stride loop

typedef float loc_f4 __attribute__((ext_vector_type(4), aligned(4)));        // 16 bytes on a 4-byte boundary
typedef uint16_t loc_u4 __attribute__((ext_vector_type(4), aligned(2)));     // 8 bytes on a 2-byte boundary

// four consecutive pixels of a row as float32 depth, and one
__device__ __forceinline__ loc_f4 load4(const float *p, float) { return *reinterpret_cast<const loc_f4 *>(p); }
__device__ __forceinline__ loc_f4 load4(const uint16_t *p, float scale) {
  const loc_u4 q = *reinterpret_cast<const loc_u4 *>(p);
  loc_f4 v;
  v.x = (float)q.x * scale;   // exact: u < 2^16 and scale is a power of two
  v.y = (float)q.y * scale;
  v.z = (float)q.z * scale;
  v.w = (float)q.w * scale;
  return v;
}
__device__ __forceinline__ float load1(const float *p, float) { return *p; }
__device__ __forceinline__ float load1(const uint16_t *p, float scale) { return (float)*p * scale; }

// The validity rule — finite, |d| >= eps, near <= d <= far — as two compares: near > 0, so a d >= near is its own absolute
// value and the rule is lo <= d <= hi with lo = max(eps, near) and hi = min(far, FLT_MAX) (the host forms them; a NaN
// fails both compares, an infinity the second).
__device__ __forceinline__ bool valid_px(float d, float lo, float hi) { return d >= lo && d <= hi; }

// The contract's float64 tests as float32 windows, so that a pass spends two compares on a pixel it does not sum.
// band_top: the largest float32 <= thr — for a float32 d, float64(d) <= thr is d <= band_top(thr).
__device__ __forceinline__ float band_top(double thr) {
  float f = (float)thr;
  if ((double)f > thr) f = nextafterf(f, -__builtin_inff());
  return f;
}
__device__ __forceinline__ bool in_cube(float d, double cd, double h) { return __builtin_fabs((double)d - cd) <= h; }
struct Window {
  float lo, hi;
};
// cube_window: the float32 depths d with |float64(d) - cd| <= h, held to [lo, hi].  The rounded difference is monotone in
// d, so they are an interval, and its ends are float32(cd -+ h) or a neighbour of it; each end is stepped onto the
// predicate ITSELF (a step or two; the loops are bounded), so the two compares select exactly the contract's pixels.
__device__ __forceinline__ Window cube_window(double cd, double h, float lo, float hi) {
  const float inf = __builtin_inff();
  float t1 = (float)(cd + h), t0 = (float)(cd - h);
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const float up = nextafterf(t1, inf), dn = nextafterf(t0, -inf);
    if (in_cube(up, cd, h)) t1 = up;
    if (in_cube(dn, cd, h)) t0 = dn;
  }
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    if (!in_cube(t1, cd, h)) t1 = nextafterf(t1, -inf);
    if (!in_cube(t0, cd, h)) t0 = nextafterf(t0, inf);
  }
  Window w;
  w.lo = t0 > lo ? t0 : lo;
  w.hi = t1 < hi ? t1 : hi;
  return w;
}

// Every pixel of [left, right) x [top, bottom) of one frame, f(depth, column, row, column in the rectangle, row in the
// rectangle).  gl lanes per row: the smallest power of two that holds the row's groups of four (4..64), so a wave takes
// 64 / gl rows at a time; everything here is uniform but the lane's own rows and group.  A lane's rows are taken kLocRows
// at a time, the loads of all of them issued before the first is used: one workgroup scans a frame, and with one load in
// flight per lane it waits for memory once per row.
constexpr int kLocRows = 8;
template <typename T, typename F>
__device__ __forceinline__ void scan_rect(const T *__restrict__ frame, int W, int left, int top, int right, int bottom,
                                          float scale, int lane, int wave, F &&f) {
  const int bw = right - left, bh = bottom - top;
  const int ngrp = bw >> 2, tail0 = ngrp << 2, ntail = bw - tail0;
  int sh = 6;
  while (sh > 2 && (1 << (sh - 1)) >= ngrp) --sh;
  const int gl = 1 << sh, rpw = 64 >> sh;
  const int sub = lane >> sh, gq = lane & (gl - 1);
  const int r0 = wave * rpw + sub, rs = kLocWaves * rpw;
  const T *__restrict__ base = frame + ((int64_t)top * W + left);
  for (int q = gq; q < ngrp; q += gl) {
    const int c = 4 * q;
    for (int r = r0; r < bh; r += kLocRows * rs) {
      loc_f4 v[kLocRows];
#pragma unroll
      for (int u = 0; u < kLocRows; ++u) {
        const int rr = r + u * rs;
        if (rr < bh) v[u] = load4(base + ((int64_t)rr * W + c), scale);
      }
#pragma unroll
      for (int u = 0; u < kLocRows; ++u) {
        const int rr = r + u * rs;
        if (rr < bh) {
          f(v[u].x, left + c, top + rr, c, rr);
          f(v[u].y, left + c + 1, top + rr, c + 1, rr);
          f(v[u].z, left + c + 2, top + rr, c + 2, rr);
          f(v[u].w, left + c + 3, top + rr, c + 3, rr);
        }
      }
    }
  }
  if (gq < ntail) {
    const int c = tail0 + gq;
    for (int r = r0; r < bh; r += kLocRows * rs) {
      float v[kLocRows];
#pragma unroll
      for (int u = 0; u < kLocRows; ++u) {
        const int rr = r + u * rs;
        if (rr < bh) v[u] = load1(base + ((int64_t)rr * W + c), scale);
      }
#pragma unroll
      for (int u = 0; u < kLocRows; ++u) {
        const int rr = r + u * rs;
        if (rr < bh) f(v[u], left + c, top + rr, c, rr);
      }
    }
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) v = v + __shfl_xor(v, k, 64);
  return v;
}
__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) v = v + __shfl_xor(v, k, 64);
  return v;
}
// the minima held by the lanes are never NaN: fminf is the plain minimum
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) v = __builtin_fminf(v, __shfl_xor(v, k, 64));
  return v;
}

struct LocArgs {
  const void *frames;        // [n_src][H][W], float32 or uint16
  float scale;               // 2^-shift (1 for float32)
  int64_t n_src;
  int H, W;
  const int64_t *index;      // [n] or null
  int n, R, refine;
  float lo, hi;              // the valid depths: max(eps, near) <= d <= min(far, FLT_MAX)
  float cube, band;
  double focal, cx, cy;
  float trunc_vox;
  int sw, sh;                // min(W, s), min(H, s): the capacity rule's sides
  int64_t capacity;
  float *depth;
  int64_t *offsets;          // [n + 1]
  int32_t *headers;          // [n][6]
  double *com;               // [n][3]
  int32_t *count, *status;   // [n]
  float *grid;               // [n][8] or null
  float *max_l;              // [n] or null
  float *mid_p;              // [n][3] or null
};

struct Rect {
  int l, t, r, b;
};

// floor(v) held to [lo, hi], as an int; written so that a NaN gives lo
__device__ __forceinline__ int clamp_floor(double v, int lo, int hi) {
  const double f = __builtin_floor(v);
  if (!(f >= (double)lo)) return lo;
  if (f > (double)hi) return hi;
  return (int)f;
}

// step 5 of the contract
__device__ __forceinline__ Rect rect_of(double c_x, double c_y, double cd, double h, const LocArgs &a) {
#pragma clang fp contract(off)
  const double F = a.focal;
  const double u0 = ((c_x - h) * F) / cd + a.cx;
  const double u1 = ((c_x + h) * F) / cd + a.cx;
  const double v0 = ((-(c_y + h)) * F) / cd + a.cy;
  const double v1 = ((-(c_y - h)) * F) / cd + a.cy;
  Rect q;
  q.l = clamp_floor(u0, 0, a.W - 1);
  q.r = clamp_floor(__builtin_floor(u1) + 1.0, q.l + 1, a.W);
  q.t = clamp_floor(v0, 0, a.H - 1);
  q.b = clamp_floor(__builtin_floor(v1) + 1.0, q.t + 1, a.H);
  if (q.r - q.l > a.sw) q.r = q.l + a.sw;
  if (q.b - q.t > a.sh) q.b = q.t + a.sh;
  return q;
}

// what thread 0 writes for a position that is not OK
__device__ __forceinline__ void write_empty(const LocArgs &a, int64_t i, int status) {
  int32_t *hd = a.headers + 6 * i;
  hd[0] = a.W, hd[1] = a.H, hd[2] = 0, hd[3] = 0, hd[4] = 1, hd[5] = 1;
  double *c = a.com + 3 * i;
  c[0] = 0.0, c[1] = 0.0, c[2] = 0.0;
  a.status[i] = status;
  if (a.grid) {
    float *g = a.grid + 8 * i;
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] = 0.f;
    if (a.max_l) a.max_l[i] = 0.f;
    if (a.mid_p) {
      float *p = a.mid_p + 3 * i;
      p[0] = 0.f, p[1] = 0.f, p[2] = 0.f;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kLocWG) void tsdf_locate_kernel(LocArgs a) {
#pragma clang fp contract(off)
  __shared__ float s_min[kLocWaves];
  __shared__ double s_red[2][kLocWaves][4];   // per pass parity and wave: N, sd, sx, sy

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = a.W, H = a.H;
  const float lo = a.lo, hi = a.hi, scale = a.scale;
  const double F = a.focal, cx = a.cx, cy = a.cy;
  const double h = (double)a.cube / 2.0;
  const float inf = __builtin_inff();

  for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
    const int64_t g = a.index ? a.index[i] : i;
    if (!(g >= 0 && g < a.n_src)) {   // (uniform) nothing of the frames is read
      if (tid == 0) write_empty(a, i, TSDF_FRAME_BAD_HEADER);
      continue;
    }
    const T *__restrict__ frame = static_cast<const T *>(a.frames) + g * ((int64_t)H * W);

    // pass 0: the smallest valid depth
    float mn = inf;
    scan_rect(frame, W, 0, 0, W, H, scale, lane, wave, [&](float d, int, int, int, int) {
      if (valid_px(d, lo, hi)) mn = d < mn ? d : mn;
    });
    mn = wave_min(mn);
    if (lane == 0) s_min[wave] = mn;
    __syncthreads();
    float dmin = s_min[0];
#pragma unroll
    for (int w = 1; w < kLocWaves; ++w) dmin = __builtin_fminf(dmin, s_min[w]);
    if (!(dmin < inf)) {   // (uniform) no valid pixel
      if (tid == 0) write_empty(a, i, TSDF_FRAME_DEGENERATE);
      __syncthreads();     // s_min is rewritten by the next position
      continue;
    }

    // pass 1, then the refinements: the sums of a set, its centre, the cube's rectangle
    // the seed set as a window of float32 depths: float64(d) <= float64(d_min) + float64(seed_band), or every valid pixel
    Window w = {lo, hi};
    if (a.band != 0.f) {
      const float top = band_top((double)dmin + (double)a.band);
      w.hi = top < hi ? top : hi;
    }
    double c_x = 0.0, c_y = 0.0, cd = 1.0;
    Rect q = {0, 0, W, H};
    for (int pass = 0; pass <= a.refine; ++pass) {
      double sn = 0.0, sd = 0.0, sx = 0.0, sy = 0.0;
      const float wl = w.lo, wh = w.hi;
      scan_rect(frame, W, q.l, q.t, q.r, q.b, scale, lane, wave, [&](float d, int x, int y, int, int) {
        if (!valid_px(d, wl, wh)) return;
        const double d64 = (double)d;
        sn = sn + 1.0;
        sd = sd + d64;
        sx = sx + d64 * ((double)x - cx);
        sy = sy + d64 * ((double)y - cy);
      });
      sn = wave_sum(sn), sd = wave_sum(sd), sx = wave_sum(sx), sy = wave_sum(sy);
      double(*red)[4] = s_red[pass & 1];
      if (lane == 0) red[wave][0] = sn, red[wave][1] = sd, red[wave][2] = sx, red[wave][3] = sy;
      __syncthreads();
      // every lane sums the sixteen partials in wave order: the same bits in every lane
      double N = red[0][0], td = red[0][1], tx = red[0][2], ty = red[0][3];
#pragma unroll 1   // (unrolled, the sixty-four partials are all in registers at once: scratch)
      for (int w = 1; w < kLocWaves; ++w) {
        N = N + red[w][0];
        td = td + red[w][1];
        tx = tx + red[w][2];
        ty = ty + red[w][3];
      }
      if (!(N > 0.0)) break;   // (uniform; never in pass 0: the pixel at d_min is in the seed set)
      c_x = (tx / F) / N;
      c_y = -((ty / F) / N);
      cd = td / N;
      q = rect_of(c_x, c_y, cd, h, a);
      q.l = __builtin_amdgcn_readfirstlane(q.l);
      q.t = __builtin_amdgcn_readfirstlane(q.t);
      q.r = __builtin_amdgcn_readfirstlane(q.r);
      q.b = __builtin_amdgcn_readfirstlane(q.b);
      w = cube_window(cd, h, lo, hi);   // the next set: valid, and |float64(d) - cd| <= h
    }

    if (tid == 0) {
      int32_t *hd = a.headers + 6 * i;
      hd[0] = W, hd[1] = H, hd[2] = q.l, hd[3] = q.t, hd[4] = q.r, hd[5] = q.b;
      double *c = a.com + 3 * i;
      c[0] = c_x, c[1] = c_y, c[2] = -cd;
      a.status[i] = TSDF_FRAME_OK;
      if (a.grid) {
        // the glue with max_l := cube, mid_p := float32(c): float32, one rounding per operation, left to right
        const float m0 = (float)c_x, m1 = (float)c_y, m2 = (float)(-cd);
        const float max_l = a.cube;
        const float vl = __fdiv_rn(max_l, (float)a.R);
        const float td = __fmul_rn(vl, a.trunc_vox);
        const float half_l = __fdiv_rn(max_l, 2.0f), half_v = __fdiv_rn(vl, 2.0f);
        float *gr = a.grid + 8 * i;
        gr[0] = __fadd_rn(__fsub_rn(m0, half_l), half_v);
        gr[1] = __fadd_rn(__fsub_rn(m1, half_l), half_v);
        gr[2] = __fadd_rn(__fsub_rn(m2, half_l), half_v);
        gr[3] = vl, gr[4] = td, gr[5] = 0.f, gr[6] = 0.f, gr[7] = 0.f;
        if (a.max_l) a.max_l[i] = max_l;
        if (a.mid_p) {
          float *p = a.mid_p + 3 * i;
          p[0] = m0, p[1] = m1, p[2] = m2;
        }
      }
    }
    __syncthreads();   // the next position writes s_min and s_red: not before this one's readers are done
  }
}

// the size a header states (what the locating kernel wrote: 1 <= sides <= W, H)
__device__ __forceinline__ int64_t header_size(const int32_t *hd) {
  return (int64_t)(hd[4] - hd[2]) * (int64_t)(hd[5] - hd[3]);
}

// offsets[0..n]: the exclusive prefix sums of the headers' sizes.  One workgroup; thread t takes the t-th chunk.
__global__ __launch_bounds__(kLocWG) void tsdf_locate_scan_kernel(const int32_t *__restrict__ headers, int n,
                                                                    int64_t *__restrict__ offsets) {
  __shared__ long long s_tot[kLocWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t chunk = ((int64_t)n + kLocWG - 1) / kLocWG;
  int64_t b = tid * chunk, e = b + chunk;
  b = b < n ? b : n;
  e = e < n ? e : n;
  long long s = 0;
  for (int64_t j = b; j < e; ++j) s += header_size(headers + 6 * j);
  long long inc = s;
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const long long t = __shfl_up(inc, k, 64);
    if (lane >= k) inc += t;
  }
  if (lane == 63) s_tot[wave] = inc;
  __syncthreads();
  long long run = inc - s;
  for (int w = 0; w < wave; ++w) run += s_tot[w];
  for (int64_t j = b; j < e; ++j) {
    offsets[j] = run;
    run += header_size(headers + 6 * j);
  }
  if (tid == kLocWG - 1) offsets[n] = run;   // the last thread's chunk ends at n (or is empty): run is the total
}

template <typename T>
__global__ __launch_bounds__(kLocWG) void tsdf_locate_copy_kernel(LocArgs a) {
#pragma clang fp contract(off)
  __shared__ int s_cnt[kLocWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = a.W, H = a.H;
  const float lo = a.lo, hi = a.hi, scale = a.scale;
  const double h = (double)a.cube / 2.0;

  for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
    const int64_t off = a.offsets[i];
    const int32_t *hd = a.headers + 6 * i;
    const int left = hd[2], top = hd[3], right = hd[4], bottom = hd[5];
    const int bw = right - left, bh = bottom - top;
    const int64_t g = a.index ? a.index[i] : i;
    // (uniform) what the two launches before this one wrote always passes; nothing outside the frame is read and
    // nothing outside the buffer written whatever they hold
    const bool inside = left >= 0 && top >= 0 && bw > 0 && bh > 0 && right <= W && bottom <= H && off >= 0 &&
                        off + (int64_t)bw * bh <= a.capacity;
    if (!inside) continue;
    if (a.status[i] != TSDF_FRAME_OK || !(g >= 0 && g < a.n_src)) {   // (uniform) one pixel of +0
      if (tid == 0) {
        a.depth[off] = 0.f;
        a.count[i] = 0;
      }
      continue;
    }
    const T *__restrict__ frame = static_cast<const T *>(a.frames) + g * ((int64_t)H * W);
    float *__restrict__ out = a.depth + off;
    const Window w = cube_window(-a.com[3 * i + 2], h, lo, hi);   // valid, and |float64(d) - cd| <= h
    const float wl = w.lo, wh = w.hi;
    const int ngrp = bw >> 2;
    int kept = 0;
    // the mapping of scan_rect, a group of four leaving as one store: f sees the group's pixels in order, column by
    // column, so the fourth (or a tail pixel) completes what is written
    loc_f4 acc = {0.f, 0.f, 0.f, 0.f};
    scan_rect(frame, W, left, top, right, bottom, scale, lane, wave, [&](float d, int, int, int col, int r) {
      const bool keep = valid_px(d, wl, wh);
      const float v = keep ? d : 0.f;
      kept += keep ? 1 : 0;
      float *__restrict__ dst = out + ((int64_t)r * bw + col);
      if (col >= (ngrp << 2)) {   // a tail pixel
        *dst = v;
        return;
      }
      const int k = col & 3;
      if (k == 0) acc.x = v;
      else if (k == 1) acc.y = v;
      else if (k == 2) acc.z = v;
      else {
        acc.w = v;
        *reinterpret_cast<loc_f4 *>(dst - 3) = acc;
      }
    });
    kept = wave_isum(kept);
    if (lane == 0) s_cnt[wave] = kept;
    __syncthreads();
    if (tid == 0) {
      int c = 0;
#pragma unroll
      for (int w = 0; w < kLocWaves; ++w) c += s_cnt[w];
      a.count[i] = c;
    }
    __syncthreads();   // s_cnt is rewritten by the next position
  }
}

// the capacity rule's s, held to what an int holds (the sides are min(W, s), min(H, s))
bool capacity_side(float cube, float near_mm, double focal, int *s) {
  if (!(cube > 0.f) || !(near_mm > 0.f) || !(focal > 0.0)) return false;
  const double v = __builtin_floor(((double)cube * focal) / (double)near_mm) + 2.0;
  *s = v < 2147483647.0 ? (int)v : 2147483647;   // (an infinite quotient lands here too)
  return true;
}

}  // namespace

extern "C" {

int tsdf_locate_version(void) { return TSDF_LOCATE_VERSION; }

int tsdf_locate_capacity(int H, int W, float cube, float near_mm, double focal, int64_t *per_frame) {
  int s = 0;
  if (!per_frame || H <= 0 || W <= 0 || !capacity_side(cube, near_mm, focal, &s)) return TSDF_ERR_INVALID_ARG;
  *per_frame = (int64_t)(W < s ? W : s) * (int64_t)(H < s ? H : s);
  return TSDF_OK;
}

int tsdf_locate_hip(const void *d_frames, int frame_type, int shift, int64_t n_src, int H, int W, const int64_t *d_index,
                    int n, float near_mm, float far_mm, float cube, float seed_band, int refine, int R, double focal,
                    double cx, double cy, float invalid_eps, float trunc_voxels, int64_t depth_capacity, void *hip_stream,
                    float *d_out_depth, int64_t *d_out_offsets, int32_t *d_out_headers, double *d_out_com,
                    int32_t *d_out_count, int32_t *d_out_status, float *d_out_grid, float *d_out_max_l,
                    float *d_out_mid_p) {
  // arguments first, then the device, then the launches
  if (n < 0) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (frame_type != TSDF_LOCATE_F32 && frame_type != TSDF_LOCATE_U16) return TSDF_ERR_INVALID_ARG;
  const bool u16 = frame_type == TSDF_LOCATE_U16;
  if (u16 && (shift < 0 || shift > 7)) return TSDF_ERR_INVALID_ARG;
  if (H <= 0 || W <= 0) return TSDF_ERR_INVALID_ARG;
  if (n_src < 1 || (!d_index && n_src != n)) return TSDF_ERR_INVALID_ARG;
  if (!(near_mm > 0.f) || !(far_mm >= near_mm) || !(cube > 0.f) || !(seed_band >= 0.f)) return TSDF_ERR_INVALID_ARG;
  if (refine < 0 || refine > 8) return TSDF_ERR_INVALID_ARG;
  if (bad_res(R)) return TSDF_ERR_INVALID_ARG;
  const tsdf_cam cam = {focal, cx, cy, invalid_eps, trunc_voxels};   // by value in the ABI, one rule all the same
  if (!cam_ok(&cam)) return TSDF_ERR_INVALID_ARG;
  if (!d_frames || !d_out_depth || !d_out_offsets || !d_out_headers || !d_out_com || !d_out_count || !d_out_status)
    return TSDF_ERR_INVALID_ARG;
  if (!d_out_grid && (d_out_max_l || d_out_mid_p)) return TSDF_ERR_INVALID_ARG;
  if (misaligned(d_frames, u16 ? 1 : 3) || misaligned(d_out_depth, 3) || misaligned(d_out_com, 7) ||
      misaligned(d_out_offsets, 7))
    return TSDF_ERR_INVALID_ARG;
  int s = 0;
  if (!capacity_side(cube, near_mm, focal, &s)) return TSDF_ERR_INVALID_ARG;
  const int sw = W < s ? W : s, sh = H < s ? H : s;
  // n * sw * sh without overflow: sw * sh < 2^62, and the comparison is a division
  const int64_t per_frame = (int64_t)sw * sh;
  if (depth_capacity < per_frame || depth_capacity / per_frame < n) return TSDF_ERR_INVALID_ARG;
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;

  LocArgs a;
  a.frames = d_frames;
  a.scale = u16 ? 1.0f / (float)(1 << shift) : 1.0f;
  a.n_src = n_src;
  a.H = H;
  a.W = W;
  a.index = d_index;
  a.n = n;
  a.R = R;
  a.refine = refine;
  a.lo = near_mm > cam.invalid_eps ? near_mm : cam.invalid_eps;
  a.hi = far_mm < 3.402823466e+38f ? far_mm : 3.402823466e+38f;
  a.cube = cube;
  a.band = seed_band;
  a.focal = cam.focal;
  a.cx = cam.cx;
  a.cy = cam.cy;
  a.trunc_vox = cam.trunc_voxels;
  a.sw = sw;
  a.sh = sh;
  a.capacity = depth_capacity;
  a.depth = d_out_depth;
  a.offsets = d_out_offsets;
  a.headers = d_out_headers;
  a.com = d_out_com;
  a.count = d_out_count;
  a.status = d_out_status;
  a.grid = d_out_grid;
  a.max_l = d_out_max_l;
  a.mid_p = d_out_mid_p;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const dim3 blocks((unsigned)(n < kLocMaxBlocks ? n : kLocMaxBlocks)), wg(kLocWG);
  if (u16)
    hipLaunchKernelGGL(tsdf_locate_kernel<uint16_t>, blocks, wg, 0, st, a);
  else
    hipLaunchKernelGGL(tsdf_locate_kernel<float>, blocks, wg, 0, st, a);
  hipLaunchKernelGGL(tsdf_locate_scan_kernel, dim3(1), wg, 0, st, d_out_headers, n, d_out_offsets);
  if (u16)
    hipLaunchKernelGGL(tsdf_locate_copy_kernel<uint16_t>, blocks, wg, 0, st, a);
  else
    hipLaunchKernelGGL(tsdf_locate_copy_kernel<float>, blocks, wg, 0, st, a);
  return launched();
}

}  // extern "C"
