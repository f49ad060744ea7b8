// tsdf_fps.hip — libtsdf_fps.so: farthest-point sampled clouds from a packed crop or from a cloud
// (include/tsdf_fps.h, which has the contract operation by operation).
//
// A translation unit and a library of its own, next to libtsdf_hip.so and the other libraries (all frozen).  It takes the
// status codes from include/tsdf.h, the host preamble every library here has from device.inc, cam_ok, finite32 and
// header_ok from prim.inc and its argument rules and its plan from fps_host.inc, plain C++ that is also built on its own
// under the CPU sanitizers.  No device global and no global atomic: every launch is self-contained.
//
// tsdf_fps_kernel: a long, strictly sequential chain of workgroup-wide arg-max reductions.  One workgroup of kFpsWG
// threads per batch position:
//   1. COUNT.  Wave w walks its piece of the items (pixels of the crop, rows of the cloud; fps_host.inc::fps_segment) 64
//      at a time, runs the loader's arithmetic and counts the candidates by ballot.  The waves' counts meet in LDS: their
//      sum is `count`, their prefix the wave's first compact index.  The pieces are in item order, so compact index c
//      orders as rank does and "lowest rank" is "lowest c".
//   2. The form (fps_host.inc::fps_holds).  A position the call cannot hold writes its zero rows and is done.
//   3. COMPACT.  The same walk again, now storing candidate c: RESIDENT into three float32 arrays in LDS, from which
//      lane t then takes the candidates t, t + kFpsWG, ... into registers (x, y, z and the running dist, fps_slots(count)
//      of them: the loop's trip count is the workgroup's, not the cap's); STREAMING as (x, y, z, +inf) into the
//      position's workspace row.
//   4. M - 1 iterations: every lane updates the dist of its candidates against the last sample and keeps its best as a
//      64-bit key, (dist's bit pattern) << 32 | ~c — dist is in [+0, +inf], so the key's unsigned order is "greatest
//      dist, then lowest c".  The key is maximised across the wave with six DPP steps, lane 63 puts the wave's into one
//      of two alternating LDS rows, ONE barrier, every wave maximises the rows' keys with four DPP steps and reads the
//      winner's coordinates (LDS resident, the workspace streaming) at a uniform address.  Thread 0 writes the row.
//      Once the greatest dist is +0 the rule selects sample 0 for ever: the rest of the rows are written in parallel.
//   5. RANKS.  The rows so far hold compact indices.  The walk runs a third time and stores every candidate's rank where
//      its x was (LDS) or its dist was (workspace), and each row's index is replaced by its rank.  (Holding the ranks
//      next to the points would cost the resident form a quarter of its cap.)
// All global indexing is in 64 bits.  Compiled with -ffp-contract=off: no fma anywhere in this file.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_fps.h"

namespace {

#include "device.inc"     // check_device, launched, misaligned: the host preamble of every library here
#include "prim.inc"       // cam_ok, finite32, header_ok
#include "fps_host.inc"   // fps_defect, fps_points_defect, fps_plan, fps_holds, fps_slots, fps_segment, kFpsWG

// the loaders: candidates from a crop, from a crop under a map, from a float32 cloud, from a float64 cloud
enum { kFpsCrop = 0, kFpsMappedCrop, kFpsCloud32, kFpsCloud64 };

typedef unsigned long long fps_key;
typedef float fps_f4 __attribute__((ext_vector_type(4)));

struct FpsArgs {
  const float *depth;       // the crop loaders
  int64_t depth_len;
  const int64_t *offsets;   // [n_src + 1]
  const int32_t *headers;   // [n_src][6]
  int64_t n_src;
  const int64_t *index;     // [n] or null
  double focal, cx, cy;
  float eps;
  const double *xforms;     // [n][24] or null
  const void *cloud;        // the cloud loaders: [n][P][3]
  int64_t P;
  int M, hint;
  int64_t capacity;
  float *work;              // [n][capacity][4] or null
  float *out_points;        // [n][M][3]
  int32_t *out_pixel;       // [n][M]
  float *out_radius2;       // [n][M] or null
  int32_t *out_count, *out_status;
};

// what an item needs of its position
struct FpsFrame {
  const float *d;
  int left, top;
  unsigned bw;
  double F, cx, cy;
  float eps;
  double m[12];
  const void *rows;
};

// item `it` of the position: is it a candidate, and its float32 point
template <int SRC>
__device__ __forceinline__ bool fps_candidate(const FpsFrame &f, int64_t it, float &x, float &y, float &z) {
  if constexpr (SRC == kFpsCloud32) {
    const float *r = static_cast<const float *>(f.rows) + 3 * it;
    x = r[0], y = r[1], z = r[2];
  } else if constexpr (SRC == kFpsCloud64) {
    const double *r = static_cast<const double *>(f.rows) + 3 * it;
    x = (float)r[0], y = (float)r[1], z = (float)r[2];
  } else {
    const unsigned u = (unsigned)it, row = u / f.bw, col = u - row * f.bw;   // it < 2^31
    const float d = f.d[it];
    if (!(__builtin_fabsf(d) >= f.eps)) return false;   // NaN is no candidate
    const double d64 = (double)d;
    const double q = d64 / f.F;                         // IEEE division
    const double px = q * ((double)(f.left + (int)col) - f.cx);
    const double py = -(q * ((double)(f.top + (int)row) - f.cy));
    const double pz = -d64;
    if constexpr (SRC == kFpsMappedCrop) {
      x = (float)((f.m[0] * px + f.m[1] * py) + (f.m[2] * pz + f.m[3]));
      y = (float)((f.m[4] * px + f.m[5] * py) + (f.m[6] * pz + f.m[7]));
      z = (float)((f.m[8] * px + f.m[9] * py) + (f.m[10] * pz + f.m[11]));
    } else {
      x = (float)px, y = (float)py, z = (float)pz;
    }
  }
  return finite32(x) && finite32(y) && finite32(z);
}

// The wave's piece of the items, 64 at a time: sink(c, rank, x, y, z) for every candidate, c counting up from `base` in
// item order.  Returns the piece's candidates.  Every lane of the wave runs every step (the bounds are the wave's).
template <int SRC, typename Sink>
__device__ __forceinline__ int fps_walk(const FpsFrame &f, int64_t items, int64_t seg, int wave, int lane, int base,
                                        Sink sink) {
  const int64_t b = wave * seg, e = b + seg < items ? b + seg : items;
  int run = base;
  for (int64_t i0 = b; i0 < e; i0 += 64) {
    const int64_t it = i0 + lane;
    float x = 0.f, y = 0.f, z = 0.f;
    const bool cand = it < e && fps_candidate<SRC>(f, it, x, y, z);
    const unsigned long long m = __ballot(cand);
    if (cand) sink(run + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)), (int)it, x, y, z);
    run += __popcll(m);
  }
  return run - base;
}

// max(v, the key of the lane the DPP control names); a lane the control gives no source keeps its own
template <int CTRL>
__device__ __forceinline__ fps_key fps_dpp_max(fps_key v) {
  const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
  const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  const fps_key o = ((fps_key)ohi << 32) | olo;
  return o > v ? o : v;
}

// lane 15 of each row of 16 lanes: the row's greatest key
__device__ __forceinline__ fps_key fps_row_max(fps_key v) {
  v = fps_dpp_max<0x111>(v);   // row_shr:1
  v = fps_dpp_max<0x112>(v);   // row_shr:2
  v = fps_dpp_max<0x114>(v);   // row_shr:4
  return fps_dpp_max<0x118>(v);   // row_shr:8
}

// lane 63: the wave's greatest key
__device__ __forceinline__ fps_key fps_wave_max(fps_key v) {
  v = fps_row_max(v);
  v = fps_dpp_max<0x142>(v);   // row_bcast:15: lane 15 of a row to the next row
  return fps_dpp_max<0x143>(v);   // row_bcast:31: lane 31 to rows 2 and 3
}

// The workgroup's greatest key, in every lane: ONE barrier.  `rows` is the LDS row of this iteration (the two rows
// alternate: a wave that runs ahead writes the other one, and cannot reach this one again before every wave has passed
// the next barrier, that is, has read it).
__device__ __forceinline__ fps_key fps_group_max(fps_key mine, fps_key *rows, int lane, int wave) {
  const fps_key w = fps_wave_max(mine);
  if (lane == 63) rows[wave] = w;
  __syncthreads();
  const fps_key v = fps_row_max(rows[lane & (kFpsWaves - 1)]);   // kFpsWaves <= 16 divides 16: lanes 0..15 hold every wave's
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 15);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 15);
  return ((fps_key)hi << 32) | lo;
}

struct FpsRows {
  float *pts;       // [M][3]
  int32_t *pix;     // [M]
  float *rad;       // [M] or null
  __device__ __forceinline__ void put(int j, float x, float y, float z, int pixel, float r2) const {
    pts[3 * (int64_t)j] = x, pts[3 * (int64_t)j + 1] = y, pts[3 * (int64_t)j + 2] = z;
    pix[j] = pixel;
    if (rad) rad[j] = r2;
  }
};

template <int SRC>
__global__ __launch_bounds__(kFpsWG) void tsdf_fps_kernel(FpsArgs a) {
#pragma clang fp contract(off)
  __shared__ float s_x[kFpsResident], s_y[kFpsResident], s_z[kFpsResident];
  __shared__ fps_key s_key[2][kFpsWaves];
  __shared__ int s_cnt[kFpsWaves];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned i = blockIdx.x;
  const int M = a.M;
  const FpsRows out = {a.out_points + 3 * (int64_t)i * M, a.out_pixel + (int64_t)i * M,
                       a.out_radius2 ? a.out_radius2 + (int64_t)i * M : nullptr};

  // the position's items (everything here is uniform)
  FpsFrame f;
  int64_t items = 0;
  bool ok = true;
  if constexpr (SRC == kFpsCloud32 || SRC == kFpsCloud64) {
    items = a.P;
    f.rows = static_cast<const char *>(a.cloud) + (int64_t)i * a.P * (SRC == kFpsCloud64 ? 24 : 12);
  } else {
    // the source frame; outside the tables it is a bad header and nothing of it is read
    const int64_t g = a.index ? a.index[i] : (int64_t)i;
    ok = g >= 0 && g < a.n_src;
    if (ok) {
      const int32_t *hd = a.headers + 6 * g;
      const int left = hd[2], top = hd[3], right = hd[4], bottom = hd[5];
      const int64_t off0 = a.offsets[g], off1 = a.offsets[g + 1], depth_len = a.depth_len;
      ok = header_ok(left, top, right, bottom, off0, off1, depth_len) && off1 - off0 <= kFpsMaxRank;
      if (ok) {
        items = off1 - off0;
        f.d = a.depth + off0, f.left = left, f.top = top, f.bw = (unsigned)(right - left);
        f.F = a.focal, f.cx = a.cx, f.cy = a.cy, f.eps = a.eps;
        if constexpr (SRC == kFpsMappedCrop) {
#pragma unroll
          for (int k = 0; k < 12; ++k) f.m[k] = a.xforms[24 * (int64_t)i + k];
        }
      }
    }
  }
  const int64_t seg = ok ? fps_segment(items) : 0;

  // 1. count
  const int mine = ok ? fps_walk<SRC>(f, items, seg, wave, lane, 0, [](int, int, float, float, float) {}) : 0;
  if (lane == 0) s_cnt[wave] = mine;
  __syncthreads();
  int base = 0, count = 0;   // at most `items` < 2^31
#pragma unroll
  for (int w = 0; w < kFpsWaves; ++w) {
    const int v = s_cnt[w];
    base += w < wave ? v : 0;
    count += v;
  }

  // 2. the form
  const FpsForm form = count > 0 ? fps_holds(count, a.work != nullptr, a.capacity, a.hint) : kFpsNone;
  if (tid == 0) {
    a.out_count[i] = count;
    a.out_status[i] = !ok ? TSDF_FRAME_BAD_HEADER : count == 0 ? TSDF_FRAME_DEGENERATE
                      : form == kFpsNone ? TSDF_FPS_FRAME_OVER_CAPACITY : TSDF_FRAME_OK;
  }
  if (form == kFpsNone) {
    for (int j = tid; j < M; j += kFpsWG) out.put(j, 0.f, 0.f, 0.f, -1, 0.f);
    return;
  }

  const float inf = __builtin_inff();
  int j = 1;   // the next row
  if (form == kFpsFormResident) {
    // 3. compact into LDS, then into registers
    fps_walk<SRC>(f, items, seg, wave, lane, base, [&](int c, int, float x, float y, float z) { s_x[c] = x, s_y[c] = y, s_z[c] = z; });
    __syncthreads();
    const int slots = fps_slots(count);
    float px[kFpsSlots], py[kFpsSlots], pz[kFpsSlots], pd[kFpsSlots];
#pragma unroll
    for (int k = 0; k < kFpsSlots; ++k) {
      const int c = k * kFpsWG + tid;   // < kFpsResident
      const bool have = c < count;
      // a slot without a candidate is the origin at dist +0: its dist stays +0, and a key of dist +0 wins only when
      // every dist is +0 — then the lowest c wins, which is candidate 0
      px[k] = have ? s_x[c] : 0.f, py[k] = have ? s_y[c] : 0.f, pz[k] = have ? s_z[c] : 0.f;
      pd[k] = have ? inf : 0.f;
    }
    float sx = s_x[0], sy = s_y[0], sz = s_z[0];
    if (tid == 0) out.put(0, sx, sy, sz, 0, inf);
    // 4. the chain
    for (; j < M; ++j) {
      float bd = -1.f;   // every dist is >= +0: slot 0 always takes over
      int bk = 0;
#pragma unroll
      for (int k = 0; k < kFpsSlots; ++k) {
        if (k < slots) {   // uniform
          const float dx = px[k] - sx, dy = py[k] - sy, dz = pz[k] - sz;
          const float d = (dx * dx + dy * dy) + dz * dz;
          const float nd = d < pd[k] ? d : pd[k];
          pd[k] = nd;
          if (nd > bd) bd = nd, bk = k;   // strictly greater: of equal dists the lane's lowest c stays
        }
      }
      const fps_key key = ((fps_key)__float_as_uint(bd) << 32) | ~(unsigned)(bk * kFpsWG + tid);
      const fps_key best = fps_group_max(key, s_key[j & 1], lane, wave);
      if ((unsigned)(best >> 32) == 0u) break;   // every dist is +0: sample 0 from here on
      const unsigned c = ~(unsigned)best;
      sx = s_x[c], sy = s_y[c], sz = s_z[c];
      if (tid == 0) out.put(j, sx, sy, sz, (int)c, __uint_as_float((unsigned)(best >> 32)));
    }
    const float x0 = s_x[0], y0 = s_y[0], z0 = s_z[0];
    for (int r = j + tid; r < M; r += kFpsWG) out.put(r, x0, y0, z0, 0, 0.f);
    // 5. ranks where x was
    __syncthreads();   // every wave has read its last winner
    int *s_rank = reinterpret_cast<int *>(s_x);
    fps_walk<SRC>(f, items, seg, wave, lane, base, [&](int c, int rank, float, float, float) { s_rank[c] = rank; });
    __syncthreads();   // also orders the rows' indices, written by other threads, before their readers
    for (int r = tid; r < M; r += kFpsWG) {
      const unsigned c = (unsigned)out.pix[r];
      out.pix[r] = c < (unsigned)count ? s_rank[c] : -1;   // always in range; the test keeps a wrong index out of LDS
    }
    return;
  }

  // the streaming form: the same steps with the state in the workspace
  fps_f4 *w = reinterpret_cast<fps_f4 *>(a.work) + (int64_t)i * a.capacity;   // count <= capacity
  fps_walk<SRC>(f, items, seg, wave, lane, base, [&](int c, int, float x, float y, float z) {
    fps_f4 v;
    v.x = x, v.y = y, v.z = z, v.w = inf;
    w[c] = v;
  });
  __syncthreads();
  const fps_f4 first = w[0];
  float sx = first.x, sy = first.y, sz = first.z;
  if (tid == 0) out.put(0, sx, sy, sz, 0, inf);
  for (; j < M; ++j) {
    fps_key key = 0;   // a lane without a candidate: below every candidate's key
    float bd = -1.f;
    for (int c = tid; c < count; c += kFpsWG) {   // the lane's own candidates: nobody else touches their dist
      const fps_f4 v = w[c];
      const float dx = v.x - sx, dy = v.y - sy, dz = v.z - sz;
      const float d = (dx * dx + dy * dy) + dz * dz;
      const float nd = d < v.w ? d : v.w;
      reinterpret_cast<float *>(w + c)[3] = nd;
      if (nd > bd) bd = nd, key = ((fps_key)__float_as_uint(nd) << 32) | ~(unsigned)c;
    }
    const fps_key best = fps_group_max(key, s_key[j & 1], lane, wave);
    if ((unsigned)(best >> 32) == 0u) break;
    const unsigned c = ~(unsigned)best;
    const fps_f4 s = w[c];   // x, y, z were written before the barrier above and never since
    sx = s.x, sy = s.y, sz = s.z;
    if (tid == 0) out.put(j, sx, sy, sz, (int)c, __uint_as_float((unsigned)(best >> 32)));
  }
  for (int r = j + tid; r < M; r += kFpsWG) out.put(r, first.x, first.y, first.z, 0, 0.f);
  __syncthreads();   // every dist has had its last reader
  fps_walk<SRC>(f, items, seg, wave, lane, base, [&](int c, int rank, float, float, float) { reinterpret_cast<int *>(w + c)[3] = rank; });
  __syncthreads();
  for (int r = tid; r < M; r += kFpsWG) {
    const unsigned c = (unsigned)out.pix[r];
    out.pix[r] = c < (unsigned)count ? reinterpret_cast<const int *>(w + c)[3] : -1;   // always in range, as above
  }
}

template <int SRC>
int launch(const FpsArgs &a, int n, void *hip_stream) {
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  hipLaunchKernelGGL((tsdf_fps_kernel<SRC>), dim3((unsigned)n), dim3(kFpsWG), 0, static_cast<hipStream_t>(hip_stream), a);
  return launched();
}

void set_out(FpsArgs &a, int M, int64_t capacity, int hint, float *work, float *points, int32_t *pixel, float *radius2,
             int32_t *count, int32_t *status) {
  a.M = M, a.hint = hint, a.capacity = capacity, a.work = work;
  a.out_points = points, a.out_pixel = pixel, a.out_radius2 = radius2, a.out_count = count, a.out_status = status;
}

}  // namespace

extern "C" {

int tsdf_fps_version(void) { return TSDF_FPS_VERSION; }

int tsdf_fps_plan(int M, int64_t capacity, int form_hint, int *resident_cap, int64_t *work_bytes, int *lds_bytes) {
  const FpsOut o = {0, M, capacity, form_hint, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (fps_shape_defect(o) != kFpsGood || !resident_cap || !work_bytes || !lds_bytes) return TSDF_ERR_INVALID_ARG;
  const FpsPlan p = fps_plan(capacity);
  *resident_cap = p.resident_cap;
  *work_bytes = p.work_bytes;
  *lds_bytes = p.lds_bytes;
  return TSDF_OK;
}

int tsdf_fps_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                 int64_t n_src, const int64_t *d_index, int n, int M, double focal, double cx, double cy,
                 float invalid_eps, float trunc_voxels, int64_t capacity, int form_hint, void *hip_stream,
                 const double *d_xforms, float *d_work, float *d_out_points, int32_t *d_out_pixel, float *d_out_radius2,
                 int32_t *d_out_count, int32_t *d_out_status) {
  // arguments first, then the device, then the launch
  const FpsCall c = {d_depth, depth_len, d_offsets, d_headers, n_src, d_index, focal, cx, cy, invalid_eps, trunc_voxels,
                     d_xforms, {n, M, capacity, form_hint, d_work, d_out_points, d_out_pixel, d_out_count, d_out_status}};
  const FpsDefect bad = fps_defect(c);
  if (bad != kFpsGood) return fps_status(bad);
  FpsArgs a = {};
  a.depth = d_depth;
  a.depth_len = depth_len;
  a.offsets = d_offsets;
  a.headers = d_headers;
  a.n_src = n_src;
  a.index = d_index;
  a.focal = focal;
  a.cx = cx;
  a.cy = cy;
  a.eps = invalid_eps;
  a.xforms = d_xforms;
  set_out(a, M, capacity, form_hint, d_work, d_out_points, d_out_pixel, d_out_radius2, d_out_count, d_out_status);
  return d_xforms ? launch<kFpsMappedCrop>(a, n, hip_stream) : launch<kFpsCrop>(a, n, hip_stream);
}

int tsdf_fps_points_hip(const void *d_points, int dtype, int n, int64_t P, int M, int64_t capacity, int form_hint,
                        void *hip_stream, float *d_work, float *d_out_points, int32_t *d_out_pixel,
                        float *d_out_radius2, int32_t *d_out_count, int32_t *d_out_status) {
  const FpsPointsCall c = {d_points, dtype, P,
                           {n, M, capacity, form_hint, d_work, d_out_points, d_out_pixel, d_out_count, d_out_status}};
  const FpsDefect bad = fps_points_defect(c);
  if (bad != kFpsGood) return fps_status(bad);
  FpsArgs a = {};
  a.cloud = d_points;
  a.P = P;
  set_out(a, M, capacity, form_hint, d_work, d_out_points, d_out_pixel, d_out_radius2, d_out_count, d_out_status);
  return dtype == TSDF_FPS_F64 ? launch<kFpsCloud64>(a, n, hip_stream) : launch<kFpsCloud32>(a, n, hip_stream);
}

}  // extern "C"
