// cloudgrid.inc — part of the one translation unit tsdf_hip.hip (included there, inside its anonymous namespace).
// tsdf_cloud_grid_hip: the grid placement of tsdf_f(data, point_cloud) (pre/tsdf_for.py:9-16,23-41) for n clouds that
// are already on the device — the extremes of max_min_point, then the float32 glue of phase1.inc.  The contract is in
// include/tsdf.h.  Independent of the voxelizer and point-cloud kernels: it calls glue() and the DPP helpers, which are
// inlined, and changes nothing of theirs.
//
// One workgroup owns one frame: a stream of P*24 bytes read once, 60 bytes written.  The frame is taken as 16-byte
// chunks of two doubles, lane <-> consecutive chunks, so a wave's load is 1 KiB contiguous.  A chunk holds (x,y), (z,x)
// or (y,z) according to its index mod 3; the workgroup has 768 threads, a multiple of 3, so a lane meets ONE kind of
// chunk in every round and keeps plain (first double, second double) extremes that are given their axes once, after the
// loop.  kCgUnroll loads per lane are issued back to back before the first is used.  Values are converted to float32
// first and reduced in float32 (rounding to nearest is monotone, so the extremes are those of the float64 reduction,
// rounded); a NaN is counted on its own and kept out of the v_min / v_max chain.

constexpr int kCgWG = 768;                 // threads per workgroup: 12 wave64, a multiple of 3 (see above)
constexpr int kCgWaves = kCgWG / 64;
constexpr int kCgUnroll = 8;               // 16-byte loads per lane in flight
constexpr int kCgRed = 8;                  // floats per wave in the LDS combine: 3 minima, 3 maxima, NaN flag, pad

typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));   // 8-byte-aligned 16-B access

struct CloudGridArgs {
  const double *points;   // [n][P][3]
  int P, R;
  float trunc_vox;
  float *grid;            // [n][8]
  float *max_l;           // [n]
  float *mid_p;           // [n][3]
  float *aabb;            // [n][6] or null
  int32_t *status;        // [n] or null
};

// One coordinate into a (min, max) pair.  `isz`: the coordinate is a z, dropped when the float64 value is 0
// (pre/tsdf_for.py:29: -0.0 is dropped, a denormal is kept and rounds to +-0).  NaN (never equal to 0, so never
// dropped) raises `nan` and enters neither extreme.
__device__ __forceinline__ void cg_take(double v, bool isz, float &mn, float &mx, bool &nan) {
  const bool is_nan = v != v;
  const bool keep = !is_nan && (!isz || v != 0.0);
  const float f = (float)v;
  nan |= is_nan;
  mn = vmin(mn, keep ? f : TSDF_INF);
  mx = vmax(mx, keep ? f : -TSDF_INF);
}

__global__ __launch_bounds__(kCgWG) void tsdf_cloud_grid_kernel(CloudGridArgs a) {
  __shared__ float s_red[kCgWaves * kCgRed];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i = blockIdx.x;
  const double *__restrict__ src = a.points + i * (int64_t)a.P * 3;
  const int64_t nd = (int64_t)a.P * 3;     // doubles of the frame
  const int64_t chunks = nd >> 1;          // whole 16-byte chunks; an odd P leaves one z behind them
  const int kind = tid % 3;                // chunk c holds doubles 2c, 2c+1: components (2c) % 3 and (2c+1) % 3
  const bool z0 = kind == 1, z1 = kind == 2;   // kind 0: (x,y)   1: (z,x)   2: (y,z)

  float mn0 = TSDF_INF, mx0 = -TSDF_INF, mn1 = TSDF_INF, mx1 = -TSDF_INF;
  bool nan = false;
  if (tid < chunks) {
    for (int64_t c0 = tid; c0 < chunks; c0 += (int64_t)kCgWG * kCgUnroll) {
      d2u v[kCgUnroll];
#pragma unroll
      for (int u = 0; u < kCgUnroll; ++u) {
        const int64_t c = c0 + (int64_t)kCgWG * u;
        // past the end: the lane's first chunk of this round again (same kind; a repeat changes no extreme)
        v[u] = *reinterpret_cast<const d2u *>(src + 2 * (c < chunks ? c : c0));
      }
#pragma unroll
      for (int u = 0; u < kCgUnroll; ++u) {
        cg_take(v[u].x, z0, mn0, mx0, nan);
        cg_take(v[u].y, z1, mn1, mx1, nan);
      }
    }
  }
  if ((nd & 1) && tid == 1) cg_take(src[nd - 1], true, mn0, mx0, nan);   // the last z of an odd P (kind 1: first = z)

  // (first, second) -> axes
  const float lo[3] = {kind == 0 ? mn0 : kind == 1 ? mn1 : TSDF_INF,     // x
                       kind == 0 ? mn1 : kind == 2 ? mn0 : TSDF_INF,     // y
                       kind == 1 ? mn0 : kind == 2 ? mn1 : TSDF_INF};    // z
  const float hi[3] = {kind == 0 ? mx0 : kind == 1 ? mx1 : -TSDF_INF,
                       kind == 0 ? mx1 : kind == 2 ? mx0 : -TSDF_INF,
                       kind == 1 ? mx0 : kind == 2 ? mx1 : -TSDF_INF};
  float part[7];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    part[k] = wave_min(lo[k]);
    part[3 + k] = wave_max(hi[k]);
  }
  part[6] = __ballot(nan) ? 1.f : 0.f;
  if (lane < 7) {
    float v = part[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) v = (lane == k) ? part[k] : v;
    s_red[wave * kCgRed + lane] = v;
  }
  __syncthreads();
  if (wave != 0) return;
  static_assert(kCgWaves <= 16, "the cross-wave reduction uses one 16-lane DPP row");
  const bool has = (lane & 15) < kCgWaves;
  const int at = has ? (lane & 15) * kCgRed : 0;
  float mn[3], mx[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    mn[k] = row0_min(has ? s_red[at + k] : TSDF_INF);
    mx[k] = row0_max(has ? s_red[at + 3 + k] : -TSDF_INF);
  }
  const bool any_nan = row0_max(has ? s_red[at + 6] : 0.f) != 0.f;
  if (tid != 0) return;

  // glue and the not-OK rule of include/tsdf.h (the voxelizer's place_grid rule, plus NaN and "no z")
  const bool any = mn[2] <= mx[2];         // some point has z != 0 (x and y are never empty: P >= 1)
  int status = TSDF_FRAME_OK;
  Grid g;
  g.max_l = g.voxel_len = g.trunc = 0.f;
  g.mid[0] = g.mid[1] = g.mid[2] = g.ori[0] = g.ori[1] = g.ori[2] = 0.f;
  if (any_nan || !any) {
    status = TSDF_FRAME_DEGENERATE;
  } else {
    CamK k{};
    k.trunc_vox = a.trunc_vox;
    g = glue(mn, mx, a.R, k);
    const bool mid_ok = finite32(g.mid[0]) && finite32(g.mid[1]) && finite32(g.mid[2]);
    if (!(g.max_l > 0.f) || !(g.max_l < TSDF_INF) || !mid_ok) {
      status = TSDF_FRAME_DEGENERATE;
      g.max_l = g.voxel_len = g.trunc = 0.f;
      g.ori[0] = g.ori[1] = g.ori[2] = 0.f;
      if (!mid_ok) g.mid[0] = g.mid[1] = g.mid[2] = 0.f;
    }
  }
  float *q = a.grid + 8 * i;
  q[0] = g.ori[0]; q[1] = g.ori[1]; q[2] = g.ori[2];
  q[3] = g.voxel_len; q[4] = g.trunc; q[5] = 0.f; q[6] = 0.f; q[7] = 0.f;
  a.max_l[i] = g.max_l;
  a.mid_p[3 * i + 0] = g.mid[0];
  a.mid_p[3 * i + 1] = g.mid[1];
  a.mid_p[3 * i + 2] = g.mid[2];
  if (a.status) a.status[i] = status;
  if (a.aabb) {
    // the extremes as reduced; a frame with a NaN or without any z != 0 gets a zero row
    const bool z = any_nan || !any;
    float *o = a.aabb + 6 * i;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      o[k] = z ? 0.f : mn[k];
      o[3 + k] = z ? 0.f : mx[k];
    }
  }
}

// Host side of tsdf_cloud_grid_hip.  Arguments are checked before the device is looked at.
int run_cloud_grid(const double *d_points, int n, int points, int R, const tsdf_cam *cam, void *hip_stream,
                   float *d_out_grid, float *d_out_max_l, float *d_out_mid_p, float *d_out_aabb, int32_t *d_out_status) {
  if (n < 0 || points < 1 || !tsdf_resolution_supported(R)) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_points || !d_out_grid || !d_out_max_l || !d_out_mid_p) return TSDF_ERR_INVALID_ARG;
  if (misaligned(d_points, 7)) return TSDF_ERR_INVALID_ARG;
  if (!cam_ok(cam)) return TSDF_ERR_INVALID_ARG;   // the whole camera, though only trunc_voxels is read
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  CloudGridArgs a;
  a.points = d_points;
  a.P = points;
  a.R = R;
  a.trunc_vox = cam ? cam->trunc_voxels : kDefaultCam.trunc_voxels;
  a.grid = d_out_grid;
  a.max_l = d_out_max_l;
  a.mid_p = d_out_mid_p;
  a.aabb = d_out_aabb;
  a.status = d_out_status;
  hipLaunchKernelGGL(tsdf_cloud_grid_kernel, dim3((unsigned)n), dim3(kCgWG), 0, static_cast<hipStream_t>(hip_stream), a);
  return launched();
}
