// cloud.inc — part of the one translation unit tsdf_hip.hip (included there, inside its anonymous namespace).
// tsdf_point_clouds_hip: back-project every valid pixel of a crop and resample the cloud to P points
// (pre/process.py:30-84, DataProcess.point_cloud + set_length) with a counter-based generator; the contract is in
// include/tsdf.h.  Independent of the voxelizer kernels: nothing here is shared with or changes them.
//
// One workgroup owns slots [lo, hi) of one frame (a frame's P slots are split over `split` workgroups when the batch is
// small compared with the CU count; each of them rebuilds the frame's bitmap, the crop is cheap to re-read).
//   1. Bitmap: the crop is read once, one float per lane, eight 64-pixel chunks per wave in flight; __ballot(d != 0)
//      gives chunk c's validity word, kept in LDS with the exclusive running count of valid pixels before it.
//   2. Slots: slot j's rank (its valid pixel's position in row-major order) is j itself or the hash draw; a binary
//      search over the running counts finds the chunk, a select of the k-th set bit the pixel.  The points of one
//      tile of 512 slots are staged in LDS and written as coalesced float64 stores (a wave writes 512 contiguous bytes).
//   A crop of more than kCloudWin chunks (98304 pixels: a 320x240 frame still fits) is taken in windows of kCloudWin
//   chunks: a counting pass over the whole crop gives m first, then every window is built in turn and each slot whose
//   rank falls inside it is resolved there and stored directly.  Same arithmetic, same result; the crop is read twice.

constexpr int kCloudWG = 512;                        // threads per workgroup (8 wave64)
constexpr int kCloudWaves = kCloudWG / 64;
constexpr int kCloudUnroll = 8;                      // chunks per wave in flight while the bitmap is built
constexpr int kCloudPerThread = 3;                   // chunks per thread in the running-count scan
constexpr int kCloudWin = kCloudWG * kCloudPerThread;  // chunks of 64 pixels per LDS window (98304 pixels)

struct CloudArgs {
  const float *depth;
  int64_t depth_len;
  const int64_t *offsets;
  const int32_t *headers;
  int n, P;
  int split;       // workgroups per frame
  int per;         // slots per workgroup (a multiple of kCloudWG)
  double focal;
  uint64_t seed;
  int64_t frame_base;
  const double *xforms;  // [n][24] or null
  double *out;           // [n][P][3]
  int32_t *count, *status;  // [n] or null
};

// splitmix64, every operation mod 2^64
__device__ __forceinline__ uint64_t cloud_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// k(j) = ((u >> 32) * m) >> 32 with u = mix(h + j), h = mix(seed + g): the 96-bit product taken exactly
__device__ __forceinline__ uint64_t cloud_draw(uint64_t h, uint64_t j, uint64_t m) {
  const uint64_t u = cloud_mix(h + j) >> 32;
  return (__umul64hi(u, m) << 32) | ((u * m) >> 32);
}

// position of the (r+1)-th set bit of w (r < popcount(w))
__device__ __forceinline__ int cloud_select_bit(uint64_t w, unsigned r) {
  int pos = 0;
  unsigned c = __popc((unsigned)w);
  if (r >= c) { r -= c; w >>= 32; pos += 32; }
  c = __popc((unsigned)w & 0xffffu);
  if (r >= c) { r -= c; w >>= 16; pos += 16; }
  c = __popc((unsigned)w & 0xffu);
  if (r >= c) { r -= c; w >>= 8; pos += 8; }
  c = __popc((unsigned)w & 0xfu);
  if (r >= c) { r -= c; w >>= 4; pos += 4; }
  c = __popc((unsigned)w & 0x3u);
  if (r >= c) { r -= c; w >>= 2; pos += 2; }
  return pos + (r >= ((unsigned)w & 1u) ? 1 : 0);
}

// Bitmap of chunks [c0, c0 + nc) of the crop (nc <= kCloudWin) into s_mask / s_pre; returns the window's valid pixels.
// Ends with a workgroup barrier.
__device__ __forceinline__ unsigned cloud_build_window(const float *__restrict__ d, int64_t px, int64_t c0, int nc,
                                                       unsigned long long *s_mask, unsigned *s_pre, unsigned *s_wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int cb = wave * kCloudUnroll; cb < nc; cb += kCloudWaves * kCloudUnroll) {
    float v[kCloudUnroll];
#pragma unroll
    for (int u = 0; u < kCloudUnroll; ++u) {
      const int64_t p = (c0 + cb + u) * 64 + lane;
      v[u] = (cb + u < nc && p < px) ? d[p] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kCloudUnroll; ++u) {
      const unsigned long long b = __ballot(v[u] != 0.f);   // NaN != 0: a NaN pixel is valid (pre/process.py:62-64)
      if (lane == 0 && cb + u < nc) s_mask[cb + u] = b;
    }
  }
  __syncthreads();
  unsigned cnt[kCloudPerThread], sum = 0;
#pragma unroll
  for (int q = 0; q < kCloudPerThread; ++q) {
    const int c = threadIdx.x * kCloudPerThread + q;
    cnt[q] = c < nc ? (unsigned)__popcll(s_mask[c]) : 0u;
    sum += cnt[q];
  }
  unsigned incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned y = __shfl_up(incl, o);
    if (lane >= o) incl += y;
  }
  if (lane == 63) s_wsum[wave] = incl;
  __syncthreads();
  unsigned before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kCloudWaves; ++w) {
    const unsigned x = s_wsum[w];
    before += w < wave ? x : 0u;
    total += x;
  }
  unsigned run = before + incl - sum;
#pragma unroll
  for (int q = 0; q < kCloudPerThread; ++q) {
    const int c = threadIdx.x * kCloudPerThread + q;
    if (c < nc) s_pre[c] = run;
    run += cnt[q];
  }
  __syncthreads();
  return total;
}

// valid pixels of the whole crop (the counting pass of a crop larger than one window)
__device__ __forceinline__ uint64_t cloud_count(const float *__restrict__ d, int64_t px, unsigned long long *s_red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nch = (px + 63) >> 6;
  uint64_t m = 0;
  for (int64_t cb = (int64_t)wave * kCloudUnroll; cb < nch; cb += kCloudWaves * kCloudUnroll) {
    float v[kCloudUnroll];
#pragma unroll
    for (int u = 0; u < kCloudUnroll; ++u) {
      const int64_t p = (cb + u) * 64 + lane;
      v[u] = p < px ? d[p] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kCloudUnroll; ++u) m += (uint64_t)__popcll(__ballot(v[u] != 0.f));
  }
  if (lane == 0) s_red[wave] = m;
  __syncthreads();
  m = 0;
#pragma unroll
  for (int w = 0; w < kCloudWaves; ++w) m += s_red[w];
  __syncthreads();
  return m;
}

// The point of crop pixel p: float64, one rounding per operation, no fma (include/tsdf.h); with a map, its forward rows
// as (A_i0 x + A_i1 y) + (A_i2 z + b_i).
__device__ __forceinline__ void cloud_point(const float *__restrict__ d, int64_t p, int64_t bw, const CloudArgs &a,
                                            double half_w, double half_h, int left, int top,
                                            const double *__restrict__ xf, double o[3]) {
#pragma clang fp contract(off)
  const int64_t r = p / bw, c = p - r * bw;
  const double dv = (double)d[p];
  const double x = ((((double)c + (double)left) - half_w) * dv) / a.focal;
  const double y = (-((((double)r + (double)top) - half_h) * dv)) / a.focal;
  const double z = -dv;
  if (xf) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double s0 = xf[4 * k] * x + xf[4 * k + 1] * y;
      const double s1 = xf[4 * k + 2] * z + xf[4 * k + 3];
      o[k] = s0 + s1;
    }
  } else {
    o[0] = x;
    o[1] = y;
    o[2] = z;
  }
}

__global__ __launch_bounds__(kCloudWG) void tsdf_point_cloud_kernel(CloudArgs a) {
  __shared__ unsigned long long s_mask[kCloudWin];
  __shared__ unsigned s_pre[kCloudWin];
  __shared__ double s_stage[3 * kCloudWG];
  __shared__ unsigned long long s_red[kCloudWaves];
  __shared__ unsigned s_wsum[kCloudWaves];

  const int tid = threadIdx.x;
  const int64_t i = blockIdx.x / a.split;
  const int s = (int)(blockIdx.x - i * a.split);
  const int64_t lo = (int64_t)s * a.per;
  const int64_t hi = lo + a.per < a.P ? lo + a.per : a.P;
  double *__restrict__ out = a.out + i * (int64_t)a.P * 3;

  const int32_t *hd = a.headers + 6 * i;
  const int W = hd[0], H = hd[1], left = hd[2], top = hd[3];
  const int64_t off0 = a.offsets[i], off1 = a.offsets[i + 1];
  const int64_t bw = (int64_t)hd[4] - left, bh = (int64_t)hd[5] - top;
  // the voxelizer's header rule (frame_from_header); a bad frame's depth is not read
  const bool hdr_ok = bw > 0 && bh > 0 && bw <= 0x7fffffff && bh <= 0x7fffffff && bw * bh == off1 - off0 &&
                      off0 >= 0 && off1 <= a.depth_len;
  const float *__restrict__ d = a.depth + (hdr_ok ? off0 : 0);
  const int64_t px = hdr_ok ? bw * bh : 0;
  const int64_t nch = (px + 63) >> 6;
  const int64_t nwin = (nch + kCloudWin - 1) / kCloudWin;

  uint64_t m = 0;
  unsigned wcount = 0;
  if (nwin == 1) {
    wcount = cloud_build_window(d, px, 0, (int)nch, s_mask, s_pre, s_wsum);
    m = wcount;
  } else if (nwin > 1) {
    m = cloud_count(d, px, s_red);
  }
  if (s == 0 && tid == 0) {
    if (a.status) a.status[i] = !hdr_ok ? TSDF_FRAME_BAD_HEADER : m == 0 ? TSDF_FRAME_DEGENERATE : TSDF_FRAME_OK;
    if (a.count) a.count[i] = m > 0x7fffffffull ? 0x7fffffff : (int32_t)m;
  }
  if (m == 0) {   // bad header or no valid pixel: all-zero rows
    for (int64_t q = lo * 3 + tid; q < hi * 3; q += kCloudWG) out[q] = 0.0;
    return;
  }

  const double half_w = (double)W / 2.0, half_h = (double)H / 2.0;
  const double *__restrict__ xf = a.xforms ? a.xforms + 24 * i : nullptr;
  const uint64_t h = cloud_mix(a.seed + (uint64_t)a.frame_base + (uint64_t)i);
  const bool keep_all = m < (uint64_t)a.P;   // slots j < m take valid pixel j (pre/process.py:74-79)
  uint64_t base = 0;
  for (int64_t w = 0; w < nwin; ++w) {
    int nc = (int)nch;
    if (nwin > 1) {
      const int64_t c0 = w * kCloudWin;
      nc = (int)(nch - c0 < kCloudWin ? nch - c0 : kCloudWin);
      wcount = cloud_build_window(d + c0 * 64, px - c0 * 64, 0, nc, s_mask, s_pre, s_wsum);
    }
    for (int64_t t0 = lo; t0 < hi; t0 += kCloudWG) {
      const int64_t j = t0 + tid;
      double o[3] = {0.0, 0.0, 0.0};
      bool have = false;
      if (j < hi) {
        const uint64_t rank = (keep_all && (uint64_t)j < m) ? (uint64_t)j : cloud_draw(h, (uint64_t)j, m);
        if (rank >= base && rank < base + wcount) {
          const unsigned r = (unsigned)(rank - base);
          int b0 = 0, b1 = nc;   // the last chunk whose running count is <= r
          while (b1 - b0 > 1) {
            const int mid = (b0 + b1) >> 1;
            if (s_pre[mid] <= r) b0 = mid;
            else b1 = mid;
          }
          const int64_t p = (w * kCloudWin + b0) * 64 + cloud_select_bit(s_mask[b0], r - s_pre[b0]);
          cloud_point(d, p, bw, a, half_w, half_h, left, top, xf, o);
          have = true;
        }
      }
      if (nwin == 1) {   // one window resolves every slot: stage the tile, then coalesced stores
        s_stage[3 * tid] = o[0];
        s_stage[3 * tid + 1] = o[1];
        s_stage[3 * tid + 2] = o[2];
        __syncthreads();
        const int64_t nt3 = 3 * ((hi - t0) < kCloudWG ? (hi - t0) : kCloudWG);
        for (int64_t q = tid; q < nt3; q += kCloudWG) out[t0 * 3 + q] = s_stage[q];
        __syncthreads();
      } else if (have) {
        out[j * 3] = o[0];
        out[j * 3 + 1] = o[1];
        out[j * 3 + 2] = o[2];
      }
    }
    base += wcount;
    __syncthreads();   // the next window overwrites the bitmap
  }
}

// Host side of tsdf_point_clouds_hip.  Arguments are checked before the device is looked at.
int run_point_clouds(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers, int n,
                     int points, const tsdf_cam *cam, uint64_t seed, int64_t frame_base, const double *d_xforms,
                     void *hip_stream, double *d_out_points, int32_t *d_out_count, int32_t *d_out_status) {
  if (n < 0 || points < 1 || !d_out_points) return TSDF_ERR_INVALID_ARG;
  if (misaligned(d_xforms, 7)) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_depth || !d_offsets || !d_headers || depth_len < 0) return TSDF_ERR_INVALID_ARG;
  if (!cam_ok(cam)) return TSDF_ERR_INVALID_ARG;   // the whole camera, though only focal is read
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  // split a frame's slots over workgroups until the launch has about two workgroups per CU
  const int tiles = (points + kCloudWG - 1) / kCloudWG;
  const int64_t want = (2 * (int64_t)num_cus() + n - 1) / n;
  int split = (int)(want < tiles ? want : tiles);
  if (split < 1) split = 1;
  const int per = ((tiles + split - 1) / split) * kCloudWG;
  split = (points + per - 1) / per;
  const int64_t blocks = (int64_t)n * split;
  if (blocks > 0x7fffffff) return TSDF_ERR_INVALID_ARG;
  CloudArgs a;
  a.depth = d_depth;
  a.depth_len = depth_len;
  a.offsets = d_offsets;
  a.headers = d_headers;
  a.n = n;
  a.P = points;
  a.split = split;
  a.per = per;
  a.focal = cam ? cam->focal : kDefaultCam.focal;
  a.seed = seed;
  a.frame_base = frame_base;
  a.xforms = d_xforms;
  a.out = d_out_points;
  a.count = d_out_count;
  a.status = d_out_status;
  hipLaunchKernelGGL(tsdf_point_cloud_kernel, dim3((unsigned)blocks), dim3(kCloudWG), 0,
                     static_cast<hipStream_t>(hip_stream), a);
  return launched();
}
