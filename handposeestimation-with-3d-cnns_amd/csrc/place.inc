// place.inc — the grid placement under a per-frame map, for a workgroup of WAVES wave64 that owns one batch position:
// tsdf_maplowp.hip (tsdf_map_place_kernel) and tsdf_mapstep.hip (tsdf_map_step_head_kernel) include it (after prim.inc,
// inside their anonymous namespace); the product does not.  Every output bit of the head is contracted to equal the
// placement kernel's, so the arithmetic both run is here, once:
//   place_f4       16 bytes of depth on a 4-byte boundary
//   Ext6           the six running extremes of a lane
//   place_pixel    one pixel: validity, back-projection, the forward map, the extremes
//   wave_min/max   the butterfly over a wave
//   place_crop     the pass over the crop and the wave's seven partials into its row of s_red
//   Placed         what a position's row holds: origin, vl, td, max_l, mid_p, status
//   place_none     the all-zero row of a position that is not OK
//   place_glue     ONE thread: s_red folded over the waves, the float32 glue (phase1.inc::glue, frame.inc::place_grid,
//                  restated operation for operation) and the degenerate rule
// There is no barrier in here: the kernel keeps the one between place_crop and place_glue, and the one that keeps the
// next position's partials out of s_red, under its own uniform conditions.  Where the map comes from, the frame and its
// header, and where the row goes stay in each kernel's file.  Needs finite32 (prim.inc) and the TSDF_FRAME_* codes.
// No device globals.  Compiled with -ffp-contract=off, fma only where __builtin_fma is written.

typedef float place_f4 __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes on a 4-byte boundary

// the running extremes of one lane: a NaN moves neither (the oracle's "v < mn", "v > mx")
struct Ext6 {
  float mn0, mn1, mn2, mx0, mx1, mx2;
};

__device__ __forceinline__ void place_pixel(float d, int col, double yc, double F, double cx, float eps,
                                            const double (&m)[12], Ext6 &e, int &any) {
  if (!(__builtin_fabsf(d) >= eps)) return;   // NaN is invalid
  const double d64 = (double)d;
  const double q = d64 / F;                   // IEEE division
  const double px = q * ((double)col - cx);
  const double py = (-q) * yc;
  const double pz = -d64;
  const float o0 = (float)__builtin_fma(m[0], px, __builtin_fma(m[1], py, __builtin_fma(m[2], pz, m[3])));
  const float o1 = (float)__builtin_fma(m[4], px, __builtin_fma(m[5], py, __builtin_fma(m[6], pz, m[7])));
  const float o2 = (float)__builtin_fma(m[8], px, __builtin_fma(m[9], py, __builtin_fma(m[10], pz, m[11])));
  e.mn0 = o0 < e.mn0 ? o0 : e.mn0;
  e.mn1 = o1 < e.mn1 ? o1 : e.mn1;
  e.mn2 = o2 < e.mn2 ? o2 : e.mn2;
  e.mx0 = o0 > e.mx0 ? o0 : e.mx0;
  e.mx1 = o1 > e.mx1 ? o1 : e.mx1;
  e.mx2 = o2 > e.mx2 ? o2 : e.mx2;
  any = 1;
}

// the extremes held by the lanes of a wave are never NaN: fminf / fmaxf are the plain minimum and maximum
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) v = __builtin_fminf(v, __shfl_xor(v, k, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, k, 64));
  return v;
}

// One pass over the crop d[bh][bw] whose first pixel is (left, top), under the forward rows m of the position's map:
// wave <-> rows, lane <-> groups of four consecutive columns, one 16-byte load per group, the bw mod 4 last columns one by
// one; then the butterfly, and lane 0 leaves the wave's partials in s_red[wave]: min xyz, max xyz, any.  Minimum and
// maximum are order-free, so any split of the pixels gives the same bits.  bw and bh are positive (header_ok).
template <int WAVES>
__device__ __forceinline__ void place_crop(const float *__restrict__ d, int left, int top, int bw, int bh, double F,
                                           double cx, double cy, float eps, const double (&m)[12], int lane, int wave,
                                           float (&s_red)[WAVES][8]) {
#pragma clang fp contract(off)
  const float inf = __builtin_inff();
  Ext6 e = {inf, inf, inf, -inf, -inf, -inf};
  int any = 0;
  const int ngrp = bw >> 2, tail0 = ngrp << 2, ntail = bw - tail0;
  // gl lanes per row: the smallest power of two that holds the row's groups (4..64), so a wave takes 64 / gl rows at a
  // time and a crop of 130 columns keeps all 64 lanes busy, not 32 (uniform)
  int sh = 6;
  while (sh > 2 && (1 << (sh - 1)) >= ngrp) --sh;
  const int gl = 1 << sh, rpw = 64 >> sh;
  const int sub = lane >> sh, gq = lane & (gl - 1);
  for (int r = wave * rpw + sub; r < bh; r += WAVES * rpw) {
    const float *__restrict__ row = d + (int64_t)r * bw;
    const double yc = (double)(top + r) - cy;
    for (int q = gq; q < ngrp; q += gl) {
      const place_f4 v = *reinterpret_cast<const place_f4 *>(row + 4 * q);
      const int c0 = left + 4 * q;
      place_pixel(v.x, c0, yc, F, cx, eps, m, e, any);
      place_pixel(v.y, c0 + 1, yc, F, cx, eps, m, e, any);
      place_pixel(v.z, c0 + 2, yc, F, cx, eps, m, e, any);
      place_pixel(v.w, c0 + 3, yc, F, cx, eps, m, e, any);
    }
    if (gq < ntail) place_pixel(row[tail0 + gq], left + tail0 + gq, yc, F, cx, eps, m, e, any);
  }
  const float w0 = wave_min(e.mn0), w1 = wave_min(e.mn1), w2 = wave_min(e.mn2);
  const float w3 = wave_max(e.mx0), w4 = wave_max(e.mx1), w5 = wave_max(e.mx2);
  const float w6 = wave_max((float)any);
  if (lane == 0) {
    s_red[wave][0] = w0, s_red[wave][1] = w1, s_red[wave][2] = w2;
    s_red[wave][3] = w3, s_red[wave][4] = w4, s_red[wave][5] = w5;
    s_red[wave][6] = w6;
  }
}

// a position's row
struct Placed {
  float ox, oy, oz, vl, td;   // grid origin, voxel length, truncation distance
  float max_l;                // the cube's edge
  float m0, m1, m2;           // mid_p
  int status;                 // TSDF_FRAME_*
};

// a row that is not OK is all zero
__device__ __forceinline__ Placed place_none(int status) {
  return Placed{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, status};
}

// What one thread makes of the waves' partials once a barrier has put them in s_red.
template <int WAVES>
__device__ __forceinline__ Placed place_glue(const float (&s_red)[WAVES][8], int R, float trunc_vox) {
#pragma clang fp contract(off)
  float mn0 = s_red[0][0], mn1 = s_red[0][1], mn2 = s_red[0][2];
  float mx0 = s_red[0][3], mx1 = s_red[0][4], mx2 = s_red[0][5], anyf = s_red[0][6];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) {
    mn0 = __builtin_fminf(mn0, s_red[w][0]);
    mn1 = __builtin_fminf(mn1, s_red[w][1]);
    mn2 = __builtin_fminf(mn2, s_red[w][2]);
    mx0 = __builtin_fmaxf(mx0, s_red[w][3]);
    mx1 = __builtin_fmaxf(mx1, s_red[w][4]);
    mx2 = __builtin_fmaxf(mx2, s_red[w][5]);
    anyf = __builtin_fmaxf(anyf, s_red[w][6]);
  }
  if (!(anyf > 0.f)) return place_none(TSDF_FRAME_DEGENERATE);   // no valid pixel
  // the glue: float32, one rounding per operation, left to right
  float mid0 = __fdiv_rn(__fadd_rn(mn0, mx0), 2.0f), len0 = __fsub_rn(mx0, mn0);
  float mid1 = __fdiv_rn(__fadd_rn(mn1, mx1), 2.0f), len1 = __fsub_rn(mx1, mn1);
  float mid2 = __fdiv_rn(__fadd_rn(mn2, mx2), 2.0f), len2 = __fsub_rn(mx2, mn2);
  float max_l = len0;
  if (len1 > max_l) max_l = len1;
  if (len2 > max_l) max_l = len2;
  float vl = __fdiv_rn(max_l, (float)R);
  float td = __fmul_rn(vl, trunc_vox);
  const float half_l = __fdiv_rn(max_l, 2.0f), half_v = __fdiv_rn(vl, 2.0f);
  float ox = __fadd_rn(__fsub_rn(mid0, half_l), half_v);
  float oy = __fadd_rn(__fsub_rn(mid1, half_l), half_v);
  float oz = __fadd_rn(__fsub_rn(mid2, half_l), half_v);
  // the degenerate rule: the extent positive and finite, the centre finite
  const bool ext_ok = max_l > 0.f && finite32(max_l);
  const bool mid_ok = finite32(mid0) && finite32(mid1) && finite32(mid2);
  int status = TSDF_FRAME_OK;
  if (!ext_ok || !mid_ok) {
    status = TSDF_FRAME_DEGENERATE;
    max_l = ox = oy = oz = vl = td = 0.f;
    if (!mid_ok) mid0 = mid1 = mid2 = 0.f;   // a zero extent keeps its finite centre
  }
  return Placed{ox, oy, oz, vl, td, max_l, mid0, mid1, mid2, status};
}
