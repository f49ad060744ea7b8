// common.inc — part of the one translation unit tsdf_hip.hip (included there, inside its anonymous namespace).
// Constants, types, VALU / DPP / float64 helpers shared by every phase.

constexpr int kWG = 1024;               // threads per workgroup (16 wave64; needs <= 128 VGPRs)
// Groups per workgroup: each walks its own frames (see the kernel).  A template parameter of the fused kernel, chosen
// per resolution (groups_for): two 512-thread groups at 32^3 — one's row stream hides behind the other's voxel pass —,
// ONE 1024-thread group from 48^3 upwards, where the voxel pass is 8x the row stream and what counts is that a CU
// writes each channel plane of its volume as one sequential run (paired A/B on 1024 full frames -> 64^3: plain -3.7 %,
// augmented -4.3 %; at 32^3 one group is +8 % on full frames, +13 % on crops).  The names below are the defaults of code
// outside the fused kernel (stamps; the split kernel's LDS layout); inside it they are shadowed by the instantiation's
// own values.
constexpr int kGroups = 2;
constexpr int kMaxGroups = 2;
constexpr int kGW = kWG / kGroups;      // threads per group
[[maybe_unused]] constexpr int kGWaves = kGW / 64;  // waves per group
constexpr int groups_for(int R) { return R >= 48 ? 1 : 2; }
constexpr int kMaxR = 128;
constexpr int kTabR = 32;               // projection tables for R <= kTabR (2 + 4 KiB per group)
constexpr int kRedStride = 12;
constexpr int kLdsBytes = 160 * 1024;   // LDS of one gfx950 CU; the workgroup takes all of it
constexpr int kMaxRows = 256;           // rows per frame the row table holds (MSRA: 240)
constexpr int kMaxCapW = 320;           // widest bounding box whose rows the split kernel captures (= one row pass)

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));  // dword-aligned 16-B access

struct CamK {
  double focal, cx, cy, inv_focal;
  float eps, trunc_vox;
};

#define TSDF_INF __builtin_inff()

// In-kernel timeline stamps: compiled only into the diagnostic library (make stamps), never into
// libtsdf_hip.so.  Lane 0 of wave 0 of each workgroup records s_memrealtime (100 MHz) per phase.
#ifdef TSDF_STAMPS
constexpr int kStampSlots = 16, kStampFrames = 8, kStampBlocks = 512;
__device__ unsigned long long g_stamps[kStampBlocks * kStampFrames * kStampSlots];
#define TSDF_STAMP(iter, slot)                                                                       \
  do {                                                                                               \
    if ((threadIdx.x & (kGW - 1)) == 0 && blockIdx.x < kStampBlocks && (iter) < kStampFrames)                      \
      g_stamps[(blockIdx.x * kStampFrames + (iter)) * kStampSlots + (slot)] =                        \
          __builtin_amdgcn_s_memrealtime();                                                          \
  } while (0)
#define TSDF_STAMP_VAL(iter, slot, val)                                                              \
  do {                                                                                               \
    if ((threadIdx.x & (kGW - 1)) == 0 && blockIdx.x < kStampBlocks && (iter) < kStampFrames)                      \
      g_stamps[(blockIdx.x * kStampFrames + (iter)) * kStampSlots + (slot)] = (val);                 \
  } while (0)
// per-wave stamps: every wave's lane 0 records when it enters (which = 0) and leaves (1) the voxel pass
__device__ unsigned long long g_wstamps[kStampBlocks * kStampFrames * 16 * 2];
#define TSDF_WSTAMP(iter, which)                                                                     \
  do {                                                                                               \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < kStampBlocks && (iter) < kStampFrames)               \
      g_wstamps[((blockIdx.x * kStampFrames + (iter)) * 16 + (threadIdx.x >> 6)) * 2 + (which)] =    \
          __builtin_amdgcn_s_memrealtime();                                                          \
  } while (0)
#else
#define TSDF_STAMP(iter, slot) do { } while (0)
#define TSDF_STAMP_VAL(iter, slot, val) do { } while (0)
#define TSDF_WSTAMP(iter, which) do { } while (0)
#endif

// ---- raw VALU min/max (no canonicalising v_max x,x,x in front; operands here are never NaN) ----
__device__ __forceinline__ float vmin(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float vmax(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float vmin3(float a, float b, float c) {
  float r;
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ float vmax3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// min(|a|, b): the absolute value is a source modifier, not an instruction
__device__ __forceinline__ float vminabs(float a, float b) {
  float r;
  asm("v_min_f32 %0, |%1|, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// ---- wave64 reductions: one DPP VALU op per step (s_nop 1 covers the VALU-write -> DPP-read hazard;
// lanes whose DPP source is out of range are write-disabled and keep their value) ----------------
#define TSDF_DPP_REDUCE(OP)                                                             \
  asm("s_nop 1\n\t" OP " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"           \
      "s_nop 1\n\t" OP " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"           \
      "s_nop 1\n\t" OP " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"           \
      "s_nop 1\n\t" OP " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"           \
      "s_nop 1\n\t" OP " %0, %0, %0 row_bcast:15 row_mask:0xf bank_mask:0xf\n\t"        \
      "s_nop 1\n\t" OP " %0, %0, %0 row_bcast:31 row_mask:0xf bank_mask:0xf\n\t"        \
      "s_nop 1"                                                                         \
      : "+v"(v))
#define TSDF_DPP_REDUCE16(OP)                                                           \
  asm("s_nop 1\n\t" OP " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"           \
      "s_nop 1\n\t" OP " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"           \
      "s_nop 1\n\t" OP " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"           \
      "s_nop 1\n\t" OP " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"           \
      "s_nop 1"                                                                         \
      : "+v"(v))

__device__ __forceinline__ float wave_min(float v) {  // result in every lane (wave-uniform)
  TSDF_DPP_REDUCE("v_min_f32_dpp");
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_max(float v) {
  TSDF_DPP_REDUCE("v_max_f32_dpp");
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
// reduce lanes 0..15 only (first DPP row); result wave-uniform
__device__ __forceinline__ float row0_min(float v) {
  TSDF_DPP_REDUCE16("v_min_f32_dpp");
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 15));
}
__device__ __forceinline__ float row0_max(float v) {
  TSDF_DPP_REDUCE16("v_max_f32_dpp");
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 15));
}

// ---- exact float64 helpers (never contracted) ----------------------------------------------
// (a * b) + c with two roundings: pre/tsdf_numba.py:31-32 as numba types it (App. A.3).
__device__ __forceinline__ double mul_then_add(double a, double b, double c) {
#pragma clang fp contract(off)
  double p = a * b;
  return p + c;
}

// Forward map, one row {A_i0, A_i1, A_i2, b_i}: o = fma(A_i0, x, fma(A_i1, y, fma(A_i2, z, b_i))) — the augmented
// form's arithmetic contract (oracle/tsdf_oracle.c::affine3_fwd).  Three instructions per row; with the
// identity row {1,0,0,0} it returns x exactly, so the identity map reproduces the plain path bit for bit.
// (The inverse map is specified with separately rounded products instead, because those can be tabulated
// per grid index: see phase2_aug.)
__device__ __forceinline__ double affine_row(const double *m, double px, double py, double pz) {
  return __builtin_fma(m[0], px, __builtin_fma(m[1], py, __builtin_fma(m[2], pz, m[3])));
}

// fl64(d / F) without the hardware division sequence (~12 dependent float64 instructions):
// with y = RN(1/F) computed by a true division on the host, q0 = RN(d*y) is within 1 ulp of d/F,
// r = d - q0*F is exact in one fma, and RN(q0 + r*y) is the correctly rounded quotient (Markstein's
// correction step).  The AABB parity tests compare the result bit for bit with the oracle's division.
__device__ __forceinline__ double div_by_focal(double d, const CamK &k) {
  const double q0 = d * k.inv_focal;
  const double r = __builtin_fma(-q0, k.focal, d);
  return __builtin_fma(r, k.inv_focal, q0);
}

// -F / vz for the augmented projection (a true division: the divisor changes from voxel to voxel).
//   FAST = false: the compiler's IEEE division (2 v_div_scale, v_rcp, 4 fma, mul, fma, v_div_fmas, v_div_fixup).
//   FAST = true:  the same sequence without its three scaling / fix-up instructions.  Those are the identity while
//                 neither operand nor the quotient comes near the ends of the exponent range, so the result is the
//                 same bit for bit; the caller proves 2^-600 < |vz| < 2^600 for a lane's whole column of voxels and
//                 2^-100 < F < 2^100 before choosing this form (phase2_aug), anything else takes the division.
// (Two Newton steps: v_rcp_f64 is good to 2^-24.4 on gfx950 (tools/probes/rcp64_probe.hip), so ONE step leaves 2^-48.7 and
// the corrected quotient is off by ~2^-97 before its final rounding — the IEEE quotient on every one of 4.2 M probed
// divisors, but a quotient of two float64 can sit within 2^-107 of a rounding boundary, so only the second step makes
// the result provably the division's.)
template <bool FAST>
__device__ __forceinline__ double neg_focal_over(double vz, const CamK &k) {
  if constexpr (!FAST) {
    return -k.focal / vz;
  } else {
    const double n = -k.focal;
    double r = __builtin_amdgcn_rcp(vz);
    r = __builtin_fma(r, __builtin_fma(-vz, r, 1.0), r);
    r = __builtin_fma(r, __builtin_fma(-vz, r, 1.0), r);
    const double q0 = n * r;
    return __builtin_fma(__builtin_fma(-vz, q0, n), r, q0);
  }
}
__device__ __forceinline__ bool mid_range(double v, double lo, double hi) {  // false for NaN
  const double a = __builtin_fabs(v);
  return a > lo && a < hi;
}

// A.1 x: f32( (f64(d)/F) * (x - cx) )      pre/tsdf_numba.py:91-92,95
__device__ __forceinline__ float backproject_x(float d, int x, const CamK &k) {
  const double q = div_by_focal((double)d, k);
  return (float)(q * ((double)x - k.cx));
}
// A.1 y: f32( (-(f64(d)/F)) * (y - cy) )   pre/tsdf_numba.py:91,93,95
__device__ __forceinline__ float backproject_y(float d, int y, const CamK &k) {
  const double q = div_by_focal((double)d, k);
  return (float)((-q) * ((double)y - k.cy));
}

// P consecutive pixels of one lane, P in 1..8 (16-byte + 12/8/4-byte pieces, 4-byte aligned).
template <int P>
struct PixN {
  float d[P];
};

typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
typedef float f3u __attribute__((ext_vector_type(3), aligned(4)));

// (Plain loads: nt on the row loads costs +12.5 % on full frames — the staging copy's re-read then misses L2 / Infinity
// Cache; cache-policy bits on the staging copy itself change nothing.  tools/patches/r05_removed_knobs.diff.)
template <int P>
__device__ __forceinline__ PixN<P> load_pix(const float *__restrict__ p) {
  PixN<P> r;
  constexpr int Q = P / 4, T = P % 4;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const f4 v = *reinterpret_cast<const f4u *>(p + 4 * q);
    r.d[4 * q] = v.x;
    r.d[4 * q + 1] = v.y;
    r.d[4 * q + 2] = v.z;
    r.d[4 * q + 3] = v.w;
  }
  if constexpr (T == 1) {
    r.d[4 * Q] = p[4 * Q];
  } else if constexpr (T == 2) {
    const auto v = *reinterpret_cast<const f2u *>(p + 4 * Q);
    r.d[4 * Q] = v.x;
    r.d[4 * Q + 1] = v.y;
  } else if constexpr (T == 3) {
    const auto v = *reinterpret_cast<const f3u *>(p + 4 * Q);
    r.d[4 * Q] = v.x;
    r.d[4 * Q + 1] = v.y;
    r.d[4 * Q + 2] = v.z;
  }
  return r;
}

struct Frame {
  const float *depth;  // frame-local base
  int l, t, r, b, bw, bh;
};

struct Grid {
  float mid[3];
  float max_l, voxel_len, trunc;
  float ori[3];
};

struct Aabb {
  float mn[3], mx[3];
  int c0, c1, r0, r1;  // bbox-relative rectangle holding every valid pixel (inclusive)
  bool any;
};

// The 10 extents phase 1 produces (per workgroup, then per frame):
//   [0..4] minima: cam x, cam y, depth, valid column index, valid row index   [5..9] the maxima
constexpr int kExt = 10;


