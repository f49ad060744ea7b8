// augdraw.inc — the augmentation's draw and map arithmetic, once: included by tsdf_augment.hip (libtsdf_augment.so, counters
// passed as kernel arguments) and by tsdf_augstep.hip (libtsdf_augstep.so, counters read from device memory).  Both kernels
// call aug_draw_row with the position's counter c and key; everything after that — the splitmix chain, the stretch and
// angle formulas, the float64 operation order of the maps, the analytic inverse, the twelve 16-byte stores — is this file.
// Arithmetic contract: include/tsdf_augment.h; float64 throughout, compiled with -ffp-contract=off.
//
// Device code only (the host preamble is device.inc).  Included inside an anonymous namespace, after
// <hip/hip_runtime.h>, <stdint.h> and include/tsdf.h.

constexpr int kAugWG = 256;   // threads per workgroup (4 wave64)

typedef double aug_d2 __attribute__((ext_vector_type(2), aligned(8)));   // 16-byte access on an 8-byte-aligned row

// splitmix64, every operation mod 2^64 (the generator of cloud.inc, restated)
__device__ __forceinline__ uint64_t aug_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// an integer angle in [-30, 30): the high word of a 32-bit draw times 60
__device__ __forceinline__ int aug_angle(uint64_t x) { return -30 + (int)(((aug_mix(x) >> 32) * 60ull) >> 32); }

__device__ __forceinline__ void aug_store(double *row, int k, double a, double b) {
  aug_d2 v;
  v.x = a;
  v.y = b;
  *reinterpret_cast<aug_d2 *>(row + 2 * k) = v;
}

// Batch position i: frame g of centres[n_src][3], drawn from (key, c).  Writes row i of xforms (and of stretch / rot when
// they are not null).
__device__ __forceinline__ void aug_draw_row(const float *centres, int64_t n_src, int64_t g, int i, uint64_t key, uint64_t c,
                                             double *xforms, double *stretch, int32_t *rot) {
  const bool ok = g >= 0 && g < n_src;

  // the draws: a function of (key, c) alone
  const uint64_t h = aug_mix(key + c);
  const double lo = 2.0 / 3.0, span = 1.5 - lo;
  const double u = (double)(aug_mix(h) >> 11) * 0x1p-53;
  double s = lo + u * span;
  int rxy = aug_angle(h + 1), rz = aug_angle(h + 2);
  if (!ok) rxy = rz = 0;   // identity map below: R = I, and s = 1 until it is reported as NaN

  const double m0 = ok ? (double)centres[3 * g + 0] : 0.0;
  const double m1 = ok ? (double)centres[3 * g + 1] : 0.0;
  const double m2 = ok ? (double)centres[3 * g + 2] : 0.0;
  if (!ok) s = 1.0;

  // R = Rx(t)·Ry(t)·Rz(tz) (augment.rotation_xyz: the same products in the same association, (Rx·Ry)·Rz)
  const double rad = 3.141592653589793 / 180.0;
  double sx, cx, sz, cz;
  sincos((double)rxy * rad, &sx, &cx);
  sincos((double)rz * rad, &sz, &cz);
  const double sy = sx, cy = cx;
  const double r10 = sx * sy, r12 = sx * cy, r20 = cx * sy, r22 = cx * cy;   // rows 1, 2 of Rx·Ry: {r10, cx, r12}, {r20, -sx, r22}
  // (a bad index: exactly I — sincos(0) already gives it, up to the sign of a zero)
  const double R[3][3] = {{ok ? cy * cz : 1.0, ok ? cy * sz : 0.0, ok ? -sy : 0.0},
                          {ok ? r10 * cz - cx * sz : 0.0, ok ? r10 * sz + cx * cz : 1.0, ok ? r12 : 0.0},
                          {ok ? r20 * cz + sx * sz : 0.0, ok ? r20 * sz - sx * cz : 0.0, ok ? r22 : 1.0}};

  // forward: A = Rᵀ·diag(s, s, 1), b = m - A·m;   inverse: A' = diag(1/s, 1/s, 1)·R, b' = m - A'·m
  const double m[3] = {m0, m1, m2};
  const double sc[3] = {s, s, 1.0};
  const double is = 1.0 / s;
  const double isc[3] = {is, is, 1.0};
  double *row = xforms + 24 * (int64_t)i;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double a0 = R[0][r] * sc[0], a1 = R[1][r] * sc[1], a2 = R[2][r] * sc[2];
    const double b = m[r] - ((a0 * m[0] + a1 * m[1]) + a2 * m[2]);
    aug_store(row, 2 * r, a0, a1);
    aug_store(row, 2 * r + 1, a2, b);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double a0 = isc[r] * R[r][0], a1 = isc[r] * R[r][1], a2 = isc[r] * R[r][2];
    const double b = m[r] - ((a0 * m[0] + a1 * m[1]) + a2 * m[2]);
    aug_store(row, 6 + 2 * r, a0, a1);
    aug_store(row, 6 + 2 * r + 1, a2, b);
  }
  if (stretch) stretch[i] = ok ? s : __builtin_nan("");
  if (rot) {
    rot[2 * i + 0] = rxy;
    rot[2 * i + 1] = rz;
  }
}
