// mapvox.inc — the voxel arithmetic under a per-frame map, stated once: tsdf_auggrid.hip (float32 voxels) and
// tsdf_maplowp.hip (float16 / bfloat16 voxels) include it after slab.inc, inside their anonymous namespace;
// tsdf_mapaccurate.hip takes the table and the constants from it and evaluates the terms per candidate pixel.  The contract
// is include/tsdf_auggrid.h (== oracle/tsdf_oracle.c::tsdf_oracle_voxels_aug); both kernels compute the same float32
// values by the same operations and differ in how they store them.
//   map_d4        four float64: one entry of the per-axis table
//   map_fill_tab  the table: per axis and grid index the three products of the inverse map with the voxel centre's
//                 coordinate (the z axis with b' added: the contract groups T^-1 as (A'_i0 x + A'_i1 y) + (A'_i2 z + b'_i),
//                 and both brackets depend on grid indices only) and v' - b of the distance terms
//   MapK, map_consts   the per-frame constants of the distance terms
//   map_quad      four consecutive voxels of the fastest axis: inverse map, IEEE division, unfused pixel index, gather,
//                 distance terms, clamp and sign
// Compiled with -ffp-contract=off, fma only where __builtin_fma is written.

typedef double map_d4 __attribute__((ext_vector_type(4)));

// s_tab: [axis][index] = {A'_0a v'_a, A'_1a v'_a, A'_2a v'_a, v'_a - b_a}, the z axis with + b'_i in its first three:
// 3 x R entries of 32 bytes in LDS.  xf: the position's 24 doubles, forward rows then inverse rows; ox, oy, oz, vl: its
// grid row.  The caller's barrier comes before the first read.
__device__ __forceinline__ void map_fill_tab(map_d4 (&s_tab)[3][kSlabMaxR], const double *__restrict__ xf,
                                             float ox, float oy, float oz, float vl, int R, int tid) {
#pragma clang fp contract(off)
  for (int e = tid; e < 3 * R; e += kSlabWG) {
    const int ax = e / R, idx = e - ax * R;
    const float o = ax == 0 ? ox : ax == 1 ? oy : oz;
    const double prod = (double)idx * (double)vl;
    const double vp = (double)o + prod;                       // v'_a
    map_d4 t;
    t.x = xf[12 + ax] * vp;                                   // A'_0a v'_a
    t.y = xf[16 + ax] * vp;
    t.z = xf[20 + ax] * vp;
    if (ax == 2) {                                            // (A'_i2 z' + b'_i)
      t.x = t.x + xf[15];
      t.y = t.y + xf[19];
      t.z = t.z + xf[23];
    }
    t.w = vp - xf[4 * ax + 3];                                // v'_a - b_a
    s_tab[ax][idx] = t;
  }
}

// the per-frame constants of the distance terms
struct MapK {
  double F, cx, cy, it;
  double g00, g10, g20, g01, g11, g21, a02, a12, a22;
  float eps;
  int left, top, right, bottom;
  int64_t bw;
};

__device__ __forceinline__ MapK map_consts(const double *__restrict__ xf, const SlabSrc &s, float eps,
                                           const SlabFrame &fr) {
#pragma clang fp contract(off)
  MapK k;
  k.F = s.focal, k.cx = s.cx, k.cy = s.cy;
  const double iF = 1.0 / k.F;
  k.it = 1.0 / (double)fr.td;
  const double p00 = xf[0] * iF, p10 = xf[4] * iF, p20 = xf[8] * iF;
  k.g00 = -p00, k.g10 = -p10, k.g20 = -p20;                   // g_i0 = -(A_i0 * iF)
  k.g01 = xf[1] * iF, k.g11 = xf[5] * iF, k.g21 = xf[9] * iF; // g_i1 = A_i1 * iF
  k.a02 = xf[2], k.a12 = xf[6], k.a22 = xf[10];
  k.eps = eps;
  k.left = fr.left, k.top = fr.top, k.right = fr.right, k.bottom = fr.bottom;
  k.bw = fr.bw;
  return k;
}

// Four consecutive voxels of the fastest axis starting at grid index f4, in the row y (ty = s_tab[1][y]) of slice sl
// (ts = s_tab[2 or 0][sl]: z in layout czyx, x in cxyz): their float32 values.  The four gathers are issued before the
// distance terms of the first voxel and are always in bounds: a rejected voxel reads the crop's first pixel and is 0.
template <int LAYOUT>
__device__ __forceinline__ void map_quad(const map_d4 (&s_tab)[3][kSlabMaxR], const MapK &k, const float *__restrict__ d,
                                         const map_d4 &ty, const map_d4 &ts, int f4, float (&v0)[4], float (&v1)[4],
                                         float (&v2)[4]) {
#pragma clang fp contract(off)
  // ---- project the four voxels and gather their depths ----
  int px[4], py[4];
  float pd[4];
  bool inb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const map_d4 tf = s_tab[LAYOUT == 0 ? 0 : 2][f4 + j];   // the lane's own axis
    const map_d4 tx = LAYOUT == 0 ? tf : ts, tz = LAYOUT == 0 ? ts : tf;
    // v = T^-1(v') = (A'_i0 x' + A'_i1 y') + (A'_i2 z' + b'_i)
    const double s0 = tx.x + ty.x, s1 = tx.y + ty.y, s2 = tx.z + ty.z;
    const double vx = s0 + tz.x, vy = s1 + tz.y, vz = s2 + tz.z;
    const double q = -k.F / vz;                              // IEEE division
    const double mx = vx * q, my = (-vy) * q;
    px[j] = trunc_i32(mx + k.cx);
    py[j] = trunc_i32(my + k.cy);
    inb[j] = px[j] >= k.left && px[j] < k.right && py[j] >= k.top && py[j] < k.bottom;
    const int64_t at = inb[j] ? (int64_t)(py[j] - k.top) * k.bw + (px[j] - k.left) : 0;   // the load is always in bounds
    pd[j] = d[at];
  }
  // ---- the distance terms ----
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double wf = s_tab[LAYOUT == 0 ? 0 : 2][f4 + j].w;
    const double wx = LAYOUT == 0 ? wf : ts.w, wz = LAYOUT == 0 ? ts.w : wf;
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
    if (inb[j] && __builtin_fabsf(pd[j]) >= k.eps) {         // NaN is invalid
      const double dxi = (double)px[j] - k.cx, dyi = (double)py[j] - k.cy, pd64 = (double)pd[j];
      const double c0 = __builtin_fma(k.g00, dxi, __builtin_fma(k.g01, dyi, k.a02));
      const double c1 = __builtin_fma(k.g10, dxi, __builtin_fma(k.g11, dyi, k.a12));
      const double c2 = __builtin_fma(k.g20, dxi, __builtin_fma(k.g21, dyi, k.a22));
      const double u0 = __builtin_fma(pd64, c0, wx);         // v'_i - w'_i, mm
      const double u1 = __builtin_fma(pd64, c1, ty.w);
      const double u2 = __builtin_fma(pd64, c2, wz);
      const double t0 = u0 * k.it, t1 = u1 * k.it, t2 = u2 * k.it;
      const double xx = t0 * t0;
      const double sq = __builtin_fma(t2, t2, __builtin_fma(t1, t1, xx));
      const bool nearv = sq <= 1.0;
      double m0 = __builtin_fabs(t0), m1 = __builtin_fabs(t1), m2 = __builtin_fabs(t2);
      if (!(m0 < 1.0)) m0 = 1.0;                             // min(|t|, 1); a NaN distance counts as far
      if (!(m1 < 1.0)) m1 = 1.0;
      if (!(m2 < 1.0)) m2 = 1.0;
      if (!nearv) m0 = m1 = m2 = 1.0;
      if (u2 < 0.0) {
        m0 = -m0;
        m1 = -m1;
        m2 = -m2;
      }
      r0 = (float)m0;
      r1 = (float)m1;
      r2 = (float)m2;
    }
    v0[j] = r0;
    v1[j] = r1;
    v2[j] = r2;
  }
}
