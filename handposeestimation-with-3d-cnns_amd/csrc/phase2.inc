// phase2.inc — part of the one translation unit tsdf_hip.hip (included there, inside its anonymous namespace).
// Phase 2: the voxel pass (pre/tsdf_numba.py:15-72) — projection tables, gather sources, per-voxel values, output stores — in its plain and augmented form.

// ---- phase 2 ---------------------------------------------------------------------------------
struct VoxK {
  double cx, cy;
  double it;   // 1 / trunc_dis
  double kq;   // (1/F) * it
  double ncx;  // -cx
  float eps;
  // Pixel coordinates are kept relative to a frame of reference (px0, py0): the bounding box when the
  // voxel pass gathers from the LDS pool, the rectangle holding every valid pixel when it gathers from
  // global memory (everything outside that rectangle is rejected by pre/tsdf_numba.py:36 or :40).
  int px0, py0;  // image coordinates of that frame's first pixel
  int dx, dy;    // its extent - 1 (inclusive upper bounds of relative coordinates)
  int stride;    // rows of the gather source: elements per row (the crop's, or the staged rectangle's) ...
  int stride4;   // ... and bytes per row
  int base;      // global gather: index of the frame of reference's first pixel in the crop (the source pointer
                 // handed to the voxel pass already points there)
  double dxc, dyc;  // px0 - cx, py0 - cy: pix - c = relative coordinate + this
};

// Column codes.  The x table (and the on-the-fly projection) hand the voxel pass a column as its BYTE offset in
// the row, 4 * column, or kColBad when the voxel projects outside the frame of reference; a row is its index or
// -1.  With that, row * stride4 + code is the gather's byte offset, and it is negative exactly when the pixel
// does not exist (row -1: code - stride4 < 0; kColBad swamps any row) — one compare and one max instead of an
// or, a compare, a select and a shift per voxel.
constexpr int kColBad = -(1 << 30);
__device__ __forceinline__ int col_code(int rel) { return rel >= 0 ? rel << 2 : kColBad; }

__device__ __forceinline__ void zero_volume(float *__restrict__ out, int R, int tid, int T, int part, int parts) {
  const int n4 = 3 * R * R * R / 4;
  const int per = (n4 + parts - 1) / parts;
  const int beg = part * per, end = beg + per < n4 ? beg + per : n4;
  f4 *o4 = reinterpret_cast<f4 *>(out);
  const f4 z = {0.f, 0.f, 0.f, 0.f};
  for (int i = beg + tid; i < end; i += T) o4[i] = z;
}

// Projection of a voxel coordinate onto a pixel coordinate, pre/tsdf_numba.py:30-32:
//   pix = int(v * q + c)  with q = -F / v_z   (multiply, round, add, round, truncate)
// returned relative to p0, or -1 when outside [p0, p0 + dmax] (then :36 or :40 rejects).
__device__ __forceinline__ int project_rel(double v, double q, double c, int p0, int dmax) {
  const int rel = trunc_i32(mul_then_add(v, q, c)) - p0;
  return (unsigned)rel <= (unsigned)dmax ? rel : -1;
}

// The gather source is either the LDS pool of captured row spans or the frame in global memory.  It is
// passed with its address space in the type: a generic pointer would make every gather a FLAT load,
// which is counted in vmcnt together with the volume stores, so each loop iteration would wait for the
// previous iteration's stores to be acknowledged by memory.  As ds_read the gather only touches lgkmcnt
// and the stores stay in flight.
typedef const __attribute__((address_space(3))) float *LdsSrc;
typedef const __attribute__((address_space(1))) float *GlobalSrc;
typedef __attribute__((address_space(1))) float *GlobalOut;  // the output volume
typedef __attribute__((address_space(1))) int *GlobalPix;    // the diagnostic pixel map

// A staged rectangle in LDS: addressed like the crop in global memory (row * stride + column,
// coordinates relative to the rectangle), only in LDS.
struct LdsRect {
  LdsSrc p;
};

// Depth of pixel (column code xc, row): pre/tsdf_numba.py:36-39.  `ent` is the row's pool entry (span capture);
// inb = the pixel exists in the source.  The load is always in bounds.
__device__ __forceinline__ float gather_px(const LdsSrc pool, const VoxK &, int xc, int, unsigned ent, bool &inb) {
  const int rel = (xc >> 2) - (int)((ent >> 9) & 511u);
  inb = (unsigned)rel < (ent & 511u);
  const int idx = inb ? (int)((ent >> 18) << 2) + rel : 0;
  return pool[idx];
}
__device__ __forceinline__ float gather_px(const GlobalSrc src, const VoxK &k, int xc, int ry, unsigned, bool &inb) {
  int off = __mul24(ry, k.stride4) + xc;   // bytes; negative iff the pixel is outside (see kColBad)
  inb = off >= 0;
  off = off > 0 ? off : 0;                  // the load is always in bounds
  return *(GlobalSrc)((const __attribute__((address_space(1))) char *)src + off);
}
__device__ __forceinline__ float gather_px(const LdsRect src, const VoxK &k, int xc, int ry, unsigned, bool &inb) {
  int off = __mul24(ry, k.stride4) + xc;
  inb = off >= 0;
  off = off > 0 ? off : 0;
  return *(LdsSrc)((const __attribute__((address_space(3))) char *)src.p + off);
}

// The same for a pixel given by its coordinates relative to the frame of reference (possibly outside it): the
// on-the-fly projection of the augmented pass, which has no tables whose entries could carry the -1.
struct Tabs;
template <class SrcP>
__device__ __forceinline__ float gather_rel(const SrcP src, const VoxK &k, const Tabs &tb, int relx, int rely, bool &inb);

// Per-voxel value, pre/tsdf_numba.py:36-68, for the 4 voxels of one lane.  Coordinates are pre-scaled
// by it = 1/trunc_dis:  tx = v_x*it - (pix_x-cx)*(pd*kq),  ty likewise,  tz = v_z*it + pd*it (w_z = -pd).
//   ex[j], ry[j], ent[j]  relative pixel of voxel j (ex: column CODE, see kColBad; ry -1: rejected) and its row's entry
//   vxs[j], vys, vzs[j]   pre-scaled voxel centre;   negthr[j] = f32_round_up(-v_z)
// Returns the mask of voxels that passed :36 and :40 (bit j).
template <class SrcP>
__device__ __forceinline__ unsigned voxel_values4(const int (&ex)[4], const int (&ry)[4], const unsigned (&ent)[4],
                                                  const double (&vxs)[4], const double vys, const double (&vzs)[4],
                                                  const float (&negthr)[4], const VoxK &k,
                                                  const SrcP src, f4 &o0, f4 &o1, f4 &o2) {
  float pd[4];
  bool inb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) pd[j] = gather_px(src, k, ex[j], ry[j], ent[j], inb[j]);   // :36-39
  bool ok[4], neg[4];
  double pd64[4], tz[4];
  bool any_near = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ok[j] = inb[j] & (__builtin_fabsf(pd[j]) >= k.eps);                     // :40 (NaN -> rejected)
    pd64[j] = (double)pd[j];
    tz[j] = __builtin_fma(pd64[j], k.it, vzs[j]);                           // :46,:49
    neg[j] = pd[j] < negthr[j];                                             // w_z > v_z  :65
    any_near |= ok[j] & (__builtin_fabs(tz[j]) <= 1.0);
  }
  // A voxel that is rejected is 0 in all channels (:33-41), one beyond the truncation distance is (+-1,+-1,+-1)
  // (:54-57), signed by :65-68: that is sv[j], and it is the whole answer unless the wave holds a near voxel.
  float sv[4];
  unsigned okm = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sv[j] = ok[j] ? (neg[j] ? -1.0f : 1.0f) : 0.0f;
    okm |= (unsigned)ok[j] << j;
  }
  o0 = f4{sv[0], sv[1], sv[2], sv[3]};
  o1 = o0;
  o2 = o0;
  if (__any(any_near)) {
    // otherwise every voxel of this wave is rejected or beyond the truncation distance along z
    // alone: dist >= |tz| > 1 -> (1,1,1), and the x/y terms are not needed
    float *p0 = reinterpret_cast<float *>(&o0), *p1 = reinterpret_cast<float *>(&o1),
          *p2 = reinterpret_cast<float *>(&o2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double a = pd64[j] * k.kq;                                      // pd/F/trunc         :43
      const double dxi = __builtin_fma((double)ex[j], 0.25, k.dxc);         // pix_x - cx         :44 (exact)
      const double dyi = (double)ry[j] + k.dyc;                             // pix_y - cy         :45
      const double tx = __builtin_fma(-dxi, a, vxs[j]);                     // (v_x - w_x)/trunc  :47
      const double ty = __builtin_fma(dyi, a, vys);                         // (v_y - w_y)/trunc  :48, w_y = -dyi*q
      const double s = __builtin_fma(tz[j], tz[j], __builtin_fma(ty, ty, tx * tx));  // dist^2 :51-52
      const bool nearv = s <= 1.0;                                          // :54 (sqrt monotone, sqrt(1)=1)
      // |t| clamped to 1 (:58-60), float32 (:70-72); times sv = +-1 or 0: exact, and the sign lands on a zero too
      const float m0 = vminabs((float)tx, 1.0f);
      const float m1 = vminabs((float)ty, 1.0f);
      const float m2 = vminabs((float)tz[j], 1.0f);
      p0[j] = nearv ? __fmul_rn(m0, sv[j]) : sv[j];
      p1[j] = nearv ? __fmul_rn(m1, sv[j]) : sv[j];
      p2[j] = nearv ? __fmul_rn(m2, sv[j]) : sv[j];
    }
  }
  return okm;
}

// One 16-byte store of the output volume.  It is written once and never re-read here, so it goes out
// non-temporal and does not evict the depth rows other workgroups are streaming through L2 / Infinity
// Cache (measured in round 1: 180 -> 155 us per 1024 frames; re-checked in round 3: without nt +16 % at 32^3).
// Round 3: the store also carries DEVICE scope (sc1): it is written through towards memory instead of waiting in
// this XCD's L2 for a write-back — same-buffer paired A/B, 24 blocks each: 1024 full frames -2.2 % +- 0.2, 1024 crops
// -1.5 %, 64^3 augmented -1.3 %, 64^3 crops -1.6 % (gpurun_out/ab_store_policy2.log); "sc0 sc1 nt" (system scope) is
// within noise of it, workgroup scope ("sc0 nt") loses the gain again (+2.7 %), dropping nt costs 16 %.  (Also tried on the
// read side: nt on the row loads is +12.5 % on full frames — the staging copy's re-read then misses L2 / Infinity Cache,
// which shows that it normally hits —, nt on the staging copy itself changes nothing; raising the wave priority of either
// phase with s_setprio costs 3-4 %.)  There is no builtin for the scope bits of a plain store, hence the
// inline assembly; the s_nop covers the "VALU overwrites the data registers of a wide store" hazard the compiler
// can no longer see.  -DTSDF_STORE_ASM='"..."' selects other bits (the one policy knob left: tools/ab_precise.py).
#ifndef TSDF_STORE_ASM
#define TSDF_STORE_ASM "sc1 nt"
#endif
__device__ __forceinline__ void store_vol4(GlobalOut p, f4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off " TSDF_STORE_ASM "\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

// Diagnostic pixel map (tsdf_debug_pixmap_hip), one voxel: see include/tsdf.h.  `frame_dc/dr` shift the
// tables' frame of reference back into the bounding box.
struct PixMapK {
  GlobalPix out;  // int32[R][R][R] of this frame, [z][y][x]; null: no map
  int bw, dc, dr;
};
__device__ __forceinline__ int pixmap_value(const PixMapK &pm, int ex, int ry, bool row_in_bbox, bool ok) {
  if (ex < 0 || !row_in_bbox) return -1;                      // :36-37
  const int idx = (ry + pm.dr) * pm.bw + ex + pm.dc;          // :38
  return ok ? idx : -2 - idx;                                 // :40-41
}

// LDS-resident per-frame tables, one set per group.  The pixel a voxel projects to factorises: pix_x
// depends on (x, z) only and pix_y on (y, z) only, so for R <= kTabR both are tabulated once per frame
// (R*R entries each, one pair per thread) instead of 3 float64 operations + a range test per voxel.
//   pxtab[.]  column code of the relative pix_x (4 * column, or kColBad)
//   pytab[.]  LDS gather: the pool entry of row pix_y (0: outside the bounding box)
//             global gather: relative pix_y, or -1
//   pyrow[.]  LDS gather: relative pix_y (0 when outside)              (uint8; rows < kMaxRows)
struct ZEntry {
  double q;      // -F / v_z                     :30
  double vzs;    // v_z / trunc_dis
  float negthr;  // f32_round_up(-v_z)
  float pad;
};

typedef __attribute__((address_space(3))) const ZEntry *LdsZ;
typedef __attribute__((address_space(3))) const int *LdsCI;
typedef __attribute__((address_space(3))) const unsigned *LdsCU;
typedef __attribute__((address_space(3))) const unsigned char *LdsCU8;
typedef __attribute__((address_space(3))) const double *LdsCD;

typedef int i4v __attribute__((ext_vector_type(4)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const i4v *LdsI4;
typedef __attribute__((address_space(3))) const u4v *LdsU4;

__device__ __forceinline__ ZEntry load_z(LdsZ p) {
  ZEntry z;
  z.q = p->q;
  z.vzs = p->vzs;
  z.negthr = p->negthr;
  z.pad = 0.f;
  return z;
}

struct Tabs {
  LdsZ ztab;
  LdsCI pxtab;
  LdsCU pytab;
  LdsCU8 pyrow;
  LdsCU rowtab;
  LdsCD atab;
};

// table index of (fast, slow) coordinates: the 4 entries a lane needs are contiguous
template <int LAYOUT>
__device__ __forceinline__ int tab_index(int x_or_y, int z, int R) {
  return LAYOUT == 0 ? z * R + x_or_y : x_or_y * R + z;
}

template <class SrcP>
struct IsLds {
  static constexpr bool value = std::is_same<SrcP, LdsSrc>::value;
};

// row entry for an on-the-fly projected row (no tables): LDS gather looks the row table up
template <class SrcP>
__device__ __forceinline__ unsigned row_entry(const Tabs &tb, int ry) {
  if constexpr (IsLds<SrcP>::value) {
    return ry >= 0 ? tb.rowtab[ry] : 0u;
  } else {
    return (unsigned)ry;
  }
}

template <>
__device__ __forceinline__ float gather_rel<GlobalSrc>(const GlobalSrc src, const VoxK &k, const Tabs &, int relx, int rely,
                                                       bool &inb) {
  inb = ((unsigned)relx <= (unsigned)k.dx) & ((unsigned)rely <= (unsigned)k.dy);   // :36
  const int idx = inb ? __mul24(rely, k.stride) + relx : 0;
  return src[idx];                                                                  // :38-39
}
template <>
__device__ __forceinline__ float gather_rel<LdsRect>(const LdsRect src, const VoxK &k, const Tabs &, int relx, int rely,
                                                     bool &inb) {
  inb = ((unsigned)relx <= (unsigned)k.dx) & ((unsigned)rely <= (unsigned)k.dy);
  const int idx = inb ? __mul24(rely, k.stride) + relx : 0;
  return src.p[idx];
}
template <>
__device__ __forceinline__ float gather_rel<LdsSrc>(const LdsSrc src, const VoxK &k, const Tabs &tb, int relx, int rely,
                                                    bool &inb) {
  const bool iny = (unsigned)rely <= (unsigned)k.dy;
  const unsigned ent = iny ? tb.rowtab[iny ? rely : 0] : 0u;
  return gather_px(src, k, relx << 2, rely, ent, inb);   // a column outside the row's window (or the box) fails its test
}

// Dynamic units (tile_ctr != null: the one-group-per-CU instantiations, R >= 48).
// With the static split a wave keeps one slab of rows (64/R4 of them: one wave tile per slice) for the whole volume and
// walks the slices.  Two things are wrong with that at 64^3 (round 4):
//  * the ORDER in which the 3 MiB volume is written.  tools/probes/vol_store_probe.hip writes [3][64][64][64] volumes,
//    store-only, in a dozen orders: the static split's order (its waves in step or out of step) is the slowest of all —
//    5.0-5.1 TB/s where the best order reaches 6.1 on the same box (profiles/r04/vol_store_probe*.log; on the pool's fast
//    boxes the spread is 6.5 vs 6.9).  Best: the 16 waves of a CU on consecutive 2-slice pieces of ONE slab, every wave
//    writing its 1 KiB piece in the three channel planes, then the next slab.  That is what units of (slab) x (2 slices)
//    drawn from a counter produce.  Paired A/Bs of the real kernels, same buffer (profiles/r04/ab_plain_dyn.log,
//    ab_aug_chunks.log): plain 64^3 full frames -4.0 %, crops -4.7 %; augmented -3.1 % / -3.2 %.  Units of 1 slice:
//    -3.6 % / -0.3 %; of 4: +0.2 % / -0.7 %; of 8: +1.4 % (augmented).
//  * each SIMD serves its four waves oldest first, so a CU's waves leave a static pass in four steps — after 55, 87, 116
//    and 141 us (profiles/r04/stamps_aug64_per_wave_static.log) — and the youngest wave of each SIMD runs the last
//    quarter of the pass alone.  With units all 16 waves stay busy to the end (..._dyn8.log: 128-131 us each).
// A unit is still "pure" — a wave tile's 64 x 4 voxels are neighbours, so the wave-uniform shortcuts keep their hit
// rate — a wave's stores are still 1 KiB contiguous, and the results are bit-identical (the A/B tool asserts it).  The
// middle slabs, whose tiles most often need the x/y terms, go first.  Per-slab state of the augmented pass is kept
// while a wave stays in its slab (it mostly does: a slab's 32 units are drawn one after the other).
// 32^3 keeps its static two-slices-per-step order: the same probe for 32^3 volumes (vol32_store_probe.hip) finds it
// among the best already.
constexpr int kDynChunk = 2;

// The unit plan of one pass over slices [sb, se) with n_slab slabs: unit -> (slab, first slice, end slice).
struct DynPlan {
  int n_slab, sb, se;
  int n_chunk, n_unit;      // chunks per slab; units in all
};
__device__ __forceinline__ DynPlan dyn_plan(int n_slab, int sb, int se) {
  DynPlan p;
  p.n_slab = n_slab;
  p.sb = sb;
  p.se = se;
  p.n_chunk = (se - sb + kDynChunk - 1) / kDynChunk;
  p.n_unit = n_slab * p.n_chunk;
  return p;
}
__device__ __forceinline__ int dyn_slab(int rank, int n_slab);
__device__ __forceinline__ void dyn_unit(const DynPlan &p, int unit, int &slab, int &zb, int &ze) {
  const int rank = unit / p.n_chunk, c = unit - rank * p.n_chunk;
  slab = dyn_slab(rank, p.n_slab);
  zb = p.sb + c * kDynChunk;
  ze = zb + kDynChunk < p.se ? zb + kDynChunk : p.se;
}

// unit number -> slab: middle-out (n_slab even: h-1, h, h-2, h+1, ...)
__device__ __forceinline__ int dyn_slab(int rank, int n_slab) {
  const int h = n_slab >> 1, k = rank >> 1;
  const int s = (rank & 1) ? h + k : h - 1 - k;
  return s < 0 ? 0 : (s >= n_slab ? n_slab - 1 : s);
}

// The voxel pass over slow-axis slices [sb, se).  T threads take part (tid in [0, T)): T = kGW when a group
// works alone, 2*kGW when the CU's other group helps (its threads come in as kGW + gtid), kWG in the split
// kernel.
template <int LAYOUT, int T, bool DBG, class SrcP>
__device__ __forceinline__ void phase2(const Grid &g, const CamK &cam, const VoxK &vk, int R, const Tabs &tb,
                                       const bool use_tab, const SrcP src, const GlobalOut out, const int tid,
                                       const int sb, const int se, const PixMapK &pm, int *tile_ctr = nullptr) {
  if (se <= sb) return;
  const double vl = (double)g.voxel_len;
  const double ox = (double)g.ori[0], oy = (double)g.ori[1];
  const int R4 = R / 4;
  const int G = R * R4;  // groups of 4 voxels per slow-axis slice
  const int64_t R3 = (int64_t)R * R * R;

  // slow axis s (z for LAYOUT 0, x for LAYOUT 1); group gi -> (y, fast4)
  int g0, gstep, s0, sstep;
  if (G <= T && (T % G) == 0) {
    g0 = tid % G;
    gstep = G;  // one group of 4 voxels per thread, T/G slices at a time
    s0 = tid / G;
    sstep = T / G;
  } else {
    g0 = tid;
    gstep = T;
    s0 = 0;
    sstep = 1;
  }
  // dynamic units (see above): (slab of 64/R4 rows) x (kDynChunk slices) drawn from a counter in LDS
  const bool dyn = tile_ctr != nullptr && R4 <= 64 && (64 % R4) == 0 && (R % (64 / R4)) == 0;  // uniform
  const int n_slab = dyn ? R / (64 / R4) : 0;
  const DynPlan plan = dyn_plan(n_slab, sb, se);
  auto draw = [&]() -> int {
    int t = 0;
    if ((tid & 63) == 0) t = __hip_atomic_fetch_add(tile_ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __builtin_amdgcn_readfirstlane(t);
  };
  int unit = dyn ? draw() : 0;
  for (int gi = g0;; gi += gstep) {
    int zb = sb + s0, ze = se, zs = sstep;   // this pass's slices (uniform)
    if (dyn) {
      if (unit >= plan.n_unit) break;
      int slab;
      dyn_unit(plan, unit, slab, zb, ze);
      gi = slab * 64 + (tid & 63);
      zs = 1;
      unit = draw();   // (the next unit's number travels while this one is computed)
    } else if (gi >= G) {
      break;
    }
    const int f4i = (gi % R4) * 4;
    const int y = gi / R4;
    const double vy = oy + (double)y * vl;                                  // :27
    const double vys = vy * vk.it;
    if constexpr (LAYOUT == 0) {
      // lanes run along x: v_x fixed per lane, loop over z
      double vx[4], vxs[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        vx[j] = ox + (double)(f4i + j) * vl;                                // :26
        vxs[j] = vx[j] * vk.it;
      }
      for (int z = zb; z < ze; z += zs) {
        const ZEntry zen = load_z(tb.ztab + z);
        int ex[4], ry[4];
        unsigned ent[4];
        if (use_tab) {
          const i4v e = *(LdsI4)(tb.pxtab + z * R + f4i);
          ex[0] = e.x; ex[1] = e.y; ex[2] = e.z; ex[3] = e.w;
          ent[0] = tb.pytab[z * R + y];
          ry[0] = IsLds<SrcP>::value ? (int)tb.pyrow[z * R + y] : (int)ent[0];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) ex[j] = col_code(project_rel(vx[j], zen.q, cam.cx, vk.px0, vk.dx));  // :31
          ry[0] = project_rel(-vy, zen.q, cam.cy, vk.py0, vk.dy);                                 // :32
          ent[0] = row_entry<SrcP>(tb, ry[0]);
        }
        ry[1] = ry[2] = ry[3] = ry[0];
        ent[1] = ent[2] = ent[3] = ent[0];
        const double vzs[4] = {zen.vzs, zen.vzs, zen.vzs, zen.vzs};
        const float negthr[4] = {zen.negthr, zen.negthr, zen.negthr, zen.negthr};
        f4 o0, o1, o2;
        const unsigned okm = voxel_values4(ex, ry, ent, vxs, vys, vzs, negthr, vk, src, o0, o1, o2);
        const int64_t e = ((int64_t)z * R + y) * R + f4i;                   // o[c][z][y][x] :70-72
        store_vol4(out + e, o0);
        store_vol4(out + R3 + e, o1);
        store_vol4(out + 2 * R3 + e, o2);
        if constexpr (DBG) {
          const bool rin = IsLds<SrcP>::value ? ent[0] != 0u : ry[0] >= 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) pm.out[e + j] = pixmap_value(pm, ex[j] >> 2, ry[0], rin, (okm >> j) & 1u);
        }
      }
    } else {
      // lanes run along z: q, v_z and pix_y fixed per lane, loop over x
      double q[4], vzs[4];
      float negthr[4];
      int ry[4];
      unsigned ent[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const ZEntry zen = load_z(tb.ztab + f4i + j);
        q[j] = zen.q;
        vzs[j] = zen.vzs;
        negthr[j] = zen.negthr;
      }
      if (use_tab) {
        const u4v e = *(LdsU4)(tb.pytab + y * R + f4i);
        ent[0] = e.x; ent[1] = e.y; ent[2] = e.z; ent[3] = e.w;
        if constexpr (IsLds<SrcP>::value) {
          const unsigned rr = *(LdsCU)(tb.pyrow + y * R + f4i);
          ry[0] = rr & 255u; ry[1] = (rr >> 8) & 255u; ry[2] = (rr >> 16) & 255u; ry[3] = rr >> 24;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) ry[j] = (int)ent[j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ry[j] = project_rel(-vy, q[j], cam.cy, vk.py0, vk.dy);
          ent[j] = row_entry<SrcP>(tb, ry[j]);
        }
      }
      for (int x = zb; x < ze; x += zs) {
        const double vx = ox + (double)x * vl;
        const double vx1 = vx * vk.it;
        const double vxs[4] = {vx1, vx1, vx1, vx1};
        int ex[4];
        if (use_tab) {
          const i4v e = *(LdsI4)(tb.pxtab + x * R + f4i);
          ex[0] = e.x; ex[1] = e.y; ex[2] = e.z; ex[3] = e.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) ex[j] = col_code(project_rel(vx, q[j], cam.cx, vk.px0, vk.dx));
        }
        f4 o0, o1, o2;
        const unsigned okm = voxel_values4(ex, ry, ent, vxs, vys, vzs, negthr, vk, src, o0, o1, o2);
        const int64_t e = ((int64_t)x * R + y) * R + f4i;                   // o[c][x][y][z] tsdf_for.py:118-120
        store_vol4(out + e, o0);
        store_vol4(out + R3 + e, o1);
        store_vol4(out + 2 * R3 + e, o2);
        if constexpr (DBG) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bool rin = IsLds<SrcP>::value ? ent[j] != 0u : ry[j] >= 0;
            pm.out[((int64_t)(f4i + j) * R + y) * R + x] = pixmap_value(pm, ex[j] >> 2, ry[j], rin, (okm >> j) & 1u);
          }
        }
      }
    }
  }
}

// Phase 2 of the augmented form (oracle/tsdf_oracle.c::tsdf_oracle_voxels_aug): the voxel centre v'
// lives in the augmented frame, v = T^-1(v') is projected and the pixel gathered as in the plain pass; the
// distances are those between v' and T(w), w the pixel's surface point.  The projection no longer factorises,
// so there are no pixel tables and q = -F / v_z is one true division per voxel; what does factorise is the
// inverse map: its three products per row, A_i0*v'_x, A_i1*v'_y, A_i2*v'_z, depend on one grid index each and
// are tabulated per frame (atab), leaving (a + b) + (c + d) — the oracle's exact rounding order.
// The distances never form w or T(w) (round 2 did: ~21 float64 operations per voxel before the first test).
// For an affine T,  v'_i - w'_i = (v'_i - b_i) + pd * c_i  with  c_i = fma(g_i0, dxi, fma(g_i1, dyi, A_i2)),
// g_i0 = -(A_i0 / F), g_i1 = A_i1 / F per frame, dxi = pix_x - cx, dyi = pix_y - cy: three fma for the z
// component that decides everything a far or rejected voxel needs (|u_z| > trunc_dis -> (+-1,+-1,+-1), sign of
// u_z), and the x / y components only in wave tiles that hold a near voxel.  The contract (include/tsdf.h,
// restated operation by operation in the oracle) is written in exactly this form.
// atab layout: [axis][index][4] = { fl(inv[4*row + axis] * (ori_axis + index*voxel_len)) for row 0..2 — the z
// entries + b_row —, (ori_axis + index*voxel_len) - fwd_b[axis] }.
// The table of the axis the LANES index (x for LAYOUT 0, z for LAYOUT 1) is stored lane-major: a lane reads the entries
// of its four voxels 4i..4i+3 — 8 pieces of 16 bytes — and the 16 lanes of a grid row read them together, so piece
// (j, half) of all lanes is one contiguous run: double offset of entry `idx`, value `row` (0..3).  With the plain
// [index][4] layout those reads were 128 bytes apart from lane to lane: ds_read_b128 banks 4-way, and since the voxel pass
// works in (slab x 2-slice) units a wave re-reads them every other unit — SQ_LDS_BANK_CONFLICT went from 20 M to 70 M
// cycles per launch between rounds 3 and 4 although the LDS instruction count fell (VERDICT round 4).
__device__ __forceinline__ int lane_slot(int idx, int row, int R4) {
  return ((2 * (idx & 3) + (row >> 1)) * R4 + (idx >> 2)) * 2 + (row & 1);
}

__device__ __forceinline__ double uniform64(double v) {  // a wave-uniform float64 -> scalar registers
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

template <int LAYOUT, int T, class SrcP>
__device__ __forceinline__ void phase2_aug(const Grid &g, const CamK &cam, const VoxK &vk, int R,
                                           const double *xf, const Tabs &tb, const SrcP src,
                                           const GlobalOut out, const int tid, const int sb, const int se,
                                           int *tile_ctr = nullptr, int stamp_iter = 0) {
  (void)stamp_iter;
  TSDF_WSTAMP(stamp_iter, 0);
  if (se <= sb) return;  // (uniform) nothing to do; the end-slice lookups below assume one slice at least
  const double *fwd = xf;
  const LdsCD tabx = tb.atab, taby = tb.atab + 4 * R, tabz = tb.atab + 8 * R;
  const int R4 = R / 4;
  const int G = R * R4;
  const int64_t R3 = (int64_t)R * R * R;
  // per-frame constants of the distance terms, kept in scalar registers
  double g0[3], g1[3], a2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    g0[i] = uniform64(-(fwd[4 * i] * cam.inv_focal));
    g1[i] = uniform64(fwd[4 * i + 1] * cam.inv_focal);
    a2[i] = fwd[4 * i + 2];
  }
  // |u_z| beyond this is beyond the truncation distance whatever x and y are: t_z = u_z * it with it = fl(1/trunc)
  // is then > 1 + 2^-31 after both roundings, so dist^2 > 1 (the gate may only err towards "look closer")
  const double tgate = uniform64((double)g.trunc * (1.0 + 0x1p-30));
  int g0i, gstep, s0, sstep;
  if (G <= T && (T % G) == 0) {
    g0i = tid % G;
    gstep = G;
    s0 = tid / G;
    sstep = T / G;
  } else {
    g0i = tid;
    gstep = T;
    s0 = 0;
    sstep = 1;
  }
  // (A wave's 64 groups of 4 voxels are one 64 x 4 tile of a slice at 64^3.  Narrower 32 x 8 tiles — fewer slices hold a
  // near voxel for them when the map rotates, 15 % fewer VALU instructions — measured +-0.2 % in a same-buffer paired A/B:
  // after this round's diet the pass is no longer bound by instruction issue.  Not kept.)
  const bool dyn = tile_ctr != nullptr && R4 <= 64 && (64 % R4) == 0 && (R % (64 / R4)) == 0;  // uniform
  const int n_slab = dyn ? R / (64 / R4) : 0;                      // slabs of 64/R4 rows: one wave tile per slice
  const DynPlan plan = dyn_plan(n_slab, sb, se);
  auto draw = [&]() -> int {
    int t = 0;
    if ((tid & 63) == 0) t = __hip_atomic_fetch_add(tile_ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __builtin_amdgcn_readfirstlane(t);
  };
  int unit = dyn ? draw() : 0;
  // Per-slab state, recomputed only when a wave's unit lies in another slab than its previous one (units of one slab are
  // drawn one after the other, so with small units a wave mostly stays in its slab).
  int gi_have = -1;
  double ty0 = 0, ty1 = 0, ty2 = 0, vby = 0, pre[4][3], vbf[4];
  bool mild = false;
  for (int gi = g0i;; gi += gstep) {
    int zb = sb + s0, ze = se, zs = sstep;   // this pass's slices (uniform)
    if (dyn) {
      if (unit >= plan.n_unit) break;
      int slab;
      dyn_unit(plan, unit, slab, zb, ze);
      gi = slab * 64 + (tid & 63);
      zs = 1;
      unit = draw();   // (the next unit's number travels while this one is computed)
    } else if (gi >= G) {
      break;
    }
    const int f4i = (gi % R4) * 4;
    const int y = gi / R4;
    if (gi != gi_have) {   // (uniform: every lane of a wave changes slab together)
      gi_have = gi;
      ty0 = taby[4 * y];
      ty1 = taby[4 * y + 1];
      ty2 = taby[4 * y + 2];
      vby = taby[4 * y + 3];   // v'_y - b_y
      // The inverse map is (A_i0 x' + A_i1 y') + (A_i2 z' + b_i), every product and sum rounded separately (the
      // oracle's affine3).  Both brackets depend on grid indices only: the z table holds (A_i2 z' + b_i), and the
      // bracket that does not change from slice to slice stays in registers — LAYOUT 0 (x, y fixed per lane) keeps
      // (A_i0 x' + A_i1 y') for its 4 voxels, LAYOUT 1 (y, z fixed) keeps the z bracket — so a voxel costs ONE add
      // per row of the map.  The same goes for v' - b of the distance terms: the fixed axes' live in registers
      // (vbf), the slice's comes from its table entry.
      // (The lanes' own axis is read from the lane-major image of its table — see lane_slot —: 16-byte pieces, the 16
      // lanes of a row side by side, so the eight ds_read_b128 of a slab change are conflict-free.)
      const LdsCD tl = LAYOUT == 0 ? tabx : tabz;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const LdsCD lo = tl + lane_slot(f4i + j, 0, R4), hi = tl + lane_slot(f4i + j, 2, R4);
        if constexpr (LAYOUT == 0) {
          pre[j][0] = lo[0] + ty0;
          pre[j][1] = lo[1] + ty1;
          pre[j][2] = hi[0] + ty2;
        } else {
          pre[j][0] = lo[0];
          pre[j][1] = lo[1];
          pre[j][2] = hi[0];
        }
        vbf[j] = hi[1];                      // v' - b of the lanes' own axis (x for LAYOUT 0, z for LAYOUT 1)
      }
      // Which division (neg_focal_over): v_z of a lane's voxel is fl(pre + slice term), monotone in the slice index
      // (every rounding is), so the pass's two end slices bound it; same sign and mid-range at both ends -> mid-range
      // in every slice of every unit of the slab.
      mild = mid_range(cam.focal, 0x1p-100, 0x1p100);
      const LdsCD tlo = (LAYOUT == 0 ? tabz : tabx) + 4 * sb, thi = (LAYOUT == 0 ? tabz : tabx) + 4 * (se - 1);
      const double s_lo = LAYOUT == 0 ? tlo[2] : tlo[2] + ty2, s_hi = LAYOUT == 0 ? thi[2] : thi[2] + ty2;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double z_a = pre[j][2] + s_lo, z_b = pre[j][2] + s_hi;
        mild = mild && mid_range(z_a, 0x1p-600, 0x1p600) && mid_range(z_b, 0x1p-600, 0x1p600) && ((z_a > 0.0) == (z_b > 0.0));
      }
      mild = __all(mild);
    }
    auto slices = [&](auto fast_tag) {
    constexpr bool FAST = decltype(fast_tag)::value;
    for (int sl = zb; sl < ze; sl += zs) {
      // ---- project the 4 voxels and gather their depths ----
      int ex[4], ry[4];
      float pd[4];
      bool ok[4];
      double sl0, sl1, sl2, vbs;  // the slice's own terms (wave-uniform)
      if constexpr (LAYOUT == 0) {
        const LdsCD tzp = tabz + 4 * sl;
        sl0 = tzp[0];
        sl1 = tzp[1];
        sl2 = tzp[2];
        vbs = tzp[3];                      // v'_z - b_z
      } else {
        const LdsCD tx = tabx + 4 * sl;
        sl0 = tx[0] + ty0;
        sl1 = tx[1] + ty1;
        sl2 = tx[2] + ty2;
        vbs = tx[3];                       // v'_x - b_x
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double vx = pre[j][0] + sl0;   // v = T^-1(v') = (A_i0 x' + A_i1 y') + (A_i2 z' + b_i)
        const double vy = pre[j][1] + sl1;
        const double vz = pre[j][2] + sl2;
        const double q = neg_focal_over<FAST>(vz, cam);                          // :30  -F / v_z
        ex[j] = trunc_i32(mul_then_add(vx, q, cam.cx)) - vk.px0;                 // :31, relative; may lie outside
        ry[j] = trunc_i32(mul_then_add(-vy, q, cam.cy)) - vk.py0;                // :32
        bool inb;
        pd[j] = gather_rel<SrcP>(src, vk, tb, ex[j], ry[j], inb);                // :36-39
        ok[j] = inb & (__builtin_fabsf(pd[j]) >= vk.eps);                        // :40
      }
      // ---- z component first: a wave whose voxels are all beyond the truncation distance along z' alone
      // needs nothing else (dist >= |t_z| > 1 -> (1,1,1)); one whose voxels are all rejected needs nothing ----
      f4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0, o2 = o0;
      if (__any(ok[0] | ok[1] | ok[2] | ok[3])) {
        double dxi[4], dyi[4], uz[4];
        float sv[4];  // 0 for a rejected voxel, else the sign of :65-68 as +-1: the whole answer unless near
        bool any_near = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dxi[j] = (double)ex[j] + vk.dxc;                                         // pix_x - cx  :44 (exact)
          dyi[j] = (double)ry[j] + vk.dyc;                                         // pix_y - cy  :45
          const double cz = __builtin_fma(g0[2], dxi[j], __builtin_fma(g1[2], dyi[j], a2[2]));
          uz[j] = __builtin_fma((double)pd[j], cz, LAYOUT == 0 ? vbs : vbf[j]);    // v'_z - w'_z  :46,:49
          any_near |= ok[j] & (__builtin_fabs(uz[j]) <= tgate);
          sv[j] = ok[j] ? (uz[j] < 0.0 ? -1.0f : 1.0f) : 0.0f;                     // w'_z > v'_z  :65
        }
        o0 = f4{sv[0], sv[1], sv[2], sv[3]};
        o1 = o0;
        o2 = o0;
        if (__any(any_near)) {
          float *p0 = reinterpret_cast<float *>(&o0), *p1 = reinterpret_cast<float *>(&o1),
                *p2 = reinterpret_cast<float *>(&o2);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double pd64 = (double)pd[j];
            const double cxx = __builtin_fma(g0[0], dxi[j], __builtin_fma(g1[0], dyi[j], a2[0]));
            const double cyy = __builtin_fma(g0[1], dxi[j], __builtin_fma(g1[1], dyi[j], a2[1]));
            const double ux = __builtin_fma(pd64, cxx, LAYOUT == 0 ? vbf[j] : vbs);  // v'_x - w'_x  :47
            const double uy = __builtin_fma(pd64, cyy, vby);                         // v'_y - w'_y  :48
            const double tx = ux * vk.it, ty = uy * vk.it, tz = uz[j] * vk.it;
            const double s2 = __builtin_fma(tz, tz, __builtin_fma(ty, ty, tx * tx));
            const bool nearv = s2 <= 1.0;                                          // :54
            const float m0 = vminabs((float)tx, 1.0f);
            const float m1 = vminabs((float)ty, 1.0f);
            const float m2 = vminabs((float)tz, 1.0f);
            p0[j] = nearv ? __fmul_rn(m0, sv[j]) : sv[j];                          // exact: sv is +-1 or 0
            p1[j] = nearv ? __fmul_rn(m1, sv[j]) : sv[j];
            p2[j] = nearv ? __fmul_rn(m2, sv[j]) : sv[j];
          }
        }
      }
      const int64_t e = ((int64_t)sl * R + y) * R + f4i;  // o[c][slow][y][fast]
      store_vol4(out + e, o0);
      store_vol4(out + R3 + e, o1);
      store_vol4(out + 2 * R3 + e, o2);
    }
    };
    if (mild) {
      slices(std::true_type{});
    } else {
      slices(std::false_type{});
    }
  }
  TSDF_WSTAMP(stamp_iter, 1);
}


