// phase1.inc — part of the one translation unit tsdf_hip.hip (included there, inside its anonymous namespace).
// Phase 1: one streaming pass over a frame's rows -> extents of the valid back-projected pixels (pre/tsdf_numba.py:75-116,140-141), and the glue that places the grid (:142-147).

// ---- row-span capture (the split kernel's redundant form; the fused kernel stages by LDS-DMA instead) ----
// While phase 1 has a row in registers it copies the row's window of valid pixels — the lane windows from
// the first to the last lane holding a valid pixel, cut at the row end — into an LDS pool and records
// where: one 32-bit entry per bbox row,
//     bits 31..18  offset in the pool, in units of 4 floats
//     bits 17..9   bbox-relative column of the first captured pixel
//     bits  8..0   number of captured pixels (0: the row has no valid pixel)
// A pixel (col, row) is then  pool[4*off4 + col - first]  when  0 <= col - first < cnt, and rejected by
// pre/tsdf_numba.py:40 otherwise (every pixel outside the window is invalid by construction).
// Every wave of the workgroup owns a fixed 1/16 of the pool and fills it with a bump pointer it keeps in a
// scalar register: allocation costs no LDS round trip (an LDS atomic with return was tried first and cost
// 3-7 us per frame: its latency is the LDS queue, which the other group's voxel pass keeps full).  Rows are
// dealt to the waves round-robin, so the waves of a frame fill up evenly.  A row that does not fit makes the
// frame "not captured": its voxel pass gathers from global memory instead (never wrong, only slower).
// (LDS pointers carry their address space in the type: through generic pointers every access would be a
// FLAT instruction, counted in vmcnt together with the row loads.)
typedef __attribute__((address_space(3))) float *LdsF;
typedef __attribute__((address_space(3))) unsigned *LdsU;
typedef __attribute__((address_space(3))) int *LdsI;

struct Capture {
  LdsF pool;           // the pool
  LdsU rowtab;         // this group's row table
  LdsI fail;           // set when a row of this frame did not fit
  int base4;           // this WAVE's private region of the pool: first unit (of 4 floats) ...
  int cap4;            // ... and size in units
  bool on;             // wave-uniform: capture this frame at all
};

constexpr unsigned kRowEmpty = (511u << 9);  // a row inside the bounding box without a valid pixel (cnt = 0);
                                             // 0 is kept for "no such row" (outside the bounding box)
__device__ __forceinline__ unsigned row_pack(int off4, int first, int cnt) {
  return ((unsigned)off4 << 18) | ((unsigned)first << 9) | (unsigned)cnt;
}

// ---- phase 1: extents of all valid back-projected pixels of rows [rbeg, rend) ----------------
// NW waves cooperate; the result is wave-uniform in every thread.
// `wave` is the (scalar) index of this wave among the NW cooperating waves, `sync` their barrier.
// DEAL: which rows a wave loads next (extents are min/max reductions: every deal gives the same bits).
//   kDealStatic  row = rbeg + wave + NW*i, fixed at compile time; a register buffer holds kU rows NW apart.
//   kDealDrawn   the rows are cut into blocks of kU adjacent rows (rowdeal.inc), a register buffer holds one block, and
//                a wave draws the number of its next block from the LDS counter *row_ctr (0 when the waves enter: reset
//                before the barrier in front of this call).  Block numbers go outside in, in runs of NW blocks: NW from
//                the top, NW from the bottom, ... meeting in the middle.  Two effects, measured on 1024 full frames ->
//                32^3 with the inputs in rotation (profiles/rowdeal/): a wave whose loads come back late no longer
//                keeps its full share while seven wait — the spread between a group's first and last wave at the end
//                of the stream falls from 2.9-3.6 us to 1.7-2.5 — and the rows read last are the middle ones, which
//                the staging copy re-reads first and most (that re-read costs 3.0 % of the launch when the inputs
//                are cold).  Drawn + top to bottom -1.4 % (crops -0.8 %), drawn + outside in block by block -2.8 %
//                (crops +-0.2 %), in runs of NW the same on full frames and -0.7...+0.3 % on crops; static blocks
//                outside in +0.5 % (crops +2.7 %); 4096 frames per launch pay +0.5 %.  docs/HISTORY.md has the table.
// AUG: the extents are those of the affinely mapped cloud p' = A p + b (xf = 12 doubles), which needs
// every valid pixel transformed (the monotone shortcut does not survive a rotation).
constexpr int kDealStatic = 0, kDealDrawn = 1;
template <int NW, bool AUG, bool CAP, int DEAL = kDealStatic, typename SYNC>
__device__ __forceinline__ void phase1_extents(const Frame &f, const CamK &k, int rbeg, int rend, float *red,
                                               float (&fin)[kExt], const int wave, SYNC sync, const Capture &cap,
                                               int stamp_iter = 0, const double *xf = nullptr, int *row_ctr = nullptr) {
  (void)stamp_iter;
  constexpr int kWaves = NW;
  constexpr int kRowStep = DEAL == kDealStatic ? NW : 1;   // distance between the rows of one register buffer
  static_assert(DEAL == kDealStatic || !CAP, "the capture's per-wave pool regions assume the static deal");
  const int lane = threadIdx.x & 63;
  float xmn = TSDF_INF, xmx = -TSDF_INF, ymn = TSDF_INF, ymx = -TSDF_INF;
  float dmn = TSDF_INF, dmx = -TSDF_INF;
  float cimn = TSDF_INF, cimx = -TSDF_INF, rimn = TSDF_INF, rimx = -TSDF_INF;  // indices (exact in f32)
  // per-wave stash of reduced row extremes: lane i keeps the i-th non-empty row piece
  float s_rmin = TSDF_INF, s_rmax = -TSDF_INF;
  int s_row = 0, cnt = 0;
  int cap_used = 0;  // units of this wave's pool region taken by the frame so far (scalar)

  auto flush_rows = [&]() {
    if (s_rmin <= s_rmax) {
      const int y = f.t + s_row;
      const float a = backproject_y(s_rmin, y, k), b = backproject_y(s_rmax, y, k);
      ymn = vmin3(ymn, a, b);
      ymx = vmax3(ymx, a, b);
      rimn = vmin(rimn, (float)s_row);
      rimx = vmax(rimx, (float)s_row);
    }
    s_rmin = TSDF_INF;
    s_rmax = -TSDF_INF;
    cnt = 0;
  };

  // One pass over the rows for the columns [cbase, cbase + 64*P): lane <-> P consecutive columns, so a
  // row of up to 320 pixels is ONE visit with every lane busy (P = ceil(width / 64), at most 5).  Loads are
  // unconditional vector loads in straight-line code (rows past the band are clamped and ignored), two
  // register buffers in ping-pong: while one is reduced the other one's rows stream in behind a counted
  // vmcnt.  A lane whose window crosses the row end reads into the next row (masked); only in the very
  // last row of the frame would that leave the buffer, so that row alone takes guarded element loads.
  auto row_pass = [&](int cbase, auto p_tag) {
    constexpr int P = decltype(p_tag)::value;
    constexpr int kU = P <= 4 ? 4 : 3;           // rows per register buffer (bytes in flight vs VGPRs; deeper
                                                 // buffers in the split kernel did not shorten its latency)
    constexpr int kStep = kWaves * kU;
    float cmin[P], cmax[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      cmin[j] = TSDF_INF;
      cmax[j] = -TSDF_INF;
    }
    const int c0 = cbase + P * lane;
    bool mine[P];                                 // the lane owns column c0 + j
#pragma unroll
    for (int j = 0; j < P; ++j) mine[j] = c0 + j < f.bw;
    const int cload = mine[0] ? c0 : f.bw - P;    // lanes past the row reload its last P pixels (all masked)
    const bool ragged = (f.bw - cbase) % P != 0 && cbase + 64 * P >= f.bw;  // some lane straddles the row end
    const float nan = __builtin_nanf("");

    auto load_rows = [&](int row0, PixN<P> (&v)[kU]) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int row = row0 + kRowStep * u;
        const int rc = row < rend ? row : rend - 1;  // scalar
        const float *rp = f.depth + (int64_t)rc * f.bw;
        if (ragged && rc == f.bh - 1) {  // scalar, last row of the frame only: nothing may be read past it
#pragma unroll
          for (int j = 0; j < P; ++j) v[u].d[j] = mine[j] ? rp[c0 + j] : nan;
        } else {
          v[u] = load_pix<P>(rp + cload);
        }
      }
    };

    auto reduce_rows = [&](int row0, const PixN<P> (&v)[kU]) {
      if (cnt > 64 - kU) flush_rows();  // wave-uniform (cnt is)
      // ---- pass 1: which lanes of each row hold a pixel with |d| >= eps; ONE pool allocation for the kU rows.
      // (Columns past the row end are not masked here: such a lane holds pixels of the next row, or a reload
      // of this row's last pixels — either can only widen the captured window up to the row end, or make an
      // empty row look occupied; pass 2 applies the exact per-pixel rule.) ----
      unsigned long long vm[kU];       // 0: nothing to do for the row
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int row = row0 + kRowStep * u;
        float amax = __builtin_fabsf(v[u].d[0]);
#pragma unroll
        for (int j = 1; j < P; ++j) amax = vmax(amax, __builtin_fabsf(v[u].d[j]));  // NaN operands are dropped
        // most row segments hold no valid pixel at all: they are skipped wave-wide (rows past the band are
        // clamped duplicates of its last row)
        vm[u] = row < rend ? __ballot(amax >= k.eps) : 0ull;                          // pre/tsdf_numba.py:87
      }
      // ---- pass 2: the extents ----
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int row = row0 + kRowStep * u;
        if (vm[u]) {
          bool ok[P];
#pragma unroll
          for (int j = 0; j < P; ++j) ok[j] = (__builtin_fabsf(v[u].d[j]) >= k.eps) & mine[j];  // :87 (NaN -> invalid)
          if constexpr (AUG) {
            const double ym = (double)(f.t + row) - k.cy;
#pragma unroll
            for (int j = 0; j < P; ++j) {
              if (ok[j]) {
                const int col = c0 + j;
                const float dj = v[u].d[j];
                const double q = div_by_focal((double)dj, k);               // :91
                const double px = q * ((double)(f.l + col) - k.cx);         // :92
                const double py = (-q) * ym;                                // :93
                const double pz = -(double)dj;                              // :94
                const float ax = (float)affine_row(xf + 0, px, py, pz);
                const float ay = (float)affine_row(xf + 4, px, py, pz);
                const float az = (float)affine_row(xf + 8, px, py, pz);
                xmn = vmin(xmn, ax);
                xmx = vmax(xmx, ax);
                ymn = vmin(ymn, ay);
                ymx = vmax(ymx, ay);
                dmn = vmin(dmn, -az);  // stored negated: aabb_from_extents flips z back
                dmx = vmax(dmx, -az);
                cimn = vmin(cimn, (float)col);
                cimx = vmax(cimx, (float)col);
                rimn = vmin(rimn, (float)row);
                rimx = vmax(rimx, (float)row);
              }
            }
          } else {
            float rmin = TSDF_INF, rmax = -TSDF_INF;
#pragma unroll
            for (int j = 0; j < P; ++j) {
              const float lo = ok[j] ? v[u].d[j] : TSDF_INF;
              const float hi = ok[j] ? v[u].d[j] : -TSDF_INF;
              cmin[j] = vmin(cmin[j], lo);
              cmax[j] = vmax(cmax[j], hi);
              rmin = vmin(rmin, lo);
              rmax = vmax(rmax, hi);
            }
            const float wmin = wave_min(rmin), wmax = wave_max(rmax);
            if (lane == cnt) {
              s_rmin = wmin;
              s_rmax = wmax;
              s_row = row;
            }
            ++cnt;
          }
        }
      }
      // ---- pass 3: copy the lane windows lf..ll of every occupied row into the pool (a handful of LDS stores
      // under one exec mask) and post the rows' entries ----
      if (CAP && cap.on) {
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int row = row0 + kRowStep * u;
          if (row >= rend) continue;  // scalar
          unsigned ent = kRowEmpty;
          if (vm[u]) {
            const int lf = __builtin_ctzll(vm[u]), ll = 63 - __builtin_clzll(vm[u]);  // scalar
            const int need = (P * (ll - lf + 1) + 3) >> 2;
            if (cap_used + need <= cap.cap4) {
              const int off4 = cap.base4 + cap_used;
              cap_used += need;
              const int first = P * lf;
              const int endc = P * (ll + 1) < f.bw ? P * (ll + 1) : f.bw;  // a window crossing the row end is cut
              const LdsF dst = cap.pool + (4 * off4 + P * (lane - lf));
              if ((unsigned)(lane - lf) <= (unsigned)(ll - lf)) {
#pragma unroll
                for (int j = 0; j < P; ++j) dst[j] = v[u].d[j];
              }
              ent = row_pack(off4, first, endc - first);
            } else if (lane == 0) {
              *cap.fail = 1;
            }
          }
          if (lane == 0) cap.rowtab[row] = ent;
        }
      }
    };

    PixN<P> bufA[kU], bufB[kU];
    if constexpr (DEAL == kDealStatic) {
      load_rows(rbeg + wave, bufA);
      for (int row0 = rbeg + wave; row0 < rend; row0 += 2 * kStep) {
        load_rows(row0 + kStep, bufB);
        reduce_rows(row0, bufA);
        load_rows(row0 + 2 * kStep, bufA);
        reduce_rows(row0 + kStep, bufB);
      }
    } else {
      // Blocks.  The number of the block after the one being loaded is on its way while a buffer is reduced (an LDS
      // atomic with return is 3-7 us per frame on the critical path, see above: here its latency is behind kU rows'
      // arithmetic).  A number past the last block maps to rend: such a buffer loads clamped rows and reduces nothing,
      // like the static deal's rows past the band.  Numbers only grow, wave by wave, so a wave whose buffer A is past
      // the end has nothing in B either.  The counter serves ONE pass: a frame wider than a column pass takes its later
      // passes on fixed block numbers (wave + NW*i).
      constexpr int kOrder = kWaves;         // outside in, in runs of NW blocks (rowdeal.inc)
      const bool drawn = cbase == 0;         // scalar
      int held = wave + kWaves;              // fixed numbers: the last one taken
      auto next_block = [&]() -> int {
        if (drawn) {
          int t = 0;
          if (lane == 0) t = __hip_atomic_fetch_add(row_ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          return __builtin_amdgcn_readfirstlane(t);
        }
        held += kWaves;
        return held;
      };
      auto block_row = [&](int blk) -> int {
        int n;
        return rbeg + rowdeal_block(blk, rend - rbeg, kU, kOrder, n);
      };
      int rowA, rowB;
      if (drawn) {
        int t = 0;
        if (lane == 0) t = __hip_atomic_fetch_add(row_ctr, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        t = __builtin_amdgcn_readfirstlane(t);
        rowA = block_row(t);
        rowB = block_row(t + 1);
      } else {
        rowA = block_row(wave);
        rowB = block_row(wave + kWaves);
      }
      load_rows(rowA, bufA);
      while (rowA < rend) {
        load_rows(rowB, bufB);
        int nb = next_block();
        reduce_rows(rowA, bufA);
        rowA = block_row(nb);
        load_rows(rowA, bufA);
        nb = next_block();
        reduce_rows(rowB, bufB);
        rowB = block_row(nb);
      }
    }
    if constexpr (!AUG) {
      // column extremes of this wave's rows -> x extent; depth extremes -> z extent
#pragma unroll
      for (int j = 0; j < P; ++j) {
        if (cmin[j] <= cmax[j]) {
          const int col = c0 + j;
          const int x = f.l + col;
          const float a = backproject_x(cmin[j], x, k), b = backproject_x(cmax[j], x, k);
          xmn = vmin3(xmn, a, b);
          xmx = vmax3(xmx, a, b);
          dmn = vmin(dmn, cmin[j]);
          dmx = vmax(dmx, cmax[j]);
          cimn = vmin(cimn, (float)col);
          cimx = vmax(cimx, (float)col);
        }
      }
    }
  };
  // P is capped at 5 (320 columns per pass, the MSRA sensor width): wider windows only cost registers
  // (the whole kernel lives in 128 VGPRs) and would spill.
  if (rbeg < rend) {
    for (int cbase = 0; cbase < f.bw; cbase += 320) {
      const int w = f.bw - cbase;  // columns left (scalar)
      if (w <= 64) row_pass(cbase, std::integral_constant<int, 1>{});
      else if (w <= 128) row_pass(cbase, std::integral_constant<int, 2>{});
      else if (w <= 192) row_pass(cbase, std::integral_constant<int, 3>{});
      else if (w <= 256) row_pass(cbase, std::integral_constant<int, 4>{});
      else row_pass(cbase, std::integral_constant<int, 5>{});
    }
  }
  TSDF_STAMP(stamp_iter, 1);
  if constexpr (!AUG) TSDF_WSTAMP(stamp_iter, 0);   // per wave: rows done (the augmented voxel pass stamps these itself)
  flush_rows();
  TSDF_STAMP(stamp_iter, 2);

  // wave -> LDS -> every wave reduces the partials itself (no second barrier)
  float part[10];
  part[0] = wave_min(xmn);
  part[1] = wave_min(ymn);
  part[2] = wave_min(dmn);
  part[3] = wave_min(cimn);
  part[4] = wave_min(rimn);
  part[5] = wave_max(xmx);
  part[6] = wave_max(ymx);
  part[7] = wave_max(dmx);
  part[8] = wave_max(cimx);
  part[9] = wave_max(rimx);
  if (lane < 10) {
    float v = part[0];
#pragma unroll
    for (int i = 1; i < 10; ++i) v = (lane == i) ? part[i] : v;
    red[wave * kRedStride + lane] = v;
  }
  TSDF_STAMP(stamp_iter, 3);
  sync();
  static_assert(kWaves <= 16, "the cross-wave reduction uses one 16-lane DPP row");
  const bool has = (lane & 15) < kWaves;
  const int src = has ? (lane & 15) * kRedStride : 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) fin[i] = row0_min(has ? red[src + i] : TSDF_INF);
#pragma unroll
  for (int i = 5; i < 10; ++i) fin[i] = row0_max(has ? red[src + i] : -TSDF_INF);
}

__device__ __forceinline__ Aabb aabb_from_extents(const float (&fin)[kExt]) {
  Aabb a;
  a.any = fin[2] <= fin[7];
  a.mn[0] = fin[0];
  a.mn[1] = fin[1];
  a.mn[2] = -fin[7];  // cam_z = -d   pre/tsdf_numba.py:94
  a.mx[0] = fin[5];
  a.mx[1] = fin[6];
  a.mx[2] = -fin[2];
  a.c0 = a.any ? (int)fin[3] : 0;
  a.c1 = a.any ? (int)fin[8] : -1;
  a.r0 = a.any ? (int)fin[4] : 0;
  a.r1 = a.any ? (int)fin[9] : -1;
  return a;
}

// ---- glue: pre/tsdf_numba.py:142-147, float32, left to right --------------------------------
__device__ __forceinline__ Grid glue(const float (&mn)[3], const float (&mx)[3], int R, const CamK &k) {
  Grid g;
  float len[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    g.mid[a] = __fdiv_rn(__fadd_rn(mn[a], mx[a]), 2.0f);
    len[a] = __fsub_rn(mx[a], mn[a]);
  }
  g.max_l = fmaxf(len[0], fmaxf(len[1], len[2]));
  g.voxel_len = __fdiv_rn(g.max_l, (float)R);
  g.trunc = __fmul_rn(g.voxel_len, k.trunc_vox);
#pragma unroll
  for (int a = 0; a < 3; ++a)
    g.ori[a] = __fadd_rn(__fsub_rn(g.mid[a], __fdiv_rn(g.max_l, 2.0f)), __fdiv_rn(g.voxel_len, 2.0f));
  return g;
}

