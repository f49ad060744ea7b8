// frame.inc — part of the one translation unit tsdf_hip.hip (included there, inside its anonymous namespace).
// Per-frame pieces shared by the fused and the split kernel: kernel arguments, frame headers, LDS layout, group barrier, grid placement, scalar outputs, labels, LDS-DMA staging, table fill.

// ---- kernel arguments ---------------------------------------------------------------------------
struct KArgs {
  const float *depth;
  const int64_t *offsets;
  const int32_t *headers;
  int n, R;
  CamK cam;
  float *tsdf, *max_l, *mid_p;
  int32_t *status;
  float *aabb, *grid, *ori;
  int aabb_only;
  const float *grid_in;
  unsigned long long *queue;  // this launch's work-queue word, or null: CU-local queues (see the kernel)
  unsigned int qepoch;        // ... and the launch's number on that word (never 0): see queue_ticket()
  const double *xforms;
  int64_t depth_len;
  const int64_t *index;   // tsdf_voxelize_indexed_hip: batch position -> frame of the resident pack (else null)
  int64_t n_src;          // ... and the number of frames in that pack
  int n_inline;           // tsdf_voxelize_indexed_host_hip: the index travels IN the kernel arguments (n <= kInlineIndex)
  int64_t inline_index[TSDF_INLINE_INDEX_MAX];
  const float *gt;        // labels (optional)
  float *gt_nor, *gt_aug;
  int n_joints, clamp;
  int32_t *pixmap;        // diagnostic pixel map (DBG instantiations only)
  int split, per;         // split kernel: workgroups per frame, slow-axis slices per workgroup
  float *xchg;            // split kernel: this stream's mailboxes for partial extents, or null (see the kernel)
  unsigned int seq;       // ... and the number this launch tags them with
  int polls;              // ... and the bound of the wait for them (kXchgPolls; tests set TSDF_XCHG_POLLS=0 to
                          // force every workgroup onto the fallback)
  const float *pca_mean, *pca_coeff;  // joint PCA (tsdf_pca; with labels only): mu[C], W[C][C]
  float *gt_pca;                      // ... out [n][pca_k]
  int pca_k;                          // ... K, or 0: no projection
};

// ---- synchronisation inside one half-workgroup (group) -------------------------------------------
// s_barrier spans all 16 waves, so the 8 waves of a group meet on an LDS counter instead: monotonic
// count, lane 0 of each wave adds 1 and polls until the group's epoch target is reached.  LDS
// operations of a wave execute in order, so everything a wave wrote to LDS before its arrival is
// visible to whoever sees the count.  Only LDS is ordered here (no vmcnt wait: output stores stay
// in flight across these barriers).
struct FrameHdr {
  int frame;  // -1: no more work
  int l, t, r, b;
  int pad;
  int64_t off0, off1;
  int64_t src;  // where the frame's offsets / header / labels are read: `frame`, or index[frame] (indexed entry)
};

// The frame's header and offsets.  Indexed entry: batch position fr reads pack frame index[fr]; an index outside the
// pack leaves off1 < off0, which frame_from_header turns into TSDF_FRAME_BAD_HEADER (nothing is read through it).
__device__ __forceinline__ void fetch_header(const KArgs &a, const int64_t *__restrict__ in_offsets,
                                             const int32_t *__restrict__ in_headers, int fr, FrameHdr &m) {
  int64_t src = fr;
  bool ok = true;
  if (a.n_inline) {           // a small batch whose index came by value: no memory outside the kernel arguments is read
    src = a.inline_index[fr];
    ok = src >= 0 && src < a.n_src;
    if (!ok) src = 0;
  } else if (a.index) {
    src = a.index[fr];
    ok = src >= 0 && src < a.n_src;
    if (!ok) src = 0;
  }
  const int32_t *h = in_headers + 6 * src;
  m.l = h[2];
  m.t = h[3];
  m.r = h[4];
  m.b = h[5];
  m.off0 = in_offsets[src];
  m.off1 = ok ? in_offsets[src + 1] : m.off0 - 1;
  m.src = src;
}

// Tail help: a group that finds the queue empty does not leave at once.  It raises idle[] and waits; the
// CU's other group, on reaching phase 2 of what is then necessarily its last frame, sees the flag, posts
// the frame's voxel parameters here and both groups split the slow axis of the volume (the pool and the
// tables are in LDS, which the two share).  Nothing has to be handed back: the helper leaves when done.
struct HelpReq {
  Grid g;
  VoxK vk;
  const float *src;  // the frame in global memory (gather source when the frame was not captured)
  float *out;
  int frame, use_tab, mode, owner;  // mode: FillMode
  int pm_bw, pm_dc, pm_dr, pad;     // diagnostic map: see PixMapK
};

struct GroupCtl {
  int bar[kMaxGroups];
  int local_next;         // CU-local work queue (launches without a global queue word)
  int tile_next;          // one-group instantiations: the voxel pass's unit counter (dynamic units)
  int lock;               // the pool lock: one group at a time between the extents barrier and the end of phase 2
  int help_for;           // 0: none; g+1: group g is asked to help with the frame in `help`
  int idle[kMaxGroups];
  int cap_fail[kMaxGroups];  // a row of the group's current frame did not fit the pool
  FrameHdr hdr[kMaxGroups];  // mailbox: the group's first wave fetches the next frame for the others
  HelpReq help;
  int row_next[kMaxGroups];  // the row stream's next block number (drawn deal: phase1.inc), reset with every header; last,
                             // so that no other member moves (the block's size, rounded to 16 bytes, stays what it was)
};

// How a frame's pixels get into LDS for the voxel pass.
//   Fused kernel: after phase 1, the rectangle holding every valid pixel is copied into the pool by LDS-DMA
//   (global_load_lds_dwordx4: no VGPR staging, all of a wave's 1 KiB pieces in flight at once); the pool is ONE resource
//   the two groups take turns on through a lock taken on the way into the extents barrier.  The rows come from L2 /
//   Infinity Cache a second time (+10 % fabric traffic).  (The alternative — capturing every row's span of valid pixels
//   during phase 1: depth read exactly once, no lock — measured slower on every workload, rounds 2-4; it is no longer
//   built into the fused kernel: tools/patches/r05_removed_knobs.diff.)
//   Split kernel: the exchange form stages the same way; the redundant form (one workgroup streams the whole frame)
//   captures the spans — one frame per workgroup: everything fits, nothing to take turns on.

__device__ __forceinline__ int lds_load(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_store(int *p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int GWAVES>
__device__ __forceinline__ void group_barrier(int *cnt, int &target) {
  target += GWAVES;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if ((threadIdx.x & 63) == 0) {
    __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target)
      __builtin_amdgcn_s_sleep(1);
  }
  asm volatile("" ::: "memory");
}

// ---- the workgroup's LDS: everything the CU has --------------------------------------------------
// Per group: projection tables, z table, (AUG) inverse-map products, row table, reduction scratch.
// Shared: control block and the row-span pool, which gets all the rest.
template <int RT, bool AUG, int GROUPS = 2>
struct Lds {
  static constexpr int kZ = RT ? RT : kMaxR;
  static constexpr bool kHasTab = !AUG && (RT == 0 || RT <= kTabR);
  static constexpr int kTabN = kHasTab ? kTabR * kTabR : 16;
  struct PerGroup {
    alignas(16) unsigned pytab[kTabN];
    alignas(16) int pxtab[kTabN];
    alignas(16) unsigned char pyrow[kTabN];
    alignas(16) ZEntry ztab[kZ];
    alignas(16) double atab[AUG ? 12 * kZ : 2];
    alignas(16) unsigned rowtab[kMaxRows];
    alignas(16) float red[16 * kRedStride];  // 16 waves in the split kernel
  };
  static constexpr int kFixed = GROUPS * (int)sizeof(PerGroup) + (int)sizeof(GroupCtl) + 64;
  static constexpr int kPoolFloats = ((kLdsBytes - kFixed) / 16) * 4;
  static constexpr int kPoolUnits = kPoolFloats / 4;
  static_assert(kPoolUnits < 16384, "pool offsets are 14 bits of 4-float units");
  struct Block {
    alignas(16) float pool[kPoolFloats];
    PerGroup pg[GROUPS];
    alignas(16) GroupCtl ctl;
  };
  static_assert(sizeof(Block) <= kLdsBytes, "LDS layout exceeds the CU");
  static_assert(RT != 32 || AUG || GROUPS != 2 || kPoolFloats == 34968, "the headline's pool keeps its size");
};

template <class PG>
__device__ __forceinline__ Tabs make_tabs(PG &pg) {
  Tabs t;
  t.ztab = (LdsZ)pg.ztab;
  t.pxtab = (LdsCI)pg.pxtab;
  t.pytab = (LdsCU)pg.pytab;
  t.pyrow = (LdsCU8)pg.pyrow;
  t.rowtab = (LdsCU)pg.rowtab;
  t.atab = (LdsCD)pg.atab;
  return t;
}

// ---- per-frame pieces shared by the fused and the split kernel ------------------------------------
// A header that contradicts its payload, or a payload outside the depth buffer, is never read.
__device__ __forceinline__ bool frame_from_header(const FrameHdr &fh, const float *depth, int64_t depth_len, Frame &f) {
  f.l = __builtin_amdgcn_readfirstlane(fh.l);
  f.t = __builtin_amdgcn_readfirstlane(fh.t);
  f.r = __builtin_amdgcn_readfirstlane(fh.r);
  f.b = __builtin_amdgcn_readfirstlane(fh.b);
  const int64_t bw = (int64_t)f.r - f.l, bh = (int64_t)f.b - f.t;  // cannot overflow in 64 bits
  f.bw = (int)bw;
  f.bh = (int)bh;
  f.depth = depth + fh.off0;
  return bw > 0 && bh > 0 && bw <= 0x7fffffff && bh <= 0x7fffffff && bw * bh == fh.off1 - fh.off0 && fh.off0 >= 0 &&
         fh.off1 <= depth_len;
}

// AABB -> grid placement and frame status (degenerate-frame rule of include/tsdf.h).
__device__ __forceinline__ void place_grid(Aabb &ab, int R, const CamK &cam, const float *grid_in, int frame,
                                           Grid &g, int &status) {
  if (!ab.any) {
    status = TSDF_FRAME_DEGENERATE;
    ab.mn[0] = ab.mn[1] = ab.mn[2] = ab.mx[0] = ab.mx[1] = ab.mx[2] = 0.f;
    return;
  }
  g = glue(ab.mn, ab.mx, R, cam);
  if (grid_in) {
    // caller-supplied placement (tsdf_cal's vox_ori, voxel_len, truncation arguments)
    const float *gi = grid_in + 8 * (int64_t)frame;
    g.ori[0] = gi[0];
    g.ori[1] = gi[1];
    g.ori[2] = gi[2];
    g.voxel_len = gi[3];
    g.trunc = gi[4];
    if (!(g.trunc > 0.f) || !(g.trunc < TSDF_INF)) status = TSDF_FRAME_DEGENERATE;
    return;
  }
  const bool mid_ok = finite32(g.mid[0]) && finite32(g.mid[1]) && finite32(g.mid[2]);
  if (!(g.max_l > 0.f) || !(g.max_l < TSDF_INF) || !mid_ok) {
    status = TSDF_FRAME_DEGENERATE;
    g.max_l = g.voxel_len = g.trunc = 0.f;
    if (!mid_ok) g.mid[0] = g.mid[1] = g.mid[2] = 0.f;
  }
}

// one thread per frame writes the scalars
__device__ __forceinline__ void write_frame_outputs(const KArgs &a, int frame, const Grid &g, const Aabb &ab, int status) {
  if (a.max_l) a.max_l[frame] = g.max_l;
  if (a.mid_p) {
    a.mid_p[3 * (int64_t)frame + 0] = g.mid[0];
    a.mid_p[3 * (int64_t)frame + 1] = g.mid[1];
    a.mid_p[3 * (int64_t)frame + 2] = g.mid[2];
  }
  if (a.status) a.status[frame] = status;
  if (a.aabb) {
    float *o = a.aabb + 6 * (int64_t)frame;
    o[0] = ab.mn[0]; o[1] = ab.mn[1]; o[2] = ab.mn[2];
    o[3] = ab.mx[0]; o[4] = ab.mx[1]; o[5] = ab.mx[2];
  }
  if (a.grid) {
    float *q = a.grid + 8 * (int64_t)frame;
    q[0] = g.mid[0]; q[1] = g.mid[1]; q[2] = g.mid[2];
    q[3] = g.max_l; q[4] = g.voxel_len; q[5] = g.trunc; q[6] = 0.f; q[7] = 0.f;
  }
  if (a.ori) {
    float *q = a.ori + 3 * (int64_t)frame;
    q[0] = g.ori[0]; q[1] = g.ori[1]; q[2] = g.ori[2];
  }
}

// Labels: pre/joint_nor.py:8-18 + the clamp of 3D_CNN/train.py:241-242, float32, three separately rounded
// operations; AUG maps the joints with the frame's forward map first (pre/process.py:232-249 does it with the
// cloud's S and R).  Frames that are not OK get 0.5 (see include/tsdf.h).
// Joint PCA projection of one frame (include/tsdf.h, tsdf_pca items 1 and 3).  Each wave whose first thread index is
// below K owns 64 components (lane i: k = 64w + i).  The coordinates go 64 at a time: lane i normalises coordinate c0 + i
// (all lanes in parallel: one division each), then the wave walks them in ascending order, broadcasting t_j with
// v_readlane, and every lane adds t_j * W[j][k] to its float64 sum — the contract's order, with no LDS and no barrier.
// gj: the frame's joints (mm), xf: its forward map or null, ok: the frame is TSDF_FRAME_OK (max_l > 0).
// Wave-uniform control flow throughout (tid & ~63 and the loop bounds are the same for every lane of a wave).
__device__ __forceinline__ void pca_project(const float *__restrict__ gj, const double *xf, const float mid[3],
                                            float max_l, bool ok, const float *__restrict__ mean,
                                            const float *__restrict__ W, int nc, int K, float *__restrict__ out,
                                            int tid, int T) {
  const int lane = tid & 63;
  for (int k0 = tid & ~63; k0 < K; k0 += T) {
    const int k = k0 + lane;
    const bool kin = k < K;
    const int kc = kin ? k : K - 1;   // (lanes past K read a valid column and discard it)
    double p = 0.0;
    for (int c0 = 0; c0 < nc; c0 += 64) {
      const int e = c0 + lane;
      float t = 0.f;
      if (e < nc) {
        const int c = e % 3;
        const float *g3 = gj + (e - c);
        float v = g3[c];
        if (xf) v = (float)affine_row(xf + 4 * c, (double)g3[0], (double)g3[1], (double)g3[2]);
        const float m = c == 0 ? mid[0] : (c == 1 ? mid[1] : mid[2]);
        const float u = ok ? __fadd_rn(__fdiv_rn(__fsub_rn(v, m), max_l), 0.5f) : 0.5f;
        t = __fsub_rn(u, mean[e]);
      }
      const int cnt = nc - c0 < 64 ? nc - c0 : 64;
      const float *w = W + (int64_t)c0 * nc + kc;
      // 16 coefficients are loaded before the 16 dependent adds that use them, by UNCONDITIONAL loads of clamped (valid)
      // addresses: a guarded load becomes a branch with its own vmcnt(0) wait, one L2 round trip per coordinate.  Fixed
      // trip counts around the convergent v_readlane; past cnt the term is +0 * +0, which leaves p unchanged (p is
      // never -0).
      for (int i0 = 0; i0 < 64; i0 += 16) {
        float wv[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int i = i0 + q < cnt ? i0 + q : cnt - 1;
          const float v = w[(int64_t)i * nc];
          wv[q] = i0 + q < cnt ? v : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float ti = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(t), i0 + q));
          p = __dadd_rn(p, __dmul_rn((double)ti, (double)wv[q]));   // exact product, one rounding
        }
      }
    }
    if (kin) out[k] = (float)p;
  }
}

template <bool PCA>
__device__ __forceinline__ void write_labels(const KArgs &a, int frame, int64_t src, const Grid &g, int status,
                                             const double *xf, int tid, int T) {
  if (!a.gt) return;
  const int nc = 3 * a.n_joints;
  if constexpr (PCA)   // (the projection uses the unclamped labels, whatever a.clamp says)
    pca_project(a.gt + src * nc, xf, g.mid, g.max_l, status == TSDF_FRAME_OK, a.pca_mean, a.pca_coeff, nc, a.pca_k,
                a.gt_pca + (int64_t)frame * a.pca_k, tid, T);
  for (int e = tid; e < nc; e += T) {
    const int c = e % 3;
    const float *gj = a.gt + src * nc + (e - c);
    float v = gj[c];
    if (xf) v = (float)affine_row(xf + 4 * c, (double)gj[0], (double)gj[1], (double)gj[2]);
    if (a.gt_aug) a.gt_aug[(int64_t)frame * nc + e] = v;  // the joints in the grid's frame (plain path: a copy)
    float o = 0.5f;
    if (status == TSDF_FRAME_OK) {
      const float m = c == 0 ? g.mid[0] : (c == 1 ? g.mid[1] : g.mid[2]);
      o = __fadd_rn(__fdiv_rn(__fsub_rn(v, m), g.max_l), 0.5f);
      if (a.clamp) {
        o = o < 0.f ? 0.f : o;
        o = o > 1.f ? 1.f : o;
      }
    }
    a.gt_nor[(int64_t)frame * nc + e] = o;
  }
}

// How a frame's pixels reach the voxel pass.
enum FillMode {
  kFillGlobal = 0,  // gather from the crop in global memory (L2)
  kFillSpans = 1,   // row spans captured into the pool during phase 1; per-row entries (split kernel, redundant form)
  kFillRect = 2     // rectangle of valid pixels staged into the pool by LDS-DMA after phase 1
};

// Voxel-pass constants.  Pixel coordinates are relative to a frame of reference: the bounding box for span
// entries, the rectangle holding every valid pixel otherwise (whole_bbox: the bounding box there too — the
// diagnostic map has to tell "outside the bounding box" from "invalid pixel").
__device__ __forceinline__ VoxK make_voxk(const CamK &cam, const Grid &g, const Frame &f, const Aabb &ab,
                                          int mode, bool whole_bbox, int rect_stride) {
  VoxK vk;
  vk.cx = cam.cx;
  vk.cy = cam.cy;
  vk.it = 1.0 / (double)g.trunc;
  vk.kq = cam.inv_focal * vk.it;
  vk.ncx = -cam.cx;
  vk.eps = cam.eps;
  int c0 = ab.c0, r0 = ab.r0, w = ab.c1 - ab.c0 + 1, h = ab.r1 - ab.r0 + 1;
  if (mode == kFillSpans || whole_bbox) {
    c0 = r0 = 0;
    w = f.bw;
    h = f.bh;
  }
  vk.px0 = f.l + c0;
  vk.py0 = f.t + r0;
  vk.dx = w - 1;
  vk.dy = h - 1;
  vk.stride = mode == kFillRect ? rect_stride : f.bw;
  vk.stride4 = 4 * vk.stride;
  vk.base = mode == kFillGlobal ? r0 * f.bw + c0 : 0;
  vk.dxc = (double)vk.px0 - cam.cx;
  vk.dyc = (double)vk.py0 - cam.cy;
  return vk;
}

// Copy the sh x sw4 pixel rectangle that starts at (row sr0, column sc0) of the frame's crop into the pool by LDS-DMA
// (global_load_lds_dwordx4), NWV waves sharing the rows.  No VGPR staging and no ds_write pass: each wave
// instruction moves up to 64 x 16 B straight into the row-major LDS image (lane i lands at base + 16*i, so lanes are
// laid out as [row][4-pixel group]); all of a wave's pieces are in flight at once.  Sources need only 4-byte
// alignment and EXEC-masked lanes leave their slot untouched (tools/probes/glds_probe.hip).  Completion is counted
// in vmcnt: the caller waits for vmcnt(0) before its barrier.
template <int NWV>
__device__ __forceinline__ void stage_rect_dma(float *stage, const Frame &f, int64_t n_frame, int sc0, int sr0, int sh,
                                               int sw4, int wave, int lane) {
  const int ng = sw4 >> 2;                       // 4-pixel groups per row
  const int64_t base_idx = (int64_t)sr0 * f.bw + sc0;
  if (ng <= 64) {
    const int rows_per = 64 / ng;                // rows one wave instruction covers
    const int rsub = lane / ng, cg = lane - rsub * ng;
    const int nblk = (sh + rows_per - 1) / rows_per;
    for (int blk = wave; blk < nblk; blk += NWV) {
      const int R0 = blk * rows_per;             // scalar
      const int row = R0 + rsub;
      const int64_t gi = base_idx + (int64_t)row * f.bw + 4 * cg;
      const bool act = rsub < rows_per && row < sh;
      float *ldst = stage + R0 * sw4;            // wave-uniform LDS base
      if (act && gi + 3 < n_frame) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(f.depth + gi),
                                         (__attribute__((address_space(3))) void *)ldst, 16, 0, 0);
      } else if (act) {  // the 16-byte piece would run past the end of the frame: element copies
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (gi + e < n_frame) ldst[(rsub * ng + cg) * 4 + e] = f.depth[gi + e];
      }
    }
  } else {
    for (int row = wave; row < sh; row += NWV) {
      for (int c4 = 0; c4 < ng; c4 += 64) {
        const int cg = c4 + lane;
        const int64_t gi = base_idx + (int64_t)row * f.bw + 4 * cg;
        float *ldst = stage + row * sw4 + 4 * c4;  // wave-uniform
        if (cg < ng && gi + 3 < n_frame) {
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(f.depth + gi),
                                           (__attribute__((address_space(3))) void *)ldst, 16, 0, 0);
        } else if (cg < ng) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (gi + e < n_frame) ldst[lane * 4 + e] = f.depth[gi + e];
        }
      }
    }
  }
}

// Per-frame tables (true divisions; (x,z)/(y,z) pairs spread over the T participating threads).
template <int LAYOUT, bool AUG, class PG>
__device__ __forceinline__ void fill_tables(PG &pg, const Grid &g, const CamK &cam, const VoxK &vk, int R,
                                            bool use_tab, bool spans, const double *xf, int vt, int T) {
  const double vl = (double)g.voxel_len;
  const double ox = (double)g.ori[0], oy = (double)g.ori[1], oz = (double)g.ori[2];
  if (vt < R) {
    const double v_z = oz + (double)vt * vl;  // :28
    ZEntry ze;
    ze.q = -cam.focal / v_z;                    // :30
    ze.vzs = v_z * vk.it;
    ze.negthr = f32_round_up(-v_z);             // pd < -v_z  <=>  w_z > v_z  (:65)
    ze.pad = 0.f;
    pg.ztab[vt] = ze;
  }
  if constexpr (AUG) {
    // per (axis, index): the three products of the inverse map and v' - b of the forward map: see phase2_aug
    const double *inv = xf + 12;
    for (int e = vt; e < 12 * R; e += T) {
      const int axis = e / (4 * R), rem = e - axis * 4 * R, i = rem >> 2, row = rem & 3;
      const double o_a = axis == 0 ? ox : (axis == 1 ? oy : oz);
      const double vp = o_a + (double)i * vl;                    // :26-28
      // the axis the lanes index is stored lane-major (lane_slot), the two the slices / slabs index as [index][4]
      const int at = axis == (LAYOUT == 0 ? 0 : 2) ? 4 * R * axis + lane_slot(i, row, R / 4) : e;
      if (row < 3) {
        const double prod = inv[4 * row + axis] * vp;
        pg.atab[at] = axis == 2 ? prod + inv[4 * row + 3] : prod;   // the z entries carry the translation
      } else {
        pg.atab[at] = vp - xf[4 * axis + 3];
      }
    }
  }
  if (use_tab) {
    for (int e = vt; e < R * R; e += T) {
      const int z = e / R, i = e - z * R;
      const double q = -cam.focal / (oz + (double)z * vl);                              // :30
      const double vx = ox + (double)i * vl, vy = oy + (double)i * vl;                  // :26-27
      const int ti = tab_index<LAYOUT>(i, z, R);
      pg.pxtab[ti] = col_code(project_rel(vx, q, cam.cx, vk.px0, vk.dx));               // :31
      const int ry = project_rel(-vy, q, cam.cy, vk.py0, vk.dy);                        // :32
      if (spans) {
        pg.pytab[ti] = ry >= 0 ? pg.rowtab[ry] : 0u;
        pg.pyrow[ti] = (unsigned char)(ry >= 0 ? ry : 0);
      } else {
        pg.pytab[ti] = (unsigned)ry;
      }
    }
  }
}

