// kernels.inc — part of the one translation unit tsdf_hip.hip (included there, inside its anonymous namespace).
// The kernels: tsdf_fused_kernel (persistent, one workgroup per CU), tsdf_split_kernel (small batches), tsdf_normalize_kernel (labels alone),
// tsdf_project_kernel (joint-PCA projection alone), tsdf_pose_error_kernel (decode + per-joint error).

// Persistent kernel, one 1024-thread workgroup per CU.  Its two 512-thread groups each walk their own
// frames through
//     stream rows -> extents -> glue                                        memory-bound
//     stage the valid pixels' rectangle (LDS-DMA) + tables -> voxel pass    store-bound (augmented: + VALU)
// independently of each other, so one group's row streaming overlaps the other group's voxel arithmetic
// and stores on the same CU.
// (The read-only inputs are passed as separate __restrict__ parameters as well as inside KArgs: alias information
// does not survive a by-value struct, and without it the compiler may not use scalar loads for wave-uniform
// reads — the per-frame transform of the augmented form became 700 vector loads in the unrolled row pass.)
// PCA: the joint-PCA projection rides on the labels (tsdf_pca) — a compile-time variant, so that the instantiations
// without it compile to exactly what they were.
template <int RT, int LAYOUT, bool AUG, bool DBG, int GROUPS, bool PCA>
__global__ __launch_bounds__(kWG) void tsdf_fused_kernel(const KArgs a, const float *__restrict__ in_depth,
                                                         const int64_t *__restrict__ in_offsets,
                                                         const int32_t *__restrict__ in_headers,
                                                         const double *__restrict__ in_xforms) {
  constexpr int kGroups = GROUPS, kGW = kWG / GROUPS, kGWaves = kGW / 64;  // (shadow the file-scope defaults)
  using L = Lds<RT, AUG, GROUPS>;
  __shared__ typename L::Block lds;
  // the two-group instantiations of a fixed resolution without augmentation draw row blocks (phase1.inc); the others
  // keep the static deal (no paired A/B of their workloads says they would gain) and compile to what they were
  constexpr int kDeal = (GROUPS == 2 && !AUG && RT != 0) ? kDealDrawn : kDealStatic;

  const int R = RT ? RT : a.R;
  const CamK &cam = a.cam;
  const int n = a.n;
  const int tid = threadIdx.x, lane = tid & 63, gtid = tid & (kGW - 1);
  const int group = __builtin_amdgcn_readfirstlane(tid / kGW);
  const int gwave = __builtin_amdgcn_readfirstlane((tid >> 6) & (kGWaves - 1));
  auto &pg = lds.pg[group];
  GroupCtl &ctl = lds.ctl;

  if (tid == 0) {
    for (int i = 0; i < kGroups; ++i) ctl.bar[i] = ctl.idle[i] = ctl.cap_fail[i] = 0;
    ctl.lock = 0;
    ctl.help_for = 0;
    ctl.local_next = kGroups;
  }
  __syncthreads();  // the only workgroup-wide barrier
  int bar_target = 0;
  auto gsync = [&]() { group_barrier<kGWaves>(&ctl.bar[group], bar_target); };

  Capture cap;   // (row-span capture is the split kernel's; phase 1 is instantiated without it here)
  cap.pool = (LdsF)lds.pool;
  cap.rowtab = (LdsU)pg.rowtab;
  cap.fail = (LdsI)&ctl.cap_fail[group];
  cap.cap4 = 0;
  cap.base4 = 0;
  cap.on = false;

  const int n_static = gridDim.x * kGroups;  // frames handed out by position (the first one per group)

  int iter = 0;
  (void)iter;
  for (;; ++iter) {
    // ---- the group's first wave fetches the next frame (index + header) and posts it in LDS ----
    if (gwave == 0) {
      int fr;
      if (iter == 0) {
        fr = blockIdx.x + gridDim.x * group;
      } else if (a.queue) {
        unsigned int t = 0;
        if (lane == 0) {
          t = queue_ticket(a.queue, a.qepoch, n);
        }
        fr = n_static + (int)__builtin_amdgcn_readfirstlane(t);
      } else {
        int t = 0;
        if (lane == 0) t = __hip_atomic_fetch_add(&ctl.local_next, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const int64_t f64i = (int64_t)blockIdx.x + (int64_t)gridDim.x * __builtin_amdgcn_readfirstlane(t);
        fr = f64i < n ? (int)f64i : n;
      }
      FrameHdr m;
      m.frame = fr < n ? fr : -1;
      m.l = m.t = m.r = m.b = m.pad = 0;
      m.off0 = m.off1 = m.src = 0;
      if (fr < n) fetch_header(a, in_offsets, in_headers, fr, m);
      if (lane == 0) {
        ctl.hdr[group] = m;
        ctl.cap_fail[group] = 0;
        if constexpr (kDeal == kDealDrawn) ctl.row_next[group] = 0;   // the row stream's block counter (phase 1)
      }
    }
    gsync();
    const FrameHdr fh = ctl.hdr[group];
    const int frame = __builtin_amdgcn_readfirstlane(fh.frame);
    if (frame < 0) break;
    TSDF_STAMP(kGroups * iter + group, 0);

    Frame f;
    const bool hdr_ok = frame_from_header(fh, in_depth, a.depth_len, f);
    float *out = a.tsdf ? a.tsdf + (int64_t)frame * 3 * R * R * R : nullptr;
    const bool want_vol = !a.aabb_only && out;

    int status = TSDF_FRAME_OK;
    Aabb ab;
    ab.any = false;
    ab.mn[0] = ab.mn[1] = ab.mn[2] = ab.mx[0] = ab.mx[1] = ab.mx[2] = 0.f;
    ab.c0 = ab.r0 = 0;
    ab.c1 = ab.r1 = -1;
    Grid g;
    g.mid[0] = g.mid[1] = g.mid[2] = 0.f;
    g.max_l = g.voxel_len = g.trunc = 0.f;
    g.ori[0] = g.ori[1] = g.ori[2] = 0.f;
    const double *xf = AUG ? in_xforms + 24 * (int64_t)frame : nullptr;

    bool holds_lock = false;  // group-uniform
    if (!hdr_ok) {
      status = TSDF_FRAME_BAD_HEADER;  // group-uniform
    } else {
      float fin[kExt];
      auto sync_ext = [&]() {
        // The group's first wave takes the pool lock on its way into the extents barrier, so the wait for
        // the other group's voxel pass hides behind this group's own slowest wave.
        if (want_vol && gwave == 0 && lane == 0) {
          while (atomicCAS(&ctl.lock, 0, 1) != 0) __builtin_amdgcn_s_sleep(2);
        }
        gsync();
      };
      phase1_extents<kGWaves, AUG, false, kDeal>(f, cam, 0, f.bh, pg.red, fin, gwave, sync_ext, cap,
                                                 kGroups * iter + group, xf, &ctl.row_next[group]);
      holds_lock = want_vol;
      ab = aabb_from_extents(fin);
      TSDF_STAMP(kGroups * iter + group, 4);
      place_grid(ab, R, cam, a.grid_in, frame, g, status);
    }

    if (gtid == 0) write_frame_outputs(a, frame, g, ab, status);
    write_labels<PCA>(a, frame, fh.src, g, status, xf, gtid, kGW);

    if (want_vol) {
      if (status != TSDF_FRAME_OK) {
        zero_volume(out, R, gtid, kGW, 0, 1);
        if constexpr (DBG) {
          if (a.pixmap)
            for (int i = gtid; i < R * R * R; i += kGW) a.pixmap[(int64_t)frame * R * R * R + i] = -1;
        }
      } else {
        // The thread's index for the tables and the voxel pass, hidden from loop-invariant code motion:
        // otherwise every constant derived from it (a dozen float64 conversions of voxel indices) is
        // computed once before the frame loop and then occupies registers, or scratch, all through phase 1.
        int vt = gtid;
        asm volatile("" : "+v"(vt));
        // ---- stage the valid pixels' rectangle into the pool by LDS-DMA.  The group holds the pool lock here (taken
        // at the extents barrier), so the whole pool is its own.
        int mode = kFillGlobal;
        // the staged image: the rectangle of valid pixels (the whole bounding box in the diagnostic build),
        // row-major from the start of the pool, rows padded to a multiple of 4 pixels (16-byte DMA pieces)
        const int sc0 = DBG ? 0 : ab.c0, sr0 = DBG ? 0 : ab.r0;
        const int sw = DBG ? f.bw : ab.c1 - ab.c0 + 1, sh = DBG ? f.bh : ab.r1 - ab.r0 + 1;
        const int sw4 = (sw + 3) & ~3;
        const bool staged = (int64_t)sw4 * sh <= L::kPoolFloats;  // group-uniform
        if (staged) {
          mode = kFillRect;
          stage_rect_dma<kGWaves>(lds.pool, f, fh.off1 - fh.off0, sc0, sr0, sh, sw4, gwave, lane);
        }
        const VoxK vk = make_voxk(cam, g, f, ab, mode, DBG, sw4);
        const bool use_tab = !AUG && R <= kTabR;  // uniform
        TSDF_STAMP(kGroups * iter + group, 5);
        fill_tables<LAYOUT, AUG>(pg, g, cam, vk, R, use_tab, false, xf, vt, kGW);
        TSDF_STAMP(kGroups * iter + group, 6);
        // the copy was issued before the tables were computed (worth 1.1 % of the launch, round 1)
        if (staged) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // LDS-DMA completion is counted in vmcnt
        TSDF_STAMP(kGroups * iter + group, 7);
        if constexpr (kGroups == 2) {
          if (gwave == 0 && lane == 0) ctl.hdr[group].pad = lds_load(&ctl.idle[group ^ 1]);
        }
        if constexpr (kGroups == 1) {
          if (gwave == 0 && lane == 0) lds_store(&ctl.tile_next, 0);   // ordered by the barrier below
        }
        gsync();
        TSDF_STAMP(kGroups * iter + group, 8);
        bool helped = false;  // group-uniform
        if constexpr (kGroups == 2) {
          // the other group is idle (so this is the launch's last frame on this CU): split the volume with it
          if (__builtin_amdgcn_readfirstlane(ctl.hdr[group].pad)) {
            helped = true;
            if (gwave == 0 && lane == 0) {
              HelpReq hq;
              hq.g = g;
              hq.vk = vk;
              hq.src = f.depth + vk.base;
              hq.mode = mode;
              hq.owner = group;
              hq.out = out;
              hq.frame = frame;
              hq.use_tab = use_tab;
              hq.pm_bw = f.bw;
              hq.pm_dc = vk.px0 - f.l;
              hq.pm_dr = vk.py0 - f.t;
              hq.pad = 0;
              ctl.help = hq;
              lds_store(&ctl.help_for, (group ^ 1) + 1);
            }
          }
        }
        TSDF_STAMP_VAL(kGroups * iter + group, 10, helped ? 2 : 1);
        const Tabs tb = make_tabs(pg);
        PixMapK pm;
        pm.out = DBG && a.pixmap ? (GlobalPix)(a.pixmap + (int64_t)frame * R * R * R) : (GlobalPix) nullptr;
        pm.bw = f.bw;
        pm.dc = vk.px0 - f.l;
        pm.dr = vk.py0 - f.t;
        auto run2 = [&](auto src) {
          if constexpr (kGroups == 2) {
            if (__builtin_expect(helped, 0)) {
              if constexpr (AUG) {
                phase2_aug<LAYOUT, 2 * kGW>(g, cam, vk, R, xf, tb, src, (GlobalOut)out, vt, 0, R);
              } else {
                phase2<LAYOUT, 2 * kGW, DBG>(g, cam, vk, R, tb, use_tab, src, (GlobalOut)out, vt, 0, R, pm);
              }
              return;
            }
          }
          if constexpr (AUG) {
            phase2_aug<LAYOUT, kGW>(g, cam, vk, R, xf, tb, src, (GlobalOut)out, vt, 0, R,
                                    kGroups == 1 ? &ctl.tile_next : nullptr, kGroups * iter + group);
          } else {
            phase2<LAYOUT, kGW, DBG>(g, cam, vk, R, tb, use_tab, src, (GlobalOut)out, vt, 0, R, pm,
                                     kGroups == 1 ? &ctl.tile_next : nullptr);
          }
        };
        if (mode == kFillRect) {
          run2(LdsRect{(LdsSrc)lds.pool});
        } else {
          run2((GlobalSrc)(f.depth + vk.base));
        }
      }
    }
    TSDF_STAMP(kGroups * iter + group, 9);
    // Close the frame: every wave of the group has left the LDS it shares (pool spans, tables, `red`, the
    // header mailbox) before the next frame rewrites them.
    gsync();
    if (holds_lock && gwave == 0 && lane == 0)
      __hip_atomic_store(&ctl.lock, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  // ---- queue empty: offer help with the other group's last frame before leaving ----
  if constexpr (kGroups == 2) {
    // Queue empty: wait until the other group either asks for help with its last frame or is idle too.
    // (help_for is written before idle[] by the same wave, and LDS operations of a wave stay in order:
    // once idle[other] reads 1, help_for is final.)
    if (gwave == 0 && lane == 0) {
      lds_store(&ctl.idle[group], 1);
      int dec;
      for (;;) {
        if (lds_load(&ctl.help_for) == group + 1) { dec = 1; break; }
        if (lds_load(&ctl.idle[group ^ 1])) { dec = lds_load(&ctl.help_for) == group + 1; break; }
        __builtin_amdgcn_s_sleep(8);
      }
      ctl.hdr[group].pad = dec;
    }
    gsync();
    if (__builtin_amdgcn_readfirstlane(ctl.hdr[group].pad)) {
      const HelpReq hq = ctl.help;
      // pointers that came through LDS are generic: say that they are global, or every access through
      // them is a FLAT instruction (counted in lgkmcnt as well as vmcnt)
      const GlobalOut hout = (GlobalOut)hq.out;
      const GlobalSrc hsrc = (GlobalSrc)hq.src;
      const Tabs tb = make_tabs(lds.pg[group ^ 1]);  // the owner's tables
      PixMapK pm;
      pm.out = DBG && a.pixmap ? (GlobalPix)(a.pixmap + (int64_t)hq.frame * R * R * R) : (GlobalPix) nullptr;
      pm.bw = hq.pm_bw;
      pm.dc = hq.pm_dc;
      pm.dr = hq.pm_dr;
      auto run2 = [&](auto src) {
        if constexpr (AUG) {
          phase2_aug<LAYOUT, 2 * kGW>(hq.g, cam, hq.vk, R, in_xforms + 24 * (int64_t)hq.frame, tb, src, hout,
                                      kGW + gtid, 0, R);
        } else {
          phase2<LAYOUT, 2 * kGW, DBG>(hq.g, cam, hq.vk, R, tb, hq.use_tab != 0, src, hout, kGW + gtid, 0, R, pm);
        }
      };
      if (hq.mode == kFillRect) {
        run2(LdsRect{(LdsSrc)lds.pool});
      } else {
        run2(hsrc);
      }
    }
  }
}

// Split kernel for small batches (n <= CUs/2): a.split workgroups per frame.  Every workgroup streams the
// whole frame with its 16 waves (the frame comes from L2 / Infinity Cache for all but the first), captures
// the spans, places the grid, fills the tables — all redundantly, so no workgroup ever waits for another —
// and voxelizes a.per slices of the slow axis.  Results are bit-identical to the fused kernel's: the
// extents are min/max reductions (order-free) and the per-voxel code is the same.
//
// XCHG: the row stream itself is split as well.  Streaming a whole frame through ONE workgroup is a chain of
// dependent cold misses (14.8 of the 17 us such a launch took), so here workgroup p of a frame streams only band p
// of its rows, publishes its 10 partial extents in a mailbox in device memory — tagged with a number unique to the
// launch on its stream — and collects the other bands' (min/max: order-free, so the result is bit-identical).
// The wait is BOUNDED: a workgroup that does not see all mailboxes in time (its siblings are not resident yet,
// e.g. behind another kernel) streams the whole frame itself, exactly like the non-XCHG form — nothing can
// deadlock.  The valid-pixel rectangle then comes into LDS by LDS-DMA (its rows were just read by the siblings:
// L2 hits).  The mailboxes are a per-stream slice of a device global owned by the library (host: xchg_for());
// launches that cannot have one (stream capture, too many streams) use the redundant form.

template <int RT, int LAYOUT, bool AUG, bool XCHG, bool PCA>
__global__ __launch_bounds__(kWG) void tsdf_split_kernel(const KArgs a, const float *__restrict__ in_depth,
                                                         const int64_t *__restrict__ in_offsets,
                                                         const int32_t *__restrict__ in_headers,
                                                         const double *__restrict__ in_xforms) {
  using L = Lds<RT, AUG>;
  __shared__ typename L::Block lds;

  const int R = RT ? RT : a.R;
  const CamK &cam = a.cam;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frame = blockIdx.x / a.split, part = blockIdx.x - frame * a.split;
  auto &pg = lds.pg[0];
  GroupCtl &ctl = lds.ctl;
  if (tid == 0) ctl.cap_fail[0] = 0;
  FrameHdr fh;
  {
    fh.frame = frame;
    fh.pad = 0;
    fetch_header(a, in_offsets, in_headers, frame, fh);  // uniform: scalar loads
  }
  __syncthreads();
  TSDF_STAMP(0, 0);
  Frame f;
  const bool hdr_ok = frame_from_header(fh, in_depth, a.depth_len, f);
  float *out = a.tsdf ? a.tsdf + (int64_t)frame * 3 * R * R * R : nullptr;
  const bool want_vol = !a.aabb_only && out;

  int status = TSDF_FRAME_OK;
  Aabb ab;
  ab.any = false;
  ab.mn[0] = ab.mn[1] = ab.mn[2] = ab.mx[0] = ab.mx[1] = ab.mx[2] = 0.f;
  ab.c0 = ab.r0 = 0;
  ab.c1 = ab.r1 = -1;
  Grid g;
  g.mid[0] = g.mid[1] = g.mid[2] = 0.f;
  g.max_l = g.voxel_len = g.trunc = 0.f;
  g.ori[0] = g.ori[1] = g.ori[2] = 0.f;
  const double *xf = AUG ? in_xforms + 24 * (int64_t)frame : nullptr;

  Capture cap;
  cap.pool = (LdsF)lds.pool;
  cap.rowtab = (LdsU)pg.rowtab;
  cap.fail = (LdsI)&ctl.cap_fail[0];
  cap.cap4 = L::kPoolUnits / (kWG / 64);
  cap.base4 = wave * cap.cap4;
  cap.on = false;
  if (!hdr_ok) {
    status = TSDF_FRAME_BAD_HEADER;
  } else {
    float fin[kExt];
    auto sync_all = [&]() { __syncthreads(); };
    bool have = false;  // workgroup-uniform: fin holds the frame's extents
    // (Small crops streamed whole by every workgroup of the frame, skipping the exchange, were tried in round 3: a
    // 16-crop launch takes 13.5 us back to back either way, a 1-crop launch 11.4 instead of 11.9.)
    if constexpr (XCHG) {
      // ---- band `part` of the rows -> partial extents -> mailbox ----
      const int S = a.split;
      const int rb = (int)((int64_t)f.bh * part / S), re = (int)((int64_t)f.bh * (part + 1) / S);
      phase1_extents<kWG / 64, AUG, false>(f, cam, rb, re, pg.red, fin, wave, sync_all, cap, 0, xf);
      float *boxes = a.xchg + (int64_t)frame * (kXchgParts * kXchgBox);
      // Every word goes out as an agent-scope atomic (written through to where the other XCDs' workgroups read it),
      // the tag after the data has been acknowledged: a release without writing the whole L2 back.
      if (tid == 0) {
        unsigned int *box = reinterpret_cast<unsigned int *>(boxes + part * kXchgBox);
#pragma unroll
        for (int i = 0; i < kExt; ++i)
          __hip_atomic_store(box + i, __float_as_uint(fin[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(box + kExt, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      TSDF_STAMP(0, 13);
      // ---- collect the siblings' (wave 0: lane q watches mailbox q), bounded ----
      if (wave == 0) {
        const int lane = tid & 63;
        const bool mine = lane < S;
        const unsigned int *box = reinterpret_cast<const unsigned int *>(boxes + (mine ? lane : 0) * kXchgBox);
        bool ready = !mine || lane == part;
        for (int it = 0; it < a.polls; ++it) {
          if (!ready) ready = __hip_atomic_load(box + kExt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.seq;
          if (__all(ready)) break;
          __builtin_amdgcn_s_sleep(1);
        }
        const bool all = __all(ready);
        if (all) {
          // the tag was written after its data was acknowledged, and these loads bypass this XCD's L2 as well
          const bool use = mine && lane != part;
#pragma unroll
          for (int i = 0; i < 5; ++i) {
            const float v = __uint_as_float(__hip_atomic_load(box + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            fin[i] = vmin(fin[i], row0_min(use ? v : TSDF_INF));
          }
#pragma unroll
          for (int i = 5; i < 10; ++i) {
            const float v = __uint_as_float(__hip_atomic_load(box + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            fin[i] = vmax(fin[i], row0_max(use ? v : -TSDF_INF));
          }
          if (lane == 0) {  // (the row table is free in this form; `red` may still be read by a slow wave)
#pragma unroll
            for (int i = 0; i < kExt; ++i) pg.rowtab[i] = __float_as_uint(fin[i]);
          }
        }
        if (lane == 0) ctl.cap_fail[1] = all ? 1 : 0;   // (a free word of the control block)
      }
      __syncthreads();
      have = lds_load(&ctl.cap_fail[1]) != 0;
      have = __builtin_amdgcn_readfirstlane(have);
      if (have) {
#pragma unroll
        for (int i = 0; i < kExt; ++i) fin[i] = __uint_as_float(pg.rowtab[i]);
      }
    }
    TSDF_STAMP(0, 12);
    if (!have) {
      // the redundant form: this workgroup streams the whole frame (and captures the valid row windows)
      cap.on = !XCHG && want_vol && f.bw <= kMaxCapW && f.bh <= kMaxRows;
      phase1_extents<kWG / 64, AUG, !XCHG>(f, cam, 0, f.bh, pg.red, fin, wave, sync_all, cap, 0, xf);
    }
    ab = aabb_from_extents(fin);
    place_grid(ab, R, cam, a.grid_in, frame, g, status);
  }
  TSDF_STAMP(0, 4);
  if (part == 0) {
    if (tid == 0) write_frame_outputs(a, frame, g, ab, status);
    write_labels<PCA>(a, frame, fh.src, g, status, xf, tid, kWG);
  }
  if (!want_vol) return;
  if (status != TSDF_FRAME_OK) {
    zero_volume(out, R, tid, kWG, part, a.split);
    return;
  }
  bool captured = cap.on && lds_load(&ctl.cap_fail[0]) == 0;
  captured = __builtin_amdgcn_readfirstlane(captured);
  int mode = captured ? kFillSpans : kFillGlobal;
  const int sw = ab.c1 - ab.c0 + 1, sh = ab.r1 - ab.r0 + 1, sw4 = (sw + 3) & ~3;
  const bool staged = XCHG && (int64_t)sw4 * sh <= L::kPoolFloats;
  if (staged) {
    mode = kFillRect;
    stage_rect_dma<kWG / 64>(lds.pool, f, fh.off1 - fh.off0, ab.c0, ab.r0, sh, sw4, wave, tid & 63);
  }
  const VoxK vk = make_voxk(cam, g, f, ab, mode, false, sw4);
  const bool use_tab = !AUG && R <= kTabR;
  fill_tables<LAYOUT, AUG>(pg, g, cam, vk, R, use_tab, mode == kFillSpans, xf, tid, kWG);
  if (staged) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // LDS-DMA completion is counted in vmcnt
  __syncthreads();
  TSDF_STAMP(0, 6);
  const Tabs tb = make_tabs(pg);
  const int sb = part * a.per, se = sb + a.per < R ? sb + a.per : R;
  PixMapK pm;
  pm.out = (GlobalPix) nullptr;
  pm.bw = f.bw;
  pm.dc = pm.dr = 0;
  auto run2 = [&](auto src) {
    if constexpr (AUG) {
      phase2_aug<LAYOUT, kWG>(g, cam, vk, R, xf, tb, src, (GlobalOut)out, tid, sb, se);
    } else {
      phase2<LAYOUT, kWG, false>(g, cam, vk, R, tb, use_tab, src, (GlobalOut)out, tid, sb, se, pm);
    }
  };
  if (mode == kFillRect) {
    run2(LdsRect{(LdsSrc)lds.pool});
  } else if (mode == kFillSpans) {
    run2((LdsSrc)lds.pool);
  } else {
    run2((GlobalSrc)(f.depth + vk.base));
  }
  TSDF_STAMP(0, 9);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  TSDF_STAMP(0, 11);
}

// Label normalisation on its own (pre/joint_nor.py:8-18) and its inverse (3D_CNN/train.py:263-266).
__global__ void tsdf_normalize_kernel(const float *__restrict__ gt, const float *__restrict__ max_l,
                                      const float *__restrict__ mid_p, int64_t total, int nc, int clamp, int inverse,
                                      float *__restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int64_t frame = e / nc;
  const int c = (int)(e - frame * nc) % 3;
  const float ml = max_l[frame], m = mid_p[3 * frame + c], v = gt[e];
  float o;
  if (inverse) {
    o = ml > 0.f ? __fadd_rn(__fmul_rn(__fsub_rn(v, 0.5f), ml), m) : m;
  } else if (ml > 0.f) {
    o = __fadd_rn(__fdiv_rn(__fsub_rn(v, m), ml), 0.5f);
    if (clamp) {
      o = o < 0.f ? 0.f : o;
      o = o > 1.f ? 1.f : o;
    }
  } else {
    o = 0.5f;
  }
  out[e] = o;
}



// Joint PCA projection from labels already on the device (tsdf_project_joints_hip): one wave per (frame, 64 components),
// the arithmetic of the fused form (pca_project); a frame with max_l == 0 is "not OK" (its labels are 0.5, include/tsdf.h).
__global__ void __launch_bounds__(64) tsdf_project_kernel(const float *__restrict__ gt, const float *__restrict__ max_l,
                                                          const float *__restrict__ mid_p, int nc,
                                                          const float *__restrict__ mean, const float *__restrict__ W,
                                                          int K, int kchunks, float *__restrict__ out) {
  const int64_t frame = blockIdx.x / kchunks;
  const int chunk = (int)(blockIdx.x - frame * kchunks);
  const float ml = max_l[frame];
  const float mid[3] = {mid_p[3 * frame], mid_p[3 * frame + 1], mid_p[3 * frame + 2]};
  pca_project(gt + frame * nc, nullptr, mid, ml, ml > 0.f, mean, W, nc, K, out + frame * K, 64 * chunk + threadIdx.x,
              64 * kchunks);
}

// Pose error (tsdf_pose_error_hip, include/tsdf.h item 4): one wave per frame, lane <-> joint (J <= 170: three rounds);
// lane 0 then reduces the frame's errors from LDS in ascending joint order.  No atomics: deterministic.
constexpr int kPoseWaves = 4;
struct PoseArgs {
  const float *pred, *mean, *W, *max_l, *mid_p, *gt;
  float *err, *fmean, *fmax, *joints;
  int64_t n;
  int nj, K;  // K == 0: pred holds normalised coordinates
};

__global__ void __launch_bounds__(64 * kPoseWaves) tsdf_pose_error_kernel(PoseArgs a) {
  __shared__ float s_err[kPoseWaves][170];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t frame = (int64_t)blockIdx.x * kPoseWaves + wave;
  const bool live = frame < a.n;
  const int nc = 3 * a.nj;
  // (frames past n run the loops on clamped indices and store nothing: the lanes of a wave stay together for v_readlane)
  const int64_t fr = live ? frame : a.n - 1;
  const float ml = a.max_l[fr];
  for (int j0 = 0; j0 < a.nj; j0 += 64) {
    const int j = j0 + lane;
    const bool act = live && j < a.nj;
    const int jr = j < a.nj ? j : a.nj - 1;
    float uh[3];
    if (a.K) {
      const float *p = a.pred + fr * a.K;
      double acc[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = (double)a.mean[3 * jr + c];
      for (int k0 = 0; k0 < a.K; k0 += 64) {
        const float pk = k0 + lane < a.K ? p[k0 + lane] : 0.f;
        const int cnt = a.K - k0 < 64 ? a.K - k0 : 64;
        const float *w = a.W + (int64_t)(3 * jr) * nc + k0;
        // 8 components' coefficients are loaded before the adds that use them, by unconditional loads of clamped (valid)
        // addresses (a guarded load becomes a branch with its own vmcnt(0) wait); fixed trip counts around the
        // convergent v_readlane; past cnt the term is +0 * +0 (value unchanged)
        for (int i0 = 0; i0 < 64; i0 += 8) {
          float wv[3][8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int i = i0 + q < cnt ? i0 + q : cnt - 1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const float v = w[(int64_t)c * nc + i];
              wv[c][q] = i0 + q < cnt ? v : 0.f;
            }
          }
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const double pv = (double)__uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(pk), i0 + q));
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = __dadd_rn(acc[c], __dmul_rn(pv, (double)wv[c][q]));
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) uh[c] = (float)acc[c];
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) uh[c] = a.pred[fr * nc + 3 * jr + c];
    }
    float d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int jc = 3 * jr + c;
      const float m = a.mid_p[3 * fr + c];
      const float x = ml > 0.f ? __fadd_rn(__fmul_rn(__fsub_rn(uh[c], 0.5f), ml), m) : m;
      if (act && a.joints) a.joints[fr * nc + jc] = x;
      d[c] = __fsub_rn(x, a.gt[fr * nc + jc]);
    }
    // __builtin_sqrtf: correctly rounded under this build's flags (__fsqrt_rn is the native approximation here)
    const float e = __builtin_sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])),
                                              __fmul_rn(d[2], d[2])));
    if (act) {
      a.err[fr * a.nj + j] = e;
      s_err[wave][j] = e;
    }
  }
  __syncthreads();
  if (live && lane == 0) {
    double s = 0.0;
    float mx = s_err[wave][0];
    for (int j = 0; j < a.nj; ++j) {
      const float e = s_err[wave][j];
      s = __dadd_rn(s, (double)e);
      mx = e > mx || e != e ? e : mx;   // (a NaN error is the frame's max, whichever joint has it)
    }
    a.fmean[frame] = (float)(s / (double)a.nj);
    a.fmax[frame] = mx;
  }
}
