// launch.inc — part of the one translation unit tsdf_hip.hip (included there, inside its anonymous namespace).
// Host side of a call: the one argument check (tsdf_host.inc), device check (device.inc), split plan, choice of
// instantiation, argument marshalling.

// CU count of the current device (cached per device id; a racing first call computes the same value)
int num_cus() {
  static std::atomic<int> cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int v = cached[dev].load(std::memory_order_relaxed);
  if (v == 0) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    cached[dev].store(v, std::memory_order_relaxed);
  }
  return v;
}

// Workgroups per frame and slices per workgroup for the split kernel (0: use the fused kernel).
void split_plan(int n, int R, int cus, int *split, int *per) {
  *split = 0;
  *per = R;
  // (beyond CUs/2 the fused kernel measured faster: 256 full frames 38 us fused, 46 us split — round 2)
  if (n > cus / 2 || n > kXchgFrames) return;
  const int G = R * (R / 4);
  const int sstep = (G <= kWG && kWG % G == 0) ? kWG / G : 1;  // slices one pass of the workgroup covers
  const int rounds = (R + sstep - 1) / sstep;
  int S = cus / n;
  if (S < 2) S = 2;
  if (S > rounds) S = rounds;
  if (S > kXchgParts) S = kXchgParts;
  if (S < 2) return;
  const int p = ((rounds + S - 1) / S) * sstep;  // slices per workgroup
  S = (R + p - 1) / p;
  if (S < 2) return;
  *split = S;
  *per = p;
}

// Bound of the exchange form's wait for its siblings' mailboxes.  The debug build (TSDF_DEBUG_HOOKS) reads
// TSDF_XCHG_POLLS from the environment so that a test can force every workgroup onto the fallback (0); the product
// reads no environment variable.
int xchg_polls() {
#ifdef TSDF_DEBUG_HOOKS
  static const int polls = [] {
    const char *e = getenv("TSDF_XCHG_POLLS");
    return e ? atoi(e) : kXchgPolls;
  }();
  return polls;
#else
  return kXchgPolls;
#endif
}

template <int RT, int LAYOUT, bool AUG, bool DBG, bool PCA = false>
hipError_t launch(hipStream_t s, KArgs &a, int dev) {
  const int cus = num_cus();
  if constexpr (!DBG) {
    int S = 0, per = a.R;
    if (!a.aabb_only && a.tsdf) split_plan(a.n, a.R, cus, &S, &per);
    if (S >= 2) {
      a.split = S;
      a.per = per;
      a.queue = nullptr;
      a.xchg = a.n <= kXchgFrames ? xchg_for(dev, s, &a.seq) : nullptr;
      a.polls = xchg_polls();
      if (a.xchg) {
        hipLaunchKernelGGL((tsdf_split_kernel<RT, LAYOUT, AUG, true, PCA>), dim3(a.n * S), dim3(kWG), 0, s, a, a.depth,
                           a.offsets, a.headers, a.xforms);
      } else {
        hipLaunchKernelGGL((tsdf_split_kernel<RT, LAYOUT, AUG, false, PCA>), dim3(a.n * S), dim3(kWG), 0, s, a, a.depth,
                           a.offsets, a.headers, a.xforms);
      }
      return hipGetLastError();
    }
  }
  // persistent: one workgroup per CU; with fewer frames per CU than groups the later groups idle or help
  const int grid = a.n < cus ? a.n : cus;
  a.split = 0;
  a.per = a.R;
  auto fused = [&](auto groups_tag) {
    constexpr int G = decltype(groups_tag)::value;
    a.queue = a.n > grid * G ? queue_word(dev, s, &a.qepoch) : nullptr;  // no dynamic frames: no word needed
    hipLaunchKernelGGL((tsdf_fused_kernel<RT, LAYOUT, AUG, DBG, G, PCA>), dim3(grid), dim3(kWG), 0, s, a, a.depth, a.offsets,
                       a.headers, a.xforms);
  };
  if constexpr (RT != 0) {
    fused(std::integral_constant<int, groups_for(RT)>{});
  } else {   // any other resolution: the instantiation is generic in R, the group count follows the resolution
    if (groups_for(a.R) == 1) fused(std::integral_constant<int, 1>{});
    else fused(std::integral_constant<int, 2>{});
  }
  return hipGetLastError();
}

// The resolutions of the BASELINE configs get instantiations of their own (R a compile-time constant), every other
// one the generic instantiation.
template <int LAYOUT, bool AUG, bool PCA = false>
hipError_t launch_r(hipStream_t s, KArgs &a, int dev) {
  if (a.R == 32) return launch<32, LAYOUT, AUG, false, PCA>(s, a, dev);
  if (a.R == 64) return launch<64, LAYOUT, AUG, false, PCA>(s, a, dev);
  return launch<0, LAYOUT, AUG, false, PCA>(s, a, dev);
}

using namespace tsdf_host;   // Frames, Outs, RunOpts and the kNeed* bits

int run(const Frames &f, const Outs &out, const RunOpts &o) {
  // (every argument check: tsdf_host.inc, shared with the sanitizer build of the host code)
  const int chk = check_run_args(f, out, o, tsdf_resolution_supported(f.R));
  if (chk == kNothingToDo) return TSDF_OK;
  if (chk != TSDF_OK) return chk;
  const int n = f.n, R = f.R, layout = f.layout;
  const tsdf_cam *cam = f.cam ? f.cam : &kDefaultCam;
  int dev = 0;
  int rc = check_device(&dev);
  if (rc != TSDF_OK) return rc;
  KArgs a;
  memset(&a, 0, sizeof a);
  a.depth = f.depth;
  a.offsets = f.offsets;
  a.headers = f.headers;
  a.n = n;
  a.R = R;
  a.cam.focal = cam->focal;
  a.cam.cx = cam->cx;
  a.cam.cy = cam->cy;
  a.cam.inv_focal = 1.0 / cam->focal;
  a.cam.eps = cam->invalid_eps;
  a.cam.trunc_vox = cam->trunc_voxels;
  a.tsdf = out.tsdf;
  a.max_l = out.max_l;
  a.mid_p = out.mid_p;
  a.status = out.status;
  a.aabb = o.aabb;
  a.grid = o.grid;
  a.ori = o.ori;
  a.aabb_only = o.aabb_only;
  a.grid_in = o.grid_in;
  a.xforms = o.xforms;
  a.depth_len = f.depth_len;
  a.index = o.index;
  a.n_src = o.n_src;
  if (o.needs & kNeedHostIndex) {   // (checked: h_index is there and n <= TSDF_INLINE_INDEX_MAX)
    a.n_inline = n;
    memcpy(a.inline_index, o.h_index, sizeof(int64_t) * (size_t)n);
  }
  if (o.labels) {
    a.gt = o.labels->d_gt;
    a.gt_nor = o.labels->d_out_gt_nor;
    a.gt_aug = o.labels->d_out_gt_aug;
    a.n_joints = o.labels->n_joints;
    a.clamp = o.labels->clamp;
  }
  if (o.pca) {
    a.pca_mean = o.pca->d_mean;
    a.pca_coeff = o.pca->d_coeff;
    a.gt_pca = o.pca->d_out_gt_pca;
    a.pca_k = o.pca->n_components;
  }
  a.pixmap = o.pixmap;
  hipStream_t s = static_cast<hipStream_t>(f.stream);
  hipError_t e;
  if (o.pixmap) {
#ifdef TSDF_DEBUG_HOOKS   // the diagnostic instantiations (DBG) exist in the debug build only
    if (layout == TSDF_LAYOUT_CZYX)
      e = R == 32 ? launch<32, 0, false, true>(s, a, dev) : launch<0, 0, false, true>(s, a, dev);
    else
      e = R == 32 ? launch<32, 1, false, true>(s, a, dev) : launch<0, 1, false, true>(s, a, dev);
#else
    return TSDF_ERR_INVALID_ARG;
#endif
  } else if (a.pca_k && o.xforms) {   // (the joint-PCA variants: labels + projection)
    e = layout == TSDF_LAYOUT_CZYX ? launch_r<0, true, true>(s, a, dev) : launch_r<1, true, true>(s, a, dev);
  } else if (a.pca_k) {
    e = layout == TSDF_LAYOUT_CZYX ? launch_r<0, false, true>(s, a, dev) : launch_r<1, false, true>(s, a, dev);
  } else if (o.xforms) {
    e = layout == TSDF_LAYOUT_CZYX ? launch_r<0, true>(s, a, dev) : launch_r<1, true>(s, a, dev);
  } else {
    e = layout == TSDF_LAYOUT_CZYX ? launch_r<0, false>(s, a, dev) : launch_r<1, false>(s, a, dev);
  }
  return e == hipSuccess ? TSDF_OK : TSDF_ERR_LAUNCH;
}

int run_normalize(const float *d_in, const float *d_max_l, const float *d_mid_p, int n, int n_joints, int clamp,
                  int inverse, void *hip_stream, float *d_out) {
  if (n < 0 || n_joints < 1 || n_joints > 170) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_in || !d_max_l || !d_mid_p || !d_out) return TSDF_ERR_INVALID_ARG;
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  const int nc = 3 * n_joints;
  const int64_t total = (int64_t)n * nc;
  const int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return TSDF_ERR_INVALID_ARG;
  hipLaunchKernelGGL(tsdf_normalize_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream),
                     d_in, d_max_l, d_mid_p, total, nc, clamp, inverse, d_out);
  return launched();
}


// tsdf_project_joints_hip: one wave per (frame, 64 components).
int run_project(const float *d_gt, const float *d_max_l, const float *d_mid_p, int n, int n_joints, const tsdf_pca *pca,
                void *hip_stream) {
  if (n < 0 || tsdf_host::check_pca(pca, n, n_joints, true) != TSDF_OK) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_gt || !d_max_l || !d_mid_p) return TSDF_ERR_INVALID_ARG;
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  const int K = pca->n_components, kchunks = (K + 63) / 64;
  const int64_t blocks = (int64_t)n * kchunks;
  if (blocks > 0x7fffffff) return TSDF_ERR_INVALID_ARG;
  hipLaunchKernelGGL(tsdf_project_kernel, dim3((unsigned)blocks), dim3(64), 0, static_cast<hipStream_t>(hip_stream), d_gt,
                     d_max_l, d_mid_p, 3 * n_joints, pca->d_mean, pca->d_coeff, K, kchunks, pca->d_out_gt_pca);
  return launched();
}

// tsdf_pose_error_hip: one wave per frame.
int run_pose_error(const float *d_pred, const tsdf_pca *pca, const float *d_max_l, const float *d_mid_p, const float *d_gt,
                   int n, int n_joints, void *hip_stream, float *d_err, float *d_fmean, float *d_fmax, float *d_joints) {
  if (n < 0 || n_joints < 1 || n_joints > 170) return TSDF_ERR_INVALID_ARG;
  if (pca && tsdf_host::check_pca(pca, n, n_joints, false) != TSDF_OK) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_pred || !d_max_l || !d_mid_p || !d_gt || !d_err || !d_fmean || !d_fmax) return TSDF_ERR_INVALID_ARG;
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  PoseArgs a;
  a.pred = d_pred;
  a.mean = pca ? pca->d_mean : nullptr;
  a.W = pca ? pca->d_coeff : nullptr;
  a.K = pca ? pca->n_components : 0;
  a.max_l = d_max_l;
  a.mid_p = d_mid_p;
  a.gt = d_gt;
  a.err = d_err;
  a.fmean = d_fmean;
  a.fmax = d_fmax;
  a.joints = d_joints;
  a.n = n;
  a.nj = n_joints;
  const int blocks = (n + kPoseWaves - 1) / kPoseWaves;
  hipLaunchKernelGGL(tsdf_pose_error_kernel, dim3((unsigned)blocks), dim3(64 * kPoseWaves), 0,
                     static_cast<hipStream_t>(hip_stream), a);
  return launched();
}
