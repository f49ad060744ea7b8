// abi.inc — the C ABI of include/tsdf.h (included by tsdf_hip.hip after its anonymous namespace).

// Every voxelizer entry describes its call (Frames, Outs, RunOpts with the bits of what it needs) and returns run():
// all argument checks are tsdf_host::check_run_args, called there.

extern "C" {

void tsdf_default_cam(tsdf_cam *cam) {
  if (cam) *cam = kDefaultCam;
}

int tsdf_version(void) { return TSDF_ABI_VERSION; }

const char *tsdf_strerror(int status) {
  switch (status) {
    case TSDF_OK: return "ok";
    case TSDF_ERR_INVALID_ARG: return "invalid argument";
    case TSDF_ERR_NO_DEVICE: return "no usable HIP device (this library is gfx950-only and has no CPU fallback)";
    case TSDF_ERR_LAUNCH: return "HIP kernel launch failed";
    default: return "unknown tsdf status";
  }
}

int tsdf_resolution_supported(int R) { return R >= 4 && R <= kMaxR && (R % 4) == 0; }

int tsdf_voxelize_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers, int n,
                      int R, const tsdf_cam *cam, int layout, void *hip_stream, float *d_out_tsdf,
                      float *d_out_max_l, float *d_out_mid_p, int32_t *d_out_status) {
  RunOpts o;
  o.needs = kNeedPlacement;
  return run(Frames{d_depth, depth_len, d_offsets, d_headers, n, R, cam, layout, hip_stream},
             Outs{d_out_tsdf, d_out_max_l, d_out_mid_p, d_out_status}, o);
}

int tsdf_voxelize_labels_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                             int n, int R, const tsdf_cam *cam, int layout, void *hip_stream, float *d_out_tsdf,
                             float *d_out_max_l, float *d_out_mid_p, int32_t *d_out_status, const tsdf_labels *labels) {
  RunOpts o;
  o.needs = kNeedPlacement | kNeedLabels;
  o.labels = labels;
  return run(Frames{d_depth, depth_len, d_offsets, d_headers, n, R, cam, layout, hip_stream},
             Outs{d_out_tsdf, d_out_max_l, d_out_mid_p, d_out_status}, o);
}

int tsdf_voxelize_indexed_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                              int64_t n_pack, const int64_t *d_index, int n, int R, const tsdf_cam *cam, int layout,
                              void *hip_stream, float *d_out_tsdf, float *d_out_max_l, float *d_out_mid_p,
                              int32_t *d_out_status, const tsdf_labels *labels) {
  RunOpts o;
  o.needs = kNeedPlacement | kNeedIndex;
  o.labels = labels;
  o.index = d_index;
  o.n_src = n_pack;
  return run(Frames{d_depth, depth_len, d_offsets, d_headers, n, R, cam, layout, hip_stream},
             Outs{d_out_tsdf, d_out_max_l, d_out_mid_p, d_out_status}, o);
}

int tsdf_voxelize_indexed_host_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets,
                                   const int32_t *d_headers, int64_t n_pack, const int64_t *h_index, int n, int R,
                                   const tsdf_cam *cam, int layout, void *hip_stream, float *d_out_tsdf, float *d_out_max_l,
                                   float *d_out_mid_p, int32_t *d_out_status, const tsdf_labels *labels) {
  RunOpts o;
  o.needs = kNeedPlacement | kNeedHostIndex;
  o.labels = labels;
  o.h_index = h_index;
  o.n_src = n_pack;
  return run(Frames{d_depth, depth_len, d_offsets, d_headers, n, R, cam, layout, hip_stream},
             Outs{d_out_tsdf, d_out_max_l, d_out_mid_p, d_out_status}, o);
}

int tsdf_voxelize_indexed_aug_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets,
                                  const int32_t *d_headers, int64_t n_pack, const int64_t *d_index, int n, int R,
                                  const tsdf_cam *cam, int layout, void *hip_stream, const double *d_xforms,
                                  float *d_out_tsdf, float *d_out_max_l, float *d_out_mid_p, int32_t *d_out_status,
                                  const tsdf_labels *labels) {
  RunOpts o;
  o.needs = kNeedPlacement | kNeedIndex | kNeedXforms;
  o.labels = labels;
  o.index = d_index;
  o.n_src = n_pack;
  o.xforms = d_xforms;
  return run(Frames{d_depth, depth_len, d_offsets, d_headers, n, R, cam, layout, hip_stream},
             Outs{d_out_tsdf, d_out_max_l, d_out_mid_p, d_out_status}, o);
}

int tsdf_voxelize_grid_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers, int n,
                           int R, const tsdf_cam *cam, int layout, void *hip_stream, const float *d_grid,
                           float *d_out_tsdf, int32_t *d_out_status) {
  RunOpts o;
  o.needs = kNeedGridIn;
  o.grid_in = d_grid;
  return run(Frames{d_depth, depth_len, d_offsets, d_headers, n, R, cam, layout, hip_stream},
             Outs{d_out_tsdf, nullptr, nullptr, d_out_status}, o);
}

int tsdf_voxelize_aug_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers, int n,
                          int R, const tsdf_cam *cam, int layout, void *hip_stream, const double *d_xforms,
                          float *d_out_tsdf, float *d_out_max_l, float *d_out_mid_p, int32_t *d_out_status) {
  RunOpts o;
  o.needs = kNeedPlacement | kNeedXforms;
  o.xforms = d_xforms;
  return run(Frames{d_depth, depth_len, d_offsets, d_headers, n, R, cam, layout, hip_stream},
             Outs{d_out_tsdf, d_out_max_l, d_out_mid_p, d_out_status}, o);
}

int tsdf_voxelize_aug_labels_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets,
                                 const int32_t *d_headers, int n, int R, const tsdf_cam *cam, int layout,
                                 void *hip_stream, const double *d_xforms, float *d_out_tsdf, float *d_out_max_l,
                                 float *d_out_mid_p, int32_t *d_out_status, const tsdf_labels *labels) {
  RunOpts o;
  o.needs = kNeedPlacement | kNeedXforms | kNeedLabels;
  o.xforms = d_xforms;
  o.labels = labels;
  return run(Frames{d_depth, depth_len, d_offsets, d_headers, n, R, cam, layout, hip_stream},
             Outs{d_out_tsdf, d_out_max_l, d_out_mid_p, d_out_status}, o);
}

int tsdf_aabb_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers, int n, int R,
                  const tsdf_cam *cam, void *hip_stream, float *d_out_aabb, float *d_out_grid,
                  float *d_out_ori, int32_t *d_out_status) {
  RunOpts o;
  o.aabb = d_out_aabb;
  o.grid = d_out_grid;
  o.ori = d_out_ori;
  o.aabb_only = 1;
  return run(Frames{d_depth, depth_len, d_offsets, d_headers, n, R, cam, TSDF_LAYOUT_CZYX, hip_stream},
             Outs{nullptr, nullptr, nullptr, d_out_status}, o);
}

int tsdf_normalize_joints_hip(const float *d_gt, const float *d_max_l, const float *d_mid_p, int n, int n_joints,
                              int clamp, void *hip_stream, float *d_out_gt_nor) {
  return run_normalize(d_gt, d_max_l, d_mid_p, n, n_joints, clamp, 0, hip_stream, d_out_gt_nor);
}

int tsdf_denormalize_joints_hip(const float *d_pred, const float *d_max_l, const float *d_mid_p, int n, int n_joints,
                                void *hip_stream, float *d_out_joints) {
  return run_normalize(d_pred, d_max_l, d_mid_p, n, n_joints, 0, 1, hip_stream, d_out_joints);
}

// ---- joint PCA and pose error ----
int tsdf_voxelize_labels_pca_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets,
                                 const int32_t *d_headers, int n, int R, const tsdf_cam *cam, int layout,
                                 void *hip_stream, const double *d_xforms, float *d_out_tsdf, float *d_out_max_l,
                                 float *d_out_mid_p, int32_t *d_out_status, const tsdf_labels *labels,
                                 const tsdf_pca *pca) {
  RunOpts o;
  o.needs = kNeedPlacement | kNeedLabels | kNeedPca;   // (xforms is optional here)
  o.xforms = d_xforms;
  o.labels = labels;
  o.pca = pca;
  return run(Frames{d_depth, depth_len, d_offsets, d_headers, n, R, cam, layout, hip_stream},
             Outs{d_out_tsdf, d_out_max_l, d_out_mid_p, d_out_status}, o);
}

int tsdf_voxelize_indexed_pca_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets,
                                  const int32_t *d_headers, int64_t n_pack, const int64_t *d_index, int n, int R,
                                  const tsdf_cam *cam, int layout, void *hip_stream, const double *d_xforms,
                                  float *d_out_tsdf, float *d_out_max_l, float *d_out_mid_p, int32_t *d_out_status,
                                  const tsdf_labels *labels, const tsdf_pca *pca) {
  RunOpts o;
  o.needs = kNeedPlacement | kNeedIndex | kNeedLabels | kNeedPca;   // (xforms is optional here)
  o.labels = labels;
  o.index = d_index;
  o.n_src = n_pack;
  o.xforms = d_xforms;
  o.pca = pca;
  return run(Frames{d_depth, depth_len, d_offsets, d_headers, n, R, cam, layout, hip_stream},
             Outs{d_out_tsdf, d_out_max_l, d_out_mid_p, d_out_status}, o);
}

int tsdf_voxelize_indexed_host_pca_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets,
                                       const int32_t *d_headers, int64_t n_pack, const int64_t *h_index, int n, int R,
                                       const tsdf_cam *cam, int layout, void *hip_stream, float *d_out_tsdf,
                                       float *d_out_max_l, float *d_out_mid_p, int32_t *d_out_status,
                                       const tsdf_labels *labels, const tsdf_pca *pca) {
  RunOpts o;
  o.needs = kNeedPlacement | kNeedHostIndex | kNeedLabels | kNeedPca;
  o.labels = labels;
  o.h_index = h_index;
  o.n_src = n_pack;
  o.pca = pca;
  return run(Frames{d_depth, depth_len, d_offsets, d_headers, n, R, cam, layout, hip_stream},
             Outs{d_out_tsdf, d_out_max_l, d_out_mid_p, d_out_status}, o);
}

int tsdf_project_joints_hip(const float *d_gt, const float *d_max_l, const float *d_mid_p, int n, int n_joints,
                            const tsdf_pca *pca, void *hip_stream) {
  return run_project(d_gt, d_max_l, d_mid_p, n, n_joints, pca, hip_stream);
}

int tsdf_pose_error_hip(const float *d_pred, const tsdf_pca *pca, const float *d_max_l, const float *d_mid_p,
                        const float *d_gt, int n, int n_joints, void *hip_stream, float *d_out_err,
                        float *d_out_frame_mean, float *d_out_frame_max, float *d_out_joints) {
  return run_pose_error(d_pred, pca, d_max_l, d_mid_p, d_gt, n, n_joints, hip_stream, d_out_err, d_out_frame_mean,
                        d_out_frame_max, d_out_joints);
}

int tsdf_point_clouds_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                          int n, int points, const tsdf_cam *cam, uint64_t seed, int64_t frame_base,
                          const double *d_xforms, void *hip_stream, double *d_out_points, int32_t *d_out_count,
                          int32_t *d_out_status) {
  return run_point_clouds(d_depth, depth_len, d_offsets, d_headers, n, points, cam, seed, frame_base, d_xforms,
                          hip_stream, d_out_points, d_out_count, d_out_status);
}

int tsdf_cloud_grid_hip(const double *d_points, int n, int points, int R, const tsdf_cam *cam, void *hip_stream,
                        float *d_out_grid, float *d_out_max_l, float *d_out_mid_p, float *d_out_aabb,
                        int32_t *d_out_status) {
  return run_cloud_grid(d_points, n, points, R, cam, hip_stream, d_out_grid, d_out_max_l, d_out_mid_p, d_out_aabb,
                        d_out_status);
}

#ifdef TSDF_DEBUG_HOOKS   // the debug build only (make debug -> build/libtsdf_hip_debug.so): include/tsdf_debug.h
int tsdf_debug_pixmap_hip(const float *d_depth, int64_t depth_len, const int64_t *d_offsets, const int32_t *d_headers,
                          int n, int R, const tsdf_cam *cam, int layout, void *hip_stream, const float *d_grid,
                          float *d_out_tsdf, int32_t *d_out_pixmap, int32_t *d_out_status) {
  RunOpts o;
  o.needs = kNeedPixmap;   // (a NULL grid: the frame's own placement)
  o.grid_in = d_grid;
  o.pixmap = d_out_pixmap;
  return run(Frames{d_depth, depth_len, d_offsets, d_headers, n, R, cam, layout, hip_stream},
             Outs{d_out_tsdf, nullptr, nullptr, d_out_status}, o);
}
#endif

int tsdf_stream_release(void *hip_stream) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    return TSDF_OK;
  }
  (void)stream_slot(dev, static_cast<hipStream_t>(hip_stream), true);
  return TSDF_OK;
}

#ifdef TSDF_DEBUG_HOOKS
int tsdf_debug_set_queue_word(void *hip_stream, uint64_t value) {
  int dev = 0;
  const int rc = check_device(&dev);
  if (rc != TSDF_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const int i = stream_slot(dev, s, false);
  if (i < 0) return TSDF_ERR_INVALID_ARG;
  if (hipStreamSynchronize(s) != hipSuccess) return TSDF_ERR_LAUNCH;
  const unsigned long long v = value;
  if (hipMemcpy(g_slots[dev].base + i, &v, sizeof v, hipMemcpyHostToDevice) != hipSuccess) return TSDF_ERR_LAUNCH;
  return TSDF_OK;
}
#endif

int tsdf_describe_launch(int n, int R, int layout, int aug, char *buf, int buflen) {
  if (!buf || buflen < 1 || n < 1 || !tsdf_resolution_supported(R)) return TSDF_ERR_INVALID_ARG;
  if (layout != TSDF_LAYOUT_CZYX && layout != TSDF_LAYOUT_CXYZ) return TSDF_ERR_INVALID_ARG;
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  const int rt = (R == 32 || R == 64) ? R : 0;   // launch_r's choice of instantiation
  int S = 0, per = R;
  split_plan(n, R, num_cus(), &S, &per);
  if (S >= 2) {
    // (the last template argument — exchange or redundant form — depends on the stream the launch is issued on:
    // launch() decides; the string names the family)
    snprintf(buf, (size_t)buflen, "tsdf_split_kernel<%d, %d, %s, x%d", rt, layout, aug ? "true" : "false", S);
  } else {
    snprintf(buf, (size_t)buflen, "tsdf_fused_kernel<%d, %d, %s, false, %d>", rt, layout, aug ? "true" : "false",
             groups_for(R));
  }
  return TSDF_OK;
}

#ifdef TSDF_STAMPS
// Diagnostic library only: copy the stamp array to the host (synchronises the device).
int tsdf_debug_read_stamps(unsigned long long *host_out, int count) {
  const int total = kStampBlocks * kStampFrames * kStampSlots;
  if (count > total) count = total;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * count) != hipSuccess)
    return -1;
  return count;
}
int tsdf_debug_read_wstamps(unsigned long long *host_out, int count) {
  const int total = kStampBlocks * kStampFrames * 16 * 2;
  if (count > total) count = total;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_wstamps), sizeof(unsigned long long) * count) != hipSuccess)
    return -1;
  return count;
}
#endif

}  // extern "C"

