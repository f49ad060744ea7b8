// patch_host.inc — the host side of libtsdf_patch.so that needs no device: the plan and the argument rules of its four
// launching entries.  Plain C++: tsdf_patch.hip includes it (inside its anonymous namespace, after include/tsdf_patch.h),
// and patch_host_main.cc includes it into a stand-alone program built under the CPU sanitizers (make patch-host-asan;
// tests/test_patch_cpu.py runs it).
//   patch_plan           pixels per lane, rows per workgroup, items per position
//   patch_groups         the workgroups of a launch: the items, at most kPatchMaxGroups (the rest by the grid-stride loop)
//   patch_frames_defect  the first argument rule tsdf_patch_frames_hip's arguments break, in the header's order
//   patch_crops_defect   the same for tsdf_patch_crops_hip
//   patch_label_defect   the same for tsdf_patch_uvd_hip and tsdf_patch_joints_hip
// misaligned (device.inc), bad_dtype (narrow.inc) and cam_ok (prim.inc) must be declared before this file is included —
// the library has them from those files, the stand-alone program carries the text of the first two and takes cam_ok from
// prim.inc's host-only half.

constexpr int kPatchWG = 256;               // threads per workgroup
constexpr int kPatchMaxGroups = 4096;       // workgroups of one launch; the items beyond are walked by the grid-stride loop
constexpr int64_t kPatchMaxJointItems = (int64_t)1 << 31;   // n * J of a label launch stays below this
static_assert(TSDF_PATCH_MIN_SIZE % 8 == 0 && TSDF_PATCH_MAX_SIZE % 8 == 0 && TSDF_PATCH_MAX_SIZE / 4 <= kPatchWG,
              "a row of the largest float32 patch fits one workgroup");

constexpr bool patch_bad_size(int S) { return S < TSDF_PATCH_MIN_SIZE || S > TSDF_PATCH_MAX_SIZE || S % 8 != 0; }
inline bool patch_bad_elem(int dtype) { return dtype != TSDF_PATCH_F32 && bad_dtype(dtype); }
// bytes of a patch element; dtype is 0, 1 or 2
constexpr int patch_elem(int dtype) { return dtype == TSDF_PATCH_F32 ? 4 : 2; }

struct PatchPlan {
  int px, lanes_per_row, rows, items;   // pixels per lane; lanes a row takes; rows per workgroup; items per position
};

// S a multiple of 8 in 8..512, dtype 0, 1 or 2
constexpr PatchPlan patch_plan(int S, int dtype) {
  const int px = 16 / patch_elem(dtype);
  const int lpr = S / px;                                  // 1..128
  const int rows = kPatchWG / lpr < S ? kPatchWG / lpr : S;
  return {px, lpr, rows, (S + rows - 1) / rows};
}

// n >= 1
constexpr unsigned patch_groups(int n, const PatchPlan &p) {
  const int64_t items = (int64_t)n * p.items;
  return (unsigned)(items < kPatchMaxGroups ? items : kPatchMaxGroups);
}

// The rules in the order they are judged; an entry returns TSDF_OK for kPatchNoop, TSDF_ERR_INVALID_ARG for any other
// value but kPatchGood.
enum PatchDefect {
  kPatchGood = 0,
  kPatchBadN,        // n < 0
  kPatchBadSize,     // S not a multiple of 8 in 8..512
  kPatchBadInterp,
  kPatchBadDtype,
  kPatchBadJ,        // J outside 1..TSDF_PATCH_MAX_JOINTS (the label entries)
  kPatchBadFrames,   // frame_type, shift, H, W (entry 3); depth_len < 0 (entry 4)
  kPatchBadSrc,      // n_src < 0
  kPatchBadCube,     // no d_cube and a scalar that is not finite and > 0
  kPatchBadCam,
  kPatchNoop,        // n == 0: nothing to do, whatever else is passed
  kPatchNoSource,    // n_src < 1, or no index and n_src != n
  kPatchNull,        // a required pointer is NULL
  kPatchUnaligned,
  kPatchTooMany      // n * J >= 2^31 (the label entries)
};

// what the four entries share
struct PatchCommon {
  const double *com;
  float cube;
  const float *cube_n;
  const double *affine;
  const int32_t *status_in;
  int n;
  double focal, cx, cy;
  float eps, trunc_vox;
};

// what the two patch entries share beyond that
struct PatchOut {
  int S, interp, dtype;
  const void *patch;
  const int32_t *status;
};

inline bool patch_bad_cube(const PatchCommon &c) {
  return !c.cube_n && (!(c.cube > 0.0f) || !(c.cube < __builtin_inff()));   // a NaN fails the first test
}

inline bool patch_bad_cam(const PatchCommon &c) {
  const tsdf_cam cam = {c.focal, c.cx, c.cy, c.eps, c.trunc_vox};   // by value in the ABI, one rule all the same
  return !cam_ok(&cam);
}

inline PatchDefect patch_shape_defect(const PatchCommon &c, const PatchOut &o) {
  if (c.n < 0) return kPatchBadN;
  if (patch_bad_size(o.S)) return kPatchBadSize;
  if (o.interp != TSDF_PATCH_NEAREST && o.interp != TSDF_PATCH_BILINEAR) return kPatchBadInterp;
  if (patch_bad_elem(o.dtype)) return kPatchBadDtype;
  return kPatchGood;
}

// the optional pointers and the two outputs of a patch entry
inline bool patch_unaligned(const PatchCommon &c, const int64_t *index, const PatchOut &o) {
  return misaligned(c.com, 7) || misaligned(c.affine, 7) || misaligned(index, 7) || misaligned(c.cube_n, 3) ||
         misaligned(c.status_in, 3) || misaligned(o.status, 3) || misaligned(o.patch, 15);
}

inline PatchDefect patch_frames_defect(const PatchCommon &c, const PatchOut &o, const void *frames, int frame_type, int shift,
                                       int64_t n_src, int H, int W, const int64_t *index) {
  const PatchDefect shape = patch_shape_defect(c, o);
  if (shape != kPatchGood) return shape;
  const bool u16 = frame_type == TSDF_LOCATE_U16;
  if (!u16 && frame_type != TSDF_LOCATE_F32) return kPatchBadFrames;
  if (u16 && (shift < 0 || shift > 7)) return kPatchBadFrames;
  if (H <= 0 || W <= 0) return kPatchBadFrames;
  if (n_src < 0) return kPatchBadSrc;
  if (patch_bad_cube(c)) return kPatchBadCube;
  if (patch_bad_cam(c)) return kPatchBadCam;
  if (c.n == 0) return kPatchNoop;
  if (n_src < 1 || (!index && n_src != c.n)) return kPatchNoSource;
  if (!frames || !c.com || !o.patch || !o.status) return kPatchNull;
  if (misaligned(frames, u16 ? 1 : 3) || patch_unaligned(c, index, o)) return kPatchUnaligned;
  return kPatchGood;
}

inline PatchDefect patch_crops_defect(const PatchCommon &c, const PatchOut &o, const float *depth, int64_t depth_len,
                                      const int64_t *offsets, const int32_t *headers, int64_t n_src, const int64_t *index) {
  const PatchDefect shape = patch_shape_defect(c, o);
  if (shape != kPatchGood) return shape;
  if (depth_len < 0) return kPatchBadFrames;
  if (n_src < 0) return kPatchBadSrc;
  if (patch_bad_cube(c)) return kPatchBadCube;
  if (patch_bad_cam(c)) return kPatchBadCam;
  if (c.n == 0) return kPatchNoop;
  if (n_src < 1 || (!index && n_src != c.n)) return kPatchNoSource;
  if (!depth || !offsets || !headers || !c.com || !o.patch || !o.status) return kPatchNull;
  if (misaligned(depth, 3) || misaligned(headers, 3) || misaligned(offsets, 7) || patch_unaligned(c, index, o))
    return kPatchUnaligned;
  return kPatchGood;
}

// in / out: the entry's required float32 pointers; i4a / i4b: its int32 outputs (tsdf_patch_joints_hip has none: pass `out`)
inline PatchDefect patch_label_defect(const PatchCommon &c, int J, const float *in, const float *out, const void *i4a,
                                      const void *i4b) {
  if (c.n < 0) return kPatchBadN;
  if (J < 1 || J > TSDF_PATCH_MAX_JOINTS) return kPatchBadJ;
  if (patch_bad_cube(c)) return kPatchBadCube;
  if (patch_bad_cam(c)) return kPatchBadCam;
  if (c.n == 0) return kPatchNoop;
  if (!in || !c.com || !out || !i4a || !i4b) return kPatchNull;
  if (misaligned(c.com, 7) || misaligned(c.affine, 7) || misaligned(c.cube_n, 3) || misaligned(c.status_in, 3) ||
      misaligned(in, 3) || misaligned(out, 3) || misaligned(i4a, 3) || misaligned(i4b, 3))
    return kPatchUnaligned;
  if ((int64_t)c.n * J >= kPatchMaxJointItems) return kPatchTooMany;
  return kPatchGood;
}

inline int patch_status(PatchDefect d) { return d == kPatchGood || d == kPatchNoop ? TSDF_OK : TSDF_ERR_INVALID_ARG; }
