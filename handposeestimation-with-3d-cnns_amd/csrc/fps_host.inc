// fps_host.inc — the host side of libtsdf_fps.so that needs no device: the argument rules of its two entries and the
// plan.  Plain C++: tsdf_fps.hip includes it (inside its anonymous namespace, after include/tsdf_fps.h), and
// fps_host_main.cc includes it into a stand-alone program built under the CPU sanitizers (make fps-host-asan;
// tests/test_fps_cpu.py runs it).
//   fps_plan          the resident cap, the workspace bytes per position and the LDS bytes
//   fps_holds         does a position of `count` candidates hold, and in which form — the kernel's own decision
//                     (constexpr, as fps_slots and fps_segment: the kernel calls the three)
//   fps_slots         the workgroup-uniform trip count of the resident form's loop over a lane's candidates
//   fps_segment       the piece of the items each wave compacts
//   fps_defect        the first argument rule tsdf_fps_hip's arguments break, in the header's order
//   fps_points_defect the same for tsdf_fps_points_hip
// The tests that exist already are not restated: misaligned (device.inc) and cam_ok (prim.inc) must be declared before
// this file is included — the library has them from those files, the stand-alone program carries the text of the first
// and takes cam_ok from prim.inc's host-only half.

#ifndef TSDF_FPS_WG
#define TSDF_FPS_WG 1024                     // threads per workgroup: 256, 512 or 1024 (DESIGN.md has the three timings)
#endif
constexpr int kFpsWG = TSDF_FPS_WG;
constexpr int kFpsWaves = kFpsWG / 64;
constexpr int kFpsResident = 12288;          // candidates of the resident form: three float32 arrays of 48 KiB in LDS
constexpr int kFpsSlots = kFpsResident / kFpsWG;   // candidates per lane, in registers
constexpr int kFpsLdsBytes = 3 * 4 * kFpsResident + 2 * kFpsWaves * 8 + kFpsWaves * 4;   // points, keys, wave counts
constexpr int64_t kFpsMaxItems = (int64_t)1 << 32;   // work-items of one launch
constexpr int64_t kFpsMaxRank = 0x7fffffff;  // ranks are int32
static_assert(kFpsWG == 256 || kFpsWG == 512 || kFpsWG == 1024, "workgroup size");
static_assert(kFpsSlots * kFpsWG == kFpsResident && kFpsLdsBytes <= 160 * 1024, "the resident form's budget");

struct FpsPlan {
  int resident_cap, lds_bytes;
  int64_t work_bytes;   // per batch position
};

// capacity in 0..kFpsMaxRank
inline FpsPlan fps_plan(int64_t capacity) { return {kFpsResident, kFpsLdsBytes, 16 * capacity}; }

enum FpsForm { kFpsNone = 0, kFpsFormResident, kFpsFormStreaming };

// The form a position of `count` candidates runs in, kFpsNone when the call cannot hold it.  `work`: the call has a
// workspace of `capacity` candidates per position.
constexpr FpsForm fps_holds(int64_t count, bool work, int64_t capacity, int form_hint) {
  const bool streams = work && count <= capacity;
  if (form_hint == 1 && streams) return kFpsFormStreaming;
  if (count <= kFpsResident) return kFpsFormResident;
  return streams ? kFpsFormStreaming : kFpsNone;
}

// Candidate c of a resident position lives in slot c / kFpsWG of lane c % kFpsWG: every lane's loop runs over the
// slots [0, fps_slots(count)), the same for the whole workgroup.  count in 1..kFpsResident.
constexpr int fps_slots(int count) { return (count + kFpsWG - 1) / kFpsWG; }

// Wave w compacts the items [w * seg, min((w + 1) * seg, items)) in steps of 64: seg is a multiple of 64, the pieces
// are disjoint, in order, and cover every item.  items in 1..kFpsMaxRank.
constexpr int64_t fps_segment(int64_t items) {
  const int64_t per = (items + kFpsWaves - 1) / kFpsWaves;
  return (per + 63) / 64 * 64;
}

// The rules in the order they are judged; an entry returns TSDF_OK for kFpsNoop, TSDF_ERR_INVALID_ARG for any other
// value but kFpsGood.
enum FpsDefect {
  kFpsGood = 0,
  kFpsBadN,        // n < 0
  kFpsBadM,        // M outside 1..65536
  kFpsBadHint,     // form_hint not 0 or 1
  kFpsBadCap,      // capacity outside 0..2^31-1
  kFpsBadDtype,    // points entry: dtype
  kFpsBadRows,     // points entry: P outside 1..2^31-1
  kFpsNoop,        // n == 0: nothing to do, whatever else is passed
  kFpsNull,        // a required pointer is NULL
  kFpsBadLen,      // depth_len < 0
  kFpsBadSrc,      // n_src < 1, or no index and n_src != n
  kFpsBadWork,     // d_work NULL with capacity != 0, or given with capacity == 0
  kFpsUnaligned,   // d_xforms off an 8-byte boundary, d_work off a 16-byte one, d_points off its element's
  kFpsBadCam,
  kFpsTooMany      // n * kFpsWG >= 2^32
};

// what the two entries share
struct FpsOut {
  int n, M;
  int64_t capacity;
  int hint;
  const float *work;
  const float *points;
  const int32_t *pixel, *count, *status;
};

struct FpsCall {
  const float *depth;
  int64_t depth_len;
  const int64_t *offsets;
  const int32_t *headers;
  int64_t n_src;
  const int64_t *index;
  double focal, cx, cy;
  float eps, trunc_vox;
  const double *xforms;
  FpsOut o;
};

struct FpsPointsCall {
  const void *points;
  int dtype;
  int64_t P;
  FpsOut o;
};

inline FpsDefect fps_shape_defect(const FpsOut &o) {
  if (o.n < 0) return kFpsBadN;
  if (o.M < 1 || o.M > TSDF_FPS_MAX_POINTS) return kFpsBadM;
  if (o.hint != 0 && o.hint != 1) return kFpsBadHint;
  if (o.capacity < 0 || o.capacity > kFpsMaxRank) return kFpsBadCap;
  return kFpsGood;
}

inline bool fps_out_null(const FpsOut &o) { return !o.points || !o.pixel || !o.count || !o.status; }

inline bool fps_work_defect(const FpsOut &o) { return (o.work != nullptr) != (o.capacity != 0); }

inline FpsDefect fps_defect(const FpsCall &c) {
  const FpsDefect shape = fps_shape_defect(c.o);
  if (shape != kFpsGood) return shape;
  if (c.o.n == 0) return kFpsNoop;
  if (!c.depth || !c.offsets || !c.headers || fps_out_null(c.o)) return kFpsNull;
  if (c.depth_len < 0) return kFpsBadLen;
  if (c.n_src < 1 || (!c.index && c.n_src != c.o.n)) return kFpsBadSrc;
  if (fps_work_defect(c.o)) return kFpsBadWork;
  if (misaligned(c.xforms, 7) || misaligned(c.o.work, 15)) return kFpsUnaligned;
  const tsdf_cam cam = {c.focal, c.cx, c.cy, c.eps, c.trunc_vox};   // by value in the ABI, one rule all the same
  if (!cam_ok(&cam)) return kFpsBadCam;
  if ((int64_t)c.o.n * kFpsWG >= kFpsMaxItems) return kFpsTooMany;
  return kFpsGood;
}

inline FpsDefect fps_points_defect(const FpsPointsCall &c) {
  const FpsDefect shape = fps_shape_defect(c.o);
  if (shape != kFpsGood) return shape;
  if (c.dtype != TSDF_FPS_F32 && c.dtype != TSDF_FPS_F64) return kFpsBadDtype;
  if (c.P < 1 || c.P > kFpsMaxRank) return kFpsBadRows;
  if (c.o.n == 0) return kFpsNoop;
  if (!c.points || fps_out_null(c.o)) return kFpsNull;
  if (fps_work_defect(c.o)) return kFpsBadWork;
  if (misaligned(c.points, c.dtype == TSDF_FPS_F64 ? 7 : 3) || misaligned(c.o.work, 15)) return kFpsUnaligned;
  if ((int64_t)c.o.n * kFpsWG >= kFpsMaxItems) return kFpsTooMany;
  return kFpsGood;
}

inline int fps_status(FpsDefect d) { return d == kFpsGood || d == kFpsNoop ? TSDF_OK : TSDF_ERR_INVALID_ARG; }
