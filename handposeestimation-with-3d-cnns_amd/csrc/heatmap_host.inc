// heatmap_host.inc — the host side of libtsdf_heatmap.so that needs no device: the argument rules of its two entries, the
// encode launch's plan and the item arithmetic the encode kernel shares with it.  Plain C++: tsdf_heatmap.hip includes it
// (inside its anonymous namespace, after include/tsdf_heatmap.h), and heatmap_host_main.cc includes it into a stand-alone
// program built under the CPU sanitizers (make heatmap-host-asan; tests/test_heatmap_cpu.py runs it).
//   heat_defect_*   the first argument rule an entry's arguments break, in the header's order.  The three tests that exist
//                   already are not restated: bad_res and misaligned (device.inc) and bad_dtype (narrow.inc) must be
//                   declared before this file is included — the library has them from those files, the stand-alone
//                   program carries their text
//   heat_plan       slabs per (frame, joint) of the encode launch from (n * J, R, CU count)
//   heat_magic, heat_div   division of a small number by a launch constant as a multiply and a shift
#if defined(__HIPCC__)
#define TSDF_HEAT_FN __host__ __device__ inline
#else
#define TSDF_HEAT_FN inline
#endif

constexpr int kHeatMaxR = 128;
constexpr int kHeatMaxJoints = 170;          // the product's limit (include/tsdf.h: tsdf_labels)
constexpr int kHeatMaxRadius = 3;
constexpr int64_t kHeatMaxUnits = 1 << 24;   // (frame, joint) pairs: one workgroup of 256 lanes each at least

// The rules in the order they are judged; an entry returns TSDF_OK for kHeatNoop, TSDF_ERR_INVALID_ARG for any other
// value but kHeatGood.
enum HeatDefect {
  kHeatGood = 0,
  kHeatNoop,       // n == 0: nothing to do, whatever else is passed
  kHeatBadN,       // n < 0
  kHeatBadRes,     // R: device.inc::bad_res's rule (a multiple of 4 in 4..128)
  kHeatBadJoints,  // n_joints outside 1..170
  kHeatBadLayout,
  kHeatBadDtype,
  kHeatBadScalar,  // encode: sigma not finite and > 0; decode: radius outside 0..3
  kHeatNull,       // a required pointer is NULL
  kHeatUnaligned,  // a volume off a 16-byte boundary, another array off a 4-byte one
  kHeatTooMany     // n * n_joints >= 2^24
};

inline HeatDefect heat_defect_shape(int n, int n_joints, int R, int layout, int dtype) {
  if (n == 0) return kHeatNoop;
  if (n < 0) return kHeatBadN;
  if (bad_res(R)) return kHeatBadRes;
  if (n_joints < 1 || n_joints > kHeatMaxJoints) return kHeatBadJoints;
  if (layout != TSDF_LAYOUT_CZYX && layout != TSDF_LAYOUT_CXYZ) return kHeatBadLayout;
  if (dtype != TSDF_HEATMAP_F32 && bad_dtype(dtype)) return kHeatBadDtype;
  return kHeatGood;
}

inline HeatDefect heat_defect_encode(const float *d_u, const int32_t *d_status, int n, int n_joints, int R, float sigma,
                                     int layout, int dtype, const void *d_out_heat, const int32_t *d_out_valid) {
  const HeatDefect shape = heat_defect_shape(n, n_joints, R, layout, dtype);
  if (shape != kHeatGood) return shape;
  if (!(sigma > 0.f) || !(sigma <= 3.402823466e38f)) return kHeatBadScalar;   // a NaN fails the first, +inf the second
  if (!d_u || !d_out_heat) return kHeatNull;
  if (misaligned(d_out_heat, 15) || misaligned(d_u, 3) || misaligned(d_status, 3) || misaligned(d_out_valid, 3)) return kHeatUnaligned;
  if ((int64_t)n * n_joints >= kHeatMaxUnits) return kHeatTooMany;
  return kHeatGood;
}

inline HeatDefect heat_defect_decode(const void *d_heat, int dtype, int n, int n_joints, int R, int layout, int radius,
                                     const float *d_out_u, const float *d_out_peak, const int32_t *d_out_arg) {
  const HeatDefect shape = heat_defect_shape(n, n_joints, R, layout, dtype);
  if (shape != kHeatGood) return shape;
  if (radius < 0 || radius > kHeatMaxRadius) return kHeatBadScalar;
  if (!d_heat || !d_out_u) return kHeatNull;
  if (misaligned(d_heat, 15) || misaligned(d_out_u, 3) || misaligned(d_out_peak, 3) || misaligned(d_out_arg, 3)) return kHeatUnaligned;
  if ((int64_t)n * n_joints >= kHeatMaxUnits) return kHeatTooMany;
  return kHeatGood;
}

inline int heat_status(HeatDefect d) { return d == kHeatGood || d == kHeatNoop ? TSDF_OK : TSDF_ERR_INVALID_ARG; }

// The encode launch: a (frame, joint) pair's R slices of the slowest axis are cut into `nslab` slabs of `slab` slices,
// the last one shorter when slab does not divide R; one workgroup per slab.  One slab when there are pairs enough to
// give every CU two workgroups; otherwise as many slabs as bring the launch to about 2 * CUs workgroups without passing
// that number (floor), a slice per slab at least.
struct HeatPlan {
  int slab, nslab;
  int64_t blocks;
};

inline HeatPlan heat_plan(int64_t units, int R, int cus) {
  int64_t want = units > 0 ? 2 * (int64_t)cus / units : 1;
  if (want < 1) want = 1;
  if (want > R) want = R;
  HeatPlan p;
  p.slab = (R + (int)want - 1) / (int)want;
  p.nslab = (R + p.slab - 1) / p.slab;
  p.blocks = units * p.nslab;
  return p;
}

// x / d for 0 <= x < 2^24 and 1 <= d <= 128 as (x * heat_magic(d)) >> 31: with m = floor(2^31 / d) + 1, m * d = 2^31 + e,
// 0 < e <= d, and the quotient is exact while x * e < 2^31.  (An item number is below 128 * 128 * 32 = 2^19.)
TSDF_HEAT_FN unsigned heat_magic(int d) { return (unsigned)((1u << 31) / (unsigned)d + 1u); }
TSDF_HEAT_FN unsigned heat_div(unsigned x, unsigned magic) { return (unsigned)(((uint64_t)x * magic) >> 31); }

// Item `item` of a slab whose rows hold RV items of V voxels: the voxel it starts at on the fastest axis, its index on
// the middle axis and its slice within the slab.
struct HeatItem {
  int fast, mid, slice;
};
TSDF_HEAT_FN HeatItem heat_item(unsigned item, int R, int RV, int V, unsigned magic_rv, unsigned magic_r) {
  const unsigned row = heat_div(item, magic_rv), sl = heat_div(row, magic_r);
  HeatItem it;
  it.fast = (int)(item - row * (unsigned)RV) * V;
  it.mid = (int)(row - sl * (unsigned)R);
  it.slice = (int)sl;
  return it;
}
