// occupancy_host.inc — the host side of libtsdf_occupancy.so that needs no device: the argument rules of its entry and
// the launch's plan.  Plain C++: tsdf_occupancy.hip includes it (inside its anonymous namespace, after
// include/tsdf_occupancy.h), and occupancy_host_main.cc includes it into a stand-alone program built under the CPU
// sanitizers (make occupancy-host-asan; tests/test_occupancy_cpu.py runs it).
//   occ_plan     slices per workgroup, workgroups per batch position and the bytes of the LDS bit mask from (R, hint)
//   occ_defect   the first argument rule the entry's arguments break, in the header's order.  The tests that exist
//                already are not restated: bad_res and misaligned (device.inc), bad_dtype (narrow.inc) and cam_ok
//                (prim.inc) must be declared before this file is included — the library has them from those files, the
//                stand-alone program carries the text of the first three and takes cam_ok from prim.inc's host-only half

constexpr int kOccWG = 512;                  // threads per workgroup (8 wave64)
constexpr int kOccLdsCap = 64 * 1024;        // bytes of bit mask per workgroup: two workgroups share a CU's LDS
constexpr int64_t kOccMaxItems = (int64_t)1 << 32;   // work-items of one launch

// A batch position's R slices of the slowest axis as `nslab` slabs of `slab` slices, the last one shorter when slab does
// not divide R.  A slice is R * R bits, a multiple of 16.
struct OccPlan {
  int slab, nslab, lds_bytes;
};

// R passes bad_res, hint >= 0
inline OccPlan occ_plan(int R, int hint) {
  const int slice_bits = R * R;
  int cap = (kOccLdsCap * 8) / slice_bits;   // slices the cap holds: >= 32 (R = 128)
  if (cap > R) cap = R;
  OccPlan p;
  if (hint > 0) {
    p.slab = hint < cap ? hint : cap;
  } else {   // the fewest slabs the cap allows, of equal size up to rounding
    const int fewest = (R + cap - 1) / cap;
    p.slab = (R + fewest - 1) / fewest;
  }
  p.nslab = (R + p.slab - 1) / p.slab;
  p.lds_bytes = 4 * ((p.slab * slice_bits + 31) / 32);
  return p;
}

// The rules in the order they are judged; the entry returns TSDF_OK for kOccNoop, TSDF_ERR_INVALID_ARG for any other
// value but kOccGood.
enum OccDefect {
  kOccGood = 0,
  kOccBadN,        // n < 0
  kOccBadRes,      // R: device.inc::bad_res's rule (a multiple of 4 in 4..128)
  kOccBadLayout,
  kOccBadDtype,
  kOccBadHint,     // slab_hint < 0
  kOccNoop,        // n == 0: nothing to do, whatever else is passed
  kOccNull,        // a required pointer is NULL
  kOccBadLen,      // depth_len < 0
  kOccBadSrc,      // n_src < 1, or no index and n_src != n
  kOccUnaligned,   // d_xforms off an 8-byte boundary, d_out_occ off a 16-byte one
  kOccBadCam,
  kOccTooMany      // n * nslab * kOccWG >= 2^32
};

struct OccCall {
  const float *depth;
  int64_t depth_len;
  const int64_t *offsets;
  const int32_t *headers;
  int64_t n_src;
  const int64_t *index;
  int n, R;
  double focal, cx, cy;
  float eps, trunc_vox;
  int layout, dtype, hint;
  const double *xforms;
  const float *max_l, *mid_p;
  const void *out;
};

inline OccDefect occ_defect(const OccCall &c) {
  if (c.n < 0) return kOccBadN;
  if (bad_res(c.R)) return kOccBadRes;
  if (c.layout != TSDF_LAYOUT_CZYX && c.layout != TSDF_LAYOUT_CXYZ) return kOccBadLayout;
  if (c.dtype != TSDF_HEATMAP_F32 && bad_dtype(c.dtype)) return kOccBadDtype;
  if (c.hint < 0) return kOccBadHint;
  if (c.n == 0) return kOccNoop;
  if (!c.depth || !c.offsets || !c.headers || !c.max_l || !c.mid_p || !c.out) return kOccNull;
  if (c.depth_len < 0) return kOccBadLen;
  if (c.n_src < 1 || (!c.index && c.n_src != c.n)) return kOccBadSrc;
  if (misaligned(c.xforms, 7) || misaligned(c.out, 15)) return kOccUnaligned;
  const tsdf_cam cam = {c.focal, c.cx, c.cy, c.eps, c.trunc_vox};   // by value in the ABI, one rule all the same
  if (!cam_ok(&cam)) return kOccBadCam;
  if ((int64_t)c.n * occ_plan(c.R, c.hint).nslab * kOccWG >= kOccMaxItems) return kOccTooMany;
  return kOccGood;
}

inline int occ_status(OccDefect d) { return d == kOccGood || d == kOccNoop ? TSDF_OK : TSDF_ERR_INVALID_ARG; }
