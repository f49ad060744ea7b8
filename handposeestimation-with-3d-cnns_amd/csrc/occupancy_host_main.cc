// occupancy_host_main.cc — occupancy_host.inc (the text tsdf_occupancy.hip compiles) as a stand-alone host program that
// checks itself: make occupancy-host-asan builds it with g++ under -fsanitize=address,undefined,
// tests/test_occupancy_cpu.py runs it.
//   * the plan, for every R in 4..128 step 4 and every hint in 0..R + 2 and 1000, 2^31 - 1: every slice lies in exactly
//     one slab, no slab is empty, only the last one is short, the mask is 4 * ceil(slab * R * R / 32) bytes and at most
//     the cap, every bit index of every slab — the kernel's own expression — lies inside the mask; a hint is followed
//     unless the cap or R is smaller; the library's own plan has the fewest slabs the cap allows (one for R <= 80, two
//     for R = 88, four for R = 128) and no slab more than one slice larger than another;
//   * the argument rules: every defect alone is reported as itself, and of two defects the one earlier in the header's
//     order is reported.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/tsdf_occupancy.h"

// The three tests occupancy_host.inc takes from its includer, as device.inc and narrow.inc (which need HIP) state them,
// line for line: tests/test_occupancy_cpu.py compares these lines with those files.  cam_ok is prim.inc's own text.
bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
[[maybe_unused]] bool bad_res(int R) { return R < 4 || R > 128 || R % 4 != 0; }
bool bad_dtype(int dtype) { return dtype != TSDF_LOWP_F16 && dtype != TSDF_LOWP_BF16; }
#define TSDF_PRIM_HOST_ONLY
#include "prim.inc"

#include "occupancy_host.inc"

static int g_fail = 0;
#define CHECK(c, ...)                      \
  do {                                     \
    if (!(c)) {                            \
      if (++g_fail <= 20) {                \
        printf("FAILED %s: ", #c);         \
        printf(__VA_ARGS__);               \
        printf("\n");                      \
      }                                    \
    }                                      \
  } while (0)

static void check_plan(int R, int hint) {
  const OccPlan p = occ_plan(R, hint);
  CHECK(p.slab >= 1 && p.slab <= R && p.nslab >= 1 && p.nslab <= R, "R %d hint %d: slab %d nslab %d", R, hint, p.slab, p.nslab);
  if (p.slab < 1 || p.nslab < 1 || p.nslab > R) return;
  const int64_t bits = (int64_t)p.slab * R * R;
  CHECK(p.lds_bytes == 4 * ((bits + 31) / 32), "R %d hint %d: %d bytes", R, hint, p.lds_bytes);
  CHECK(p.lds_bytes <= kOccLdsCap, "R %d hint %d: %d bytes pass the cap", R, hint, p.lds_bytes);
  std::vector<int> seen(R, 0);
  for (int s = 0; s < p.nslab; ++s) {   // the kernel's own bounds
    const int sb = s * p.slab, se = sb + p.slab < R ? sb + p.slab : R;
    CHECK(se > sb, "R %d hint %d: slab %d is empty", R, hint, s);
    if (s + 1 < p.nslab) CHECK(se - sb == p.slab, "R %d hint %d: slab %d is short", R, hint, s);
    for (int z = sb; z < se; ++z) ++seen[z];
    // the last bit a point of this slab can set, the kernel's expression, and the words the expansion reads
    const int64_t last = ((int64_t)(se - 1 - sb) * R + (R - 1)) * R + (R - 1);
    CHECK(last / 32 < p.lds_bytes / 4, "R %d hint %d: bit %ld of slab %d outside the mask", R, hint, (long)last, s);
    const int64_t nbits = (int64_t)(se - sb) * R * R;
    CHECK(nbits % 16 == 0 && (nbits + 31) / 32 <= p.lds_bytes / 4, "R %d hint %d: slab %d has %ld bits", R, hint, s, (long)nbits);
  }
  for (int z = 0; z < R; ++z) CHECK(seen[z] == 1, "R %d hint %d: slice %d in %d slabs", R, hint, z, seen[z]);
  const int cap = (kOccLdsCap * 8) / (R * R) < R ? (kOccLdsCap * 8) / (R * R) : R;
  CHECK((int64_t)(cap + 1) * R * R > (int64_t)kOccLdsCap * 8 || cap == R, "R %d: cap %d", R, cap);
  if (hint > 0) {
    CHECK(p.slab == (hint < cap ? hint : cap), "R %d hint %d: slab %d", R, hint, p.slab);
    return;
  }
  // the library's plan
  if (p.nslab > 1) CHECK((int64_t)((R + p.nslab - 2) / (p.nslab - 1)) > cap, "R %d: %d slabs would do", R, p.nslab - 1);
  const int shortest = R - (p.nslab - 1) * p.slab;
  CHECK(p.nslab == 1 || p.slab - shortest <= p.nslab - 1, "R %d: slabs of %d and %d", R, p.slab, shortest);
  if (R <= 80) CHECK(p.nslab == 1 && p.slab == R, "R %d: %d slabs", R, p.nslab);
  if (R == 88) CHECK(p.nslab == 2 && p.slab == 44, "R 88: %d x %d", p.nslab, p.slab);
  if (R == 128) CHECK(p.nslab == 4 && p.slab == 32 && p.lds_bytes == kOccLdsCap, "R 128: %d x %d", p.nslab, p.slab);
}

template <typename P>
static const P *at(uintptr_t v) {
  return reinterpret_cast<const P *>(v);
}

static void check_rules() {
  const float inf = 1.0f / 0.0f, nan = inf - inf;
  const OccCall good = {at<float>(64), 100, at<int64_t>(64), at<int32_t>(64), 3, at<int64_t>(64), 3, 32, 241.42, 160.0, 120.0,
                        1.0f, 3.0f, 0, 0, 0, at<double>(64), at<float>(64), at<float>(64), at<void>(64)};
  CHECK(occ_defect(good) == kOccGood, "good arguments");
  // rule k of the order breaks with edit k; each edit touches a field no other edit touches (but n)
  typedef void (*Edit)(OccCall &);
  const Edit edits[] = {
      [](OccCall &a) { a.n = -1; },          [](OccCall &a) { a.R = 30; },          [](OccCall &a) { a.layout = 2; },
      [](OccCall &a) { a.dtype = 3; },       [](OccCall &a) { a.hint = -1; },       [](OccCall &a) { a.n = 0; },
      [](OccCall &a) { a.max_l = nullptr; }, [](OccCall &a) { a.depth_len = -1; },  [](OccCall &a) { a.n_src = 0; },
      [](OccCall &a) { a.out = at<void>(72); }, [](OccCall &a) { a.focal = 0.0; },
  };
  const OccDefect order[] = {kOccBadN,   kOccBadRes, kOccBadLayout, kOccBadDtype,  kOccBadHint, kOccNoop,
                             kOccNull,   kOccBadLen, kOccBadSrc,    kOccUnaligned, kOccBadCam};
  const int n_rules = (int)(sizeof(order) / sizeof(order[0]));
  for (int i = 0; i < n_rules; ++i) {
    OccCall a = good;
    edits[i](a);
    CHECK(occ_defect(a) == order[i], "rule %d alone gives %d", i, (int)occ_defect(a));
    CHECK(occ_status(occ_defect(a)) == (order[i] == kOccNoop ? TSDF_OK : TSDF_ERR_INVALID_ARG), "rule %d status", i);
    for (int j = i + 1; j < n_rules; ++j) {
      if ((i == 0 || i == 5) && (j == 0 || j == 5)) continue;   // n < 0 and n == 0 are one field
      OccCall b = a;
      edits[j](b);
      if (i == 0 && j != 5) b.n = -1;
      CHECK(occ_defect(b) == order[i], "rules %d and %d give %d", i, j, (int)occ_defect(b));
    }
  }
  // the values of each rule
  for (int R = -8; R <= 260; ++R) {
    OccCall a = good;
    a.R = R;
    CHECK((occ_defect(a) == kOccGood) == (R >= 4 && R <= 128 && R % 4 == 0), "R %d", R);
  }
  for (int dt = -1; dt <= 4; ++dt) {
    OccCall a = good;
    a.dtype = dt;
    CHECK((occ_defect(a) == kOccGood) == (dt >= 0 && dt <= 2), "dtype %d", dt);
  }
  for (int lay = -1; lay <= 3; ++lay) {
    OccCall a = good;
    a.layout = lay;
    CHECK((occ_defect(a) == kOccGood) == (lay == 0 || lay == 1), "layout %d", lay);
  }
  for (float v : {0.f, -0.f, -1.f, nan, -inf}) {
    OccCall a = good;
    a.eps = v;
    CHECK(occ_defect(a) == kOccBadCam, "invalid_eps %g", (double)v);
    a = good, a.trunc_vox = v;
    CHECK(occ_defect(a) == kOccBadCam, "trunc_voxels %g", (double)v);
    a = good, a.focal = (double)v;
    CHECK(occ_defect(a) == kOccBadCam, "focal %g", (double)v);
  }
  {   // the optional pointers, every required one, the source rule, the alignments and the launch's size
    OccCall a = good;
    a.xforms = nullptr, a.index = nullptr;
    CHECK(occ_defect(a) == kOccGood, "optional pointers");
    a = good, a.depth = nullptr;
    CHECK(occ_defect(a) == kOccNull, "no depth");
    a = good, a.offsets = nullptr;
    CHECK(occ_defect(a) == kOccNull, "no offsets");
    a = good, a.headers = nullptr;
    CHECK(occ_defect(a) == kOccNull, "no headers");
    a = good, a.mid_p = nullptr;
    CHECK(occ_defect(a) == kOccNull, "no mid_p");
    a = good, a.out = nullptr;
    CHECK(occ_defect(a) == kOccNull, "no output");
    a = good, a.index = nullptr, a.n_src = 4;
    CHECK(occ_defect(a) == kOccBadSrc, "no index and n_src != n");
    a = good, a.n_src = 1;
    CHECK(occ_defect(a) == kOccGood, "an index into one frame");
    a = good, a.xforms = at<double>(68);
    CHECK(occ_defect(a) == kOccUnaligned, "xforms");
    a = good, a.out = at<void>(80);
    CHECK(occ_defect(a) == kOccGood, "16-byte aligned output");
    a = good, a.depth_len = 0;
    CHECK(occ_defect(a) == kOccGood, "an empty depth buffer is the header rule's");
    a = good, a.n = 1 << 23;   // 2^23 workgroups of 512 lanes
    CHECK(occ_defect(a) == kOccTooMany, "too many");
    a.n = (1 << 23) - 1;
    CHECK(occ_defect(a) == kOccGood, "just few enough");
    a.R = 128;                 // four slabs each
    CHECK(occ_defect(a) == kOccTooMany, "too many slabs");
    a.n = (1 << 21) - 1;
    CHECK(occ_defect(a) == kOccGood, "just few enough slabs");
    a.hint = 1;                // 128 slabs each
    CHECK(occ_defect(a) == kOccTooMany, "too many by the hint");
  }
}

int main() {
  long plans = 0;
  for (int R = 4; R <= 128; R += 4) {
    for (int hint = 0; hint <= R + 2; ++hint, ++plans) check_plan(R, hint);
    check_plan(R, 1000);
    check_plan(R, 2147483647);
    plans += 2;
  }
  check_rules();
  if (g_fail) {
    printf("occupancy: %d checks FAILED\n", g_fail);
    return 1;
  }
  printf("occupancy host code ok (%ld plans)\n", plans);
  return 0;
}
