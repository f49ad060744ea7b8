// fps_host_main.cc — fps_host.inc (the text tsdf_fps.hip compiles) as a stand-alone host program that checks itself:
// make fps-host-asan builds it with g++ under -fsanitize=address,undefined, tests/test_fps_cpu.py runs it.
//   * the plan: the resident cap is at least 8192 and slots x lanes, the LDS bytes hold three float32 arrays of it, the
//     two key rows and the wave counts inside 160 KiB, the workspace is 16 bytes per candidate;
//   * the form: every (count, workspace, capacity, hint) around the cap and the capacity holds exactly when the header
//     says so, and streams exactly when the hint or the cap says so;
//   * the slots: candidate c of lane c % WG and slot c / WG is below the trip count, and the trip count is the least;
//   * the segments: for item counts around every multiple of the wave count and of 64, and up to 2^31 - 1, the waves'
//     pieces are disjoint, in order, multiples of 64 long and cover every item;
//   * the argument rules of both entries: every defect alone is reported as itself, and of two defects the one earlier
//     in the header's order is reported.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "../../include/tsdf_fps.h"

// The test fps_host.inc takes from its includer, as device.inc (which needs HIP) states it, line for line:
// tests/test_fps_cpu.py compares this line with that file.  cam_ok is prim.inc's own text.
bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
#define TSDF_PRIM_HOST_ONLY
#include "prim.inc"

#include "fps_host.inc"

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

static void check_plan() {
  CHECK(kFpsResident >= 8192 && kFpsSlots * kFpsWG == kFpsResident, "cap %d", kFpsResident);
  CHECK(kFpsLdsBytes == 12 * kFpsResident + 16 * kFpsWaves + 4 * kFpsWaves && kFpsLdsBytes <= 160 * 1024, "lds %d", kFpsLdsBytes);
  CHECK(kFpsWaves <= 16 && 16 % kFpsWaves == 0, "%d waves: the exchange reads the rows' keys with lanes 0..15", kFpsWaves);
  for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)76800, kFpsMaxRank}) {
    const FpsPlan p = fps_plan(cap);
    CHECK(p.resident_cap == kFpsResident && p.lds_bytes == kFpsLdsBytes && p.work_bytes == 16 * cap, "plan %ld", (long)cap);
  }
}

static long check_forms() {
  long cases = 0;
  const int64_t counts[] = {1, 2, 100, kFpsResident - 1, kFpsResident, kFpsResident + 1, 76800, kFpsMaxRank};
  const int64_t caps[] = {1, 99, 100, 101, kFpsResident, kFpsResident + 1, 76799, 76800, kFpsMaxRank};
  for (int64_t count : counts)
    for (int hint = 0; hint <= 1; ++hint) {
      // no workspace
      const FpsForm bare = fps_holds(count, false, 0, hint);
      CHECK(bare == (count <= kFpsResident ? kFpsFormResident : kFpsNone), "count %ld bare", (long)count);
      ++cases;
      for (int64_t cap : caps) {
        ++cases;
        const FpsForm f = fps_holds(count, true, cap, hint);
        const bool holds = count <= kFpsResident || count <= cap;
        CHECK((f != kFpsNone) == holds, "count %ld cap %ld hint %d holds", (long)count, (long)cap, hint);
        const bool streams = count <= cap && (hint == 1 || count > kFpsResident);
        CHECK((f == kFpsFormStreaming) == streams, "count %ld cap %ld hint %d streams", (long)count, (long)cap, hint);
      }
    }
  return cases;
}

static void check_slots() {
  for (int count = 1; count <= kFpsResident; ++count) {
    const int s = fps_slots(count);
    CHECK(s >= 1 && s <= kFpsSlots && (count - 1) / kFpsWG < s && (int64_t)(s - 1) * kFpsWG < count, "count %d: %d slots", count, s);
  }
}

static long check_segments() {
  long cases = 0;
  auto one = [&](int64_t items) {
    if (items < 1 || items > kFpsMaxRank) return;
    ++cases;
    const int64_t seg = fps_segment(items);
    CHECK(seg > 0 && seg % 64 == 0, "items %ld: seg %ld", (long)items, (long)seg);
    CHECK(seg * kFpsWaves >= items, "items %ld: the pieces end at %ld", (long)items, (long)(seg * kFpsWaves));
    CHECK(seg * kFpsWaves - items < (int64_t)64 * kFpsWaves + kFpsWaves, "items %ld: seg %ld is too long", (long)items, (long)seg);
    int64_t covered = 0;
    for (int w = 0; w < kFpsWaves; ++w) {   // the kernel's own bounds
      const int64_t b = w * seg, e = b + seg < items ? b + seg : items;
      if (b < e) {
        CHECK(b == covered, "items %ld: wave %d starts at %ld after %ld", (long)items, w, (long)b, (long)covered);
        covered = e;
      }
    }
    CHECK(covered == items, "items %ld: %ld covered", (long)items, (long)covered);
  };
  for (int64_t m = 0; m <= 40; ++m)
    for (int64_t d = -2; d <= 2; ++d) {
      one(m * kFpsWaves + d);
      one(m * 64 + d);
      one(m * 64 * kFpsWaves + d);
    }
  for (int64_t items : {(int64_t)9216, (int64_t)76800, (int64_t)1 << 30, kFpsMaxRank - 1, kFpsMaxRank}) one(items);
  return cases;
}

template <typename P>
static const P *at(uintptr_t v) {
  return reinterpret_cast<const P *>(v);
}

static void check_rules() {
  const float inf = 1.0f / 0.0f, nan = inf - inf;
  const FpsOut out = {3, 1024, 100, 0, at<float>(64), at<float>(64), at<int32_t>(64), at<int32_t>(64), at<int32_t>(64)};
  const FpsCall good = {at<float>(64), 100, at<int64_t>(64), at<int32_t>(64), 3, at<int64_t>(64), 241.42, 160.0, 120.0, 1.0f,
                        3.0f, at<double>(64), out};
  CHECK(fps_defect(good) == kFpsGood, "good arguments");
  {   // rule k of the order breaks with edit k; each edit touches a field no other edit touches (but n)
    typedef void (*Edit)(FpsCall &);
    const Edit edits[] = {
        [](FpsCall &a) { a.o.n = -1; },          [](FpsCall &a) { a.o.M = 0; },           [](FpsCall &a) { a.o.hint = 2; },
        [](FpsCall &a) { a.o.capacity = -1; },   [](FpsCall &a) { a.o.n = 0; },           [](FpsCall &a) { a.o.pixel = nullptr; },
        [](FpsCall &a) { a.depth_len = -1; },    [](FpsCall &a) { a.n_src = 0; },         [](FpsCall &a) { a.o.work = nullptr; },
        [](FpsCall &a) { a.xforms = at<double>(68); }, [](FpsCall &a) { a.focal = 0.0; },
    };
    const FpsDefect order[] = {kFpsBadN, kFpsBadM,   kFpsBadHint, kFpsBadCap,    kFpsNoop,  kFpsNull,
                               kFpsBadLen, kFpsBadSrc, kFpsBadWork, kFpsUnaligned, kFpsBadCam};
    const int n_rules = (int)(sizeof(order) / sizeof(order[0]));
    for (int i = 0; i < n_rules; ++i) {
      FpsCall a = good;
      edits[i](a);
      CHECK(fps_defect(a) == order[i], "rule %d alone gives %d", i, (int)fps_defect(a));
      CHECK(fps_status(fps_defect(a)) == (order[i] == kFpsNoop ? TSDF_OK : TSDF_ERR_INVALID_ARG), "rule %d status", i);
      for (int j = i + 1; j < n_rules; ++j) {
        if ((i == 0 || i == 4) && (j == 0 || j == 4)) continue;   // n < 0 and n == 0 are one field
        FpsCall b = a;
        edits[j](b);
        if (i == 0 && j != 4) b.o.n = -1;
        CHECK(fps_defect(b) == order[i], "rules %d and %d give %d", i, j, (int)fps_defect(b));
      }
    }
  }
  {   // the same for the cloud entry
    const FpsPointsCall fine = {at<void>(64), TSDF_FPS_F64, 6000, out};
    CHECK(fps_points_defect(fine) == kFpsGood, "good cloud arguments");
    typedef void (*Edit)(FpsPointsCall &);
    const Edit edits[] = {
        [](FpsPointsCall &a) { a.o.n = -1; },        [](FpsPointsCall &a) { a.o.M = 65537; }, [](FpsPointsCall &a) { a.o.hint = -1; },
        [](FpsPointsCall &a) { a.o.capacity = (int64_t)1 << 31; }, [](FpsPointsCall &a) { a.dtype = 2; },
        [](FpsPointsCall &a) { a.P = 0; },           [](FpsPointsCall &a) { a.o.n = 0; },     [](FpsPointsCall &a) { a.o.status = nullptr; },
        [](FpsPointsCall &a) { a.o.work = nullptr; }, [](FpsPointsCall &a) { a.points = at<void>(68); },
    };
    const FpsDefect order[] = {kFpsBadN,    kFpsBadM, kFpsBadHint, kFpsBadCap,  kFpsBadDtype,
                               kFpsBadRows, kFpsNoop, kFpsNull,    kFpsBadWork, kFpsUnaligned};
    const int n_rules = (int)(sizeof(order) / sizeof(order[0]));
    for (int i = 0; i < n_rules; ++i) {
      FpsPointsCall a = fine;
      edits[i](a);
      CHECK(fps_points_defect(a) == order[i], "cloud rule %d alone gives %d", i, (int)fps_points_defect(a));
      for (int j = i + 1; j < n_rules; ++j) {
        if ((i == 0 || i == 6) && (j == 0 || j == 6)) continue;
        FpsPointsCall b = a;
        edits[j](b);
        if (i == 0 && j != 6) b.o.n = -1;
        CHECK(fps_points_defect(b) == order[i], "cloud rules %d and %d give %d", i, j, (int)fps_points_defect(b));
      }
    }
    FpsPointsCall a = fine;
    a.dtype = TSDF_FPS_F32, a.points = at<void>(68);
    CHECK(fps_points_defect(a) == kFpsGood, "a float32 cloud on a 4-byte boundary");
    a.points = at<void>(66);
    CHECK(fps_points_defect(a) == kFpsUnaligned, "a float32 cloud off it");
    a = fine, a.P = kFpsMaxRank;
    CHECK(fps_points_defect(a) == kFpsGood, "2^31 - 1 rows");
    a.P = kFpsMaxRank + 1;
    CHECK(fps_points_defect(a) == kFpsBadRows, "2^31 rows");
  }
  // the values of each rule
  for (int M = -2; M <= 65538; ++M) {
    FpsCall a = good;
    a.o.M = M;
    CHECK((fps_defect(a) == kFpsGood) == (M >= 1 && M <= 65536), "M %d", M);
  }
  for (int hint = -2; hint <= 3; ++hint) {
    FpsCall a = good;
    a.o.hint = hint;
    CHECK((fps_defect(a) == kFpsGood) == (hint == 0 || hint == 1), "hint %d", hint);
  }
  for (float v : {0.f, -0.f, -1.f, nan, -inf}) {
    FpsCall a = good;
    a.eps = v;
    CHECK(fps_defect(a) == kFpsBadCam, "invalid_eps %g", (double)v);
    a = good, a.trunc_vox = v;
    CHECK(fps_defect(a) == kFpsBadCam, "trunc_voxels %g", (double)v);
    a = good, a.focal = (double)v;
    CHECK(fps_defect(a) == kFpsBadCam, "focal %g", (double)v);
  }
  {   // the optional pointers, every required one, the source rule, the workspace, the alignments and the launch's size
    FpsCall a = good;
    a.xforms = nullptr, a.index = nullptr;
    CHECK(fps_defect(a) == kFpsGood, "optional pointers");
    a = good, a.o.work = nullptr, a.o.capacity = 0;
    CHECK(fps_defect(a) == kFpsGood, "no workspace");
    a = good, a.o.capacity = 0;
    CHECK(fps_defect(a) == kFpsBadWork, "a workspace of no capacity");
    a = good, a.o.capacity = kFpsMaxRank;
    CHECK(fps_defect(a) == kFpsGood, "the largest capacity");
    a = good, a.depth = nullptr;
    CHECK(fps_defect(a) == kFpsNull, "no depth");
    a = good, a.offsets = nullptr;
    CHECK(fps_defect(a) == kFpsNull, "no offsets");
    a = good, a.headers = nullptr;
    CHECK(fps_defect(a) == kFpsNull, "no headers");
    a = good, a.o.points = nullptr;
    CHECK(fps_defect(a) == kFpsNull, "no points");
    a = good, a.o.count = nullptr;
    CHECK(fps_defect(a) == kFpsNull, "no count");
    a = good, a.o.status = nullptr;
    CHECK(fps_defect(a) == kFpsNull, "no status");
    a = good, a.index = nullptr, a.n_src = 4;
    CHECK(fps_defect(a) == kFpsBadSrc, "no index and n_src != n");
    a = good, a.n_src = 1;
    CHECK(fps_defect(a) == kFpsGood, "an index into one frame");
    a = good, a.o.work = at<float>(72);
    CHECK(fps_defect(a) == kFpsUnaligned, "workspace");
    a = good, a.depth_len = 0;
    CHECK(fps_defect(a) == kFpsGood, "an empty depth buffer is the header rule's");
    a = good, a.o.n = (int)(kFpsMaxItems / kFpsWG);
    CHECK(fps_defect(a) == kFpsTooMany, "too many");
    a.o.n -= 1;
    CHECK(fps_defect(a) == kFpsGood, "just few enough");
  }
}

int main() {
  check_plan();
  const long forms = check_forms();
  check_slots();
  const long segs = check_segments();
  check_rules();
  if (g_fail) {
    printf("fps: %d checks FAILED\n", g_fail);
    return 1;
  }
  printf("fps host code ok (%d lanes, cap %d, %ld forms, %ld segments)\n", kFpsWG, kFpsResident, forms, segs);
  return 0;
}
