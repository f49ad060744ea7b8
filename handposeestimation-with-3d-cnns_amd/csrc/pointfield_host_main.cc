// pointfield_host_main.cc — pointfield_host.inc (the text tsdf_pointfield.hip compiles) as a stand-alone host program that
// checks itself: make pointfield-host-asan builds it with g++ under -fsanitize=address,undefined,
// tests/test_pointfield_cpu.py runs it.
//   * the plan: for every P the LDS bytes hold three float32 arrays of whole waves and the waves' counts inside 160 KiB,
//     16-byte aligned; the workgroups of a position cover its joints and no more; the register form's clouds fit its slots;
//   * the argument rules of both entries: every defect alone is reported as itself, and of two defects the one earlier
//     in the header's order is reported.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>
#include <limits>

#include "../../include/tsdf_pointfield.h"

// The test pointfield_host.inc takes from its includer, as device.inc (which needs HIP) states it, line for line:
// tests/test_pointfield_cpu.py compares this line with that file.
bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

#include "pointfield_host.inc"

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

static long check_plan() {
  long cases = 0;
  for (int P = 1; P <= TSDF_POINTFIELD_MAX_CLOUD; ++P) {
    const int pad = pf_padded(P);
    CHECK(pad >= P && pad - P < 64 && pad % 64 == 0, "P %d pads to %d", P, pad);
    for (int J : {1, kPfJoints - 1, kPfJoints, kPfJoints + 1, 21, TSDF_POINTFIELD_MAX_JOINTS}) {
      if (J < 1) continue;
      const PfPlan p = pf_plan(P, J);
      ++cases;
      CHECK(p.lds_bytes == 12 * pad + kPfTailBytes && p.lds_bytes % 16 == 0 && p.lds_bytes <= 160 * 1024, "P %d lds %d", P, p.lds_bytes);
      CHECK(p.joints == kPfJoints && (int64_t)p.groups * p.joints >= J && (int64_t)(p.groups - 1) * p.joints < J,
            "P %d J %d: %d groups", P, J, p.groups);
    }
  }
  CHECK(pf_plan(TSDF_POINTFIELD_MAX_CLOUD, 1).lds_bytes == 147472, "the cap's LDS");
  CHECK(pf_padded(64 * kPfRegSlots) / 64 == kPfRegSlots && pf_padded(64 * kPfRegSlots + 1) / 64 == kPfRegSlots + 1, "the register form's slots");
  CHECK(pf_elem(TSDF_POINTFIELD_F32) == 4 && pf_elem(TSDF_POINTFIELD_F16) == 2 && pf_elem(TSDF_POINTFIELD_BF16) == 2, "element sizes");
  return cases;
}

struct Call {
  PfIn in;
  int most_k;
  const void *field, *f4a, *f4b;
};

static PfDefect judge(const Call &c) { return pf_defect(c.in, c.most_k, c.field, c.f4a, c.f4b); }

static long check_rules() {
  const float *ok4 = reinterpret_cast<const float *>(64);
  const int32_t *st = reinterpret_cast<const int32_t *>(64);
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const Call good = {{ok4, 100, 3, 100, 21, 8, 30.0, TSDF_POINTFIELD_CP, TSDF_POINTFIELD_F32, st}, TSDF_POINTFIELD_MAX_K, ok4, ok4, ok4};
  CHECK(judge(good) == kPfGood, "good");
  // the defects in the header's order, each as a change of the good call
  struct Bad {
    PfDefect what;
    void (*make)(Call &);
  };
  static double s_inf, s_nan;
  s_inf = inf, s_nan = nan;
  const Bad bads[] = {
      {kPfBadN, [](Call &c) { c.in.n = -1; }},
      {kPfBadP, [](Call &c) { c.in.P = 0; }},
      {kPfBadP, [](Call &c) { c.in.P = TSDF_POINTFIELD_MAX_CLOUD + 1; }},
      {kPfBadJ, [](Call &c) { c.in.J = 0; }},
      {kPfBadJ, [](Call &c) { c.in.J = TSDF_POINTFIELD_MAX_JOINTS + 1; }},
      {kPfBadK, [](Call &c) { c.in.K = 0; }},
      {kPfBadK, [](Call &c) { c.in.K = TSDF_POINTFIELD_MAX_K + 1; }},
      {kPfBadPitch, [](Call &c) { c.in.pitch = 99; }},
      {kPfBadRadius, [](Call &c) { c.in.radius = 0.0; }},
      {kPfBadRadius, [](Call &c) { c.in.radius = -1.0; }},
      {kPfBadRadius, [](Call &c) { c.in.radius = s_inf; }},
      {kPfBadRadius, [](Call &c) { c.in.radius = s_nan; }},
      {kPfBadLayout, [](Call &c) { c.in.layout = 2; }},
      {kPfBadLayout, [](Call &c) { c.in.layout = -1; }},
      {kPfBadDtype, [](Call &c) { c.in.dtype = 3; }},
      {kPfBadDtype, [](Call &c) { c.in.dtype = -1; }},
      {kPfNoop, [](Call &c) { c.in.n = 0; }},
      {kPfNull, [](Call &c) { c.in.points = nullptr; }},
      {kPfNull, [](Call &c) { c.field = nullptr; }},
      {kPfNull, [](Call &c) { c.f4a = nullptr; }},
      {kPfNull, [](Call &c) { c.f4b = nullptr; }},
      {kPfNull, [](Call &c) { c.in.status = nullptr; }},
      {kPfUnaligned, [](Call &c) { c.in.points = reinterpret_cast<const float *>(66); }},
      {kPfUnaligned, [](Call &c) { c.field = reinterpret_cast<const float *>(66); }},
      {kPfUnaligned, [](Call &c) { c.f4a = reinterpret_cast<const float *>(66); }},
      {kPfUnaligned, [](Call &c) { c.f4b = reinterpret_cast<const float *>(65); }},
      {kPfTooMany, [](Call &c) { c.in.n = 1 << 22; }},   // 6 groups a position
  };
  long cases = 0;
  const int count = (int)(sizeof bads / sizeof bads[0]);
  for (int i = 0; i < count; ++i) {
    Call one = good;
    bads[i].make(one);
    CHECK(judge(one) == bads[i].what, "defect %d alone", i);
    ++cases;
    for (int j = i + 1; j < count; ++j) {
      if (bads[j].what == bads[i].what) continue;
      Call two = good;
      bads[j].make(two);   // the later one first, so that the earlier one's change stands
      bads[i].make(two);
      CHECK(judge(two) == bads[i].what, "defects %d and %d", i, j);
      ++cases;
    }
  }
  // decode's cap on M; a 2-byte field may sit on an even address; the boundary of the launch
  Call c = good;
  c.most_k = TSDF_POINTFIELD_MAX_VOTES;
  c.in.K = TSDF_POINTFIELD_MAX_VOTES;
  CHECK(judge(c) == kPfGood, "M at its cap");
  c.in.K = TSDF_POINTFIELD_MAX_VOTES + 1;
  CHECK(judge(c) == kPfBadK, "M above its cap");
  c = good;
  c.in.K = TSDF_POINTFIELD_MAX_K;
  CHECK(judge(c) == kPfGood, "K at its cap, above P");
  c.field = reinterpret_cast<const float *>(66);
  c.in.dtype = TSDF_POINTFIELD_BF16;
  CHECK(judge(c) == kPfGood, "a 2-byte field at an even address");
  c.field = reinterpret_cast<const float *>(65);
  CHECK(judge(c) == kPfUnaligned, "a 2-byte field at an odd address");
  c = good;
  c.in.J = kPfJoints;
  c.in.n = (1 << 24) - 1;
  CHECK(judge(c) == kPfGood, "one group a position, just below 2^32 work-items");
  c.in.n = 1 << 24;
  CHECK(judge(c) == kPfTooMany, "2^32 work-items");
  c.in.J = kPfJoints + 1;
  c.in.n = (1 << 23) - 1;
  CHECK(judge(c) == kPfGood, "two groups a position");
  c.in.n = 1 << 23;
  CHECK(judge(c) == kPfTooMany, "two groups a position, 2^32 work-items");
  CHECK(pf_status(kPfGood) == TSDF_OK && pf_status(kPfNoop) == TSDF_OK && pf_status(kPfTooMany) == TSDF_ERR_INVALID_ARG, "status");
  CHECK(pf_encode_defect(good.in, ok4, ok4, st) == kPfGood && pf_decode_defect(good.in, ok4, ok4, ok4) == kPfGood, "the two entries");
  CHECK(pf_decode_defect(good.in, ok4, nullptr, ok4) == kPfNull && pf_encode_defect(good.in, nullptr, ok4, st) == kPfNull, "their pointers");
  return cases;
}

int main() {
  const long plans = check_plan();
  const long rules = check_rules();
  if (g_fail) {
    printf("pointfield host code: %d checks FAILED\n", g_fail);
    return 1;
  }
  printf("pointfield host code ok (%d lanes, %d joints a group, cap %d, %ld plans, %ld rule cases)\n", kPfWG, kPfJoints,
         TSDF_POINTFIELD_MAX_CLOUD, plans, rules);
  return 0;
}
