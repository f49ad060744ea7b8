// group_host_main.cc — group_host.inc (the text tsdf_group.hip compiles) as a stand-alone host program that checks
// itself: make group-host-asan builds it with g++ under -fsanitize=address,undefined, tests/test_group_cpu.py runs it.
//   * the plan: for every P the LDS bytes hold three float32 arrays of whole waves and the waves' counts inside 160 KiB,
//     16-byte aligned; the workgroups of a position cover its queries and no more;
//   * the segments: for every P the waves' pieces are disjoint, in order, multiples of 64 long and cover every row;
//   * the argument rules of both entries: every defect alone is reported as itself, and of two defects the one earlier
//     in the header's order is reported.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "../../include/tsdf_group.h"

// The test group_host.inc takes from its includer, as device.inc (which needs HIP) states it, line for line:
// tests/test_group_cpu.py compares this line with that file.
bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

#include "group_host.inc"

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
  for (int P = 1; P <= TSDF_GROUP_MAX_CLOUD; ++P) {
    const int pad = grp_padded(P);
    CHECK(pad >= P && pad - P < 64 && pad % 64 == 0, "P %d pads to %d", P, pad);
    for (int C : {1, kGrpQueries - 1, kGrpQueries, kGrpQueries + 1, P, 0x7fffffff}) {
      const GrpPlan p = grp_plan(P, C);
      ++cases;
      CHECK(p.lds_bytes == 12 * pad + kGrpTailBytes && p.lds_bytes % 16 == 0 && p.lds_bytes <= 160 * 1024, "P %d lds %d", P, p.lds_bytes);
      CHECK(p.queries == kGrpQueries && (int64_t)p.groups * p.queries >= C && (int64_t)(p.groups - 1) * p.queries < C,
            "P %d C %d: %d groups", P, C, p.groups);
    }
  }
  CHECK(grp_plan(TSDF_GROUP_MAX_CLOUD, 1).lds_bytes == 147472, "the cap's LDS");
  return cases;
}

static void check_segments() {
  for (int P = 1; P <= TSDF_GROUP_MAX_CLOUD; ++P) {
    const int seg = grp_segment(P);
    CHECK(seg % 64 == 0 && seg >= 64 && (int64_t)seg * kGrpWaves >= P, "P %d seg %d", P, seg);
    int covered = 0;
    for (int w = 0; w < kGrpWaves; ++w) {
      const int b = w * seg, e = b + seg < P ? b + seg : P;
      if (b < e) {
        CHECK(b == covered, "P %d wave %d starts at %d", P, w, b);
        covered = e;
      }
    }
    CHECK(covered == P, "P %d covered %d", P, covered);
  }
}

struct Call {
  GrpIn in;
  const void *first, *a4, *b4, *v8;
};

static GrpDefect judge(const Call &c) { return grp_defect(c.in, c.first, c.a4, c.b4, c.v8); }

static long check_rules() {
  const float *ok4 = reinterpret_cast<const float *>(64);
  const int32_t *st = reinterpret_cast<const int32_t *>(64);
  const Call good = {{ok4, 100, ok4, 3, 100, 50, 8, st}, ok4, ok4, ok4, ok4};
  CHECK(judge(good) == kGrpGood, "good");
  // the defects in the header's order, each as a change of the good call
  struct Bad {
    GrpDefect what;
    void (*make)(Call &);
  };
  const Bad bads[] = {
      {kGrpBadN, [](Call &c) { c.in.n = -1; }},
      {kGrpBadP, [](Call &c) { c.in.P = 0; }},
      {kGrpBadP, [](Call &c) { c.in.P = TSDF_GROUP_MAX_CLOUD + 1; }},
      {kGrpBadC, [](Call &c) { c.in.C = 0; }},
      {kGrpBadK, [](Call &c) { c.in.K = 0; }},
      {kGrpBadK, [](Call &c) { c.in.K = TSDF_GROUP_MAX_K + 1; }},
      {kGrpBadPitch, [](Call &c) { c.in.pitch = 99; }},
      {kGrpNoop, [](Call &c) { c.in.n = 0; }},
      {kGrpNull, [](Call &c) { c.in.points = nullptr; }},
      {kGrpNull, [](Call &c) { c.first = nullptr; }},
      {kGrpNull, [](Call &c) { c.in.status = nullptr; }},
      {kGrpBadPrefix, [](Call &c) { c.in.query = nullptr, c.in.C = 101; }},
      {kGrpUnaligned, [](Call &c) { c.in.points = reinterpret_cast<const float *>(66); }},
      {kGrpUnaligned, [](Call &c) { c.in.query = reinterpret_cast<const float *>(66); }},
      {kGrpUnaligned, [](Call &c) { c.a4 = reinterpret_cast<const float *>(66); }},
      {kGrpUnaligned, [](Call &c) { c.b4 = reinterpret_cast<const float *>(65); }},
      {kGrpUnaligned, [](Call &c) { c.v8 = reinterpret_cast<const float *>(68); }},
      {kGrpTooMany, [](Call &c) { c.in.n = 1 << 23; }},
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
  // the optional pointers may be NULL; C <= P holds without a query tensor; the boundary of the launch
  Call c = good;
  c.in.query = nullptr, c.a4 = c.b4 = c.v8 = nullptr;
  CHECK(judge(c) == kGrpGood, "optional pointers");
  c.in.C = 100;
  CHECK(judge(c) == kGrpGood, "C == P");
  c = good;
  c.in.n = (1 << 23) - 1;   // 2 groups a position: 2^24 - 2 groups of 256
  CHECK(judge(c) == kGrpGood, "just below 2^32 work-items");
  c.in.C = 32;
  c.in.n = (1 << 24) - 1;
  CHECK(judge(c) == kGrpGood, "one group a position");
  c.in.n = 1 << 24;
  CHECK(judge(c) == kGrpTooMany, "2^32 work-items");
  CHECK(grp_status(kGrpGood) == TSDF_OK && grp_status(kGrpNoop) == TSDF_OK && grp_status(kGrpTooMany) == TSDF_ERR_INVALID_ARG, "status");
  return cases;
}

int main() {
  const long plans = check_plan();
  check_segments();
  const long rules = check_rules();
  if (g_fail) {
    printf("group host code: %d checks FAILED\n", g_fail);
    return 1;
  }
  printf("group host code ok (%d lanes, %d queries a group, cap %d, %ld plans, %ld rule cases)\n", kGrpWG, kGrpQueries,
         TSDF_GROUP_MAX_CLOUD, plans, rules);
  return 0;
}
