// group_host.inc — the host side of libtsdf_group.so that needs no device: the argument rules of its two entries and
// the plan.  Plain C++: tsdf_group.hip includes it (inside its anonymous namespace, after include/tsdf_group.h), and
// group_host_main.cc includes it into a stand-alone program built under the CPU sanitizers (make group-host-asan;
// tests/test_group_cpu.py runs it).
//   grp_plan         the LDS bytes, the queries per workgroup and the workgroups per position
//   grp_padded       the cloud's rows rounded up to whole waves: the extent of each LDS array
//   grp_segment      the piece of the cloud each wave compacts
//   grp_knn_defect   the first argument rule tsdf_knn_hip's arguments break, in the header's order
//   grp_normals_defect  the same for tsdf_normals_hip
// misaligned (device.inc) must be declared before this file is included — the library has it from that file, the
// stand-alone program carries its text.

constexpr int kGrpWG = 256;                      // threads per workgroup
constexpr int kGrpWaves = kGrpWG / 64;
constexpr int kGrpPerWave = 8;                   // queries a wave answers, one after the other
constexpr int kGrpQueries = kGrpWaves * kGrpPerWave;   // queries per workgroup
constexpr int kGrpTailBytes = 16;                // the waves' candidate counts, behind the three coordinate arrays
constexpr int64_t kGrpMaxItems = (int64_t)1 << 32;     // work-items of one launch
static_assert(kGrpPerWave <= 64, "the normals kernel keeps query j of a wave in lane j");
static_assert(TSDF_GROUP_MAX_CLOUD % 64 == 0 && 12 * TSDF_GROUP_MAX_CLOUD + kGrpTailBytes <= 160 * 1024, "the LDS budget");
static_assert(kGrpWaves * 4 <= kGrpTailBytes, "one count per wave");

// P rounded up to whole waves; P in 1..TSDF_GROUP_MAX_CLOUD
constexpr int grp_padded(int P) { return (P + 63) / 64 * 64; }

// Wave w compacts the rows [w * seg, min((w + 1) * seg, P)) in steps of 64: seg is a multiple of 64, the pieces are
// disjoint, in order, and cover every row.
constexpr int grp_segment(int P) { return ((P + kGrpWaves - 1) / kGrpWaves + 63) / 64 * 64; }

struct GrpPlan {
  int lds_bytes, queries, groups;
};

// P in 1..TSDF_GROUP_MAX_CLOUD, C >= 1
inline GrpPlan grp_plan(int P, int C) {
  return {12 * grp_padded(P) + kGrpTailBytes, kGrpQueries, (int)(((int64_t)C + kGrpQueries - 1) / kGrpQueries)};
}

// The rules in the order they are judged; an entry returns TSDF_OK for kGrpNoop, TSDF_ERR_INVALID_ARG for any other
// value but kGrpGood.
enum GrpDefect {
  kGrpGood = 0,
  kGrpBadN,        // n < 0
  kGrpBadP,        // P outside 1..TSDF_GROUP_MAX_CLOUD
  kGrpBadC,        // C < 1
  kGrpBadK,        // K outside 1..TSDF_GROUP_MAX_K
  kGrpBadPitch,    // pitch < P
  kGrpNoop,        // n == 0: nothing to do, whatever else is passed
  kGrpNull,        // a required pointer is NULL
  kGrpBadPrefix,   // no d_query and C > P
  kGrpUnaligned,
  kGrpTooMany      // n * groups * kGrpWG >= 2^32
};

// what the two entries share
struct GrpIn {
  const float *points;
  int64_t pitch;
  const float *query;
  int n, P, C, K;
  const int32_t *status;   // the OUTPUT status
};

inline GrpDefect grp_shape_defect(int P, int C, int K) {
  if (P < 1 || P > TSDF_GROUP_MAX_CLOUD) return kGrpBadP;
  if (C < 1) return kGrpBadC;
  if (K < 1 || K > TSDF_GROUP_MAX_K) return kGrpBadK;
  return kGrpGood;
}

// `first`: the entry's first output; a4 / b4: its optional float32 pointers; v8: its optional float64 pointer
inline GrpDefect grp_defect(const GrpIn &c, const void *first, const void *a4, const void *b4, const void *v8) {
  if (c.n < 0) return kGrpBadN;
  const GrpDefect shape = grp_shape_defect(c.P, c.C, c.K);
  if (shape != kGrpGood) return shape;
  if (c.pitch < c.P) return kGrpBadPitch;
  if (c.n == 0) return kGrpNoop;
  if (!c.points || !first || !c.status) return kGrpNull;
  if (!c.query && c.C > c.P) return kGrpBadPrefix;
  if (misaligned(c.points, 3) || misaligned(c.query, 3) || misaligned(a4, 3) || misaligned(b4, 3) || misaligned(v8, 7))
    return kGrpUnaligned;
  if ((int64_t)c.n * grp_plan(c.P, c.C).groups * kGrpWG >= kGrpMaxItems) return kGrpTooMany;
  return kGrpGood;
}

inline GrpDefect grp_knn_defect(const GrpIn &c, const int32_t *index, const float *dist2, const float *offset) {
  return grp_defect(c, index, dist2, offset, nullptr);
}

inline GrpDefect grp_normals_defect(const GrpIn &c, const double *view, const float *normals, const float *curvature) {
  return grp_defect(c, normals, curvature, nullptr, view);
}

inline int grp_status(GrpDefect d) { return d == kGrpGood || d == kGrpNoop ? TSDF_OK : TSDF_ERR_INVALID_ARG; }
