// pointfield_host.inc — the host side of libtsdf_pointfield.so that needs no device: the plan and the argument rules of
// its two entries.  Plain C++: tsdf_pointfield.hip includes it (inside its anonymous namespace, after
// include/tsdf_pointfield.h), and pointfield_host_main.cc includes it into a stand-alone program built under the CPU
// sanitizers (make pointfield-host-asan; tests/test_pointfield_cpu.py runs it).
//   pf_plan           the LDS bytes, the joints per workgroup and the workgroups per position
//   pf_padded         the cloud's rows rounded up to whole waves: the extent of each LDS array
//   pf_encode_defect  the first argument rule tsdf_pointfield_encode_hip's arguments break, in the header's order
//   pf_decode_defect  the same for tsdf_pointfield_decode_hip
// misaligned (device.inc) must be declared before this file is included — the library has it from that file, the
// stand-alone program carries its text.

constexpr int kPfWG = 256;                       // threads per workgroup
constexpr int kPfWaves = kPfWG / 64;
constexpr int kPfPerWave = 1;                    // joints a wave serves, one after the other
constexpr int kPfJoints = kPfWaves * kPfPerWave; // joints per workgroup
constexpr int kPfTailBytes = 16;                 // the waves' candidate counts, behind the three coordinate arrays
constexpr int kPfRegSlots = 16;                  // a lane keeps its keys in registers for clouds of up to 64 * this rows
constexpr int64_t kPfMaxItems = (int64_t)1 << 32;   // work-items of one launch
static_assert(TSDF_POINTFIELD_MAX_CLOUD % 64 == 0 && 12 * TSDF_POINTFIELD_MAX_CLOUD + kPfTailBytes <= 160 * 1024, "the LDS budget");
static_assert(kPfWaves * 4 <= kPfTailBytes, "one count per wave");

// P rounded up to whole waves; P in 1..TSDF_POINTFIELD_MAX_CLOUD
constexpr int pf_padded(int P) { return (P + 63) / 64 * 64; }

struct PfPlan {
  int lds_bytes, joints, groups;
};

// P in 1..TSDF_POINTFIELD_MAX_CLOUD, J >= 1
inline PfPlan pf_plan(int P, int J) {
  return {12 * pf_padded(P) + kPfTailBytes, kPfJoints, (int)(((int64_t)J + kPfJoints - 1) / kPfJoints)};
}

// The rules in the order they are judged; an entry returns TSDF_OK for kPfNoop, TSDF_ERR_INVALID_ARG for any other
// value but kPfGood.
enum PfDefect {
  kPfGood = 0,
  kPfBadN,        // n < 0
  kPfBadP,        // P outside 1..TSDF_POINTFIELD_MAX_CLOUD
  kPfBadJ,        // J outside 1..TSDF_POINTFIELD_MAX_JOINTS
  kPfBadK,        // K outside 1..TSDF_POINTFIELD_MAX_K (encode), M outside 1..TSDF_POINTFIELD_MAX_VOTES (decode)
  kPfBadPitch,    // pitch < P
  kPfBadRadius,   // not finite, or not > 0
  kPfBadLayout,
  kPfBadDtype,
  kPfNoop,        // n == 0: nothing to do, whatever else is passed
  kPfNull,        // a required pointer is NULL
  kPfUnaligned,
  kPfTooMany      // n * groups * kPfWG >= 2^32
};

// what the two entries share
struct PfIn {
  const float *points;
  int64_t pitch;
  int n, P, J, K;   // K: encode's K or decode's M
  double radius;
  int layout, dtype;
  const int32_t *status;   // the OUTPUT status
};

inline PfDefect pf_shape_defect(int P, int J, int K, int most_k) {
  if (P < 1 || P > TSDF_POINTFIELD_MAX_CLOUD) return kPfBadP;
  if (J < 1 || J > TSDF_POINTFIELD_MAX_JOINTS) return kPfBadJ;
  if (K < 1 || K > most_k) return kPfBadK;
  return kPfGood;
}

// bytes of a field element; dtype is 0, 1 or 2
constexpr int pf_elem(int dtype) { return dtype == TSDF_POINTFIELD_F32 ? 4 : 2; }

// `most_k`: the entry's cap on K; `field`: the field pointer (either direction); f4a / f4b: the entry's two other
// required float32 / int32 pointers (joints and valid; out_joints and out_weight)
inline PfDefect pf_defect(const PfIn &c, int most_k, const void *field, const void *f4a, const void *f4b) {
  if (c.n < 0) return kPfBadN;
  const PfDefect shape = pf_shape_defect(c.P, c.J, c.K, most_k);
  if (shape != kPfGood) return shape;
  if (c.pitch < c.P) return kPfBadPitch;
  if (!(c.radius > 0.0) || !(c.radius < __builtin_inf())) return kPfBadRadius;   // a NaN fails the first test
  if (c.layout != TSDF_POINTFIELD_CP && c.layout != TSDF_POINTFIELD_PC) return kPfBadLayout;
  if (c.dtype != TSDF_POINTFIELD_F32 && c.dtype != TSDF_POINTFIELD_F16 && c.dtype != TSDF_POINTFIELD_BF16) return kPfBadDtype;
  if (c.n == 0) return kPfNoop;
  if (!c.points || !field || !f4a || !f4b || !c.status) return kPfNull;
  if (misaligned(c.points, 3) || misaligned(f4a, 3) || misaligned(f4b, 3) || misaligned(field, (uintptr_t)pf_elem(c.dtype) - 1))
    return kPfUnaligned;
  if ((int64_t)c.n * pf_plan(c.P, c.J).groups * kPfWG >= kPfMaxItems) return kPfTooMany;
  return kPfGood;
}

inline PfDefect pf_encode_defect(const PfIn &c, const float *joints, const void *field, const int32_t *valid) {
  return pf_defect(c, TSDF_POINTFIELD_MAX_K, field, joints, valid);
}

inline PfDefect pf_decode_defect(const PfIn &c, const void *field, const float *joints, const float *weight) {
  return pf_defect(c, TSDF_POINTFIELD_MAX_VOTES, field, joints, weight);
}

inline int pf_status(PfDefect d) { return d == kPfGood || d == kPfNoop ? TSDF_OK : TSDF_ERR_INVALID_ARG; }
