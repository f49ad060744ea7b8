// patch_host_main.cc — patch_host.inc (the text tsdf_patch.hip compiles) as a stand-alone host program that checks itself:
// make patch-host-asan builds it with g++ under -fsanitize=address,undefined, tests/test_patch_cpu.py runs it.
//   * the plan, for every S and every dtype: a lane's pixels are one 16-byte store, the lanes of a band fit the workgroup,
//     every (row, column) of the patch belongs to exactly one (item, lane, pixel) — walked with the kernel's own
//     expressions —, and no band but the last is short; the workgroups of a launch cover the items or stop at the cap;
//   * the argument rules of the four entries: every defect alone is reported as itself, and of two defects the one earlier
//     in the header's order is reported.
#include <stdint.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "../../include/tsdf_patch.h"

// The two tests patch_host.inc takes from its includer, as device.inc and narrow.inc (which need HIP) state them, line for
// line: tests/test_patch_cpu.py compares these lines with those files.  cam_ok is prim.inc's own text.
bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
bool bad_dtype(int dtype) { return dtype != TSDF_LOWP_F16 && dtype != TSDF_LOWP_BF16; }
#define TSDF_PRIM_HOST_ONLY
#include "prim.inc"

#include "patch_host.inc"

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
  for (int S = TSDF_PATCH_MIN_SIZE; S <= TSDF_PATCH_MAX_SIZE; S += 8) {
    for (int dtype : {TSDF_PATCH_F32, (int)TSDF_LOWP_F16, (int)TSDF_LOWP_BF16}) {
      const PatchPlan p = patch_plan(S, dtype);
      ++cases;
      CHECK(p.px * patch_elem(dtype) == 16 && p.px == (dtype == TSDF_PATCH_F32 ? 4 : 8), "S %d dtype %d: %d pixels a lane", S, dtype, p.px);
      CHECK(p.lanes_per_row * p.px == S && p.rows >= 1 && p.rows <= S && p.rows * p.lanes_per_row <= kPatchWG,
            "S %d dtype %d: %d lanes a row, %d rows", S, dtype, p.lanes_per_row, p.rows);
      CHECK(p.rows == S || (p.rows + 1) * p.lanes_per_row > kPatchWG, "S %d dtype %d: a band could hold another row", S, dtype);
      CHECK((int64_t)p.items * p.rows >= S && (int64_t)(p.items - 1) * p.rows < S, "S %d dtype %d: %d items", S, dtype, p.items);
      // the kernel's own walk: item (band), lane -> (row, first column)
      std::vector<unsigned char> seen((size_t)S * S, 0);
      for (int band = 0; band < p.items; ++band) {
        for (int tid = 0; tid < kPatchWG; ++tid) {
          const int r_in = tid / p.lanes_per_row, col0 = (tid - r_in * p.lanes_per_row) * p.px;
          const int row = band * p.rows + r_in;
          if (!(r_in < p.rows) || row >= S) continue;
          CHECK(col0 >= 0 && col0 + p.px <= S && ((int64_t)row * S + col0) * patch_elem(dtype) % 16 == 0, "S %d: lane %d leaves its row", S, tid);
          if (col0 + p.px > S) continue;
          for (int j = 0; j < p.px; ++j) ++seen[(size_t)row * S + col0 + j];
        }
      }
      bool once = true;
      for (unsigned char v : seen) once = once && v == 1;
      CHECK(once, "S %d dtype %d: a pixel is not written exactly once", S, dtype);
      for (int n : {1, 2, 4095, 4096, 4097, 70000, std::numeric_limits<int>::max()}) {
        const int64_t items = (int64_t)n * p.items;
        const unsigned g = patch_groups(n, p);
        CHECK(g >= 1 && g <= (unsigned)kPatchMaxGroups && (items <= kPatchMaxGroups ? g == items : g == (unsigned)kPatchMaxGroups),
              "S %d n %d: %u groups", S, n, g);
      }
    }
  }
  CHECK(patch_plan(128, TSDF_PATCH_F32).rows == 8 && patch_plan(128, TSDF_PATCH_F32).items == 16, "128^2 float32");
  CHECK(patch_plan(176, TSDF_LOWP_BF16).rows == 11 && patch_plan(176, TSDF_LOWP_BF16).items == 16, "176^2 bfloat16");
  CHECK(patch_plan(8, TSDF_PATCH_F32).rows == 8 && patch_plan(8, TSDF_PATCH_F32).items == 1, "8^2");
  CHECK(patch_plan(512, TSDF_PATCH_F32).rows == 2 && patch_plan(512, TSDF_PATCH_F32).items == 256, "512^2 float32");
  for (int S : {0, -8, 4, 12, 7, 520, 1024}) CHECK(patch_bad_size(S), "S %d passes", S);
  for (int d : {-1, 3}) CHECK(patch_bad_elem(d), "dtype %d passes", d);
  return cases;
}

struct Call {
  PatchCommon c;
  PatchOut o;
  const void *src;   // frames or depth
  int frame_type, shift;
  int64_t n_src, depth_len;
  int H, W;
  const int64_t *index, *offsets;
  const int32_t *headers;
  int J;
  const float *in, *out;
  const void *i4a, *i4b;
};

static PatchDefect frames(const Call &k) { return patch_frames_defect(k.c, k.o, k.src, k.frame_type, k.shift, k.n_src, k.H, k.W, k.index); }
static PatchDefect crops(const Call &k) {
  return patch_crops_defect(k.c, k.o, static_cast<const float *>(k.src), k.depth_len, k.offsets, k.headers, k.n_src, k.index);
}
static PatchDefect label(const Call &k) { return patch_label_defect(k.c, k.J, k.in, k.out, k.i4a, k.i4b); }

struct Bad {
  PatchDefect what;
  void (*make)(Call &);
  int entries;   // bit 0 frames, bit 1 crops, bit 2 the label entries
};

static long check_rules() {
  static const double nan = std::numeric_limits<double>::quiet_NaN();
  static const float inff = std::numeric_limits<float>::infinity(), nanf_ = std::numeric_limits<float>::quiet_NaN();
  const double *ok8 = reinterpret_cast<const double *>(64);
  const float *ok4 = reinterpret_cast<const float *>(64);
  const int32_t *st = reinterpret_cast<const int32_t *>(64);
  const int64_t *ix = reinterpret_cast<const int64_t *>(64);
  const Call good = {{ok8, 250.f, nullptr, nullptr, nullptr, 3, 241.42, 160.0, 120.0, 1.f, 3.f}, {128, 0, 0, ok4, st}, ok4,
                     TSDF_LOCATE_F32, 0, 3, 1000, 240, 320, nullptr, ix, st, 21, ok4, ok4, st, st};
  CHECK(frames(good) == kPatchGood && crops(good) == kPatchGood && label(good) == kPatchGood, "good");
  // the defects in the header's order, each as a change of the good call
  const Bad bads[] = {
      {kPatchBadN, [](Call &k) { k.c.n = -1; }, 7},
      {kPatchBadSize, [](Call &k) { k.o.S = 0; }, 3},
      {kPatchBadSize, [](Call &k) { k.o.S = 12; }, 3},
      {kPatchBadSize, [](Call &k) { k.o.S = 520; }, 3},
      {kPatchBadInterp, [](Call &k) { k.o.interp = 2; }, 3},
      {kPatchBadInterp, [](Call &k) { k.o.interp = -1; }, 3},
      {kPatchBadDtype, [](Call &k) { k.o.dtype = 3; }, 3},
      {kPatchBadDtype, [](Call &k) { k.o.dtype = -1; }, 3},
      {kPatchBadJ, [](Call &k) { k.J = 0; }, 4},
      {kPatchBadJ, [](Call &k) { k.J = TSDF_PATCH_MAX_JOINTS + 1; }, 4},
      {kPatchBadFrames, [](Call &k) { k.frame_type = 2; }, 1},
      {kPatchBadFrames, [](Call &k) { k.frame_type = TSDF_LOCATE_U16, k.shift = 8; }, 1},
      {kPatchBadFrames, [](Call &k) { k.frame_type = TSDF_LOCATE_U16, k.shift = -1; }, 1},
      {kPatchBadFrames, [](Call &k) { k.H = 0; }, 1},
      {kPatchBadFrames, [](Call &k) { k.W = -1; }, 1},
      {kPatchBadFrames, [](Call &k) { k.depth_len = -1; }, 2},
      {kPatchBadSrc, [](Call &k) { k.n_src = -1; }, 3},
      {kPatchBadCube, [](Call &k) { k.c.cube = 0.f, k.c.cube_n = nullptr; }, 7},
      {kPatchBadCube, [](Call &k) { k.c.cube = -1.f, k.c.cube_n = nullptr; }, 7},
      {kPatchBadCube, [](Call &k) { k.c.cube = inff, k.c.cube_n = nullptr; }, 7},
      {kPatchBadCube, [](Call &k) { k.c.cube = nanf_, k.c.cube_n = nullptr; }, 7},
      {kPatchBadCam, [](Call &k) { k.c.focal = 0.0; }, 7},
      {kPatchBadCam, [](Call &k) { k.c.focal = nan; }, 7},
      {kPatchBadCam, [](Call &k) { k.c.eps = 0.f; }, 7},
      {kPatchBadCam, [](Call &k) { k.c.trunc_vox = -1.f; }, 7},
      {kPatchNoop, [](Call &k) { k.c.n = 0; }, 7},
      {kPatchNoSource, [](Call &k) { k.n_src = 0, k.index = reinterpret_cast<const int64_t *>(64); }, 3},
      {kPatchNoSource, [](Call &k) { k.n_src = 4, k.index = nullptr; }, 3},
      {kPatchNull, [](Call &k) { k.src = nullptr; }, 3},
      {kPatchNull, [](Call &k) { k.offsets = nullptr; }, 2},
      {kPatchNull, [](Call &k) { k.headers = nullptr; }, 2},
      {kPatchNull, [](Call &k) { k.c.com = nullptr; }, 7},
      {kPatchNull, [](Call &k) { k.o.patch = nullptr; }, 3},
      {kPatchNull, [](Call &k) { k.o.status = nullptr; }, 3},
      {kPatchNull, [](Call &k) { k.in = nullptr; }, 4},
      {kPatchNull, [](Call &k) { k.out = nullptr; }, 4},
      {kPatchNull, [](Call &k) { k.i4a = nullptr; }, 4},
      {kPatchNull, [](Call &k) { k.i4b = nullptr; }, 4},
      {kPatchUnaligned, [](Call &k) { k.src = reinterpret_cast<const void *>(66); }, 3},
      {kPatchUnaligned, [](Call &k) { k.offsets = reinterpret_cast<const int64_t *>(68); }, 2},
      {kPatchUnaligned, [](Call &k) { k.headers = reinterpret_cast<const int32_t *>(66); }, 2},
      {kPatchUnaligned, [](Call &k) { k.c.com = reinterpret_cast<const double *>(68); }, 7},
      {kPatchUnaligned, [](Call &k) { k.c.affine = reinterpret_cast<const double *>(68); }, 7},
      {kPatchUnaligned, [](Call &k) { k.c.cube_n = reinterpret_cast<const float *>(66); }, 7},
      {kPatchUnaligned, [](Call &k) { k.c.status_in = reinterpret_cast<const int32_t *>(66); }, 7},
      {kPatchUnaligned, [](Call &k) { k.index = reinterpret_cast<const int64_t *>(68); }, 3},
      {kPatchUnaligned, [](Call &k) { k.o.patch = reinterpret_cast<const void *>(72); }, 3},
      {kPatchUnaligned, [](Call &k) { k.o.status = reinterpret_cast<const int32_t *>(66); }, 3},
      {kPatchUnaligned, [](Call &k) { k.in = reinterpret_cast<const float *>(66); }, 4},
      {kPatchUnaligned, [](Call &k) { k.out = reinterpret_cast<const float *>(66); }, 4},
      {kPatchUnaligned, [](Call &k) { k.i4a = reinterpret_cast<const void *>(66); }, 4},
      {kPatchTooMany, [](Call &k) { k.c.n = 1 << 20, k.J = 1 << 11; }, 4},
  };
  PatchDefect (*const judges[3])(const Call &) = {frames, crops, label};
  long cases = 0;
  const int count = (int)(sizeof bads / sizeof bads[0]);
  for (int e = 0; e < 3; ++e) {
    for (int i = 0; i < count; ++i) {
      if (!(bads[i].entries >> e & 1)) continue;
      Call one = good;
      bads[i].make(one);
      CHECK(judges[e](one) == bads[i].what, "entry %d: defect %d alone", e, i);
      ++cases;
      for (int j = i + 1; j < count; ++j) {
        if (!(bads[j].entries >> e & 1) || bads[j].what == bads[i].what) continue;
        Call two = good;
        bads[j].make(two);   // the later one first, so that the earlier one's change stands
        bads[i].make(two);
        CHECK(judges[e](two) == bads[i].what, "entry %d: defects %d and %d", e, i, j);
        ++cases;
      }
    }
  }
  // a per-position cube replaces the scalar; uint16 frames may sit on an even address; an index lifts n_src == n
  Call k = good;
  k.c.cube = 0.f, k.c.cube_n = ok4;
  CHECK(frames(k) == kPatchGood && crops(k) == kPatchGood && label(k) == kPatchGood, "d_cube replaces a bad scalar");
  k = good;
  k.frame_type = TSDF_LOCATE_U16, k.shift = 7, k.src = reinterpret_cast<const void *>(66);
  CHECK(frames(k) == kPatchGood, "uint16 frames at an even address");
  k.src = reinterpret_cast<const void *>(65);
  CHECK(frames(k) == kPatchUnaligned, "uint16 frames at an odd address");
  k = good;
  k.n_src = 1, k.index = ix;
  CHECK(frames(k) == kPatchGood && crops(k) == kPatchGood, "an index into one source");
  k = good;
  k.o.S = 512, k.o.interp = 1, k.o.dtype = TSDF_LOWP_BF16;
  CHECK(frames(k) == kPatchGood && crops(k) == kPatchGood, "the largest patch");
  k = good;
  k.c.n = 1 << 15, k.J = 65535;
  CHECK(label(k) == kPatchGood, "just below 2^31 joints");
  k.J = 65536;
  CHECK(label(k) == kPatchTooMany, "2^31 joints");
  CHECK(patch_status(kPatchGood) == TSDF_OK && patch_status(kPatchNoop) == TSDF_OK && patch_status(kPatchUnaligned) == TSDF_ERR_INVALID_ARG, "status");
  return cases;
}

int main() {
  const long plans = check_plan();
  const long rules = check_rules();
  if (g_fail) {
    printf("patch host code: %d checks FAILED\n", g_fail);
    return 1;
  }
  printf("patch host code ok (%d lanes, at most %d groups, S %d..%d, %ld plans, %ld rule cases)\n", kPatchWG, kPatchMaxGroups,
         TSDF_PATCH_MIN_SIZE, TSDF_PATCH_MAX_SIZE, plans, rules);
  return 0;
}
