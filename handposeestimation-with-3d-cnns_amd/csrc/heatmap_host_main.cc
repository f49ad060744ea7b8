// heatmap_host_main.cc — heatmap_host.inc (the text tsdf_heatmap.hip compiles) as a stand-alone host program that checks
// itself: make heatmap-host-asan builds it with g++ under -fsanitize=address,undefined, tests/test_heatmap_cpu.py runs it.
//   * the plan, for every R in 4..128 step 4, every n * J in 1..700 and 1, 8, 256 and 304 CUs: every slice lies in exactly
//     one slab, no slab is empty, only the last one is short, and the workgroup count is the rule's — n * J when that is
//     2 * CUs or more, otherwise the largest n * J * nslab that slabs of equal size reach without passing 2 * CUs
//     (n * J itself when even one more slab would pass it, n * J * R when a slice per slab stays below it);
//   * the item arithmetic, for every R and both item widths: every item of a whole volume maps to the row and column a
//     division gives; heat_div is a division for EVERY numerator below 2^20 (an item number is below 2^19) and every
//     divisor 1..128, and on every 997th numerator from there to 2^24, where heatmap_host.inc's inequality is the proof;
//   * the argument rules of both entries: every defect alone is reported as itself, and of two defects the one earlier
//     in the header's order is reported, n == 0 before everything.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/tsdf_heatmap.h"

// The three tests heatmap_host.inc takes from its includer, as device.inc and narrow.inc (which need HIP) state them, line
// for line: tests/test_heatmap_cpu.py compares these lines with those files.
bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
[[maybe_unused]] bool bad_res(int R) { return R < 4 || R > 128 || R % 4 != 0; }
bool bad_dtype(int dtype) { return dtype != TSDF_LOWP_F16 && dtype != TSDF_LOWP_BF16; }

#include "heatmap_host.inc"

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

static void check_plan(int64_t units, int R, int cus) {
  const HeatPlan p = heat_plan(units, R, cus);
  CHECK(p.slab >= 1 && p.slab <= R && p.nslab >= 1 && p.nslab <= R, "units %ld R %d cus %d: slab %d nslab %d", (long)units, R,
        cus, p.slab, p.nslab);
  if (p.slab < 1 || p.nslab < 1 || p.nslab > R) return;
  std::vector<int> seen(R, 0);
  for (int s = 0; s < p.nslab; ++s) {   // the kernel's own bounds
    const int sb = s * p.slab, se = sb + p.slab < R ? sb + p.slab : R;
    CHECK(se > sb, "units %ld R %d cus %d: slab %d is empty", (long)units, R, cus, s);
    if (s + 1 < p.nslab) CHECK(se - sb == p.slab, "units %ld R %d cus %d: slab %d is short", (long)units, R, cus, s);
    for (int z = sb; z < se; ++z) ++seen[z];
  }
  for (int z = 0; z < R; ++z) CHECK(seen[z] == 1, "units %ld R %d cus %d: slice %d in %d slabs", (long)units, R, cus, z, seen[z]);
  CHECK(p.blocks == units * p.nslab, "units %ld R %d cus %d: blocks %ld", (long)units, R, cus, (long)p.blocks);
  // the rule
  const int64_t target = 2 * (int64_t)cus;
  if (units >= target) {
    CHECK(p.nslab == 1 && p.slab == R, "units %ld R %d cus %d: %d slabs", (long)units, R, cus, p.nslab);
    return;
  }
  CHECK(p.blocks <= target, "units %ld R %d cus %d: %ld workgroups", (long)units, R, cus, (long)p.blocks);
  // no smaller slab size (more workgroups) stays within the target, a slice per slab being the limit
  if (p.slab > 1) {
    const int finer = (R + p.slab - 2) / (p.slab - 1);
    CHECK(units * finer > target, "units %ld R %d cus %d: slabs of %d slices would do", (long)units, R, cus, p.slab - 1);
  }
}

static void check_items(int R, int V) {
  const int RV = R / V;
  const unsigned mrv = heat_magic(RV), mr = heat_magic(R);
  const unsigned nit = (unsigned)(R * R * RV);
  std::vector<unsigned char> seen((size_t)R * R * RV, 0);
  for (unsigned item = 0; item < nit; ++item) {
    const HeatItem it = heat_item(item, R, RV, V, mrv, mr);
    const int fast = (int)(item % RV) * V, mid = (int)(item / RV) % R, slice = (int)(item / RV) / R;
    CHECK(it.fast == fast && it.mid == mid && it.slice == slice, "R %d V %d item %u: (%d, %d, %d)", R, V, item, it.slice, it.mid,
          it.fast);
    if (it.slice >= 0 && it.slice < R && it.mid >= 0 && it.mid < R && it.fast >= 0 && it.fast + V <= R)
      ++seen[((size_t)it.slice * R + it.mid) * RV + it.fast / V];
  }
  for (size_t k = 0; k < seen.size(); ++k) CHECK(seen[k] == 1, "R %d V %d: piece %zu written %d times", R, V, k, seen[k]);
}

static long check_div() {
  long cases = 0;
  for (int d = 1; d <= 128; ++d) {
    const unsigned m = heat_magic(d);
    for (unsigned x = 0; x < (1u << 24); x += (x < (1u << 20) ? 1u : 997u), ++cases)
      CHECK(heat_div(x, m) == x / (unsigned)d, "%u / %d", x, d);
    CHECK(heat_div((1u << 24) - 1, m) == ((1u << 24) - 1) / (unsigned)d, "2^24 - 1 over %d", d);
  }
  return cases;
}

// One argument set per rule that breaks it and nothing else, in the order of the rules; `good` breaks none.
struct EncArgs {
  const float *u;
  const int32_t *status;
  int n, J, R;
  float sigma;
  int layout, dtype;
  const void *out;
  const int32_t *valid;
};
struct DecArgs {
  const void *heat;
  int dtype, n, J, R, layout, radius;
  const float *u, *peak;
  const int32_t *arg;
};
static HeatDefect enc(const EncArgs &a) {
  return heat_defect_encode(a.u, a.status, a.n, a.J, a.R, a.sigma, a.layout, a.dtype, a.out, a.valid);
}
static HeatDefect dec(const DecArgs &a) {
  return heat_defect_decode(a.heat, a.dtype, a.n, a.J, a.R, a.layout, a.radius, a.u, a.peak, a.arg);
}

template <typename P>
static const P *at(uintptr_t v) {
  return reinterpret_cast<const P *>(v);
}

static void check_rules() {
  const float inf = 1.0f / 0.0f, nan = inf - inf;
  const EncArgs good = {at<float>(64), at<int32_t>(64), 3, 21, 32, 1.7f, 0, 0, at<void>(64), at<int32_t>(64)};
  CHECK(enc(good) == kHeatGood, "encode: good arguments");
  // rule k of the order breaks with edit k; each edit touches fields no other edit touches but the scalar ones
  typedef void (*EncEdit)(EncArgs &);
  const EncEdit enc_edits[] = {
      [](EncArgs &a) { a.n = 0; },  [](EncArgs &a) { a.n = -1; },        [](EncArgs &a) { a.R = 30; },
      [](EncArgs &a) { a.J = 171; }, [](EncArgs &a) { a.layout = 2; },    [](EncArgs &a) { a.dtype = 3; },
      [](EncArgs &a) { a.sigma = 0.f; }, [](EncArgs &a) { a.u = nullptr; }, [](EncArgs &a) { a.out = at<void>(72); },
  };
  const HeatDefect order[] = {kHeatNoop,     kHeatBadN,      kHeatBadRes, kHeatBadJoints, kHeatBadLayout,
                              kHeatBadDtype, kHeatBadScalar, kHeatNull,   kHeatUnaligned};
  const int n_rules = (int)(sizeof(order) / sizeof(order[0]));
  for (int i = 0; i < n_rules; ++i) {
    EncArgs a = good;
    enc_edits[i](a);
    CHECK(enc(a) == order[i], "encode: rule %d alone gives %d", i, (int)enc(a));
    CHECK(heat_status(enc(a)) == (i == 0 ? TSDF_OK : TSDF_ERR_INVALID_ARG), "encode: rule %d status", i);
    for (int j = i + 1; j < n_rules; ++j) {
      if (i < 2 && j < 2) continue;   // n == 0 and n < 0 are one field
      EncArgs b = a;
      enc_edits[j](b);
      CHECK(enc(b) == order[i], "encode: rules %d and %d give %d", i, j, (int)enc(b));
    }
  }
  typedef void (*DecEdit)(DecArgs &);
  const DecArgs dgood = {at<void>(64), 2, 3, 21, 32, 1, 2, at<float>(64), at<float>(64), at<int32_t>(64)};
  CHECK(dec(dgood) == kHeatGood, "decode: good arguments");
  const DecEdit dec_edits[] = {
      [](DecArgs &a) { a.n = 0; },   [](DecArgs &a) { a.n = -1; },       [](DecArgs &a) { a.R = 132; },
      [](DecArgs &a) { a.J = 0; },   [](DecArgs &a) { a.layout = -1; },  [](DecArgs &a) { a.dtype = -1; },
      [](DecArgs &a) { a.radius = 4; }, [](DecArgs &a) { a.heat = nullptr; }, [](DecArgs &a) { a.u = at<float>(66); },
  };
  for (int i = 0; i < n_rules; ++i) {
    DecArgs a = dgood;
    dec_edits[i](a);
    CHECK(dec(a) == order[i], "decode: rule %d alone gives %d", i, (int)dec(a));
    for (int j = i + 1; j < n_rules; ++j) {
      if (i < 2 && j < 2) continue;
      DecArgs b = a;
      dec_edits[j](b);
      CHECK(dec(b) == order[i], "decode: rules %d and %d give %d", i, j, (int)dec(b));
    }
  }
  // the values of each rule
  for (int R = -8; R <= 260; ++R) {
    EncArgs a = good;
    a.R = R;
    CHECK((enc(a) == kHeatGood) == (R >= 4 && R <= 128 && R % 4 == 0), "R %d", R);
  }
  for (int J = -1; J <= 200; ++J) {
    DecArgs a = dgood;
    a.J = J;
    CHECK((dec(a) == kHeatGood) == (J >= 1 && J <= 170), "J %d", J);
  }
  for (float s : {-1.f, -0.f, 0.f, nan, inf, -inf}) {
    EncArgs a = good;
    a.sigma = s;
    CHECK(enc(a) == kHeatBadScalar, "sigma %g", (double)s);
  }
  for (float s : {1e-38f, 0.5f, 1.7f, 3e38f}) {
    EncArgs a = good;
    a.sigma = s;
    CHECK(enc(a) == kHeatGood, "sigma %g", (double)s);
  }
  for (int r = -2; r <= 6; ++r) {
    DecArgs a = dgood;
    a.radius = r;
    CHECK((dec(a) == kHeatGood) == (r >= 0 && r <= 3), "radius %d", r);
  }
  for (int dt = -1; dt <= 4; ++dt) {
    EncArgs a = good;
    a.dtype = dt;
    CHECK((enc(a) == kHeatGood) == (dt >= 0 && dt <= 2), "dtype %d", dt);
  }
  {   // the optional pointers, the alignments and the launch's size
    EncArgs a = good;
    a.status = nullptr, a.valid = nullptr;
    CHECK(enc(a) == kHeatGood, "encode: optional pointers");
    a = good, a.out = nullptr;
    CHECK(enc(a) == kHeatNull, "encode: no output");
    a = good, a.u = at<float>(66);
    CHECK(enc(a) == kHeatUnaligned, "encode: u");
    a = good, a.status = at<int32_t>(65);
    CHECK(enc(a) == kHeatUnaligned, "encode: status");
    a = good, a.valid = at<int32_t>(70);
    CHECK(enc(a) == kHeatUnaligned, "encode: valid");
    a = good, a.out = at<void>(80);
    CHECK(enc(a) == kHeatGood, "encode: 16-byte aligned output");
    a = good, a.n = 98690, a.J = 170;   // 16,777,300 pairs
    CHECK(enc(a) == kHeatTooMany, "encode: too many");
    a.n = 98688;                         // 16,776,960
    CHECK(enc(a) == kHeatGood, "encode: just few enough");
    DecArgs d = dgood;
    d.peak = nullptr, d.arg = nullptr;
    CHECK(dec(d) == kHeatGood, "decode: optional pointers");
    d = dgood, d.u = nullptr;
    CHECK(dec(d) == kHeatNull, "decode: no output");
    d = dgood, d.heat = at<void>(72);
    CHECK(dec(d) == kHeatUnaligned, "decode: heat");
    d = dgood, d.peak = at<float>(66);
    CHECK(dec(d) == kHeatUnaligned, "decode: peak");
    d = dgood, d.arg = at<int32_t>(66);
    CHECK(dec(d) == kHeatUnaligned, "decode: arg");
    d = dgood, d.n = 1 << 24, d.J = 1;
    CHECK(dec(d) == kHeatTooMany, "decode: too many");
  }
}

int main() {
  long plans = 0;
  for (int R = 4; R <= 128; R += 4)
    for (int64_t units = 1; units <= 700; ++units)
      for (int cus : {1, 8, 256, 304}) {
        check_plan(units, R, cus);
        ++plans;
      }
  for (int R = 4; R <= 128; R += 4) {
    check_items(R, 4);
    if (R % 8 == 0) check_items(R, 8);
  }
  check_div();
  check_rules();
  if (g_fail) {
    printf("heatmap: %d checks FAILED\n", g_fail);
    return 1;
  }
  printf("heatmap host code ok (%ld plans)\n", plans);
  return 0;
}
