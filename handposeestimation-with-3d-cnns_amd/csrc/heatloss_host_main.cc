// heatloss_host_main.cc — heatloss_host.inc (the text tsdf_heatloss.hip compiles, on top of heatmap_host.inc) as a
// stand-alone host program that checks itself: make heatloss-host-asan builds it with g++ under
// -fsanitize=address,undefined, tests/test_heatloss_cpu.py runs it.
//   * the quad arithmetic of the forward kernels, for every R in 4..128 step 4: every quad of a whole volume maps to the
//     slice, row and column a division gives, and the walk the kernels make — pieces of 4 elements, and pieces of 8 split
//     into two quads, for every lane of a workgroup in the kernels' own loop — meets every element of the volume exactly
//     once and never leaves it, also where an 8-element piece straddles two rows (R % 8 != 0);
//   * the gradient kernels' walk, heat_plan and heat_item as those kernels use them, for 1, 8, 256 and 304 CUs and a few
//     unit counts: every element of a volume is written exactly once;
//   * the argument rules of the four entries: every defect alone is reported as itself, and of two defects the one earlier
//     in the header's order is reported, n == 0 before everything; the values of the scalar rule; the optional pointers
//     and every alignment.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/tsdf_heatloss.h"

// The three tests heatmap_host.inc takes from its includer, as device.inc and narrow.inc (which need HIP) state them, line
// for line: tests/test_heatloss_cpu.py compares these lines with those files.
bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
[[maybe_unused]] bool bad_res(int R) { return R < 4 || R > 128 || R % 4 != 0; }
bool bad_dtype(int dtype) { return dtype != TSDF_LOWP_F16 && dtype != TSDF_LOWP_BF16; }

#include "heatmap_host.inc"
#include "heatloss_host.inc"

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

// the forward kernels' loop over a volume of pieces of E elements, lane by lane
static long check_quads(int R, int E) {
  const int R3 = R * R * R, nvec = R3 / E, kWG = 256, kDepth = 4;
  const unsigned mrq = heat_magic(R / 4), mr = heat_magic(R);
  std::vector<unsigned char> seen((size_t)R3, 0);
  long quads = 0;
  for (int tid = 0; tid < kWG; ++tid)
    for (int v0 = tid; v0 < nvec; v0 += kDepth * kWG)
      for (int k = 0; k < kDepth; ++k) {
        const int vi = v0 + k * kWG;
        if (vi >= nvec) break;
        for (int h = 0; h < E / 4; ++h, ++quads) {
          const unsigned q = (unsigned)(vi * (E / 4) + h);
          const HeatQuad c = heat_quad(q, R, mrq, mr);
          const int fast = (int)(q % (unsigned)(R / 4)) * 4, mid = (int)(q / (unsigned)(R / 4)) % R, slow = (int)(q / (unsigned)(R / 4)) / R;
          CHECK(c.fast == fast && c.mid == mid && c.slow == slow, "R %d E %d quad %u: (%d, %d, %d)", R, E, q, c.slow, c.mid, c.fast);
          if (c.slow < 0 || c.slow >= R || c.mid < 0 || c.mid >= R || c.fast < 0 || c.fast + 4 > R) continue;
          const size_t e = ((size_t)c.slow * R + c.mid) * R + c.fast;
          CHECK(e == (size_t)vi * E + 4 * h, "R %d E %d piece %d half %d is element %zu", R, E, vi, h, e);
          for (int j = 0; j < 4; ++j) ++seen[e + j];
        }
      }
  for (size_t e = 0; e < seen.size(); ++e) CHECK(seen[e] == 1, "R %d E %d: element %zu read %d times", R, E, e, seen[e]);
  return quads;
}

// the gradient kernels' loop over one unit's volume: slabs of the plan, items of V voxels
static void check_grad_walk(int64_t units, int R, int V, int cus) {
  const HeatPlan p = heat_plan(units, R, cus);
  const int RV = R / V, kWG = 256;
  const unsigned mrv = heat_magic(RV), mr = heat_magic(R);
  std::vector<unsigned char> seen((size_t)R * R * R, 0);
  for (int s = 0; s < p.nslab; ++s) {
    const int sb = s * p.slab, se = sb + p.slab < R ? sb + p.slab : R;
    const unsigned nit = (unsigned)((se - sb) * R * RV);
    for (int tid = 0; tid < kWG; ++tid)
      for (unsigned item = (unsigned)tid; item < nit; item += kWG) {
        const HeatItem it = heat_item(item, R, RV, V, mrv, mr);
        const int sl = sb + it.slice;
        if (sl < 0 || sl >= R || it.mid < 0 || it.mid >= R || it.fast < 0 || it.fast + V > R) {
          CHECK(false, "units %ld R %d V %d cus %d: item %u of slab %d leaves the volume", (long)units, R, V, cus, item, s);
          continue;
        }
        const size_t e = ((size_t)sl * R + it.mid) * R + it.fast;
        for (int j = 0; j < V; ++j) ++seen[e + j];
      }
  }
  for (size_t e = 0; e < seen.size(); ++e)
    CHECK(seen[e] == 1, "units %ld R %d V %d cus %d: element %zu written %d times", (long)units, R, V, cus, e, seen[e]);
}

// One argument set per entry; `good` breaks no rule.
struct Args {
  const void *vol;       // pred / heat
  int dtype;
  const float *u;        // labels (loss), out_u (soft-argmax), grad_u (its gradient)
  const int32_t *status;
  const float *w;
  const double *dbl;     // out_sse / out_stats / stats
  const int32_t *valid;
  const void *out;       // out_grad
  int n, J, R;
  float scalar;          // sigma / beta
  int layout;
};
typedef HeatDefect (*Entry)(const Args &);
static HeatDefect sse(const Args &a) {
  return heat_defect_sse(a.vol, a.dtype, a.u, a.status, a.n, a.J, a.R, a.scalar, a.layout, a.dbl, a.valid);
}
static HeatDefect sse_grad(const Args &a) {
  return heat_defect_sse_grad(a.vol, a.dtype, a.u, a.status, a.w, a.n, a.J, a.R, a.scalar, a.layout, a.out);
}
static HeatDefect soft(const Args &a) { return heat_defect_soft_argmax(a.vol, a.dtype, a.n, a.J, a.R, a.scalar, a.layout, a.u, a.dbl); }
static HeatDefect soft_grad(const Args &a) {
  return heat_defect_soft_argmax_grad(a.vol, a.dtype, a.dbl, a.u, a.n, a.J, a.R, a.scalar, a.layout, a.out);
}

template <typename P>
static const P *at(uintptr_t v) {
  return reinterpret_cast<const P *>(v);
}

static void check_rules() {
  const float inf = 1.0f / 0.0f, nan = inf - inf;
  const Args good = {at<void>(64), 2, at<float>(64), at<int32_t>(64), at<float>(64), at<double>(64), at<int32_t>(64), at<void>(64),
                     3,            21, 32,           1.7f,             0};
  const Entry entries[] = {sse, sse_grad, soft, soft_grad};
  const char *names[] = {"sse", "sse_grad", "soft_argmax", "soft_argmax_grad"};
  // rule k of the order breaks with edit k; each edit touches fields no other edit touches (n apart)
  typedef void (*Edit)(Args &);
  const Edit edits[] = {
      [](Args &a) { a.n = 0; },      [](Args &a) { a.n = -1; },          [](Args &a) { a.R = 30; },
      [](Args &a) { a.J = 171; },    [](Args &a) { a.layout = 2; },      [](Args &a) { a.dtype = 3; },
      [](Args &a) { a.scalar = 0.f; }, [](Args &a) { a.u = nullptr; },   [](Args &a) { a.vol = at<void>(72); },
  };
  const HeatDefect order[] = {kHeatNoop,     kHeatBadN,      kHeatBadRes, kHeatBadJoints, kHeatBadLayout,
                              kHeatBadDtype, kHeatBadScalar, kHeatNull,   kHeatUnaligned};
  const int n_rules = (int)(sizeof(order) / sizeof(order[0]));
  for (int f = 0; f < 4; ++f) {
    const Entry fn = entries[f];
    CHECK(fn(good) == kHeatGood, "%s: good arguments", names[f]);
    for (int i = 0; i < n_rules; ++i) {
      Args a = good;
      edits[i](a);
      CHECK(fn(a) == order[i], "%s: rule %d alone gives %d", names[f], i, (int)fn(a));
      CHECK(heat_status(fn(a)) == (i == 0 ? TSDF_OK : TSDF_ERR_INVALID_ARG), "%s: rule %d status", names[f], i);
      for (int j = i + 1; j < n_rules; ++j) {
        if (i < 2 && j < 2) continue;   // n == 0 and n < 0 are one field
        Args b = a;
        edits[j](b);
        CHECK(fn(b) == order[i], "%s: rules %d and %d give %d", names[f], i, j, (int)fn(b));
      }
      // and the last rule after every other one
      if (i >= 2) {
        Args b = a;
        b.n = 1 << 24;
        CHECK(fn(b) == order[i], "%s: rule %d and too many give %d", names[f], i, (int)fn(b));
      }
    }
    Args a = good;
    a.n = 1 << 24, a.J = 1;
    CHECK(fn(a) == kHeatTooMany, "%s: too many", names[f]);
    a = good, a.n = 98690, a.J = 170;   // 16,777,300 pairs
    CHECK(fn(a) == kHeatTooMany, "%s: too many", names[f]);
    a.n = 98688;                         // 16,776,960
    CHECK(fn(a) == kHeatGood, "%s: just few enough", names[f]);
    // the values of each rule
    for (int R = -8; R <= 260; ++R) {
      a = good, a.R = R;
      CHECK((fn(a) == kHeatGood) == (R >= 4 && R <= 128 && R % 4 == 0), "%s: R %d", names[f], R);
    }
    for (int J = -1; J <= 200; ++J) {
      a = good, a.J = J;
      CHECK((fn(a) == kHeatGood) == (J >= 1 && J <= 170), "%s: J %d", names[f], J);
    }
    for (int dt = -1; dt <= 4; ++dt) {
      a = good, a.dtype = dt;
      CHECK((fn(a) == kHeatGood) == (dt >= 0 && dt <= 2), "%s: dtype %d", names[f], dt);
    }
    for (float s : {-1.f, -0.f, 0.f, nan, inf, -inf}) {
      a = good, a.scalar = s;
      CHECK(fn(a) == kHeatBadScalar, "%s: scalar %g", names[f], (double)s);
    }
    for (float s : {1e-38f, 0.5f, 1.7f, 8.f, 3e38f}) {
      a = good, a.scalar = s;
      CHECK(fn(a) == kHeatGood, "%s: scalar %g", names[f], (double)s);
    }
    // 16-byte volumes, 8-byte doubles
    a = good, a.vol = at<void>(80);
    CHECK(fn(a) == kHeatGood, "%s: 16-byte aligned volume", names[f]);
    a = good, a.vol = nullptr;
    CHECK(fn(a) == kHeatNull, "%s: no volume", names[f]);
    a = good, a.u = at<float>(66);
    CHECK(fn(a) == kHeatUnaligned, "%s: u", names[f]);
  }
  {   // the pointers each entry has of its own
    Args a = good;
    a.status = nullptr, a.valid = nullptr;
    CHECK(sse(a) == kHeatGood && sse_grad(a) == kHeatGood, "loss: optional pointers");
    a = good, a.dbl = nullptr;
    CHECK(sse(a) == kHeatNull && soft(a) == kHeatNull && soft_grad(a) == kHeatNull && sse_grad(a) == kHeatGood, "no doubles");
    a = good, a.dbl = at<double>(68);
    CHECK(sse(a) == kHeatUnaligned && soft(a) == kHeatUnaligned && soft_grad(a) == kHeatUnaligned, "doubles off 8 bytes");
    a = good, a.dbl = at<double>(72);
    CHECK(sse(a) == kHeatGood && soft(a) == kHeatGood && soft_grad(a) == kHeatGood, "doubles on 8 bytes");
    a = good, a.out = nullptr;
    CHECK(sse_grad(a) == kHeatNull && soft_grad(a) == kHeatNull && sse(a) == kHeatGood && soft(a) == kHeatGood, "no gradient");
    a = good, a.out = at<void>(72);
    CHECK(sse_grad(a) == kHeatUnaligned && soft_grad(a) == kHeatUnaligned, "gradient off 16 bytes");
    a = good, a.out = a.vol;
    CHECK(sse_grad(a) == kHeatGood && soft_grad(a) == kHeatGood, "in place");
    a = good, a.w = nullptr;
    CHECK(sse_grad(a) == kHeatNull && sse(a) == kHeatGood, "no w");
    a = good, a.w = at<float>(65);
    CHECK(sse_grad(a) == kHeatUnaligned, "w");
    a = good, a.status = at<int32_t>(65);
    CHECK(sse(a) == kHeatUnaligned && sse_grad(a) == kHeatUnaligned && soft(a) == kHeatGood, "status");
    a = good, a.valid = at<int32_t>(70);
    CHECK(sse(a) == kHeatUnaligned && sse_grad(a) == kHeatGood, "valid");
  }
}

int main() {
  long quads = 0;
  for (int R = 4; R <= 128; R += 4) {
    quads += check_quads(R, 4);
    quads += check_quads(R, 8);
  }
  for (int R : {4, 8, 12, 20, 32, 44, 64, 128})
    for (int64_t units : {1, 2, 63, 85, 340, 700})
      for (int cus : {1, 8, 256, 304}) {
        if (R == 128 && units > 2) continue;
        check_grad_walk(units, R, 4, cus);
        if (R % 8 == 0) check_grad_walk(units, R, 8, cus);
      }
  check_rules();
  if (g_fail) {
    printf("heatloss: %d checks FAILED\n", g_fail);
    return 1;
  }
  printf("heatloss host code ok (%ld quads)\n", quads);
  return 0;
}
