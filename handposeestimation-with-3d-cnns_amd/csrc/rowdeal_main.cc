// rowdeal_main.cc — rowdeal.inc (the text tsdf_hip.hip compiles for the device) as a stand-alone host program that checks
// itself: make rowdeal-host-asan builds it with g++ under -fsanitize=address,undefined, tests/test_rowdeal_cpu.py runs it.
// For every frame height 1..260, kU in {3, 4}, the orders 0, 1 and 8 (rowdeal.inc) and 8 and 16 waves:
//   * the blocks cover every row exactly once, none leaves [0, bh), every block is one run of adjacent rows, only the
//     block that ends at the frame's end is shorter than kU (cut, not wrapped), and that one exists when kU does not
//     divide bh;
//   * every number the waves draw past the last block (each wave draws beyond the end before it stops) is empty and
//     maps to bh, the "no row" value the row loop stops on;
//   * the row loop itself, restated here with its two buffers and its draw two blocks ahead, reduces every row exactly
//     once under the drawn deal (waves advancing in a pseudo-random interleaving) and under the static block numbers
//     (wave + NW * i), and a wave whose buffer A is past the end never holds a block in B.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rowdeal.inc"

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

static void check_cover(int bh, int kU, int order, int nw) {
  const int nblk = rowdeal_blocks(bh, kU);
  CHECK(nblk == (bh + kU - 1) / kU && nblk >= 1, "bh %d kU %d", bh, kU);
  std::vector<int> seen(bh, 0);
  int n_cut = 0;
  for (int b = 0; b < nblk; ++b) {
    int n = -1;
    const int r0 = rowdeal_block(b, bh, kU, order, n);
    CHECK(n >= 1 && n <= kU, "bh %d kU %d order %d block %d: n %d", bh, kU, order, b, n);
    CHECK(r0 >= 0 && r0 + n <= bh, "bh %d kU %d order %d block %d: rows [%d, %d)", bh, kU, order, b, r0, r0 + n);
    CHECK(r0 % kU == 0, "bh %d kU %d order %d block %d starts at %d", bh, kU, order, b, r0);
    if (n < kU) {
      ++n_cut;
      CHECK(r0 + n == bh, "bh %d kU %d order %d block %d is short but ends at %d", bh, kU, order, b, r0 + n);
    }
    for (int r = r0; r < r0 + n && r >= 0 && r < bh; ++r) ++seen[r];
    if (order == kRowsTopDown) CHECK(r0 == b * kU, "bh %d kU %d block %d", bh, kU, b);
  }
  for (int r = 0; r < bh; ++r) CHECK(seen[r] == 1, "bh %d kU %d order %d row %d seen %d times", bh, kU, order, r, seen[r]);
  CHECK(n_cut == (bh % kU ? 1 : 0), "bh %d kU %d order %d: %d short blocks", bh, kU, order, n_cut);
  if (order == 1) {   // top, bottom, top, bottom ... towards the middle
    int n;
    for (int b = 0; b + 2 < nblk; ++b) {
      const int a = rowdeal_block(b, bh, kU, order, n), c = rowdeal_block(b + 2, bh, kU, order, n);
      CHECK((b & 1) ? c == a - kU : c == a + kU, "bh %d kU %d block %d -> %d", bh, kU, b, b + 2);
    }
    CHECK(rowdeal_block(0, bh, kU, order, n) == 0, "bh %d kU %d: block 0", bh, kU);
    if (nblk > 1) CHECK(rowdeal_block(1, bh, kU, order, n) == (nblk - 1) * kU, "bh %d kU %d: block 1", bh, kU);
  }
  for (int b = nblk; b < nblk + 4 * nw + 4; ++b) {   // what the waves draw past the end
    int n = -1;
    CHECK(rowdeal_block(b, bh, kU, order, n) == bh && n == 0, "bh %d kU %d order %d block %d past the end", bh, kU, order, b);
  }
  int n = -1;
  CHECK(rowdeal_block(-1, bh, kU, order, n) == bh && n == 0, "bh %d: block -1", bh);
}

// The row loop of phase1_extents (block deals), one wave at a time: `step` advances wave w by one buffer.
struct Wave {
  int rowA, rowB, held, phase;   // phase 0: not started, 1: in the loop before reduce(A), 2: before reduce(B), 3: done
};

static void check_loop(int bh, int kU, int order, int nw, bool drawn, unsigned seed) {
  std::vector<int> seen(bh, 0);
  std::vector<Wave> wv(nw);
  int ctr = 0, done = 0;
  auto row_of = [&](int blk) { int n; return rowdeal_block(blk, bh, kU, order, n); };
  auto reduce = [&](int row0) {
    for (int u = 0; u < kU; ++u)
      if (row0 + u < bh) ++seen[row0 + u];
  };
  for (int w = 0; w < nw; ++w) wv[w] = Wave{0, 0, w + nw, 0};
  auto next_block = [&](Wave &x) {
    if (drawn) return ctr++;
    x.held += nw;
    return x.held;
  };
  while (done < nw) {
    seed = seed * 1664525u + 1013904223u;
    Wave &x = wv[(seed >> 16) % nw];
    const int w = (int)(&x - &wv[0]);
    if (x.phase == 3) continue;
    if (x.phase == 0) {
      if (drawn) {
        const int t = ctr;
        ctr += 2;
        x.rowA = row_of(t);
        x.rowB = row_of(t + 1);
      } else {
        x.rowA = row_of(w);
        x.rowB = row_of(w + nw);
      }
      x.phase = 1;
    }
    if (x.phase == 1) {
      if (!(x.rowA < bh)) {
        CHECK(x.rowB == bh, "bh %d kU %d order %d nw %d: A empty, B holds row %d", bh, kU, order, nw, x.rowB);
        x.phase = 3;
        ++done;
        continue;
      }
      const int nb = next_block(x);
      reduce(x.rowA);
      x.rowA = row_of(nb);
      x.phase = 2;
    } else {
      const int nb = next_block(x);
      reduce(x.rowB);
      x.rowB = row_of(nb);
      x.phase = 1;
    }
  }
  for (int r = 0; r < bh; ++r)
    CHECK(seen[r] == 1, "loop bh %d kU %d order %d nw %d drawn %d: row %d reduced %d times", bh, kU, order, nw, (int)drawn, r,
          seen[r]);
}

int main() {
  long cases = 0;
  for (int bh = 1; bh <= 260; ++bh)
    for (int kU = 3; kU <= 4; ++kU)
      for (int order : {0, 1, 8})
        for (int nw = 8; nw <= 16; nw += 8) {
          check_cover(bh, kU, order, nw);
          check_loop(bh, kU, order, nw, true, 12345u + bh);
          check_loop(bh, kU, order, nw, true, 99u * bh + kU);
          check_loop(bh, kU, order, nw, false, 7u + bh);
          ++cases;
        }
  if (g_fail) {
    printf("rowdeal: %d checks FAILED\n", g_fail);
    return 1;
  }
  printf("rowdeal host code ok (%ld cases)\n", cases);
  return 0;
}
