// depth16_host_main.cc — libtsdf_depth16.so's host-only code (depth16_host.inc, the same source text the library
// compiles) as a stand-alone program for the CPU sanitizers:
//   g++ -fsanitize=address,undefined   /   -fsanitize=thread      (csrc/Makefile: depth16-host-asan, depth16-host-tsan)
// It runs tsdf_depth16_host_gather on valid arguments (one thread and sixteen, small and above the threading threshold,
// against a plain loop) and on deliberately inconsistent ones (each must come back as TSDF_ERR_INVALID_ARG with the
// destination untouched), prints one line and exits 0 — or says what was wrong and exits 1.  A sanitizer report ends it
// on its own.  Test infrastructure (tests/test_depth16_cpu.py runs it as a child process), never shipped.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "depth16_host.inc"

namespace {

int failures = 0;

void expect(bool ok, const char *what) {
  if (!ok) {
    fprintf(stderr, "FAILED: %s\n", what);
    ++failures;
  }
}

// n_src frames of 1..max_len pixels, filled with a counter, and a shuffled index with repeats
struct Pack {
  std::vector<uint16_t> depth;
  std::vector<int64_t> offsets, index;
};

Pack make_pack(int64_t n_src, int64_t max_len, int64_t n, uint64_t seed) {
  Pack p;
  p.offsets.push_back(0);
  uint64_t z = seed;
  auto next = [&z]() {
    z = z * 6364136223846793005ull + 1442695040888963407ull;
    return z >> 33;
  };
  for (int64_t f = 0; f < n_src; ++f) p.offsets.push_back(p.offsets.back() + 1 + (int64_t)(next() % (uint64_t)max_len));
  p.depth.resize((size_t)p.offsets.back());
  for (size_t i = 0; i < p.depth.size(); ++i) p.depth[i] = (uint16_t)(i * 2654435761u >> 7);
  for (int64_t i = 0; i < n; ++i) p.index.push_back((int64_t)(next() % (uint64_t)n_src));
  return p;
}

void check_valid(const Pack &p, int threads, const char *what) {
  const int64_t n = (int64_t)p.index.size();
  int64_t total = 0;
  for (int64_t i = 0; i < n; ++i) total += p.offsets[p.index[i] + 1] - p.offsets[p.index[i]];
  std::vector<uint16_t> dst((size_t)total + 3, 0xABCD);   // three guard words behind the destination
  std::vector<int64_t> off((size_t)n + 1, -1);
  const int rc = tsdf_depth16_host_gather(p.depth.data(), (int64_t)p.depth.size(), p.offsets.data(),
                                          (int64_t)p.offsets.size() - 1, p.index.data(), n, dst.data(), total, off.data(),
                                          threads);
  expect(rc == TSDF_OK, what);
  int64_t at = 0;
  bool same = off[0] == 0;
  for (int64_t i = 0; i < n && same; ++i) {
    const int64_t b = p.offsets[p.index[i]], e = p.offsets[p.index[i] + 1];
    for (int64_t k = b; k < e && same; ++k) same = dst[(size_t)at++] == p.depth[(size_t)k];
    same = same && off[i + 1] == at;
  }
  expect(same && at == total, what);
  expect(dst[(size_t)total] == 0xABCD && dst[(size_t)total + 2] == 0xABCD, "guard words behind the destination");
}

void check_refusals() {
  Pack p = make_pack(12, 40, 9, 5);
  const int64_t n_src = 12, n = 9, len = (int64_t)p.depth.size();
  std::vector<uint16_t> dst((size_t)len * n, 0x5A5A);
  std::vector<int64_t> off((size_t)n + 1);
  const int64_t cap = (int64_t)dst.size();
  auto call = [&](const uint16_t *src, int64_t src_len, const int64_t *so, int64_t ns, const int64_t *ix, int64_t nn,
                  uint16_t *d, int64_t dl, int64_t *dof) {
    return tsdf_depth16_host_gather(src, src_len, so, ns, ix, nn, d, dl, dof, 4);
  };
  const uint16_t *S = p.depth.data();
  const int64_t *SO = p.offsets.data(), *IX = p.index.data();
  expect(call(S, len, SO, n_src, IX, n, dst.data(), cap, off.data()) == TSDF_OK, "the valid call of the refusal set");
  for (auto &v : dst) v = 0x5A5A;
  expect(call(S, -1, SO, n_src, IX, n, dst.data(), cap, off.data()) == TSDF_ERR_INVALID_ARG, "src_len < 0");
  expect(call(S, len, SO, -1, IX, n, dst.data(), cap, off.data()) == TSDF_ERR_INVALID_ARG, "n_src < 0");
  expect(call(S, len, SO, n_src, IX, -1, dst.data(), cap, off.data()) == TSDF_ERR_INVALID_ARG, "n < 0");
  expect(call(nullptr, len, SO, n_src, IX, n, dst.data(), cap, off.data()) == TSDF_ERR_INVALID_ARG, "src NULL");
  expect(call(S, len, nullptr, n_src, IX, n, dst.data(), cap, off.data()) == TSDF_ERR_INVALID_ARG, "src_offsets NULL");
  expect(call(S, len, SO, n_src, nullptr, n, dst.data(), cap, off.data()) == TSDF_ERR_INVALID_ARG, "index NULL");
  expect(call(S, len, SO, n_src, IX, n, nullptr, cap, off.data()) == TSDF_ERR_INVALID_ARG, "dst NULL");
  expect(call(S, len, SO, n_src, IX, n, dst.data(), cap, nullptr) == TSDF_ERR_INVALID_ARG, "dst_offsets NULL");
  expect(call(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr) == TSDF_OK, "n == 0 with nothing at all");
  // a pack that claims more payload than it has, offsets that run backwards, a negative offset
  std::vector<int64_t> all(n_src);
  for (int64_t f = 0; f < n_src; ++f) all[(size_t)f] = f;
  expect(call(S, len - 1, SO, n_src, all.data(), n_src, dst.data(), cap, std::vector<int64_t>(n_src + 1).data()) ==
             TSDF_ERR_INVALID_ARG, "offsets leave the source");
  std::vector<int64_t> bad = p.offsets;
  bad[5] = bad[4] - 1;
  expect(call(S, len, bad.data(), n_src, all.data(), n_src, dst.data(), cap, std::vector<int64_t>(n_src + 1).data()) ==
             TSDF_ERR_INVALID_ARG, "offsets run backwards");
  bad = p.offsets;
  bad[0] = -3;
  expect(call(S, len, bad.data(), n_src, all.data(), n_src, dst.data(), cap, std::vector<int64_t>(n_src + 1).data()) ==
             TSDF_ERR_INVALID_ARG, "a negative offset");
  bad = p.offsets;
  bad[n_src] = INT64_MAX;   // would overflow the running sum (and leaves the source)
  expect(call(S, len, bad.data(), n_src, all.data(), n_src, dst.data(), cap, std::vector<int64_t>(n_src + 1).data()) ==
             TSDF_ERR_INVALID_ARG, "a huge offset");
  // indices outside the pack
  std::vector<int64_t> ix = p.index;
  ix[3] = n_src;
  expect(call(S, len, SO, n_src, ix.data(), n, dst.data(), cap, off.data()) == TSDF_ERR_INVALID_ARG, "index == n_src");
  ix[3] = -1;
  expect(call(S, len, SO, n_src, ix.data(), n, dst.data(), cap, off.data()) == TSDF_ERR_INVALID_ARG, "index < 0");
  // a destination one element short
  int64_t total = 0;
  for (int64_t i = 0; i < n; ++i) total += p.offsets[p.index[i] + 1] - p.offsets[p.index[i]];
  expect(call(S, len, SO, n_src, IX, n, dst.data(), total - 1, off.data()) == TSDF_ERR_INVALID_ARG, "dst_len short");
  expect(call(S, len, SO, n_src, IX, n, dst.data(), total, off.data()) == TSDF_OK, "dst_len exact");
  for (size_t i = (size_t)total; i < dst.size(); ++i)
    if (dst[i] != 0x5A5A) {
      expect(false, "a refused or exact call wrote behind its destination");
      break;
    }
}

}  // namespace

int main() {
  check_valid(make_pack(1, 1, 1, 1), 1, "one frame of one pixel");
  check_valid(make_pack(50, 300, 64, 2), 1, "small gather, one thread");
  check_valid(make_pack(50, 300, 64, 2), 16, "small gather, sixteen threads asked (runs on one)");
  const Pack big = make_pack(400, 20000, 300, 3);   // ~3 M pixels: above the threading threshold
  check_valid(big, 1, "large gather, one thread");
  check_valid(big, 16, "large gather, sixteen threads");
  check_valid(big, 1000, "large gather, thread count clamped");
  check_refusals();
  if (failures) return 1;
  printf("depth16 host code ok\n");
  return 0;
}
