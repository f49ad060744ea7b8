// depth16_host.inc — the part of libtsdf_depth16.so that never touches the GPU, in plain C++17 (no HIP types, no HIP
// calls): tsdf_depth16_host_gather of include/tsdf_depth16.h, the 16-bit twin of tsdf_host::gather (tsdf_host.inc).
//
// Included by tsdf_depth16.hip (the library) AND by depth16_host_main.cc, a stand-alone program that g++ builds with
//   -fsanitize=address,undefined   /   -fsanitize=thread      (csrc/Makefile: depth16-host-asan, depth16-host-tsan)
// and tests/test_depth16_cpu.py runs as a child process: the same source text under the CPU sanitizers.
#pragma once

#include <stdint.h>
#include <string.h>

#include <thread>

#include "../../include/tsdf_depth16.h"

namespace tsdf_depth16_host {

// frames index[0..n) of a packed host buffer copied back to back into dst; dst_offsets[n+1] is filled in; `threads`
// workers split the elements evenly.  Everything is validated before the first byte is copied.  (static: the library
// exports what its header declares and nothing else, not even weak symbols of this function and its thread objects.)
static int gather(const uint16_t *src, int64_t src_len, const int64_t *src_offsets, int64_t n_src, const int64_t *index,
                  int64_t n, uint16_t *dst, int64_t dst_capacity, int64_t *dst_offsets, int threads) {
  if (src_len < 0 || n < 0 || n_src < 0) return TSDF_ERR_INVALID_ARG;
  if (n > 0 && (!src || !src_offsets || !index || !dst || !dst_offsets)) return TSDF_ERR_INVALID_ARG;
  if (!dst_offsets) return TSDF_OK;  // (n == 0 and nowhere to write the single 0)
  dst_offsets[0] = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t f = index[i];
    if (f < 0 || f >= n_src) return TSDF_ERR_INVALID_ARG;
    const int64_t b = src_offsets[f], e = src_offsets[f + 1];
    if (b < 0 || e < b || e > src_len) return TSDF_ERR_INVALID_ARG;       // a damaged pack: nothing is read
    if (e - b > INT64_MAX - dst_offsets[i]) return TSDF_ERR_INVALID_ARG;  // (the running sum cannot overflow)
    dst_offsets[i + 1] = dst_offsets[i] + (e - b);
  }
  const int64_t total = dst_offsets[n];
  if (total > dst_capacity) return TSDF_ERR_INVALID_ARG;
  if (threads < 1) threads = 1;
  if (threads > 64) threads = 64;
  if (total < (1 << 19)) threads = 1;  // under a megabyte: starting threads costs more than the copy
  auto work = [&](int t, int of) {
    // frames whose first element falls into this worker's share of the elements
    const int64_t lo = (int64_t)((__int128)total * t / of), hi = (int64_t)((__int128)total * (t + 1) / of);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t a = dst_offsets[i];
      if (a < lo) continue;
      if (a >= hi) break;
      const int64_t len = dst_offsets[i + 1] - a;
      if (len > 0) memcpy(dst + a, src + src_offsets[index[i]], sizeof(uint16_t) * (size_t)len);
    }
  };
  if (threads == 1) {
    work(0, 1);
    return TSDF_OK;
  }
  // std::thread's constructor may throw (std::system_error: no resources); nothing may cross the C boundary, so the
  // shares of workers that could not be started are copied here
  std::thread pool[64];
  int started = 1;  // share 0 is this thread's
  try {
    for (; started < threads; ++started) pool[started] = std::thread(work, started, threads);
  } catch (...) {
  }
  work(0, threads);
  for (int t = started; t < threads; ++t) work(t, threads);
  for (int t = 1; t < started; ++t) pool[t].join();
  return TSDF_OK;
}

}  // namespace tsdf_depth16_host

extern "C" int tsdf_depth16_host_gather(const uint16_t *src, int64_t src_len, const int64_t *src_offsets, int64_t n_src,
                                        const int64_t *index, int64_t n, uint16_t *dst, int64_t dst_len,
                                        int64_t *dst_offsets, int n_threads) {
  return tsdf_depth16_host::gather(src, src_len, src_offsets, n_src, index, n, dst, dst_len, dst_offsets, n_threads);
}
