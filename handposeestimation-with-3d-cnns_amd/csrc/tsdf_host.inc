// tsdf_host.inc — the part of the library that never touches the GPU, in plain C++17 (no HIP types, no HIP calls).
//
// Included by tsdf_hip.hip (the product: one translation unit, one hipcc command) AND compiled on its own by
//   g++ -std=c++17 -fsanitize=address,undefined   /   -fsanitize=thread      (csrc/Makefile: host-asan, host-tsan)
// through tsdf_host_test.cc, which exports a few test hooks on top — so that the product's own threaded gather, its
// offset validation, its argument checks and its per-stream slot table run under the sanitizers on the CPU tier
// (tests/test_tiers_cpu.py).  GPU sanitizers are not available on the pool; this is the code that needs none.
//
// Contents:
//   tsdf_host::gather()          frames of a packed host buffer copied back to back by a few threads
//                                (tsdf_host_gather_frames / _n of include/tsdf.h)
//   tsdf_host::Frames / Outs / RunOpts   one call of a voxelizer entry, as abi.inc hands it to run()
//   tsdf_host::check_run_args()  ALL argument validation of the voxelizer entries, driven by RunOpts::needs; run() calls
//                                it once, the entries themselves check nothing
//   tsdf_host::check_pca()       the joint-PCA descriptor
//   tsdf_host::SlotTable         (stream, thread) -> slot of the per-stream device words, under its own mutex, with the
//                                launch counter that tags a stream's work-queue word
#pragma once

#include <stdint.h>
#include <string.h>

#include <mutex>
#include <thread>

#include "../../include/tsdf.h"

namespace tsdf_host {

// the camera rule (cam_ok) as every library here applies it; the device primitives of prim.inc stay out of this file
#define TSDF_PRIM_HOST_ONLY
#include "prim.inc"
#undef TSDF_PRIM_HOST_ONLY

// ---- frames index[0..n) of a packed host buffer copied back to back into dst ------------------------------------
// dst_offsets[n+1] is filled in; `threads` workers split the bytes evenly.  src_len < 0: unknown (the v4 entry).
// Everything is validated before the first byte is copied: an index outside the pack, offsets that run backwards or
// leave the source (a damaged pack), a destination that is too small.
inline int gather(const float *src, int64_t src_len, const int64_t *src_offsets, int64_t n_src, const int64_t *index,
                  int64_t n, float *dst, int64_t dst_capacity, int64_t *dst_offsets, int threads) {
  if (n < 0 || n_src < 0 || (n > 0 && (!src || !src_offsets || !index || !dst || !dst_offsets))) return TSDF_ERR_INVALID_ARG;
  if (!dst_offsets) return n == 0 ? TSDF_OK : TSDF_ERR_INVALID_ARG;
  dst_offsets[0] = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t f = index[i];
    if (f < 0 || f >= n_src) return TSDF_ERR_INVALID_ARG;
    const int64_t b = src_offsets[f], e = src_offsets[f + 1];
    if (b < 0 || e < b || (src_len >= 0 && e > src_len)) return TSDF_ERR_INVALID_ARG;  // a damaged pack: nothing is read
    if (e - b > INT64_MAX - dst_offsets[i]) return TSDF_ERR_INVALID_ARG;                 // (the running sum cannot overflow)
    dst_offsets[i + 1] = dst_offsets[i] + (e - b);
  }
  const int64_t total = dst_offsets[n];
  if (total > dst_capacity) return TSDF_ERR_INVALID_ARG;
  if (threads < 1) threads = 1;
  if (threads > 64) threads = 64;
  if (total < (1 << 18)) threads = 1;  // under a megabyte: starting threads costs more than the copy
  auto work = [&](int t, int of) {
    // frames whose first element falls into this worker's share of the elements
    const int64_t lo = (int64_t)((__int128)total * t / of), hi = (int64_t)((__int128)total * (t + 1) / of);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t a = dst_offsets[i];
      if (a < lo) continue;
      if (a >= hi) break;
      const int64_t len = dst_offsets[i + 1] - a;
      if (len > 0) memcpy(dst + a, src + src_offsets[index[i]], sizeof(float) * (size_t)len);
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

// ---- one call of a voxelizer entry: the packed frames, the outputs, and what the entry adds ----------------------------
// Every extern "C" voxelizer entry (abi.inc) fills these three and hands them to run() (launch.inc), which calls
// check_run_args() once.  They live here so that the sanitizer build compiles the check with the structs it reads.
struct Frames {
  const float *depth;
  int64_t depth_len;
  const int64_t *offsets;
  const int32_t *headers;
  int n, R;
  const tsdf_cam *cam;
  int layout;
  void *stream;
};

struct Outs {
  float *tsdf, *max_l, *mid_p;
  int32_t *status;
};

// what an entry requires when n > 0 (RunOpts::needs)
enum : unsigned {
  kNeedPlacement = 1u << 0,  // max_l and mid_p
  kNeedIndex = 1u << 1,      // index, in device memory; n_src frames in the pack
  kNeedHostIndex = 1u << 2,  // h_index, in host memory, at most TSDF_INLINE_INDEX_MAX entries; n_src frames in the pack
  kNeedXforms = 1u << 3,
  kNeedLabels = 1u << 4,     // (also when n == 0)
  kNeedPca = 1u << 5,        // (also when n == 0; implies labels)
  kNeedGridIn = 1u << 6,
  kNeedPixmap = 1u << 7,
};

struct RunOpts {
  unsigned needs = 0;
  float *aabb = nullptr, *grid = nullptr, *ori = nullptr;
  int aabb_only = 0;
  const float *grid_in = nullptr;
  const double *xforms = nullptr;
  const tsdf_labels *labels = nullptr;
  int32_t *pixmap = nullptr;
  const int64_t *index = nullptr;  // indexed entry
  int64_t n_src = 0;
  const int64_t *h_index = nullptr;  // indexed entry, index in HOST memory, copied into the kernel arguments
  const tsdf_pca *pca = nullptr;     // joint PCA projection fused into the labels (requires labels)
};

// ---- the joint-PCA descriptor (include/tsdf.h, tsdf_pca) for n frames of n_joints joints ------------------------------
// need_out: the entry writes d_out_gt_pca (every entry but tsdf_pose_error_hip).
inline int check_pca(const tsdf_pca *pca, int n, int n_joints, bool need_out) {
  if (!pca || n_joints < 1 || n_joints > 170) return TSDF_ERR_INVALID_ARG;
  if (pca->n_components < 1 || pca->n_components > 3 * n_joints) return TSDF_ERR_INVALID_ARG;
  if (n > 0 && (!pca->d_mean || !pca->d_coeff || (need_out && !pca->d_out_gt_pca))) return TSDF_ERR_INVALID_ARG;
  return TSDF_OK;
}

// ---- what every voxelizer entry checks before it looks at the device ----------------------------------------------
// TSDF_OK: go on (n > 0);  1: nothing to do (n == 0, after the checks that do not need data);  < 0: the error.
constexpr int kNothingToDo = 1;
inline int check_run_args(const Frames &f, const Outs &out, const RunOpts &o, int resolution_supported) {
  const int n = f.n;
  // -- what holds for an empty batch too: sizes, descriptors, alignment
  if (n < 0 || !resolution_supported) return TSDF_ERR_INVALID_ARG;
  if (f.layout != TSDF_LAYOUT_CZYX && f.layout != TSDF_LAYOUT_CXYZ) return TSDF_ERR_INVALID_ARG;
  if ((o.needs & (kNeedLabels | kNeedPca)) && !o.labels) return TSDF_ERR_INVALID_ARG;
  if (o.labels) {
    if (o.labels->n_joints < 1 || o.labels->n_joints > 170) return TSDF_ERR_INVALID_ARG;
    if (n > 0 && (!o.labels->d_gt || !o.labels->d_out_gt_nor)) return TSDF_ERR_INVALID_ARG;
  }
  if ((o.needs & kNeedPca) && check_pca(o.pca, n, o.labels->n_joints, true) != TSDF_OK) return TSDF_ERR_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(o.xforms) & 7) return TSDF_ERR_INVALID_ARG;
  if ((o.needs & (kNeedIndex | kNeedHostIndex)) && (o.n_src < 0 || (n > 0 && o.n_src == 0))) return TSDF_ERR_INVALID_ARG;
  if ((o.needs & kNeedHostIndex) && n > TSDF_INLINE_INDEX_MAX) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return kNothingToDo;
  // -- n > 0: everything the launch reads or writes
  if ((o.needs & kNeedPlacement) && (!out.max_l || !out.mid_p)) return TSDF_ERR_INVALID_ARG;
  if ((o.needs & kNeedIndex) && !o.index) return TSDF_ERR_INVALID_ARG;
  if ((o.needs & kNeedHostIndex) && !o.h_index) return TSDF_ERR_INVALID_ARG;
  if ((o.needs & kNeedXforms) && !o.xforms) return TSDF_ERR_INVALID_ARG;
  if ((o.needs & kNeedGridIn) && !o.grid_in) return TSDF_ERR_INVALID_ARG;
  if ((o.needs & kNeedPixmap) && !o.pixmap) return TSDF_ERR_INVALID_ARG;
  if (!f.depth || !f.offsets || !f.headers || f.depth_len < 0) return TSDF_ERR_INVALID_ARG;
  if (!o.aabb_only && (!out.tsdf || (reinterpret_cast<uintptr_t>(out.tsdf) & 15))) return TSDF_ERR_INVALID_ARG;
  if (!cam_ok(f.cam)) return TSDF_ERR_INVALID_ARG;
  return TSDF_OK;
}

// ---- per-stream slots -------------------------------------------------------------------------------------------------
// Launches of one stream execute in order, so a device word owned by the stream is never shared by two running launches,
// however many are in flight.  hipStreamPerThread is one handle for a different stream per thread: it is keyed by the
// calling thread as well.  The table also counts the launches that used a slot's work-queue word: the count (never 0)
// travels to the kernel as the word's EPOCH, which is how a word left dirty by a launch that never finished — or
// written by anything else — is recognised and re-initialised instead of skewing every ticket (see queue_ticket()).
template <int N>
struct SlotTable {
  std::mutex mu;
  struct Entry {
    bool used;
    const void *s;
    std::thread::id tid;
  } e[N] = {};
  uint32_t epoch[N] = {};
  int high = 0;  // entries [0, high) may be in use

  // Index of (stream, calling thread if per_thread) — taking a free slot for a pair seen for the first time — or -1
  // when the table is full.  Cost: a linear scan of the entries in use, under the mutex.
  int acquire(const void *stream, bool per_thread) {
    const std::thread::id me = per_thread ? std::this_thread::get_id() : std::thread::id();
    std::lock_guard<std::mutex> lock(mu);
    int free_i = -1;
    for (int i = 0; i < high; ++i) {
      if (e[i].used) {
        if (e[i].s == stream && e[i].tid == me) return i;
      } else if (free_i < 0) {
        free_i = i;
      }
    }
    if (free_i < 0 && high < N) free_i = high++;
    if (free_i < 0) return -1;
    e[free_i].used = true;
    e[free_i].s = stream;
    e[free_i].tid = me;
    return free_i;
  }
  // Forget the pair (its slot, and the slot's epoch counter, pass to the next pair that needs one).
  void release(const void *stream, bool per_thread) {
    const std::thread::id me = per_thread ? std::this_thread::get_id() : std::thread::id();
    std::lock_guard<std::mutex> lock(mu);
    for (int i = 0; i < high; ++i)
      if (e[i].used && e[i].s == stream && e[i].tid == me) e[i].used = false;
  }
  // The epoch of the next launch through slot i's queue word: 1, 2, ..., 2^32 - 1, 1, ... (0 is what a fresh word holds).
  uint32_t next_epoch(int i) {
    std::lock_guard<std::mutex> lock(mu);
    uint32_t v = ++epoch[i];
    if (v == 0) v = ++epoch[i];
    return v;
  }
};

}  // namespace tsdf_host

extern "C" {

int tsdf_host_gather_frames(const float *src, const int64_t *src_offsets, int64_t n_src, const int64_t *index, int64_t n,
                            float *dst, int64_t dst_capacity, int64_t *dst_offsets, int threads) {
  return tsdf_host::gather(src, -1, src_offsets, n_src, index, n, dst, dst_capacity, dst_offsets, threads);
}

int tsdf_host_gather_frames_n(const float *src, int64_t src_len, const int64_t *src_offsets, int64_t n_src,
                              const int64_t *index, int64_t n, float *dst, int64_t dst_capacity, int64_t *dst_offsets,
                              int threads) {
  if (src_len < 0) return TSDF_ERR_INVALID_ARG;
  return tsdf_host::gather(src, src_len, src_offsets, n_src, index, n, dst, dst_capacity, dst_offsets, threads);
}

}  // extern "C"
