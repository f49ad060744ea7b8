// tsdf_augstep.hip — libtsdf_augstep.so: the augmentation's draws and maps from DEVICE-RESIDENT key and counters
// (include/tsdf_augstep.h).
//
// A translation unit and a library of its own, next to libtsdf_hip.so and libtsdf_augment.so (both frozen).  It shares the
// status codes of include/tsdf.h, the host preamble of device.inc and, with tsdf_augment.hip, augdraw.inc: the draw and map
// arithmetic exists once.
//
// What it adds to tsdf_aug_draw_hip: that entry takes key and counter0 as kernel arguments and gives position i the counter
// counter0 + i.  Two things cannot be done with it: a batch whose counters are not contiguous (a shuffled batch in which
// every frame has a fixed draw of its own) needs one launch per frame, and a launch captured into a graph has its key and
// counter frozen into the kernel node, so every replay repeats one augmentation.  Here the kernel loads {key, counter0}
// from d_state[2] and, optionally, a per-position counter from d_counters[n].
//
// Kernel: the shape of tsdf_aug_draw_kernel — one lane per batch position, 256-thread workgroups, no LDS, no atomics, the
// 192-byte row as twelve 16-byte stores.  The two state words are loaded once per lane from an address that is uniform
// across the launch (the compiler is free to make them scalar loads); nothing but the outputs is written.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_augstep.h"

namespace {

#include "device.inc"    // check_device, launched, misaligned: the host preamble of every library here
#include "augdraw.inc"   // aug_mix, aug_angle, aug_draw_row: shared with tsdf_augment.hip

struct AugAtArgs {
  const float *centres;      // [n_src][3]
  int64_t n_src;
  const int64_t *index;      // [n] or null
  int n;
  const uint64_t *state;     // {key, counter0}
  const int64_t *counters;   // [n] or null
  double *xforms;            // [n][24]
  double *stretch;           // [n] or null
  int32_t *rot;              // [n][2] or null
};

__global__ __launch_bounds__(kAugWG) void tsdf_aug_draw_at_kernel(AugAtArgs a) {
  const int i = blockIdx.x * kAugWG + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t key = a.state[0], counter0 = a.state[1];
  const int64_t g = a.index ? a.index[i] : (int64_t)i;
  const uint64_t c = counter0 + (a.counters ? (uint64_t)a.counters[i] : (uint64_t)i);
  aug_draw_row(a.centres, a.n_src, g, i, key, c, a.xforms, a.stretch, a.rot);
}

}  // namespace

extern "C" {

int tsdf_augstep_version(void) { return TSDF_AUGSTEP_VERSION; }

int tsdf_aug_draw_at_hip(const float *d_centres, int64_t n_src, const int64_t *d_index, int n, const uint64_t *d_state,
                         const int64_t *d_counters, void *hip_stream, double *d_out_xforms, double *d_out_stretch,
                         int32_t *d_out_rot) {
  // arguments are checked before the device is looked at
  if (n < 0) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_centres || !d_state || !d_out_xforms || n_src < 1) return TSDF_ERR_INVALID_ARG;
  if (misaligned(d_out_xforms, 7) || misaligned(d_state, 7)) return TSDF_ERR_INVALID_ARG;
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  AugAtArgs a;
  a.centres = d_centres;
  a.n_src = n_src;
  a.index = d_index;
  a.n = n;
  a.state = d_state;
  a.counters = d_counters;
  a.xforms = d_out_xforms;
  a.stretch = d_out_stretch;
  a.rot = d_out_rot;
  const unsigned blocks = ((unsigned)n + kAugWG - 1) / kAugWG;
  hipLaunchKernelGGL(tsdf_aug_draw_at_kernel, dim3(blocks), dim3(kAugWG), 0, static_cast<hipStream_t>(hip_stream), a);
  return launched();
}

}  // extern "C"
