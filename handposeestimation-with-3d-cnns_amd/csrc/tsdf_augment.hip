// tsdf_augment.hip — libtsdf_augment.so: the 3-D augmentation's draws and maps on the GPU (include/tsdf_augment.h).
//
// A translation unit and a library of its own, next to the product (tsdf_hip.hip -> libtsdf_hip.so, whose ABI is
// frozen): it shares the status codes of include/tsdf.h and the host preamble of device.inc — none of the product's other
// .inc files is included.
// The draw and map arithmetic is in augdraw.inc, which tsdf_augstep.hip (libtsdf_augstep.so) includes too.
//
// What it replaces: augment.random_affines per batch on the host (a numpy Generator, stacked rotation matrices,
// np.linalg.inv over n 3x3 blocks, a pinned buffer and a copy).  Here one launch of a few microseconds writes the
// float64[n][24] maps tsdf_voxelize_*aug_hip read, from a counter: position i of the batch draws from
// (key, counter0 + i), so an augmented step sends frame indices and nothing else, and a range of counters gives the same
// maps however it is cut into launches.
//
// Kernel: one lane per batch position, 256-thread workgroups, no LDS, no atomics.  A lane's work is three splitmix64
// chains, two sincos and ~60 float64 multiply-adds; its 192-byte row leaves as twelve 16-byte stores
// (global_store_dwordx4).  Rows are 192 bytes apart, so a wave's store instruction touches 64 separate 16-byte pieces
// — at n = 16..1024 rows (3..196 KB) the launch is latency, not bandwidth; the wide store keeps it at 12 store
// instructions per lane instead of 24 or 48.
// Arithmetic contract (include/tsdf_augment.h): float64 throughout, -ffp-contract=off (stretch = lo + u*span is
// "multiply, round, add, round", as augment.device_draws_np computes it).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_augment.h"

namespace {

#include "device.inc"    // check_device, launched, misaligned: the host preamble of every library here
#include "augdraw.inc"   // aug_mix, aug_angle, aug_draw_row: shared with tsdf_augstep.hip

struct AugArgs {
  const float *centres;    // [n_src][3]
  int64_t n_src;
  const int64_t *index;    // [n] or null
  int n;
  uint64_t key, counter0;
  double *xforms;          // [n][24]
  double *stretch;         // [n] or null
  int32_t *rot;            // [n][2] or null
};

__global__ __launch_bounds__(kAugWG) void tsdf_aug_draw_kernel(AugArgs a) {
  const int i = blockIdx.x * kAugWG + threadIdx.x;
  if (i >= a.n) return;
  const int64_t g = a.index ? a.index[i] : (int64_t)i;
  aug_draw_row(a.centres, a.n_src, g, i, a.key, a.counter0 + (uint64_t)i, a.xforms, a.stretch, a.rot);
}

}  // namespace

extern "C" {

int tsdf_augment_version(void) { return TSDF_AUGMENT_VERSION; }

int tsdf_aug_draw_hip(const float *d_centres, int64_t n_src, const int64_t *d_index, int n, uint64_t key,
                      uint64_t counter0, void *hip_stream, double *d_out_xforms, double *d_out_stretch,
                      int32_t *d_out_rot) {
  // arguments are checked before the device is looked at
  if (n < 0) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  if (!d_centres || !d_out_xforms || n_src < 1) return TSDF_ERR_INVALID_ARG;
  if (misaligned(d_out_xforms, 7)) return TSDF_ERR_INVALID_ARG;
  const int rc = check_device(nullptr);
  if (rc != TSDF_OK) return rc;
  AugArgs a;
  a.centres = d_centres;
  a.n_src = n_src;
  a.index = d_index;
  a.n = n;
  a.key = key;
  a.counter0 = counter0;
  a.xforms = d_out_xforms;
  a.stretch = d_out_stretch;
  a.rot = d_out_rot;
  const unsigned blocks = ((unsigned)n + kAugWG - 1) / kAugWG;
  hipLaunchKernelGGL(tsdf_aug_draw_kernel, dim3(blocks), dim3(kAugWG), 0, static_cast<hipStream_t>(hip_stream), a);
  return launched();
}

}  // extern "C"
