// tsdf_depth16.hip — libtsdf_depth16.so: 16-bit depth widened to the float32 buffer the voxelizer reads, and the 16-bit
// twin of the loaders' host gather (include/tsdf_depth16.h).
//
// A translation unit and a library of its own, next to libtsdf_hip.so and the three aug* extensions (all frozen).  It
// shares the status codes of include/tsdf.h and the host preamble of device.inc (device_cus sizes the grid); the host
// gather is depth16_host.inc (plain C++, also built on its own under the CPU sanitizers).
//
// Kernel: a streaming conversion, 2 bytes in and 4 bytes out per pixel, nothing reused — it should run at memory rate.
//   * A lane converts eight pixels per step: ONE 16-byte load, eight v_cvt + v_mul, TWO 16-byte stores.  A wave's load
//     covers 1 KiB of contiguous source, each of its two stores 64 x 16 B at a 32-byte lane stride.
//   * Grid-stride loop over the groups of eight, 64-bit indices; the grid is 8 workgroups of 256 threads per CU (fewer
//     when there are fewer groups than that), whatever n_px is.
//   * Alignment.  d_dst is only 4-byte aligned and d_src only 2-byte aligned.  The host peels `head` = 0..3 pixels so
//     that d_dst + head is 16-byte aligned: every vector store is aligned.  The source of the body, d_src + head, is
//     then 16-byte aligned or not, independently of that, so it is loaded through a vector type DECLARED 2-byte aligned:
//     the compiler lowers such a load to whatever the target guarantees for that alignment — for gfx950 under HSA
//     (unaligned access mode) still one global_load_dwordx4, which the memory pipeline serves at any 2-byte boundary
//     (a misaligned wave touches one more 128-byte line than an aligned one).  One kernel for every combination.
//     The head and the tail (n_px - head) % 8 pixels are converted one by one by the first lanes of the grid.
//   * No LDS, no atomics, no inline assembly, no scratch (make depth16-resources).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_depth16.h"
#include "depth16_host.inc"

namespace {

#include "device.inc"   // device_cus, launched, misaligned: the host preamble of every library here

constexpr int kWG = 256;          // threads per workgroup (4 wave64)
constexpr int kWGPerCU = 8;       // workgroups per CU the grid is sized for

typedef unsigned short d16_u16x8 __attribute__((ext_vector_type(8), aligned(2)));   // 16 bytes on a 2-byte boundary
typedef float d16_f32x4 __attribute__((ext_vector_type(4)));                         // 16 bytes, 16-byte aligned

// src/dst: the call's arrays.  Pixels [0, head) and [head + 8 * groups, n_px) are converted one by one; group g is
// pixels head + 8g .. head + 8g + 7, and dst + head is 16-byte aligned (the host chose head so).
__global__ __launch_bounds__(kWG) void tsdf_depth16_widen_kernel(const uint16_t *__restrict__ src, int64_t n_px,
                                                                 int64_t head, int64_t groups, float scale,
                                                                 float *__restrict__ dst) {
  const int64_t tid = (int64_t)blockIdx.x * kWG + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kWG;
  const int64_t tail0 = head + 8 * groups;   // first pixel of the tail; n_px - tail0 < 8
  if (tid < head) dst[tid] = (float)src[tid] * scale;
  if (tid < n_px - tail0) dst[tail0 + tid] = (float)src[tail0 + tid] * scale;

  const uint16_t *s = src + head;
  float *d = dst + head;
  for (int64_t g = tid; g < groups; g += stride) {
    const d16_u16x8 q = *reinterpret_cast<const d16_u16x8 *>(s + 8 * g);
    d16_f32x4 lo, hi;
    lo.x = (float)q.s0 * scale;
    lo.y = (float)q.s1 * scale;
    lo.z = (float)q.s2 * scale;
    lo.w = (float)q.s3 * scale;
    hi.x = (float)q.s4 * scale;
    hi.y = (float)q.s5 * scale;
    hi.z = (float)q.s6 * scale;
    hi.w = (float)q.s7 * scale;
    d16_f32x4 *o = reinterpret_cast<d16_f32x4 *>(d + 8 * g);
    o[0] = lo;
    o[1] = hi;
  }
}

}  // namespace

extern "C" {

int tsdf_depth16_version(void) { return TSDF_DEPTH16_VERSION; }

int tsdf_depth16_widen_hip(const uint16_t *d_src, int64_t n_px, int shift, float *d_dst, void *hip_stream) {
  // arguments are checked before the device is looked at
  if (n_px < 0 || shift < 0 || shift > TSDF_DEPTH16_MAX_SHIFT) return TSDF_ERR_INVALID_ARG;
  if (n_px == 0) return TSDF_OK;
  if (!d_src || !d_dst) return TSDF_ERR_INVALID_ARG;
  if (misaligned(d_src, 1) || misaligned(d_dst, 3)) return TSDF_ERR_INVALID_ARG;
  const int cus = device_cus();
  if (cus < 0) return cus;

  const uintptr_t da = reinterpret_cast<uintptr_t>(d_dst);
  int64_t head = (int64_t)(((16 - (da & 15)) & 15) >> 2);   // pixels up to the destination's next 16-byte boundary
  if (head > n_px) head = n_px;
  const int64_t groups = (n_px - head) / 8;
  // every group gets a lane's turn; the head and the tail (at most 3 and 7 pixels) fit the first workgroup
  int64_t blocks = (groups + kWG - 1) / kWG;
  if (blocks < 1) blocks = 1;
  if (blocks > (int64_t)cus * kWGPerCU) blocks = (int64_t)cus * kWGPerCU;
  const float scale = 1.0f / (float)(1 << shift);
  hipLaunchKernelGGL(tsdf_depth16_widen_kernel, dim3((unsigned)blocks), dim3(kWG), 0, static_cast<hipStream_t>(hip_stream),
                     d_src, n_px, head, groups, scale, d_dst);
  return launched();
}

}  // extern "C"
