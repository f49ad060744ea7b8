// tsdf_pointfield.hip — libtsdf_pointfield.so: point-wise offset-field labels of sampled clouds and their voting decode
// (include/tsdf_pointfield.h, which has the contract operation by operation).
//
// A translation unit and a library of its own, next to libtsdf_hip.so and the other libraries (all frozen).  It takes the
// status codes from include/tsdf.h, the host preamble every library here has from device.inc, finite32 from prim.inc and
// its argument rules and its plan from pointfield_host.inc, plain C++ that is also built on its own under the CPU
// sanitizers.  No device global and no global atomic: every launch is self-contained.
//
// Both kernels are a SELECTION WITHOUT A SORT per joint over a cloud resident in LDS: membership in a top-K set needs the
// K-th smallest key, not a sorted list.  A workgroup of kPfWG threads serves kPfJoints joints of ONE batch position; the
// grid is one-dimensional, block b is tile b % tiles of position b / tiles.
//   1. STAGE (pf_stage).  Row i of the cloud goes to slot i of three float32 arrays in (dynamic) LDS; a row that is no
//      candidate (and the padding up to whole waves) gets a NaN x.  The candidates are counted by ballot; the waves' counts
//      meet in LDS: their sum is m.  The slots are NOT compacted: both kernels write or read the field by rank, and slot
//      order is rank order, so "ties to the lowest rank" is "ties to the lowest slot" with no rank array (which the LDS
//      has no room for at the cap).
//   2. KEYS.  One wave owns a joint at a time.  Lane l owns the slots 64 s + l.  The key of a slot is a 32-bit unsigned
//      whose order is the selection's: encode, the bits of dist2; decode, the complement of the heat's order-preserving
//      image (a NaN above every number).  A slot without a candidate holds all ones, above every key.  For clouds of up
//      to 64 * kPfRegSlots rows a lane keeps its keys in registers (REG); beyond, it recomputes them on every pass.
//   3. SELECT (pf_select).  The k-th smallest key bit by bit from the top: per bit one pass over the slots, a ballot of
//      "matches the prefix and has a 0 here", a popcount; the count decides the bit.  What remains of k at the end is r,
//      how many of the keys equal to the k-th belong to the set: the first r in slot order.  k >= m skips the passes.
//   4. WALK.  One more pass in slot order with a running count of the ties.  Encode writes the four channels of each row
//      (in "cp" 64 lanes write 64 consecutive values of a channel; in "pc" the same values go out as strided stores).
//      Decode hands each selected candidate, in ascending order, to the lane of its compact index and ends with the
//      butterfly of the contract's tree sum.
// All global indexing is in 64 bits.  Compiled with -ffp-contract=off: no fused multiply-add anywhere in this file.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_pointfield.h"

namespace {

#include "device.inc"           // check_device, launched, misaligned: the host preamble of every library here
#include "prim.inc"             // finite32
#include "pointfield_host.inc"  // pf_encode_defect, pf_decode_defect, pf_plan, pf_padded, kPfWG

constexpr unsigned kPfNone = ~0u;        // a slot without a candidate: above every key
constexpr unsigned kPfNanKey = ~0u - 1;  // decode: a NaN heat, above every number's key

struct PfArgs {
  const float *points;      // [n][pitch][3]
  int64_t pitch;
  const float *joints;      // encode: [n][J][3]
  const void *field_in;     // decode: the field
  const int32_t *status_in; // [n] or null
  int P, J, K;              // K: encode's K, decode's M
  unsigned tiles;           // workgroups per position
  double radius;
  int layout, dtype;
  void *out_field;          // encode: the field
  int32_t *out_valid;       // encode: [n][J]
  float *out_joints;        // decode: [n][J][3]
  float *out_weight;        // decode: [n][J]
  int32_t *out_status;      // [n]
};

// What a workgroup holds of its position: slot i is row i (x a NaN where the row is no candidate), and m.
struct PfCloud {
  const float *x, *y, *z;   // [pf_padded(P)] each
  int m;
};

// `read` false (a position with an input status): nothing is read and m is 0.
__device__ __forceinline__ PfCloud pf_stage(char *lds, const float *rows, int P, bool read, int wave, int lane) {
  const int pad = pf_padded(P);
  float *x = reinterpret_cast<float *>(lds), *y = x + pad, *z = y + pad;
  int *s_cnt = reinterpret_cast<int *>(z + pad);
  int mine = 0;
  for (int i0 = wave * 64; i0 < pad; i0 += kPfWG) {   // the bounds are the wave's
    const int i = i0 + lane;                          // < pad
    float px = __builtin_nanf(""), py = 0.f, pz = 0.f;
    bool cand = false;
    if (read && i < P) {
      const float *r = rows + 3 * (int64_t)i;
      const float a = r[0], b = r[1], c = r[2];
      cand = finite32(a) && finite32(b) && finite32(c);
      if (cand) px = a, py = b, pz = c;
    }
    x[i] = px, y[i] = py, z[i] = pz;
    mine += __popcll(__ballot(cand));
  }
  if (lane == 0) s_cnt[wave] = mine;
  __syncthreads();
  PfCloud c;
  c.x = x, c.y = y, c.z = z, c.m = 0;
#pragma unroll
  for (int w = 0; w < kPfWaves; ++w) c.m += s_cnt[w];
  return c;
}

// f(s) for every slot row s < ns of the lane.  REG: fully unrolled, so that an array indexed by s stays in registers.
template <bool REG, typename F>
__device__ __forceinline__ void pf_slots(int ns, F f) {
  if constexpr (REG) {
#pragma unroll
    for (int s = 0; s < kPfRegSlots; ++s)
      if (s < ns) f(s);   // uniform
  } else {
    for (int s = 0; s < ns; ++s) f(s);
  }
}

// this lane's number among the set lanes of `m` below it
__device__ __forceinline__ int pf_below(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// 3. The k-th smallest key of the wave's slots, 1 <= k <= the number of keys below kPfNone: its value, and how many of the
// keys equal to it are among the k smallest.  Uniform in, uniform out.
template <bool REG, typename Key>
__device__ __forceinline__ void pf_select(int ns, int k, Key key, unsigned &kth, int &ties_in) {
  unsigned prefix = 0;
  for (int b = 31; b >= 0; --b) {
    const unsigned above = ~((2u << b) - 1u);   // the bits above b (b == 31: none)
    int zeros = 0;
    pf_slots<REG>(ns, [&](int s) {
      const unsigned v = key(s);
      zeros += __popcll(__ballot(((v ^ prefix) & above) == 0u && ((v >> b) & 1u) == 0u));
    });
    if (k > zeros) prefix |= 1u << b, k -= zeros;
  }
  kth = prefix, ties_in = k;
}

struct PfBlock {
  unsigned pos, tile;
  int lane, wave, status_in;
  const float *rows;
};

__device__ __forceinline__ PfBlock pf_block(const PfArgs &a) {
  PfBlock b;
  const int tid = threadIdx.x;
  b.lane = tid & 63;
  b.wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform, and known to be
  b.pos = blockIdx.x / a.tiles;
  b.tile = blockIdx.x - b.pos * a.tiles;
  b.status_in = a.status_in ? a.status_in[b.pos] : 0;
  b.rows = a.points + 3 * (int64_t)b.pos * a.pitch;
  return b;
}

// the element of channel `ch` and row `i` of position `pos`
__device__ __forceinline__ int64_t pf_at(const PfArgs &a, unsigned pos, int ch, int i) {
  const int64_t C = 4 * (int64_t)a.J;
  return a.layout == TSDF_POINTFIELD_CP ? ((int64_t)pos * C + ch) * a.P + i : ((int64_t)pos * a.P + i) * C + ch;
}

// one field value out: float32, or narrowed by round-to-nearest-even (v_cvt_f16_f32 with subnormals; v_cvt_pk_bf16_f32)
__device__ __forceinline__ void pf_store(void *out, int dtype, int64_t at, float v) {
  if (dtype == TSDF_POINTFIELD_F32) {
    static_cast<float *>(out)[at] = v;
  } else if (dtype == TSDF_POINTFIELD_F16) {
    static_cast<_Float16 *>(out)[at] = (_Float16)v;
  } else {
    static_cast<__bf16 *>(out)[at] = (__bf16)v;
  }
}

// one field value in, widened exactly
__device__ __forceinline__ float pf_load(const void *in, int dtype, int64_t at) {
  if (dtype == TSDF_POINTFIELD_F32) return static_cast<const float *>(in)[at];
  if (dtype == TSDF_POINTFIELD_F16) return (float)static_cast<const _Float16 *>(in)[at];
  return __uint_as_float((unsigned)static_cast<const unsigned short *>(in)[at] << 16);
}

template <bool REG>
__global__ __launch_bounds__(kPfWG) void tsdf_pointfield_encode_kernel(PfArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char pf_lds[];
  const PfBlock b = pf_block(a);
  const int lane = b.lane, P = a.P;
  const PfCloud cl = pf_stage(pf_lds, b.rows, P, b.status_in == 0, b.wave, lane);
  if (b.tile == 0 && threadIdx.x == 0)
    a.out_status[b.pos] = b.status_in != 0 ? b.status_in : cl.m == 0 ? TSDF_FRAME_DEGENERATE : TSDF_FRAME_OK;

  const int ns = pf_padded(P) / 64;
  const int j0 = (int)b.tile * kPfJoints + b.wave * kPfPerWave;   // tile < tiles: j0 < J + kPfJoints
  for (int kk = 0; kk < kPfPerWave && j0 + kk < a.J; ++kk) {
    const int j = j0 + kk;
    const int64_t jrow = (int64_t)b.pos * a.J + j;
    const float *q = a.joints + 3 * jrow;
    const float qx = q[0], qy = q[1], qz = q[2];   // uniform
    const bool live = cl.m > 0 && finite32(qx) && finite32(qy) && finite32(qz);   // m is 0 for a position that is not read
    if (lane == 0) a.out_valid[jrow] = live ? 1 : 0;

    // 2. the key of slot 64 s + lane: the bits of dist2
    auto compute = [&](int s) -> unsigned {
      const int i = 64 * s + lane;   // < pf_padded(P)
      const float px = cl.x[i];
      if (!(px == px)) return kPfNone;
      const float dx = qx - px, dy = qy - cl.y[i], dz = qz - cl.z[i];
      return __float_as_uint((dx * dx + dy * dy) + dz * dz);
    };
    unsigned kreg[REG ? kPfRegSlots : 1];
    auto key = [&](int s) -> unsigned {
      if constexpr (REG) return kreg[s];
      else return compute(s);
    };
    const bool all = a.K >= cl.m;   // the pure ball rule
    unsigned kth = kPfNone;
    int ties_in = 0;
    if (live) {
      if constexpr (REG) pf_slots<REG>(ns, [&](int s) { kreg[s] = compute(s); });
      if (!all) pf_select<REG>(ns, a.K, key, kth, ties_in);
    }

    // 4. the rows in order
    int ties = 0;
    pf_slots<REG>(ns, [&](int s) {
      const int i = 64 * s + lane;
      const unsigned v = live ? key(s) : kPfNone;
      const bool tie = v == kth;   // never for `all`: kth is kPfNone and such a slot is no member
      const unsigned long long tm = __ballot(tie);
      const bool in = v != kPfNone && (all || v < kth || (tie && ties + pf_below(tm) < ties_in));
      ties += __popcll(tm);
      float h = 0.f, vx = 0.f, vy = 0.f, vz = 0.f;
      if (in) {
        const float dist2 = __uint_as_float(v);
        const double d = __builtin_sqrt((double)dist2);
        if (d <= a.radius) {   // false for an infinite dist2
          const double t = d / a.radius;
          h = (float)(1.0 - t);
          if (dist2 != 0.f) {
            const float dx = qx - cl.x[i], dy = qy - cl.y[i], dz = qz - cl.z[i];
            vx = (float)((double)dx / d), vy = (float)((double)dy / d), vz = (float)((double)dz / d);
          }
        }
      }
      if (i < P) {
        pf_store(a.out_field, a.dtype, pf_at(a, b.pos, j, i), h);
        pf_store(a.out_field, a.dtype, pf_at(a, b.pos, a.J + 3 * j, i), vx);
        pf_store(a.out_field, a.dtype, pf_at(a, b.pos, a.J + 3 * j + 1, i), vy);
        pf_store(a.out_field, a.dtype, pf_at(a, b.pos, a.J + 3 * j + 2, i), vz);
      }
    });
  }
}

// v = v + v[lane ^ s] for s = 1 .. 32: the same bits in every lane
__device__ __forceinline__ double pf_tree(double v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v = v + __shfl_xor(v, s);
  return v;
}

template <bool REG>
__global__ __launch_bounds__(kPfWG) void tsdf_pointfield_decode_kernel(PfArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char pf_lds[];
  const PfBlock b = pf_block(a);
  const int lane = b.lane, P = a.P;
  const PfCloud cl = pf_stage(pf_lds, b.rows, P, b.status_in == 0, b.wave, lane);
  if (b.tile == 0 && threadIdx.x == 0)
    a.out_status[b.pos] = b.status_in != 0 ? b.status_in : cl.m == 0 ? TSDF_FRAME_DEGENERATE : TSDF_FRAME_OK;

  const int ns = pf_padded(P) / 64;
  const int j0 = (int)b.tile * kPfJoints + b.wave * kPfPerWave;
  for (int kk = 0; kk < kPfPerWave && j0 + kk < a.J; ++kk) {
    const int j = j0 + kk;
    const int64_t jrow = (int64_t)b.pos * a.J + j;
    const bool live = cl.m > 0;

    // 2. the key of slot 64 s + lane: the complement of the heat's order-preserving image, so that the greatest heat has
    // the smallest key; a NaN is kPfNanKey, above every number (-inf's key is 0xff800000)
    auto compute = [&](int s) -> unsigned {
      const int i = 64 * s + lane;   // < pf_padded(P); a slot >= P holds a NaN x
      const float px = cl.x[i];
      if (!(px == px)) return kPfNone;
      const float h = pf_load(a.field_in, a.dtype, pf_at(a, b.pos, j, i));
      if (!(h == h)) return kPfNanKey;
      const unsigned u = __float_as_uint(h);
      const unsigned image = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
      return ~image;
    };
    unsigned kreg[REG ? kPfRegSlots : 1];
    auto key = [&](int s) -> unsigned {
      if constexpr (REG) return kreg[s];
      else return compute(s);
    };
    const bool all = a.K >= cl.m;
    unsigned kth = kPfNone;
    int ties_in = 0;
    if (live) {
      if constexpr (REG) pf_slots<REG>(ns, [&](int s) { kreg[s] = compute(s); });
      if (!all) pf_select<REG>(ns, a.K, key, kth, ties_in);
    }

    // 4. the selected candidates in ascending order, each added in the lane of its compact index
    double sw = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
    int ties = 0, cands = 0;
    if (live) {
      pf_slots<REG>(ns, [&](int s) {
        const int i = 64 * s + lane;
        const unsigned v = key(s);
        const bool tie = v == kth;
        const unsigned long long tm = __ballot(tie), cm = __ballot(v != kPfNone);
        const bool sel = v != kPfNone && (all || v < kth || (tie && ties + pf_below(tm) < ties_in));
        const int c = cands + pf_below(cm);
        ties += __popcll(tm), cands += __popcll(cm);
        double w = 0.0, wx = 0.0, wy = 0.0, wz = 0.0;
        if (sel) {
          if (v != kPfNanKey) {
            const unsigned image = ~v;
            const float hf = __uint_as_float((image & 0x80000000u) ? (image ^ 0x80000000u) : ~image);
            const double h = (double)hf;
            w = h < 0.0 ? 0.0 : h > 1.0 ? 1.0 : h;
          }
          const double vx = (double)pf_load(a.field_in, a.dtype, pf_at(a, b.pos, a.J + 3 * j, i));
          const double vy = (double)pf_load(a.field_in, a.dtype, pf_at(a, b.pos, a.J + 3 * j + 1, i));
          const double vz = (double)pf_load(a.field_in, a.dtype, pf_at(a, b.pos, a.J + 3 * j + 2, i));
          const double nv = __builtin_sqrt((vx * vx + vy * vy) + vz * vz);
          const bool ok = nv > 0.0 && nv < __builtin_inf();   // false for a NaN
          const double ux = ok ? vx / nv : 0.0, uy = ok ? vy / nv : 0.0, uz = ok ? vz / nv : 0.0;
          const double reach = a.radius * (1.0 - w);
          const double ex = (double)cl.x[i] + reach * ux, ey = (double)cl.y[i] + reach * uy, ez = (double)cl.z[i] + reach * uz;
          wx = w * ex, wy = w * ey, wz = w * ez;
        }
        unsigned long long sm = __ballot(sel);
        while (sm != 0ull) {   // uniform
          const int from = __builtin_ctzll(sm);
          sm &= sm - 1ull;
          const int to = __shfl(c, from) & 63;
          const double bw = __shfl(w, from), bx = __shfl(wx, from), by = __shfl(wy, from), bz = __shfl(wz, from);
          if (lane == to) sw = sw + bw, sx = sx + bx, sy = sy + by, sz = sz + bz;
        }
      });
    }
    const double W = pf_tree(sw), X = pf_tree(sx), Y = pf_tree(sy), Z = pf_tree(sz);
    if (lane == 0) {
      const bool have = W != 0.0;   // W is a sum of values in [0, 1]: never a NaN
      a.out_joints[3 * jrow] = have ? (float)(X / W) : 0.f;
      a.out_joints[3 * jrow + 1] = have ? (float)(Y / W) : 0.f;
      a.out_joints[3 * jrow + 2] = have ? (float)(Z / W) : 0.f;
      a.out_weight[jrow] = have ? (float)W : 0.f;
    }
  }
}

// A kernel that asks for more than 64 KiB of dynamic LDS must be told so once per device (host state, not a stream
// operation: a captured launch stays self-contained).
template <typename Kernel>
int pf_launch(Kernel kernel, std::atomic<int> *told, const PfArgs &a, int n, void *hip_stream) {
  int dev = 0;
  const int rc = check_device(&dev);
  if (rc != TSDF_OK) return rc;
  const PfPlan p = pf_plan(a.P, a.J);
  if (p.lds_bytes > 64 * 1024) {
    const bool cached = dev >= 0 && dev < 64;
    if (!cached || told[dev].load(std::memory_order_relaxed) == 0) {
      if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              12 * TSDF_POINTFIELD_MAX_CLOUD + kPfTailBytes) != hipSuccess) {
        (void)hipGetLastError();
        return TSDF_ERR_LAUNCH;
      }
      if (cached) told[dev].store(1, std::memory_order_relaxed);
    }
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)n * (unsigned)p.groups), dim3(kPfWG), (size_t)p.lds_bytes,
                     static_cast<hipStream_t>(hip_stream), a);
  return launched();
}

PfArgs pf_args(const PfIn &c, const int32_t *status_in, int32_t *status) {
  PfArgs a = {};
  a.points = c.points, a.pitch = c.pitch, a.status_in = status_in;
  a.P = c.P, a.J = c.J, a.K = c.K, a.tiles = (unsigned)pf_plan(c.P, c.J).groups;
  a.radius = c.radius, a.layout = c.layout, a.dtype = c.dtype;
  a.out_status = status;
  return a;
}

}  // namespace

extern "C" {

int tsdf_pointfield_version(void) { return TSDF_POINTFIELD_VERSION; }

int tsdf_pointfield_plan(int P, int J, int K, int *lds_bytes, int *joints_per_group, int *groups_per_position) {
  if (pf_shape_defect(P, J, K, TSDF_POINTFIELD_MAX_K) != kPfGood || !lds_bytes || !joints_per_group || !groups_per_position)
    return TSDF_ERR_INVALID_ARG;
  const PfPlan p = pf_plan(P, J);
  *lds_bytes = p.lds_bytes;
  *joints_per_group = p.joints;
  *groups_per_position = p.groups;
  return TSDF_OK;
}

int tsdf_pointfield_encode_hip(const float *d_points, int64_t pitch, const float *d_joints, const int32_t *d_status_in,
                               int n, int P, int J, int K, double radius, int layout, int dtype, void *hip_stream,
                               void *d_out_field, int32_t *d_out_valid, int32_t *d_out_status) {
  // arguments first, then the device, then the launch
  const PfIn c = {d_points, pitch, n, P, J, K, radius, layout, dtype, d_out_status};
  const PfDefect bad = pf_encode_defect(c, d_joints, d_out_field, d_out_valid);
  if (bad != kPfGood) return pf_status(bad);
  PfArgs a = pf_args(c, d_status_in, d_out_status);
  a.joints = d_joints, a.out_field = d_out_field, a.out_valid = d_out_valid;
  static std::atomic<int> told[2][64];
  return P <= 64 * kPfRegSlots ? pf_launch(tsdf_pointfield_encode_kernel<true>, told[0], a, n, hip_stream)
                               : pf_launch(tsdf_pointfield_encode_kernel<false>, told[1], a, n, hip_stream);
}

int tsdf_pointfield_decode_hip(const float *d_points, int64_t pitch, const void *d_field, const int32_t *d_status_in,
                               int n, int P, int J, int M, double radius, int layout, int dtype, void *hip_stream,
                               float *d_out_joints, float *d_out_weight, int32_t *d_out_status) {
  const PfIn c = {d_points, pitch, n, P, J, M, radius, layout, dtype, d_out_status};
  const PfDefect bad = pf_decode_defect(c, d_field, d_out_joints, d_out_weight);
  if (bad != kPfGood) return pf_status(bad);
  PfArgs a = pf_args(c, d_status_in, d_out_status);
  a.field_in = d_field, a.out_joints = d_out_joints, a.out_weight = d_out_weight;
  static std::atomic<int> told[2][64];
  return P <= 64 * kPfRegSlots ? pf_launch(tsdf_pointfield_decode_kernel<true>, told[0], a, n, hip_stream)
                               : pf_launch(tsdf_pointfield_decode_kernel<false>, told[1], a, n, hip_stream);
}

}  // extern "C"
