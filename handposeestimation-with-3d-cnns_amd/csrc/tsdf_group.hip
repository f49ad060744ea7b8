// tsdf_group.hip — libtsdf_group.so: kNN grouping and PCA surface normals of sampled clouds
// (include/tsdf_group.h, which has the contract operation by operation).
//
// A translation unit and a library of its own, next to libtsdf_hip.so and the other libraries (all frozen).  It takes the
// status codes from include/tsdf.h, the host preamble every library here has from device.inc, finite32 from prim.inc and
// its argument rules and its plan from group_host.inc, plain C++ that is also built on its own under the CPU sanitizers.
// No device global and no global atomic: every launch is self-contained.
//
// Both kernels are a top-K selection per query over a cloud resident in LDS.  A workgroup of kGrpWG threads serves
// kGrpQueries queries of ONE batch position; the grid is one-dimensional, block b is tile b % tiles of position b / tiles.
//   1. STAGE.  Wave w walks its piece of the cloud's rows (group_host.inc::grp_segment) 64 at a time and counts the
//      candidates by ballot; the waves' counts meet in LDS: their sum is m, their prefix the wave's first compact index.
//      The same walk again stores candidate c into three float32 arrays in (dynamic) LDS.  The pieces are in row order,
//      so compact index c orders as rank does and "lowest rank" is "lowest c".
//   2. SEARCH (grp_search), no barrier inside.  One wave owns a query at a time; the query's coordinates are uniform.
//      Each step takes 64 consecutive candidates, one a lane, and computes their keys, (dist bits) << 32 | c.  A ballot
//      against the current K-th key skips the step when no key beats it.  Otherwise the 64 keys are bitonic-sorted
//      across the wave and merged into the running sorted list (one key a lane for K <= 64, two for K <= 128): the
//      element-wise minimum against the reversed new keys is a bitonic sequence of the smallest, which a bitonic merge
//      sorts.  A slot without a key holds all ones, above every key.
//   3a. kNN: slot j of the list is row j of the query; the offsets are recomputed from LDS by the same expressions.
//       The rows hold compact indices; when rows were dropped (m < P) the walk runs a third time, stores every
//       candidate's rank where its x was, and every lane replaces the indices it wrote itself.
//   3b. normals: the tree sums of the contract over the list's slots give the query's covariance, which lane j of the
//       wave keeps for the wave's query j; after the wave's last query the Jacobi runs once, one query a lane.
// All global indexing is in 64 bits.  Compiled with -ffp-contract=off: no fused multiply-add anywhere in this file.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "../../include/tsdf_group.h"

namespace {

#include "device.inc"      // check_device, launched, misaligned: the host preamble of every library here
#include "prim.inc"        // finite32
#include "group_host.inc"  // grp_knn_defect, grp_normals_defect, grp_plan, grp_padded, grp_segment, kGrpWG

typedef unsigned long long grp_key;
constexpr grp_key kGrpNone = ~0ull;   // a slot without a key: above every key (dist bits are at most +inf's)

struct GrpArgs {
  const float *points;      // [n][pitch][3]
  int64_t pitch;
  const float *query;       // [n][C][3] or null
  const int32_t *status_in; // [n] or null
  const double *view;       // [n][3] or null
  int P, C, K;
  unsigned tiles;           // workgroups per position
  int32_t *out_index;       // kNN: [n][C][K]
  float *out_dist2;         // [n][C][K] or null
  float *out_offset;        // [n][C][K][3] or null
  float *out_normals;       // normals: [n][C][3]
  float *out_curv;          // [n][C] or null
  int32_t *out_status;      // [n]
};

// The wave's piece of the rows, 64 at a time: sink(c, rank, x, y, z) for every candidate, c counting up from `base` in
// row order.  Returns the piece's candidates.  Every lane of the wave runs every step (the bounds are the wave's).
template <typename Sink>
__device__ __forceinline__ int grp_walk(const float *rows, int P, int seg, int wave, int lane, int base, Sink sink) {
  const int b = wave * seg, e = b + seg < P ? b + seg : P;
  int run = base;
  for (int i0 = b; i0 < e; i0 += 64) {
    const int it = i0 + lane;
    float x = 0.f, y = 0.f, z = 0.f;
    bool cand = false;
    if (it < e) {
      const float *r = rows + 3 * (int64_t)it;
      x = r[0], y = r[1], z = r[2];
      cand = finite32(x) && finite32(y) && finite32(z);
    }
    const unsigned long long m = __ballot(cand);
    if (cand) sink(run + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)), it, x, y, z);
    run += __popcll(m);
  }
  return run - base;
}

// What a workgroup holds of its position: the candidates in LDS, their number, this wave's first compact index.
struct GrpCloud {
  float *x, *y, *z;   // [grp_padded(P)] each; x is the candidates' ranks after grp_ranks
  int m, base;
};

// 1. count, 2. compact.  `read` false (a position with an input status): nothing is read and m is 0.
__device__ __forceinline__ GrpCloud grp_stage(char *lds, const float *rows, int P, bool read, int wave, int lane) {
  const int pad = grp_padded(P);
  GrpCloud c;
  c.x = reinterpret_cast<float *>(lds), c.y = c.x + pad, c.z = c.y + pad;
  c.m = c.base = 0;
  if (!read) return c;   // uniform
  int *s_cnt = reinterpret_cast<int *>(c.z + pad);
  const int seg = grp_segment(P);
  const int mine = grp_walk(rows, P, seg, wave, lane, 0, [](int, int, float, float, float) {});
  if (lane == 0) s_cnt[wave] = mine;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kGrpWaves; ++w) {
    const int v = s_cnt[w];
    c.base += w < wave ? v : 0;
    c.m += v;
  }
  grp_walk(rows, P, seg, wave, lane, c.base, [&](int k, int, float x, float y, float z) { c.x[k] = x, c.y[k] = y, c.z[k] = z; });
  __syncthreads();
  return c;
}

__device__ __forceinline__ grp_key grp_min(grp_key a, grp_key b) { return b < a ? b : a; }
__device__ __forceinline__ grp_key grp_max(grp_key a, grp_key b) { return b < a ? a : b; }

// The key of lane ^ J.  Within a row of 16 lanes the exchanges of 1, 2 and 8 lanes are DPP moves (quad_perm [1,0,3,2],
// quad_perm [2,3,0,1], row_ror:8 — each its own inverse); the others go through the LDS crossbar.
template <int J>
__device__ __forceinline__ grp_key grp_other(grp_key v, int lane) {
  const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
  unsigned olo, ohi;
  if constexpr (J == 1 || J == 2 || J == 8) {
    constexpr int ctrl = J == 1 ? 0xB1 : J == 2 ? 0x4E : 0x128;
    olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, ctrl, 0xf, 0xf, false);
    ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, ctrl, 0xf, 0xf, false);
  } else {
    const int at = (lane ^ J) << 2;
    olo = (unsigned)__builtin_amdgcn_ds_bpermute(at, lo);
    ohi = (unsigned)__builtin_amdgcn_ds_bpermute(at, hi);
  }
  return ((grp_key)ohi << 32) | olo;
}

// One compare-exchange of a sorting network with lane ^ J: a lane of `smaller` keeps the smaller of the two keys, any
// other the greater.  One 64-bit comparison and one select: the other's key is taken iff "it is smaller" is what the lane
// wants (of equal keys, which only empty slots are, either will do).
template <int J>
__device__ __forceinline__ grp_key grp_exchange(grp_key v, int lane, bool smaller) {
  const grp_key o = grp_other<J>(v, lane);
  return (o < v) == smaller ? o : v;
}

// a bitonic sequence of 2 * J keys into order, ascending in the lanes where `lane & K` is 0 and descending in the others
// (K = 64: ascending everywhere)
template <int K, int J>
__device__ __forceinline__ grp_key grp_merge(grp_key v, int lane) {
  v = grp_exchange<J>(v, lane, ((lane & K) == 0) == ((lane & J) == 0));
  if constexpr (J > 1) v = grp_merge<K, J / 2>(v, lane);
  return v;
}

// 64 keys, one a lane, in ascending order by lane: the bitonic sorting network, 21 exchanges
__device__ __forceinline__ grp_key grp_sort64(grp_key v, int lane) {
  v = grp_merge<2, 1>(v, lane);
  v = grp_merge<4, 2>(v, lane);
  v = grp_merge<8, 4>(v, lane);
  v = grp_merge<16, 8>(v, lane);
  v = grp_merge<32, 16>(v, lane);
  return grp_merge<64, 32>(v, lane);
}

// a bitonic sequence of 64 keys into ascending order: 6 exchanges
__device__ __forceinline__ grp_key grp_merge64(grp_key v, int lane) { return grp_merge<64, 32>(v, lane); }

// 2. the K smallest keys of the cloud for the query (qx, qy, qz), ascending: slot j in r[j / 64] of lane j % 64.
template <int NL>
__device__ __forceinline__ void grp_search(const GrpCloud &cl, float qx, float qy, float qz, int K, int lane, grp_key (&r)[NL]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int l = 0; l < NL; ++l) r[l] = kGrpNone;
  grp_key kth = kGrpNone;   // slot K - 1: what a key must beat
  for (int c0 = 0; c0 < cl.m; c0 += 64) {
    const int c = c0 + lane;   // < grp_padded(P)
    grp_key key = kGrpNone;
    if (c < cl.m) {
      const float dx = cl.x[c] - qx, dy = cl.y[c] - qy, dz = cl.z[c] - qz;
      const float d = (dx * dx + dy * dy) + dz * dz;
      key = ((grp_key)__float_as_uint(d) << 32) | (unsigned)c;
    }
    if (__ballot(key < kth) == 0ull) continue;   // uniform
    key = grp_sort64(key, lane);
    const grp_key rev = __shfl(key, 63 - lane);
    if constexpr (NL == 1) {
      r[0] = grp_merge64(grp_min(r[0], rev), lane);
    } else {
      // the new keys as 128, padded with empty slots and reversed: the low half's minimum is the list's own
      const grp_key h = grp_min(r[1], rev);
      const grp_key lo = grp_min(r[0], h), hi = grp_max(r[0], h);
      r[0] = grp_merge64(lo, lane);
      r[1] = grp_merge64(hi, lane);
    }
    grp_key last = r[0];
    if constexpr (NL == 2) last = K > 64 ? r[1] : r[0];
    kth = __shfl(last, (K - 1) & 63);
  }
}

// the query of row `q` of the position: false when it gives a "no result" row
__device__ __forceinline__ bool grp_query(const GrpArgs &a, const float *rows, int64_t row, int q, int m, float &qx, float &qy, float &qz) {
  qx = qy = qz = 0.f;
  if (m == 0) return false;   // also a position that is not read
  const float *p = a.query ? a.query + 3 * row : rows + 3 * (int64_t)q;   // q < C <= P without a.query
  qx = p[0], qy = p[1], qz = p[2];
  return finite32(qx) && finite32(qy) && finite32(qz);
}

struct GrpBlock {
  unsigned pos, tile;
  int lane, wave, status_in;
  const float *rows;
};

__device__ __forceinline__ GrpBlock grp_block(const GrpArgs &a) {
  GrpBlock b;
  const int tid = threadIdx.x;
  b.lane = tid & 63;
  b.wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform, and known to be
  b.pos = blockIdx.x / a.tiles;
  b.tile = blockIdx.x - b.pos * a.tiles;
  b.status_in = a.status_in ? a.status_in[b.pos] : 0;
  b.rows = a.points + 3 * (int64_t)b.pos * a.pitch;
  return b;
}

template <int NL>
__global__ __launch_bounds__(kGrpWG) void tsdf_knn_kernel(GrpArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char grp_lds[];
  const GrpBlock b = grp_block(a);
  const int lane = b.lane, K = a.K;
  const GrpCloud cl = grp_stage(grp_lds, b.rows, a.P, b.status_in == 0, b.wave, lane);
  if (b.tile == 0 && threadIdx.x == 0)
    a.out_status[b.pos] = b.status_in != 0 ? b.status_in : cl.m == 0 ? TSDF_FRAME_DEGENERATE : TSDF_FRAME_OK;

  const int q0 = (int)b.tile * kGrpQueries + b.wave * kGrpPerWave;   // tile < tiles: q0 < C + kGrpQueries
  for (int k = 0; k < kGrpPerWave && q0 + k < a.C; ++k) {
    const int q = q0 + k;
    const int64_t row = (int64_t)b.pos * a.C + q;
    float qx, qy, qz;
    const bool live = grp_query(a, b.rows, row, q, cl.m, qx, qy, qz);   // uniform
    grp_key r[NL];
    if (live) grp_search<NL>(cl, qx, qy, qz, K, lane, r);
    const grp_key first = live ? __shfl(r[0], 0) : 0ull;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const int j = l * 64 + lane;
      if (j >= K) continue;
      const int64_t at = row * K + j;
      int idx = -1;
      float d = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
      if (live) {
        const grp_key key = r[l] == kGrpNone ? first : r[l];   // slots m..K-1 repeat slot 0
        idx = (int)(unsigned)key;                              // < m
        d = __uint_as_float((unsigned)(key >> 32));
        dx = cl.x[idx] - qx, dy = cl.y[idx] - qy, dz = cl.z[idx] - qz;
      }
      a.out_index[at] = idx;
      if (a.out_dist2) a.out_dist2[at] = d;
      if (a.out_offset) a.out_offset[3 * at] = dx, a.out_offset[3 * at + 1] = dy, a.out_offset[3 * at + 2] = dz;
    }
  }

  // 3a. ranks where x was: only when rows were dropped, else the compact index is the rank
  if (cl.m == a.P || cl.m == 0) return;   // uniform for the workgroup
  __syncthreads();   // every wave has read its last coordinates
  int *s_rank = reinterpret_cast<int *>(cl.x);
  grp_walk(b.rows, a.P, grp_segment(a.P), b.wave, lane, cl.base, [&](int c, int rank, float, float, float) { s_rank[c] = rank; });
  __syncthreads();
  for (int k = 0; k < kGrpPerWave && q0 + k < a.C; ++k) {
    const int64_t row = (int64_t)b.pos * a.C + q0 + k;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const int j = l * 64 + lane;
      if (j >= K) continue;
      const unsigned c = (unsigned)a.out_index[row * K + j];   // this lane's own store
      if (c < (unsigned)cl.m) a.out_index[row * K + j] = s_rank[c];   // a "no result" row keeps its -1
    }
  }
}

// v = v + v[lane ^ s] for s = 1 .. 32: the same bits in every lane
__device__ __forceinline__ double grp_tree(double v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v = v + __shfl_xor(v, s);
  return v;
}

// tsdf_obb.hip's jacobi_rot, restated: one rotation of the pair (p, q), r the third index
__device__ __forceinline__ void grp_rot(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p,
                                        double &v0q, double &v1p, double &v1q, double &v2p, double &v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double th2 = theta * theta;
  double t = 1.0 / (__builtin_fabs(theta) + __builtin_sqrt(th2 + 1.0));
  if (theta < 0.0) t = -t;
  const double t2 = t * t;
  const double c = 1.0 / __builtin_sqrt(t2 + 1.0);
  const double s = t * c;
  const double tp = t * apq;
  app = app - tp;
  aqq = aqq + tp;
  apq = 0.0;
  const double rp = arp, rq = arq;
  const double crp = c * rp, srq = s * rq, srp = s * rp, crq = c * rq;
  arp = crp - srq;
  arq = srp + crq;
#define GRP_ROT_V(vp, vq)                              \
  {                                                    \
    const double a_ = vp, b_ = vq;                     \
    const double ca_ = c * a_, sb_ = s * b_;           \
    const double sa_ = s * a_, cb_ = c * b_;           \
    vp = ca_ - sb_;                                    \
    vq = sa_ + cb_;                                    \
  }
  GRP_ROT_V(v0p, v0q)
  GRP_ROT_V(v1p, v1q)
  GRP_ROT_V(v2p, v2q)
#undef GRP_ROT_V
}

template <int NL>
__global__ __launch_bounds__(kGrpWG) void tsdf_normals_kernel(GrpArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char grp_lds[];
  const GrpBlock b = grp_block(a);
  const int lane = b.lane, K = a.K;
  const GrpCloud cl = grp_stage(grp_lds, b.rows, a.P, b.status_in == 0, b.wave, lane);
  if (b.tile == 0 && threadIdx.x == 0)
    a.out_status[b.pos] = b.status_in != 0 ? b.status_in : cl.m == 0 ? TSDF_FRAME_DEGENERATE : TSDF_FRAME_OK;

  // lane k: the wave's query k — its covariance, itself widened, and its m' (-1: a "no result" row)
  double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, ox = 0.0, oy = 0.0, oz = 0.0;
  int mk = -1;
  const int q0 = (int)b.tile * kGrpQueries + b.wave * kGrpPerWave;
  const int mp = K < cl.m ? K : cl.m;   // m'
  for (int k = 0; k < kGrpPerWave && q0 + k < a.C; ++k) {
    const int q = q0 + k;
    float qx, qy, qz;
    if (!grp_query(a, b.rows, (int64_t)b.pos * a.C + q, q, cl.m, qx, qy, qz)) continue;   // uniform
    grp_key r[NL];
    grp_search<NL>(cl, qx, qy, qz, K, lane, r);
    // slot `lane` and slot `lane + 64`; a slot >= m' contributes +0.0
    double px0 = 0.0, py0 = 0.0, pz0 = 0.0, px1 = 0.0, py1 = 0.0, pz1 = 0.0;
    const bool have0 = lane < mp, have1 = NL == 2 && 64 + lane < mp;
    if (have0) {
      const unsigned c = (unsigned)r[0];   // < m
      px0 = (double)cl.x[c], py0 = (double)cl.y[c], pz0 = (double)cl.z[c];
    }
    if constexpr (NL == 2) {
      if (have1) {
        const unsigned c = (unsigned)r[1];
        px1 = (double)cl.x[c], py1 = (double)cl.y[c], pz1 = (double)cl.z[c];
      }
    }
    const double cnt = (double)mp;
    const double mx = grp_tree(px0 + px1) / cnt, my = grp_tree(py0 + py1) / cnt, mz = grp_tree(pz0 + pz1) / cnt;
    const double ex0 = px0 - mx, ey0 = py0 - my, ez0 = pz0 - mz, ex1 = px1 - mx, ey1 = py1 - my, ez1 = pz1 - mz;
#define GRP_COV(u, v) (grp_tree((have0 ? u##0 * v##0 : 0.0) + (have1 ? u##1 * v##1 : 0.0)) / cnt)
    const double cxx = GRP_COV(ex, ex), cxy = GRP_COV(ex, ey), cxz = GRP_COV(ex, ez);
    const double cyy = GRP_COV(ey, ey), cyz = GRP_COV(ey, ez), czz = GRP_COV(ez, ez);
#undef GRP_COV
    if (lane == k) {
      a00 = cxx, a01 = cxy, a02 = cxz, a11 = cyy, a12 = cyz, a22 = czz;
      ox = (double)qx, oy = (double)qy, oz = (double)qz;
      mk = mp;
    }
  }

  // 3b. one query a lane
  if (lane >= kGrpPerWave || q0 + lane >= a.C) return;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < TSDF_GROUP_SWEEPS; ++sweep) {
    grp_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0,1), r = 2
    grp_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0,2), r = 1
    grp_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1,2), r = 0
  }
  // the smallest diagonal element, ties to the lowest column
  const bool col1 = a11 < a00;
  const bool col2 = a22 < (col1 ? a11 : a00);
  double nx = col2 ? v02 : col1 ? v01 : v00, ny = col2 ? v12 : col1 ? v11 : v10, nz = col2 ? v22 : col1 ? v21 : v20;
  // towards the viewpoint
  const double *view = a.view ? a.view + 3 * (int64_t)b.pos : nullptr;
  const double wx = (view ? view[0] : 0.0) - ox, wy = (view ? view[1] : 0.0) - oy, wz = (view ? view[2] : 0.0) - oz;
  const double d = (nx * wx + ny * wy) + nz * wz;
  if (d < 0.0) nx = -nx, ny = -ny, nz = -nz;
  // the diagonal ascending: exchanges (0,1), (1,2), (0,1)
  double l0 = a00, l1 = a11, l2 = a22;
#define GRP_ORDER(u, v)                                       \
  {                                                           \
    const double lo_ = v < u ? v : u, hi_ = v < u ? u : v;    \
    u = lo_, v = hi_;                                         \
  }
  GRP_ORDER(l0, l1)
  GRP_ORDER(l1, l2)
  GRP_ORDER(l0, l1)
#undef GRP_ORDER
  const double sum = (l0 + l1) + l2;
  double curv = sum == 0.0 ? 0.0 : l0 / sum;
  if (mk < 3) nx = ny = nz = curv = 0.0;   // also a "no result" row
  const int64_t row = (int64_t)b.pos * a.C + q0 + lane;
  a.out_normals[3 * row] = (float)nx, a.out_normals[3 * row + 1] = (float)ny, a.out_normals[3 * row + 2] = (float)nz;
  if (a.out_curv) a.out_curv[row] = (float)curv;
}

// A kernel that asks for more than 64 KiB of dynamic LDS must be told so once per device (host state, not a stream
// operation: a captured launch stays self-contained).
template <typename Kernel>
int grp_launch(Kernel kernel, std::atomic<int> *told, const GrpArgs &a, int n, void *hip_stream) {
  int dev = 0;
  const int rc = check_device(&dev);
  if (rc != TSDF_OK) return rc;
  const GrpPlan p = grp_plan(a.P, a.C);
  if (p.lds_bytes > 64 * 1024) {
    const bool cached = dev >= 0 && dev < 64;
    if (!cached || told[dev].load(std::memory_order_relaxed) == 0) {
      if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              12 * TSDF_GROUP_MAX_CLOUD + kGrpTailBytes) != hipSuccess) {
        (void)hipGetLastError();
        return TSDF_ERR_LAUNCH;
      }
      if (cached) told[dev].store(1, std::memory_order_relaxed);
    }
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)n * (unsigned)p.groups), dim3(kGrpWG), (size_t)p.lds_bytes,
                     static_cast<hipStream_t>(hip_stream), a);
  return launched();
}

GrpArgs grp_args(const GrpIn &c, const int32_t *status_in, int32_t *status) {
  GrpArgs a = {};
  a.points = c.points, a.pitch = c.pitch, a.query = c.query, a.status_in = status_in;
  a.P = c.P, a.C = c.C, a.K = c.K, a.tiles = (unsigned)grp_plan(c.P, c.C).groups;
  a.out_status = status;
  return a;
}

}  // namespace

extern "C" {

int tsdf_group_version(void) { return TSDF_GROUP_VERSION; }

int tsdf_group_plan(int P, int C, int K, int *lds_bytes, int *queries_per_group, int *groups_per_position) {
  if (grp_shape_defect(P, C, K) != kGrpGood || !lds_bytes || !queries_per_group || !groups_per_position)
    return TSDF_ERR_INVALID_ARG;
  const GrpPlan p = grp_plan(P, C);
  *lds_bytes = p.lds_bytes;
  *queries_per_group = p.queries;
  *groups_per_position = p.groups;
  return TSDF_OK;
}

int tsdf_knn_hip(const float *d_points, int64_t pitch, const float *d_query, const int32_t *d_status_in, int n, int P,
                 int C, int K, void *hip_stream, int32_t *d_out_index, float *d_out_dist2, float *d_out_offset,
                 int32_t *d_out_status) {
  // arguments first, then the device, then the launch
  const GrpIn c = {d_points, pitch, d_query, n, P, C, K, d_out_status};
  const GrpDefect bad = grp_knn_defect(c, d_out_index, d_out_dist2, d_out_offset);
  if (bad != kGrpGood) return grp_status(bad);
  GrpArgs a = grp_args(c, d_status_in, d_out_status);
  a.out_index = d_out_index, a.out_dist2 = d_out_dist2, a.out_offset = d_out_offset;
  static std::atomic<int> told[2][64];
  return K <= 64 ? grp_launch(tsdf_knn_kernel<1>, told[0], a, n, hip_stream)
                 : grp_launch(tsdf_knn_kernel<2>, told[1], a, n, hip_stream);
}

int tsdf_normals_hip(const float *d_points, int64_t pitch, const float *d_query, const int32_t *d_status_in,
                     const double *d_view, int n, int P, int C, int K, void *hip_stream, float *d_out_normals,
                     float *d_out_curvature, int32_t *d_out_status) {
  const GrpIn c = {d_points, pitch, d_query, n, P, C, K, d_out_status};
  const GrpDefect bad = grp_normals_defect(c, d_view, d_out_normals, d_out_curvature);
  if (bad != kGrpGood) return grp_status(bad);
  GrpArgs a = grp_args(c, d_status_in, d_out_status);
  a.view = d_view, a.out_normals = d_out_normals, a.out_curv = d_out_curvature;
  static std::atomic<int> told[2][64];
  return K <= 64 ? grp_launch(tsdf_normals_kernel<1>, told[0], a, n, hip_stream)
                 : grp_launch(tsdf_normals_kernel<2>, told[1], a, n, hip_stream);
}

}  // extern "C"
