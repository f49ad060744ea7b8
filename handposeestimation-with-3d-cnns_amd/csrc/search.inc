// search.inc — what the two ACCURATE kernels share beyond slab.inc: tsdf_accurate.hip and tsdf_mapaccurate.hip include it
// (after slab.inc, inside their anonymous namespace); nothing else does.  Such a kernel walks, per item of V voxels of the
// fastest axis, a pixel rectangle of the crop and keeps per voxel the pixel of smallest s = tx^2 + ty^2 + tz^2 (t: voxel
// minus surface point over the truncation distance T, in float64).  What is the same for both is here:
//   acc_f4, acc_i4, V    an item: 4 voxels per lane, one 16-byte store per channel
//   clip_lo, clip_hi     a window bound clipped to the crop as an int; a NaN selects the whole side
//   search_rect          the corner-quotient rectangle of camera-frame ranges x, y and a depth interval
//   search_bad_frame     slab_bad_frame, and `nearest` = -1 over the slab of a frame that is not OK
//   search_store         an item's three channel vectors and its `nearest` vector
//   search_halve         host: slab.inc's plan halved down to kMinBlocks workgroups
//   search_launch        host: the layout's instantiation on the stream
// The projection, gather and sign, the walk, the value evaluation and the tail of the argument struct stay in each file:
// they differ in arithmetic, not in names.
//
// WHAT MAY BE DISCARDED BEFORE s IS EVALUATED.  The contracts allow only candidates whose evaluated s provably exceeds
// min(1, best so far).  A candidate with s > 1 never decides anything: if the true minimum is <= 1 the minimiser and every
// pixel that ties with it have s <= 1, and if it is > 1 the voxel is far and names no pixel.  Two tests use that:
//   The z term.  Both kernels evaluate s = fma(tz, tz, fma(ty, ty, tx * tx)), and the argument does not look at how tz
//     came about.  For a float64 |tz| > 1, tz^2 >= (1 + 2^-52)^2 > 1 + 2^-52, the inner fma is the rounding of a
//     non-negative real and so >= 0, and rounding is monotone: the evaluated s would be >= 1 + 2^-52 > 1.  Skipping on
//     !(|tz| <= 1) therefore skips exactly candidates whose EVALUATED s exceeds 1 (or is a NaN, which wins no comparison):
//     no margin is needed.
//   The rectangle.  Let a point w within T of the voxel have its camera-frame coordinates bounded: w_x in [xa, xb], w_y in
//     [ya, yb] and its depth d = -w_z in [dlo, dhi] (each file says why its six arguments are such bounds).  Its pixel is
//     col = cx + F * w_x / d, row = cy - F * w_y / d: quotients that are monotone in the numerator and in d separately
//     while d keeps one sign, so over the box their extremes are at the four corners.  The callers pass the bounds for
//     T' = T * (1 + 2^-20) and, for the V voxels of an item, the union of their ranges; search_rect rounds the corner
//     values outwards by floor - 1 / ceil + 1 (+ 2: the upper bounds are exclusive) and clips to the crop.  A pixel outside
//     has a real |t| > 1 + 2^-20 in some coordinate, a real s > 1 + 2^-19, and with the contracts' evaluation error of
//     2^-40 (relative beyond s = 2) an evaluated s > 1.  The corner values carry a few roundings of relative 2^-53 on pixel
//     coordinates that matter only inside the crop, i.e. below 2^31: far less than the one pixel added; a NaN bound (cx or
//     cy is not judged) selects the whole side.
//     A valid pixel has |d| >= eps.  When [dlo, dhi] does not stay on one side of zero by eps the quotient is unbounded:
//     there is NO finite rectangle and the whole crop is walked.
// The operation order of search_rect is part of that count of roundings (-ffp-contract=off): do not reassociate it.

typedef float acc_f4 __attribute__((ext_vector_type(4)));
typedef int acc_i4 __attribute__((ext_vector_type(4)));

constexpr int V = 4;   // voxels per lane and item: one 16-byte store per channel
constexpr int64_t kMinBlocks = 1024;   // workgroups a launch aims for at least: four per CU of an MI355X

// lower clip of a window bound: max(lo, min(hi, b)) as an int; a NaN gives lo (the whole side)
__device__ __forceinline__ int clip_lo(double b, int lo, int hi) {
  return !(b > (double)lo) ? lo : (b < (double)hi ? trunc_i32(b) : hi);
}

// upper clip: min(hi, max(lo, b)); a NaN gives hi
__device__ __forceinline__ int clip_hi(double b, int lo, int hi) {
  return !(b < (double)hi) ? hi : (b > (double)lo ? trunc_i32(b) : lo);
}

struct SearchRect {
  int c0, c1, r0, r1;   // columns [c0, c1) x rows [r0, r1), image coordinates
};

// The pixels of the crop [left, right) x [top, bottom) that a point with w_x in [xa, xb], w_y in [ya, yb] and depth in
// [dlo, dhi] can project to; the whole crop where the depth interval does not stay epsd away from zero on one side.
__device__ __forceinline__ SearchRect search_rect(double xa, double xb, double ya, double yb, double dlo, double dhi,
                                                  double epsd, double F, double cx, double cy, int left, int top,
                                                  int right, int bottom) {
#pragma clang fp contract(off)
  SearchRect w = {left, right, top, bottom};
  if (dlo >= epsd || dhi <= -epsd) {                           // one sign, away from zero: a finite rectangle
    const double i0 = 1.0 / dlo, i1 = 1.0 / dhi;
    const double x00 = xa * i0, x01 = xa * i1, x10 = xb * i0, x11 = xb * i1;
    const double y00 = ya * i0, y01 = ya * i1, y10 = yb * i0, y11 = yb * i1;
    const double qxlo = __builtin_fmin(__builtin_fmin(x00, x01), __builtin_fmin(x10, x11));
    const double qxhi = __builtin_fmax(__builtin_fmax(x00, x01), __builtin_fmax(x10, x11));
    const double qylo = __builtin_fmin(__builtin_fmin(y00, y01), __builtin_fmin(y10, y11));
    const double qyhi = __builtin_fmax(__builtin_fmax(y00, y01), __builtin_fmax(y10, y11));
    // col = cx + F * (w_x / d), row = cy - F * (w_y / d); outwards by one pixel beyond floor / ceil
    w.c0 = clip_lo(__builtin_floor(cx + F * qxlo) - 1.0, left, right);
    w.c1 = clip_hi(__builtin_ceil(cx + F * qxhi) + 2.0, left, right);
    w.r0 = clip_lo(__builtin_floor(cy - F * qyhi) - 1.0, top, bottom);
    w.r1 = clip_hi(__builtin_ceil(cy - F * qylo) + 2.0, top, bottom);
  }
  return w;
}

// slab_bad_frame for a kernel that also writes `nearest` (the position's [R][R][R], or null): a frame that is not OK has
// -1 there over the slab.  True: the kernel returns.
__device__ __forceinline__ bool search_bad_frame(const SlabFrame &fr, const Slab &blk, int32_t *status, float *out,
                                                 int32_t *nearest, int R, int64_t per, int tid) {
  if (!slab_bad_frame<acc_f4>(fr, blk, status, out, R, per, tid)) return false;
  if (nearest) {
    const acc_i4 none = {-1, -1, -1, -1};
    acc_i4 *p = reinterpret_cast<acc_i4 *>(nearest + (int64_t)blk.sb * R * R);
    for (int64_t q = tid; q < per; q += kSlabWG) p[q] = none;
  }
  return true;
}

// An item's results at element e of a channel ([slow][y][fast], R3 elements per channel): plain 16-byte vector stores, as
// in tsdf_auggrid.hip; these kernels are bound by their search, not by their stores.
__device__ __forceinline__ void search_store(float *__restrict__ out, int32_t *__restrict__ nearest, int64_t R3, int64_t e,
                                             acc_f4 o0, acc_f4 o1, acc_f4 o2, acc_i4 on) {
  *reinterpret_cast<acc_f4 *>(out + e) = o0;
  *reinterpret_cast<acc_f4 *>(out + R3 + e) = o1;
  *reinterpret_cast<acc_f4 *>(out + 2 * R3 + e) = o2;
  if (nearest) *reinterpret_cast<acc_i4 *>(nearest + e) = on;
}

// slab_plan sizes a workgroup for a kernel that is bound by its stores.  These are bound by their search, and a small
// batch is as long as its slowest workgroup: below kMinBlocks workgroups the slabs are halved (down to one slice).
// A voxel's result does not depend on the slab it is in.
inline void search_halve(SlabPlan &plan, int n, int R) {
  while (plan.slab > 1 && plan.blocks < kMinBlocks) {
    plan.slab = (plan.slab + 1) / 2;
    plan.nslab = (R + plan.slab - 1) / plan.slab;
    plan.blocks = (int64_t)n * plan.nslab;
  }
}

// k0 / k1: the kernel's instantiations for TSDF_LAYOUT_CZYX / TSDF_LAYOUT_CXYZ (the layout has passed slab_bad_shape).
template <class ARGS>
int search_launch(void (*k0)(ARGS), void (*k1)(ARGS), int layout, const SlabPlan &plan, void *hip_stream, const ARGS &a) {
  hipLaunchKernelGGL(layout == TSDF_LAYOUT_CZYX ? k0 : k1, dim3((unsigned)plan.blocks), dim3(kSlabWG), 0,
                     static_cast<hipStream_t>(hip_stream), a);
  return launched();
}
