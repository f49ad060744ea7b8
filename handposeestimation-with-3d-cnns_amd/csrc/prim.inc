// prim.inc — the device primitives every voxelizing library here shares: tsdf_hip.hip (before common.inc),
// tsdf_auggrid.hip, tsdf_obb.hip, tsdf_lowp.hip and tsdf_maplowp.hip include it, so each rule below exists once.
//   kDefaultCam    the camera an entry uses when the caller passes none
//   cam_ok         the camera rule: which tsdf_cam an entry accepts (host code, plain C++)
//   trunc_i32      int() of a float64, the pixel index's truncation
//   finite32       a float32 that is neither infinite nor NaN
//   f32_round_up   the float32 threshold of a float64 comparison
//   header_ok      the voxelizer's header rule: is this frame's depth read at all
// No device globals, and nothing of the product's other .inc files is needed.
//
// Included inside an anonymous namespace, after device.inc (so after <hip/hip_runtime.h>, <stdint.h> and include/tsdf.h).
// tsdf_host.inc — plain C++, also compiled without HIP — includes it too, inside namespace tsdf_host and with
// TSDF_PRIM_HOST_ONLY defined: it then gets cam_ok alone, so check_run_args and the entries that do not go through run()
// apply one and the same rule.  cam_ok is defined once per translation unit, by whichever inclusion comes first (in
// tsdf_hip.hip that is tsdf_host.inc's: the product's own files see tsdf_host::cam_ok through launch.inc's using-directive).

// The camera rule of every entry that takes a tsdf_cam: NULL is the default camera; otherwise focal, invalid_eps and
// trunc_voxels must each be > 0 (written so that NaN fails).  It covers the whole struct, whichever fields the entry reads.
#ifndef TSDF_PRIM_CAM_OK
#define TSDF_PRIM_CAM_OK
inline bool cam_ok(const tsdf_cam *cam) {
  return !cam || (cam->focal > 0.0 && cam->invalid_eps > 0.0f && cam->trunc_voxels > 0.0f);
}
#endif

#ifndef TSDF_PRIM_HOST_ONLY

const tsdf_cam kDefaultCam = {241.42, 160.0, 120.0, 1.0f, 3.0f};   // pre/tsdf_numba.py:8-10, as in include/tsdf.h

// int() of a float64, toward zero; v_cvt_i32_f64 saturates out-of-range values and maps NaN to 0
// (same rule as oracle/tsdf_oracle.c::trunc_i32).
__device__ __forceinline__ int trunc_i32(double v) {
  int r;
  asm("v_cvt_i32_f64 %0, %1" : "=v"(r) : "v"(v));
  return r;
}

__device__ __forceinline__ bool finite32(float v) { return __builtin_fabsf(v) < __builtin_inff(); }   // false for NaN

// smallest float32 >= t  (so that for a float32 p:  p < t  <=>  p < result)
__device__ __forceinline__ float f32_round_up(double t) {
  float f = (float)t;
  if ((double)f < t) f = nextafterf(f, __builtin_inff());
  return f;
}

// The voxelizer's header rule for a crop [left, right) x [top, bottom) whose pixels are depth[off0, off1): a header that
// contradicts its payload, or a payload outside the depth buffer, is never read.  (The extents cannot overflow in 64 bits.)
// off0, off1 and depth_len come by reference, and from the caller's locals, not from members of a kernel's argument
// struct: the compiler simplifies this function before it inlines it, and with the three by value (then known to be
// defined) it settles on another, equivalent sequence for the tests than for the expression written in place —
// tsdf_auggrid.hip's code object would no longer be the one it was before the rule moved here.  For the same reason
// the product's own two sites (frame.inc::frame_from_header, cloud.inc) keep the rule written in place: a call of this
// function there changes the product's instructions.
__device__ __forceinline__ bool header_ok(int left, int top, int right, int bottom, const int64_t &off0,
                                          const int64_t &off1, const int64_t &depth_len) {
  const int64_t bw = (int64_t)right - left, bh = (int64_t)bottom - top;
  return bw > 0 && bh > 0 && bw <= 0x7fffffff && bh <= 0x7fffffff && bw * bh == off1 - off0 && off0 >= 0 &&
         off1 <= depth_len;
}

#endif  // TSDF_PRIM_HOST_ONLY
