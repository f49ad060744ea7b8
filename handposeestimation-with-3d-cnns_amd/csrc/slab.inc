// slab.inc — the scaffold of a kernel that voxelizes on a grid row the caller supplies: tsdf_auggrid.hip, tsdf_lowp.hip,
// tsdf_maplowp.hip, tsdf_accurate.hip and tsdf_mapaccurate.hip include it (after prim.inc, inside their anonymous
// namespace); the product does not.  Such a kernel is launched as n x ceil(R / slab) workgroups of kSlabWG threads, and a workgroup owns `slab`
// consecutive slices (indices of the slowest output axis) of one batch position.  What is the same for all of them is here:
//   SlabSrc          the members every such kernel's argument struct opens with: source tables, index, plan, camera
//   slab_of_block    workgroup -> (batch position, slab index, slices [sb, se))
//   slab_head        the block's source frame (through the index, if any): its crop, depth, grid row and status
//   slab_bad_frame   the status, and the zeros of a slab whose frame is not OK (slab_zero_fill)
//   slab_plan        host: slices per workgroup, workgroups per position, workgroups in all
//   slab_bad_shape   host: the R / layout test of an entry (device.inc::bad_res and the layout enum)
//   slab_args_ok     host: the argument checks every entry makes between `n == 0` and the device, with the plan
//   slab_src         host: a SlabSrc from an entry's arguments, its camera and its plan
// The voxel arithmetic of each kernel and the tail of its argument struct stay in its own file; what the two accurate
// kernels share beyond this (their search rectangle, bad-frame tail, store and launch) is in search.inc.

constexpr int kSlabWG = 256;       // threads per workgroup (4 wave64)
constexpr int kSlabMaxR = 128;     // largest resolution (device.inc::bad_res)
constexpr int kSlabItems = 512;    // items (V voxels each) a workgroup aims for: two per lane

// What every kernel here is handed first.  A kernel's argument struct holds it as its FIRST member and adds a tail of its
// own (88 bytes, 8-byte aligned: the tail starts where it would without the nesting).
struct SlabSrc {
  const float *depth;
  int64_t depth_len;
  const int64_t *offsets;   // [n_src + 1]
  const int32_t *headers;   // [n_src][6]
  int64_t n_src;
  const int64_t *index;     // [n] or null: batch position i voxelizes source frame index[i], without it frame i
  int n, R;
  int slab;    // slices per workgroup
  int nslab;   // workgroups per batch position
  double focal, cx, cy;
};
static_assert(sizeof(SlabSrc) == 88 && alignof(SlabSrc) == 8, "the kernel-argument layout of every user");

struct Slab {
  int64_t i;    // batch position
  int sidx;     // which of the position's workgroups
  int sb, se;   // its slices
  __device__ __forceinline__ bool first() const { return sidx == 0; }   // the one that writes the status
};

__device__ __forceinline__ Slab slab_of_block(int nslab, int slab, int R) {
  Slab s;
  s.i = blockIdx.x / (unsigned)nslab;
  s.sidx = (int)(blockIdx.x - s.i * nslab);
  s.sb = s.sidx * slab;
  s.se = s.sb + slab < R ? s.sb + slab : R;
  return s;
}

struct SlabFrame {
  int left, top, right, bottom;   // the crop rectangle
  int64_t bw;                     // its row stride
  int64_t off0;                   // its first pixel in the depth buffer
  float ox, oy, oz, vl, td;       // grid origin, voxel length, truncation distance
  int status;                     // TSDF_FRAME_*: a bad header before an unusable grid row
};

// The head of a kernel (all uniform): the block's source frame — through the index, if any; outside the tables it is a
// bad header and nothing of it is read, a bad frame's depth neither — on its grid row.  ROWS_OF_SOURCES: `grid` holds a
// row per source frame (tsdf_auggrid.hip, tsdf_lowp.hip, tsdf_accurate.hip); otherwise a row per batch position
// (tsdf_maplowp.hip, tsdf_mapaccurate.hip).  (depth_len and src_ok reach header_ok by reference, from locals: see there.)
template <bool ROWS_OF_SOURCES>
__device__ __forceinline__ SlabFrame slab_head(const SlabSrc &s, const Slab &blk, const float *grid) {
  const int64_t gi = s.index ? s.index[blk.i] : blk.i;
  const bool src_ok = gi >= 0 && gi < s.n_src;
  const int64_t g = src_ok ? gi : 0, depth_len = s.depth_len;
  const float *gr = grid + 8 * (ROWS_OF_SOURCES ? g : blk.i);
  SlabFrame f;
  const int32_t *hd = s.headers + 6 * g;
  f.left = hd[2], f.top = hd[3], f.right = hd[4], f.bottom = hd[5];
  const int64_t off0 = s.offsets[g], off1 = s.offsets[g + 1];
  f.bw = (int64_t)f.right - f.left;
  const bool hdr_ok = src_ok && header_ok(f.left, f.top, f.right, f.bottom, off0, off1, depth_len);
  f.ox = gr[0], f.oy = gr[1], f.oz = gr[2], f.vl = gr[3], f.td = gr[4];
  const bool grid_ok =
      f.td > 0.0f && finite32(f.td) && finite32(f.vl) && finite32(f.ox) && finite32(f.oy) && finite32(f.oz);
  f.status = !hdr_ok ? TSDF_FRAME_BAD_HEADER : !grid_ok ? TSDF_FRAME_DEGENERATE : TSDF_FRAME_OK;
  f.off0 = off0;
  return f;
}

// (uniform) zeros for a slab: slices [sb, se) of every channel are contiguous, `per` 16-byte pieces VEC of them.
// out: the position's [3][R][R][R] volume of T.
template <class VEC, class T>
__device__ __forceinline__ void slab_zero_fill(T *out, int R, int sb, int64_t per, int tid) {
  static_assert(sizeof(VEC) == 16, "16-byte pieces");
  const int64_t R3 = (int64_t)R * R * R;
  const VEC z = {0, 0, 0, 0};
  for (int c = 0; c < 3; ++c) {
    VEC *p = reinterpret_cast<VEC *>(out + c * R3 + (int64_t)sb * R * R);
    for (int64_t q = tid; q < per; q += kSlabWG) p[q] = z;
  }
}

// After slab_head: workgroup 0 of the position writes the status, and a frame that is not OK has the slab zero-filled,
// `per` pieces VEC per channel.  True: the caller returns (having filled what else it writes).
template <class VEC, class T>
__device__ __forceinline__ bool slab_bad_frame(const SlabFrame &fr, const Slab &blk, int32_t *status, T *out, int R,
                                               int64_t per, int tid) {
  if (blk.first() && tid == 0 && status) status[blk.i] = fr.status;
  if (fr.status == TSDF_FRAME_OK) return false;   // (uniform)
  slab_zero_fill<VEC>(out, R, blk.sb, per, tid);
  return true;
}

struct SlabPlan {
  int slab;         // slices per workgroup
  int nslab;        // workgroups per batch position
  int64_t blocks;   // workgroups of the launch
};

// n positions at R^3 in items of V voxels.  False: the launch would hold 2^32 work-items or more.
bool slab_plan(int n, int R, int V, SlabPlan &p) {
  const int per = R * (R / V);   // items per slice
  p.slab = (kSlabItems + per - 1) / per;
  if (p.slab > R) p.slab = R;
  p.nslab = (R + p.slab - 1) / p.slab;
  p.blocks = (int64_t)n * p.nslab;
  return p.blocks * kSlabWG <= 0xffffffffll;
}

bool slab_bad_shape(int R, int layout) {
  return bad_res(R) || (layout != TSDF_LAYOUT_CZYX && layout != TSDF_LAYOUT_CXYZ);
}

// What every entry checks after `n == 0` (each entry keeps what comes before, in its own order, and the tests of its own
// pointers): the source tables, the n_src / index rule, the camera, and a launch of fewer than 2^32 work-items.  R has
// passed slab_bad_shape.
inline bool slab_args_ok(const float *depth, int64_t depth_len, const int64_t *offsets, const int32_t *headers,
                         int64_t n_src, const int64_t *index, int n, int R, int V, const tsdf_cam *cam, SlabPlan &plan) {
  if (!depth || !offsets || !headers || depth_len < 0) return false;
  if (n_src < 1 || (!index && n_src != n)) return false;
  return cam_ok(cam) && slab_plan(n, R, V, plan);
}

inline SlabSrc slab_src(const float *depth, int64_t depth_len, const int64_t *offsets, const int32_t *headers,
                        int64_t n_src, const int64_t *index, int n, int R, const tsdf_cam &cam, const SlabPlan &plan) {
  return {depth, depth_len, offsets, headers, n_src, index, n, R, plan.slab, plan.nslab, cam.focal, cam.cx, cam.cy};
}
