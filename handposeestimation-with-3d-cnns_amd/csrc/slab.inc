// slab.inc — the scaffold of a kernel that voxelizes on a grid row the caller supplies: tsdf_auggrid.hip, tsdf_lowp.hip
// and tsdf_maplowp.hip include it (after prim.inc, inside their anonymous namespace); the product does not.  Such a kernel is
// launched as n x ceil(R / slab) workgroups of kSlabWG threads, and a workgroup owns `slab` consecutive slices (indices
// of the slowest output axis) of one batch position.  What is the same for all of them is here:
//   slab_of_block    workgroup -> (batch position, slab index, slices [sb, se))
//   slab_frame       a source frame's crop, depth, grid row and status (slab_frame_row: on a row the kernel picks)
//   slab_zero_fill   the zeros of a slab whose frame is not OK
//   slab_plan        host: slices per workgroup, workgroups per position, workgroups in all
//   slab_bad_shape   host: the R / layout test of an entry (device.inc::bad_res and the layout enum)
// The voxel arithmetic of each kernel stays in its own file.

constexpr int kSlabWG = 256;       // threads per workgroup (4 wave64)
constexpr int kSlabMaxR = 128;     // largest resolution (device.inc::bad_res)
constexpr int kSlabItems = 512;    // items (V voxels each) a workgroup aims for: two per lane

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

// A source frame g of the tables with the grid row gr to voxelize it on (all uniform).  src_ok: g lies inside the
// tables — the caller has clamped a g that does not, and the frame is then a bad header.  A bad frame's depth is not read.
// (depth_len and src_ok by reference, from the caller's locals: see header_ok.)
__device__ __forceinline__ SlabFrame slab_frame_row(const int64_t &depth_len, const int64_t *offsets,
                                                    const int32_t *headers, const float *gr, int64_t g,
                                                    const bool &src_ok) {
  SlabFrame f;
  const int32_t *hd = headers + 6 * g;
  f.left = hd[2], f.top = hd[3], f.right = hd[4], f.bottom = hd[5];
  const int64_t off0 = offsets[g], off1 = offsets[g + 1];
  f.bw = (int64_t)f.right - f.left;
  const bool hdr_ok = src_ok && header_ok(f.left, f.top, f.right, f.bottom, off0, off1, depth_len);
  f.ox = gr[0], f.oy = gr[1], f.oz = gr[2], f.vl = gr[3], f.td = gr[4];
  const bool grid_ok =
      f.td > 0.0f && finite32(f.td) && finite32(f.vl) && finite32(f.ox) && finite32(f.oy) && finite32(f.oz);
  f.status = !hdr_ok ? TSDF_FRAME_BAD_HEADER : !grid_ok ? TSDF_FRAME_DEGENERATE : TSDF_FRAME_OK;
  f.off0 = off0;
  return f;
}

// The grid rows belong to SOURCE frames (tsdf_auggrid.hip, tsdf_lowp.hip): row g of `grid`.  Where they belong to batch
// positions (tsdf_maplowp.hip) the kernel calls slab_frame_row with the position's row.
__device__ __forceinline__ SlabFrame slab_frame(const int64_t &depth_len, const int64_t *offsets,
                                                const int32_t *headers, const float *grid, int64_t g,
                                                const bool &src_ok) {
  return slab_frame_row(depth_len, offsets, headers, grid + 8 * g, g, src_ok);
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
