// rowdeal.inc — part of the one translation unit tsdf_hip.hip (included there, inside its anonymous namespace); plain
// C++ that also compiles on the host (tests/test_rowdeal_cpu.py includes it into a stand-alone program).
// The row stream's block deal: the bh rows of a frame are cut into blocks of kU adjacent rows (one register buffer of
// phase 1: 3.75 KiB at 320 columns); block number -> rows is this one function.
#if defined(__HIPCC__)
#define TSDF_ROWDEAL_FN __host__ __device__ inline
#else
#define TSDF_ROWDEAL_FN inline
#endif

// order 0: blocks in frame order.  order r >= 1: outside in — r blocks from the top edge, r from the bottom edge, and so
// on until they meet in the middle, so the rows read last are the middle ones, which the staging copy is likeliest to
// re-read.  (r = 1 alternates block by block; phase 1 takes r = the number of waves that share the rows, which keeps
// the waves of a round on adjacent rows.)
constexpr int kRowsTopDown = 0;
constexpr int kRowsOutsideIn = 1;

TSDF_ROWDEAL_FN int rowdeal_blocks(int bh, int kU) { return (bh + kU - 1) / kU; }

// Block `blk` of a frame of bh rows: its first row; `n` gets its number of rows — kU, less for the block the frame's
// end cuts (never wrapped), 0 for a block number past the last (the counter is drawn beyond the end by every wave).
TSDF_ROWDEAL_FN int rowdeal_block(int blk, int bh, int kU, int order, int &n) {
  const int nblk = rowdeal_blocks(bh, kU);
  if (blk < 0 || blk >= nblk) {
    n = 0;
    return bh;
  }
  int pos = blk;
  if (order >= kRowsOutsideIn) {   // runs of `order` blocks, alternately from the top and from the bottom
    const int run = blk / order, k = (run >> 1) * order + (blk - run * order);
    pos = (run & 1) ? nblk - 1 - k : k;
  }
  const int row0 = pos * kU;
  n = bh - row0 < kU ? bh - row0 : kU;
  return row0;
}
