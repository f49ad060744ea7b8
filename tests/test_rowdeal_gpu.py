"""GPU tier of the row stream's block deal (csrc/phase1.inc, csrc/rowdeal.inc): the fused 32^3 kernel against the oracle
on small frames chosen for the deal — heights around every multiple of a block and of a whole round of blocks, widths in
every columns-per-lane class with a ragged last lane and a second column pass, valid pixels only in the first or last row,
the first or last column, or the single middle row, an all-invalid frame and a NaN-laden one.  A batch holds 2 * CUs + 5
frames, so both groups of every CU, the work queue and the tail help run.  Status, max_l, mid_p and the volumes are
compared bit for bit (extents are min/max reductions: no row order and no row-to-wave assignment may change a bit; the
voxel pass agrees with the oracle exactly on these frames).  The oracle's result is computed once and shared."""
import numpy as np
import pytest
import torch

import oracle
from frame_zoo import HEIGHTS, SEED, WIDTHS, _blob, rowdeal_frames

pytestmark = pytest.mark.gpu


def _batch(n):
    rng = np.random.default_rng(SEED)
    imgs = rowdeal_frames(rng)
    assert len(imgs) <= n, "an MI355X has 256 CUs: the batch holds every frame above"
    k = 0
    while len(imgs) < n:                                                               # fill up with fresh draws
        imgs.append(_blob(rng, HEIGHTS[(5 * k + 3) % 13], WIDTHS[(7 * k + 1) % 13]))
        k += 1
    headers, chunks = [], []
    for i in rng.permutation(n):                                                       # any frame may be a CU's last
        d = imgs[i]
        bh, bw = d.shape
        left, top = int(rng.integers(0, 640 - bw + 1)), int(rng.integers(0, 480 - bh + 1))
        headers.append([640, 480, left, top, left + bw, top + bh])
        chunks.append(d.reshape(-1))
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([c.size for c in chunks])
    return np.concatenate(chunks), offsets, np.array(headers, np.int32)


@pytest.fixture(scope="module")
def case():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dev = torch.device("cuda:0")
    n = 2 * torch.cuda.get_device_properties(dev).multi_processor_count + 5
    depth, off, hdr = _batch(n)
    ref = oracle.voxelize(depth, off, hdr, R=32, n_threads=8)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    assert (ref["status"] == 1).sum() >= 2 and (ref["status"] == 0).sum() >= n - 40       # the batch is what it says
    dt, ot, ht = (torch.from_numpy(a).to(dev) for a in (depth, off, hdr))
    return dt, ot, ht, ref


def _same(out, ref, what):
    got = {k: getattr(out, k).cpu().numpy() for k in ("status", "max_l", "mid_p", "tsdf")}
    np.testing.assert_array_equal(got["status"], ref["status"], err_msg=what)
    for k in ("max_l", "mid_p", "tsdf"):
        a, b = got[k].view(np.uint32), np.ascontiguousarray(ref[k], np.float32).view(np.uint32)
        bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
        print(f"{what}: {k}: {bad.size} frames differ" + (f", max |d| {np.nanmax(np.abs(got[k] - ref[k])):.3g}" if bad.size else ""))
        assert bad.size == 0, f"{what}: {k} differs from the oracle in frames {bad[:10].tolist()}"


def test_default_stream(pkg, case):
    dt, ot, ht, ref = case
    out = pkg.voxelize(dt, ot, ht, res=32)
    torch.cuda.synchronize()
    _same(out, ref, "default stream")


def test_non_default_stream(pkg, case):
    dt, ot, ht, ref = case
    s = torch.cuda.Stream(dt.device)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = pkg.voxelize(dt, ot, ht, res=32)
    s.synchronize()
    _same(out, ref, "side stream")


def test_twice_into_the_same_buffers(pkg, case):
    """The block counter is reset with every frame header and with every launch: the second launch into buffers that
    were overwritten in between gives the same bits."""
    dt, ot, ht, ref = case
    out = pkg.voxelize(dt, ot, ht, res=32)
    torch.cuda.synchronize()
    for rep in range(2):
        out.tsdf.fill_(7.0)
        out.max_l.fill_(-1.0)
        out.mid_p.fill_(-1.0)
        out.status.fill_(99)
        again = pkg.voxelize(dt, ot, ht, res=32, out=out)
        torch.cuda.synchronize()
        assert again.tsdf.data_ptr() == out.tsdf.data_ptr()
        _same(out, ref, f"out= launch {rep}")
