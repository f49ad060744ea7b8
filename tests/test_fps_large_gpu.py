"""The sampling kernel beyond the 32-bit element range (include/tsdf_fps.h: all global indexing is in 64 bits): one source
frame placed behind 2^31 elements of an otherwise unread pack and selected by ``index``.  Its result is compared with the
same crop in a pack of its own, which is compared with the numpy restatement (tests/fps_ref.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fps_ref as fr  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GAP = 2 ** 31 + 3           # elements in front of the frame: its offset does not fit 32 bits and is off a 16-byte boundary


def test_a_frame_behind_2_31_elements(pkg):
    dev = torch.device("cuda:0")
    free, _ = torch.cuda.mem_get_info(dev)
    assert free > 10 * 2 ** 30, "this test needs 10 GiB of device memory"
    depth, off, hdr = fr.crops(2)
    crop, header = depth[off[1]:off[2]], hdr[1]
    want = fr.batch(crop, np.array([0, len(crop)]), header[None], 128)
    assert want.status.tolist() == [0] and fr.RESIDENT >= want.count[0] > 1000
    small = pkg.farthest_points(torch.from_numpy(crop).to(dev), torch.tensor([0, len(crop)], device=dev),
                                torch.from_numpy(header[None].copy()).to(dev), points=128)
    got = fr.Fps(*[t.cpu().numpy() for t in small])
    assert fr.same(got, want) is None, fr.same(got, want)
    # frame 0 is the 2^31 + 3 elements in front (never read: nothing selects it); frame 1 is the crop
    big = torch.empty(GAP + len(crop), dtype=torch.float32, device=dev)
    big[GAP:] = torch.from_numpy(crop).to(dev)
    offsets = torch.tensor([0, GAP, GAP + len(crop)], dtype=torch.int64, device=dev)
    headers = torch.from_numpy(np.stack([np.array([640, 480, 0, 0, 1, 1], np.int32), header])).to(dev)
    index = torch.tensor([1, 1], dtype=torch.int64, device=dev)
    for kw in (dict(), dict(capacity=int(want.count[0]), form=1)):
        far = pkg.farthest_points(big, offsets, headers, points=128, index=index, **kw)
        for a, b in zip(far, small):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[0]), kw
    # selected, frame 0 contradicts its header (1 pixel, 2^31 + 3 elements): status 2, and still nothing of it is read
    bad = pkg.farthest_points(big, offsets, headers, points=4, index=torch.tensor([0], dtype=torch.int64, device=dev))
    assert bad.status.tolist() == [2] and bad.count.tolist() == [0] and bad.pixel.tolist() == [[-1] * 4]
