"""The occupancy kernel beyond the 32-bit element range (include/tsdf_occupancy.h: all output indexing is in 64 bits): one
bfloat16 volume of 1025 x 128^3 = 2^31 + 2^21 elements, its positions indexed from four source frames.  Every position is
compared on the device with its source frame's volume from a four-position launch, which is compared with the numpy
restatement (tests/occupancy_ref.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_ref as orf  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, R = 1025, 128


def test_a_volume_of_more_than_2_31_elements(pkg):
    dev = torch.device("cuda:0")
    assert N * R ** 3 > 2 ** 31
    free, _ = torch.cuda.mem_get_info(dev)
    assert free > 8 * 2 ** 30, "this test needs 8 GiB of device memory"
    depth, off, hdr = orf.crops()
    t = tuple(torch.from_numpy(a).to(dev) for a in (depth, off, hdr))
    ab = pkg.aabb(*t)
    max_l, mid_p = ab.grid[:, 3].contiguous(), ab.grid[:, :3].contiguous()
    four = torch.arange(4, device=dev)
    small, status = pkg.occupancy_volumes(*t, max_l[:4], mid_p[:4], res=R, dtype=torch.bfloat16, index=four)
    vol, _, rows = orf.batch(depth, off, hdr, max_l[:4].cpu().numpy(), mid_p[:4].cpu().numpy(), R, index=[0, 1, 2, 3])
    assert not status.any() and all(r.outside == 0 for r in rows)
    assert np.array_equal(small.view(torch.int16).cpu().numpy().astype(np.int64), vol.astype(np.int64) * 0x3f80)
    index = (torch.arange(N, device=dev) * 3 + 1) % 4                      # position 1024 takes frame 1
    out = torch.full((N, 1, R, R, R), -3.0, dtype=torch.bfloat16, device=dev)
    big, status = pkg.occupancy_volumes(*t, max_l[index], mid_p[index], res=R, dtype=torch.bfloat16, index=index, out=out)
    assert big.data_ptr() == out.data_ptr() and big.numel() > 2 ** 31 and not status.any()
    bits, want = big.view(torch.int16), small.view(torch.int16)
    for g in range(4):
        where = torch.nonzero(index == g).flatten()
        assert len(where) >= 256
        for chunk in where.split(64):
            assert bool((bits[chunk] == want[g]).all()), (g, chunk[0].item())
    assert bool((bits[N - 1] == want[int(index[N - 1])]).all()) and bool(want.any())
