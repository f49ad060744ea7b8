"""The patch kernel beyond the 32-bit ranges (include/tsdf_patch.h: all global indexing is in 64 bits, the items are walked
by a grid-stride loop): a uint16 frame table longer than 2^31 elements with an index on both sides of that line, 70,000
positions in one launch, and a float32 patch buffer beyond 2^32 bytes.  Each is compared bit for bit with the numpy
restatement (tests/patch_ref.py) on sampled positions, the first and the last among them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patch_ref as pr  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _need_memory(dev, gib):
    free, _ = torch.cuda.mem_get_info(dev)
    assert free > gib * 2 ** 30, f"this test needs {gib} GiB of device memory"


def _to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_a_uint16_frame_table_longer_than_2_31_elements(pkg):
    dev = torch.device("cuda:0")
    _need_memory(dev, 8)
    H = W = 1024
    N = 2 ** 31 // (H * W) + 2                                 # 2050 frames of 2^20 pixels
    live = [0, 2047, 2048, N - 1]                              # frame 2047 ends at element 2^31, frame 2048 begins there
    assert (N - 1) * H * W > 2 ** 31 and 2048 * H * W == 2 ** 31
    rng = np.random.default_rng(41)
    small = rng.integers(440 * 4, 470 * 4, size=(len(live), H, W), dtype=np.uint16)        # shift 2: 440..470 mm
    small[:, ::97, ::89] = 0
    raw = torch.zeros((N, H, W), dtype=torch.int16, device=dev)          # the same bits; uint16 fills are not everywhere in torch
    for k, g in enumerate(live):
        raw[g].copy_(_to(dev, small[k].view(np.int16)))
    table = raw.view(torch.uint16)
    index = np.array([N - 1, 0, 2048, 2047, 2047, N, -1, 2048], np.int64)
    at = [(1020.0, 1021.0), (3.0, 2.0), (512.3, 600.7), (1000.0, 20.0), (0.0, 1023.0), (5.0, 5.0), (5.0, 5.0), (1023.0, 0.0)]
    com = np.stack([pr.com_at(px, py, 455.0) for px, py in at])
    for interp, name in ((0, "nearest"), (1, "bilinear")):
        got = pkg.frame_patches(table, _to(dev, com), size=16, cube=40.0, interp=name, shift=2, index=_to(dev, index))
        remap = np.array([live.index(g) if g in live else -1 for g in index], np.int64)
        want, st = pr.patches(pr.frames_source(pr.widen(small, 2)), com, S=16, cube=40.0, interp=interp, index=remap)
        assert got.status.tolist() == st.tolist() == [0, 0, 0, 0, 0, 2, 2, 0]
        assert np.array_equal(got.patch.view(torch.int32).cpu().numpy()[:, 0], pr.bits(want, pr.F32))
        assert (got.patch[[0, 1, 2, 3, 4, 7]] != 1.0).flatten(1).any(dim=1).all()
    assert table.numel() > 2 ** 31


def test_70000_positions_in_one_launch(pkg):
    dev = torch.device("cuda:0")
    n, S = 70000, 8
    c = pr.families()["tiny"]
    rng = np.random.default_rng(42)
    com = np.stack([pr.com_at(px, py, 450.0) for px, py in zip(rng.uniform(-2, 18, n), rng.uniform(-2, 14, n))])
    cube = rng.uniform(10.0, 40.0, n).astype(np.float32)
    index = torch.zeros(n, dtype=torch.int64, device=dev)
    out = pkg.PatchBatch(torch.full((n, 1, S, S), 9.0, dtype=torch.bfloat16, device=dev), torch.full((n,), 9, dtype=torch.int32, device=dev))
    pkg.frame_patches(_to(dev, c["source"]), _to(dev, com), size=S, cube=_to(dev, cube), interp="bilinear", dtype=torch.bfloat16,
                      index=index, out=out)
    assert not (out.patch == 9.0).any() and not out.status.any()           # every pixel of every position was written
    sample = [0, 1, 4095, 4096, 4097, 8191, 8192, 65535, 65536, n - 2, n - 1] + rng.integers(0, n, 40).tolist()
    want, _ = pr.patches(pr.source_of(c), com, S=S, cube=cube, interp=1, index=np.zeros(n, np.int64), positions=sample)
    got = out.patch.view(torch.int16).cpu().numpy()[:, 0]
    assert np.array_equal(got[sample], pr.bits(want[sample], pr.BF16))
    assert (out.patch[sample].float() != 1.0).any()


def test_a_float32_patch_buffer_beyond_2_32_bytes(pkg):
    dev = torch.device("cuda:0")
    _need_memory(dev, 10)
    n, S = 4097, 512
    c = pr.families()["tiny"]
    rng = np.random.default_rng(43)
    com = np.stack([pr.com_at(px, py, 450.0) for px, py in zip(rng.uniform(2, 14, n), rng.uniform(2, 10, n))])
    index = torch.zeros(n, dtype=torch.int64, device=dev)
    out = pkg.PatchBatch(torch.full((n, 1, S, S), 9.0, device=dev), torch.full((n,), 9, dtype=torch.int32, device=dev))
    assert out.patch.numel() * 4 > 2 ** 32
    pkg.frame_patches(_to(dev, c["source"]), _to(dev, com), size=S, cube=25.0, index=index, out=out)
    assert not out.status.any()
    for lo in range(0, n, 512):                                            # every pixel was written, in pieces that fit
        assert not (out.patch[lo:lo + 512] == 9.0).any()
    sample = [0, 1, 2047, 2048, n - 2, n - 1]                              # position 2048 begins at byte 2^31, n - 1 at 2^32
    want, _ = pr.patches(pr.source_of(c), com, S=S, cube=25.0, index=np.zeros(n, np.int64), positions=sample)
    got = out.patch[sample].view(torch.int32).cpu().numpy()[:, 0]
    assert np.array_equal(got, pr.bits(want[sample], pr.F32))
    assert (out.patch[n - 1] != 1.0).any()
