"""GPU tier of the shared placement (csrc/place.inc): the two kernels that run it, tsdf_map_place_kernel and
tsdf_map_step_head_kernel, each held to the oracle's placement (tests/auggrid_ref.py::pixel_grids) DIRECTLY and bit for
bit, on the hand-built pack of tests/place_ref.py — every lane grouping of the crop pass, every tail length, unaligned rows
and frames, more rows than one trip of the workgroup takes.  (The head against the chain, tests/test_mapstep_gpu.py, compares
two runs of one text and so says nothing about the crop pass itself.)  tests/test_place_cpu.py shows that the oracle places
every frame of the pack.  One small launch each, no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auggrid_ref as ar  # noqa: E402
import place_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu


def up(*arrays):
    return tuple(torch.from_numpy(np.array(a)).to(torch.device("cuda")) for a in arrays)   # (a copy: the pack is read-only)


def assert_placed_as_the_oracle(got, depth, off, hdr, xf):
    rows, max_l, mid_p = ar.pixel_grids(depth, off, hdr, xf, pr.R)
    for name, want in (("grid", rows), ("max_l", max_l), ("mid_p", mid_p)):
        have = getattr(got, name).cpu().numpy()
        differ = np.flatnonzero((have.view(np.uint32) != want.view(np.uint32)).reshape(len(hdr), -1).any(axis=1))
        assert differ.size == 0, (name, [pr.SHAPES[i] for i in differ])
    assert got.status.tolist() == [0] * len(hdr)


def test_map_grids_equals_the_oracle_on_every_lane_grouping(pkg):
    depth, off, hdr, xf, _ = pr.pack()
    mg = pkg.map_grids(*up(depth, off, hdr, xf), res=pr.R)
    torch.cuda.synchronize()
    assert_placed_as_the_oracle(mg, depth, off, hdr, xf)


def test_map_step_head_equals_the_oracle_under_its_own_maps(pkg):
    depth, off, hdr, _, centres = pr.pack()
    d, o, h, c = up(depth, off, hdr, centres)
    head = pkg.map_step_head(d, o, h, c, pkg.aug_state(0x5EED0FACE0FF1CE5, 3, device=d.device), res=pr.R)
    torch.cuda.synchronize()
    assert head.gt_aug is None and head.gt_nor is None
    assert_placed_as_the_oracle(head, depth, off, hdr, head.xforms.cpu().numpy())
