"""CPU tier of the shared placement (csrc/place.inc): the conditions on the hand-built pack of tests/place_ref.py that the
GPU tier (tests/test_place_gpu.py) relies on, checked where the reference alone runs — the oracle places every frame, and
the pack holds a frame for every lane grouping of the crop pass.  Nothing here touches a GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auggrid_ref as ar  # noqa: E402
import place_ref as pr  # noqa: E402


def test_the_oracle_places_every_frame_of_the_pack():
    depth, off, hdr, xf, centres = pr.pack()
    assert len(hdr) == len(pr.SHAPES) == 25 and xf.shape == (25, 24) and centres.shape == (25, 3)
    rows, max_l, mid_p = ar.pixel_grids(depth, off, hdr, xf, pr.R)   # (asserts a valid pixel in every frame)
    # status 0 by the placement's rule: the extent positive and finite, the centre finite, hence a usable grid row
    assert (max_l > 0).all() and np.isfinite(max_l).all() and np.isfinite(mid_p).all()
    assert all(ar.grid_ok(r) for r in rows)
    for i in range(len(hdr)):
        d = depth[off[i]:off[i + 1]]
        assert np.isnan(d).sum() == 1 and 400.0 <= np.nanmin(d[d != 0]) and np.nanmax(d) <= 900.0
    zeros = float((depth == 0).mean())
    print(f"pixels {depth.size}, zero {zeros:.3f}")
    assert 0.15 < zeros < 0.25


def test_the_pack_holds_every_lane_grouping():
    _, off, hdr, _, _ = pr.pack()
    w, h = hdr[:, 4] - hdr[:, 2], hdr[:, 5] - hdr[:, 3]
    assert [(int(a), int(b)) for a, b in zip(w, h)] == list(pr.SHAPES)
    assert {pr.lane_shift(int(x)) for x in w} == {2, 3, 4, 5, 6}
    ngrp = w // 4
    for p in (2, 4, 8, 16, 32, 64):                       # below and at every power of two: p lanes hold up to p groups
        assert {p - 1, p} <= set(ngrp.tolist()), p
    assert (ngrp > 64).any() and set((w % 4).tolist()) == {0, 1, 2, 3}
    assert any(o % 4 for o in off[:-1].tolist())          # frames that start off a 16-byte boundary
    sh = np.array([pr.lane_shift(int(x)) for x in w])
    trips = -(-h // (16 * (64 >> sh)))                    # row-loop trips of a workgroup of 16 waves
    at = list(pr.SHAPES).index
    assert (trips[at((5, 300))], trips[at((130, 40))], trips[at((132, 40))]) == (2, 2, 3)
    assert (16, 1) in pr.SHAPES
