"""CPU tier of the grid-stride tests: the position tables of tests/stride_ref.py hold what they claim at the sizes
tests/test_stride_gpu.py launches, GRID is the cap the four .hip files state, and the packs built from the tables pass each
reference's header rule where the kind is OK and fail it where the kind is bad_header.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auggrid_ref as ar  # noqa: E402
import locate_ref as lr  # noqa: E402
import obb_ref as ob  # noqa: E402
import stride_ref as sr  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "handposeestimation-with-3d-cnns_amd", "csrc")
ENTRY_KINDS = {"obb": sr.OBB_KINDS, "indexed": sr.KINDS, "locate": sr.LOCATE_KINDS}


def test_grid_is_the_cap_of_every_kernel_file():
    names = {}
    for f in ("tsdf_obb.hip", "tsdf_maplowp.hip", "tsdf_mapstep.hip", "tsdf_locate.hip"):
        with open(os.path.join(CSRC, f)) as fh:
            found = re.findall(r"constexpr int (k\w+MaxBlocks) = 1 << 16;", fh.read())
        assert len(found) == 1, f
        names[f] = found[0]
    assert names == {"tsdf_obb.hip": "kObbMaxBlocks", "tsdf_maplowp.hip": "kPlaceMaxBlocks",
                     "tsdf_mapstep.hip": "kHeadMaxBlocks", "tsdf_locate.hip": "kLocMaxBlocks"}
    assert sr.GRID == 1 << 16
    assert sr.GRID < sr.N2 < 2 * sr.GRID < sr.N3 < 3 * sr.GRID


@pytest.mark.parametrize("entry", sorted(ENTRY_KINDS))
@pytest.mark.parametrize("n", [sr.N2, sr.N3])
def test_tables_put_every_kind_behind_every_kind(n, entry):
    kinds = ENTRY_KINDS[entry]
    k = len(kinds)
    for seed in (1, 2):
        t = sr.table(n, seed, kinds)
        assert t.shape == (n,) and t.min() == 0 and t.max() == k - 1
        pairs = sr.pair_counts(t, k)
        assert pairs.sum() == n - sr.GRID and pairs.min() >= sr.MIN_PAIRS, (entry, pairs)
        if n > 2 * sr.GRID:
            between_ok, between_bad = sr.middle_counts(t, kinds)
            assert between_ok.min() >= 1 and between_bad.min() >= 1, (entry, between_ok, between_bad)
        assert np.array_equal(t, sr.table(n, seed, kinds))          # seeded
    assert not np.array_equal(sr.table(n, 1, kinds), sr.table(n, 2, kinds))


def test_crops_are_the_kinds_they_claim():
    cs = sr.crops()
    depth, off, hdr = sr.crop_pack()
    assert len(cs) <= 64 and len(set(c.name for c in cs)) == len(cs)
    ref = ob.batch(depth, off, hdr)
    for j, (c, f) in enumerate(zip(cs, ref)):
        bh, bw = c.img.shape
        assert bh * bw <= 300 * 4
        good = c.kind != "bad_header"
        assert ob.header_ok(hdr[j], off[j], off[j + 1], len(depth)) == good, c.name
        assert ar.header_ok(hdr[j], off[j], off[j + 1], len(depth)) == good, c.name
        assert (c.obb_kind == "bad_header") == (not good)
        # obb: the restatement's status is the kind's
        assert f["status"] == {"degenerate": 1, "bad_header": 2}.get(c.obb_kind, 0), c.name
        with np.errstate(invalid="ignore"):
            valid = int((np.abs(c.img) >= 1.0).sum())
        if c.kind == "degenerate":
            assert valid <= 1, c.name                     # no extent for the placement
        elif good:
            assert valid >= 2, c.name
        if c.kind == "ok_small":
            assert bw <= 3 and bh * bw <= 12
        if c.kind == "ok_rows":
            assert bh > 16
        if c.kind == "ok_wide":
            assert bw > 256 and bh >= 2
    assert {c.name: f["N"] for c, f in zip(cs, ref) if c.obb_kind != c.kind} == {"two_valid_pixels": 2}
    for kinds, obb in ((sr.OBB_KINDS, True), (sr.KINDS, False)):
        pools = sr.sources_of(kinds, obb)
        assert all(len(p) >= 4 for p, name in zip(pools, kinds) if name != "bad_index")
        assert [len(p) for p, name in zip(pools, kinds) if name == "bad_index"] == ([] if obb else [0])


@pytest.mark.parametrize("n", [sr.N2, sr.N3])
def test_tiled_pack_keeps_every_header_and_payload(n):
    depth, off, hdr = (torch.from_numpy(a.copy()) for a in sr.crop_pack())
    pools = sr.sources_of(sr.OBB_KINDS, obb=True)
    t = sr.table(n, 1, sr.OBB_KINDS)
    src = sr.draw_sources(t, pools, len(hdr), 3)
    for j, pool in enumerate(pools):
        assert np.isin(src[t == j], pool).all() and set(src[t == j]) == set(pool)      # every source is used
    td, to, th = sr.tile(depth, off, hdr, torch.from_numpy(src))
    assert int(to[-1]) == td.numel() and td.numel() * 4 < 1 << 30
    sizes = (off[1:] - off[:-1]).numpy()
    assert np.array_equal(np.diff(to.numpy()), sizes[src]) and torch.equal(th, hdr[torch.from_numpy(src)])
    # the header rule position by position (vectorised): area == payload exactly where the kind is not bad_header
    h = th.numpy().astype(np.int64)
    bw, bh = h[:, 4] - h[:, 2], h[:, 5] - h[:, 3]
    ok = (bw > 0) & (bh > 0) & (bw * bh == np.diff(to.numpy()))
    assert np.array_equal(ok, t != sr.OBB_KINDS.index("bad_header"))
    for i in np.random.default_rng(5).integers(0, n, 200):                               # and the payloads themselves
        a = td[int(to[i]):int(to[i + 1])].numpy()
        b = depth[int(off[src[i]]):int(off[src[i] + 1])].numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_indexed_positions_draw_their_kind():
    n_src = len(sr.crops())
    pools = sr.sources_of(sr.KINDS)
    t = sr.table(sr.N3, 2, sr.KINDS)
    src = sr.draw_sources(t, pools, n_src, 4)
    bad = t == sr.KINDS.index("bad_index")
    assert set(src[bad]) == {-1, n_src} and ((src[~bad] >= 0) & (src[~bad] < n_src)).all()
    kind_of = np.array([sr.KINDS.index(c.kind) for c in sr.crops()])
    assert np.array_equal(kind_of[src[~bad]], t[~bad])
    row = sr.small_row(torch.from_numpy(src), n_src).numpy()
    assert np.array_equal(sr.small_index(n_src)[row], src)


def test_locate_frames_are_the_kinds_they_claim():
    frames, kinds = sr.locate_frames()
    assert frames.shape[1:] == (sr.LOC_H, sr.LOC_W) and len(frames) <= 64 and sr.LOC_H > 16
    assert lr.capacity(sr.LOC_H, sr.LOC_W, 250.0, 100.0, sr.LOC_CAM[0]) * sr.N3 * 4 < 1 << 30
    u16 = sr.locate_frames_u16()
    assert np.array_equal(u16.astype(np.float32) * np.float32(2.0 ** -sr.LOC_SHIFT), frames)
    clipped = 0
    for refine in (0, 1, 2):
        for band in (0.0, 150.0):
            for f, kind in zip(frames, kinds):
                r = lr.locate_frame(f, sr.LOC_CAM, **dict(lr.PARAMS, refine=refine, seed_band=band))
                assert r["status"] == (1 if kind == "degenerate" else 0)
                assert r["margin"] >= lr.MARGIN                        # the GPU tier may compare rectangles exactly
                left, top, right, bottom = r["rect"]
                if kind == "ok_small":
                    assert 2 <= r["count"] <= 3
                if kind == "ok_wide":
                    clipped += left == 0 or top == 0 or right == sr.LOC_W or bottom == sr.LOC_H
    assert clipped
    pools = sr.locate_sources()
    assert [len(p) > 0 for p in pools] == [name != "bad_index" for name in sr.LOCATE_KINDS]
