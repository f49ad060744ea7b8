"""CPU tier of the resolution tests: what the case list of tests/plan_ref.py reaches, shown on the restated launch plans
(those of the two accurate entries included: slab_plan followed by their halving loop), and the conditions on the oracle's volumes of the six source frames at all 32 resolutions — so that the GPU tier
(tests/test_resolutions_gpu.py) compares volumes that hold rejected voxels and voxels near the surface everywhere."""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auggrid_ref as ar  # noqa: E402
import plan_ref as pr  # noqa: E402

CU_COUNTS = (256, 304, 64)    # the MI355X, and two other device sizes the case list is a function of


def test_the_restated_plans_on_known_values():
    """The figures the host code's comments and the existing GPU tests state, on 256 CUs."""
    assert len(pr.RES) == 32 and pr.RES[0] == 4 and pr.RES[-1] == 128 and all(R % 4 == 0 for R in pr.RES)
    for R in (4, 8, 16):
        assert all(pr.split_plan(n, R, 256) == (0, R) for n in (1, 3, 40, 128))
    assert pr.split_plan(1, 12, 256) == (12, 1)
    assert pr.split_plan(16, 40, 256) == (14, 3) and pr.last_part(40, 14, 3) == 1
    assert pr.split_plan(1, 76, 256) == (16, 5) and pr.last_part(76, 16, 5) == 1
    for R in (44, 72, 92, 100):
        S, per = pr.split_plan(1, R, 256)
        assert pr.last_part(R, S, per) == 2, R
    assert pr.split_plan(40, 28, 256) == (6, 5) and pr.last_part(28, 6, 5) == 3
    assert [R for R in pr.RES if pr.sstep(R) > 1 and pr.split_plan(1, R, 256)[0]] == [32]
    assert pr.split_plan(129, 32, 256) == (0, 32) and pr.split_plan(128, 32, 256) == (2, 16)
    assert [R for R in pr.RES if pr.g_divides(R, 512)] == [4, 8, 16, 32]
    assert [R for R in pr.RES if pr.g_divides(R, 1024)] == [4, 8, 16, 32, 64]
    assert [R for R in pr.RES if pr.dyn(R)] == [64, 128]
    assert [R for R in pr.RES if pr.groups_for(R) == 1] == list(range(48, 129, 4))
    assert pr.use_tab(32) and not pr.use_tab(36) and not pr.use_tab(32, aug=True)
    assert pr.slab_plan(4, 4) == (4, 1) and pr.slab_plan(32, 4) == (2, 16) and pr.slab_plan(128, 8) == (1, 128)
    assert pr.slab_ragged(20, 4) and pr.slab_ragged(28, 4) and pr.slab_ragged(40, 8) and not pr.slab_ragged(32, 8)
    assert pr.describe(300, 32, 0, 0, 256) == "tsdf_fused_kernel<32, 0, false, false, 2>"
    assert pr.describe(300, 64, 0, 1, 256) == "tsdf_fused_kernel<64, 0, true, false, 1>"
    assert pr.describe(16, 32, 1, 0, 256) == "tsdf_split_kernel<32, 1, false, x8"
    assert pr.describe(300, 48, 0, 0, 256) == "tsdf_fused_kernel<0, 0, false, false, 1>"


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_the_case_list_reaches_every_class(cus):
    cases = pr.cases(cus)
    assert {R for R, _, _ in cases} == set(pr.RES)
    split = [(R, n) for R, n, kind in cases if kind == "split"]
    classes = {pr.split_class(n, R, cus) for R, n in split}
    assert {"none", "equal", "last1", "last2"} <= classes, classes
    # sstep > 1 in a launch that does split, and the split kernel up to its limit n = CUs/2
    assert any(pr.sstep(R) > 1 and pr.split_plan(n, R, cus)[0] >= 2 for R, n in split)
    # (a device of more than 256 CUs meets the exchange's 128-frame limit first: its n = CUs/2 launch is a fused one)
    assert cus // 2 > pr.K_XCHG_FRAMES or any(n == cus // 2 and pr.split_plan(n, R, cus)[0] >= 2 for R, n in split)
    # the other kinds never split; 'static' deals by position (no queue), 'queue' has more frames than groups
    for R, n, kind in cases:
        if kind != "split":
            grid = min(n, cus)
            assert pr.split_plan(n, R, cus)[0] == 0 and n > cus // 2, (R, n)
            assert (n > grid * pr.groups_for(R)) == (kind == "queue"), (R, n, kind)
    # the lane mapping: T = 512 (a group of the two-group kernel alone), T = 1024 (helped, split, one-group kernel)
    two = [R for R in pr.RES if pr.groups_for(R) == 2]
    assert {pr.g_divides(R, 512) for R in two} == {True, False}
    assert {pr.g_divides(R, 1024) for R in two} == {True, False}            # tail help and the split kernel among R < 48
    one = [R for R in pr.RES if pr.groups_for(R) == 1]
    assert {pr.g_divides(R, 1024) for R in one} == {True, False}
    assert {pr.dyn(R) for R in one} == {True, False}
    assert {pr.use_tab(R) for R in pr.RES} == {True, False}
    # tail help (R < 48, queue-driven) on both lane mappings and with and without tables
    helped = [R for R, n, kind in cases if kind == "queue" and pr.groups_for(R) == 2]
    assert {pr.g_divides(R, 1024) for R in helped} == {True, False} and {pr.use_tab(R) for R in helped} == {True, False}
    # the slab kernels: a ragged and a whole last slab, float32 (V = 4) and 16-bit (V = 8 and V = 4)
    assert {pr.slab_ragged(R, 4) for R in pr.RES} == {True, False}
    assert {pr.lowp_items(R) for R in pr.RES} == {4, 8}
    for V in (4, 8):
        assert {pr.slab_ragged(R, V) for R in pr.RES if pr.lowp_items(R) == V} == {True, False}, V
    # one position per workgroup and several workgroups per position
    assert {pr.slab_plan(R, pr.lowp_items(R))[1] == 1 for R in pr.RES} == {True, False}


def test_the_accurate_plan_on_known_values():
    """The figures the accurate entries' comments and their GPU tests state."""
    assert pr.accurate_plan(1, 4) == (1, 4, 2) and pr.accurate_plan(1024, 4) == (4, 1, 0)
    assert pr.accurate_plan(2, 20) == (1, 20, 3) and pr.accurate_plan(300, 20) == (6, 4, 0)       # 6 slices, the last slab 2
    assert pr.accurate_plan(1100, 8) == (8, 1, 0) and pr.accurate_plan(1, 64) == (1, 64, 0)
    assert pr.accurate_plan(1100, 12) == (12, 1, 0) and pr.accurate_plan(3, 12) == (1, 12, 4)     # 12 -> 6 -> 3 -> 2 -> 1
    assert pr.accurate_batch_sizes(4) == [(1, "one"), (512, "partway"), (1024, "whole")]
    assert pr.accurate_batch_sizes(128) == [(1, "one"), (8, "whole")]
    assert pr.accurate_plan(512, 4) == (2, 2, 1) and pr.accurate_plan(511, 4) == (1, 4, 2)
    assert pr.accurate_plan(103, 20) == (2, 10, 2) and pr.accurate_plan(102, 20) == (1, 20, 3)


def test_the_accurate_case_list_reaches_every_plan():
    """What tests/test_resolutions_gpu.py launches the two accurate entries at: every R, and among the final plans slabs of
    one slice, slabs of several that divide R, slabs that leave a ragged last slab, and all three batch regimes."""
    final = {(R, kind): (n, *pr.accurate_plan(n, R)) for R in pr.RES for n, kind in pr.accurate_batch_sizes(R)}
    assert {R for R, _ in final} == set(pr.RES)
    for R in pr.RES:
        n1, slab, nslab, h1 = final[R, "one"]
        assert (n1, slab, nslab) == (1, 1, R)                                 # n = 1: always one slice per workgroup
        nw, slab, nslab, hw = final[R, "whole"]
        assert hw == 0 and (slab, nslab) == pr.slab_plan(R, 4) and nw * nslab >= pr.K_MIN_BLOCKS > (nw - 1) * nslab
        assert ((R, "partway") in final) == (h1 >= 2) == (R <= 28), R
        if (R, "partway") in final:
            n, slab, nslab, h = final[R, "partway"]
            assert 1 <= h == h1 - 1 and 1 < slab < pr.slab_plan(R, 4)[0] and 1 < n < nw
            assert n * nslab >= pr.K_MIN_BLOCKS and pr.accurate_plan(n - 1, R)[2] == h1      # the smallest such n
        else:                                                                 # no partway state: the loop runs out or never runs
            assert h1 <= 1 and {pr.accurate_plan(n, R)[2] for n in range(1, nw + 1)} == {h1, 0}
    assert final[4, "whole"][0] == 1024 and final[128, "whole"][0] == 8
    # from R = 48 on slab_plan's slab is one slice: 'one' and 'whole' differ in the batch only
    assert [R for R in pr.RES if final[R, "one"][3] == 0] == list(range(48, 129, 4))
    several = {(R, kind): v for (R, kind), v in final.items() if v[1] > 1}
    divides = sorted({R for (R, _), v in several.items() if R % v[1] == 0})
    ragged = sorted({R for (R, _), v in several.items() if R % v[1] != 0})
    assert ragged == [20, 28] and len(divides) >= 8, (ragged, divides)        # (V = 4 has no other ragged slab_plan: below)
    assert ragged == [R for R in pr.RES if pr.slab_ragged(R, 4)]
    assert {pr.accurate_last_slab(final[R, "whole"][0], R) for R in ragged} == {1, 2}
    # a slab that holds the whole position, and a halved slab of several slices, at several resolutions each
    assert sorted(R for (R, kind), v in several.items() if v[2] == 1) == [4, 8, 12]
    assert sorted(R for (R, kind), v in several.items() if kind == "partway") == [4, 8, 12, 16, 20, 24, 28]


def test_the_sources():
    depth, off, hdr = pr.sources()
    assert len(hdr) == pr.N_SRC == 6 and off[-1] == depth.size
    w, h = hdr[:, 4] - hdr[:, 2], hdr[:, 5] - hdr[:, 3]
    assert [(int(a), int(b)) for a, b in zip(w[:4], h[:4])] == [(126, 97), (142, 107), (138, 130), (97, 141)]
    assert (w[4:] == 320).all() and (h[4:] == 240).all()
    assert any(o % 4 for o in off[1:4])                                      # frames on unaligned addresses
    ramp = depth[off[5]:off[6]]
    assert ramp.size == 76800 and (ramp >= 1.0).all() and np.isfinite(ramp).all()
    xf = pr.source_maps()
    assert xf.shape == (6, 24) and all(not np.allclose(x[:12], ar.identity_xforms(1)[0, :12]) for x in xf)
    d, o, h6 = pr.cycled(15)
    assert len(h6) == 15 and o[-1] == d.size and np.array_equal(h6[12:], hdr[:3]) and np.array_equal(d[:off[6]], depth)
    assert np.array_equal(np.diff(o), np.tile(np.diff(off), 3)[:15])


def _zero_and_near(vol):
    """Per frame: voxels that are 0 in every channel, and values strictly between 0 and 1 in magnitude."""
    a = np.abs(vol)
    n = a.shape[0]
    zero = (a == 0).all(axis=1).reshape(n, -1).sum(axis=1)
    near = ((a > 0) & (a < 1)).reshape(n, -1).sum(axis=1)
    return zero, near


@pytest.mark.parametrize("R", pr.RES)
def test_every_source_has_zero_and_near_voxels(R):
    """status 0, at least one rejected voxel and at least one voxel near the surface for every source — plain and under
    its map —, and at the ends of the range the counts of the four crops.  The oracle's volume on the rows of its own
    placement is the volume of its fused entry, so the GPU tier holds the slab kernels to the same arrays."""
    depth, off, hdr = pr.sources()
    xf = pr.source_maps()
    plain = oracle.voxelize(depth, off, hdr, R=R, n_threads=8, extras=True)
    mapped = oracle.voxelize_aug(depth, off, hdr, xf, R=R, n_threads=8)
    for name, res in (("plain", plain), ("mapped", mapped)):
        assert not res["status"].any(), (name, R)
        zero, near = _zero_and_near(res["tsdf"])
        assert (zero >= 1).all() and (near >= 1).all(), (name, R, zero, near)
        if name == "plain" and R in (4, 128):
            assert (near[:4] >= (120 if R == 4 else 139000)).all(), near
    if R in (4, 20, 32):
        rows = np.zeros((6, 8), np.float32)
        rows[:, :3], rows[:, 3], rows[:, 4] = plain["ori"], plain["grid"][:, 4], plain["grid"][:, 5]
        for i in range(6):
            v = oracle.voxels(depth[off[i]:off[i + 1]], hdr[i], rows[i, :3], rows[i, 3], rows[i, 4], R=R)
            assert np.array_equal(v.view(np.uint32), plain["tsdf"][i].view(np.uint32))
        arows, max_l, mid_p = ar.pixel_grids(depth, off, hdr, xf, R)
        assert np.array_equal(max_l.view(np.uint32), mapped["max_l"].view(np.uint32))
        assert np.array_equal(mid_p.view(np.uint32), mapped["mid_p"].view(np.uint32))
        vol, st = ar.voxelize_aug_grid_ref(depth, off, hdr, xf, arows, R, "czyx")
        assert not st.any() and np.array_equal(vol.view(np.uint32), mapped["tsdf"].view(np.uint32))
