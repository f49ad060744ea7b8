"""GPU tier of the composed maps and the fused step head (include/tsdf_mapstep.h): tsdf_compose_kernel bit for bit against
numpy (tests/mapstep_ref.py::compose_np); tsdf_map_step_head_hip bit for bit, on every output, against the chain of existing
entries it replaces (aug_xforms_at, compose_xforms, map_grids, transform_joints, normalize_joints) — shapes, indices,
counters, edge frames, independence of the batch, the draw-only form, the state read at run time; AugmentedStep(base=,
fused_head=) replayed from its graph against the eager step and the chain assembled by hand; and what the composed step
means, against the oracle fed the GPU's composed maps.

Nothing but the last test has a tolerance: everything else is torch.equal on the bits.  The last one uses the project's
contract figure for the augmented entry, TOL = 1e-5 (tests/auggrid_ref.py), and for the 2-byte volume the band
(o - TOL).to(dtype) <= g <= (o + TOL).to(dtype) of tests/test_maplowp_gpu.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auggrid_ref as ar  # noqa: E402
import mapstep_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = ar.TOL
KEY = 0x5EED0FACE0FF1CE5
WRAP = (1 << 64) - 40          # counter0 + i wraps mod 2^64 inside a batch of more than 40
VIEW = {torch.float64: torch.int64, torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def dev():
    return torch.device("cuda")


def up(*arrays):
    return tuple(torch.from_numpy(np.array(a)).to(dev()) for a in arrays)      # (a copy: the shared frames are read-only)


def same(a, b):
    """Equal shapes, types and BITS (a NaN equals itself, -0 is not +0)."""
    if a is None or b is None:
        return a is None and b is None
    if a.dtype is not b.dtype or a.shape != b.shape:
        return False
    v = VIEW.get(a.dtype)
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v)) if v is not None else torch.equal(a, b)


def in_band(g, ref, tol):
    lo, hi = (ref - tol).to(g.dtype).float(), (ref + tol).to(g.dtype).float()
    gf = g.float()
    return bool(((lo <= gf) & (gf <= hi)).all())


FIELDS = ("xforms", "grid", "max_l", "mid_p", "status", "gt_aug", "gt_nor", "stretch", "rot")


def chain(pkg, d, o, h, centres, state, base=None, index=None, counters=None, gt=None, res=32, clamp=True):
    """The head's outputs from the existing entries, one launch each."""
    n_src = h.shape[0]
    U, stretch, rot = pkg.aug_xforms_at(centres, state, index=index, counters=counters, return_params=True)
    T = pkg.compose_xforms(U, base, index) if base is not None else U
    mg = pkg.map_grids(d, o, h, T, res=res, index=index)
    gaug = gnor = None
    if gt is not None:
        g = gt if index is None else gt.index_select(0, index.clamp(0, n_src - 1))
        gaug = pkg.transform_joints(g, T)
        gnor = pkg.normalize_joints(gaug, mg.max_l, mg.mid_p, clamp=clamp)
    return dict(zip(FIELDS, (T, mg.grid, mg.max_l, mg.mid_p, mg.status, gaug, gnor, stretch, rot)))


def head(pkg, d, o, h, centres, state, **kw):
    b, stretch, rot = pkg.map_step_head(d, o, h, centres, state, return_params=True, **kw)
    assert isinstance(b, pkg.MapStepBatch)
    return dict(zip(FIELDS, (*b, stretch, rot)))


def assert_same(got, want, what=""):
    for name in FIELDS:
        assert same(got[name], want[name]), (what, name)


def sentinel_out(pkg, n, gt_shape=None):
    nan = float("nan")
    f = lambda *s: torch.full(s, nan, device=dev())
    return pkg.MapStepBatch(torch.full((n, 24), nan, dtype=torch.float64, device=dev()), f(n, 8), f(n), f(n, 3),
                            torch.full((n,), -7, dtype=torch.int32, device=dev()),
                            f(n, *gt_shape) if gt_shape else None, f(n, *gt_shape) if gt_shape else None)


@functools.lru_cache(maxsize=None)
def _pack36(pkg):
    """The 36 frames on the GPU with their OBB maps, the centres in the camera frame and in the OBB frame (R = 32), and
    joints about every camera-frame centre (sigma 80 mm: some labels leave [0, 1]).  Made once, never modified."""
    d, o, h = up(*mr.frames36())
    base = pkg.obb_xforms(d, o, h)
    assert not bool(base.status.any())
    c_cam = pkg.aabb(d, o, h, res=32).grid[:, :3].contiguous()
    c_obb = pkg.map_grids(d, o, h, base.xforms, res=32).mid_p
    gt = c_cam[:, None, :] + torch.from_numpy(np.random.default_rng(7).normal(0, 80, (36, 21, 3)).astype(np.float32)).to(dev())
    torch.cuda.synchronize()
    return d, o, h, base.xforms, c_cam, c_obb, gt.contiguous()


# ---- compose_xforms ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_compose_equals_numpy_bit_for_bit(pkg, n):
    inner = _pack36(pkg)[3]
    rng = np.random.default_rng(n)
    centres, = up(rng.normal(0, 150, (n, 3)).astype(np.float32) + np.float32([0, 0, -450]))
    outer = pkg.aug_xforms(centres, key=KEY, counter0=n)
    idx = rng.integers(0, 36, n)
    if n >= 3:
        idx[[0, 1, 2]] = [36, -1, idx[3 % n]]        # n_inner, -1 and a repeat
    else:
        idx[0] = 36
    ti, = up(idx.astype(np.int64))
    got = pkg.compose_xforms(outer, inner, ti)
    rep = inner.repeat((n + 35) // 36, 1)[:n].contiguous()
    plain = pkg.compose_xforms(outer, rep)
    into = outer.clone()
    assert pkg.compose_xforms(into, inner, ti, out=into) is into          # in place
    torch.cuda.synchronize()
    o_np, i_np = outer.cpu().numpy(), inner.cpu().numpy()
    want = mr.compose_np(o_np, i_np, idx)
    assert got.dtype is torch.float64 and got.shape == (n, 24)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64))
    assert np.array_equal(plain.cpu().numpy().view(np.uint64), mr.compose_np(o_np, rep.cpu().numpy()).view(np.uint64))
    assert same(into, got)
    bad = torch.from_numpy((idx < 0) | (idx >= 36)).to(dev())
    assert bool(bad.any()) and same(got[bad], outer[bad])                  # a bad index: out == outer
    assert n < 3 or not same(got[~bad], outer[~bad])
    if n == 65:
        with pytest.raises(ValueError):
            pkg.compose_xforms(outer, inner)                               # no index: one inner map per outer map
        with pytest.raises(ValueError):
            pkg.compose_xforms(outer, inner, ti[:5])
        with pytest.raises(ValueError):
            pkg.compose_xforms(outer[:, :12], inner, ti)
        assert pkg.compose_xforms(outer[:0], inner, ti[:0]).shape == (0, 24)


# ---- the head against the chain ----
def _cases(rng):
    """(name, index, counters, counter0, J, clamp): n = 1, 16, 65 and 300 through an index, and the pack itself."""
    i16 = rng.integers(0, 36, 16)
    i16[[2, 9]] = [-1, 36]
    c16 = rng.integers(-2 ** 62, 2 ** 62, 16)
    c16[:3] = [-1, -(2 ** 63), 0]
    return [("n1", np.array([17]), None, 5, 21, True),
            ("n16", i16, c16, WRAP, 1, False),
            ("n65", rng.integers(0, 36, 65), None, WRAP, 21, False),
            ("n300", rng.integers(0, 36, 300), rng.integers(-1000, 1000, 300), 1 << 40, 21, True),
            ("pack", None, None, WRAP, 21, True),
            ("pack_counters", None, rng.integers(-50, 50, 36), 0, 1, True)]


@pytest.mark.parametrize("with_base", [True, False], ids=["base", "nobase"])
@pytest.mark.parametrize("R", [8, 32, 64])
def test_head_equals_the_chain_on_every_output(pkg, R, with_base):
    d, o, h, base, c_cam, c_obb, gt = _pack36(pkg)
    centres = c_obb if with_base else c_cam
    clamped = beyond = False
    for name, idx, cnt, c0, J, clamp in _cases(np.random.default_rng(R)):
        state = pkg.aug_state(KEY + R, c0, device=dev())
        ti = up(idx.astype(np.int64))[0] if idx is not None else None
        tc = up(cnt.astype(np.int64))[0] if cnt is not None else None
        g = gt[:, :J].contiguous()
        kw = dict(base=base if with_base else None, index=ti, counters=tc, gt=g, res=R, clamp=clamp)
        got = head(pkg, d, o, h, centres, state, **kw)
        want = chain(pkg, d, o, h, centres, state, **kw)
        torch.cuda.synchronize()
        n = 36 if idx is None else len(idx)
        assert got["xforms"].shape == (n, 24) and got["grid"].shape == (n, 8) and got["gt_nor"].shape == (n, J, 3)
        assert_same(got, want, name)
        st = got["status"].tolist()
        assert st == [0 if idx is None or 0 <= g_ < 36 else 2 for g_ in (idx if idx is not None else range(36))], name
        okp = got["status"] == 0
        assert bool((got["max_l"][okp] > 0).all()) and not bool(torch.isnan(got["gt_nor"]).any())
        if name == "n16":     # the bad positions: identity, NaN stretch, zero row, labels 0.5
            ident, = up(pkg.augment.identity_affines(1)[0])
            for k in (2, 9):
                assert torch.equal(got["xforms"][k], ident) and bool(torch.isnan(got["stretch"][k]))
                assert not bool(got["grid"][k].any()) and bool((got["gt_nor"][k] == 0.5).all())
        if clamp:
            clamped |= bool(((got["gt_nor"] == 0) | (got["gt_nor"] == 1)).any())
        else:
            beyond |= bool((got["gt_nor"] > 1).any())
    assert clamped and beyond     # the clamp had something to do, and without it labels left [0, 1]


def test_head_edge_frames_into_sentinel_filled_outputs(pkg):
    R = 8
    d36, o36, h36 = mr.frames36()
    good = [mr.frame(d36, o36, h36, i) for i in range(6)]

    def with_depth(i, fill):
        return np.full_like(good[i][0], fill), good[i][1], good[i][2]

    one = with_depth(3, 0.0)
    one[0][len(one[0]) // 2] = 600.0                               # one valid pixel: zero extent, a finite centre
    parts = [good[0], good[1], good[2], with_depth(2, 0.0), one, with_depth(4, np.nan), with_depth(4, 0.5), good[5], good[0]]
    depth, off, hdr = mr.concat(parts)
    hdr = hdr.copy()
    hdr[1, 4] += 1                                                 # bbox area != payload
    hdr[2, 4] = hdr[2, 2]                                          # right == left
    depth = depth[:-5]                                             # the last frame's payload ends past the buffer
    d, o, h = up(depth, off, hdr)
    base = pkg.obb_xforms(d, o, h).xforms
    base[7, 1] = float("nan")                                      # a NaN in a base row: every x of frame 7 is NaN
    centres = pkg.map_grids(d, o, h, base, res=R).mid_p
    gt = torch.from_numpy(np.random.default_rng(3).normal(0, 80, (9, 21, 3)).astype(np.float32)).to(dev())
    gt[:, :, 2] -= 450
    state = pkg.aug_state(KEY, 7, device=dev())
    idx, = up(np.array([8, 7, 6, 5, 4, 3, 2, 1, 0, 9, -1, 4, 0], np.int64))
    for ti in (None, idx):
        n = 9 if ti is None else len(idx)
        for clamp in (True, False):
            kw = dict(base=base, index=ti, gt=gt, res=R, clamp=clamp)
            out = sentinel_out(pkg, n, (21, 3))
            got = head(pkg, d, o, h, centres, state, out=out, **kw)
            want = chain(pkg, d, o, h, centres, state, **kw)
            torch.cuda.synchronize()
            assert got["xforms"] is out.xforms and got["grid"] is out.grid and got["gt_nor"] is out.gt_nor
            assert_same(got, want, (ti is None, clamp))
        st = got["status"].tolist()
        assert st == ([0, 2, 2, 1, 1, 1, 1, 1, 2] if ti is None else [2, 1, 1, 1, 1, 1, 2, 2, 0, 2, 2, 1, 0])
        assert float(got["max_l"][4]) == 0 and bool(got["mid_p"][4].any())     # frame 4: the zero extent keeps its centre
        bad = got["status"] != 0
        assert not bool(got["grid"][bad].any()) and bool((got["gt_nor"][bad] == 0.5).all())
        assert not bool(torch.isnan(got["grid"]).any()) and not bool(torch.isnan(got["max_l"]).any())
    # the same frames without a base: the placement's own statuses
    got = head(pkg, d, o, h, centres, state, gt=gt, res=R, out=sentinel_out(pkg, 9, (21, 3)))
    want = chain(pkg, d, o, h, centres, state, gt=gt, res=R)
    torch.cuda.synchronize()
    assert_same(got, want, "nobase")
    assert got["status"].tolist() == [0, 2, 2, 1, 1, 1, 1, 0, 2]
    # the optional outputs may be NULL: the row alone
    S = pkg._lib.load_mapstep()
    xf = torch.empty((9, 24), dtype=torch.float64, device=dev())
    grid = torch.full((9, 8), float("nan"), device=dev())
    rc = S.tsdf_map_step_head_hip(d.data_ptr(), d.numel(), o.data_ptr(), h.data_ptr(), 9, None, 9, R, 241.42, 160.0, 120.0,
                                  1.0, 3.0, centres.data_ptr(), None, state.data_ptr(), None, None, 0, 1,
                                  torch.cuda.current_stream().cuda_stream, xf.data_ptr(), grid.data_ptr(), None, None, None,
                                  None, None, None, None)
    torch.cuda.synchronize()
    assert rc == 0 and same(grid, got["grid"]) and same(xf, got["xforms"])


def test_head_under_another_camera_equals_the_chain_under_it(pkg):
    """The entry takes its camera by value: every constant reaches the kernel (the chain's entries take the struct)."""
    d, o, h, base, _, c_obb, gt = _pack36(pkg)
    state = pkg.aug_state(KEY, 9, device=dev())
    idx, = up(np.array([0, 11, 35, 34, 20, 11], np.int64))
    default = head(pkg, d, o, h, c_obb, state, base=base, index=idx, gt=gt, res=16)
    for consts in ((300.5, 150.25, 130.75, 1.0, 3.0), (241.42, 160.0, 120.0, 450.0, 3.0), (241.42, 160.0, 120.0, 1.0, 5.5)):
        cam = pkg.TsdfCam(*consts)
        got = head(pkg, d, o, h, c_obb, state, base=base, index=idx, gt=gt, res=16, cam=cam)
        U, stretch, rot = pkg.aug_xforms_at(c_obb, state, index=idx, return_params=True)
        T = pkg.compose_xforms(U, base, idx)
        mg = pkg.map_grids(d, o, h, T, res=16, cam=cam, index=idx)
        gaug = pkg.transform_joints(gt.index_select(0, idx), T)
        gnor = pkg.normalize_joints(gaug, mg.max_l, mg.mid_p)
        torch.cuda.synchronize()
        want = dict(zip(FIELDS, (T, mg.grid, mg.max_l, mg.mid_p, mg.status, gaug, gnor, stretch, rot)))
        assert_same(got, want, consts)
        assert consts[3] != 1.0 or not same(got["grid"], default["grid"]), consts    # focal, centre, trunc: they mattered
    with pytest.raises(pkg.TsdfError):
        pkg.map_step_head(d, o, h, c_obb, state, cam=pkg.TsdfCam(0.0, 160.0, 120.0, 1.0, 3.0))


def test_head_every_frame_alone_equals_its_row_in_the_batch(pkg):
    R = 32
    d, o, h, base, _, c_obb, gt = _pack36(pkg)
    state = pkg.aug_state(KEY, WRAP, device=dev())
    whole = head(pkg, d, o, h, c_obb, state, base=base, gt=gt, res=R)
    again = head(pkg, d, o, h, c_obb, state, base=base, gt=gt, res=R)
    torch.cuda.synchronize()
    assert_same(again, whole, "determinism")
    depth, off, hdr = mr.frames36()
    for i in range(36):
        fd, fo, fh = up(*mr.frame(depth, off, hdr, i))
        cnt = torch.tensor([i], dtype=torch.int64, device=dev())
        alone = head(pkg, fd, fo, fh, c_obb[i:i + 1].contiguous(), state, base=base[i:i + 1].contiguous(), counters=cnt,
                     gt=gt[i:i + 1].contiguous(), res=R)
        for name in FIELDS:
            assert same(alone[name], whole[name][i:i + 1]), (i, name)


def test_head_without_the_placement_writes_the_maps_alone(pkg):
    d, o, h, base, _, c_obb, _ = _pack36(pkg)
    nan_depth = torch.full_like(d, float("nan"))
    state = pkg.aug_state(KEY, 3, device=dev())
    idx, cnt = up(np.array([5, 35, -1, 0, 36, 5, 20], np.int64), np.array([9, -9, 0, 1, 2, 3, 1 << 50], np.int64))
    for kw in (dict(base=base, index=idx, counters=cnt), dict(base=None, index=idx), dict(base=base)):
        n = 7 if "index" in kw else 36
        out = sentinel_out(pkg, n)
        b, stretch, rot = pkg.map_step_head(nan_depth, o, h, c_obb, state, place=False, out=out, return_params=True, **kw)
        want = chain(pkg, d, o, h, c_obb, state, **kw)
        torch.cuda.synchronize()
        assert b.xforms is out.xforms and b[1:] == (None,) * 6
        assert same(b.xforms, want["xforms"]) and same(stretch, want["stretch"]) and same(rot, want["rot"])
        assert bool(torch.isnan(out.grid).all()) and bool(torch.isnan(out.max_l).all()) and bool((out.status == -7).all())
        full = pkg.map_step_head(d, o, h, c_obb, state, **kw)
        assert same(full.xforms, b.xforms)
    with pytest.raises(ValueError, match="place"):
        pkg.map_step_head(d, o, h, c_obb, state, place=False, gt=torch.zeros((36, 63), device=dev()))
    with pytest.raises(ValueError):
        pkg.map_step_head(d, o, h, c_obb[:35].contiguous(), state)
    with pytest.raises(ValueError):
        pkg.map_step_head(d, o, h, c_obb, state, base=base[:35].contiguous())
    with pytest.raises(ValueError):
        pkg.map_step_head(d, o, h, c_obb, state, index=idx, counters=cnt[:3])
    with pytest.raises(ValueError):
        pkg.map_step_head(d, o, h, c_obb, state, res=10)
    assert pkg.map_step_head(d, o, h, c_obb, state, index=idx[:0]).grid.shape == (0, 8)


def test_head_reads_the_state_when_it_runs(pkg):
    d, o, h, base, _, c_obb, gt = _pack36(pkg)
    s1, s2 = pkg.aug_state(KEY, 0, device=dev()), pkg.aug_state(KEY ^ 0xFFFF, WRAP, device=dev())
    state = s1.clone()
    kw = dict(base=base, gt=gt, res=32)
    a = head(pkg, d, o, h, c_obb, state, **kw)
    state.copy_(s2)                                                # queued between two identical launches
    b = head(pkg, d, o, h, c_obb, state, **kw)
    wa, wb = chain(pkg, d, o, h, c_obb, s1, **kw), chain(pkg, d, o, h, c_obb, s2, **kw)
    torch.cuda.synchronize()
    assert_same(a, wa, "first state")
    assert_same(b, wb, "second state")
    for name in ("xforms", "grid", "gt_nor", "stretch"):
        assert not same(a[name], b[name]), name


# ---- AugmentedStep(base=, fused_head=) ----
@functools.lru_cache(maxsize=None)
def _labelled(pkg):
    """The 10 crops and one crop without a valid pixel on the GPU, with OBB maps and joints near every grid centre."""
    depth, off, hdr = mr.frames36()
    d10 = (depth[:off[10]], off[:11], hdr[:10])
    f4 = mr.frame(depth, off, hdr, 4)
    depth, off, hdr = mr.concat([d10, (np.zeros_like(f4[0]),) + f4[1:]])
    mid = oracle.voxelize(depth[:off[10]], off[:11], hdr[:10], R=32, want_tsdf=False)["mid_p"]
    mid = np.concatenate([mid, mid[4:5]])
    gt = (mid[:, None, :] + np.random.default_rng(7).normal(0, 40, (11, 21, 3))).astype(np.float32).reshape(11, 63)
    d, o, h, g = up(depth, off, hdr, gt)
    base = pkg.obb_xforms(d, o, h)
    assert base.status.tolist() == [0] * 10 + [1]
    return (depth, off, hdr, gt), (d, o, h, g), base.xforms


STEPS = [([3, 1, 7, 7, 0, 2], 0xABCDEF, 0), ([9, 8, 10, 5, 4, 6], 0xABCDEF, WRAP), ([0, 1, 2, 3, 4, 5], 12345, 1 << 40)]


def _snap(res):
    o, nor, aug = res
    return tuple(t.clone() for t in (*o, nor, aug))


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_augmented_step_in_the_base_frame(pkg, kind):
    dt = None if kind == "f32" else torch.bfloat16
    n, R = 6, 32
    _, (d, o, h, g), base = _labelled(pkg)
    kw = dict(gt=g, res=R, dtype=dt, base=base)
    graph = pkg.AugmentedStep(d, o, h, n, graph=True, **kw)
    eager = pkg.AugmentedStep(d, o, h, n, graph=False, **kw)
    assert graph.graph is not None and eager.graph is None
    centres = pkg.map_grids(d, o, h, base, res=R).mid_p
    torch.cuda.synchronize()
    assert same(graph.centres, centres) and same(eager.centres, centres)   # the base-frame grid centres
    before = None
    for index, key, c0 in STEPS:
        got = _snap(graph.step(index, key, c0))
        xf = graph.xforms.clone()
        ref = _snap(eager.step(index, key, c0))
        # the chain by hand
        ti = torch.tensor(index, dtype=torch.int64, device=dev())
        U = pkg.aug_xforms_at(centres, pkg.aug_state(key, c0, device=dev()), index=ti)
        T = pkg.compose_xforms(U, base, ti)
        if dt is None:
            hand = pkg.voxelize_indexed(d, o, h, ti, g, res=R, xforms=T, gt_copy=True)
        else:
            hand = pkg.voxelize_aug_lowp(d, o, h, T, res=R, dtype=dt, gt=g, index=ti)
        torch.cuda.synchronize()
        hand = (*hand[0], hand[1], hand[2])
        assert same(xf, T) and same(eager.xforms, T) and not same(T, U)
        assert got[0].dtype is (dt or torch.float32) and bool(got[0].any())
        for k in range(6):
            assert same(got[k], ref[k]), ("graph vs eager", k)
            assert same(got[k], hand[k]), ("graph vs chain", k)
        assert got[3].tolist() == [1 if i == 10 else 0 for i in index]
        assert before is None or not same(before, got[0])                      # another step, other volumes
        before = got[0]


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_fused_head_without_a_base_equals_the_default_step(pkg, kind):
    dt = None if kind == "f32" else torch.bfloat16
    n, R = 6, 32
    _, (d, o, h, g), _ = _labelled(pkg)
    centres = pkg.aabb(d, o, h, res=R).grid[:, :3].contiguous()
    kw = dict(gt=g, centres=centres, res=R, dtype=dt)
    plain = pkg.AugmentedStep(d, o, h, n, graph=True, **kw)
    fused = pkg.AugmentedStep(d, o, h, n, graph=True, fused_head=True, **kw)
    bare = pkg.AugmentedStep(d, o, h, n, graph=False, fused_head=True, centres=centres, res=R, dtype=dt)
    for index, key, c0 in STEPS:
        want = _snap(plain.step(index, key, c0))
        got = _snap(fused.step(index, key, c0))
        o_b = bare.step(index, key, c0)
        torch.cuda.synchronize()
        for k in range(6):
            assert same(got[k], want[k]), k
        assert same(fused.xforms, plain.xforms)
        assert isinstance(o_b, pkg.TsdfBatch) and all(same(x, y) for x, y in zip(o_b, want[:4]))   # without labels


# ---- what the composed step means ----
def test_composed_step_against_the_oracle(pkg):
    n, R = 10, 32
    (depth, off, hdr, gt), (d, o, h, g), base = _labelled(pkg)
    depth, off, hdr, gt = depth[:off[10]], off[:11], hdr[:10], gt[:10]
    index = list(range(10))
    f32 = pkg.AugmentedStep(d, o, h, n, gt=g, res=R, base=base, graph=False)
    bf = pkg.AugmentedStep(d, o, h, n, gt=g, res=R, base=base, graph=False, dtype=torch.bfloat16)
    o32, nor32, aug32 = f32.step(index, KEY, 11)
    o16, nor16, aug16 = bf.step(index, KEY, 11)
    torch.cuda.synchronize()
    T = f32.xforms.cpu().numpy()
    assert same(bf.xforms, f32.xforms)
    # the maps are compositions: the augmentation about the OBB-frame centre, after the OBB map
    U = pkg.aug_xforms_at(f32.centres, pkg.aug_state(KEY, 11, device=dev()), index=f32.index).cpu().numpy()
    assert np.array_equal(T.view(np.uint64), mr.compose_np(U, base.cpu().numpy()[:10]).view(np.uint64))
    want = oracle.voxelize_aug(depth, off, hdr, T, R=R)
    assert not want["status"].any() and o32.status.tolist() == [0] * 10 and o16.status.tolist() == [0] * 10
    ref = torch.from_numpy(want["tsdf"]).to(dev())
    assert bool((ref.abs() < 1).logical_and(ref != 0).any())
    assert float((o32.tsdf - ref).abs().max()) <= TOL
    assert in_band(o16.tsdf, ref, TOL)
    want_aug = oracle.transform_joints(gt, T)
    want_nor = oracle.normalize_joints(want_aug, want["max_l"], want["mid_p"])
    for out, nor, aug in ((o32, nor32, aug32), (o16, nor16, aug16)):
        assert np.array_equal(out.max_l.cpu().numpy().view(np.uint32), want["max_l"].view(np.uint32))
        assert np.array_equal(out.mid_p.cpu().numpy().view(np.uint32), want["mid_p"].view(np.uint32))
        assert np.array_equal(aug.cpu().numpy().view(np.uint32), want_aug.view(np.uint32))
        assert np.array_equal(nor.cpu().numpy().view(np.uint32), want_nor.view(np.uint32))
