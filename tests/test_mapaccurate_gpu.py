"""GPU tier of the accurate directional TSDF under a per-frame map (include/tsdf_mapaccurate.h):
tsdf_map_grid_accurate_kernel against the brute-force float64 reference of tests/mapaccurate_ref.py under
``accurate_ref.compare`` — outside the fragile set ``nearest`` is equal, far voxels are bit-exact, near values lie within
1e-5; the fragile set may hold at most 1e-4 of a case's voxels (it is empty on every input here:
tests/test_mapaccurate_cpu.py, tests/test_window_cpu.py) —, the sparse frames that reach the edges of the search window
(tests/sparse_ref.py), then the batch behaviour, bad inputs, another camera, graph capture, the relation to the
plain accurate pass and the consumers.  The references are computed once per case, shared and never modified."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accurate_ref as ar  # noqa: E402
import map_geom_ref as mg  # noqa: E402
import mapaccurate_ref as mr  # noqa: E402
import sparse_ref as sp  # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = ("czyx", "cxyz")


def dev():
    return torch.device("cuda")


def up(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev()) for a in arrays)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return a.dtype is b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def check(got, nn, cases, layout, label):
    """Positions of a batch against their cases' references, one by one under the rules."""
    got, nn = got.cpu().numpy(), nn.cpu().numpy()
    for i, c in enumerate(cases):
        r = c["ref"]
        wv, (wn, wf) = ar.to_layout(r["vol"], (r["nearest"], r["fragile"]), layout)
        ar.compare(got[i:i + 1], nn[i:i + 1], wv[None], wn[None], wf[None], f"{label}[{i}] {layout}")


def run(pkg, keys, R, layout, label, cam=None):
    """The cases ``keys`` (all at R) as one batch on the GPU, compared; returns (tsdf, nearest)."""
    depth, off, hdr, xf, grid, cs = mr.batch(keys)
    td, to, th, tx, tg = up(depth, off, hdr, xf, grid)
    tsdf, st, nn = pkg.voxelize_map_grid_accurate(td, to, th, tx, tg, res=R, layout=layout, nearest=True, cam=cam)
    torch.cuda.synchronize()
    n = len(keys)
    assert tsdf.shape == (n, 3, R, R, R) and tsdf.dtype is torch.float32 and nn.shape == (n, R, R, R) and nn.dtype is torch.int32
    assert st.tolist() == [0] * n
    check(tsdf, nn, cs, layout, label)
    return tsdf, nn


# ---- against the reference ----
@pytest.mark.parametrize("name", mg.MAPS)
def test_every_map_on_two_crops(pkg, name):
    keys = [k for _, k in mr.PAIRS_R12 if k[2] == name]
    assert len(keys) == 2
    for layout in LAYOUTS:
        run(pkg, keys, 12, layout, name)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", mr.NON_EXACT)
def test_ragged_last_slab(pkg, name, layout):
    key, = [k for _, k in mr.PAIRS_R20 if k[2] == name]
    run(pkg, [key], 20, layout, f"{name} R=20")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("R", [4, 64])
def test_slab_edge_cases(pkg, R, layout):
    # R = 4: one slab holds the frame; R = 64: one slice per slab
    key, = [k for _, k in mr.SLAB_EDGES if k[3] == R]
    run(pkg, [key], R, layout, f"general small_odd R={R}")


@pytest.mark.parametrize("label,key", mr.NO_RECTANGLE, ids=[c[0].replace(" ", "_") for c in mr.NO_RECTANGLE])
def test_mixed_sign_and_negative_depth(pkg, label, key):
    # voxels within the truncation distance of the camera plane have no finite rectangle: the whole crop is walked
    for layout in LAYOUTS:
        run(pkg, [key], 12, layout, label)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_shifted_grid_most_voxels_far(pkg, layout):
    (label, key), = mr.SHIFTED
    assert mr.case(*key)["ref"]["near"].mean() < 0.5
    _, nn = run(pkg, [key], 12, layout, label)
    assert bool((nn == -1).any()) and bool((nn >= 0).any())


def test_inverse_rows_that_are_not_the_inverse(pkg):
    # the identity's inverse rows under rx100: the projection (sign, rejection) follows them, the distances and the search
    # window follow the FORWARD rows — a window derived from the caller's inverse would miss the nearest pixels
    (label, key), = mr.WRONG_INVERSE
    proper = ("synth", 0, "rx100", 12, None, None)
    for layout in LAYOUTS:
        tsdf, nn = run(pkg, [key, proper], 12, layout, label)
        a, b = mr.case(*key)["ref"], mr.case(*proper)["ref"]
        assert np.array_equal(a["near"], b["near"]) and np.array_equal(a["nearest"], b["nearest"])   # the same search
        assert torch.equal(nn[0], nn[1]) and not torch.equal(bits(tsdf[0]), bits(tsdf[1]))           # another sign rule


def test_broken_forward_parts_among_good_positions(pkg):
    keys = [("synth", 0, "identity", 12, None, None), ("synth", 0, "singular", 12, None, None),
            ("synth", 0, "rx100", 12, None, None), ("synth", 0, "nanfwd", 12, None, None),
            ("synth", 0, "general", 12, None, None)]
    for layout in LAYOUTS:
        tsdf, nn = run(pkg, keys, 12, layout, "broken")
        assert bool((nn[1] >= 0).any())                                # diag(1, 1, 0): just arithmetic, some voxels near
        assert bool((nn[3] == -1).all()) and not bool(torch.isnan(tsdf[3]).any())    # a NaN s wins no comparison


# ---- the search window ----
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(sp.MAPPED))
def test_sparse_frames_reach_the_search_windows_edges(pkg, name, layout):
    """The sparse frames of tests/sparse_ref.py under shear / aniso / general / rx100 and their own cameras: inputs on which
    a search window that is slightly too small loses the nearest pixel (tests/test_window_cpu.py counts what each mistake
    would lose on them) — a frame of negative depths, a grid that reaches within the window's depth half-extent of the
    camera plane (items with no finite rectangle next to windowed ones), a crop box whose four sides cut windows."""
    c = sp.mapped_case(name)
    R = c["R"]
    td, to, th, tx, tg = up(c["depth"], c["off"], c["hdr"], c["xf"], c["grid"])
    tsdf, st, nn = pkg.voxelize_map_grid_accurate(td, to, th, tx, tg, res=R, layout=layout, nearest=True,
                                                  cam=None if c["cam"] is None else pkg.TsdfCam(*c["cam"]))
    torch.cuda.synchronize()
    assert tsdf.shape == (1, 3, R, R, R) and nn.shape == (1, R, R, R) and st.tolist() == [0]
    check(tsdf, nn, [c], layout, f"sparse {name}")


# ---- batch behaviour ----
MAPS7 = ("identity", "rx100", "shear", "general", "obb", "x2", "cyc")


def _two_sources():
    """Crops 0 and 3 as a pack of two SOURCE frames, and positions (crop, map) drawn from them through an index."""
    pos = [(c, m) for m in MAPS7 for c in mr.CROPS_R12]
    pos = [pos[k] for k in np.random.default_rng(14).permutation(len(pos))] + [(0, "general"), (0, "general"), (3, "x2")]
    cs = [mr.case("synth", c, m, 12) for c, m in pos]
    srcs = [mr.source("synth", c) for c in mr.CROPS_R12]
    depth = np.concatenate([s[0] for s in srcs])
    off = np.cumsum([0] + [s[0].size for s in srcs]).astype(np.int64)
    hdr = np.stack([s[1] for s in srcs])
    index = np.array([mr.CROPS_R12.index(c) for c, _ in pos], np.int64)
    return depth, off, hdr, index, np.concatenate([c["xf"] for c in cs]), np.concatenate([c["grid"] for c in cs]), cs


def test_one_source_frame_at_several_positions_independence_and_determinism(pkg):
    R = 12
    depth, off, hdr, index, xf, grid, cs = _two_sources()
    td, to, th, ti, tx, tg = up(depth, off, hdr, index, xf, grid)
    n = len(cs)
    for layout in LAYOUTS:
        kw = dict(res=R, layout=layout, nearest=True)
        whole, st, wn = pkg.voxelize_map_grid_accurate(td, to, th, tx, tg, index=ti, **kw)
        again, _, an = pkg.voxelize_map_grid_accurate(td, to, th, tx, tg, index=ti, **kw)
        torch.cuda.synchronize()
        assert st.tolist() == [0] * n and same(whole, again) and same(wn, an)
        check(whole, wn, cs, layout, "indexed")
        assert same(whole[-3], whole[-2]) and same(wn[-3], wn[-2])     # the same (frame, map, row) twice: the same bits
        # a permutation with repeats of the positions: every position's bits are its own
        perm = torch.from_numpy(np.random.default_rng(15).integers(0, n, 25)).to(dev())
        g, st, gn = pkg.voxelize_map_grid_accurate(td, to, th, tx[perm].contiguous(), tg[perm].contiguous(), index=ti[perm], **kw)
        assert not bool(st.any()) and same(g, whole[perm]) and same(gn, wn[perm])
        for i in (0, 5, n - 1):                                        # n = 1, without an index: the same bits alone
            c = cs[i]
            alone, st, aln = pkg.voxelize_map_grid_accurate(*up(c["depth"], c["off"], c["hdr"], c["xf"], c["grid"]), **kw)
            assert st.tolist() == [0] and same(alone[0], whole[i]) and same(aln[0], wn[i]), i
    # out= a view of a larger buffer: the rest of it stays untouched; without `nearest` the result has two members
    buf = torch.full((n + 2, 3, R, R, R), 7.0, dtype=torch.float32, device=dev())
    res = pkg.voxelize_map_grid_accurate(td, to, th, tx, tg, res=R, layout="cxyz", index=ti, out=buf[1:n + 1])
    torch.cuda.synchronize()
    assert len(res) == 2 and res[0].data_ptr() == buf[1].data_ptr()
    assert same(buf[1:n + 1], whole) and bool((buf[0] == 7.0).all()) and bool((buf[n + 1] == 7.0).all())


def test_large_batch_takes_whole_slabs(pkg):
    # a small batch is cut into one-slice workgroups; from 1024 workgroups on a workgroup owns slab.inc's slab: at R = 20 that
    # is 6 slices, the last slab ragged (2), at R = 12 the whole frame.  A voxel's bits do not depend on the slab it is in.
    for R, n, keys in ((20, 300, [k for _, k in mr.PAIRS_R20[:3]]),
                       (12, 1100, [k for _, k in mr.PAIRS_R12 if k[2] in ("general", "obb", "mirror")][:5])):
        depth, off, hdr, xf, grid, cs = mr.batch(keys)
        td, to, th, tx, tg = up(depth, off, hdr, xf, grid)
        idx = torch.arange(n, dtype=torch.int64, device=dev()) % len(keys)
        for layout in LAYOUTS:
            kw = dict(res=R, layout=layout, nearest=True)
            few, st2, n2 = pkg.voxelize_map_grid_accurate(td, to, th, tx, tg, **kw)       # one slice per workgroup
            check(few, n2, cs, layout, f"R={R}")
            many, st, nn = pkg.voxelize_map_grid_accurate(td, to, th, tx[idx].contiguous(), tg[idx].contiguous(), index=idx, **kw)
            torch.cuda.synchronize()
            assert not bool(st.any()) and not bool(st2.any())
            assert same(many, few[idx]) and same(nn, n2[idx]), (R, layout)


# ---- bad inputs ----
def test_bad_inputs_among_good_positions(pkg):
    R = 12
    keys = [k for _, k in mr.PAIRS_R12 if k[2] in ("identity", "shear", "general")]      # six positions, six source frames
    depth, off, hdr, xf, grid, cs = mr.batch(keys)
    td, to, th, tx, tg = up(depth, off, hdr, xf, grid)
    clean, st, cn = pkg.voxelize_map_grid_accurate(td, to, th, tx, tg, res=R, nearest=True)
    torch.cuda.synchronize()
    assert not bool(st.any()) and all(bool(clean[i].any()) for i in range(6))
    A, n = pkg._lib.load_mapaccurate(), 6
    cam = pkg.default_cam()

    def raw(d, dlen, o, h, x, g, index=None, n_out=n):
        """The entry itself into NaN-filled buffers: every byte of every output must be written."""
        out = torch.full((n_out, 3, R, R, R), float("nan"), dtype=torch.float32, device=dev())
        nn = torch.full((n_out, R, R, R), 0x7fc00000, dtype=torch.int32, device=dev())        # a NaN's bits
        stt = torch.full((n_out,), -7, dtype=torch.int32, device=dev())
        rc = A.tsdf_voxelize_map_grid_accurate_hip(d.data_ptr(), dlen, o.data_ptr(), h.data_ptr(), h.shape[0],
                                                   index.data_ptr() if index is not None else None, n_out, R, cam.focal, cam.cx,
                                                   cam.cy, cam.invalid_eps, cam.trunc_voxels, 0, None, x.data_ptr(), g.data_ptr(),
                                                   out.data_ptr(), nn.data_ptr(), stt.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        return out, nn, stt

    def verify(out, nn, stt, want_status):
        assert stt.tolist() == want_status
        assert not bool(torch.isnan(out).any())
        for k, s in enumerate(want_status):
            if s:
                assert not bool(bits(out[k]).any()) and bool((nn[k] == -1).all()), k          # +0 everywhere, nearest -1
            else:
                assert same(out[k], clean[k]) and same(nn[k], cn[k]), k

    # bad headers: an area that contradicts the payload, an empty box, a payload outside the buffer
    h2 = hdr.copy()
    h2[1, 4] += 1
    h2[3, 4] = h2[3, 2]
    verify(*raw(td, td.numel(), to, up(h2)[0], tx, tg), [0, 2, 0, 2, 0, 0])
    verify(*raw(td, int(off[6]) - 5, to, th, tx, tg), [0, 0, 0, 0, 0, 2])
    # an index outside the tables: positions 1, 3 and 5 name no source frame, the others their own
    idx = np.array([0, -1, 2, 6, 4, 2 ** 40], np.int64)
    verify(*raw(td, td.numel(), to, th, tx, tg, index=up(idx)[0]), [0, 2, 0, 2, 0, 2])
    # unusable grid rows (the POSITION's): trunc_dis zero / negative, a NaN origin, an infinite voxel_len, a NaN trunc_dis
    g2 = grid.copy()
    g2[0, 4], g2[1, 4], g2[2, 1], g2[4, 3], g2[5, 4] = 0.0, -1.0, np.nan, np.inf, np.nan
    verify(*raw(td, td.numel(), to, th, tx, up(g2)[0]), [1, 1, 1, 0, 1, 1])
    # a bad header wins over a bad row
    verify(*raw(td, td.numel(), to, up(h2)[0], tx, up(g2)[0]), [1, 2, 1, 2, 1, 1])
    # a crop without a valid pixel (zeros, below eps, NaN): status 0, a zero volume, nothing near
    for fill in (0.0, 0.5, np.nan):
        dz = depth.copy()
        dz[off[1]:off[2]] = fill
        out, nn, stt = raw(up(dz)[0], td.numel(), to, th, tx, tg)
        assert stt.tolist() == [0] * 6 and not bool(bits(out[1]).any()) and bool((nn[1] == -1).all())
        assert same(out[0], clean[0]) and same(out[2], clean[2])
    # the wrapper's own refusals, and the empty batch
    with pytest.raises(ValueError):
        pkg.voxelize_map_grid_accurate(td, to, th, tx, tg[:2], res=R)
    with pytest.raises(ValueError):
        pkg.voxelize_map_grid_accurate(td, to, th, tx[:2], tg, res=R)
    with pytest.raises(TypeError):
        pkg.voxelize_map_grid_accurate(td, to, th, tx.float(), tg, res=R)
    with pytest.raises(TypeError):
        pkg.voxelize_map_grid_accurate(td, to, th, tx, tg, res=R, out=torch.empty((6, 3, R, R, R), dtype=torch.float16, device=dev()))
    with pytest.raises(ValueError):
        pkg.voxelize_map_grid_accurate(td, to, th, tx, tg, res=10)
    e, est, en = pkg.voxelize_map_grid_accurate(td, to, th, tx[:0], tg[:0], res=R, index=up(idx[:0])[0], nearest=True)
    assert e.shape == (0, 3, R, R, R) and est.shape == (0,) and en.shape == (0, R, R, R)


# ---- another camera ----
def test_non_default_camera(pkg):
    (label, key), = mr.camera_pairs()
    hc = pkg.TsdfCam(*key[5])
    for layout in LAYOUTS:
        tsdf, _ = run(pkg, [key], 12, layout, label, cam=hc)
    # the camera is read: the default one gives another volume
    c = mr.case(*key)
    other, _ = pkg.voxelize_map_grid_accurate(*up(c["depth"], c["off"], c["hdr"], c["xf"], c["grid"]), res=12, layout="cxyz")
    assert not same(other, tsdf)


# ---- graph capture ----
def test_capture_into_a_graph_two_replays(pkg):
    d, R = dev(), 12
    depth, off, hdr, index, xf, grid, cs = _two_sources()
    changed = (depth * 1.01).astype(np.float32)
    td, to, th, ti, tx, tg = up(depth, off, hdr, index, xf, grid)
    n = len(cs)
    out = torch.empty((n, 3, R, R, R), dtype=torch.float32, device=d)

    def step():
        return pkg.voxelize_map_grid_accurate(td, to, th, tx, tg, res=R, index=ti, out=out, nearest=True)

    step()                                   # eagerly once: library loads and the device check happen here
    torch.cuda.synchronize()
    first = out.clone()
    side = torch.cuda.Stream(d)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _, st, nn = step()
    for k, src in enumerate((changed, depth)):               # two replays, on two depth buffers
        td.copy_(torch.from_numpy(src))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        have, have_st, have_nn = out.clone(), st.clone(), nn.clone()
        eager, eager_st, eager_nn = pkg.voxelize_map_grid_accurate(td, to, th, tx, tg, res=R, index=ti, nearest=True)
        torch.cuda.synchronize()
        assert same(have, eager) and same(have_st, eager_st) and same(have_nn, eager_nn), k
        assert same(have, first) == (k == 1)                  # the depth did change the volumes, and changed them back


# ---- the plain accurate pass ----
def test_identity_map_against_the_plain_accurate_pass(pkg):
    R = 12
    for crop in mr.CROPS_R12:
        c = mr.case("synth", crop, "identity", R)
        plain = ar.accurate_frame(c["depth"], c["hdr"][0], c["grid"][0, :3], c["grid"][0, 3], c["grid"][0, 4], R)
        fragile = c["ref"]["fragile"] | plain["fragile"]
        assert fragile.mean() <= ar.FRAGILE_CAP
        td, to, th, tx, tg = up(c["depth"], c["off"], c["hdr"], c["xf"], c["grid"])
        for layout in LAYOUTS:
            a, _, an = pkg.voxelize_grid_accurate(td, to, th, tg, res=R, layout=layout, nearest=True)
            m, _, mn = pkg.voxelize_map_grid_accurate(td, to, th, tx, tg, res=R, layout=layout, nearest=True)
            torch.cuda.synchronize()
            ok = torch.from_numpy(ar.to_layout(c["ref"]["vol"], (~fragile,), layout)[1][0]).to(dev())
            assert torch.equal(an[0][ok], mn[0][ok]) and bool((mn >= 0).any())
            err = float((a[0] - m[0]).abs()[:, ok].max())
            print(f"identity crop{crop} {layout}: mapped vs plain accurate, largest difference {err:.3g}")
            assert err <= ar.TOL


# ---- the consumers ----
def _labelled6(pkg):
    """The six synthetic crops on the GPU with joints near every grid centre: (d, o, h, gt)."""
    depth, off, hdr = mr._synth6()
    mid = np.stack([mg.centre(depth[off[i]:off[i + 1]], hdr[i]) for i in range(6)])
    gt = (mid[:, None, :] + np.random.default_rng(7).normal(0, 40, (6, 21, 3))).astype(np.float32).reshape(6, 63)
    return up(depth, off, hdr, gt)


def test_voxelize_aug_accurate_is_its_chain(pkg):
    d, o, h, g = _labelled6(pkg)
    R = 12
    depth, off, hdr = mr._synth6()
    names = ["general", "obb", "rx100", "shear", "identity", "aniso"]
    xf, = up(mg.xforms_for(names, depth, off, hdr, ids=range(6)))
    index = torch.tensor([4, 0, 0, 5, 2], dtype=torch.int64, device=dev())
    for layout, idx in (("czyx", None), ("cxyz", index)):
        x = xf if idx is None else xf[:5].contiguous()
        want = pkg.voxelize_aug(d, o, h, x, res=R, layout=layout) if idx is None else \
            pkg.voxelize_indexed(d, o, h, idx, res=R, layout=layout, xforms=x)
        got, nor, aug = pkg.voxelize_aug_accurate(d, o, h, x, res=R, layout=layout, gt=g, index=idx)
        bare = pkg.voxelize_aug_accurate(d, o, h, x, res=R, layout=layout, index=idx)
        placed = pkg.map_grids(d, o, h, x, res=R, index=idx)
        vol, st = pkg.voxelize_map_grid_accurate(d, o, h, x, placed.grid, res=R, layout=layout, index=idx)
        lab = pkg.voxelize_aug_lowp(d, o, h, x, res=R, layout=layout, gt=g, index=idx)
        torch.cuda.synchronize()
        assert isinstance(got, pkg.TsdfBatch) and got.tsdf.dtype is torch.float32 and st.tolist() == [0] * x.shape[0]
        assert same(got.tsdf, vol) and same(bare.tsdf, vol)
        for name in ("max_l", "mid_p", "status"):                     # the placement's: voxelize_aug's bit for bit
            assert same(getattr(got, name), getattr(want, name)) and same(getattr(bare, name), getattr(want, name)), name
        assert same(nor, lab[1]) and same(aug, lab[2])
        proj = want.tsdf
        assert not same(got.tsdf, proj)
        assert int(((proj == 0).all(dim=1) & (got.tsdf != 0).any(dim=1)).sum()) > 0   # rejected voxels gain a value
        for dt in (torch.float16, torch.bfloat16):
            low = pkg.voxelize_aug_accurate(d, o, h, x, res=R, layout=layout, dtype=dt, index=idx)
            assert low.tsdf.dtype is dt and torch.equal(low.tsdf, vol.to(dt))
            assert same(low.max_l, want.max_l) and same(low.status, want.status)


def test_voxelize_obb_with_the_accurate_tsdf(pkg):
    d, o, h, g = _labelled6(pkg)
    R = 12
    for layout in LAYOUTS:
        base = pkg.voxelize_obb(d, o, h, res=R, layout=layout, gt=g)
        proj = pkg.voxelize_obb(d, o, h, res=R, layout=layout, gt=g, tsdf="projective")
        acc = pkg.voxelize_obb(d, o, h, res=R, layout=layout, gt=g, tsdf="accurate")
        xf = pkg.obb_xforms(d, o, h).xforms
        hand = pkg.voxelize_aug_accurate(d, o, h, xf, res=R, layout=layout, gt=g)
        torch.cuda.synchronize()
        assert len(acc) == 4 and same(acc[3], xf) and same(acc[3], base[3])
        assert same(acc[0].tsdf, hand[0].tsdf) and not same(acc[0].tsdf, base[0].tsdf)
        for name in ("max_l", "mid_p", "status"):
            assert same(getattr(acc[0], name), getattr(base[0], name)), name
        assert same(acc[1], base[1]) and same(acc[2], base[2])        # the labels
        assert all(same(x, y) for x, y in zip(base[0], proj[0])) and same(base[1], proj[1])   # the default is what it was
        bare, xf2 = pkg.voxelize_obb(d, o, h, res=R, layout=layout, tsdf="accurate", dtype=torch.bfloat16)
        assert bare.tsdf.dtype is torch.bfloat16 and torch.equal(bare.tsdf, acc[0].tsdf.to(torch.bfloat16)) and same(xf2, xf)
    with pytest.raises(ValueError, match="tsdf must be"):
        pkg.voxelize_obb(d, o, h, tsdf="exact")


STEPS = [([3, 1, 5, 5, 0, 2], 0xABCDEF, 0), ([4, 2, 0, 5, 1, 3], 0xABCDEF, 6), ([0, 1, 2, 3, 4, 5], 12345, 1 << 40)]


def _snap(res):
    o, nor, aug = res
    return tuple(t.clone() for t in (*o, nor, aug))


@pytest.mark.parametrize("head", ["chain", "fused_head", "base"])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_augmented_step_with_the_accurate_tsdf(pkg, kind, head):
    dt = None if kind == "f32" else torch.bfloat16
    n, R = 6, 12
    d, o, h, g = _labelled6(pkg)
    base = pkg.obb_xforms(d, o, h).xforms if head == "base" else None
    kw = dict(gt=g, res=R, dtype=dt, base=base, fused_head=head == "fused_head", layout="cxyz")
    graph = pkg.AugmentedStep(d, o, h, n, graph=True, tsdf="accurate", **kw)
    eager = pkg.AugmentedStep(d, o, h, n, graph=False, tsdf="accurate", **kw)
    proj = pkg.AugmentedStep(d, o, h, n, graph=False, **kw)
    assert graph.graph is not None and eager.graph is None and graph.out.tsdf.dtype is (dt or torch.float32)
    before = None
    for index, key, c0 in STEPS:
        got = _snap(graph.step(index, key, c0))
        xf = graph.xforms.clone()
        ref = _snap(eager.step(index, key, c0))
        want = _snap(proj.step(index, key, c0))
        ti = torch.tensor(index, dtype=torch.int64, device=dev())
        hand = pkg.voxelize_aug_accurate(d, o, h, xf, res=R, layout="cxyz", dtype=dt, gt=g, index=ti)
        torch.cuda.synchronize()
        hand = (*hand[0], hand[1], hand[2])
        assert same(xf, proj.xforms) and same(eager.xforms, xf)
        assert got[3].tolist() == [0] * n and bool(got[0].any())
        for k in range(6):
            assert same(got[k], ref[k]), ("graph vs eager", k)
            assert same(got[k], hand[k]), ("graph vs chain", k)
        for k in range(1, 6):                                          # scalars and labels: the projective step's
            assert same(got[k], want[k]), ("accurate vs projective", k)
        assert not same(got[0], want[0])
        assert before is None or not same(before, got[0])              # another step, other volumes
        before = got[0]
    # an unchanged replay equals the one before; without labels the step returns the batch alone
    again = _snap(graph.step(*STEPS[-1]))
    torch.cuda.synchronize()
    assert all(same(x, y) for x, y in zip(again, got))
    bare = pkg.AugmentedStep(d, o, h, n, res=R, dtype=dt, base=base, fused_head=head == "fused_head", layout="cxyz",
                             tsdf="accurate")
    ob = bare.step(*STEPS[-1])
    torch.cuda.synchronize()
    assert isinstance(ob, pkg.TsdfBatch) and all(same(x, y) for x, y in zip(ob, got[:4]))
    with pytest.raises(ValueError, match="tsdf must be"):
        pkg.AugmentedStep(d, o, h, n, tsdf="exact")
