"""GPU tier of the accurate directional TSDF (include/tsdf_accurate.h): tsdf_grid_accurate_kernel against the brute-force
float64 reference of tests/accurate_ref.py under that file's comparison rules — outside the fragile set ``nearest`` is
equal, far voxels are bit-exact, near values lie within 1e-5; the fragile set may hold at most 1e-4 of a case's voxels (it is
empty on every input here: tests/test_accurate_cpu.py, tests/test_window_cpu.py) —, the sparse frames that reach the
edges of the search window (tests/sparse_ref.py), then the batch behaviour, bad inputs, another camera, graph
capture and the consumers.  The references are computed once per case, shared and never modified."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accurate_ref as ar  # noqa: E402
import locate_ref as lr  # noqa: E402
import sparse_ref as sp  # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = ("czyx", "cxyz")


def dev():
    return torch.device("cuda")


def up(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev()) for a in arrays)


def bits(t):
    return t.contiguous().view(torch.int32)


def run_case(pkg, c, R, layout, label, cam=None):
    """One one-frame case of accurate_ref.case on the GPU, compared under the rules."""
    td, to, th, tg = up(c["depth"], c["off"], c["hdr"], c["grid"])
    tsdf, st, nn = pkg.voxelize_grid_accurate(td, to, th, tg, res=R, layout=layout, nearest=True, cam=cam)
    torch.cuda.synchronize()
    assert tsdf.shape == (1, 3, R, R, R) and tsdf.dtype is torch.float32 and nn.shape == (1, R, R, R) and nn.dtype is torch.int32
    assert st.tolist() == [0]
    r = c["ref"]
    wv, (wn, wf) = ar.to_layout(r["vol"], (r["nearest"], r["fragile"]), layout)
    ar.compare(tsdf.cpu().numpy(), nn.cpu().numpy(), wv[None], wn[None], wf[None], f"{label} {layout}")
    return tsdf, nn


# ---- against the reference ----
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("R", ar.SYNTH_RES)
@pytest.mark.parametrize("seed", ar.SYNTH_SEEDS)
def test_synthetic_crops(pkg, seed, R, layout):
    run_case(pkg, ar.case("synth", seed, R), R, layout, f"synth{seed} R={R}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("R", [4, 64])
def test_slab_edge_cases(pkg, R, layout):
    # R = 4: one slab holds the frame; R = 64: one slice per slab
    run_case(pkg, ar.case("golden", "small_odd", R), R, layout, f"small_odd R={R}")


@pytest.mark.parametrize("name", ar.GOLDEN)
def test_golden_fixtures(pkg, name):
    for R in ar.GOLDEN_RES:
        for layout in LAYOUTS:
            run_case(pkg, ar.case("golden", name, R), R, layout, f"{name} R={R}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_shifted_grid_most_voxels_far(pkg, layout):
    c = ar.case("synth", 1, 12, shifted=True)
    assert c["ref"]["near"].mean() < 0.5
    tsdf, nn = run_case(pkg, c, 12, layout, "synth1 R=12 shifted")
    assert bool((nn == -1).any()) and bool((nn >= 0).any())


# ---- the search window ----
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(sp.PLAIN))
def test_sparse_frames_reach_the_search_windows_edges(pkg, name, layout):
    """The sparse frames of tests/sparse_ref.py, under their own cameras: inputs on which a search window that is slightly
    too small loses the nearest pixel (tests/test_window_cpu.py counts what each mistake would lose on them) — a frame of
    negative depths, a grid that reaches within T of the camera plane (items with no finite rectangle next to windowed ones),
    a crop box whose four sides cut windows."""
    c = sp.plain_case(name)
    run_case(pkg, c, c["R"], layout, f"sparse {name}", cam=None if c["cam"] is None else pkg.TsdfCam(*c["cam"]))


# ---- batch behaviour ----
def _pack6(R):
    """Six source frames (two synthetic crops, four fixtures) as one pack with their grid rows, and their references."""
    cs = [ar.case("synth", 1, R), ar.case("synth", 2, R)] + [ar.case("golden", g, R) for g in
                                                            ("small_odd", "mixed_checker", "neg_all_flip", "corner_tl")]
    depth = np.concatenate([c["depth"] for c in cs])
    off = np.cumsum([0] + [c["depth"].size for c in cs]).astype(np.int64)
    hdr = np.concatenate([c["hdr"] for c in cs])
    grid = np.concatenate([c["grid"] for c in cs])
    return cs, depth, off, hdr, grid


def test_index_batch_independence_and_determinism(pkg):
    R = 12
    cs, depth, off, hdr, grid = _pack6(R)
    td, to, th, tg = up(depth, off, hdr, grid)
    for layout in LAYOUTS:
        kw = dict(res=R, layout=layout, nearest=True)
        whole, st, wn = pkg.voxelize_grid_accurate(td, to, th, tg, **kw)
        again, _, an = pkg.voxelize_grid_accurate(td, to, th, tg, **kw)
        torch.cuda.synchronize()
        assert not bool(st.any()) and torch.equal(bits(whole), bits(again)) and torch.equal(wn, an)
        for i, c in enumerate(cs):                           # the batch against the reference, frame by frame
            wv, (wnn, wf) = ar.to_layout(c["ref"]["vol"], (c["ref"]["nearest"], c["ref"]["fragile"]), layout)
            ar.compare(whole[i:i + 1].cpu().numpy(), wn[i:i + 1].cpu().numpy(), wv[None], wnn[None], wf[None], f"pack[{i}] {layout}")
        rng = np.random.default_rng(40)
        idx = np.concatenate([rng.permutation(6), rng.integers(0, 6, 34)]).astype(np.int64)      # n = 40: a permutation, repeats
        tidx, = up(idx)
        g, st, gn = pkg.voxelize_grid_accurate(td, to, th, tg, index=tidx, **kw)
        torch.cuda.synchronize()
        assert g.shape[0] == 40 and not bool(st.any())
        assert torch.equal(bits(g), bits(whole[tidx])) and torch.equal(gn, wn[tidx])
        for i in range(6):                                   # n = 1: a frame's bits are the same alone
            alone, st, aln = pkg.voxelize_grid_accurate(*up(depth[off[i]:off[i + 1]], np.array([0, off[i + 1] - off[i]], np.int64),
                                                            hdr[i:i + 1], grid[i:i + 1]), **kw)
            assert st.tolist() == [0] and torch.equal(bits(alone[0]), bits(whole[i])) and torch.equal(aln[0], wn[i]), i
    # out= a view of a larger buffer: the rest of it stays untouched; without `nearest` the result has two members
    buf = torch.full((8, 3, R, R, R), 7.0, dtype=torch.float32, device=dev())
    res = pkg.voxelize_grid_accurate(td, to, th, tg, res=R, layout="cxyz", out=buf[1:7])
    torch.cuda.synchronize()
    assert len(res) == 2 and res[0].data_ptr() == buf[1].data_ptr()
    assert torch.equal(bits(buf[1:7]), bits(whole)) and bool((buf[0] == 7.0).all()) and bool((buf[7] == 7.0).all())


def test_large_batch_takes_whole_slabs(pkg):
    # a small batch is cut into one-slice workgroups; from 1024 workgroups on a workgroup owns slab.inc's slab: at R = 20 that
    # is 6 slices, the last slab ragged (2), at R = 8 the whole frame.  A voxel's bits do not depend on the slab it is in.
    for R, n in ((20, 300), (8, 1100)):
        cs = [ar.case("synth", 1, R), ar.case("synth", 2, R)]
        depth = np.concatenate([c["depth"] for c in cs])
        off = np.cumsum([0] + [c["depth"].size for c in cs]).astype(np.int64)
        td, to, th, tg = up(depth, off, np.concatenate([c["hdr"] for c in cs]), np.concatenate([c["grid"] for c in cs]))
        idx = torch.arange(n, dtype=torch.int64, device=dev()) % 2
        for layout in LAYOUTS:
            kw = dict(res=R, layout=layout, nearest=True)
            two, st2, n2 = pkg.voxelize_grid_accurate(td, to, th, tg, **kw)          # 2 positions: one slice per workgroup
            for i, c in enumerate(cs):
                wv, (wn, wf) = ar.to_layout(c["ref"]["vol"], (c["ref"]["nearest"], c["ref"]["fragile"]), layout)
                ar.compare(two[i:i + 1].cpu().numpy(), n2[i:i + 1].cpu().numpy(), wv[None], wn[None], wf[None], f"R={R} [{i}] {layout}")
            many, st, nn = pkg.voxelize_grid_accurate(td, to, th, tg, index=idx, **kw)
            torch.cuda.synchronize()
            assert not bool(st.any()) and not bool(st2.any())
            assert torch.equal(bits(many), bits(two[idx])) and torch.equal(nn, n2[idx]), (R, layout)


# ---- bad inputs ----
def test_bad_inputs_among_good_frames(pkg):
    R = 8
    cs, depth, off, hdr, grid = _pack6(R)
    td, to, th, tg = up(depth, off, hdr, grid)
    clean, st, cn = pkg.voxelize_grid_accurate(td, to, th, tg, res=R, nearest=True)
    torch.cuda.synchronize()
    assert not bool(st.any()) and all(bool(clean[i].any()) for i in range(6))
    A, n = pkg._lib.load_accurate(), 6
    cam = pkg.default_cam()

    def raw(d, dlen, o, h, g, index=None, n_out=n):
        """The entry itself into NaN-filled buffers: every byte of every output must be written."""
        out = torch.full((n_out, 3, R, R, R), float("nan"), dtype=torch.float32, device=dev())
        nn = torch.full((n_out, R, R, R), 0x7fc00000, dtype=torch.int32, device=dev())        # a NaN's bits
        stt = torch.full((n_out,), -7, dtype=torch.int32, device=dev())
        rc = A.tsdf_voxelize_grid_accurate_hip(d.data_ptr(), dlen, o.data_ptr(), h.data_ptr(), h.shape[0],
                                               index.data_ptr() if index is not None else None, n_out, R, cam.focal, cam.cx, cam.cy,
                                               cam.invalid_eps, cam.trunc_voxels, 0, None, g.data_ptr(), out.data_ptr(),
                                               nn.data_ptr(), stt.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        return out, nn, stt

    def check(out, nn, stt, want_status, src=None):
        src = list(range(len(want_status))) if src is None else src
        assert stt.tolist() == want_status
        assert not bool(torch.isnan(out).any())
        for k, (s, g) in enumerate(zip(want_status, src)):
            if s:
                assert not bool(bits(out[k]).any()) and bool((nn[k] == -1).all()), k          # +0 everywhere, nearest -1
            else:
                assert torch.equal(bits(out[k]), bits(clean[g])) and torch.equal(nn[k], cn[g]), k

    # bad headers: an area that contradicts the payload, an empty box, a payload outside the buffer
    h2 = hdr.copy()
    h2[1, 4] += 1
    h2[3, 4] = h2[3, 2]
    check(*raw(td, td.numel(), to, up(h2)[0], tg), [0, 2, 0, 2, 0, 0])
    check(*raw(td, int(off[6]) - 5, to, th, tg), [0, 0, 0, 0, 0, 2])
    # an index outside the tables, among repeats
    idx = np.array([2, -1, 0, 6, 5, 2, 2 ** 40], np.int64)
    check(*raw(td, td.numel(), to, th, tg, index=up(idx)[0], n_out=7), [0, 2, 0, 2, 0, 0, 2], src=[2, 0, 0, 0, 5, 2, 0])
    # unusable grid rows: trunc_dis zero / negative, a NaN origin, an infinite voxel_len, a NaN trunc_dis
    g2 = grid.copy()
    g2[0, 4], g2[1, 4], g2[2, 1], g2[4, 3], g2[5, 4] = 0.0, -1.0, np.nan, np.inf, np.nan
    check(*raw(td, td.numel(), to, th, up(g2)[0]), [1, 1, 1, 0, 1, 1])
    # a bad header wins over a bad row
    check(*raw(td, td.numel(), to, up(h2)[0], up(g2)[0]), [1, 2, 1, 2, 1, 1])
    # a crop without a valid pixel (zeros, below eps, NaN): status 0, a zero volume, nothing near
    for fill in (0.0, 0.5, np.nan):
        dz = depth.copy()
        dz[off[1]:off[2]] = fill
        out, nn, stt = raw(up(dz)[0], td.numel(), to, th, tg)
        assert stt.tolist() == [0] * 6 and not bool(bits(out[1]).any()) and bool((nn[1] == -1).all())
        assert torch.equal(bits(out[0]), bits(clean[0])) and torch.equal(bits(out[2]), bits(clean[2]))
    # the wrapper's own refusals, and the empty batch
    with pytest.raises(ValueError):
        pkg.voxelize_grid_accurate(td, to, th, tg[:2], res=R)
    with pytest.raises(TypeError):
        pkg.voxelize_grid_accurate(td, to, th, tg, res=R, out=torch.empty((6, 3, R, R, R), dtype=torch.float16, device=dev()))
    with pytest.raises(ValueError):
        pkg.voxelize_grid_accurate(td, to, th, tg, res=R, out=clean[:2])
    with pytest.raises(ValueError):
        pkg.voxelize_grid_accurate(td, to, th, tg, res=10)
    e, est, en = pkg.voxelize_grid_accurate(td, to, th, tg, res=R, index=up(idx[:0])[0], nearest=True)
    assert e.shape == (0, 3, R, R, R) and est.shape == (0,) and en.shape == (0, R, R, R)


# ---- another camera ----
@pytest.mark.parametrize("which", [0, 1, 2], ids=["f300", "f588", "eps420"])
def test_non_default_camera(pkg, which):
    label, cam, depth, off, hdr, grid = ar.camera_cases()[which]
    R = 12
    hc = pkg.TsdfCam(*cam)
    td, to, th, tg = up(depth, off, hdr, grid)
    for layout in LAYOUTS:
        want, wst, wn, wf = ar.voxelize_grid_accurate_ref(depth, off, hdr, grid, R, layout, cam=cam)
        tsdf, st, nn = pkg.voxelize_grid_accurate(td, to, th, tg, res=R, layout=layout, cam=hc, nearest=True)
        torch.cuda.synchronize()
        assert st.tolist() == wst.tolist() == [0, 0]
        ar.compare(tsdf.cpu().numpy(), nn.cpu().numpy(), want, wn, wf, f"camera {label} {layout}")
    # the camera is read: the default one gives another volume
    other, _ = pkg.voxelize_grid_accurate(td, to, th, tg, res=R, layout="cxyz")
    assert not torch.equal(bits(other), bits(tsdf))


# ---- graph capture ----
def test_capture_into_a_graph_two_replays(pkg):
    d, R = dev(), 12
    cs, depth, off, hdr, grid = _pack6(R)
    changed = (depth * 1.01).astype(np.float32)
    td, to, th, tg = up(depth, off, hdr, grid)
    idx = torch.tensor([3, 1, 5, 5, 0, 2], dtype=torch.int64, device=d)
    out = torch.empty((6, 3, R, R, R), dtype=torch.float32, device=d)

    def step():
        return pkg.voxelize_grid_accurate(td, to, th, tg, res=R, index=idx, out=out, nearest=True)

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
        eager, eager_st, eager_nn = pkg.voxelize_grid_accurate(td, to, th, tg, res=R, index=idx, nearest=True)
        torch.cuda.synchronize()
        assert torch.equal(bits(have), bits(eager)) and torch.equal(have_st, eager_st) and torch.equal(have_nn, eager_nn), k
        assert torch.equal(bits(have), bits(first)) == (k == 1)   # the depth did change the volumes, and changed them back


# ---- consumers ----
def test_voxelize_accurate_equals_voxelize_but_for_the_volume(pkg, synth):
    parts = [synth.synth_batch(4, "crop", seed0=42), (np.zeros(12, np.float32), np.array([0, 12], np.int64),
                                                      np.array([[320, 240, 50, 60, 54, 63]], np.int32))]
    depth = np.concatenate([p[0] for p in parts])
    off = np.concatenate([parts[0][1], parts[0][1][-1:] + 12]).astype(np.int64)
    hdr = np.concatenate([parts[0][2], parts[1][2]])
    hdr[2, 5] += 1                                            # a bad header as well
    td, to, th = up(depth, off, hdr)
    for R, layout in ((12, "czyx"), (8, "cxyz")):
        want = pkg.voxelize(td, to, th, res=R, layout=layout)
        got = pkg.voxelize_accurate(td, to, th, res=R, layout=layout)
        ab = pkg.aabb(td, to, th, res=R)
        rows = torch.cat([ab.ori, ab.grid[:, 4:6], torch.zeros_like(ab.ori)], dim=1)
        direct, _ = pkg.voxelize_grid_accurate(td, to, th, rows, res=R, layout=layout)
        torch.cuda.synchronize()
        assert isinstance(got, pkg.TsdfBatch) and got.tsdf.dtype is torch.float32
        assert want.status.tolist() == [0, 0, 2, 0, 1]
        assert torch.equal(got.max_l, want.max_l) and torch.equal(got.mid_p, want.mid_p) and torch.equal(got.status, want.status)
        assert torch.equal(bits(got.tsdf), bits(direct))
        assert not bool(bits(got.tsdf[2]).any()) and not bool(bits(got.tsdf[4]).any())
        # every voxel the plain pass calls near stays near; voxels it rejects gain a value
        pn = ((want.tsdf != 0) & (want.tsdf.abs() < 1)).any(dim=1)
        assert bool(pn.any()) and bool((got.tsdf != 0).any(dim=1)[pn].all())
        assert int(((want.tsdf == 0).all(dim=1) & (got.tsdf != 0).any(dim=1)).sum()) > 0


def test_voxelize_frames_with_the_accurate_tsdf(pkg):
    H, W, cam, _ = lr.SETS["64x48"]
    hc = pkg.TsdfCam(*cam)
    t, = up(lr.frames_of("64x48")[:3])
    R = 8
    for placement in ("aabb", "cube"):
        for layout in LAYOUTS:
            base, c0 = pkg.voxelize_frames(t, R, placement=placement, layout=layout, cam=hc)
            proj, _ = pkg.voxelize_frames(t, R, placement=placement, layout=layout, cam=hc, tsdf="projective")
            acc, crops = pkg.voxelize_frames(t, R, placement=placement, layout=layout, cam=hc, tsdf="accurate")
            if placement == "cube":
                rows = crops.grid
            else:
                ab = pkg.aabb(crops.depth, crops.offsets, crops.headers, res=R, cam=hc)
                rows = torch.cat([ab.ori, ab.grid[:, 4:6], torch.zeros_like(ab.ori)], dim=1)
            want, _ = pkg.voxelize_grid_accurate(crops.depth, crops.offsets, crops.headers, rows, res=R, layout=layout, cam=hc)
            torch.cuda.synchronize()
            assert torch.equal(bits(acc.tsdf), bits(want)) and acc.status.tolist() == [0, 0, 0]
            for name in ("max_l", "mid_p", "status"):
                assert torch.equal(getattr(acc, name), getattr(base, name)), name
            # the default call is what it was: the same as the explicit "projective", the located pack through the old entry
            assert all(torch.equal(x, y) for x, y in zip(base, proj))
            if placement == "aabb":
                old = pkg.voxelize(c0.depth, c0.offsets, c0.headers, res=R, layout=layout, cam=hc)
            else:
                old = pkg.voxelize_grid(c0.depth, c0.offsets, c0.headers, c0.grid, res=R, layout=layout, cam=hc)
            assert torch.equal(bits(base.tsdf), bits(old[0] if placement == "cube" else old.tsdf))
            assert not torch.equal(bits(acc.tsdf), bits(base.tsdf))
    b16, crops = pkg.voxelize_frames(t, R, placement="cube", dtype=torch.bfloat16, cam=hc, tsdf="accurate")
    f32, _ = pkg.voxelize_grid_accurate(crops.depth, crops.offsets, crops.headers, crops.grid, res=R, cam=hc)
    assert b16.tsdf.dtype is torch.bfloat16 and torch.equal(b16.tsdf, f32.to(torch.bfloat16))


def test_preprocess_tree_accurate_through_the_default_hooks(pkg, synth, tmp_path):
    """export's two accurate default hooks: ``TSDF/<g>.npz`` holds the volumes of the explicit chain on the same pack (and,
    with placement="cloud", on the saved cloud) bit for bit, and nothing else moves against the projective tree."""
    db, R, g = str(tmp_path / "db"), 8, "1"
    synth.synth_msra_tree(db, n_sub=1, n_ges=1, n_frames=3, seed=8)
    sub, = os.listdir(db)
    pk = pkg.packing.pack_bin_files(pkg.packing.gesture_bin_paths(os.path.join(db, sub, g), 3))
    td, to, th = pk.to_torch(dev())
    npz = os.path.join(sub, "TSDF", g + ".npz")
    for kw in (dict(), dict(placement="cloud", point_clouds="device")):
        files = {}
        for tsdf in ("projective", "accurate"):
            out = str(tmp_path / (tsdf + "-" + kw.get("placement", "pixels")))
            pkg.export.preprocess_tree(db, out, res=R, points_num=64, rng=np.random.default_rng(3), tsdf=tsdf, device=dev(), **kw)
            files[tsdf] = {os.path.relpath(os.path.join(dp, f), out): os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs}
        fa, fp = files["accurate"], files["projective"]
        assert sorted(fa) == sorted(fp) and npz in fa
        za, zp = np.load(fa[npz]), np.load(fp[npz])
        assert (za["tsdf"] != zp["tsdf"]).any()                       # the comparison below is not of equals
        for k in fa:
            if k != npz:
                assert open(fa[k], "rb").read() == open(fp[k], "rb").read(), k
        assert sorted(za.files) == sorted(zp.files) == ["max_l", "mid_p", "status", "tsdf"]
        for f in ("max_l", "mid_p", "status"):
            assert za[f].dtype == zp[f].dtype and za[f].tobytes() == zp[f].tobytes(), f
        if kw:
            pts, = up(np.load(fa[os.path.join(sub, "Point_Cloud", g + ".npy")]))
            want, _ = pkg.voxelize_grid_accurate(td, to, th, pkg.cloud_grids(pts, res=R).grid, res=R, layout="cxyz")
        else:
            want = pkg.voxelize_accurate(td, to, th, res=R, layout="cxyz").tsdf
        assert za["tsdf"].dtype == np.float32 and za["tsdf"].shape == (3, 3, R, R, R)
        assert np.array_equal(za["tsdf"].view(np.uint32), want.cpu().numpy().view(np.uint32))
