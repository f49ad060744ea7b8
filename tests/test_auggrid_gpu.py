"""GPU tier of libtsdf_auggrid.so (include/tsdf_auggrid.h): tsdf_voxelize_aug_grid_hip on every voxel against the oracle's
augmented voxel arithmetic on the same grid (tests/auggrid_ref.py), tsdf_transform_joints_hip bit for bit against the
oracle and the fused entry, process_batch_aug stage by stage, graph capture, and
export.preprocess_tree(aug_placement="cloud") on the device."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auggrid_ref as ar  # noqa: E402
import cloud_grid_ref as cg  # noqa: E402

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

PKG = "handposeestimation-with-3d-cnns_amd"
TOL = ar.TOL
LAYOUTS = ("czyx", "cxyz")


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def up(*arrays):
    d = dev()
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(d) for a in arrays)


@pytest.fixture(scope="module")
def crops(pkg, synth):
    """The 10 crops and their maps (random_affines about the plain grid centres, rng=5), on the host and on the device."""
    import oracle

    depth, off, hdr = synth.synth_batch(10, "crop", seed0=1200)
    plain = oracle.voxelize(depth, off, hdr, R=32, want_tsdf=False)
    assert not plain["status"].any()
    xf = pkg.augment.random_affines(plain["mid_p"].astype(np.float64), rng=5)[0]
    return (depth, off, hdr, xf), up(depth, off, hdr, xf)


def cloud_grid_rows(pkg, t, R, xforms=True):
    """Grid (a): the placement of a 512-point resample of the (mapped) cloud — tighter than the hand."""
    td, to, th, txf = t
    pc = pkg.point_clouds(td, to, th, points=512, xforms=txf if xforms else None)
    g = pkg.cloud_grids(pc.points, res=R)
    torch.cuda.synchronize()
    assert not pc.status.any() and not g.status.any()
    return g


def raw_call(pkg, td, to, th, txf, tgrid, R, layout, out, st):
    """The C entry on caller-owned outputs (the wrapper allocates its own)."""
    G = pkg._lib.load_auggrid()
    rc = G.tsdf_voxelize_aug_grid_hip(td.data_ptr(), td.numel(), to.data_ptr(), th.data_ptr(), th.shape[0], R, None,
                                      pkg._lib.LAYOUTS[layout], torch.cuda.current_stream().cuda_stream, txf.data_ptr(),
                                      tgrid.data_ptr(), out.data_ptr(), st.data_ptr() if st is not None else None)
    assert rc == 0
    torch.cuda.synchronize()


# R = 8: one workgroup per frame, half its lanes idle; 12: three 4-voxel groups per row; 20: four slabs per frame, the
# last one ragged (6 + 6 + 6 + 2 slices); 32: 16 slabs of 2 slices; 64: one slice per workgroup, four items per lane
@pytest.mark.parametrize("R", [8, 12, 20, 32, 64])
def test_every_voxel_against_the_oracle_on_the_same_grid(pkg, crops, R):
    (depth, off, hdr, xf), t = crops
    g = cloud_grid_rows(pkg, t, R)
    grid_a = g.grid.cpu().numpy()
    grid_b = grid_a.copy()
    grid_b[:, 0] += np.float32(0.75) * g.max_l.cpu().numpy()        # three quarters of the voxels leave the box
    for name, grid in (("a", grid_a), ("b", grid_b)):
        tg, = up(grid)
        for layout in LAYOUTS:
            want, wst = ar.voxelize_aug_grid_ref(depth, off, hdr, xf, grid, R, layout)
            got, st = pkg.voxelize_aug_grid(*t[:3], t[3], tg, res=R, layout=layout)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            assert got.shape == (10, 3, R, R, R) and np.array_equal(st.cpu().numpy(), wst) and not wst.any()
            err = float(np.abs(got - want).max())                   # every voxel
            near, nonzero = ar.near_counts(want)
            rejected = float((want == 0).all(axis=1).mean())
            print(f"R={R} grid {name} [{layout}]: max |hip - oracle| = {err:.3g}; fewest near voxels {near.min()}, "
                  f"fewest non-zero {nonzero.min()}, rejected {rejected:.3f}")
            if name == "a":
                assert near.min() >= 100                            # not a comparison of zeros
            else:
                assert rejected > 0.7 and near.min() > 0            # whole lanes and waves rejected, the rest still live
            assert np.array_equal(got == 0, want == 0)
            assert err <= TOL


@pytest.mark.parametrize("n", [1, 300])
def test_batch_sizes(pkg, crops, n):
    """One frame, and more frames than CUs (1.8 MB of output) at R = 8; every frame against the oracle."""
    (depth, off, hdr, xf0), _ = crops
    R = 8
    pick = np.arange(n) % 10
    sizes = (off[1:] - off[:-1])[pick]
    o = np.zeros(n + 1, np.int64)
    o[1:] = np.cumsum(sizes)
    d = np.concatenate([depth[off[k]:off[k + 1]] for k in pick])
    h = hdr[pick]
    import oracle
    mid = oracle.voxelize(d, o, h, R=R, want_tsdf=False)["mid_p"]
    xf = pkg.augment.random_affines(mid.astype(np.float64), rng=6)[0]
    t = up(d, o, h, xf)
    grid = cloud_grid_rows(pkg, t, R).grid
    got, st = pkg.voxelize_aug_grid(*t, grid, res=R)
    torch.cuda.synchronize()
    want, wst = ar.voxelize_aug_grid_ref(d, o, h, xf, grid.cpu().numpy(), R, "czyx")
    assert np.array_equal(st.cpu().numpy(), wst) and not wst.any()
    near, _ = ar.near_counts(want)
    assert near.min() >= 100
    err = np.abs(got.cpu().numpy() - want).reshape(n, -1).max(axis=1)
    print(f"n={n}: worst frame {err.max():.3g}")
    assert err.max() <= TOL


@pytest.mark.parametrize("R", [32, 64])
def test_identity_map_is_voxelize_grid(pkg, crops, R):
    _, t = crops
    td, to, th, _ = t
    ident, = up(ar.identity_xforms(10))
    grid = cloud_grid_rows(pkg, t, R, xforms=False).grid
    for layout in LAYOUTS:
        a, sa = pkg.voxelize_aug_grid(td, to, th, ident, grid, res=R, layout=layout)
        b, sb = pkg.voxelize_grid(td, to, th, grid, res=R, layout=layout)
        torch.cuda.synchronize()
        assert torch.equal(sa, sb) and not sa.any() and bool((b != 0).any())
        assert torch.equal(a == 0, b == 0) and torch.equal(torch.signbit(a), torch.signbit(b))
        assert torch.equal(a[:, 2], b[:, 2])
        err = float((a[:, :2] - b[:, :2]).abs().max())
        print(f"R={R} [{layout}]: x / y differ by at most {err:.3g}")
        assert err <= TOL


def test_frames_that_are_not_ok_among_good_ones(pkg, crops):
    (depth, off, hdr, xf), t = crops
    R = 12
    n = 9                                           # frames 0..8; frame 8's payload will lie outside the buffer
    grid = cloud_grid_rows(pkg, t, R).grid.cpu().numpy()[:n]
    depth_n, off_n, hdr_n, xf_n = depth[:off[n]], off[:n + 1], hdr[:n], xf[:n]
    d = dev()
    for layout in LAYOUTS:
        clean_out = torch.full((n, 3, R, R, R), float("nan"), device=d)
        clean_st = torch.full((n,), -7, dtype=torch.int32, device=d)
        raw_call(pkg, *up(depth_n, off_n, hdr_n, xf_n, grid), R, layout, clean_out, clean_st)
        assert not clean_st.any() and not torch.isnan(clean_out).any()
        bad_hdr, bad_grid = hdr_n.copy(), grid.copy()
        bad_hdr[1, 4] = bad_hdr[1, 2] - 3           # right < left
        bad_grid[3] = 0                             # the row tsdf_cloud_grid_hip writes for a degenerate cloud
        bad_grid[5, 4] = -1                         # trunc_dis = -1
        bad_grid[6, 1] = np.inf                     # a non-finite vox_ori
        cut = depth_n[:off[8]]                      # frame 8 keeps its offsets and header, its payload is gone
        out = torch.full((n, 3, R, R, R), float("nan"), device=d)
        st = torch.full((n,), -7, dtype=torch.int32, device=d)
        raw_call(pkg, *up(cut, off_n, bad_hdr, xf_n, bad_grid), R, layout, out, st)
        assert st.cpu().tolist() == [0, 2, 0, 1, 0, 1, 1, 0, 2]
        assert not torch.isnan(out).any()                                        # every byte was written
        for i in (1, 3, 5, 6, 8):
            assert not out[i].any()
        for i in (0, 2, 4, 7):
            assert torch.equal(out[i].view(torch.int32), clean_out[i].view(torch.int32)) and bool(out[i].any())
        want, wst = ar.voxelize_aug_grid_ref(cut, off_n, bad_hdr, xf_n, bad_grid, R, layout, depth_len=cut.size)
        assert wst.tolist() == st.cpu().tolist() and np.abs(out.cpu().numpy() - want).max() <= TOL
        # NaN and -inf grid words, and a status pointer that is NULL
        worse = grid.copy()
        worse[0, 3] = np.nan
        worse[2, 4] = np.inf
        worse[4, 2] = -np.inf
        out2 = torch.full((n, 3, R, R, R), float("nan"), device=d)
        raw_call(pkg, *up(depth_n, off_n, hdr_n, xf_n, worse), R, layout, out2, None)
        for i in range(n):
            if i in (0, 2, 4):
                assert not out2[i].any()
            else:
                assert torch.equal(out2[i].view(torch.int32), clean_out[i].view(torch.int32))


@pytest.mark.parametrize("J", [1, 21, 170])
def test_transform_joints(pkg, crops, J):
    import oracle

    (depth, off, hdr, xf), t = crops
    rng = np.random.default_rng(J)
    gt = (rng.normal(0, 60, (10, J, 3)) + [0, 0, -420]).astype(np.float32)
    tg, = up(gt)
    got = pkg.transform_joints(tg, t[3])
    flat = pkg.transform_joints(tg.reshape(10, 3 * J), t[3])
    _, _, fused = pkg.voxelize_aug(*t[:3], t[3], res=8, gt=tg)
    torch.cuda.synchronize()
    assert got.shape == (10, J, 3) and flat.shape == (10, 3 * J) and torch.equal(got.reshape(10, -1), flat)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), oracle.transform_joints(gt, xf).view(np.uint32))
    assert torch.equal(got.view(torch.int32), fused.view(torch.int32))
    assert float((got - tg).abs().max()) > 1.0          # the maps move the joints
    with pytest.raises(ValueError):
        pkg.transform_joints(tg[:9], t[3])
    with pytest.raises(ValueError):
        pkg.transform_joints(tg.reshape(10, -1)[:, :3 * J - 1].contiguous(), t[3])
    with pytest.raises(TypeError):
        pkg.transform_joints(tg.double(), t[3])
    assert pkg.transform_joints(tg[:0], t[3][:0]).shape == (0, J, 3)


def test_wrapper_refuses_bad_shapes(pkg, crops):
    _, (td, to, th, txf) = crops
    grid = torch.zeros((10, 8), device=dev())
    for bad in (dict(xforms=txf[:9]), dict(xforms=txf.float()), dict(grid=grid[:, :7].contiguous()), dict(grid=grid.double()),
                dict(res=30), dict(layout="xyzc")):
        kw = dict(xforms=txf, grid=grid, res=8, layout="czyx")
        kw.update(bad)
        with pytest.raises((ValueError, TypeError)):
            pkg.voxelize_aug_grid(td, to, th, kw["xforms"], kw["grid"], res=kw["res"], layout=kw["layout"])
    out, st = pkg.voxelize_aug_grid(td[:0], to[:1], th[:0], txf[:0], grid[:0], res=8)
    assert out.shape == (0, 3, 8, 8, 8) and st.numel() == 0


@pytest.fixture(scope="module")
def batch12(synth):
    depth, off, hdr = synth.synth_batch(12, "crop", seed0=1300)
    rng = np.random.default_rng(2)
    gt = (rng.normal(0, 60, (12, 63)) + np.tile([0, 0, -420], 21)).astype(np.float32)
    return depth, off, hdr, gt


def run_aug(pkg, depth, off, hdr, gt=None, **kw):
    t = up(depth, off, hdr)
    out = pkg.process_batch_aug(*t, gt=up(gt)[0] if gt is not None else None, **kw)
    torch.cuda.synchronize()
    return out, t


def test_process_batch_aug_stage_by_stage(pkg, batch12):
    depth, off, hdr, gt = batch12
    kw = dict(points=512, seed=11, aug_seed=12, key=99, res=12)
    for layout in LAYOUTS:
        o, t = run_aug(pkg, depth, off, hdr, gt, layout=layout, **kw)
        pb = pkg.process_batch(*t, points=512, seed=11, res=12, layout=layout)
        for name in ("points", "tsdf", "max_l", "mid_p", "status", "count"):
            assert torch.equal(getattr(o, name), getattr(pb, name)), name
        assert not o.status.any() and not o.status_aug.any()
        assert torch.equal(o.xforms, pkg.aug_xforms(o.mid_p, key=99, counter0=0))
        pa = pkg.point_clouds(*t, points=512, seed=12, xforms=o.xforms)
        assert torch.equal(o.points_aug, pa.points)
        pts = o.points_aug.cpu().numpy()
        grid, max_l, mid_p, _, status = cg.cloud_grids(pts, R=12)
        assert not status.any()
        assert cg.same_values(o.max_l_aug.cpu().numpy(), max_l) and cg.same_values(o.mid_p_aug.cpu().numpy(), mid_p)
        xf = o.xforms.cpu().numpy()
        want, _ = ar.voxelize_aug_grid_ref(depth, off, hdr, xf, grid, 12, layout)
        near, _ = ar.near_counts(want)
        err = float(np.abs(o.tsdf_aug.cpu().numpy() - want).max())
        print(f"process_batch_aug [{layout}]: max |tsdf_aug - oracle| = {err:.3g}, fewest near voxels {near.min()}")
        assert near.min() >= 100 and err <= TOL
        assert torch.equal(o.gt_aug, pkg.transform_joints(t[0].new_tensor(gt), o.xforms)) and o.gt_aug.shape == (12, 63)
        assert not torch.equal(o.tsdf_aug, o.tsdf) and not torch.equal(o.max_l_aug, o.max_l)
    # caller-supplied maps, no labels
    mine = pkg.aug_xforms(o.mid_p, key=5)
    o2, _ = run_aug(pkg, depth, off, hdr, None, xforms=mine, **kw)
    assert o2.gt_aug is None and o2.xforms is mine and not torch.equal(o2.tsdf_aug, o.tsdf_aug)
    assert torch.equal(o2.tsdf, pkg.process_batch(*t, points=512, seed=11, res=12).tsdf)


def test_process_batch_aug_split_over_two_calls(pkg, batch12):
    depth, off, hdr, gt = batch12
    kw = dict(points=512, seed=3, aug_seed=4, key=1234567, res=8)
    one, _ = run_aug(pkg, depth, off, hdr, gt, frame_base=40, **kw)
    k = 5
    a, _ = run_aug(pkg, depth[:off[k]], off[:k + 1], hdr[:k], gt[:k], frame_base=40, **kw)
    b, _ = run_aug(pkg, depth[off[k]:], off[k:] - off[k], hdr[k:], gt[k:], frame_base=40 + k, **kw)
    for name in one._fields:
        both = torch.cat([getattr(a, name), getattr(b, name)])
        whole = getattr(one, name)
        assert both.dtype == whole.dtype and both.cpu().numpy().tobytes() == whole.cpu().numpy().tobytes(), name
    other, _ = run_aug(pkg, depth, off, hdr, gt, frame_base=41, **kw)
    assert not torch.equal(other.xforms, one.xforms)


def test_process_batch_aug_frame_without_valid_pixels(pkg, synth):
    good = synth.synth_frame(5, "crop")
    empty = (np.array([320, 240, 10, 10, 50, 40], np.int32), np.zeros(40 * 30, np.float32))
    bad = (np.array([320, 240, 10, 10, 5, 60], np.int32), np.full(2500, 400.0, np.float32))      # right < left
    frames = [good, empty, bad, good]
    hdr = np.stack([h for h, _ in frames])
    off = np.zeros(5, np.int64)
    off[1:] = np.cumsum([d.size for _, d in frames])
    depth = np.concatenate([d for _, d in frames])
    o, _ = run_aug(pkg, depth, off, hdr, None, points=300, res=8)
    assert o.status.cpu().tolist() == [0, 1, 2, 0] and o.status_aug.cpu().tolist() == [0, 1, 2, 0]
    assert not o.tsdf_aug[1:3].any() and not o.max_l_aug[1:3].any() and not o.points_aug[1:3].any()
    assert bool(o.tsdf_aug[0].any()) and bool(o.tsdf_aug[3].any()) and float(o.max_l_aug[0]) > 0
    # on its own the volume stage does not scan the crop: a usable grid and no valid pixel is a zero volume, status 0
    t = up(depth, off, hdr, ar.identity_xforms(4))
    grid = torch.zeros((4, 8), device=dev())
    grid[:, 2], grid[:, 3], grid[:, 4] = -450.0, 4.0, 12.0
    vol, st = pkg.voxelize_aug_grid(*t, grid, res=8)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0, 0, 2, 0] and not vol[1].any()


def test_capture_into_a_graph_and_replay(pkg, crops):
    _, t = crops
    R = 32
    grid = cloud_grid_rows(pkg, t, R).grid
    eager, est = pkg.voxelize_aug_grid(*t, grid, res=R)      # (also loads the code object outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, st = pkg.voxelize_aug_grid(*t, grid, res=R)
    for _ in range(2):
        out.fill_(float("nan"))
        st.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32)) and torch.equal(st, est)
    assert bool(eager.any()) and not torch.isnan(eager).any()


def test_preprocess_tree_aug_placement_cloud_on_the_device(pkg, synth, tmp_path):
    export = importlib.import_module(PKG + ".export")
    db = str(tmp_path / "db")
    synth.synth_msra_tree(db, n_sub=1, n_ges=2, n_frames=3, seed=6)
    outs = {}
    for mode in ("cloud", "pixels"):
        outs[mode] = str(tmp_path / mode)
        export.preprocess_tree(db, outs[mode], points_num=500, point_clouds="device", placement="cloud", aug=True,
                               aug_placement=mode, rng=np.random.default_rng(1), aug_rng=np.random.default_rng(2),
                               device=dev())
    for g in ("1", "2"):
        pk = pkg.packing.pack_bin_files(pkg.packing.gesture_bin_paths(os.path.join(db, "P0", g), 3))
        sub = os.path.join(outs["cloud"], "P0")
        pc = np.load(os.path.join(sub, "Point_Cloud_aug", g + ".npy"))
        z = np.load(os.path.join(sub, "TSDF_aug", g + ".npz"))
        grid, max_l, mid_p, _, status = cg.cloud_grids(pc)
        assert pc.shape == (3, 500, 3) and not status.any()
        assert np.array_equal(z["max_l"], max_l) and np.array_equal(z["mid_p"], mid_p) and np.array_equal(z["status"], status)
        want, _ = ar.voxelize_aug_grid_ref(pk.depth, pk.offsets, pk.headers, z["xform"], grid, 32, "cxyz")
        near, _ = ar.near_counts(want)
        err = float(np.abs(z["tsdf"] - want).max())
        print(f"gesture {g}: max |TSDF_aug - oracle| = {err:.3g}, fewest near voxels {near.min()}")
        assert near.min() >= 100 and err <= TOL
        zp = np.load(os.path.join(outs["pixels"], "P0", "TSDF_aug", g + ".npz"))
        assert np.array_equal(z["xform"], zp["xform"]) and not np.array_equal(z["max_l"], zp["max_l"])
        for d in ("ground_truth_aug", "Point_Cloud_aug", "Point_Cloud", "ground_truth"):
            a, b = (np.load(os.path.join(outs[m], "P0", d, g + ".npy")) for m in ("cloud", "pixels"))
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), d
