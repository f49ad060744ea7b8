"""CPU tier: the grid placed on the resampled cloud (DataProcess.process()'s rule).  The numpy restatement of
tsdf_cloud_grid_hip (tests/cloud_grid_ref.py) against what the reference's tsdf_f returned for the clouds of
tests/golden/process_ref_<k>.npz, the oracle's loop on those grids, the not-OK rules, the C entry's argument checks and
export.preprocess_tree(placement="cloud") through its hooks.  Nothing here touches a GPU."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_grid_ref as cg  # noqa: E402
from cloud_grid_ref import frames_and_clouds, recorded  # noqa: E402

PKG = "handposeestimation-with-3d-cnns_amd"


@pytest.fixture(scope="module")
def mg():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return importlib.import_module("make_goldens")     # its frame list and cloud rule; not the reference
    finally:
        sys.path.pop(0)


def check_grid_against_record(name, got, g):
    grid, max_l, mid_p, aabb, status = (x[0] for x in got)
    assert status == 0, name
    assert cg.same_values(aabb[:3], g["point_min"]) and cg.same_values(aabb[3:], g["point_max"]), name
    assert cg.same_values(max_l, g["max_l"]) and cg.same_values(mid_p, g["mid_p"]), name
    assert cg.same_values(grid[:3], g["vox_ori"]) and cg.same_values(grid[3], g["voxel_len"]), name
    assert cg.same_values(grid[4], g["trunc"]) and not grid[5:].any(), name


def test_restatement_equals_the_reference_on_every_fixture(mg, golden_dir):
    names = []
    for name, _, _, cloud, g in frames_and_clouds(mg, golden_dir):
        check_grid_against_record(name, cg.cloud_grids(cloud[None]), g)
        names.append(name)
    vol = [n for n in names if "@" not in n]
    assert vol == [n for n, _, _ in mg.volume_frames()] and len(vol) == 22
    assert {n.split("@P")[1] for n in names if "@" in n} == {"500", "20000"}


def test_cloud_placement_differs_from_pixel_placement(mg, golden_dir):
    """full_0 has more than 6000 valid pixels: the grid of the resampled cloud is not the grid of all pixels."""
    g = dict(recorded(golden_dir))["full_0"]
    pix = np.load(os.path.join(golden_dir, "full_0.npz"))
    assert abs(float(g["max_l"]) - 289.10) < 0.01 and abs(float(pix["max_l"]) - 292.41) < 0.01


def test_oracle_loop_on_the_cloud_grid_equals_loop64_on_every_voxel(mg, golden_dir):
    import oracle

    n = flips = 0
    for name, h, d, _, g in frames_and_clouds(mg, golden_dir):
        if "loop64" not in g:
            continue
        out = oracle.voxels(d, h, g["vox_ori"], g["voxel_len"], g["trunc"], R=32, layout=0)
        np.testing.assert_array_equal(out, g["loop64"], err_msg=name)           # no voxel left out
        loop32 = g["loop64"].copy()
        loop32.reshape(-1)[g["loop32_diff_index"]] = g["loop32_diff_value"]
        assert int((np.abs(out - loop32) > 1e-5).any(axis=0).sum()) == int(g["n_flip"]), name
        flips += int(g["n_flip"])
        n += 1
    assert n == 22 and flips == 25


def one(points, **kw):
    grid, max_l, mid_p, aabb, status = cg.cloud_grids(np.asarray(points, np.float64)[None], **kw)
    return grid[0], max_l[0], mid_p[0], aabb[0], int(status[0])


def test_z_rule_and_glue_on_hand_made_clouds():
    pts = [[1.0, 2.0, 0.0], [-3.0, 5.0, -400.0], [7.0, -1.0, -0.0], [0.5, 0.5, -380.0], [9.0, 9.0, 5e-324]]
    grid, max_l, mid_p, aabb, st = one(pts)
    assert st == 0
    assert list(aabb[:2]) == [-3.0, -1.0] and list(aabb[3:5]) == [9.0, 9.0]      # x, y over all five points
    assert aabb[2] == -400.0 and aabb[5] == 0.0                                   # 0 and -0 dropped, the denormal kept
    assert max_l == 400.0 and list(mid_p) == [3.0, 4.0, -200.0]
    assert grid[3] == np.float32(400.0) / np.float32(32) and grid[4] == grid[3] * np.float32(3)
    assert list(grid[:3]) == [np.float32(m) - np.float32(200) + grid[3] / np.float32(2) for m in mid_p]
    # resolution and truncation are parameters
    g64 = one(pts, R=64, trunc_voxels=2.0)[0]
    assert g64[3] == np.float32(400.0) / np.float32(64) and g64[4] == g64[3] * np.float32(2)
    # float64 values round to float32 once, extremes of the rounded values
    p = np.array([[0.1, 0.2, -300.3], [1e-9, 1 + 1e-12, -300.3 - 1e-9]])
    _, _, _, ab, _ = one(p)
    assert cg.same_values(ab, np.float32([1e-9, 0.2, -300.3 - 1e-9, 0.1, 1 + 1e-12, -300.3]))


def test_not_ok_clouds():
    zero = np.zeros(8, np.float32)
    # all-zero cloud (what point_clouds writes for a frame that is not OK), and x / y present but no z != 0
    for pts in (np.zeros((10, 3)), [[1.0, 2.0, 0.0], [3.0, 4.0, -0.0]]):
        grid, max_l, mid_p, aabb, st = one(pts)
        assert st == 1 and max_l == 0 and not grid.any() and not mid_p.any() and not aabb.any()
    # one point: zero extent, the centre is kept
    grid, max_l, mid_p, aabb, st = one([[1.0, 2.0, -3.0]])
    assert st == 1 and max_l == 0 and np.array_equal(grid, zero) and list(mid_p) == [1.0, 2.0, -3.0]
    assert list(aabb) == [1.0, 2.0, -3.0, 1.0, 2.0, -3.0]
    # NaN in any value that enters an extreme: x, y of every point (also of one whose z is dropped), z unless it is 0
    base = np.array([[1.0, 2.0, -300.0], [4.0, 6.0, -350.0], [2.0, 3.0, 0.0]])
    assert one(base)[4] == 0
    for r, c in ((0, 0), (1, 1), (1, 2), (2, 0), (2, 1)):
        p = base.copy()
        p[r, c] = np.nan
        grid, max_l, mid_p, aabb, st = one(p)
        assert st == 1 and max_l == 0 and not grid.any() and not mid_p.any() and not aabb.any(), (r, c)
    # infinite coordinates: non-finite extent (and centre)
    for v in (np.inf, -np.inf, 1e39):
        p = base.copy()
        p[0, 1] = v
        grid, max_l, mid_p, _, st = one(p)
        assert st == 1 and max_l == 0 and not grid.any() and not mid_p.any()
    p = base.copy()
    p[0, 0], p[1, 0] = np.inf, -np.inf
    assert one(p)[4] == 1
    # a finite centre with an overflowing extent: mid_p is kept
    p = np.array([[3e38, 0.0, -1.0], [-3e38, 1.0, -2.0]])
    grid, max_l, mid_p, _, st = one(p)
    assert st == 1 and max_l == 0 and not grid.any() and list(mid_p) == [0.0, 0.5, -1.5]


def test_restatement_is_max_min_point_of_the_drop_in(pkg):
    """tsdf_for.max_min_point / tsdf_f's glue of the package (the host path DataProcess.process() keeps) give the same
    values on ordinary clouds."""
    tf = importlib.import_module(PKG + ".tsdf_for")
    rng = np.random.default_rng(5)
    for P in (1, 2, 65, 6000):
        pts = rng.normal(0, 80, (P + 1, 3)) + [0, 0, -400]
        pts[rng.integers(0, P + 1, 3), 2] = 0.0
        pts[0, 2] = -400.0
        pmax, pmin = tf.max_min_point(pts)
        _, _, _, aabb, _ = one(pts)
        assert np.array_equal(aabb[:3], pmin) and np.array_equal(aabb[3:], pmax)


def test_symbol_exported_and_arguments_checked(pkg):
    L = pkg._lib.load()
    assert hasattr(L, "tsdf_cloud_grid_hip") and pkg.cloud_grids and pkg.CloudGridBatch
    assert pkg.process_batch and pkg.ProcessBatch
    null, one_, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(20)
    f = L.tsdf_cloud_grid_hip
    assert f(null, 0, 6000, 32, None, null, null, null, null, null, null) == 0          # n == 0: a no-op
    assert f(null, 1, 6000, 32, None, null, one_, one_, one_, null, null) == -1         # NULL d_points
    assert f(one_, 1, 6000, 32, None, null, null, one_, one_, null, null) == -1         # NULL grid
    assert f(one_, 1, 6000, 32, None, null, one_, null, one_, null, null) == -1         # NULL max_l
    assert f(one_, 1, 6000, 32, None, null, one_, one_, null, null, null) == -1         # NULL mid_p
    assert f(one_, -1, 6000, 32, None, null, one_, one_, one_, null, null) == -1        # n < 0
    assert f(one_, 1, 0, 32, None, null, one_, one_, one_, null, null) == -1            # points < 1
    assert f(one_, 1, 6000, 30, None, null, one_, one_, one_, null, null) == -1         # unsupported R
    assert f(odd, 1, 6000, 32, None, null, one_, one_, one_, null, null) == -1          # d_points not 8-byte aligned
    assert L.tsdf_version() == 7


def _hooks():
    import oracle

    def vox(pk, res, layout, device):
        r = oracle.voxelize(pk.depth, pk.offsets, pk.headers, R=res, layout=0 if layout == "czyx" else 1)
        return r["tsdf"], r["max_l"], r["mid_p"], r["status"]

    def vox_aug(pk, xf, gt, res, layout, device):
        r = oracle.voxelize_aug(pk.depth, pk.offsets, pk.headers, xf, R=res, layout=0 if layout == "czyx" else 1)
        return r["tsdf"], r["max_l"], r["mid_p"], r["status"], oracle.transform_joints(gt, xf)

    calls = []

    def vox_cloud(pk, cloud, res, layout, device):
        calls.append(np.array(cloud))
        grid, max_l, mid_p, _, status = cg.cloud_grids(cloud, R=res)
        tsdf = np.zeros((len(pk), 3, res, res, res), np.float32)
        for i in range(len(pk)):
            if status[i] == 0:
                h, d = pk.frame(i)
                tsdf[i] = oracle.voxels(d, h, grid[i, :3], grid[i, 3], grid[i, 4], R=res,
                                        layout=0 if layout == "czyx" else 1)
        return tsdf, max_l, mid_p, status
    return vox, vox_aug, vox_cloud, calls


def _files(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            out[os.path.relpath(os.path.join(dp, f), root)] = open(os.path.join(dp, f), "rb").read()
    return out


def _same_file(name, a, b, tmp):
    """npy files byte for byte; npz archives (their members carry time stamps) array for array."""
    if not name.endswith(".npz"):
        return a == b
    pa, pb = os.path.join(tmp, "a.npz"), os.path.join(tmp, "b.npz")
    open(pa, "wb").write(a)
    open(pb, "wb").write(b)
    za, zb = np.load(pa), np.load(pb)
    return sorted(za.files) == sorted(zb.files) and all(
        za[k].dtype == zb[k].dtype and za[k].tobytes() == zb[k].tobytes() for k in za.files)


def test_preprocess_tree_placement_cloud_through_the_hooks(pkg, synth, tmp_path):
    export = importlib.import_module(PKG + ".export")
    pca = importlib.import_module(PKG + ".pca")
    db = str(tmp_path / "db")
    synth.synth_msra_tree(db, n_sub=2, n_ges=2, n_frames=3, seed=4)
    vox, vox_aug, vox_cloud, calls = _hooks()
    kw = dict(res=8, points_num=200, voxelize_fn=vox, voxelize_aug_fn=vox_aug, voxelize_cloud_fn=vox_cloud)
    today, pixels, cloud = str(tmp_path / "today"), str(tmp_path / "pixels"), str(tmp_path / "cloud")
    pdir = str(tmp_path / "pca")
    export.preprocess_tree(db, today, rng=np.random.default_rng(7), aug=True, aug_rng=np.random.default_rng(8), res=8,
                           points_num=200, voxelize_fn=vox, voxelize_aug_fn=vox_aug)          # the call as it was
    export.preprocess_tree(db, pixels, rng=np.random.default_rng(7), aug=True, aug_rng=np.random.default_rng(8),
                           placement="pixels", **kw)
    assert not calls                                                       # the cloud hook is for placement="cloud" only
    export.preprocess_tree(db, cloud, rng=np.random.default_rng(7), aug=True, aug_rng=np.random.default_rng(8),
                           placement="cloud", pca_dir=pdir, **kw)
    assert len(calls) == 4
    ft, fp, fc = _files(today), _files(pixels), _files(cloud)
    scratch = str(tmp_path)
    assert sorted(ft) == sorted(fp) == sorted(fc)
    assert all(_same_file(k, ft[k], fp[k], scratch) for k in ft)          # placement="pixels" is today's output
    # the draws and their order did not move: clouds, labels and counts of the cloud run are those of the pixels run
    for k in fc:
        if k.startswith("data_num") or k.split(os.sep)[1] in ("Point_Cloud", "ground_truth", "num", "num_aug"):
            assert fc[k] == fp[k], k
    arng = np.random.default_rng(8)
    labels, differ = {}, 0
    for s in ("P0", "P1"):
        for g in ("1", "2"):
            pc = np.load(os.path.join(cloud, s, "Point_Cloud", g + ".npy"))
            z = np.load(os.path.join(cloud, s, "TSDF", g + ".npz"))
            zp = np.load(os.path.join(pixels, s, "TSDF", g + ".npz"))
            assert pc.shape == (3, 200, 3) and pc.dtype == np.float64
            grid, max_l, mid_p, _, status = cg.cloud_grids(pc, R=8)
            # the saved max_l / mid_p are a function of the saved cloud, frame by frame
            assert np.array_equal(z["max_l"], max_l) and np.array_equal(z["mid_p"], mid_p)
            assert np.array_equal(z["status"], status) and z["tsdf"].shape == zp["tsdf"].shape
            assert z["tsdf"].dtype == np.float32 and z["tsdf"].any()
            differ += int((z["max_l"] != zp["max_l"]).sum())
            # the augmented twins: maps centred on the mid_p that was written, all-pixels placement under the map
            za = np.load(os.path.join(cloud, s, "TSDF_aug", g + ".npz"))
            xf = pkg.augment.random_affines(z["mid_p"].astype(np.float64), rng=arng)[0]
            gdir = os.path.join(db, s, g)
            pk = pkg.packing.pack_bin_files(pkg.packing.gesture_bin_paths(gdir, 3))
            pca_ = export.resample_point_clouds(pk, 200, arng, xforms=xf)      # (the augmented cloud's draws come next)
            assert np.array_equal(pca_, np.load(os.path.join(cloud, s, "Point_Cloud_aug", g + ".npy")))
            assert np.array_equal(za["xform"], xf)
            gt = np.load(os.path.join(cloud, s, "ground_truth", g + ".npy"))
            labels.setdefault(s, []).append(pca.normalize_labels_np(gt, z["max_l"], z["mid_p"])[z["status"] == 0])
    assert differ > 0                                                      # frames with more than 200 valid pixels
    # pca_dir uses the max_l / mid_p that were written
    for t, s in enumerate(("P0", "P1")):
        other = "P1" if s == "P0" else "P0"
        want = pca.fit_labels(np.concatenate(labels[other]), fold=t)
        got = pca.JointPCA.load(os.path.join(pdir, "%d.npz" % t))
        assert np.array_equal(got.mean, want.mean) and np.array_equal(got.coeff, want.coeff)


def test_preprocess_tree_placement_arguments(pkg, synth, tmp_path):
    export = importlib.import_module(PKG + ".export")
    db = str(tmp_path / "db")
    synth.synth_msra_tree(db, n_sub=1, n_ges=1, n_frames=2, seed=1)
    vox, _, vox_cloud, _ = _hooks()
    for pc in (False, None):
        with pytest.raises(ValueError):
            export.preprocess_tree(db, str(tmp_path / "x"), res=4, point_clouds=pc, placement="cloud", voxelize_fn=vox,
                                   voxelize_cloud_fn=vox_cloud)
    with pytest.raises(ValueError):
        export.preprocess_tree(db, str(tmp_path / "y"), res=4, placement="points", voxelize_fn=vox)
    assert "placement=\"cloud\"" in export.__doc__ and "all deliberate and switchable" not in export.__doc__


def test_live_reference_max_min_point_and_glue(mg, golden_dir):
    """The reference's own tsdf_f, run here when the reference is present: its max_min_point and glue against the
    restatement on the fixtures' clouds and on seeded clouds with zeros in z (the loop itself is not run)."""
    if not os.path.isfile(os.path.join(mg.REF_PRE, "tsdf_for.py")):
        pytest.skip("the reference checkout is not on this machine")
    rng = np.random.default_rng(99)
    clouds = [(name, h, d, cloud) for name, h, d, cloud, _ in frames_and_clouds(mg, golden_dir)]
    for P in (1, 2, 63, 64, 65, 511, 6001):
        pts = rng.normal(0, 90, (P + 1, 3)) + [0, 0, -420]
        pts[rng.integers(0, P + 1, max(1, P // 7)), 2] = rng.choice([0.0, -0.0])
        pts[-1, 2] = -333.0
        h, d = clouds[0][1], clouds[0][2]
        clouds.append(("random_P%d" % (P + 1), h, d, pts))
    for name, h, d, cloud in clouds:
        g = mg.run_reference_process(h, d, cloud, volumes=False)
        check_grid_against_record(name, cg.cloud_grids(cloud[None]), g)
