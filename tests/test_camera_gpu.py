"""GPU tier of the camera tests: every entry that takes a tsdf_cam under five cameras that are not the MSRA one, against
the references given the same constants, and every Python composite against the chain of its parts.

The cameras and the two batches are tests/camera_ref.py's: the four of test_custom_camera_constants and CAM_EPS, whose
invalid_eps = 420.5 mm lies inside batch B's depths (410..450 mm) so that about half of every frame's pixels are invalid
under it, and makes 7 of batch A's crops degenerate.  tests/test_camera_cpu.py asserts those conditions, and the
restatement's own input conditions for the principal axes, on the references.

No tolerance is new: volumes against the oracle <= 1e-5 (tests/test_parity_gpu.py), placement bit for bit, 2-byte volumes
inside in_band(g, o, TOL) of tests/test_maplowp_gpu.py, the principal-axis maps by check_frame of tests/test_obb_gpu.py,
the joint PCA by pca_ref.bound64, point clouds bit for bit.

The guard against a test that cannot see a dropped ``cam=``: wherever a camera differs from the default in a field the
entry reads (for invalid_eps: wherever it changes the batch's valid pixels), the reference under that camera is asserted to
differ from the reference under the default camera.  Where it does not differ in any such field (point_clouds reads focal
alone, and CAM_EPS has the default focal) the two references are the same by the contract, and the test then pins exactly
that: the other fields are not read."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auggrid_ref as ar  # noqa: E402
import camera_ref as cr  # noqa: E402
import cloud_grid_ref as cg  # noqa: E402
import obb_ref as ob  # noqa: E402
import pca_ref  # noqa: E402
import point_cloud_ref as pcr  # noqa: E402
from test_maplowp_gpu import in_band  # noqa: E402
from test_obb_gpu import check_frame  # noqa: E402

pytestmark = pytest.mark.gpu

PKG = cr.PKG
TOL = 1e-5                       # volumes against the oracle (tests/test_parity_gpu.py; ar.TOL is the same figure)
LAY = {"czyx": 0, "cxyz": 1}
DTYPES = (torch.float16, torch.bfloat16)
FOCAL, CX, CY, EPS, TRUNC = range(5)
cams = pytest.mark.parametrize("cam", cr.CAMS, ids=cr.CAM_IDS)
two_cams = pytest.mark.parametrize("cam", [cr.CAM_EPS, cr.FRACTIONAL], ids=["eps420", "f300"])
BATCHES = {"A": cr.batch_a, "B": cr.batch_b}


def dev():
    return torch.device("cuda")


def up(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev()) for a in arrays)


def bits(a):
    """The bit patterns of an array or tensor: equality of these is bit-exactness (-0 is not +0, a NaN matches itself)."""
    if hasattr(a, "detach"):
        a = a.detach().contiguous()
        if a.dtype in (torch.float16, torch.bfloat16):
            a = a.view(torch.int16)
        a = a.cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    x, y = bits(a), bits(b)
    return x.shape == y.shape and np.array_equal(x, y)


def hip_cam(pkg, cam):
    return pkg.TsdfCam(*cam)


def reads_differently(cam, name, fields):
    """The camera differs from the default in something an entry that reads ``fields`` can see on batch ``name``."""
    if any(cam[k] != cr.DEFAULT[k] for k in fields if k != EPS):
        return True
    if EPS in fields:
        depth, off, _ = BATCHES[name]()
        return not np.array_equal(cr.valid_counts(depth, off, cam[EPS]), cr.valid_counts(depth, off, 1.0))
    return False


def guard(cam, name, fields, under_cam, under_default):
    """The reference can see the camera: it differs from the default camera's wherever the entry reads a difference
    (and is the same where it reads none: then the contract says the result does not depend on the other fields)."""
    a = np.concatenate([bits(x).astype(np.uint64).reshape(-1) for x in under_cam])
    b = np.concatenate([bits(x).astype(np.uint64).reshape(-1) for x in under_default])
    assert np.array_equal(a, b) != reads_differently(cam, name, fields), (cam, name)


# ---- references, computed once per (batch, camera, resolution, layout) and never modified -----------------------------
@functools.lru_cache(maxsize=16)
def plain_ref(name, cam, R, layout="czyx", want_tsdf=True):
    depth, off, hdr = BATCHES[name]()
    return oracle.voxelize(depth, off, hdr, R=R, layout=LAY[layout], n_threads=8, want_tsdf=want_tsdf, extras=True, cam=cam)


def rows_of(ref):
    """The float32[n,8] grid rows (vox_ori[3], voxel_len, trunc_dis, 0, 0, 0) of an oracle placement."""
    n = len(ref["ori"])
    return np.concatenate([ref["ori"], ref["grid"][:, 4:6], np.zeros((n, 3), np.float32)], axis=1)


@functools.lru_cache(maxsize=None)
def joints(name):
    """float32[n,63] joints about every frame's default-camera grid centre (the same for every camera)."""
    ref = plain_ref(name, None, 32, want_tsdf=False)
    n = len(ref["status"])
    return (ref["mid_p"][:, None, :] + np.random.default_rng(7).normal(0, 40, (n, 21, 3))).astype(np.float32).reshape(n, 63)


@functools.lru_cache(maxsize=None)
def ok_frames(name, cam):
    """The frames of a batch that are OK under a camera, with their maps (random_affines about the camera's own grid
    centres): the mapped entries' inputs.  All of B under every camera; all of A but the crops CAM_EPS empties."""
    depth, off, hdr = BATCHES[name]()
    ref = plain_ref(name, cam, 32, want_tsdf=False)
    keep = [i for i in range(len(hdr)) if ref["status"][i] == 0]
    assert len(keep) >= 17
    aug = importlib.import_module(PKG + ".augment")
    xf = aug.random_affines(ref["mid_p"][keep].astype(np.float64), rng=11)[0]
    return cr.take(depth, off, hdr, keep) + (xf, joints(name)[keep])


@functools.lru_cache(maxsize=None)
def mapped_ref(name, cam, R):
    depth, off, hdr, xf, _ = ok_frames(name, cam)
    return ar.pixel_grids(depth, off, hdr, xf, R, cam)


@functools.lru_cache(maxsize=None)
def mapped_volume(name, cam, R, layout):
    depth, off, hdr, xf, _ = ok_frames(name, cam)
    vol, st = ar.voxelize_aug_grid_ref(depth, off, hdr, xf, mapped_ref(name, cam, R)[0], R, layout, cam)
    assert not st.any()
    return vol


def check_placement(got, ref):
    assert np.array_equal(got.status.cpu().numpy(), ref["status"])
    assert same(got.max_l, ref["max_l"]) and same(got.mid_p, ref["mid_p"])


def check_volume(got_tsdf, ref_tsdf):
    g = got_tsdf.float().cpu().numpy()
    err = float(np.abs(g - ref_tsdf).max())
    print(f"max |hip - oracle| = {err:.3g}")
    assert np.isfinite(g).all() and err <= TOL


# ---- the main library ----------------------------------------------------------------------------------------------------
@cams
@pytest.mark.parametrize("name", ["A", "B"])
def test_aabb(pkg, cam, name):
    t = up(*BATCHES[name]())
    for R in (32, 16):
        ref = plain_ref(name, cam, R, want_tsdf=False)
        r = pkg.aabb(*t, res=R, cam=hip_cam(pkg, cam))
        torch.cuda.synchronize()
        assert np.array_equal(r.status.cpu().numpy(), ref["status"])
        assert same(r.grid, ref["grid"]) and same(r.ori, ref["ori"])       # mid_p[3], max_l, voxel_len, trunc_dis; vox_ori
        ok = ref["status"] == 0
        assert ok.sum() >= 17 and same(r.aabb.cpu().numpy()[ok], ref["aabb"][ok])
        base = plain_ref(name, None, R, want_tsdf=False)
        guard(cam, name, (FOCAL, CX, CY, EPS, TRUNC), (ref["grid"], ref["status"]), (base["grid"], base["status"]))


@cams
@pytest.mark.parametrize("name", ["A", "B"])
def test_voxelize_grid_and_its_two_byte_twin(pkg, cam, name):
    """voxelize_grid and voxelize_grid_lowp on the oracle's rows against oracle.voxels(cam=) on those rows (the volume of
    oracle.voxelize: the same function on the same rows); a frame that is not OK has a zero row and a zero volume."""
    t = up(*BATCHES[name]())
    hc = hip_cam(pkg, cam)
    for R, layout in ((32, "czyx"), (32, "cxyz"), (16, "cxyz"), (16, "czyx")):
        ref = plain_ref(name, cam, R, layout)
        rows, = up(rows_of(ref))
        vol, st = pkg.voxelize_grid(*t, rows, res=R, layout=layout, cam=hc)
        torch.cuda.synchronize()
        assert np.array_equal(st.cpu().numpy(), ref["status"])
        check_volume(vol, ref["tsdf"])
        o, = up(ref["tsdf"])
        for dtype in DTYPES:
            low, st2 = pkg.voxelize_grid_lowp(*t, rows, res=R, layout=layout, dtype=dtype, cam=hc)
            torch.cuda.synchronize()
            assert torch.equal(st2, st) and low.dtype is dtype
            assert in_band(low, o, TOL)
        # the volume on the SAME rows under the default camera is another one: the voxel pass reads focal, cx, cy, eps
        if R == 32 and layout == "czyx":
            depth, off, hdr = BATCHES[name]()
            base = oracle.voxelize(depth, off, hdr, R=R, layout=LAY[layout], n_threads=8)
            i = int(np.flatnonzero(ref["status"] == 0)[0])
            on_rows = oracle.voxels(depth[off[i]:off[i + 1]], hdr[i], ref["ori"][i], ref["grid"][i, 4], ref["grid"][i, 5], R, 0)
            assert np.array_equal(on_rows, ref["tsdf"][i]) != reads_differently(cam, name, (FOCAL, CX, CY, EPS))
            guard(cam, name, (FOCAL, CX, CY, EPS, TRUNC), (ref["tsdf"],), (base["tsdf"],))


@cams
@pytest.mark.parametrize("name", ["A", "B"])
def test_voxelize_labels(pkg, cam, name):
    t = up(*BATCHES[name]())
    gt = joints(name)
    tg, = up(gt)
    for R, layout in ((32, "cxyz"), (16, "czyx")):
        ref = plain_ref(name, cam, R, layout)
        out, nor = pkg.voxelize_labels(*t, tg, res=R, layout=layout, cam=hip_cam(pkg, cam))
        torch.cuda.synchronize()
        check_placement(out, ref)
        check_volume(out.tsdf, ref["tsdf"])
        ok = ref["status"] == 0
        want = oracle.normalize_joints(gt[ok], ref["max_l"][ok], ref["mid_p"][ok])
        assert same(nor.cpu().numpy()[ok], want)
        assert (nor.cpu().numpy()[~ok] == 0.5).all()
        base = plain_ref(name, None, R, want_tsdf=False)
        okb = ok & (base["status"] == 0)
        guard(cam, name, (FOCAL, CX, CY, EPS), (oracle.normalize_joints(gt[okb], ref["max_l"][okb], ref["mid_p"][okb]),),
              (oracle.normalize_joints(gt[okb], base["max_l"][okb], base["mid_p"][okb]),))


def _index(n, rng):
    """27 frame numbers, shuffled, with repeats."""
    return np.concatenate([rng.integers(0, n, 5), rng.permutation(n)]).astype(np.int64)[:27]


@cams
def test_voxelize_indexed(pkg, cam):
    """A shuffled index with repeats, with and without maps, with and without labels: the oracle on the gathered batch."""
    hc = hip_cam(pkg, cam)
    aug = importlib.import_module(PKG + ".augment")
    for name, R, layout in (("B", 32, "czyx"), ("A", 16, "cxyz")):
        depth, off, hdr = BATCHES[name]()
        gt = joints(name)
        idx = _index(len(hdr), np.random.default_rng(5))
        sub = cr.take(depth, off, hdr, idx)
        td, to, th, tg, ti = up(depth, off, hdr, gt, idx)
        ref = oracle.voxelize(*sub, R=R, layout=LAY[layout], n_threads=8, cam=cam)
        ok = ref["status"] == 0
        bare = pkg.voxelize_indexed(td, to, th, ti, res=R, layout=layout, cam=hc)
        out, nor, gsel = pkg.voxelize_indexed(td, to, th, ti, tg, res=R, layout=layout, cam=hc, gt_copy=True)
        torch.cuda.synchronize()
        for got in (bare, out):
            check_placement(got, ref)
            check_volume(got.tsdf, ref["tsdf"])
        assert same(gsel, gt[idx])
        # the index in ordinary host memory travels inside the kernel arguments (tsdf_voxelize_indexed_host_hip)
        byv, nor_v = pkg.voxelize_indexed(td, to, th, torch.from_numpy(idx), tg, res=R, layout=layout, cam=hc)
        torch.cuda.synchronize()
        assert len(idx) <= pkg._lib.INLINE_INDEX_MAX and same(nor_v, nor)
        for a, b in zip(byv, out):
            assert same(a, b)
        assert same(nor.cpu().numpy()[ok], oracle.normalize_joints(gt[idx][ok], ref["max_l"][ok], ref["mid_p"][ok]))
        # with maps, about the camera's own grid centres
        xf = aug.random_affines(ref["mid_p"].astype(np.float64), rng=4)[0]
        tx, = up(xf)
        refa = oracle.voxelize_aug(*sub, xf, R=R, layout=LAY[layout], n_threads=8, cam=cam)
        assert np.array_equal(refa["status"], ref["status"])
        barea = pkg.voxelize_indexed(td, to, th, ti, res=R, layout=layout, cam=hc, xforms=tx)
        outa, nora, gaug = pkg.voxelize_indexed(td, to, th, ti, tg, res=R, layout=layout, cam=hc, xforms=tx, gt_copy=True)
        torch.cuda.synchronize()
        for got in (barea, outa):
            check_placement(got, refa)
            check_volume(got.tsdf, refa["tsdf"])
        want_aug = oracle.transform_joints(gt[idx], xf)
        assert same(gaug, want_aug)
        assert same(nora.cpu().numpy()[ok], oracle.normalize_joints(want_aug[ok], refa["max_l"][ok], refa["mid_p"][ok]))
        based = oracle.voxelize(*sub, R=R, layout=LAY[layout], n_threads=8)
        basea = oracle.voxelize_aug(*sub, xf, R=R, layout=LAY[layout], n_threads=8)
        guard(cam, name, (FOCAL, CX, CY, EPS, TRUNC), (ref["tsdf"], ref["max_l"]), (based["tsdf"], based["max_l"]))
        guard(cam, name, (FOCAL, CX, CY, EPS, TRUNC), (refa["tsdf"], refa["max_l"]), (basea["tsdf"], basea["max_l"]))


@cams
def test_joint_pca_through_the_indexed_entry(pkg, cam):
    """voxelize_indexed(pca=) and project_joints under a camera: the restatement bit for bit, and the order-free float64
    reference within pca_ref.bound64."""
    P = importlib.import_module(PKG + ".pca")
    hc = hip_cam(pkg, cam)
    J, K = 21, 50
    rng = np.random.default_rng(1000 + J)
    q = np.linalg.qr(rng.normal(size=(3 * J, 3 * J)))[0]
    pca = P.fit_labels((0.5 + rng.normal(0, 0.15, (6 * J + 40, 3 * J)) @ q).astype(np.float32)).to("cuda")
    aug = importlib.import_module(PKG + ".augment")
    for name in ("A", "B"):
        depth, off, hdr = BATCHES[name]()
        gt = joints(name)
        idx = _index(len(hdr), np.random.default_rng(6))
        td, to, th, tg, ti = up(depth, off, hdr, gt, idx)
        ref = oracle.voxelize(*cr.take(depth, off, hdr, idx), R=32, n_threads=8, want_tsdf=False, cam=cam)
        xf = aug.random_affines(ref["mid_p"].astype(np.float64), rng=8)[0]
        for xforms in (None, up(xf)[0]):
            out0, nor0, g0 = pkg.voxelize_indexed(td, to, th, ti, tg, cam=hc, clamp=False, gt_copy=True, xforms=xforms)
            out, nor, g, gt_pca = pkg.voxelize_indexed(td, to, th, ti, tg, cam=hc, clamp=False, gt_copy=True, xforms=xforms,
                                                       pca=pca, k=K)
            torch.cuda.synchronize()
            for a, b in zip(tuple(out) + (nor, g), tuple(out0) + (nor0, g0)):
                assert same(a, b)
            if xforms is None:
                check_placement(out, ref)
            st = out.status.cpu().numpy()
            assert (st == 0).sum() >= 17
            u = pca_ref.normalize(g.cpu().numpy(), out.max_l.cpu().numpy(), out.mid_p.cpu().numpy(), st == 0)
            assert same(nor.cpu().numpy()[st == 0], u[st == 0])
            assert same(gt_pca, pca_ref.project(u, pca.mean, pca.coeff, K))
            alone = pkg.project_joints(g, out.max_l, out.mid_p, pca, K, out=torch.full((len(idx), K), float("nan"), device="cuda"))
            assert same(alone, gt_pca)
            ref64, scale = pca_ref.project64(u, pca.mean, pca.coeff, K)
            assert (np.abs(gt_pca.cpu().numpy() - ref64) <= pca_ref.bound64(ref64, scale, 3 * J)).all()


def _described(pkg, n, R, aug):
    import ctypes
    buf = ctypes.create_string_buffer(160)
    assert pkg._lib.load().tsdf_describe_launch(n, R, 0, int(aug), buf, 160) == 0
    return buf.value.decode()


@functools.lru_cache(maxsize=None)
def _crops(n):
    """n crops: A's 24 and B's 24 in turn."""
    a, b = cr.batch_a(), cr.batch_b()
    both = cr.concat([cr.take(*a, range(24)), b])
    return cr.take(*both, [i % 48 for i in range(n)])


def _fused_and_split(pkg, cam, sets):
    """voxelize and voxelize_aug on each (batch, R, layout, expected kernel) against the oracle under the camera."""
    hc = hip_cam(pkg, cam)
    aug = importlib.import_module(PKG + ".augment")
    for (depth, off, hdr), R, layout, kernel in sets:
        n = len(hdr)
        if kernel is not None:
            assert _described(pkg, n, R, False).startswith(kernel) and _described(pkg, n, R, True).startswith(kernel)
        t = up(depth, off, hdr)
        ref = oracle.voxelize(depth, off, hdr, R=R, layout=LAY[layout], n_threads=8, cam=cam)
        got = pkg.voxelize(*t, res=R, layout=layout, cam=hc)
        torch.cuda.synchronize()
        check_placement(got, ref)
        check_volume(got.tsdf, ref["tsdf"])
        assert (ref["status"] == 0).sum() >= n // 2
        xf = aug.random_affines(ref["mid_p"].astype(np.float64), rng=4)[0]
        refa = oracle.voxelize_aug(depth, off, hdr, xf, R=R, layout=LAY[layout], n_threads=8, cam=cam)
        gota = pkg.voxelize_aug(*t, up(xf)[0], res=R, layout=layout, cam=hc)
        torch.cuda.synchronize()
        check_placement(gota, refa)
        check_volume(gota.tsdf, refa["tsdf"])
        base = oracle.voxelize(depth, off, hdr, R=R, layout=LAY[layout], n_threads=8)
        basea = oracle.voxelize_aug(depth, off, hdr, xf, R=R, layout=LAY[layout], n_threads=8)
        assert not np.array_equal(ref["tsdf"], base["tsdf"]) and not np.array_equal(refa["tsdf"], basea["tsdf"])


@cams
def test_voxelize_and_voxelize_aug_at_64(pkg, cam):
    """R = 64 (the launch<64, ...> instantiations): 9 crops and 3 full frames."""
    a = cr.batch_a()
    mixed = cr.concat([cr.take(*cr.batch_b(), range(5)), cr.take(*a, [0, 1, 2, 3]), cr.take(*a, [24, 25, 26])])
    _fused_and_split(pkg, cam, [(mixed, 64, "czyx", None)])


@cams
def test_voxelize_and_voxelize_aug_on_the_fused_and_the_split_tier(pkg, cam):
    """R = 32: CUs / 2 + 1 crops take the persistent (fused) kernel — csrc/launch.inc::split_plan sends at most CUs / 2
    frames to the split kernel — and 9 frames take the split kernel."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _fused_and_split(pkg, cam, [(_crops(cus // 2 + 1), 32, "czyx", "tsdf_fused_kernel"),
                                (_crops(9), 32, "cxyz", "tsdf_split_kernel")])


# ---- the mapped entries of the extension libraries -------------------------------------------------------------------------
@cams
@pytest.mark.parametrize("name", ["A", "B"])
def test_map_grids_aug_grid_and_map_grid_lowp(pkg, cam, name):
    hc = hip_cam(pkg, cam)
    depth, off, hdr, xf, _ = ok_frames(name, cam)
    t = up(depth, off, hdr, xf)
    n = len(hdr)
    for R in (32, 8):
        rows, max_l, mid_p = mapped_ref(name, cam, R)
        mg = pkg.map_grids(*t, res=R, cam=hc)
        torch.cuda.synchronize()
        assert same(mg.grid, rows) and same(mg.max_l, max_l) and same(mg.mid_p, mid_p) and mg.status.tolist() == [0] * n
        trows, = up(rows)
        for layout in ("czyx", "cxyz"):
            want = mapped_volume(name, cam, R, layout)
            vol, st = pkg.voxelize_aug_grid(*t, trows, res=R, layout=layout, cam=hc)
            torch.cuda.synchronize()
            assert st.tolist() == [0] * n
            err = float(np.abs(vol.cpu().numpy() - want).max())
            print(f"{name} R={R} {layout}: max |hip - oracle| = {err:.3g}")
            assert err <= ar.TOL
            o, = up(want)
            for dtype in DTYPES:
                low, st2 = pkg.voxelize_map_grid_lowp(*t, trows, res=R, layout=layout, dtype=dtype, cam=hc)
                torch.cuda.synchronize()
                assert st2.tolist() == [0] * n and in_band(low, o, TOL)
                # trunc_voxels is not read there (the truncation distance comes with the rows)
                other = pkg.TsdfCam(cam[0], cam[1], cam[2], cam[3], cam[4] + 1.75)
                assert same(pkg.voxelize_map_grid_lowp(*t, trows, res=R, layout=layout, dtype=dtype, cam=other)[0], low)
        if R == 32:
            brows, bmax_l, bmid_p = ar.pixel_grids(depth, off, hdr, xf, R)
            guard(cam, name, (FOCAL, CX, CY, EPS, TRUNC), (rows, max_l, mid_p), (brows, bmax_l, bmid_p))
            bvol, _ = ar.voxelize_aug_grid_ref(depth, off, hdr, xf, rows, R, "czyx")
            guard(cam, name, (FOCAL, CX, CY, EPS), (mapped_volume(name, cam, R, "czyx"),), (bvol,))


# ---- the principal-axis maps ---------------------------------------------------------------------------------------------
def _obb(pkg, depth, off, hdr, cam):
    r = pkg.obb_xforms(*up(depth, off, hdr), cam=hip_cam(pkg, cam))
    torch.cuda.synchronize()
    return pkg.ObbBatch(*(x.cpu().numpy() for x in r))


@cams
@pytest.mark.parametrize("name", ["A", "B"])
def test_obb_xforms(pkg, cam, name):
    depth, off, hdr = BATCHES[name]()
    ref = ob.batch(depth, off, hdr, None, *cam[:4])
    got = _obb(pkg, depth, off, hdr, cam)
    # status and count bit for bit, whatever the camera leaves of a frame
    assert got.status.tolist() == [f["status"] for f in ref]
    assert got.count.tolist() == [float(f["N"]) for f in ref]
    ident = ob.identity()
    n_ok = 0
    for i, f in enumerate(ref):
        if f["status"] == 0:
            check_frame(got, i, f)          # no frame is left out of the axes comparison (tests/test_camera_cpu.py)
            n_ok += 1
        else:
            assert np.array_equal(got.xforms[i], ident), i
            assert not got.mean[i].any() and not got.cov[i].any() and not got.eigenvalues[i].any(), i
    assert n_ok >= 17
    if name == "A" and cam == cr.CAM_EPS:
        assert sum(f["status"] == 1 for f in ref[:24]) >= 5 and sum(f["status"] == 0 for f in ref[:24]) >= 10
    base = ob.batch(depth, off, hdr)
    guard(cam, name, (FOCAL, CX, CY, EPS), [f["xf"] for f in ref] + [np.array([f["N"] for f in ref], np.int64)],
          [f["xf"] for f in base] + [np.array([f["N"] for f in base], np.int64)])


# ---- point clouds and cloud grids ---------------------------------------------------------------------------------------------
@cams
@pytest.mark.parametrize("name", ["A", "B"])
def test_point_clouds(pkg, cam, name):
    depth, off, hdr = BATCHES[name]()
    t = up(depth, off, hdr)
    P, seed = 1500, 9
    want = pcr.point_clouds(depth, off, hdr, P, seed=seed, focal=cam[FOCAL])
    got = pkg.point_clouds(*t, points=P, seed=seed, cam=hip_cam(pkg, cam))
    torch.cuda.synchronize()
    assert pcr.same_bits(got.points.cpu().numpy(), want[0])
    assert np.array_equal(got.count.cpu().numpy(), want[1]) and np.array_equal(got.status.cpu().numpy(), want[2])
    # the principal point is the header's W/2, H/2, not the camera's; invalid_eps and trunc_voxels are not read
    for other in ((cam[FOCAL], 11.5, 200.25, 420.5, 0.5), (cam[FOCAL], 160.0, 120.0, 1e-3, 9.0)):
        again = pkg.point_clouds(*t, points=P, seed=seed, cam=hip_cam(pkg, other))
        torch.cuda.synchronize()
        for a, b in zip(again, got):
            assert same(a, b)
    guard(cam, name, (FOCAL,), (want[0],), (pcr.point_clouds(depth, off, hdr, P, seed=seed)[0],))


@cams
def test_cloud_grids(pkg, cam):
    depth, off, hdr = cr.batch_b()
    pts = pcr.point_clouds(depth, off, hdr, 700, seed=2)[0]
    tp, = up(pts)
    for R in (32, 16):
        want = cg.cloud_grids(pts, R=R, trunc_voxels=cam[TRUNC])
        got = pkg.cloud_grids(tp, res=R, cam=hip_cam(pkg, cam))
        torch.cuda.synchronize()
        for field, a, b in zip(("grid", "max_l", "mid_p", "aabb"), got, want):
            assert cg.same_values(a.cpu().numpy(), b), field
        assert np.array_equal(got.status.cpu().numpy(), want[4]) and not want[4].any()
        # everything but trunc_voxels is not read
        again = pkg.cloud_grids(tp, res=R, cam=pkg.TsdfCam(77.7, 3.5, 250.25, 420.5, cam[TRUNC]))
        torch.cuda.synchronize()
        for a, b in zip(again, got):
            assert same(a, b)
        guard(cam, "B", (TRUNC,), (want[0],), (cg.cloud_grids(pts, R=R)[0],))


# ---- the composites: every field bit-identical to the chain of the parts under the same camera ------------------------------
def same_fields(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None and y is None) or same(x, y), k


def any_differs(a, b):
    return any(x is not None and not same(x, y) for x, y in zip(a, b))


@two_cams
def test_voxelize_lowp_and_voxelize_aug_lowp(pkg, cam):
    hc = hip_cam(pkg, cam)
    depth, off, hdr, xf, gt = ok_frames("B", cam)
    td, to, th, tx, tg = up(depth, off, hdr, xf, gt)
    for dtype, layout in ((torch.bfloat16, "czyx"), (torch.float16, "cxyz")):
        got = pkg.voxelize_lowp(td, to, th, res=32, layout=layout, dtype=dtype, cam=hc)
        ab = pkg.aabb(td, to, th, res=32, cam=hc)
        rows = torch.cat([ab.ori, ab.grid[:, 4:6], torch.zeros_like(ab.ori)], dim=1)
        vol, _ = pkg.voxelize_grid_lowp(td, to, th, rows, res=32, layout=layout, dtype=dtype, cam=hc)
        same_fields(got, (vol, ab.grid[:, 3], ab.grid[:, :3], ab.status))
        assert any_differs(got, pkg.voxelize_lowp(td, to, th, res=32, layout=layout, dtype=dtype))
        # a camera in the placement alone, or in the voxel pass alone, is another volume: both hand-offs count
        assert not same(got.tsdf, pkg.voxelize_grid_lowp(td, to, th, rows, res=32, layout=layout, dtype=dtype)[0])
        got = pkg.voxelize_aug_lowp(td, to, th, tx, res=32, layout=layout, dtype=dtype, cam=hc, gt=tg)
        mg = pkg.map_grids(td, to, th, tx, res=32, cam=hc)
        vol, _ = pkg.voxelize_map_grid_lowp(td, to, th, tx, mg.grid, res=32, layout=layout, dtype=dtype, cam=hc)
        g_aug = pkg.transform_joints(tg, tx)
        same_fields(tuple(got[0]) + got[1:], (vol, mg.max_l, mg.mid_p, mg.status,
                                             pkg.normalize_joints(g_aug, mg.max_l, mg.mid_p), g_aug))
        bare = pkg.voxelize_aug_lowp(td, to, th, tx, res=32, layout=layout, dtype=dtype, cam=hc)
        same_fields(bare, got[0])
        plain = pkg.voxelize_aug_lowp(td, to, th, tx, res=32, layout=layout, dtype=dtype, gt=tg)
        assert any_differs(got[0], plain[0])
        assert not same(got[0].tsdf, pkg.voxelize_map_grid_lowp(td, to, th, tx, mg.grid, res=32, layout=layout, dtype=dtype)[0])
    torch.cuda.synchronize()


@two_cams
def test_voxelize_obb(pkg, cam):
    hc = hip_cam(pkg, cam)
    depth, off, hdr = cr.batch_b()
    td, to, th, tg = up(depth, off, hdr, joints("B"))
    xf = pkg.obb_xforms(td, to, th, cam=hc).xforms
    assert not same(xf, pkg.obb_xforms(td, to, th).xforms)
    for dtype in (None, torch.bfloat16):
        out, nor, gobb, xf2 = pkg.voxelize_obb(td, to, th, res=32, cam=hc, gt=tg, dtype=dtype)
        if dtype is None:
            want = pkg.voxelize_aug(td, to, th, xf, res=32, cam=hc, gt=tg)
        else:
            want = pkg.voxelize_aug_lowp(td, to, th, xf, res=32, dtype=dtype, cam=hc, gt=tg)
        same_fields(tuple(out) + (nor, gobb, xf2), tuple(want[0]) + (want[1], want[2], xf))
        bare, xf3 = pkg.voxelize_obb(td, to, th, res=32, cam=hc, dtype=dtype)
        same_fields(tuple(bare) + (xf3,), tuple(out) + (xf,))
        plain = pkg.voxelize_obb(td, to, th, res=32, gt=tg, dtype=dtype)
        assert any_differs(tuple(out) + (xf2,), tuple(plain[0]) + (plain[3],))
        # the camera's maps under the default camera's voxel pass are another volume: both hand-offs count
        if dtype is None:
            assert not same(out.tsdf, pkg.voxelize_aug(td, to, th, xf, res=32, gt=tg)[0].tsdf)
    torch.cuda.synchronize()


@two_cams
def test_process_batch_and_process_batch_aug(pkg, cam):
    hc = hip_cam(pkg, cam)
    depth, off, hdr = cr.batch_b()
    td, to, th, tg = up(depth, off, hdr, joints("B"))
    kw = dict(points=700, seed=3, frame_base=5, res=32)
    for dtype, layout in ((None, "czyx"), (torch.float16, "cxyz")):
        pc = pkg.point_clouds(td, to, th, points=700, seed=3, frame_base=5, cam=hc)
        grids = pkg.cloud_grids(pc.points, res=32, cam=hc)
        if dtype is None:
            vol, st = pkg.voxelize_grid(td, to, th, grids.grid, res=32, layout=layout, cam=hc)
        else:
            vol, st = pkg.voxelize_grid_lowp(td, to, th, grids.grid, res=32, layout=layout, dtype=dtype, cam=hc)
        assert not bool(pc.status.any()) and not bool(grids.status.any())
        got = pkg.process_batch(td, to, th, layout=layout, cam=hc, dtype=dtype, **kw)
        plain_parts = (pc.points, vol, grids.max_l, grids.mid_p, st, pc.count)
        same_fields(got, plain_parts)
        assert any_differs(got, pkg.process_batch(td, to, th, layout=layout, dtype=dtype, **kw))
        # the augmented half, on maps that are handed in and on maps drawn from the key
        for xforms in (pkg.aug_xforms(grids.mid_p, key=21, counter0=5), None):
            ga = pkg.process_batch_aug(td, to, th, xforms=xforms, gt=tg, aug_seed=4, key=21, layout=layout, cam=hc,
                                       dtype=dtype, **kw)
            xf = pkg.aug_xforms(grids.mid_p, key=21, counter0=5)
            pa = pkg.point_clouds(td, to, th, points=700, seed=4, frame_base=5, xforms=xf, cam=hc)
            ca = pkg.cloud_grids(pa.points, res=32, cam=hc)
            if dtype is None:
                va, sa = pkg.voxelize_aug_grid(td, to, th, xf, ca.grid, res=32, layout=layout, cam=hc)
            else:
                va, sa = pkg.voxelize_map_grid_lowp(td, to, th, xf, ca.grid, res=32, layout=layout, dtype=dtype, cam=hc)
            assert not bool(pa.status.any()) and not bool(ca.status.any())
            same_fields(ga, (pc.points, vol, grids.max_l, grids.mid_p, pa.points, va, ca.max_l, ca.mid_p,
                             pkg.transform_joints(tg, xf), st, sa, pc.count, xf))
            nocam = pkg.process_batch_aug(td, to, th, xforms=xforms, gt=tg, aug_seed=4, key=21, layout=layout, dtype=dtype, **kw)
            assert any_differs((ga.tsdf,), (nocam.tsdf,)) and any_differs((ga.tsdf_aug,), (nocam.tsdf_aug,))
    torch.cuda.synchronize()


@two_cams
def test_augmented_step(pkg, cam):
    """AugmentedStep(cam=..., graph=False), float32 and bfloat16: the chain of the parts it names, with the camera in each."""
    hc = hip_cam(pkg, cam)
    depth, off, hdr = cr.batch_b()
    td, to, th, tg = up(depth, off, hdr, joints("B"))
    n = 9
    idx = torch.tensor([3, 23, 0, 7, 7, 11, 19, 2, 14], dtype=torch.int64, device=dev())
    centres = pkg.aabb(td, to, th, res=32, cam=hc).grid[:, :3].contiguous()
    assert not same(centres, pkg.aabb(td, to, th, res=32).grid[:, :3].contiguous())
    xf = pkg.aug_xforms_at(centres, pkg.aug_state(77, 1000, device=dev()), index=idx)
    for dtype in (None, torch.bfloat16):
        step = pkg.AugmentedStep(td, to, th, n, gt=tg, res=32, cam=hc, graph=False, dtype=dtype)
        assert same(step.centres, centres)
        out, nor, gaug = step.step(idx, key=77, counter0=1000)
        torch.cuda.synchronize()
        assert same(step.xforms, xf)
        if dtype is None:
            want, wnor, wg = pkg.voxelize_indexed(td, to, th, idx, tg, res=32, cam=hc, xforms=xf, gt_copy=True)
        else:
            want, wnor, wg = pkg.voxelize_aug_lowp(td, to, th, xf, res=32, dtype=dtype, cam=hc, gt=tg, index=idx)
        same_fields(tuple(out) + (nor, gaug), tuple(want) + (wnor, wg))
        assert not bool(out.status.any())
        plain = pkg.AugmentedStep(td, to, th, n, gt=tg, res=32, graph=False, dtype=dtype)
        pout, pnor, _ = plain.step(idx, key=77, counter0=1000)
        torch.cuda.synchronize()
        assert any_differs(tuple(out) + (nor,), tuple(pout) + (pnor,))
        # the camera's centres under the default camera's voxel pass are another volume: both hand-offs count
        half = pkg.AugmentedStep(td, to, th, n, gt=tg, centres=centres, res=32, graph=False, dtype=dtype)
        hout = half.step(idx, key=77, counter0=1000)[0]
        torch.cuda.synchronize()
        assert same(half.xforms, xf) and not same(hout.tsdf, out.tsdf)
