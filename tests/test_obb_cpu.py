"""CPU tier of the principal-axis maps (include/tsdf_obb.h): libtsdf_obb.so as far as it goes without a GPU — the binding,
the version, the argument checks before device work —, the soundness of the tests' own restatement (tests/obb_ref.py), the
invariance the feature exists for, and the public names and refusals.  Nothing here touches a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obb_ref as ob  # noqa: E402
from abi_util import declared_functions, exported  # noqa: E402

torch = pytest.importorskip("torch")



# ---- binding ----
def test_row_binds_exactly_its_header_with_types(pkg):
    ext = pkg._lib._EXTS["obb"]
    want = ["tsdf_obb_version", "tsdf_obb_xforms_hip"]
    assert declared_functions("tsdf_obb.h") == want == sorted([ext.version_symbol, *ext.entries])
    funcs, named = exported(pkg._lib.OBB_LIB_PATH)
    assert funcs == want and named == want
    assert ext.path == pkg._lib.OBB_LIB_PATH and ext.version == pkg._lib.OBB_VERSION == 1
    L = pkg._lib.load_obb()
    assert L.tsdf_obb_version() == 1
    for entry in (ext.version_symbol, *ext.entries):
        fn = getattr(L, entry)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, entry
    vp, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert list(L.tsdf_obb_xforms_hip.argtypes) == [vp, i64, vp, vp, i, ctypes.POINTER(pkg._lib.TsdfCam), vp, vp, vp, vp]
    assert list(L.tsdf_obb_xforms_hip.argtypes) == ext.entries["tsdf_obb_xforms_hip"]
    assert pkg._lib.load_obb() is L and L is not pkg._lib.load()
    # the product beside it is what it was
    assert pkg._lib.load().tsdf_version() == 7


def test_argument_validation_happens_before_device_work(pkg):
    fn = pkg._lib.load_obb().tsdf_obb_xforms_hip
    null, one, odd4, odd2 = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(68), ctypes.c_void_p(66)

    def call(depth=one, depth_len=100, offsets=one, headers=one, n=1, xforms=one, moments=one, status=one):
        return fn(depth, depth_len, offsets, headers, n, None, null, xforms, moments, status)

    assert call(n=-1) == -1
    for name in ("depth", "offsets", "headers", "xforms"):
        assert call(**{name: null}) == -1, name
    assert call(depth_len=-1) == -1
    assert call(xforms=odd4) == -1            # not 8-byte aligned
    assert call(moments=odd4) == -1
    assert call(status=odd2) == -1            # not 4-byte aligned
    # n == 0 is a no-op with NULL everywhere, whatever else is passed
    assert fn(null, 0, null, null, 0, None, null, null, null, null) == 0
    assert fn(null, -5, null, null, 0, None, null, odd4, odd4, odd2) == 0


# ---- the restatement ----
@pytest.fixture(scope="module")
def frames(synth):
    """The 24 crops and 12 full frames the GPU tier uses, each with its restatement."""
    out = []
    for n, kind in ((24, "crop"), (12, "full")):
        depth, off, hdr = synth.synth_batch(n, kind, seed0=42)
        out += ob.batch(depth, off, hdr)
    assert len(out) == 36 and all(f["status"] == 0 for f in out)
    return out


def test_restatement_properties(pkg, frames):
    for f in frames:
        A, C, mu, lam = f["A"], f["C"], f["mu"], f["lam"]
        assert np.abs(A @ A.T - np.eye(3)).max() <= 64 * ob.U
        assert abs(np.linalg.det(A) - 1.0) <= 64 * ob.U
        D = A @ C @ A.T
        tr = np.trace(C)
        assert np.abs(D - np.diag(np.diag(D))).max() <= 256 * ob.U * tr       # diagonal ...
        assert np.abs(np.diag(D) - lam).max() <= 256 * ob.U * tr               # ... with the eigenvalues,
        assert lam[0] >= lam[1] >= lam[2] >= -256 * ob.U * tr                  # descending
        mapped = ob.apply(f["xf"], f["pts"])
        scale = np.abs(f["pts"]).max()
        assert np.abs(mapped.mean(axis=0) - mu).max() <= 4 * f["N"] * ob.U * scale   # a rotation about the centroid
        assert A[0, 1] >= 0 and A[2, 2] >= 0
        b = f["xf"][:12].reshape(3, 4)[:, 3]
        np.testing.assert_allclose(pkg.augment.pack_affine(A, b), f["xf"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(ob.apply(f["xf"], mapped, inverse=True), f["pts"], rtol=0, atol=1e-9)


def test_the_gpu_tiers_input_conditions_hold(frames):
    """What tests/test_obb_gpu.py asserts of its inputs, shown here too: separated eigenvalues and signs away from 0."""
    gaps = [min(ob.rel_gaps(f["lam"])) for f in frames]
    e1y = [abs(f["A"][0, 1]) for f in frames]
    e3z = [abs(f["A"][2, 2]) for f in frames]
    print(f"smallest relative gap {min(gaps):.3g}, |e1.y| {min(e1y):.3g}, |e3.z| {min(e3z):.3g}")
    assert min(gaps) >= 1e-3 and min(e1y) >= 1e-6 and min(e3z) >= 1e-6


def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) if axis == "z" else np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]])


def _map_of_cloud(pts):
    """The restatement's map of an arbitrary cloud (what ob.frame does after the back-projection)."""
    mu = pts.sum(axis=0) / len(pts)
    q = pts - mu
    w, V = np.linalg.eigh((q.T @ q) / len(pts))
    e1, e3 = V[:, 2].copy(), V[:, 0].copy()
    if e1[1] < 0:
        e1 = -e1
    if e3[2] < 0:
        e3 = -e3
    A = np.stack([e1, np.cross(e3, e1), e3])
    return A, ob.pack_rotation(A, mu)


def test_invariance_under_rotation_about_the_centroid(frames):
    """The point of the feature: a cloud turned about its centroid, mapped with ITS OWN map, lands where the mapped
    original does, to 1e-9 mm — for every (frame, turn) where no sign rule changes side.  The sign rules look at e1.y and
    e3.z in the camera frame, so a turn that carries one of them through 0 picks the mirrored axes; the result is then
    the mapped original turned by 180 degrees about an axis of the box (signs diag(s1, s1 s3, s3) about the centroid), and
    that is checked too, so all 216 pairs are compared.

    Figures for these seeds: 140 of the 216 pairs keep both signs (per turn: z+5 19, z-5 18, z+20 19, z-20 18, x+10 32,
    x-10 34 of 36 frames); every one of the 36 frames keeps them under at least one turn, but only 1 under all six — the
    synthetic hands lie along the image's x axis (|e1.y| is mostly below 0.03), so the rule on e1.y is close to a coin toss
    under a turn about z.  A frame counts as qualifying when at least one of its turns keeps both signs; the pairs that
    keep them must also number at least 20 per turn on average (120 of 216), so the test cannot pass empty."""
    turns = [("z", 5), ("z", -5), ("z", 20), ("z", -20), ("x", 10), ("x", -10)]
    qualified, pairs = 0, 0
    for f in frames:
        pts, mu, A = f["pts"], f["mu"], f["A"]
        want = ob.apply(f["xf"], pts)
        kept = 0
        for axis, deg in turns:
            Q = _rot(axis, deg)
            turned = (pts - mu) @ Q.T + mu
            # the original's axes, carried along: the turned cloud's axes up to the signs its own rules pick
            e1, e3 = Q @ A[0], Q @ A[2]
            assert e1[1] != 0 and e3[2] != 0
            s1, s3 = (1.0 if e1[1] > 0 else -1.0), (1.0 if e3[2] > 0 else -1.0)
            got = ob.apply(_map_of_cloud(turned)[1], turned)
            assert np.abs(got - ((want - mu) * np.array([s1, s1 * s3, s3]) + mu)).max() <= 1e-9
            kept += s1 > 0 and s3 > 0
        pairs += kept
        qualified += kept > 0
    print(f"{qualified} of {len(frames)} frames keep their signs under a turn; {pairs} of {6 * len(frames)} pairs do")
    assert qualified >= 20 and pairs >= 120


# ---- public names and refusals ----
def test_public_names_and_refusals(pkg, synth):
    for name in ("obb_xforms", "voxelize_obb", "invert_xforms", "ObbBatch"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
    assert pkg.ObbBatch._fields == ("xforms", "status", "count", "mean", "cov", "eigenvalues")
    assert "obb_xforms" in pkg.__doc__ and 'frame="obb"' in pkg.__doc__
    depth, off, hdr = (torch.from_numpy(x) for x in synth.synth_batch(2, "crop", seed0=3))
    with pytest.raises(ValueError, match="GPU"):
        pkg.obb_xforms(depth, off, hdr)
    with pytest.raises(ValueError, match="GPU"):
        pkg.voxelize_obb(depth, off, hdr)
    with pytest.raises(TypeError):
        pkg.obb_xforms(depth.numpy(), off, hdr)
    # invert_xforms is a pure tensor operation
    xf = torch.arange(48, dtype=torch.float64).reshape(2, 24)
    inv = pkg.invert_xforms(xf)
    assert torch.equal(inv[:, :12], xf[:, 12:]) and torch.equal(inv[:, 12:], xf[:, :12])
    assert torch.equal(pkg.invert_xforms(inv), xf)
    with pytest.raises(ValueError):
        pkg.invert_xforms(xf.reshape(4, 12))
    # the loader refuses before anything is uploaded (there is no GPU here to upload to)
    d, o, h = synth.synth_batch(4, "crop", seed0=3)
    ds = pkg.MSRADepthDataset.from_packs([pkg.packing.PackedFrames(d, o, h, np.zeros((4, 63), np.float32))])
    for kw in (dict(frame="obb", augment=True), dict(frame="obb", augment="device"), dict(frame="x"),
               dict(frame="obb", augment="device", graph=True)):
        with pytest.raises(ValueError):
            pkg.ResidentLoader(ds, batch_size=2, device="cuda", **kw)
    ld = pkg.ResidentLoader(ds, batch_size=2, device="cuda", frame="obb")
    assert ld.frame == "obb" and ld.obb is None and ld.obb_status is None
    assert pkg.ResidentLoader(ds, batch_size=2, device="cuda").frame == "camera"
    assert pkg.VoxelBatch._fields == ("tsdf", "gt", "max_l", "mid_p", "status", "gt_nor")
