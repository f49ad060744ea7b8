"""CPU tier of the composed maps and the fused step head (include/tsdf_mapstep.h): libtsdf_mapstep.so as far as it goes
without a GPU — the build rule, the binding through _lib._EXTS, the version, the argument checks before device work
—, the public names, and the reference the GPU tier compares against (tests/mapstep_ref.py::compose_np): that it composes.
Nothing here touches a GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapstep_ref as mr  # noqa: E402
import obb_ref  # noqa: E402
from abi_util import declared_functions, exported  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "handposeestimation-with-3d-cnns_amd", "csrc")
INVALID, NO_DEVICE = -1, -2
WANT = ["tsdf_compose_xforms_hip", "tsdf_map_step_head_hip", "tsdf_mapstep_version"]


# ---- build rule ----
def test_make_rules_cross_compile_for_gfx950_without_scratch():
    r = subprocess.run(["make", "-C", CSRC, "mapstep", "mapstep-resources"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stdout + r.stderr
    for kernel in ("tsdf_compose_kernel", "tsdf_map_step_draw_kernel", "tsdf_map_step_head_kernel"):
        assert kernel in text, kernel
    scratch = [ln for ln in text.splitlines() if "ScratchSize" in ln]
    assert len(scratch) == 3 and all(ln.split("]:")[1].split()[0] == "0" for ln in scratch), scratch


# ---- binding ----
def test_row_binds_exactly_its_header_with_types(pkg):
    ext = pkg._lib._EXTS["mapstep"]
    assert isinstance(ext, pkg._lib._Ext)
    assert declared_functions("tsdf_mapstep.h") == WANT == sorted([ext.version_symbol, *ext.entries])
    funcs, named = exported(pkg._lib.MAPSTEP_LIB_PATH)
    assert funcs == WANT and named == WANT
    assert ext.path == pkg._lib.MAPSTEP_LIB_PATH and ext.version == pkg._lib.MAPSTEP_VERSION == 1
    L = pkg._lib.load_mapstep()
    assert L.tsdf_mapstep_version() == 1
    for entry in (ext.version_symbol, *ext.entries):
        fn = getattr(L, entry)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, entry
    vp, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    f64, f32 = ctypes.c_double, ctypes.c_float
    assert list(L.tsdf_compose_xforms_hip.argtypes) == [vp, vp, i64, vp, i, vp, vp]
    assert list(L.tsdf_map_step_head_hip.argtypes) == [vp, i64, vp, vp, i64, vp, i, i, f64, f64, f64, f32, f32, vp, vp, vp, vp,
                                                       vp, i, i, vp] + [vp] * 9
    for name, args in ext.entries.items():
        assert list(getattr(L, name).argtypes) == args and args
    assert pkg._lib.load_mapstep() is L and L is not pkg._lib.load() and L is not pkg._lib.load_maplowp()
    # the product beside it is what it was
    assert pkg._lib.load().tsdf_version() == 7


# ---- argument checks ----
def test_argument_validation_happens_before_device_work(pkg):
    L = pkg._lib.load_mapstep()
    null, one, odd, odd4 = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(72), ctypes.c_void_p(68)

    def compose(outer=one, inner=one, n_inner=1, index=null, n=1, out=one):
        return L.tsdf_compose_xforms_hip(outer, inner, n_inner, index, n, null, out)

    assert compose(n=-1) == INVALID
    for name in ("outer", "inner", "out"):
        assert compose(**{name: null}) == INVALID, name
        assert compose(**{name: odd4}) == INVALID, name                   # 4-byte, not 8-byte aligned
        assert compose(**{name: odd}) == NO_DEVICE, name                  # 8-byte aligned will do
    assert compose(n_inner=0, index=one) == INVALID and compose(n_inner=-3, index=one) == INVALID
    assert compose(n_inner=2) == INVALID and compose(n=2) == INVALID      # no index: n_inner must equal n
    assert compose() == NO_DEVICE                                         # valid arguments get as far as the device
    assert compose(n_inner=5, index=one, n=3) == NO_DEVICE
    assert compose(n=2 ** 31 - 1, n_inner=2 ** 31 - 1) == NO_DEVICE
    assert compose(n=0, n_inner=0) == 0                                    # n == 0 is a no-op
    assert L.tsdf_compose_xforms_hip(null, null, 0, null, 0, null, null) == 0

    def head(depth=one, depth_len=100, offsets=one, headers=one, n_src=1, index=null, n=1, R=32,
             cam=(241.42, 160.0, 120.0, 1.0, 3.0), centres=one, base=null, state=one, counters=null, gt=null, n_joints=0,
             clamp=1, xforms=one, grid=one, max_l=one, mid_p=one, status=one, gt_aug=null, gt_nor=null, stretch=null,
             rot=null):
        return L.tsdf_map_step_head_hip(depth, depth_len, offsets, headers, n_src, index, n, R, *cam, centres, base, state,
                                        counters, gt, n_joints, clamp, null, xforms, grid, max_l, mid_p, status, gt_aug,
                                        gt_nor, stretch, rot)

    labels = dict(gt=one, n_joints=21, gt_aug=one, gt_nor=one)
    draw_only = dict(depth=null, offsets=null, headers=null, grid=null, max_l=null, mid_p=null, status=null)
    assert head(n=-1) == INVALID
    for R in (0, 2, 3, 6, 30, 132, 256, -4):
        assert head(R=R) == INVALID, R
    for name in ("centres", "state", "xforms"):
        assert head(**{name: null}) == INVALID, name
    assert head(n_src=0, index=one) == INVALID and head(n_src=-3, index=one) == INVALID
    assert head(n_src=2) == INVALID and head(n=2) == INVALID              # no index: n_src must equal n
    for name in ("xforms", "state", "base"):
        assert head(**{name: odd4}) == INVALID, name
        assert head(**{name: odd}) == NO_DEVICE, name
    # the camera comes by value and goes through the camera rule of every entry (csrc/prim.inc::cam_ok): focal,
    # invalid_eps and trunc_voxels each > 0, a NaN is not, whichever fields the launch reads; n == 0 stays a no-op
    nan = float("nan")
    for bad in ((0.0, 160.0, 120.0, 1.0, 3.0), (-1.0, 160.0, 120.0, 1.0, 3.0), (nan, 160.0, 120.0, 1.0, 3.0),
                (241.42, 160.0, 120.0, 0.0, 3.0), (241.42, 160.0, 120.0, -1.0, 3.0), (241.42, 160.0, 120.0, nan, 3.0),
                (241.42, 160.0, 120.0, 1.0, 0.0), (241.42, 160.0, 120.0, 1.0, nan), (241.42, 160.0, 120.0, 1.0, -0.0)):
        assert head(cam=bad) == INVALID, bad
        assert head(cam=bad, **draw_only) == INVALID, bad
        assert head(cam=bad, n=0, n_src=0) == 0, bad
    for good in ((588.03, 320.5, 240.25, 0.5, 2.0), (241.42, nan, -7.0, 1e-3, 8.0)):   # cx, cy are not judged
        assert head(cam=good) == NO_DEVICE and head(cam=good, **draw_only) == NO_DEVICE, good
    # with a grid the source tables are read ...
    for name in ("depth", "offsets", "headers"):
        assert head(**{name: null}) == INVALID, name
    assert head(depth_len=-1) == INVALID
    # ... without one they are not, and nothing that needs the placement may be asked for
    assert head(**draw_only) == NO_DEVICE
    assert head(**dict(draw_only, depth_len=-1)) == NO_DEVICE
    for name in ("max_l", "mid_p", "status"):
        assert head(**dict(draw_only, **{name: one})) == INVALID, name
    assert head(**dict(draw_only, **labels)) == INVALID
    # labels: d_gt needs d_out_gt_nor and 1..170 joints; the label outputs need d_gt
    assert head(**labels) == NO_DEVICE
    assert head(**dict(labels, gt_aug=null)) == NO_DEVICE
    assert head(**dict(labels, gt_nor=null)) == INVALID
    for nj in (0, -1, 171):
        assert head(**dict(labels, n_joints=nj)) == INVALID, nj
    assert head(**dict(labels, n_joints=1)) == NO_DEVICE and head(**dict(labels, n_joints=170)) == NO_DEVICE
    assert head(gt_aug=one) == INVALID and head(gt_nor=one) == INVALID
    # valid arguments get as far as the device, and there is none here
    assert head() == NO_DEVICE
    assert head(max_l=null, mid_p=null, status=null) == NO_DEVICE         # every scalar output is optional
    assert head(base=one, counters=one, stretch=one, rot=one) == NO_DEVICE
    assert head(n_src=5, index=one, n=3) == NO_DEVICE
    assert head(n=2 ** 31 - 1, n_src=2 ** 31 - 1) == NO_DEVICE            # the head strides over any n
    for R in (4, 12, 64, 128):
        assert head(R=R) == NO_DEVICE, R
    assert head(n=0, n_src=0) == 0                                        # n == 0 is a no-op
    assert L.tsdf_map_step_head_hip(null, 0, null, null, 0, null, 0, 32, 0.0, 0.0, 0.0, 0.0, 0.0, null, null, null, null, null,
                                    0, 0, null, null, null, null, null, null, null, null, null, null) == 0


# ---- public names and refusals ----
def test_public_names_and_refusals(pkg, synth):
    for name in ("compose_xforms", "map_step_head", "MapStepBatch"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
        assert name in pkg.__doc__ or name == "MapStepBatch", name   # (the docstring lists functions, not result types)
    assert "tsdf_mapstep.h" in pkg.__doc__ and "AugmentedStep(base=" in pkg.__doc__
    assert pkg.MapStepBatch._fields == ("xforms", "grid", "max_l", "mid_p", "status", "gt_aug", "gt_nor")
    assert "base" in pkg.AugmentedStep.__doc__ and "fused_head" in pkg.AugmentedStep.__doc__
    depth, off, hdr = (torch.from_numpy(x) for x in synth.synth_batch(2, "crop", seed0=3))
    xf = torch.from_numpy(pkg.augment.identity_affines(2))
    # there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        pkg.compose_xforms(xf, xf)
    with pytest.raises(ValueError, match="GPU"):
        pkg.map_step_head(depth, off, hdr, torch.zeros((2, 3)), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="GPU"):
        pkg.AugmentedStep(depth, off, hdr, 2, base=xf)
    with pytest.raises(ValueError, match="fused_head"):
        pkg.AugmentedStep(depth, off, hdr, 2, fused_head=1.5)
    with pytest.raises(TypeError):
        pkg.compose_xforms(np.zeros((2, 24)), xf)


# ---- the reference composes ----
def _affines(pkg, n, seed):
    """n random augmentations about random centres a few hundred millimetres from the origin."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 150, (n, 3)) + np.array([0.0, 0.0, -450.0])
    return pkg.augment.random_affines(centres, rng=seed)[0]


def _obb36():
    depth, off, hdr = mr.frames36()
    frames = obb_ref.batch(depth, off, hdr)
    assert all(f["status"] == 0 for f in frames)
    return np.stack([f["xf"] for f in frames]), np.stack([f["mu"] for f in frames])


def _check_composes(outer, inner, pts):
    """The composed forward map is inner-then-outer and the composed inverse undoes it, at points pts [n,k,3].

    The bounds are a priori.  With S the sum of the absolute values of the fully expanded terms of one output coordinate
    (|P||Q||p| + |P||q| + |p_b|), either way of computing it — the composed rows applied once, or the two maps applied in
    turn — puts at most 9 roundings on a term, (1 + u)^9 - 1 < 10u, so the two differ by less than 20 u S: the test asks
    24 u S.  The way back adds what the inputs themselves are off by: the inverse rows of a map are the inverse of its
    forward rows only to rounding — a rotation from sin / cos products or an eigen-decomposition is orthogonal to about
    10u, and np.linalg.inv, b' = -A'b add a few u — so each of the two maps contributes up to 16 u S and the arithmetic
    of the round trip (two applications of composed rows) 20 u S: 52 u S, the test asks 64 u S."""
    comp = mr.compose_np(outer, inner)
    n = len(outer)
    c4, o4, i4 = (np.abs(x.reshape(n, 2, 3, 4)) for x in (comp, outer, inner))
    for k in range(n):
        p = pts[k]
        want = mr.apply(outer[k], mr.apply(inner[k], p))
        got = mr.apply(comp[k], p)
        ap = np.abs(p)
        inner_s = ap @ i4[k, 0, :, :3].T + i4[k, 0, :, 3]                       # |Q||p| + |q|
        S = inner_s @ o4[k, 0, :, :3].T + o4[k, 0, :, 3]                        # |P|(|Q||p| + |q|) + |p_b|
        assert (np.abs(got - want) <= 24 * mr.U * S).all(), (k, np.abs(got - want).max(), (24 * mr.U * S).min())
        back = mr.apply(comp[k], got, inverse=True)
        Sc = (np.abs(got) @ c4[k, 1, :, :3].T + c4[k, 1, :, 3])                 # the composed inverse's own terms at T(p)
        Sb = np.maximum(Sc, (S @ o4[k, 1, :, :3].T + o4[k, 1, :, 3]) @ i4[k, 1, :, :3].T + i4[k, 1, :, 3])
        assert (np.abs(back - p) <= 64 * mr.U * Sb).all(), (k, np.abs(back - p).max(), (64 * mr.U * Sb).min())


def test_compose_np_composes_random_affines(pkg):
    outer, inner = _affines(pkg, 64, 1), _affines(pkg, 64, 2)
    pts = np.random.default_rng(3).normal(0, 120, (64, 50, 3)) + np.array([0.0, 0.0, -450.0])
    _check_composes(outer, inner, pts)
    _check_composes(inner, outer, pts)


def test_compose_np_composes_augmentations_with_obb_maps(pkg):
    inner, mu = _obb36()
    outer = pkg.augment.random_affines(mu, rng=4)[0]
    pts = mu[:, None, :] + np.random.default_rng(5).normal(0, 60, (36, 50, 3))
    _check_composes(outer, inner, pts)


def test_compose_np_identity_index_and_layout(pkg):
    inner, mu = _obb36()
    outer = pkg.augment.random_affines(mu, rng=6)[0]
    ident = pkg.augment.identity_affines(36)
    # the identity on either side returns the other map, as numbers
    assert np.array_equal(mr.compose_np(ident, inner), inner) and np.array_equal(mr.compose_np(outer, ident), outer)
    assert np.array_equal(mr.compose_np(ident, outer), outer) and np.array_equal(mr.compose_np(inner, ident), inner)
    # an index gathers the inner maps; outside them the result is outer itself, NaNs and all
    idx = np.array([7, 3, 3, 35, 0, -1, 36, 1], np.int64)
    o8 = outer[:8].copy()
    o8[5, 3] = np.nan
    got = mr.compose_np(o8, inner, idx)
    ok = (idx >= 0) & (idx < 36)
    assert np.array_equal(got[ok], mr.compose_np(o8[ok], inner[idx[ok]]))
    assert np.array_equal(got[~ok].view(np.uint64), o8[~ok].view(np.uint64))
    # the halves: the forward rows of the result use forward rows alone, the inverse rows inverse rows alone
    swapped = mr.compose_np(np.concatenate([outer[:, :12], ident[:, 12:]], 1), np.concatenate([inner[:, :12], ident[:, 12:]], 1))
    assert np.array_equal(swapped[:, :12], mr.compose_np(outer, inner)[:, :12]) and np.array_equal(swapped[:, 12:], ident[:, 12:])
    # one entry written out by hand
    P, Q = outer[0].reshape(2, 3, 4)[0], inner[0].reshape(2, 3, 4)[0]
    c = mr.compose_np(outer[:1], inner[:1])[0].reshape(2, 3, 4)
    assert c[0, 1, 2] == (P[1, 0] * Q[0, 2] + P[1, 1] * Q[1, 2]) + P[1, 2] * Q[2, 2]
    assert c[0, 2, 3] == ((P[2, 0] * Q[0, 3] + P[2, 1] * Q[1, 3]) + P[2, 2] * Q[2, 3]) + P[2, 3]
    Pi, Qi = inner[0].reshape(2, 3, 4)[1], outer[0].reshape(2, 3, 4)[1]
    assert c[1, 0, 3] == ((Pi[0, 0] * Qi[0, 3] + Pi[0, 1] * Qi[1, 3]) + Pi[0, 2] * Qi[2, 3]) + Pi[0, 3]
