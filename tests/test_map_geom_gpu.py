"""GPU tier of the geometric pin of the mapped voxel contract: every voxel pass that takes a per-frame map — the split and
the fused (static, queue) kernels of voxelize_aug, voxelize_aug_grid, voxelize_map_grid_lowp — against
tests/map_geom_ref.py (the header's sentence formed explicitly in longdouble) under the named map family: turns past 90
degrees about every axis, anisotropic scale, shear, reflection, a general affine map, the frame's own principal-axis map,
power-of-two scales and the cyclic axis permutations.

One comparison for all of them: the kernel's volume against ``map_geom_ref.voxels`` evaluated on the grid row the kernel
itself placed (``map_grids``, whose max_l / mid_p bits are asserted equal to the fused entry's, so no placement tolerance
leaks into the volumes); <= 1e-5 (the project's contract figure) in every non-fragile voxel, zero masks equal everywhere.
tests/test_map_geom_cpu.py asserts on the same frames and maps that the fragile share is <= 1e-4 and that no frame is
zeros against zeros.  The placement itself is checked against ``map_geom_ref.placement`` within the bound derived there,
the labels within one float32 spacing.  The exact relations (scales: the identity volume bit for bit; cyclic maps: its
magnitudes permuted bit for bit) cannot be passed by rounding luck.  Run with -s to see the figures."""
import ctypes
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
import camera_ref  # noqa: E402
import map_geom_ref as mg  # noqa: E402
from test_pca_paths_gpu import kernel_path, n_for  # noqa: E402

pytestmark = pytest.mark.gpu

PKG = "handposeestimation-with-3d-cnns_amd"
TOL = ar.TOL
DEV = "cuda"
PERIOD = len(mg.MAPS)
CAMS = {"default": mg.DEFAULT_CAM, "f300": camera_ref.FRACTIONAL}
# half a spacing of the 2-byte type just below 1, where the spacing of |values| <= 1 is largest: float16 has 11
# significant bits (spacing 2^-11 in [0.5, 1)), bfloat16 has 8 (2^-8) — round-to-nearest of a float32 within TOL of the
# reference lands within TOL + that half spacing of it
LOWP = {"f16": (torch.float16, 2.0 ** -12), "bf16": (torch.bfloat16, 2.0 ** -9)}


def up(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def fbits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def rt(R):
    return R if R in (32, 64) else 0      # the compile-time resolutions (csrc/abi.inc::tsdf_describe_launch)


def described(pkg, n, R, layout, aug=1):
    buf = ctypes.create_string_buffer(160)
    assert pkg._lib.load().tsdf_describe_launch(n, R, ar.LAYOUTS[layout], int(aug), buf, 160) == 0
    return buf.value.decode()


@functools.lru_cache(maxsize=None)
def _period(cam="default"):
    """The 15 positions of one period (tests/map_geom_ref.py::case_batch): one frame per map.  Never modified."""
    return mg.case_batch(importlib.import_module(PKG + ".synth"), PERIOD, CAMS[cam])


def tiled(n, cam="default"):
    """n positions, position k = position k mod 15 of the period."""
    depth, off, hdr, names, xf = _period(cam)
    k = [i % PERIOD for i in range(n)]
    d, o, h = mg.take(depth, off, hdr, k)
    return d, o, h, [names[i] for i in k], xf[k]


_REFS = {}


def reference(cam, k, row, R):
    """map_geom_ref.voxels (czyx) of period position k on the grid row ``row``: computed once per row, never modified."""
    key = (cam, k, R, np.asarray(row, np.float32).tobytes())
    if key not in _REFS:
        depth, off, hdr, _, xf = _period(cam)
        _REFS[key] = mg.voxels(depth[off[k]:off[k + 1]], hdr[k], row, R, "czyx", xf[k], CAMS[cam])
    return _REFS[key]


def check_volume(vol, row, k, R, layout, cam="default", extra=0.0):
    """One frame's volume (numpy float32 / float64 [3,R,R,R] in ``layout``) against the reference on ``row``; returns the
    largest deviation outside the fragile set."""
    ref, valid, fragile = reference(cam, k, row, R)
    if layout == "cxyz":
        ref = ref.transpose(0, 3, 2, 1)
    solid = ~np.broadcast_to(mg.mask_in(fragile, layout), ref.shape)
    err = np.abs(vol.astype(np.float64) - ref.astype(np.float64))
    worst = float(err[solid].max())
    assert worst <= TOL + extra, (mg.MAPS[k], R, layout, worst)
    assert np.array_equal((vol != 0).any(0), mg.mask_in(valid, layout)[0]), (mg.MAPS[k], "zero mask")
    assert np.array_equal(vol == 0, ~np.broadcast_to(mg.mask_in(valid, layout), ref.shape)), (mg.MAPS[k], "zero channels")
    if extra:     # a 2-byte volume: far values and zeros are exact
        for v in (1.0, -1.0):
            assert (vol[solid & (ref == v)] == v).all(), (mg.MAPS[k], v)
    return worst


def check_placement(mgb, ks, R, cam="default"):
    """map_grids' rows, max_l, mid_p of period positions ``ks`` against map_geom_ref.placement + the float32 glue, within the
    bound derived in tests/map_geom_ref.py."""
    depth, off, hdr, _, xf = _period(cam)
    rows, max_l, mid_p = mgb.grid.cpu().numpy(), mgb.max_l.cpu().numpy(), mgb.mid_p.cpu().numpy()
    assert not mgb.status.any() and not rows[:, 5:].any()
    for i, k in enumerate(ks):
        mn, mx, M = mg.placement(depth[off[k]:off[k + 1]], hdr[k], xf[k], R, CAMS[cam])
        g, ori = oracle.glue(mn, mx, R, CAMS[cam])
        b = mg.placement_bounds(M, R)
        assert np.abs(mid_p[i].astype(np.float64) - g[:3]).max() <= b["mid_p"], mg.MAPS[k]
        assert abs(float(max_l[i]) - float(g[3])) <= b["max_l"], mg.MAPS[k]
        assert abs(float(rows[i, 3]) - float(g[4])) <= b["voxel_len"], mg.MAPS[k]
        assert np.abs(rows[i, :3].astype(np.float64) - ori).max() <= b["vox_ori"], mg.MAPS[k]
        assert float(rows[i, 4]) == float(np.float32(rows[i, 3] * np.float32(CAMS[cam][4])))
    return rows


def run_aug(pkg, n, R, layout, cam="default"):
    """voxelize_aug and map_grids of n tiled positions; the two placements agree bit for bit.  -> (TsdfBatch, MapGridBatch)"""
    c = None if cam == "default" else pkg.TsdfCam(*CAMS[cam])
    t = up(*[a for j, a in enumerate(tiled(n, cam)) if j != 3])
    out = pkg.voxelize_aug(*t, res=R, layout=layout, cam=c)
    mgb = pkg.map_grids(*t, res=R, cam=c)
    torch.cuda.synchronize()
    assert not out.status.any()
    assert torch.equal(fbits(mgb.max_l), fbits(out.max_l)) and torch.equal(fbits(mgb.mid_p), fbits(out.mid_p))
    return out, mgb


def check_frames(out, mgb, frames, R, layout, cam="default"):
    rows = mgb.grid[frames].cpu().numpy()
    vols = out.tsdf[frames].cpu().numpy()
    return max(check_volume(vols[j], rows[j], f % PERIOD, R, layout, cam) for j, f in enumerate(frames))


def check_periods(out, n):
    """Every period of the batch equals the first, compared on the device."""
    for p in range(PERIOD, n, PERIOD):
        m = min(PERIOD, n - p)
        assert torch.equal(fbits(out.tsdf[p:p + m]), fbits(out.tsdf[:m])), p
        assert torch.equal(fbits(out.max_l[p:p + m]), fbits(out.max_l[:m])), p
        assert torch.equal(fbits(out.mid_p[p:p + m]), fbits(out.mid_p[:m])), p


# ---- voxelize_aug: small batches (the split kernel wherever the library splits) ----
def slice_rounds(R):
    """csrc/launch.inc::split_plan: the passes a 1024-thread workgroup needs for the R slices of a volume.  Below two there
    is nothing to split and a small batch goes to the fused kernel (tests/test_pca_paths_gpu.py::kernel_path assumes two at
    least, which holds from R = 20 on)."""
    G = R * (R // 4)
    sstep = 1024 // G if G <= 1024 and 1024 % G == 0 else 1
    return -(-R // sstep)


@pytest.mark.parametrize("layout", ["czyx", "cxyz"])
@pytest.mark.parametrize("R", [32, 16])
@pytest.mark.parametrize("n", [1, 6, 15])
def test_small_batches(pkg, cus, n, R, layout):
    """n <= CUs / 2 frames: tsdf_split_kernel at R = 32; a 16^3 volume is ONE pass of the workgroup, so the plan does not
    split it and the same batches run on the fused kernel's static path — both against the reference."""
    assert kernel_path(n, R, cus) == "split"
    name = described(pkg, n, R, layout)
    if slice_rounds(R) >= 2:
        assert name.startswith(f"tsdf_split_kernel<{rt(R)}, {ar.LAYOUTS[layout]}, true, x"), name
    else:
        assert R == 16 and name == f"tsdf_fused_kernel<{rt(R)}, {ar.LAYOUTS[layout]}, true, false, 2>", name
    out, mgb = run_aug(pkg, n, R, layout)
    check_placement(mgb, list(range(n)), R)
    worst = check_frames(out, mgb, list(range(n)), R, layout)
    print(f"voxelize_aug small batch n={n} R={R} {layout}: {name}  max|kernel-ref| {worst:.3e}")


@pytest.mark.parametrize("R", [64, 48])
def test_split_kernel_large_grids(pkg, cus, R):
    ks = [mg.MAPS.index(m) for m in ("rx100", "general", "cyc")]
    depth, off, hdr, _, xf = _period()
    d, o, h = mg.take(depth, off, hdr, ks)
    assert kernel_path(3, R, cus) == "split"
    name = described(pkg, 3, R, "czyx")
    assert name.startswith(f"tsdf_split_kernel<{rt(R)}, 0, true, x"), name
    t = up(d, o, h, xf[ks])
    out = pkg.voxelize_aug(*t, res=R)
    mgb = pkg.map_grids(*t, res=R)
    torch.cuda.synchronize()
    assert not out.status.any()
    assert torch.equal(fbits(mgb.max_l), fbits(out.max_l)) and torch.equal(fbits(mgb.mid_p), fbits(out.mid_p))
    rows = check_placement(mgb, ks, R)
    vols = out.tsdf.cpu().numpy()
    worst = max(check_volume(vols[j], rows[j], k, R, "czyx") for j, k in enumerate(ks))
    print(f"voxelize_aug split n=3 R={R} czyx: {name}...  max|kernel-ref| {worst:.3e}")


def test_split_kernel_other_camera(pkg, cus):
    n, R, layout, cam = 15, 32, "czyx", "f300"
    assert kernel_path(n, R, cus) == "split"
    out, mgb = run_aug(pkg, n, R, layout, cam)
    check_placement(mgb, list(range(n)), R, cam)
    worst = check_frames(out, mgb, list(range(n)), R, layout, cam)
    # the camera matters: the default camera's volume of the same frames is another one
    other = pkg.voxelize_aug(*up(*[a for j, a in enumerate(tiled(n, cam)) if j != 3]), res=R)
    assert not torch.equal(fbits(other.tsdf), fbits(out.tsdf))
    print(f"voxelize_aug split n={n} R={R} {layout} camera f300: max|kernel-ref| {worst:.3e}")


# ---- voxelize_aug: the fused kernel ----
@pytest.mark.parametrize("R", [32, 48])
def test_fused_static_kernel(pkg, cus, R):
    n = n_for("static", R, cus, 132)
    name = described(pkg, n, R, "czyx")
    assert name == f"tsdf_fused_kernel<{rt(R)}, 0, true, false, {2 if R < 48 else 1}>", name
    out, mgb = run_aug(pkg, n, R, "czyx")
    check_periods(out, n)
    first, last = list(range(PERIOD)), list(range(n - PERIOD, n))
    check_placement(pkg.MapGridBatch(*[f[:PERIOD] for f in mgb]), first, R)
    worst = max(check_frames(out, mgb, first, R, "czyx"), check_frames(out, mgb, last, R, "czyx"))
    print(f"voxelize_aug fused static n={n} R={R}: {name}  max|kernel-ref| {worst:.3e}")


@pytest.mark.parametrize("R,want", [(16, 520), (48, 260)])
def test_fused_queue_kernel(pkg, cus, R, want):
    n = n_for("queue", R, cus, want)
    name = described(pkg, n, R, "czyx")
    assert name == f"tsdf_fused_kernel<{rt(R)}, 0, true, false, {2 if R < 48 else 1}>", name
    out, mgb = run_aug(pkg, n, R, "czyx")
    check_periods(out, n)
    first = list(range(PERIOD))
    check_placement(pkg.MapGridBatch(*[f[:PERIOD] for f in mgb]), first, R)
    worst = check_frames(out, mgb, first, R, "czyx")
    print(f"voxelize_aug fused queue n={n} R={R}: {name}  max|kernel-ref| {worst:.3e}")


# ---- the caller-supplied-grid passes ----
@pytest.mark.parametrize("layout", ["czyx", "cxyz"])
@pytest.mark.parametrize("R", [12, 32])
def test_aug_grid(pkg, R, layout):
    depth, off, hdr, names, xf = _period()
    t = up(depth, off, hdr, xf)
    mgb = pkg.map_grids(*t, res=R)
    tsdf, status = pkg.voxelize_aug_grid(*t, mgb.grid, res=R, layout=layout)
    torch.cuda.synchronize()
    assert not status.any()
    rows = check_placement(mgb, list(range(PERIOD)), R)
    vols = tsdf.cpu().numpy()
    worst = max(check_volume(vols[k], rows[k], k, R, layout) for k in range(PERIOD))
    print(f"voxelize_aug_grid R={R} {layout}: max|kernel-ref| {worst:.3e}")


# batch position -> source frame: every frame at least once, in another order, five of them twice
INDEX = [14, 3, 7, 0, 11, 3, 9, 1, 13, 5, 2, 8, 12, 4, 6, 10, 14, 0, 9, 9]


@pytest.mark.parametrize("dt", list(LOWP))
@pytest.mark.parametrize("layout", ["czyx", "cxyz"])
@pytest.mark.parametrize("R", [12, 32])
def test_map_grid_lowp(pkg, R, layout, dt):
    dtype, half = LOWP[dt]
    assert sorted(set(INDEX)) == list(range(PERIOD)) and len(INDEX) > PERIOD
    depth, off, hdr, names, xf = _period()
    td, to, th, tx, ti = up(depth, off, hdr, xf[INDEX], np.array(INDEX, np.int64))
    mgb = pkg.map_grids(td, to, th, tx, res=R, index=ti)
    tsdf, status = pkg.voxelize_map_grid_lowp(td, to, th, tx, mgb.grid, res=R, layout=layout, dtype=dtype, index=ti)
    torch.cuda.synchronize()
    assert tsdf.dtype is dtype and tsdf.shape == (len(INDEX), 3, R, R, R) and not status.any()
    rows = check_placement(mgb, INDEX, R)
    vols = tsdf.float().cpu().numpy()
    worst = max(check_volume(vols[j], rows[j], k, R, layout, extra=half) for j, k in enumerate(INDEX))
    # a repeated frame is the same volume
    assert torch.equal(tsdf[INDEX.index(9)].view(torch.int16), tsdf[-1].view(torch.int16))
    print(f"voxelize_map_grid_lowp {dt} R={R} {layout}: max|kernel-ref| {worst:.3e} (bound {TOL + half:.3e})")


# ---- labels ----
@pytest.mark.parametrize("J", [1, 21, 170])
def test_labels(pkg, J):
    """gt_aug of voxelize_aug(gt=) and transform_joints against T(joint) in longdouble within one float32 spacing, and the
    way back through invert_xforms.

    The round trip: y = fl32(A x + b) errs by at most half a float32 spacing of y, i.e. <= 2^-24 |y| per coordinate, and
    |y|_inf <= |A|_inf |x|_inf + |b|_inf; the way back multiplies that by A^-1 and rounds once more:
        |z - x|_inf <= 2^-24 (|A^-1|_inf (|A|_inf |x|_inf + |b|_inf) + |z|_inf) + r
    — cond_inf(A) |x| + |A^-1| |b| in units of the float32 rounding — where r collects what is not float32: the float64
    evaluation of both chains (<= 8 * 2^-53 times the same magnitudes) and the distance of the packed inverse rows from
    the true inverse, | A^-1 (A x + b) + b^-1 - x |, measured here in longdouble."""
    names = ["general", "mirror", "cyc"] * 2
    depth, off, hdr, _, xf = mg.case_batch(importlib.import_module(PKG + ".synth"), 6, names=names)
    rng = np.random.default_rng(900 + J)
    gt = rng.normal(0, 45, (6, J, 3))
    for i in range(6):
        gt[i, :, 2] -= float(depth[off[i]:off[i + 1]][depth[off[i]:off[i + 1]] != 0].mean())
    gt = gt.astype(np.float32).reshape(6, 3 * J)
    ref = mg.joints(gt, xf)
    bound = mg.joint_bound(gt, xf, ref)
    td, to, th, tx, tg = up(depth, off, hdr, xf, gt)
    out, gt_nor, gt_aug = pkg.voxelize_aug(td, to, th, tx, res=16, gt=tg)
    alone = pkg.transform_joints(tg, tx)
    back = pkg.transform_joints(alone, pkg.invert_xforms(tx))
    torch.cuda.synchronize()
    assert torch.equal(fbits(alone), fbits(gt_aug))
    got = alone.cpu().numpy()
    diff = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    assert (diff <= bound).all(), float((diff / bound).max())
    assert np.array_equal(got[2].reshape(J, 3), gt[2].reshape(J, 3)[:, [1, 2, 0]])          # cyc: exact
    # normalised labels: the project's own formula on the kernel's gt_aug and placement
    want_nor = oracle.normalize_joints(got, out.max_l.cpu().numpy(), out.mid_p.cpu().numpy())
    assert np.array_equal(gt_nor.cpu().numpy().view(np.uint32), want_nor.view(np.uint32))
    # the way back
    z = back.cpu().numpy().astype(np.float64).reshape(6, J, 3)
    x = gt.astype(np.float64).reshape(6, J, 3)
    worst = 0.0
    for i in range(6):
        f, inv = xf[i, :12].reshape(3, 4), xf[i, 12:].reshape(3, 4)
        nA, nAi = np.abs(f[:, :3]).sum(1).max(), np.abs(inv[:, :3]).sum(1).max()
        nx, nb, nz = np.abs(x[i]).max(), np.abs(f[:, 3]).max(), np.abs(z[i]).max()
        L = np.longdouble
        resid = (x[i].astype(L) @ f[:, :3].astype(L).T + f[:, 3].astype(L)) @ inv[:, :3].astype(L).T + inv[:, 3].astype(L) - x[i]
        r = float(np.abs(resid).max()) + 8 * 2.0 ** -53 * (nAi * (nA * nx + nb) + np.abs(inv[:, 3]).max())
        lim = 2.0 ** -24 * (nAi * (nA * nx + nb) + nz) + r
        d = float(np.abs(z[i] - x[i]).max())
        worst = max(worst, d / lim)
        assert d <= lim, (names[i], d, lim)
    print(f"labels J={J}: {int((diff > 0).sum())} of {diff.size} coordinates one spacing off, largest {diff.max():.3e} mm; "
          f"round trip at most {worst:.2f} of its bound")


# ---- exact relations to the identity volume ----
def _exact_inputs(name):
    depth, off, hdr, _, xf = mg.case_batch(importlib.import_module(PKG + ".synth"), 6, names=[name] * 6)
    return up(depth, off, hdr, xf)


def _check_scale(got, ident, s):
    assert torch.equal(fbits(got.max_l), fbits(ident.max_l * s)) and torch.equal(fbits(got.mid_p), fbits(ident.mid_p * s))


def _check_cycle(got_tsdf, ident_tsdf, name, layout):
    """|volume| under a cyclic map == the identity's magnitudes with channels and grid axes permuted, bit for bit."""
    for i in range(got_tsdf.shape[0]):
        want = mg.cyc_of_identity(ident_tsdf[i], name, layout).abs().contiguous()
        got = got_tsdf[i].abs()
        assert torch.equal(got.view(torch.int16 if got.element_size() == 2 else torch.int32),
                           want.view(torch.int16 if want.element_size() == 2 else torch.int32)), (name, i)
    assert bool((got_tsdf != mg.cyc_of_identity(ident_tsdf[0], name, layout)[None]).any())       # the signs do differ


@pytest.mark.parametrize("layout", ["czyx", "cxyz"])
@pytest.mark.parametrize("R", [32, 64])
def test_exact_relations_voxelize_aug(pkg, R, layout):
    ident = pkg.voxelize_aug(*_exact_inputs("identity"), res=R, layout=layout)
    assert not ident.status.any() and bool((ident.tsdf != 0).any())
    for name, s in mg.SCALES.items():
        got = pkg.voxelize_aug(*_exact_inputs(name), res=R, layout=layout)
        assert torch.equal(fbits(got.tsdf), fbits(ident.tsdf)), name
        _check_scale(got, ident, s)
    for name, sig in mg.CYCLES.items():
        got = pkg.voxelize_aug(*_exact_inputs(name), res=R, layout=layout)
        assert torch.equal(fbits(got.max_l), fbits(ident.max_l)), name
        assert torch.equal(fbits(got.mid_p), fbits(ident.mid_p[:, list(sig)])), name
        _check_cycle(got.tsdf, ident.tsdf, name, layout)


@pytest.mark.parametrize("layout", ["czyx", "cxyz"])
def test_exact_relations_grid_passes(pkg, layout):
    R = 32

    def passes(name):
        t = _exact_inputs(name)
        mgb = pkg.map_grids(*t, res=R)
        vols = {"f32": pkg.voxelize_aug_grid(*t, mgb.grid, res=R, layout=layout)[0]}
        for dt, (dtype, _) in LOWP.items():
            vols[dt] = pkg.voxelize_map_grid_lowp(*t, mgb.grid, res=R, layout=layout, dtype=dtype)[0]
        return mgb, vols

    imgb, ident = passes("identity")
    assert all(bool((v != 0).any()) for v in ident.values())
    for name, s in mg.SCALES.items():
        mgb, vols = passes(name)
        _check_scale(mgb, imgb, s)
        assert torch.equal(fbits(mgb.grid), fbits(imgb.grid * s)), name
        for dt, v in vols.items():
            assert torch.equal(v.view(torch.int16 if dt != "f32" else torch.int32),
                               ident[dt].view(torch.int16 if dt != "f32" else torch.int32)), (name, dt)
    for name, sig in mg.CYCLES.items():
        mgb, vols = passes(name)
        assert torch.equal(fbits(mgb.max_l), fbits(imgb.max_l)) and torch.equal(fbits(mgb.mid_p), fbits(imgb.mid_p[:, list(sig)]))
        assert torch.equal(fbits(mgb.grid[:, :3]), fbits(imgb.grid[:, list(sig)])), name
        assert torch.equal(fbits(mgb.grid[:, 3:]), fbits(imgb.grid[:, 3:])), name
        for dt, v in vols.items():
            _check_cycle(v, ident[dt], name, layout)
