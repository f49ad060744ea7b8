"""CPU tier of the accurate directional TSDF (include/tsdf_accurate.h): libtsdf_accurate.so as far as it goes without a GPU —
the build rule and its resource report, the binding through _lib._EXTS, the version, every argument check before device
work —, the public names, export.preprocess_tree(tsdf=...) through stubbed hooks, and the properties of the reference
the GPU tier compares against (tests/accurate_ref.py) on the very inputs that tier uses.  Nothing here touches a GPU."""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accurate_ref as ar  # noqa: E402
from abi_util import declared_functions, exported  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "handposeestimation-with-3d-cnns_amd"
CSRC = os.path.join(ROOT, PKG, "csrc")
INVALID, NO_DEVICE = -1, -2
WANT = ["tsdf_accurate_version", "tsdf_voxelize_grid_accurate_hip"]
NAN = float("nan")
GOOD_CAM = (241.42, 160.0, 120.0, 1.0, 3.0)
# a good call with dummy pointers would launch on them where there is a device: "valid arguments get as far as the device
# check" is asserted where that check answers -2; the refusals are asserted everywhere (they return before the device)
NO_GPU = not torch.cuda.is_available()


# ---- build rule ----
def _scratch_lines(text):
    return [ln for ln in text.splitlines() if "ScratchSize" in ln]


def test_make_rules_cross_compile_for_gfx950_without_scratch():
    r = subprocess.run(["make", "-C", CSRC, "accurate", "accurate-resources"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stdout + r.stderr
    names = [ln for ln in text.splitlines() if "Function Name" in ln]
    assert sum("tsdf_grid_accurate_kernel" in ln for ln in names) == 2 == len(names), names      # one per layout
    scratch = _scratch_lines(text)
    assert len(scratch) == 2 and all(ln.split("]:")[1].split()[0] == "0" for ln in scratch), scratch
    # the committed report says the same
    report = open(os.path.join(ROOT, "profiles", "accurate", "resources.txt")).read()
    assert sum("tsdf_grid_accurate_kernel" in ln for ln in report.splitlines() if "Function Name" in ln) == 2
    committed = _scratch_lines(report)
    assert len(committed) == 2 and all(ln.split("]:")[1].split()[0] == "0" for ln in committed), committed


def test_the_build_inputs_are_exact():
    lines = open(os.path.join(CSRC, "Makefile")).read().splitlines()
    deps, = [ln for ln in lines if re.match(r"^accurate_DEPS := ", ln)]
    assert deps.split(":=")[1].split() == ["prim.inc", "slab.inc", "search.inc"]
    src = open(os.path.join(CSRC, "tsdf_accurate.hip")).read()
    assert sorted(re.findall(r'#include "(\w+\.inc)"', src)) == sorted(["device.inc", "prim.inc", "slab.inc", "search.inc"])


def test_the_accurate_kernels_share_one_search_scaffold():
    read = lambda name: open(os.path.join(CSRC, name), errors="replace").read()   # noqa: E731
    inc, plain, mapped = read("search.inc"), read("tsdf_accurate.hip"), read("tsdf_mapaccurate.hip")
    defined = {"clip_lo": r"\bint clip_lo\(", "clip_hi": r"\bint clip_hi\(", "search_rect": r"\bSearchRect search_rect\(",
               "kMinBlocks": r"\bconstexpr int64_t kMinBlocks\b"}
    for name, pattern in defined.items():
        assert len(re.findall(pattern, inc)) == 1, name
        for text in (plain, mapped):
            assert not re.search(pattern, text), name
            assert not re.search(rf"\b(int|SearchRect|constexpr \w+) {name}\b", text), name   # nor defined in another form
    # both call the one rectangle, and neither restates its arithmetic (the reciprocals of the depth interval's ends)
    for text in (plain, mapped):
        assert len(re.findall(r"\bsearch_rect\(", text)) == 1 and "1.0 / dlo" not in text and "clip_lo(" not in text
    assert "1.0 / dlo" in inc
    # nothing else under csrc/ includes it
    users = sorted(f for f in os.listdir(CSRC) if f != "search.inc" and os.path.isfile(os.path.join(CSRC, f))
                   and re.search(r'#include\s+"search\.inc"', read(f)))
    assert users == ["tsdf_accurate.hip", "tsdf_mapaccurate.hip"]
    for text in (plain, mapped):                                     # after slab.inc, inside the anonymous namespace
        assert text.index("namespace {") < text.index('#include "slab.inc"') < text.index('#include "search.inc"') \
            < text.index("}  // namespace")


# ---- binding ----
def test_row_binds_exactly_its_header_with_types(pkg):
    assert not hasattr(pkg._lib, "_EXTS2")                      # one table: tests/test_ext_table_cpu.py pins all of it
    ext = pkg._lib._EXTS["accurate"]
    assert isinstance(ext, pkg._lib._Ext)
    assert declared_functions("tsdf_accurate.h") == WANT == sorted([ext.version_symbol, *ext.entries])
    funcs, named = exported(pkg._lib.ACCURATE_LIB_PATH)
    assert funcs == WANT and named == WANT
    assert ext.path == pkg._lib.ACCURATE_LIB_PATH and ext.version == pkg._lib.ACCURATE_VERSION == 1
    L = pkg._lib.load_accurate()
    assert L.tsdf_accurate_version() == 1
    for entry in (ext.version_symbol, *ext.entries):
        fn = getattr(L, entry)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, entry
    vp, i64, i, f64, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_float
    assert list(L.tsdf_voxelize_grid_accurate_hip.argtypes) == [vp, i64, vp, vp, i64, vp, i, i, f64, f64, f64, f32, f32, i, vp,
                                                                vp, vp, vp, vp]
    for name, args in ext.entries.items():
        assert list(getattr(L, name).argtypes) == args and args
    assert pkg._lib.load_accurate() is L and L is not pkg._lib.load() and L is not pkg._lib.load_lowp()
    # the header's own text: the camera comes by value, so nothing in it names the camera struct
    text = open(os.path.join(ROOT, "include", "tsdf_accurate.h")).read()
    assert "tsdf_cam" not in text and "#define TSDF_ACCURATE_VERSION 1" in text
    # the product beside it is what it was
    assert pkg._lib.load().tsdf_version() == 7


# ---- argument checks ----
def _caller(L):
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(72)

    def call(depth=one, depth_len=100, offsets=one, headers=one, n_src=1, index=null, n=1, R=32, cam=GOOD_CAM, layout=0,
             grid=one, out=one, nearest=one, status=one):
        return L.tsdf_voxelize_grid_accurate_hip(depth, depth_len, offsets, headers, n_src, index, n, R, *cam, layout, null,
                                                 grid, out, nearest, status)
    return call, null, one, odd


def test_argument_validation_happens_before_device_work(pkg):
    L = pkg._lib.load_accurate()
    call, null, one, odd = _caller(L)
    assert call(n=-1) == INVALID
    for name in ("depth", "offsets", "headers", "grid", "out"):
        assert call(**{name: null}) == INVALID, name
    assert call(depth_len=-1) == INVALID
    assert call(n_src=0, index=one) == INVALID and call(n_src=-3, index=one) == INVALID
    assert call(n_src=2) == INVALID and call(n=2) == INVALID          # no index: n_src must equal n
    for R in (0, 2, 3, 6, 30, 132, 256, -4):
        assert call(R=R) == INVALID, R
    for layout in (-1, 2):
        assert call(layout=layout) == INVALID
    assert call(n=0, n_src=0, R=30) == INVALID and call(n=0, n_src=0, layout=2) == INVALID   # judged before n == 0
    assert call(out=odd) == INVALID and call(nearest=odd) == INVALID   # 8-byte, not 16-byte aligned
    assert call(out=ctypes.c_void_p(68)) == INVALID and call(nearest=ctypes.c_void_p(68)) == INVALID
    # the camera comes by value and goes through the camera rule of every entry (csrc/prim.inc::cam_ok)
    for k in (0, 3, 4):
        for v in (0.0, -0.0, -1.0, NAN):
            bad = tuple(v if j == k else GOOD_CAM[j] for j in range(5))
            assert call(cam=bad) == INVALID, bad
            assert call(cam=bad, nearest=null, status=null) == INVALID, bad
            assert call(cam=bad, n=0, n_src=0) == 0, bad               # n == 0 is a no-op whatever the camera
    # more than 2^32 work-items: at R = 128 a position is 128 workgroups of 256 lanes
    big = 2 ** 31 - 1
    assert call(n=big, n_src=big, R=128) == INVALID
    assert call(n=2 ** 17, n_src=2 ** 17, R=128) == INVALID            # exactly 2^32
    if NO_GPU:   # valid arguments get as far as the device, and there is none here
        assert call() == NO_DEVICE
        assert call(status=null) == NO_DEVICE and call(nearest=null) == NO_DEVICE       # both are optional
        assert call(n_src=5, index=one, n=3) == NO_DEVICE
        assert call(n=2 ** 17 - 1, n_src=2 ** 17 - 1, R=128) == NO_DEVICE
        for R in (4, 12, 64, 128):
            assert call(R=R, layout=1) == NO_DEVICE, R
        for good in ((588.03, 320.5, 240.25, 0.5, 2.0), (241.42, NAN, -7.0, 1e-3, 8.0)):   # cx, cy are not judged
            assert call(cam=good) == NO_DEVICE, good


def test_n_zero_is_a_no_op_whatever_else_is_passed(pkg):
    L = pkg._lib.load_accurate()
    call, null, one, odd = _caller(L)
    assert call(n=0, n_src=0) == 0
    assert call(n=0, depth=null, depth_len=-5, out=odd, nearest=odd, cam=(NAN, NAN, NAN, -1.0, 0.0)) == 0
    assert L.tsdf_voxelize_grid_accurate_hip(null, 0, null, null, 0, null, 0, 32, 0.0, 0.0, 0.0, 0.0, 0.0, 0, null, null, null,
                                             null, null) == 0
    assert call(n=0, R=5) == INVALID and call(n=0, layout=7) == INVALID   # the shape is checked whatever n is, as in lowp


# ---- public names and refusals ----
def test_public_names_and_refusals(pkg, synth):
    for name in ("voxelize_grid_accurate", "voxelize_accurate"):
        assert name in pkg.__all__ and hasattr(pkg, name) and name in pkg.__doc__, name
    assert "tsdf_accurate.h" in pkg.__doc__ and 'tsdf="accurate"' in pkg.__doc__
    assert "tsdf_voxelize_grid_accurate_hip" in pkg.voxelize_grid_accurate.__doc__
    assert "accurate" in pkg.voxelize_frames.__doc__
    depth, off, hdr = (torch.from_numpy(x) for x in synth.synth_batch(2, "crop", seed0=3))
    grid = torch.zeros((2, 8))
    with pytest.raises(ValueError, match="GPU"):
        pkg.voxelize_grid_accurate(depth, off, hdr, grid)
    with pytest.raises(ValueError, match="GPU"):
        pkg.voxelize_accurate(depth, off, hdr)
    with pytest.raises(ValueError, match="layout"):
        pkg.voxelize_grid_accurate(depth, off, hdr, grid, layout="xyz")
    frames = torch.zeros((2, 30, 41))
    with pytest.raises(ValueError, match="tsdf"):
        pkg.voxelize_frames(frames, tsdf="exact")
    with pytest.raises(ValueError, match="GPU"):
        pkg.voxelize_frames(frames, tsdf="accurate")


# ---- export.preprocess_tree(tsdf=...) through stubbed hooks ----
def _files(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            out[os.path.relpath(os.path.join(dp, f), root)] = os.path.join(dp, f)
    return out


def _same(pa, pb):
    if not pa.endswith(".npz"):
        return open(pa, "rb").read() == open(pb, "rb").read()
    za, zb = np.load(pa), np.load(pb)
    return sorted(za.files) == sorted(zb.files) and all(
        za[k].dtype == zb[k].dtype and za[k].tobytes() == zb[k].tobytes() for k in za.files)


def test_preprocess_tree_tsdf_through_stubbed_hooks(pkg, synth, tmp_path, monkeypatch):
    export = importlib.import_module(PKG + ".export")
    db = str(tmp_path / "db")
    synth.synth_msra_tree(db, n_sub=1, n_ges=2, n_frames=2, seed=5)
    R, calls = 4, []

    def rows_of(pk):
        rows, max_l, mid_p = np.zeros((len(pk), 8), np.float32), np.zeros(len(pk), np.float32), np.zeros((len(pk), 3), np.float32)
        for i in range(len(pk)):
            h, d = pk.frame(i)
            nv, mn, mx = oracle.aabb(d, h)
            g, ori = oracle.glue(mn, mx, R)
            rows[i, :3], rows[i, 3], rows[i, 4] = ori, g[4], g[5]
            max_l[i], mid_p[i] = g[3], g[:3]
        return rows, max_l, mid_p

    def stub(name, accurate, cloud):
        def fn(pk, *rest):
            res, layout, device = rest[-3:]
            calls.append(name)
            assert res == R and (len(rest) == 4) == cloud
            rows, max_l, mid_p = rows_of(pk)
            if accurate:
                tsdf = ar.voxelize_grid_accurate_ref(pk.depth, pk.offsets, pk.headers, rows, R, layout)[0]
            else:
                tsdf = np.stack([oracle.voxels(pk.frame(i)[1], pk.frame(i)[0], rows[i, :3], rows[i, 3], rows[i, 4], R=R,
                                               layout=ar.LAYOUTS[layout]) for i in range(len(pk))])
            return tsdf, max_l, mid_p, np.zeros(len(pk), np.int32)
        return fn

    for name, acc, cloud in (("_default_voxelize", False, False), ("_default_voxelize_cloud", False, True),
                             ("_default_voxelize_accurate", True, False), ("_default_voxelize_cloud_accurate", True, True)):
        monkeypatch.setattr(export, name, stub(name, acc, cloud))
    kw = dict(res=R, points_num=100)
    out = {k: str(tmp_path / k) for k in ("today", "proj", "acc", "acc_cloud", "proj_cloud", "hook")}
    export.preprocess_tree(db, out["today"], rng=np.random.default_rng(7), **kw)                       # the call as it was
    export.preprocess_tree(db, out["proj"], rng=np.random.default_rng(7), tsdf="projective", **kw)
    assert calls == ["_default_voxelize"] * 4
    del calls[:]
    export.preprocess_tree(db, out["acc"], rng=np.random.default_rng(7), tsdf="accurate", **kw)
    assert calls == ["_default_voxelize_accurate"] * 2
    del calls[:]
    export.preprocess_tree(db, out["proj_cloud"], rng=np.random.default_rng(7), placement="cloud", **kw)
    export.preprocess_tree(db, out["acc_cloud"], rng=np.random.default_rng(7), placement="cloud", tsdf="accurate", **kw)
    assert calls == ["_default_voxelize_cloud"] * 2 + ["_default_voxelize_cloud_accurate"] * 2
    del calls[:]
    mine = stub("mine", False, False)
    export.preprocess_tree(db, out["hook"], rng=np.random.default_rng(7), tsdf="accurate", voxelize_fn=mine, **kw)
    assert calls == ["mine"] * 2                                     # a hook the caller passes is called as it is
    del calls[:]
    files = {k: _files(v) for k, v in out.items()}
    assert all(sorted(files[k]) == sorted(files["today"]) for k in files)
    assert all(_same(files["today"][k], files["proj"][k]) for k in files["today"])      # the default tree is unchanged
    assert all(_same(files["today"][k], files["hook"][k]) for k in files["today"])
    for a, p in (("acc", "today"), ("acc_cloud", "proj_cloud")):
        differ = 0
        for k in files[a]:
            if os.sep + "TSDF" + os.sep not in k:
                assert _same(files[a][k], files[p][k]), k            # clouds, labels, counts: byte for byte the same
                continue
            za, zp = np.load(files[a][k]), np.load(files[p][k])
            assert sorted(za.files) == sorted(zp.files)               # the schema the reference's train.py reads
            for f in za.files:
                assert za[f].dtype == zp[f].dtype and za[f].shape == zp[f].shape
                if f != "tsdf":
                    assert np.array_equal(za[f], zp[f]), (k, f)
            differ += int((za["tsdf"] != zp["tsdf"]).sum())
            assert not ((zp["tsdf"] != 0) & (np.abs(zp["tsdf"]) < 1) & (za["tsdf"] == 0)).any()
        assert differ > 0, a
    with pytest.raises(ValueError, match="accurate"):
        export.preprocess_tree(db, str(tmp_path / "x"), tsdf="accurate", aug=True, **kw)
    with pytest.raises(ValueError, match="tsdf"):
        export.preprocess_tree(db, str(tmp_path / "y"), tsdf="exact", **kw)
    assert not calls


# ---- the reference, on the inputs of the GPU tier ----
# (the dense ones; the sparse frames of tests/sparse_ref.py, whose grids and cameras are their own, have their reference's
# properties and both lists' search windows checked in tests/test_window_cpu.py)
CASES = ar.all_cases()


@pytest.mark.parametrize("label,kind,name,R,shifted", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_reference_properties_on_every_gpu_input(label, kind, name, R, shifted):
    c = ar.case(kind, name, R, shifted)
    r = c["ref"]
    vol, plain, near, nearest, pm = r["vol"], r["plain"], r["near"], r["nearest"], r["pixmap"]
    nvox = R ** 3
    # (a) the fragile set is within the cap (expected: empty)
    nfr = int(r["fragile"].sum())
    print(f"{label}: {nfr} fragile, {int(near.sum())} near of {nvox}")
    assert nfr <= ar.FRAGILE_CAP * nvox
    # (b) a far voxel equals the oracle's plain volume bit for bit, and names no pixel
    far = ~near
    assert np.array_equal(vol[:, far].view(np.uint32), plain[:, far].view(np.uint32))
    assert (nearest[far] == -1).all() and (nearest[near] >= 0).all()
    assert set(np.unique(np.abs(plain[:, far & ~r["fragile"]]))) <= {0.0, 1.0}
    # (c) a plain-near voxel is accurate-near and no farther from the surface; the same pixel gives the same values
    pnear = (pm >= 0) & (np.abs(plain) < 1).any(axis=0)
    assert near[pnear & ~r["fragile"]].all()                          # (the mixed-sign fixtures have no plain-near voxel)
    assert pnear.any() or name.startswith("mixed_")
    na, npl = np.linalg.norm(vol.astype(np.float64), axis=0), np.linalg.norm(plain.astype(np.float64), axis=0)
    assert (na[pnear] <= npl[pnear] + 1e-5).all()
    same = pnear & (nearest == pm)
    assert same.any() or name.startswith("mixed_")
    assert not same.any() or np.abs(vol[:, same] - plain[:, same]).max() <= 1e-5
    # (e) the case reaches the new ground: voxels the projective pass rejects although a point is within the distance
    new = int(((pm < 0) & near).sum())
    assert new > 0
    assert (vol[:, (pm < 0) & near] >= 0).all()                       # ... and they are positive: free space


def test_reference_on_a_crop_with_one_valid_pixel():
    # (d) every near voxel names the one pixel and the values are the closed form
    F, cx, cy = ar.DEFAULT_CAM[:3]
    left, top, bw, bh = 150, 100, 7, 5
    depth = np.zeros(bw * bh, np.float32)
    k = 2 * bw + 4
    depth[k] = np.float32(400.25)
    header = np.array([320, 240, left, top, left + bw, top + bh], np.int32)
    col, row, d = left + 4, top + 2, float(depth[k])
    w = np.array([(col - cx) * d / F, -(row - cy) * d / F, -d])
    R, vl = 8, np.float32(2.5)
    ori = (w - 3.3 * float(vl)).astype(np.float32)
    td = np.float32(7.5)
    r = ar.accurate_frame(depth, header, ori, vl, td, R)
    assert r["near"].any() and not r["near"].all() and not r["fragile"].any()
    assert (r["nearest"][r["near"]] == k).all() and (r["nearest"][~r["near"]] == -1).all()
    c = ar.centres(ori, vl, R)
    zz, yy, xx = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
    t = np.stack([c[0][xx] - w[0], c[1][yy] - w[1], c[2][zz] - w[2]]) / float(td)
    assert np.array_equal(r["near"], (t ** 2).sum(axis=0) <= 1.0)
    want = np.minimum(np.abs(t), 1.0).astype(np.float32)
    sign = np.where(np.signbit(r["plain"][0]) & (r["pixmap"] >= 0), -1.0, 1.0).astype(np.float32)
    assert np.abs(r["vol"][:, r["near"]] - (want * sign)[:, r["near"]]).max() <= 1e-6
    # no valid pixel at all: a zero volume, nothing near
    z = ar.accurate_frame(np.zeros(bw * bh, np.float32), header, ori, vl, td, R)
    assert not z["vol"].any() and (z["nearest"] == -1).all() and not z["fragile"].any()


def test_reference_status_rules_and_layouts():
    c = ar.case("golden", "small_odd", 8)
    depth, off, hdr, grid = c["depth"], c["off"], c["hdr"], c["grid"]
    d2 = np.concatenate([depth, depth])
    o2 = np.array([0, depth.size, 2 * depth.size], np.int64)
    h2, g2 = np.concatenate([hdr, hdr]), np.concatenate([grid, grid])
    g2[1, 4] = 0.0
    tsdf, st, nn, fr = ar.voxelize_grid_accurate_ref(d2, o2, h2, g2, 8, "czyx", index=[0, 1, 2, -1, 0])
    assert st.tolist() == [0, 1, 2, 2, 0] and not tsdf[1:4].any() and (nn[1:4] == -1).all()
    assert np.array_equal(tsdf[0], c["ref"]["vol"]) and np.array_equal(tsdf[4], tsdf[0]) and np.array_equal(nn[0], nn[4])
    t1, s1, n1, _ = ar.voxelize_grid_accurate_ref(depth, off, hdr, grid, 8, "cxyz")
    assert np.array_equal(t1[0], tsdf[0].transpose(0, 3, 2, 1)) and np.array_equal(n1[0], nn[0].transpose(2, 1, 0))
    _, s2, _, _ = ar.voxelize_grid_accurate_ref(depth, off, hdr, grid, 8, "czyx", depth_len=depth.size - 1)
    assert s2.tolist() == [2]
