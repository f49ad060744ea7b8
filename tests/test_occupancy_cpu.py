"""CPU tier of the occupancy volumes (include/tsdf_occupancy.h): the properties of the numpy restatement the GPU tier compares
with (tests/occupancy_ref.py) on that tier's own inputs, and libtsdf_occupancy.so as far as it goes without a GPU — the
loader's row against header and binary, the version, every argument refusal before device work, the plan, the build rule
and the resource report, the host-only code under the CPU sanitizers as a child process —, the public names and
refusals with launches stubbed, and AugmentedStep(occupancy=...) through stubbed primitives.  Nothing here touches a GPU."""
import ctypes
import importlib
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_geom_ref as mg  # noqa: E402
import occupancy_ref as orf  # noqa: E402
from abi_util import declared_functions, exported  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "handposeestimation-with-3d-cnns_amd"
CSRC = os.path.join(ROOT, PKG, "csrc")
INVALID, NO_DEVICE = -1, -2
WANT = ["tsdf_occupancy_hip", "tsdf_occupancy_plan", "tsdf_occupancy_version"]
OTHERS = ["augment", "augstep", "auggrid", "depth16", "obb", "lowp", "maplowp", "mapstep", "locate", "accurate", "mapaccurate",
          "heatmap", "heatloss"]


# ---- the reference, on the inputs of the GPU tier ----
@pytest.fixture(scope="module")
def inputs(synth):
    """name -> (pack, xforms or None, resolutions): the GPU tier's crops, zoo frames and mapped batch."""
    zp, _ = orf.zoo_pack()
    d, o, h, names, xf = mg.case_batch(synth, 15)
    return {"crops": (orf.crops(), None, (8, 32, 88, 128)), "zoo": (zp, None, (8, 16)), "maps": ((d, o, h), xf, (8, 32, 88))}


def test_the_cloud_s_own_cube_holds_every_point_and_the_skin_rule_is_what_keeps_the_outermost(inputs):
    lo = hi = 0
    for name, (pack, xf, resolutions) in inputs.items():
        max_l, mid_p = orf.placed(pack, xf)
        for R in resolutions:
            vol, status, rows = orf.batch(*pack, max_l, mid_p, R, xforms=xf)
            live = [r for r in rows if r.status == 0]
            assert len(live) >= len(rows) - 2 and all(r.status == 1 for r in rows if r.status)   # (the zoo's two empty frames)
            assert sum(r.outside for r in live) == 0, (name, R)
            assert all(r.vol.sum() >= 1 for r in live) and all(r.skin_lo + r.skin_hi <= 6 for r in live)
            lo += sum(r.skin_lo for r in live)
            hi += sum(r.skin_hi for r in live)
            # without the rule those pixels are lost, and nothing else changes
            _, _, bare = orf.batch(*pack, max_l, mid_p, R, xforms=xf, skin=False)
            assert [b.outside for b in bare] == [r.skin_lo + r.skin_hi for r in rows]
            print(f"{name} R={R}: skin low {sum(r.skin_lo for r in live)}, high {sum(r.skin_hi for r in live)}, outside 0")
    assert lo >= 1 and hi >= 1
    # half the cube: points are dropped
    pack, _, _ = inputs["crops"]
    max_l, mid_p = orf.placed(pack)
    _, _, rows = orf.batch(*pack, max_l / np.float32(2), mid_p, 32)
    assert all(r.outside > 100 and r.vol.sum() > 100 for r in rows)


def test_no_map_is_the_identity_map_and_a_permutation_or_reflection_moves_the_volume_exactly(inputs):
    pack, _, _ = inputs["crops"]
    n = len(pack[2])
    max_l, mid_p = orf.placed(pack)
    ident = np.tile(mg.pack(np.eye(3), np.zeros(3)), (n, 1))
    for R in (8, 32):
        for layout in orf.LAYOUTS:
            plain, _, _ = orf.batch(*pack, max_l, mid_p, R, layout)
            mapped, _, _ = orf.batch(*pack, max_l, mid_p, R, layout, xforms=ident)
            assert np.array_equal(plain, mapped) and plain.any()
    # T(p) = (p_y, p_z, p_x) and its square: the grid's centre is permuted with the points, the glue is per axis
    plain, _, _ = orf.batch(*pack, max_l, mid_p, 32)                       # [n, 1, z, y, x]
    for name, s in mg.CYCLES.items():
        xf = np.tile(mg.pack(mg.MATRICES[name], np.zeros(3)), (n, 1))
        got, _, _ = orf.batch(*pack, max_l, mid_p[:, list(s)], 32, xforms=xf)
        xyz = plain[:, 0].transpose(0, 3, 2, 1)                            # [n, x, y, z] of the camera frame
        want = xyz.transpose(0, 1 + s[0], 1 + s[1], 1 + s[2])              # mapped axis a runs along camera axis s[a]
        assert np.array_equal(got[:, 0].transpose(0, 3, 2, 1), want)
    # a reflection about a grid whose arithmetic is dyadic (max_l = 1024, R = 64: voxel_len 16, ori and iv exact), its
    # centre 4 mm off the optical axis so that the pixels of column cx and row cy (o = 0 exactly) lie on no voxel face
    big, mid = np.full(n, 1024, np.float32), np.tile(np.float32([4, 4, -508]), (n, 1))
    plain, _, rows = orf.batch(*pack, big, mid, 64)
    assert all(r.outside == 0 and r.vol.sum() > 50 for r in rows)       # (a hand of ~150 mm in 16 mm voxels)
    for axis in range(3):
        sign = np.ones(3)
        sign[axis] = -1.0
        xf = np.tile(mg.pack(np.diag(sign), np.zeros(3)), (n, 1))
        got, _, _ = orf.batch(*pack, big, mid * np.float32(sign), 64, xforms=xf)
        assert np.array_equal(got, np.flip(plain, axis=4 - axis))          # x is the last axis of czyx


def test_layouts_are_transposes_and_statuses_follow_the_header_and_the_row():
    pack = orf.crops()
    max_l, mid_p = orf.placed(pack)
    a, _, _ = orf.batch(*pack, max_l, mid_p, 12, "czyx")
    b, _, _ = orf.batch(*pack, max_l, mid_p, 12, "cxyz")
    assert np.array_equal(a.transpose(0, 1, 4, 3, 2), b)
    bad = max_l.copy()
    bad[:5] = [0, -1, np.nan, np.inf, 1e-45]
    mp = mid_p.copy()
    mp[5, 1] = np.nan
    vol, status, _ = orf.batch(*pack, bad, mp, 8)
    assert status.tolist() == [1] * 6 and not vol.any()
    vol, status, _ = orf.batch(*pack, max_l, mid_p, 8, index=[0, -1, 6, 2 ** 40, -2 ** 40, 5])
    assert status.tolist() == [0, 2, 2, 2, 2, 0] and vol[0].any() and vol[5].any() and not vol[1:5].any()


# ---- library pins ----
def test_row_binds_exactly_its_header_with_types(pkg):
    lib = pkg._lib
    ext = lib._OCCUPANCY
    assert isinstance(ext, lib._Ext) and "occupancy" not in lib._EXTS
    assert declared_functions("tsdf_occupancy.h") == WANT == sorted([ext.version_symbol, *ext.entries])
    funcs, named = exported(lib.OCCUPANCY_LIB_PATH)
    assert funcs == WANT and named == WANT
    assert ext.path == lib.OCCUPANCY_LIB_PATH and ext.version == lib.OCCUPANCY_VERSION == 1
    L = lib.load_occupancy()
    assert L.tsdf_occupancy_version() == 1
    vp, i, i64, f32, f64, ip = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.POINTER(ctypes.c_int)
    assert list(L.tsdf_occupancy_version.argtypes) == []
    assert list(L.tsdf_occupancy_plan.argtypes) == [i, i, ip, ip, ip]
    assert list(L.tsdf_occupancy_hip.argtypes) == [vp, i64, vp, vp, i64, vp, i, i, f64, f64, f64, f32, f32, i, i, i, vp, vp, vp,
                                                   vp, vp, vp]
    for name in (ext.version_symbol, *ext.entries):
        assert getattr(L, name).restype is ctypes.c_int
    assert lib.load_occupancy() is L and L is not lib.load()
    assert all(L is not getattr(lib, "load_" + other)() for other in OTHERS)
    # the camera comes by value: the header names no camera struct (tests/test_camera_cpu.py pins who does)
    text = open(os.path.join(ROOT, "include", "tsdf_occupancy.h")).read()
    assert "tsdf_cam" not in text and "#define TSDF_OCCUPANCY_VERSION 1" in text
    assert "commutative and idempotent" in text and "skin rule" in text
    assert lib.load().tsdf_version() == 7 and lib.load_heatmap().tsdf_heatmap_version() == 1


def test_wrong_version_and_missing_library_raise_import_error(pkg, monkeypatch):
    lib = pkg._lib
    row = lib._OCCUPANCY
    monkeypatch.delitem(lib._ext_libs, "occupancy", raising=False)
    monkeypatch.setattr(lib, "_OCCUPANCY", row._replace(version=row.version + 1))
    with pytest.raises(ImportError, match="version 1.*csrc occupancy"):
        lib.load_occupancy()
    monkeypatch.setattr(lib, "_OCCUPANCY", row._replace(path=os.path.join(ROOT, "build", "no_such_libtsdf_occupancy.so")))
    with pytest.raises(ImportError, match="csrc occupancy"):
        lib.load_occupancy()


# ---- build pins ----
def test_makefile_builds_it_outside_the_pinned_table():
    src = open(os.path.join(CSRC, "Makefile")).read()
    lines = src.splitlines()
    assert "occupancy_DEPS := prim.inc narrow.inc occupancy_host.inc ../../include/tsdf_heatmap.h ../../include/tsdf_lowp.h" in lines
    assert "$(eval $(call EXT_RULES,occupancy))" in lines
    (all_line,) = [ln for ln in lines if ln.startswith("all:")]
    (phony,) = [ln for ln in lines if ln.startswith(".PHONY:")]
    assert "occupancy" in all_line.split() and {"occupancy", "occupancy-resources", "occupancy-host-asan"} <= set(phony.split())
    assert "../libtsdf_occupancy.so" in lines[lines.index("clean:") + 1].split()
    assert "occupancy_host.inc" in src.split("$(filter-out", 1)[1].split(",", 1)[0].split()   # not a part of the product
    (exts,) = [ln for ln in lines if re.match(r"^EXTS := ", ln)]
    assert exts.split(":=")[1].split() == OTHERS[:11]


def test_make_rules_cross_compile_for_gfx950_without_scratch():
    r = subprocess.run(["make", "-C", CSRC, "occupancy", "occupancy-resources"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stdout + r.stderr
    assert "tsdf_occupancy_kernel" in text
    scratch = [ln for ln in text.splitlines() if "ScratchSize" in ln]
    # 2 layouts x 3 element types x (mapped, not mapped)
    assert len(scratch) == 12 and all(ln.split("]:")[1].split()[0] == "0" for ln in scratch), scratch
    vgprs = [int(ln.split("VGPRs:")[1].split()[0]) for ln in text.splitlines() if " VGPRs:" in ln]
    assert len(vgprs) == 12 and max(vgprs) <= 128          # two workgroups of 512 lanes a CU
    unit = open(os.path.join(CSRC, "tsdf_occupancy.hip")).read()
    assert sorted(re.findall(r'#include "(\w+\.inc)"', unit)) == ["device.inc", "narrow.inc", "occupancy_host.inc", "prim.inc"]
    body = unit.split("namespace {", 1)[1]
    assert body.count("atomicOr(") == 1 and "atomicOr(&mask[" in body and "extern __shared__ unsigned s_mask[]" in body
    assert body.count("f, s_mask);") == 5                              # the one atomic is on LDS: every call passes the mask
    assert not re.search(r"atomic(Add|Max|Min|CAS|Exch|And|Xor)", body) and "__device__ int" not in unit   # no device globals
    assert "__builtin_fma" not in unit and "fma(" not in body
    recorded = open(os.path.join(ROOT, "profiles", "occupancy", "resources.txt")).read()
    assert recorded.count("ScratchSize [bytes/lane]: 0") == 12 and f"VGPRs: {max(vgprs)}" in recorded


def test_the_library_includes_the_same_text():
    unit = open(os.path.join(CSRC, "tsdf_occupancy.hip")).read()
    inc, main = (open(os.path.join(CSRC, f)).read() for f in ("occupancy_host.inc", "occupancy_host_main.cc"))
    theirs = open(os.path.join(CSRC, "device.inc")).read().splitlines() + open(os.path.join(CSRC, "narrow.inc")).read().splitlines()
    for name in ("bad_res", "misaligned", "bad_dtype"):
        (line,) = [ln for ln in main.splitlines() if re.search(rf"\bbool {name}\(", ln)]
        assert line in theirs, name
        assert f"{name}(" in inc and not re.search(rf"\bbool {name}\(", inc), name            # used, not restated
    assert "cam_ok(" in inc and "bool cam_ok" not in inc and "bool cam_ok" not in main and '#include "prim.inc"' in main
    order = [unit.index(f'#include "{f}"') for f in ("device.inc", "prim.inc", "narrow.inc", "occupancy_host.inc")]
    assert order == sorted(order) and "occ_defect(" in unit and "occ_plan(" in unit


def test_host_code_under_sanitizers_as_a_stand_alone_program():
    subprocess.check_call(["make", "-C", CSRC, "-B", "occupancy-host-asan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "build", "occupancy_host_asan")
    env = dict(os.environ)
    env.update(ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "occupancy host code ok (2272 plans)" in r.stdout, tail     # sum over the 32 resolutions of R + 3 hints, and 2 more
    assert "Sanitizer" not in tail and "runtime error" not in tail and "FAILED" not in tail, tail


# ---- the plan ----
def test_plan_tiles_every_resolution_under_the_cap(pkg):
    L = pkg._lib.load_occupancy()
    cap = pkg._lib.OCCUPANCY_LDS_CAP
    assert cap == orf.LDS_CAP == 65536
    slab, nslab, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert len(orf.RESOLUTIONS) == 32
    for R in orf.RESOLUTIONS:
        for hint in (0, 1, 3, R, 1000):
            assert L.tsdf_occupancy_plan(R, hint, slab, nslab, lds) == 0
            s, ns, b = slab.value, nslab.value, lds.value
            assert (s, ns, b) == orf.plan(R, hint), (R, hint)
            assert 1 <= s <= R and (ns - 1) * s < R <= ns * s                      # the slabs tile [0, R), none empty
            assert b == 4 * -(-s * R * R // 32) and b <= cap
            if hint:
                assert s == min(hint, R, cap * 8 // (R * R))
        whole = orf.plan(R)
        assert (whole[1] == 1) == (R <= 80) and whole[1] == -(-R // min(R, cap * 8 // (R * R)))   # the fewest the cap allows
    assert orf.plan(88)[:2] == (44, 2) and orf.plan(128) == (32, 4, cap) and orf.plan(8, 3)[:2] == (3, 3)
    for bad in ((0, 0), (30, 0), (132, 0), (-4, 0), (32, -1)):
        assert L.tsdf_occupancy_plan(*bad, slab, nslab, lds) == INVALID
    assert L.tsdf_occupancy_plan(32, 0, None, nslab, lds) == INVALID


# ---- refusals ----
null, one, odd8, odd4 = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(72), ctypes.c_void_p(68)
nan, inf = float("nan"), float("inf")


def _entry(pkg):
    """The entry on dummy pointers (64: aligned for every check), every argument good unless named."""
    L = pkg._lib.load_occupancy()

    def occ(depth=one, depth_len=100, offsets=one, headers=one, n_src=3, index=one, n=3, R=32, focal=241.42, cx=160.0, cy=120.0,
            eps=1.0, trunc=3.0, layout=0, dtype=0, slab=0, xforms=one, max_l=one, mid_p=one, out=one, status=one):
        return L.tsdf_occupancy_hip(depth, depth_len, offsets, headers, n_src, index, n, R, focal, cx, cy, eps, trunc, layout,
                                    dtype, slab, null, xforms, max_l, mid_p, out, status)
    return occ


FIRST = [dict(n=-1), *[dict(R=R) for R in (0, 2, 3, 6, 30, 132, 256, -4)], dict(layout=2), dict(layout=-1), dict(dtype=3),
         dict(dtype=-1), dict(slab=-1), dict(slab=-2 ** 31)]                       # refused whatever n is
LATER = [dict(depth=null), dict(offsets=null), dict(headers=null), dict(max_l=null), dict(mid_p=null), dict(out=null),
         dict(depth_len=-1), dict(n_src=0), dict(n_src=-5), dict(index=null, n_src=4), dict(index=null, n_src=2),
         dict(xforms=odd4), dict(out=odd8), dict(out=odd4),
         *[dict([(k, v)]) for k in ("focal", "eps", "trunc") for v in (0.0, -0.0, -1.0, nan, -inf)],
         dict(n=2 ** 23), dict(n=2 ** 21, R=128), dict(n=2 ** 16, R=128, slab=1)]  # ... with n > 0; n == 0 is a no-op


def test_every_defect_is_refused_before_device_work(pkg):
    occ = _entry(pkg)
    for kw in FIRST:
        assert occ(**kw) == INVALID, kw
        if "n" not in kw:
            assert occ(n=0, **kw) == INVALID, kw
    for kw in LATER:
        assert occ(**kw) == INVALID, kw
        if "n" not in kw:
            assert occ(n=0, **kw) == 0, kw
    assert occ(n=0) == 0 and occ(n=0, index=null, n_src=7) == 0
    L = pkg._lib.load_occupancy()
    assert L.tsdf_occupancy_hip(null, -1, null, null, 0, null, 0, 32, nan, nan, nan, nan, nan, 1, 2, 5, null, null, null, null,
                                null, null) == 0


# Good arguments reach check_device.  On a machine WITH a device they would launch on the dummy pointers, so this row is
# checked where the device check answers -2.
@pytest.mark.skipif(torch.cuda.is_available(), reason="good arguments with dummy pointers must stop at the device check")
def test_good_arguments_get_as_far_as_the_device(pkg):
    occ = _entry(pkg)
    assert occ() == NO_DEVICE
    for R in (4, 12, 88, 128):
        for dtype in (0, 1, 2):
            for layout in (0, 1):
                assert occ(R=R, dtype=dtype, layout=layout) == NO_DEVICE
    assert occ(xforms=null) == NO_DEVICE and occ(status=null) == NO_DEVICE and occ(index=null) == NO_DEVICE
    assert occ(out=ctypes.c_void_p(80), xforms=ctypes.c_void_p(72)) == NO_DEVICE
    assert occ(n=2 ** 23 - 1) == NO_DEVICE and occ(n=2 ** 21 - 1, R=128) == NO_DEVICE and occ(slab=1000) == NO_DEVICE
    assert occ(depth_len=0) == NO_DEVICE and occ(cx=nan, cy=-inf) == NO_DEVICE          # the camera rule is cam_ok's
    P = pkg._lib.load()
    for R in range(-8, 264):
        assert (occ(R=R) == INVALID) == (not P.tsdf_resolution_supported(R)), R


# ---- Python wrappers ----
@pytest.fixture()
def V():
    return importlib.import_module(PKG + ".voxelize")


def test_public_names_and_refusals(pkg, V, monkeypatch):
    log = []
    monkeypatch.setattr(V, "_call", lambda *a, **kw: log.append(a))
    for name in ("occupancy_volumes", "voxelize_occupancy"):
        assert name in pkg.__all__ and hasattr(pkg, name) and name in pkg.__doc__, name
    assert "tsdf_occupancy.h" in pkg.__doc__ and "libtsdf_occupancy.so" in pkg.__doc__ and "AugmentedStep(occupancy=" in pkg.__doc__
    assert list(inspect.signature(pkg.occupancy_volumes).parameters) == [
        "depth", "offsets", "headers", "max_l", "mid_p", "res", "layout", "dtype", "cam", "xforms", "index", "out", "slab"]
    assert list(inspect.signature(pkg.voxelize_occupancy).parameters) == [
        "depth", "offsets", "headers", "res", "layout", "dtype", "cam", "xforms"]
    params = list(inspect.signature(pkg.AugmentedStep.__init__).parameters)
    assert params[-2:] == ["occupancy", "tsdf"] and inspect.signature(pkg.AugmentedStep.__init__).parameters["occupancy"].default is None
    pack = torch.rand(30), torch.tensor([0, 10, 20, 30]), torch.zeros((3, 6), dtype=torch.int32)
    max_l, mid_p = torch.rand(3), torch.rand(3, 3)
    # there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        pkg.occupancy_volumes(*pack, max_l, mid_p)
    with pytest.raises(ValueError, match="GPU"):
        pkg.voxelize_occupancy(*pack)
    # everything else, with the device check out of the way: judged before the launch
    monkeypatch.setattr(V, "_dev_check", lambda name, t, dtype, device=None, host_ok=False: V_dev_check(name, t, dtype))
    for fn in (lambda **kw: pkg.occupancy_volumes(*pack, max_l, mid_p, **kw), lambda **kw: pkg.voxelize_occupancy(*pack, **kw)):
        for bad in (0, 30, 132, 31.5, "x", None):
            with pytest.raises(ValueError, match="resolution"):
                fn(res=bad)
        with pytest.raises(ValueError, match="layout"):
            fn(layout="xyzc")
        for bad in (torch.float64, torch.int8, "float32", None):
            with pytest.raises(ValueError, match="float32, torch.float16 or torch.bfloat16"):
                fn(dtype=bad)
    for bad in (-1, 1.0, True, "2", None, 2 ** 31):
        with pytest.raises(ValueError, match="slab"):
            pkg.occupancy_volumes(*pack, max_l, mid_p, slab=bad)
    shapes = [dict(max_l=torch.rand(4)), dict(mid_p=torch.rand(3, 2)), dict(mid_p=torch.rand(9)), dict(max_l=max_l.double()),
              dict(xforms=torch.rand(3, 24)), dict(xforms=torch.rand((3, 12), dtype=torch.float64)),
              dict(out=torch.zeros((3, 3, 32, 32, 32))), dict(out=torch.zeros((3, 1, 32, 32, 32), dtype=torch.float16)),
              dict(index=torch.tensor([0, 1])), dict(index=torch.tensor([[0, 1, 2]])), dict(index=torch.tensor([0, 1, 2], dtype=torch.int32))]
    for kw in shapes:
        args = dict(max_l=max_l, mid_p=mid_p)
        args.update(kw)
        with pytest.raises(ValueError):
            pkg.occupancy_volumes(*pack, **args)
    for bad in (pack[0].double(), pack[0].numpy(), None):                # not a float32 tensor: a ValueError all the same
        with pytest.raises(ValueError):
            pkg.occupancy_volumes(bad, pack[1], pack[2], max_l, mid_p)
    assert log == []                                                    # refused before anything is launched
    # and a good call is one launch of the entry, the stream at position 16
    occ, status = pkg.occupancy_volumes(*pack, max_l, mid_p, res=8, layout="cxyz", dtype=torch.bfloat16, slab=3)
    (dev, fn, args, stream_at), = log
    assert fn.__name__ == "tsdf_occupancy_hip" and stream_at == 16 and len(args) == 22 and args[16] is None
    assert args[4:8] == [3, None, 3, 8] and args[8:13] == [241.42, 160.0, 120.0, 1.0, 3.0] and args[13:16] == [1, 2, 3]
    assert args[17] is None and args[18] == max_l.data_ptr() and args[19] == mid_p.data_ptr() and args[20] == occ.data_ptr()
    assert occ.shape == (3, 1, 8, 8, 8) and occ.dtype is torch.bfloat16 and status.dtype is torch.int32 and args[21] == status.data_ptr()


def V_dev_check(name, t, dtype):
    """``_dev_check`` without "lives on the GPU": the rest of it is under test."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def test_voxelize_occupancy_places_then_bins(pkg, V, monkeypatch):
    N = 3
    log = []
    place = V.MapGridBatch(None, torch.rand(N), torch.rand(N, 3), torch.tensor([0, 1, 0], dtype=torch.int32))

    def stub(name, ret):
        def fn(*a, **kw):
            log.append((name, a, kw))
            return ret(*a, **kw)
        return fn
    monkeypatch.setattr(V, "_place_aabb", stub("_place_aabb", lambda *a, **kw: place))
    monkeypatch.setattr(V, "map_grids", stub("map_grids", lambda *a, **kw: place._replace(grid=torch.rand(N, 8))))
    monkeypatch.setattr(V, "_occupancy", stub("_occupancy", lambda *a, **kw: (torch.zeros((N, 1, 8, 8, 8)), None)))
    pack = torch.rand(30), torch.tensor([0, 10, 20, 30]), torch.zeros((N, 6), dtype=torch.int32)
    cam = pkg._lib.TsdfCam()
    xf = torch.rand((N, 24), dtype=torch.float64)
    for xforms, first in ((None, "_place_aabb"), (xf, "map_grids")):
        del log[:]
        out = pkg.voxelize_occupancy(*pack, res=8, layout="cxyz", dtype=torch.float16, cam=cam, xforms=xforms)
        assert [e[0] for e in log] == [first, "_occupancy"]
        _, a, kw = log[1]
        assert all(x is y for x, y in zip(a[:3], pack)) and a[3] is place.max_l and a[4] is place.mid_p
        assert a[5:] == (8, "cxyz", torch.float16, cam, xforms, None, None, 0, False)
        assert isinstance(out, V.TsdfBatch) and out.max_l is place.max_l and out.mid_p is place.mid_p and out.status is place.status
        assert out.tsdf.shape == (N, 1, 8, 8, 8)
        if xforms is None:
            assert log[0][2].get("rows", log[0][1][-1]) is False


# ---- AugmentedStep(occupancy=...) through stubbed primitives ----
N, R8 = 3, 8
BF16 = torch.bfloat16
STUBBED = ("aug_xforms_at", "map_step_head", "voxelize_indexed", "map_grids", "_map_grid_lowp", "_map_grid_accurate",
           "narrow_volumes", "transform_joints", "normalize_joints", "joint_heatmaps", "aabb", "_occupancy")


class Rec:
    """Recorders in the style of tests/test_mapaccurate_cpu.py: ``log`` holds (name, arguments by parameter name) of every
    primitive call; every stub returns the ``out`` it was given."""

    def __init__(self, V, monkeypatch):
        self.log = []
        for name in STUBBED:
            monkeypatch.setattr(V, name, self._stub(name, getattr(V, name)))
        monkeypatch.setattr(V, "_dev_check", lambda *a, **kw: None)    # ("on the GPU": the check is not under test)
        monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)

    def _stub(self, name, real):
        sig = inspect.signature(real)

        def fn(*a, **kw):
            b = sig.bind(*a, **kw)
            b.apply_defaults()
            self.log.append((name, dict(b.arguments)))
            out = b.arguments.get("out")
            return (out, None) if name in ("_map_grid_lowp", "_occupancy") else (out, None, None) if name == "_map_grid_accurate" else out
        fn.__name__ = name
        return fn

    def names(self):
        return [e[0] for e in self.log]


LABELS = ["transform_joints", "normalize_joints"]
# what the step launches without occupancy=, configuration by configuration (AugmentedStep's docstring, option by option)
CONFIGS = {
    "plain": (dict(), ["aug_xforms_at", "voxelize_indexed"]),
    "plain_gt": (dict(gt=True), ["aug_xforms_at", "voxelize_indexed"]),
    "dtype": (dict(dtype=BF16), ["aug_xforms_at", "map_grids", "_map_grid_lowp"]),
    "dtype_gt": (dict(dtype=BF16, gt=True), ["aug_xforms_at", "map_grids", "_map_grid_lowp"] + LABELS),
    "head": (dict(fused_head=True, gt=True), ["map_step_head", "voxelize_indexed"]),
    "base_dtype": (dict(base=True, dtype=torch.float16, gt=True), ["map_step_head", "_map_grid_lowp"]),
    "accurate": (dict(tsdf="accurate"), ["aug_xforms_at", "map_grids", "_map_grid_accurate"]),
    "accurate_dtype_gt": (dict(tsdf="accurate", dtype=BF16, gt=True),
                          ["aug_xforms_at", "map_grids", "_map_grid_accurate", "narrow_volumes"] + LABELS),
    "heatmap": (dict(gt=True, heatmap=(12, 1.7)), ["aug_xforms_at", "voxelize_indexed", "joint_heatmaps"]),
    "head_dtype_heatmap": (dict(fused_head=True, dtype=BF16, gt=True, heatmap=(8, 1.0, BF16)),
                           ["map_step_head", "_map_grid_lowp", "joint_heatmaps"]),
}


def _step(V, kw, **more):
    kw = dict(kw)
    if kw.get("gt"):
        kw["gt"] = torch.rand(N, 21, 3)
    if kw.get("base"):
        kw["base"] = torch.rand((N, 24), dtype=torch.float64)
    pack = torch.rand(30), torch.tensor([0, 10, 20, 30]), torch.zeros((N, 6), dtype=torch.int32)
    return V.AugmentedStep(*pack, N, centres=torch.rand(N, 3), res=R8, layout="cxyz", graph=False, **kw, **more), pack


@pytest.mark.parametrize("name", list(CONFIGS))
def test_augmented_step_adds_exactly_one_launch_at_the_end(V, monkeypatch, name):
    kw, want = CONFIGS[name]
    rec = Rec(V, monkeypatch)
    s, _ = _step(V, kw)
    assert rec.names() == want and s.occ is None                       # occupancy=None: the launches there were
    del rec.log[:]
    s, _ = _step(V, kw, occupancy=None)
    assert rec.names() == want
    for occupancy, dtype in (((88,), torch.float32), ((12, BF16), BF16), ([4, torch.float16], torch.float16)):
        del rec.log[:]
        cam = None
        s, pack = _step(V, kw, occupancy=occupancy)
        assert rec.names() == want + ["_occupancy"]                    # one more, and it is the last
        a = rec.log[-1][1]
        assert all(a[k] is t for k, t in zip(("depth", "offsets", "headers"), pack))
        assert a["max_l"] is s.out.max_l and a["mid_p"] is s.out.mid_p and a["xforms"] is s.xforms and a["index"] is s.index
        assert a["out"] is s.occ and s.occ.shape == (N, 1, occupancy[0], occupancy[0], occupancy[0]) and s.occ.dtype is dtype
        assert (a["res"], a["layout"], a["dtype"], a["cam"], a["slab"], a["want_status"]) == (occupancy[0], "cxyz", dtype, cam, 0, False)
        del rec.log[:]
        s._run()                                                       # what a step without a graph issues
        assert rec.names() == want + ["_occupancy"] and rec.log[-1][1]["out"] is s.occ


def test_augmented_step_refuses_a_bad_occupancy_before_anything(V, monkeypatch):
    rec = Rec(V, monkeypatch)
    for bad, what in (((), "occupancy must be"), (88, "occupancy must be"), ((88, BF16, 1), "occupancy must be"),
                      ((30,), "resolution"), ((None,), "resolution"), ((88, torch.int8), "float32, torch.float16 or torch.bfloat16"),
                      ((88, "bfloat16"), "float32, torch.float16 or torch.bfloat16")):
        with pytest.raises(ValueError, match=what):
            _step(V, {}, occupancy=bad)
    assert rec.log == []
