"""CPU tier of the accurate directional TSDF under a per-frame map (include/tsdf_mapaccurate.h): libtsdf_mapaccurate.so as far
as it goes without a GPU — its build rule and resource report, what of its row in _lib._EXTS is its own (the table's every
row is pinned in tests/test_ext_table_cpu.py), the version, every argument check before device work —, the public names,
the ``tsdf=`` keyword of the composed entries through stubbed primitives, and the properties of the reference the GPU tier compares against (tests/mapaccurate_ref.py)
on the very inputs that tier uses.  Nothing here touches a GPU."""
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
import accurate_ref as ar  # noqa: E402
import map_geom_ref as mg  # noqa: E402
import mapaccurate_ref as mr  # noqa: E402
from abi_util import declared_functions, exported  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "handposeestimation-with-3d-cnns_amd"
CSRC = os.path.join(ROOT, PKG, "csrc")
INVALID, NO_DEVICE = -1, -2
WANT = ["tsdf_mapaccurate_version", "tsdf_voxelize_map_grid_accurate_hip"]
NAN = float("nan")
GOOD_CAM = (241.42, 160.0, 120.0, 1.0, 3.0)
NO_GPU = not torch.cuda.is_available()


# ---- build rule ----
def _scratch_lines(text):
    return [ln for ln in text.splitlines() if "ScratchSize" in ln]


def test_make_rules_cross_compile_for_gfx950_without_scratch():
    r = subprocess.run(["make", "-C", CSRC, "mapaccurate", "mapaccurate-resources"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stdout + r.stderr
    names = [ln for ln in text.splitlines() if "Function Name" in ln]
    assert sum("tsdf_map_grid_accurate_kernel" in ln for ln in names) == 2 == len(names), names      # one per layout
    scratch = _scratch_lines(text)
    assert len(scratch) == 2 and all(ln.split("]:")[1].split()[0] == "0" for ln in scratch), scratch
    # the committed report says the same
    report = open(os.path.join(ROOT, "profiles", "mapaccurate", "resources.txt")).read()
    assert sum("tsdf_map_grid_accurate_kernel" in ln for ln in report.splitlines() if "Function Name" in ln) == 2
    committed = _scratch_lines(report)
    assert len(committed) == 2 and all(ln.split("]:")[1].split()[0] == "0" for ln in committed), committed


def test_the_build_rule_is_the_tables_and_its_inputs_are_exact():
    lines = open(os.path.join(CSRC, "Makefile")).read().splitlines()
    exts, = [ln for ln in lines if re.match(r"^EXTS := ", ln)]
    assert exts.split(":=")[1].split().count("mapaccurate") == 1       # a name on the line: the table's macro builds it
    assert "$(foreach e,$(EXTS),$(eval $(call EXT_RULES,$(e))))" in lines
    assert not [ln for ln in lines if "EXT_RULES,mapaccurate" in ln]   # ... and nothing calls it once more
    deps, = [ln for ln in lines if re.match(r"^mapaccurate_DEPS := ", ln)]
    assert deps.split(":=")[1].split() == ["prim.inc", "slab.inc", "search.inc", "mapvox.inc"]
    src = open(os.path.join(CSRC, "tsdf_mapaccurate.hip")).read()
    assert sorted(re.findall(r'#include "(\w+\.inc)"', src)) == sorted(["device.inc", "prim.inc", "slab.inc", "search.inc",
                                                                       "mapvox.inc"])
    # all, clean and .PHONY reach the library through $(EXTS) and its derived lists; none names it by hand
    rule = {ln.split(":")[0]: ln for ln in lines if re.match(r"^(all|\.PHONY):", ln)}
    assert "$(EXTS)" in rule["all"].split()
    for t in ("$(EXTS)", "$(EXT_RES)", "$(EXT_ASM)"):
        assert t in rule[".PHONY"].split(), t
    clean = lines[lines.index("clean:") + 1]
    assert "$(EXTS:%=../libtsdf_%.so)" in clean.split()
    assert "EXT_RES := $(addsuffix -resources,$(EXTS))" in lines and "EXT_ASM := $(addsuffix -asm,$(EXTS))" in lines
    assert not [ln for ln in (rule["all"], rule[".PHONY"], clean) if "mapaccurate" in ln]


# ---- binding: what is this library's own (every row's shape, loader and refusals: tests/test_ext_table_cpu.py) ----
def test_the_rows_literal_names_and_argument_types(pkg):
    lib = pkg._lib
    assert [name for name, row in lib._EXTS.items() if row.path == lib.MAPACCURATE_LIB_PATH] == ["mapaccurate"]
    ext = lib._EXTS["mapaccurate"]
    assert declared_functions("tsdf_mapaccurate.h") == WANT == sorted([ext.version_symbol, *ext.entries])
    funcs, named = exported(lib.MAPACCURATE_LIB_PATH)
    assert funcs == WANT and named == WANT
    assert ext.version == lib.MAPACCURATE_VERSION == 1
    L = lib.load_mapaccurate()
    assert L.tsdf_mapaccurate_version() == 1 and lib._ext_libs["mapaccurate"] is L
    vp, i64, i, f64, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_float
    assert list(L.tsdf_voxelize_map_grid_accurate_hip.argtypes) == [vp, i64, vp, vp, i64, vp, i, i, f64, f64, f64, f32, f32, i,
                                                                    vp, vp, vp, vp, vp, vp]
    text = open(os.path.join(ROOT, "include", "tsdf_mapaccurate.h")).read()
    assert "tsdf_cam" not in text and "#define TSDF_MAPACCURATE_VERSION 1" in text      # the camera comes by value
    # the libraries beside it are what they were
    assert lib.load().tsdf_version() == 7 and lib.load_accurate().tsdf_accurate_version() == 1
    assert exported(lib.ACCURATE_LIB_PATH)[1] == ["tsdf_accurate_version", "tsdf_voxelize_grid_accurate_hip"]


def test_a_refused_load_keeps_no_library(pkg, monkeypatch):
    lib = pkg._lib
    row = lib._EXTS["mapaccurate"]
    monkeypatch.delitem(lib._ext_libs, "mapaccurate", raising=False)
    monkeypatch.setitem(lib._EXTS, "mapaccurate", row._replace(version=row.version + 1))   # the row is read at call time
    with pytest.raises(ImportError, match="version 1"):
        lib.load_mapaccurate()
    assert "mapaccurate" not in lib._ext_libs
    monkeypatch.setitem(lib._EXTS, "mapaccurate", row._replace(path=os.path.join(ROOT, "build", "no_such_libtsdf_mapaccurate.so")))
    with pytest.raises(ImportError, match="csrc mapaccurate"):
        lib.load_mapaccurate()
    assert "mapaccurate" not in lib._ext_libs


# ---- argument checks ----
def _caller(L):
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(72)

    def call(depth=one, depth_len=100, offsets=one, headers=one, n_src=1, index=null, n=1, R=32, cam=GOOD_CAM, layout=0,
             xforms=one, grid=one, out=one, nearest=one, status=one):
        return L.tsdf_voxelize_map_grid_accurate_hip(depth, depth_len, offsets, headers, n_src, index, n, R, *cam, layout, null,
                                                     xforms, grid, out, nearest, status)
    return call, null, one, odd


def test_argument_validation_happens_before_device_work(pkg):
    L = pkg._lib.load_mapaccurate()
    call, null, one, odd = _caller(L)
    assert call(n=-1) == INVALID
    for name in ("depth", "offsets", "headers", "xforms", "grid", "out"):
        assert call(**{name: null}) == INVALID, name
    assert call(depth_len=-1) == INVALID
    assert call(n_src=0, index=one) == INVALID and call(n_src=-3, index=one) == INVALID
    assert call(n_src=2) == INVALID and call(n=2) == INVALID          # no index: n_src must equal n
    for R in (0, 2, 3, 6, 30, 132, 256, -4):
        assert call(R=R) == INVALID, R
    for layout in (-1, 2):
        assert call(layout=layout) == INVALID
    assert call(n=0, n_src=0, R=30) == INVALID and call(n=0, n_src=0, layout=2) == INVALID   # judged before n == 0
    assert call(xforms=ctypes.c_void_p(68)) == INVALID                 # 4-byte, not 8-byte aligned
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
        assert call(xforms=odd) == NO_DEVICE                           # 8-byte aligned is enough for the maps
        assert call(n_src=5, index=one, n=3) == NO_DEVICE
        assert call(n=2 ** 17 - 1, n_src=2 ** 17 - 1, R=128) == NO_DEVICE
        for R in (4, 12, 64, 128):
            assert call(R=R, layout=1) == NO_DEVICE, R
        for good in ((588.03, 320.5, 240.25, 0.5, 2.0), (241.42, NAN, -7.0, 1e-3, 8.0)):   # cx, cy are not judged
            assert call(cam=good) == NO_DEVICE, good


def test_n_zero_is_a_no_op_whatever_else_is_passed(pkg):
    L = pkg._lib.load_mapaccurate()
    call, null, one, odd = _caller(L)
    assert call(n=0, n_src=0) == 0
    assert call(n=0, depth=null, depth_len=-5, xforms=ctypes.c_void_p(68), out=odd, nearest=odd,
                cam=(NAN, NAN, NAN, -1.0, 0.0)) == 0
    assert L.tsdf_voxelize_map_grid_accurate_hip(null, 0, null, null, 0, null, 0, 32, 0.0, 0.0, 0.0, 0.0, 0.0, 0, null, null,
                                                 null, null, null, null) == 0
    assert call(n=0, R=5) == INVALID and call(n=0, layout=7) == INVALID   # the shape is checked whatever n is


# ---- public names and refusals ----
def test_public_names_and_refusals(pkg, synth):
    for name in ("voxelize_map_grid_accurate", "voxelize_aug_accurate"):
        assert name in pkg.__all__ and hasattr(pkg, name) and name in pkg.__doc__, name
    assert "tsdf_mapaccurate.h" in pkg.__doc__ and 'AugmentedStep(tsdf="accurate")' in pkg.__doc__
    assert 'voxelize_obb(tsdf="accurate")' in pkg.__doc__
    assert "tsdf_voxelize_map_grid_accurate_hip" in pkg.voxelize_map_grid_accurate.__doc__
    assert "accurate" in pkg.voxelize_obb.__doc__ and "accurate" in pkg.AugmentedStep.__doc__
    assert list(inspect.signature(pkg.voxelize_obb).parameters)[-1] == "tsdf"
    assert list(inspect.signature(pkg.AugmentedStep.__init__).parameters)[-1] == "tsdf"
    assert inspect.signature(pkg.voxelize_obb).parameters["tsdf"].default == "projective"
    assert inspect.signature(pkg.AugmentedStep.__init__).parameters["tsdf"].default == "projective"
    assert list(inspect.signature(pkg.voxelize_map_grid_accurate).parameters) == [
        "depth", "offsets", "headers", "xforms", "grid", "res", "layout", "cam", "index", "out", "nearest"]
    assert list(inspect.signature(pkg.voxelize_aug_accurate).parameters) == [
        "depth", "offsets", "headers", "xforms", "res", "layout", "dtype", "cam", "gt", "clamp", "index"]
    depth, off, hdr = (torch.from_numpy(x) for x in synth.synth_batch(2, "crop", seed0=3))
    xf, grid = torch.zeros((2, 24), dtype=torch.float64), torch.zeros((2, 8))
    with pytest.raises(ValueError, match="GPU"):
        pkg.voxelize_map_grid_accurate(depth, off, hdr, xf, grid)
    with pytest.raises(ValueError, match="GPU"):
        pkg.voxelize_aug_accurate(depth, off, hdr, xf)
    with pytest.raises(ValueError, match="layout"):
        pkg.voxelize_map_grid_accurate(depth, off, hdr, xf, grid, layout="xyz")
    with pytest.raises(ValueError, match="float16 or torch.bfloat16"):
        pkg.voxelize_aug_accurate(depth, off, hdr, xf, dtype=torch.float32)
    # the pass table still refuses the combination, in the pinned words, and says where the pass is
    V = importlib.import_module(PKG + ".voxelize")
    assert "voxelize_map_grid_accurate" in V._grid_pass.__doc__
    with pytest.raises(ValueError, match="accurate"):
        V._grid_pass(depth, off, hdr, grid, res=8, layout="czyx", cam=None, xforms=xf, tsdf="accurate")


# ---- the composed entries through stubbed primitives ----
N, R8 = 3, 8
BF16 = torch.bfloat16
STUBBED = ("obb_xforms", "map_grids", "_map_grid_accurate", "narrow_volumes", "transform_joints", "normalize_joints",
           "aug_xforms_at", "map_step_head", "voxelize_indexed", "voxelize_aug", "voxelize_aug_lowp", "_map_grid_lowp", "aabb")


class Rec:
    """Recorders in the style of tests/test_compose_cpu.py: ``log`` holds (name, arguments by parameter name, what was
    returned) of every primitive call; every stub returns CPU tensors of the right shapes, or the ``out`` it was given."""

    def __init__(self, V, monkeypatch):
        self.V, self.log = V, []
        for name in STUBBED:
            monkeypatch.setattr(V, name, self._stub(name, getattr(V, name)))
        monkeypatch.setattr(V, "_dev_check", lambda *a, **kw: None)    # ("on the GPU": the check is not under test)

    def _stub(self, name, real):
        sig = inspect.signature(real)

        def fn(*a, **kw):
            b = sig.bind(*a, **kw)
            b.apply_defaults()
            ret = getattr(self, "_" + name.lstrip("_"))(b.arguments)
            self.log.append((name, dict(b.arguments), ret))
            return ret
        fn.__name__ = name
        return fn

    def names(self):
        return [e[0] for e in self.log]

    def _obb_xforms(self, a):
        z = torch.zeros
        return self.V.ObbBatch(torch.rand((N, 24), dtype=torch.float64), z(N, dtype=torch.int32), z(N), z(N, 3), z(N, 6), z(N, 3))

    def _map_grids(self, a):
        return a["out"] if a["out"] is not None else self.V.MapGridBatch(torch.rand(N, 8), torch.rand(N), torch.rand(N, 3),
                                                                         torch.tensor([0, 12, 0], dtype=torch.int32))

    def _map_grid_accurate(self, a):
        vol = a["out"] if a["out"] is not None else torch.rand((N, 3, R8, R8, R8))
        return vol, (torch.zeros(N, dtype=torch.int32) if a["want_status"] else None), None

    def _map_grid_lowp(self, a):
        raise AssertionError("the projective pass in an accurate chain")

    _voxelize_indexed = _aabb = _map_grid_lowp

    def _narrow_volumes(self, a):
        return a["out"] if a["out"] is not None else a["tsdf32"].to(a["dtype"])

    def _transform_joints(self, a):
        return a["out"] if a["out"] is not None else torch.rand_like(a["gt"])

    _normalize_joints = _transform_joints

    def _aug_xforms_at(self, a):
        return a["out"]

    def _map_step_head(self, a):
        return a["out"]

    def _voxelize_aug(self, a):
        b = self.V.TsdfBatch(torch.rand((N, 3, R8, R8, R8)), torch.rand(N), torch.rand(N, 3), torch.zeros(N, dtype=torch.int32))
        return b if a["gt"] is None else (b, torch.rand_like(a["gt"]), torch.rand_like(a["gt"]))

    _voxelize_aug_lowp = _voxelize_aug_accurate = _voxelize_aug


@pytest.fixture()
def V():
    return importlib.import_module(PKG + ".voxelize")


@pytest.fixture()
def rec(V, monkeypatch):
    return Rec(V, monkeypatch)


@pytest.fixture()
def pack():
    return torch.rand(30), torch.tensor([0, 10, 20, 30]), torch.zeros((N, 6), dtype=torch.int32)


def _same_pack(args, pack):
    return all(args[k] is t for k, t in zip(("depth", "offsets", "headers"), pack))


@pytest.mark.parametrize("dtype", [None, BF16])
@pytest.mark.parametrize("with_gt", [False, True])
def test_voxelize_aug_accurate_chain(V, rec, pack, pkg, with_gt, dtype):
    cam = pkg._lib.TsdfCam()
    xf, index = torch.rand((N, 24), dtype=torch.float64), torch.tensor([2, 0, 1])
    gt = torch.rand(N, 63) if with_gt else None
    out = V.voxelize_aug_accurate(*pack, xf, res=R8, layout="cxyz", dtype=dtype, cam=cam, gt=gt, clamp=False, index=index)
    assert rec.names() == ["map_grids", "_map_grid_accurate"] + (["narrow_volumes"] if dtype else []) + \
        (["transform_joints", "normalize_joints"] if with_gt else [])
    (_, pa, placed), (_, va, (vol32, _, _)) = rec.log[:2]
    assert _same_pack(pa, pack) and pa["xforms"] is xf and pa["res"] == R8 and pa["cam"] is cam and pa["index"] is index
    assert _same_pack(va, pack) and va["xforms"] is xf and va["grid"] is placed.grid and va["cam"] is cam
    assert (va["res"], va["layout"]) == (R8, "cxyz") and va["index"] is index
    assert va["out"] is None and va["want_status"] is False and va["nearest"] is False
    batch = out[0] if with_gt else out
    assert isinstance(batch, V.TsdfBatch)
    assert batch.max_l is placed.max_l and batch.mid_p is placed.mid_p and batch.status is placed.status
    if dtype:
        _, na, narrow = rec.log[2]
        assert na["tsdf32"] is vol32 and na["dtype"] is dtype and batch.tsdf is narrow and narrow.dtype is dtype
    else:
        assert batch.tsdf is vol32
    if with_gt:
        (_, ta, gt_aug), (_, la, gt_nor) = rec.log[-2:]
        assert torch.equal(ta["gt"], gt.index_select(0, index)) and ta["xforms"] is xf
        assert la["gt"] is gt_aug and la["max_l"] is placed.max_l and la["mid_p"] is placed.mid_p and la["clamp"] is False
        assert out[1] is gt_nor and out[2] is gt_aug


def test_voxelize_obb_tsdf_keyword(V, rec, pack, pkg, monkeypatch):
    cam = pkg._lib.TsdfCam()
    gt = torch.rand(N, 63)
    monkeypatch.setattr(V, "voxelize_aug_accurate", rec._stub("voxelize_aug_accurate", V.voxelize_aug_accurate))
    for bad in ("exact", None, "Accurate", 1):
        with pytest.raises(ValueError, match="tsdf must be 'projective' or 'accurate'"):
            V.voxelize_obb(*pack, tsdf=bad)
    assert rec.log == []                                               # refused before anything is launched
    for dtype in (None, BF16):
        del rec.log[:]
        r = V.voxelize_obb(*pack, res=R8, layout="cxyz", cam=cam, gt=gt, clamp=False, dtype=dtype, tsdf="accurate")
        assert rec.names() == ["obb_xforms", "voxelize_aug_accurate"]
        (_, oa, ob), (_, va, ret) = rec.log
        assert _same_pack(oa, pack) and oa["cam"] is cam
        assert _same_pack(va, pack) and va["xforms"] is ob.xforms and va["dtype"] is dtype and va["gt"] is gt
        assert (va["res"], va["layout"], va["clamp"]) == (R8, "cxyz", False) and va["cam"] is cam and va["index"] is None
        assert r[0] is ret[0] and r[1] is ret[1] and r[2] is ret[2] and r[3] is ob.xforms
    # the default and the explicit "projective" take the entries they took
    for kw, want in (({}, "voxelize_aug"), ({"tsdf": "projective"}, "voxelize_aug"), ({"dtype": BF16}, "voxelize_aug_lowp")):
        del rec.log[:]
        V.voxelize_obb(*pack, res=R8, **kw)
        assert rec.names() == ["obb_xforms", want]


def _step(V, pack, monkeypatch, **kw):
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    kw.setdefault("graph", False)
    return V.AugmentedStep(*pack, N, centres=torch.rand(N, 3), res=R8, **kw)


def test_augmented_step_refuses_another_tsdf_before_anything(V, rec, pack, monkeypatch):
    for bad in ("exact", None, "ACCURATE"):
        with pytest.raises(ValueError, match="tsdf must be 'projective' or 'accurate'"):
            _step(V, pack, monkeypatch, tsdf=bad)
    with pytest.raises(ValueError, match="tsdf must be 'projective' or 'accurate'"):
        _step(V, pack, monkeypatch, tsdf="exact", dtype=torch.float32, graph="yes")   # ... before every other refusal
    assert rec.log == []


@pytest.mark.parametrize("head", [False, True], ids=["chain", "head"])
@pytest.mark.parametrize("dtype", [None, BF16])
@pytest.mark.parametrize("with_gt", [False, True], ids=["", "gt"])
def test_augmented_step_accurate_chain(V, rec, pack, monkeypatch, head, dtype, with_gt):
    gt = torch.rand(N, 21, 3) if with_gt else None
    base = torch.rand((N, 24), dtype=torch.float64) if head else None
    s = _step(V, pack, monkeypatch, tsdf="accurate", dtype=dtype, gt=gt, base=base, layout="cxyz", clamp=False)
    first = ["map_step_head"] if head else ["aug_xforms_at", "map_grids"]
    labels = ["transform_joints", "normalize_joints"] if with_gt and not head else []
    assert rec.names() == first + ["_map_grid_accurate"] + (["narrow_volumes"] if dtype else []) + labels
    assert s.accurate and s.out.tsdf.dtype is (dtype or torch.float32) and s.out.tsdf.shape == (N, 3, R8, R8, R8)
    _, fa, _ = rec.log[0]
    if head:
        assert fa["place"] is True and fa["base"] is base and fa["gt"] is gt and fa["index"] is s.index
        assert fa["out"].xforms is s.xforms and fa["out"].grid is s._grid.grid and fa["out"].max_l is s.out.max_l
        assert fa["out"].mid_p is s.out.mid_p and fa["out"].status is s.out.status
        assert fa["out"].gt_aug is s.gt_aug and fa["out"].gt_nor is s.gt_nor
    else:
        assert fa["out"] is s.xforms and fa["index"] is s.index
        _, pa, _ = rec.log[1]
        assert pa["xforms"] is s.xforms and pa["index"] is s.index and pa["out"] is s._grid
        assert s._grid.max_l is s.out.max_l and s._grid.mid_p is s.out.mid_p and s._grid.status is s.out.status
    _, va, (vol32, st, _) = rec.log[len(first)]
    assert _same_pack(va, pack) and va["xforms"] is s.xforms and va["grid"] is s._grid.grid and va["index"] is s.index
    assert (va["res"], va["layout"]) == (R8, "cxyz") and va["want_status"] is False and st is None and va["nearest"] is False
    assert va["out"] is not None and va["out"].dtype is torch.float32                 # a static buffer: nothing is allocated
    if dtype:
        _, na, _ = rec.log[len(first) + 1]
        assert na["tsdf32"] is va["out"] and na["out"] is s.out.tsdf and na["dtype"] is dtype and va["out"] is not s.out.tsdf
    else:
        assert va["out"] is s.out.tsdf
    if labels:
        (_, ta, _), (_, la, _) = rec.log[-2:]
        assert ta["xforms"] is s.xforms and ta["out"] is s.gt_aug and la["gt"] is s.gt_aug and la["out"] is s.gt_nor
        assert la["max_l"] is s.out.max_l and la["mid_p"] is s.out.mid_p and la["clamp"] is False


# ---- the reference, on the inputs of the GPU tier ----
# (the dense ones; the sparse frames of tests/sparse_ref.py, whose grids and cameras are their own, have their reference's
# properties and both lists' search windows checked in tests/test_window_cpu.py)
CASES = mr.all_cases()


@pytest.mark.parametrize("label,key", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_reference_properties_on_every_gpu_input(label, key):
    c = mr.case(*key)
    r, R = c["ref"], key[3]
    vol, near, nearest, valid, pix = r["vol"], r["near"], r["nearest"], r["valid"], r["pix"]
    nvox = R ** 3
    # (a) the fragile set is within the cap (expected: empty)
    nfr = int(r["fragile"].sum())
    print(f"{label}: {nfr} fragile, {int(near.sum())} near of {nvox}, {int((near & ~valid).sum())} silhouette")
    assert nfr <= ar.FRAGILE_CAP * nvox
    ok = ~r["fragile"] & ~r["proj_fragile"]
    # (b) a far voxel has the mapped projective value, bit for bit — +0 if rejected, else +-1 — and names no pixel
    far = ~near
    assert (nearest[far] == -1).all() and (nearest[near] >= 0).all()
    assert np.array_equal(vol[:, far].view(np.uint32), np.repeat(r["far"][None], 3, 0)[:, far].view(np.uint32))
    assert np.array_equal(vol[:, far & ok].view(np.uint32), r["proj"][:, far & ok].view(np.uint32))
    assert not vol[:, far & ~valid].view(np.uint32).any()
    # (c) a projective-near voxel is accurate-near with s no larger; the same pixel gives the same bits
    pnear = valid & (r["s_proj"] <= 1.0)
    assert near[pnear & ok].all()
    assert (r["s_best"][pnear] <= r["s_proj"][pnear] * (1 + 1e-12) + 1e-12).all()
    same = near & valid & (nearest == pix) & ok
    if key[4] != "wrong_inverse" and key[2] != "nanfwd" and not str(key[1]).startswith("mixed_"):
        assert pnear.any() and same.any()
    assert np.array_equal(vol[:, same].view(np.uint32), r["proj"][:, same].view(np.uint32))
    # (d) the case reaches the new ground: voxels the projective pass rejects although a mapped point is within the distance
    new = near & ~valid
    if key[2] == "nanfwd":
        assert not near.any()                                          # a NaN s wins no comparison: every voxel is far
    else:
        assert new.any() and (vol[:, new] >= 0).all()                  # ... and they are positive: free space


def test_reference_on_a_crop_with_one_valid_pixel_under_general():
    F, cx, cy = ar.DEFAULT_CAM[:3]
    left, top, bw, bh = 150, 100, 7, 5
    depth = np.zeros(bw * bh, np.float32)
    k = 2 * bw + 4
    depth[k] = np.float32(400.25)
    header = np.array([320, 240, left, top, left + bw, top + bh], np.int32)
    col, row, d = left + 4, top + 2, float(depth[k])
    w = np.array([(col - cx) * d / F, -(row - cy) * d / F, -d])
    A, b = mg.MATRICES["general"], np.array([12.0, -7.5, 3.25])
    xf = mg.pack(A, b)
    tw = A @ w + b
    R, vl, td = 8, np.float32(2.5), np.float32(7.5)
    ori = (tw - 3.3 * float(vl)).astype(np.float32)
    grid_row = np.array([*ori, vl, td, 0, 0, 0], np.float32)
    r = mr.frame(depth, header, grid_row, R, xf)
    assert r["near"].any() and not r["near"].all() and not r["fragile"].any()
    assert (r["nearest"][r["near"]] == k).all() and (r["nearest"][~r["near"]] == -1).all()
    c = mg.centres(grid_row, R)
    zz, yy, xx = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
    t = np.stack([c[0][xx] - tw[0], c[1][yy] - tw[1], c[2][zz] - tw[2]]) / float(td)
    assert np.array_equal(r["near"], (t ** 2).sum(axis=0) <= 1.0)
    want = np.minimum(np.abs(t), 1.0).astype(np.float32)
    sign = np.where(r["negative"], -1.0, 1.0).astype(np.float32)
    assert np.abs(r["vol"][:, r["near"]] - (want * sign)[:, r["near"]]).max() <= 1e-6
    # no valid pixel at all: a zero volume, nothing near
    z = mr.frame(np.zeros(bw * bh, np.float32), header, grid_row, R, xf)
    assert not z["vol"].view(np.uint32).any() and (z["nearest"] == -1).all() and not z["fragile"].any()


@pytest.mark.parametrize("crop", mr.CROPS_R12)
@pytest.mark.parametrize("name", sorted(mg.SCALES))
def test_reference_under_exact_scale_maps_is_the_identity_case(name, crop):
    ident = mr.case("synth", crop, "identity", 12)
    c = mr.case("synth", crop, name, 12)
    s = np.float32(mg.SCALES[name])
    scaled = ident["grid"][0].copy()
    scaled[:5] *= s
    assert np.array_equal(c["grid"][0], scaled)                       # the pair's own placement IS the scaled row
    assert np.array_equal(c["ref"]["nearest"], ident["ref"]["nearest"])
    assert np.array_equal(c["ref"]["vol"].view(np.uint32), ident["ref"]["vol"].view(np.uint32))
    assert np.array_equal(c["ref"]["s_best"], ident["ref"]["s_best"])


def test_reference_status_rules_and_layouts():
    keys = [k for _, k in mr.PAIRS_R12[:4]]
    depth, off, hdr, xf, grid, cs = mr.batch(keys)
    g2 = grid[[0, 1, 2, 3, 0, 1]].copy()
    g2[1, 4] = 0.0
    x2 = xf[[0, 1, 2, 3, 0, 1]]
    frames = {0: cs[0]["ref"], 4: cs[0]["ref"]}
    tsdf, st, nn, fr = mr.voxelize_map_grid_accurate_ref(depth, off, hdr, x2, g2, 12, "czyx", index=[0, 1, 4, -1, 0, 1],
                                                         frames=frames)
    assert st.tolist() == [0, 1, 2, 2, 0, 0] and not tsdf[[1, 2, 3]].any() and (nn[[1, 2, 3]] == -1).all()   # rows: per POSITION
    assert np.array_equal(tsdf[0], cs[0]["ref"]["vol"]) and np.array_equal(tsdf[4], tsdf[0])
    assert np.array_equal(tsdf[5], cs[1]["ref"]["vol"]) and np.array_equal(nn[5], cs[1]["ref"]["nearest"])
    t1, s1, n1, _ = mr.voxelize_map_grid_accurate_ref(depth, off, hdr, xf, grid, 12, "cxyz", frames={1: cs[1]["ref"]})
    assert np.array_equal(t1[1], cs[1]["ref"]["vol"].transpose(0, 3, 2, 1))
    assert np.array_equal(n1[1], cs[1]["ref"]["nearest"].transpose(2, 1, 0))
    assert np.array_equal(t1[0], tsdf[0].transpose(0, 3, 2, 1))       # computed, not handed in: the same frame
    _, s2, _, _ = mr.voxelize_map_grid_accurate_ref(depth, off, hdr, xf, grid, 12, "czyx", depth_len=depth.size - 1,
                                                    frames={i: c["ref"] for i, c in enumerate(cs)})
    assert s2.tolist() == [0, 0, 0, 2]
