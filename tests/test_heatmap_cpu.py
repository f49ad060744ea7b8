"""CPU tier of the voxel heatmap labels (include/tsdf_heatmap.h): libtsdf_heatmap.so as far as it goes without a GPU — the
build rule, the loader's row against header and binary, the version, every argument refusal before device work —, the
properties of the numpy restatement the GPU tier compares with (tests/heatmap_ref.py), the public names and refusals, and
the library's host-only code under the CPU sanitizers as a child process.  Nothing here touches a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heatmap_ref as hr  # noqa: E402
from abi_util import declared_functions, exported  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "handposeestimation-with-3d-cnns_amd", "csrc")
INVALID, NO_DEVICE = -1, -2
WANT = ["tsdf_heatmap_joints_hip", "tsdf_heatmap_version", "tsdf_joint_heatmaps_hip"]
OTHERS = ["augment", "augstep", "auggrid", "depth16", "obb", "lowp", "maplowp", "mapstep", "locate", "accurate", "mapaccurate"]


# ---- library pins ----
def test_row_binds_exactly_its_header_with_types(pkg):
    lib = pkg._lib
    ext = lib._HEATMAP
    assert isinstance(ext, lib._Ext) and "heatmap" not in lib._EXTS
    assert declared_functions("tsdf_heatmap.h") == WANT == sorted([ext.version_symbol, *ext.entries])
    funcs, named = exported(lib.HEATMAP_LIB_PATH)
    assert funcs == WANT and named == WANT
    assert ext.path == lib.HEATMAP_LIB_PATH and ext.version == lib.HEATMAP_VERSION == 1
    L = lib.load_heatmap()
    assert L.tsdf_heatmap_version() == 1
    for entry in (ext.version_symbol, *ext.entries):
        fn = getattr(L, entry)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, entry
    vp, i, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert list(L.tsdf_heatmap_version.argtypes) == []
    assert list(L.tsdf_joint_heatmaps_hip.argtypes) == [vp, vp, i, i, i, f32, i, i, vp, vp, vp]
    assert list(L.tsdf_heatmap_joints_hip.argtypes) == [vp, i, i, i, i, i, i, vp, vp, vp, vp]
    for name, args in ext.entries.items():
        assert list(getattr(L, name).argtypes) == args and args
    # one object, distinct from every other loader's
    assert lib.load_heatmap() is L and L is not lib.load()
    assert all(L is not getattr(lib, "load_" + other)() for other in OTHERS)
    text = open(os.path.join(ROOT, "include", "tsdf_heatmap.h")).read()
    assert "tsdf_cam" not in text and "#define TSDF_HEATMAP_VERSION 1" in text
    assert lib.load().tsdf_version() == 7   # the product beside it is what it was


def test_wrong_version_and_missing_library_raise_import_error(pkg, monkeypatch):
    lib = pkg._lib
    row = lib._HEATMAP
    monkeypatch.delitem(lib._ext_libs, "heatmap", raising=False)
    monkeypatch.setattr(lib, "_HEATMAP", row._replace(version=row.version + 1))
    with pytest.raises(ImportError, match="version 1.*csrc heatmap"):
        lib.load_heatmap()
    monkeypatch.setattr(lib, "_HEATMAP", row._replace(path=os.path.join(ROOT, "build", "no_such_libtsdf_heatmap.so")))
    with pytest.raises(ImportError, match="csrc heatmap"):
        lib.load_heatmap()


# ---- build pins ----
def test_makefile_builds_it_outside_the_pinned_table():
    lines = open(os.path.join(CSRC, "Makefile")).read().splitlines()
    assert "heatmap_DEPS := narrow.inc heatmap_host.inc ../../include/tsdf_lowp.h" in lines
    assert "$(eval $(call EXT_RULES,heatmap))" in lines
    (all_line,) = [ln for ln in lines if ln.startswith("all:")]
    (phony,) = [ln for ln in lines if ln.startswith(".PHONY:")]
    assert "heatmap" in all_line.split() and "heatmap" in phony.split() and "heatmap-host-asan" in phony.split()
    clean = lines[lines.index("clean:") + 1]
    assert "../libtsdf_heatmap.so" in clean.split()
    (exts,) = [ln for ln in lines if re.match(r"^EXTS := ", ln)]
    assert exts.split(":=")[1].split() == OTHERS


def test_make_rules_cross_compile_for_gfx950_without_scratch():
    r = subprocess.run(["make", "-C", CSRC, "heatmap", "heatmap-resources"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stdout + r.stderr
    assert "tsdf_heat_encode_kernel" in text and "tsdf_heat_decode_kernel" in text
    scratch = [ln for ln in text.splitlines() if "ScratchSize" in ln]
    # encode: 2 layouts x (float32, and 2 dtypes x {8, 4} voxels a lane); decode: 2 layouts x 3 dtypes
    assert len(scratch) == 16 and all(ln.split("]:")[1].split()[0] == "0" for ln in scratch), scratch
    src = open(os.path.join(CSRC, "tsdf_heatmap.hip")).read()
    assert sorted(re.findall(r'#include "(\w+\.inc)"', src)) == ["device.inc", "heatmap_host.inc", "narrow.inc"]
    assert "atomic" not in src.split("namespace {", 1)[1] and "__device__ int" not in src   # no atomics, no device globals


# ---- refusals ----
null, one, odd8, odd2 = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(72), ctypes.c_void_p(66)
nan, inf = float("nan"), float("inf")


def _calls(pkg):
    """The two entries on dummy pointers (64: aligned for every check), every argument good unless named."""
    L = pkg._lib.load_heatmap()

    def enc(u=one, status=one, n=3, J=21, R=32, sigma=1.7, layout=0, dtype=0, heat=one, valid=one):
        return L.tsdf_joint_heatmaps_hip(u, status, n, J, R, sigma, layout, dtype, null, heat, valid)

    def dec(heat=one, dtype=0, n=3, J=21, R=32, layout=0, radius=0, u=one, peak=one, arg=one):
        return L.tsdf_heatmap_joints_hip(heat, dtype, n, J, R, layout, radius, null, u, peak, arg)

    return L, enc, dec


def test_every_defect_is_refused_before_device_work(pkg):
    L, enc, dec = _calls(pkg)
    shared = [dict(n=-1), *[dict(R=R) for R in (0, 2, 3, 6, 30, 132, 256, -4)], dict(J=0), dict(J=171), dict(J=-1),
              dict(layout=2), dict(layout=-1), dict(dtype=3), dict(dtype=-1), dict(n=2 ** 24, J=1), dict(n=98690, J=170)]
    defects = {
        enc: shared + [dict(sigma=s) for s in (0.0, -0.0, -1.0, nan, inf, -inf, 1e-50)] +
        [dict(u=null), dict(heat=null), dict(heat=odd8), dict(u=odd2), dict(status=odd2), dict(valid=odd2)],
        dec: shared + [dict(radius=r) for r in (-1, 4, 100)] +
        [dict(heat=null), dict(u=null), dict(heat=odd8), dict(u=odd2), dict(peak=odd2), dict(arg=odd2)],
    }
    for call, rows in defects.items():
        for kw in rows:
            assert call(**kw) == INVALID, (call.__name__, kw)
            if "n" not in kw:      # n == 0 is a no-op whatever comes after it in the order
                assert call(n=0, **kw) == 0, (call.__name__, kw)
        assert call(n=0) == 0 and call(n=0, J=0, R=5) == 0
    assert L.tsdf_joint_heatmaps_hip(null, null, 0, 0, 0, nan, 9, 9, null, null, null) == 0
    assert L.tsdf_heatmap_joints_hip(null, 9, 0, 0, 0, 9, 9, null, null, null, null) == 0


# Good arguments reach check_device.  On a machine WITH a device they would launch on the dummy pointers, so this row is
# checked where the device check answers -2.
@pytest.mark.skipif(torch.cuda.is_available(), reason="good arguments with dummy pointers must stop at the device check")
def test_good_arguments_get_as_far_as_the_device(pkg):
    L, enc, dec = _calls(pkg)
    for call in (enc, dec):
        assert call() == NO_DEVICE
        for R in (4, 12, 64, 128):
            for dtype in (0, 1, 2):
                for layout in (0, 1):
                    assert call(R=R, dtype=dtype, layout=layout) == NO_DEVICE
        assert call(J=1) == NO_DEVICE and call(J=170) == NO_DEVICE and call(n=98688, J=170) == NO_DEVICE
    assert enc(status=null, valid=null) == NO_DEVICE and dec(peak=null, arg=null) == NO_DEVICE      # the optional ones
    assert enc(heat=ctypes.c_void_p(80), u=ctypes.c_void_p(68)) == NO_DEVICE
    for r in (0, 1, 2, 3):
        assert dec(radius=r) == NO_DEVICE
    for s in (1e-30, 0.5, 4.0, 3e38):
        assert enc(sigma=s) == NO_DEVICE
    # the resolution rule is the product's
    P = pkg._lib.load()
    for R in range(-8, 264):
        assert (enc(R=R) == INVALID) == (dec(R=R) == INVALID) == (not P.tsdf_resolution_supported(R)), R


# ---- restatement properties ----
def test_the_separable_product_is_the_gaussian_formed_directly():
    """(g_z g_y) g_x against exp(-|i - c|^2 k) formed in one piece, both rounded to float32: within 1 float32 ulp (three
    correctly rounded exp and two products carry a few 1e-16 of relative error into one rounding)."""
    rng = np.random.default_rng(11)
    worst, draws = 0.0, 0
    for R in (4, 8, 12, 20, 32, 44, 64):
        for sigma in (0.5, 1.0, 1.7, 2.5, 4.0):
            u = rng.uniform(-0.1, 1.1, size=(1, 6, 3)).astype(np.float32)
            heat, valid = hr.encode(u, None, R, sigma, "czyx")
            assert valid.all()
            k = 1.0 / (2.0 * np.float64(np.float32(sigma)) ** 2)
            c = u[0].astype(np.float64) * R - 0.5
            i = np.arange(R, dtype=np.float64)
            for j in range(6):
                d2 = ((i - c[j, 2]) ** 2)[:, None, None] + ((i - c[j, 1]) ** 2)[None, :, None] + ((i - c[j, 0]) ** 2)[None, None, :]
                direct = np.exp(-(d2 * k))
                direct = np.where(direct < hr.TINY, 0.0, direct).astype(np.float32)
                got = heat[0, j]
                both = (direct > 2.0 ** -120) & (got > 2.0 ** -120)     # away from the flush threshold
                ulp = np.abs(got[both].astype(np.float64) - direct[both]) / np.spacing(direct[both]).astype(np.float64)
                worst = max(worst, float(ulp.max()))
                assert (np.abs(got.astype(np.float64) - direct) <= 2.0 ** -23 * direct + 2.0 ** -125).all()
                draws += 1
    print(f"separable against direct: worst {worst} ulp over {draws} draws")
    assert draws == 210 and worst <= 1.0


def test_the_argmax_is_the_nearest_voxel_and_a_tie_goes_to_the_lower_index():
    rng = np.random.default_rng(5)
    for R in (8, 12, 32):
        for layout in hr.LAYOUTS:
            u = rng.uniform(0.0, 1.0, size=(2, 5, 3)).astype(np.float32)
            heat, _ = hr.encode(u, None, R, 1.7, layout)
            got, peak, arg = hr.decode(heat, R, layout, 0)
            c = u.astype(np.float64) * R - 0.5
            near = np.clip(np.rint(c), 0, R - 1)
            dist = np.abs(c - np.rint(c))
            sure = dist < 0.49                                       # away from a half-voxel tie
            want = ((near + 0.5) / R).astype(np.float32)
            assert np.array_equal(got[sure], want[sure]) and sure.mean() > 0.9
            assert (peak > 0).all() and (arg >= 0).all()
    # c = (3.5, 2, 7.5) at R = 8: x ties between 3 and 4, z = 7.5 is nearest to 7 alone (8 is outside)
    u = ((np.array([[[3.5, 2.0, 7.5]]]) + 0.5) / 8).astype(np.float32)
    assert np.array_equal(u.astype(np.float64) * 8 - 0.5, [[[3.5, 2.0, 7.5]]])
    for layout in hr.LAYOUTS:
        heat, _ = hr.encode(u, None, 8, 1.7, layout)
        top = np.argwhere(heat[0, 0] == heat[0, 0].max())
        assert len(top) == 2
        got, peak, arg = hr.decode(heat, 8, layout, 0)
        assert np.array_equal(got[0, 0], ((np.array([3, 2, 7]) + 0.5) / 8).astype(np.float32))
        assert arg[0, 0] == ((7 * 8 + 2) * 8 + 3 if layout == "czyx" else (3 * 8 + 2) * 8 + 7)
    # the NaN, fallback and flush rules of the restatement itself
    v = np.full((1, 1, 4, 4, 4), np.nan, np.float32)
    got, peak, arg = hr.decode(v, 4, "czyx", 2)
    assert arg[0, 0] == -1 and np.isnan(peak[0, 0]) and np.array_equal(got[0, 0], [0.5, 0.5, 0.5])
    v = np.full((1, 1, 4, 4, 4), -2.0, np.float32)
    v[0, 0, 3, 3, 3] = -1.0
    got, peak, arg = hr.decode(v, 4, "czyx", 3)
    assert arg[0, 0] == 63 and peak[0, 0] == -1.0 and np.array_equal(got[0, 0], np.float32([0.875] * 3))
    heat, valid = hr.encode(np.float32([[[50, 0.5, 0.5], [np.nan, 0.5, 0.5]], [[0.5, 0.5, 0.5]] * 2]), np.int32([0, 2]), 8, 0.5)
    assert not heat[0].any() and not heat[1].any() and valid.tolist() == [[1, 0], [0, 0]]
    small = hr.encode(np.float32([[[0.5, 0.5, 0.5]]]), None, 32, 0.5)[0]
    assert ((small > 0) & (small < 2.0 ** -126)).sum() == 0 and (small == 0).sum() > 1000
    assert abs(float(small.max()) - np.exp(-1.5)) < 1e-7      # c = 15.5 on every axis: half a voxel off, k = 2


def test_plan_restatement_covers_the_three_shapes():
    for cus in (1, 8, 256, 304):
        for R in (4, 12, 32, 44, 128):
            for nj in (1, 2, 63, 85, 340, 511, 512, 513, 700):
                slab, nslab, wgs = hr.plan(nj, R, cus)
                assert 1 <= slab <= R and (nslab - 1) * slab < R <= nslab * slab and wgs == nj * nslab
                assert nslab == 1 if nj >= 2 * cus else wgs <= max(2 * cus, nj)
    assert {hr.plan_class(nj, R, 256) for nj in (1, 63, 85, 340) for R in (4, 8, 12, 20, 32, 44, 64)} == {"one", "equal", "ragged"}


# ---- Python wrappers ----
def test_public_names_and_refusals(pkg, synth):
    for name in ("joint_heatmaps", "heatmap_joints", "HeatmapJoints"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
        assert name in pkg.__doc__ or name == "HeatmapJoints", name     # (the docstring lists functions, not result types)
    assert "tsdf_heatmap.h" in pkg.__doc__ and "AugmentedStep(heatmap=" in pkg.__doc__
    assert pkg.HeatmapJoints._fields == ("u", "peak", "arg")
    u = torch.full((2, 63), 0.5)
    heat = torch.zeros((2, 3, 8, 8, 8))
    # there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        pkg.joint_heatmaps(u)
    with pytest.raises(ValueError, match="GPU"):
        pkg.heatmap_joints(heat)
    # and everything else is judged before anything could be launched (the tensors are on the CPU: a launch cannot follow)
    for bad in (torch.float64, torch.int16, "float32", None):
        with pytest.raises(ValueError, match="float32, torch.float16 or torch.bfloat16"):
            pkg.joint_heatmaps(u, dtype=bad)
    with pytest.raises(ValueError, match="float32, torch.float16 or torch.bfloat16"):
        pkg.heatmap_joints(heat.double())
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), 1e-50, "1.7", None):
        with pytest.raises(ValueError, match="sigma"):
            pkg.joint_heatmaps(u, sigma=bad)
    for bad in (-1, 4, 1.0, True, None):
        with pytest.raises(ValueError, match="radius"):
            pkg.heatmap_joints(heat, radius=bad)
    for fn, x in ((pkg.joint_heatmaps, u), (pkg.heatmap_joints, heat)):
        with pytest.raises(ValueError, match="layout"):
            fn(x, layout="xyzc")
    for bad in (0, 30, 132, 31.5, "x", None):
        with pytest.raises(ValueError, match="resolution"):
            pkg.joint_heatmaps(u, res=bad)
    # AugmentedStep(heatmap=...) judges its tuple and asks for gt before it looks at the pack
    depth, off, hdr = (torch.from_numpy(x) for x in synth.synth_batch(2, "crop", seed0=3))
    with pytest.raises(ValueError, match="heatmap needs gt"):
        pkg.AugmentedStep(depth, off, hdr, 2, heatmap=(44, 1.7))
    for bad, what in (((44,), "heatmap must be"), (44, "heatmap must be"), ((30, 1.7), "resolution"), ((44, 0.0), "sigma"),
                      ((44, 1.7, torch.int8), "float32, torch.float16 or torch.bfloat16")):
        with pytest.raises(ValueError, match=what):
            pkg.AugmentedStep(depth, off, hdr, 2, gt=torch.zeros((2, 63)), heatmap=bad)
    with pytest.raises(ValueError, match="GPU"):       # a good tuple gets as far as the pack's own check
        pkg.AugmentedStep(depth, off, hdr, 2, gt=torch.zeros((2, 63)), heatmap=(44, 1.7, torch.bfloat16))


# ---- sanitizer child ----
def test_host_code_under_sanitizers_as_a_stand_alone_program():
    subprocess.check_call(["make", "-C", CSRC, "-B", "heatmap-host-asan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "build", "heatmap_host_asan")
    env = dict(os.environ)
    env.update(ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "heatmap host code ok (89600 plans)" in r.stdout, tail     # 32 resolutions x 700 x 4 CU counts
    assert "Sanitizer" not in tail and "runtime error" not in tail and "FAILED" not in tail, tail


def test_the_library_includes_the_same_text():
    """The library and the stand-alone program compile ONE text of the rules: heatmap_host.inc, which takes the three tests
    that exist already (bad_res, misaligned, bad_dtype) from its includer — the library from device.inc and narrow.inc, the
    program from copies of those lines."""
    unit = open(os.path.join(CSRC, "tsdf_heatmap.hip")).read()
    inc, main = (open(os.path.join(CSRC, f)).read() for f in ("heatmap_host.inc", "heatmap_host_main.cc"))
    theirs = open(os.path.join(CSRC, "device.inc")).read().splitlines() + open(os.path.join(CSRC, "narrow.inc")).read().splitlines()
    for name in ("bad_res", "misaligned", "bad_dtype"):
        (line,) = [ln for ln in main.splitlines() if re.search(rf"\bbool {name}\(", ln)]
        assert line in theirs, name
        assert f"{name}(" in inc and not re.search(rf"\bbool {name}\(", inc), name            # used, not restated
    assert unit.index('#include "device.inc"') < unit.index('#include "narrow.inc"') < unit.index('#include "heatmap_host.inc"')
    assert '#include "heatmap_host.inc"' in unit and "heat_plan(" in unit and "heat_item(" in unit
    for name in ("heat_defect_encode(", "heat_defect_decode("):
        assert name in unit and name in open(os.path.join(CSRC, "heatmap_host.inc")).read()
