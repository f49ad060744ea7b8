"""CPU tier of the farthest-point sampled clouds (include/tsdf_fps.h): the properties of the numpy restatement the GPU tier
compares with (tests/fps_ref.py) on that tier's own inputs — the prefix property, the radii, the covering, the tie rule,
the hard values, and that each deliberate mistake is seen —, and libtsdf_fps.so as far as it goes without a GPU: the
loader's row against header and binary, every argument refusal before device work, the plan, the build rule and the
resource report, the host-only code under the CPU sanitizers as a child process, the public names and refusals with
launches stubbed, and AugmentedStep(fps=...) through stubbed primitives.  Nothing here touches a GPU."""
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
import fps_ref as fr  # noqa: E402
import frame_zoo as fz  # noqa: E402
import occupancy_ref as orf  # noqa: E402
from abi_util import declared_functions, exported  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "handposeestimation-with-3d-cnns_amd"
CSRC = os.path.join(ROOT, PKG, "csrc")
INVALID, NO_DEVICE = -1, -2
WANT = ["tsdf_fps_hip", "tsdf_fps_plan", "tsdf_fps_points_hip", "tsdf_fps_version"]
BIG = 200000     # a capacity above every count of the zoo


# ---- the reference, on the inputs of the GPU tier ----
@pytest.fixture(scope="module")
def groups():
    """name -> (call, M): the GPU tier's groups, each a function of ``mistake`` that returns the reference's Fps."""
    pack, zoo, exact = fr.crops(16), fr.zoo_pack()[0], fr.exact_pack()
    maps = fz.aug_maps(orf.placed(pack)[1])
    return {
        "crops": (lambda **kw: fr.batch(*pack, 1024, capacity=BIG, **kw), 1024),
        "crops_mapped": (lambda **kw: fr.batch(*pack, 128, xforms=maps, capacity=BIG, **kw), 128),
        "zoo": (lambda **kw: fr.batch(*zoo, 200, capacity=BIG, **kw), 200),
        "exact": (lambda **kw: fr.batch(*exact, 64, **kw), 64),
        "ties": (lambda **kw: fr.cloud_batch(fr.tie_clouds(), 70, **kw), 70),
        "hard": (lambda **kw: fr.cloud_batch(fr.hard_clouds(), 16, **kw), 16),
    }


@pytest.fixture(scope="module")
def refs(groups):
    return {name: call() for name, (call, _) in groups.items()}


def test_the_first_k_rows_are_the_k_point_result(groups, refs):
    pack = fr.crops(4)
    whole = fr.batch(*pack, 300)
    for k in (1, 2, 7, 64, 299):
        assert fr.same(fr.batch(*pack, k), whole, k) is None, k
    clouds = fr.tie_clouds()
    whole = fr.cloud_batch(clouds, 70)
    for k in (1, 2, 32, 33, 64, 65):
        assert fr.same(fr.cloud_batch(clouds, k), whole, k) is None, k


def test_radius2_starts_at_infinity_and_never_grows_and_the_samples_cover_the_cloud_within_it(refs):
    for name, ref in refs.items():
        live = ref.status == 0
        assert live.any(), name
        r2 = ref.radius2[live]
        assert np.isposinf(r2[:, 0]).all() and (r2[:, 1:] <= r2[:, :-1]).all(), name
        assert (ref.radius2[~live] == 0).all() and (ref.pixel[~live] == -1).all() and not ref.points[~live].any()
    # every candidate lies within sqrt(radius2[M-1]) of some sample: its running dist is at most the last maximum
    pack = fr.crops(3)
    ref = fr.batch(*pack, 128, capacity=BIG)
    for i in range(3):
        p, rank = fr.crop_candidates(pack[0][pack[1][i]:pack[1][i + 1]], pack[2][i])
        d = ((p[:, None, :].astype(np.float64) - ref.points[i][None, :127].astype(np.float64)) ** 2).sum(2).min(1)
        assert d.max() <= float(ref.radius2[i, 127]) * (1 + 1e-6)
        assert np.array_equal(p[np.searchsorted(rank, ref.pixel[i])], ref.points[i])        # pixel is the point's rank
        assert len(set(ref.pixel[i].tolist())) == 128                                       # 128 distinct pixels


def test_a_frame_of_fewer_candidates_repeats_row_0(refs):
    ref = refs["exact"]
    assert ref.count.tolist() == [7, 63, 64, 0] and ref.status.tolist() == [0, 0, 0, 1]
    for i, c in ((0, 7), (1, 63), (2, 64)):
        assert len(set(ref.pixel[i, :c].tolist())) == c                      # every candidate once ...
        assert (ref.pixel[i, c:] == ref.pixel[i, 0]).all() and (ref.radius2[i, c:] == 0).all()   # ... then row 0 again
        assert (ref.points[i, c:] == ref.points[i, 0]).all() and (ref.radius2[i, 1:c] > 0).all()
    zoo = refs["zoo"]
    assert (zoo.count < 200).sum() >= 10 and (zoo.count > 200).sum() >= 10 and (zoo.count > fr.RESIDENT).sum() >= 3
    assert {1, 2}.issubset(set(zoo.count.tolist())) or zoo.count.min() <= 2


def test_ties_go_to_the_lowest_rank():
    lat = fr.lattice()                                                       # 4 x 4 x 2, x fastest, step 8
    idx, rad = fr.select(lat, 32)
    # sample 0 is row 0, a corner.  The farthest point is the opposite corner alone (no tie); then the corners of the
    # far face tie in pairs and the lower row wins
    assert idx[0] == 0 and idx[1] == 31 and rad[1] == np.float32(24 ** 2 + 24 ** 2 + 8 ** 2)
    assert rad[2] == rad[3] and idx[2] < idx[3]
    assert sorted(idx.tolist()) == list(range(32)) and rad[31] == 64.0       # every point once, the last a step away
    clouds = fr.tie_clouds()
    ref = fr.cloud_batch(clouds, 70)
    assert ref.count.tolist() == [64] * 5 and not ref.status.any()
    assert sorted(ref.pixel[0, :32].tolist()) == list(range(32))             # of two copies the first is taken ...
    assert (ref.pixel[0, 32:] == 0).all() and (ref.radius2[0, 32:] == 0).all()   # ... and the copies never are
    assert ref.pixel[2].tolist() == [0] * 70                                 # one point 64 times
    assert ref.pixel[3].tolist() == [0, 1] + [0] * 68                        # two points alternating
    assert sorted(ref.pixel[4, :64].tolist()) == list(range(64)) and (ref.pixel[4, 64:] == ref.pixel[4, 0]).all()
    high = fr.cloud_batch(clouds, 70, mistake="ties_high")
    assert all((high.pixel[i] != ref.pixel[i]).any() for i in range(5))


def test_infinite_distances_and_dropped_rows(refs):
    ref = refs["hard"]
    clouds = fr.hard_clouds()
    assert ref.count.tolist() == [37, 20, 0, 1] and ref.status.tolist() == [0, 0, 1, 0]
    assert not {5, 9, 17} & set(ref.pixel[0].tolist())                       # NaN / inf rows are no candidates
    assert (ref.pixel[1] % 2 == 1).all()                                     # 1e39 overflows float32: dropped
    assert ref.pixel[3].tolist() == [23] * 16 and ref.points[3, 5].tolist() == [1.0, 2.0, 3.0]
    # row 0 of cloud 0 is 1e30-sized: from it every other point is +inf away, so the ranks come in order while the
    # maximum is +inf — the tie rule at +inf
    inf_rows = np.isposinf(ref.radius2[0])
    assert inf_rows[:14].all() and not inf_rows[14:].any()
    assert (np.diff(ref.pixel[0, :14]) > 0).all() and not np.isnan(ref.radius2).any()
    assert np.isfinite(ref.points).all() and np.abs(clouds[0, ::3]).max() > 1e30


def test_each_mistake_changes_a_selected_rank(groups, refs):
    """The table of DESIGN.md: which group of the GPU tier sees which mistake."""
    seen = {}
    for name, (call, M) in groups.items():
        for mistake in fr.MISTAKES:
            bad = call(mistake=mistake)
            rows = int((bad.pixel != refs[name].pixel).any(1).sum())
            seen[name, mistake] = rows
            print(f"{name:13s} {mistake:10s} changes {rows} of {len(bad.pixel)} positions")
    for mistake in fr.MISTAKES:
        assert sum(seen[name, mistake] > 0 for name in groups) >= 2, mistake
    assert seen["ties", "ties_high"] == 5 and seen["zoo", "skip_first"] >= 60
    assert seen["crops", "float64"] >= 1 and seen["crops", "ties_high"] >= 1 and seen["crops", "skip_first"] == 16


# ---- library pins ----
def test_row_binds_exactly_its_header_with_types(pkg):
    lib = pkg._lib
    ext = lib._FPS
    assert isinstance(ext, lib._Ext) and "fps" not in lib._EXTS
    assert declared_functions("tsdf_fps.h") == WANT == sorted([ext.version_symbol, *ext.entries])
    funcs, named = exported(lib.FPS_LIB_PATH)
    assert funcs == WANT and named == WANT
    assert ext.path == lib.FPS_LIB_PATH and ext.version == lib.FPS_VERSION == 1
    L = lib.load_fps()
    assert L.tsdf_fps_version() == 1
    vp, i, i64, f32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
    ip, lp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)
    assert list(L.tsdf_fps_plan.argtypes) == [i, i64, i, ip, lp, ip]
    assert list(L.tsdf_fps_hip.argtypes) == [vp, i64, vp, vp, i64, vp, i, i, f64, f64, f64, f32, f32, i64, i, vp, vp, vp, vp,
                                             vp, vp, vp, vp]
    assert list(L.tsdf_fps_points_hip.argtypes) == [vp, i, i, i64, i, i64, i, vp, vp, vp, vp, vp, vp, vp]
    for name in (ext.version_symbol, *ext.entries):
        assert getattr(L, name).restype is ctypes.c_int
    assert lib.load_fps() is L and L is not lib.load() and L is not lib.load_occupancy()
    text = open(os.path.join(ROOT, "include", "tsdf_fps.h")).read()
    assert "tsdf_cam" not in text and "#define TSDF_FPS_VERSION 1" in text and "#define TSDF_FPS_FRAME_OVER_CAPACITY 3" in text
    assert "dist is never a NaN" in text and "the first k rows of an M-point result are the k-point" in text
    assert lib.TSDF_FPS_FRAME_OVER_CAPACITY == fr.OVER_CAPACITY == 3 and lib.FPS_MAX_POINTS == fr.MAX_POINTS == 65536
    assert lib.load().tsdf_version() == 7 and lib.load_occupancy().tsdf_occupancy_version() == 1


def test_wrong_version_and_missing_library_raise_import_error(pkg, monkeypatch):
    lib = pkg._lib
    row = lib._FPS
    monkeypatch.delitem(lib._ext_libs, "fps", raising=False)
    monkeypatch.setattr(lib, "_FPS", row._replace(version=row.version + 1))
    with pytest.raises(ImportError, match="version 1.*csrc fps"):
        lib.load_fps()
    monkeypatch.setattr(lib, "_FPS", row._replace(path=os.path.join(ROOT, "build", "no_such_libtsdf_fps.so")))
    with pytest.raises(ImportError, match="csrc fps"):
        lib.load_fps()


# ---- build pins ----
def test_makefile_builds_it_outside_the_pinned_table():
    src = open(os.path.join(CSRC, "Makefile")).read()
    lines = src.splitlines()
    assert "fps_DEPS := prim.inc fps_host.inc" in lines and "$(eval $(call EXT_RULES,fps))" in lines
    (all_line,) = [ln for ln in lines if ln.startswith("all:")]
    (phony,) = [ln for ln in lines if ln.startswith(".PHONY:")]
    assert "fps" in all_line.split() and {"fps", "fps-resources", "fps-asm", "fps-host-asan"} <= set(phony.split())
    assert "../libtsdf_fps.so" in lines[lines.index("clean:") + 1].split()
    assert "fps_host.inc" in src.split("$(filter-out", 1)[1].split(",", 1)[0].split()   # not a part of the product
    (exts,) = [ln for ln in lines if re.match(r"^EXTS := ", ln)]
    assert "fps" not in exts.split() and len(exts.split(":=")[1].split()) == 11
    assert "-ffp-contract=off" in src


def test_make_rules_cross_compile_for_gfx950_without_scratch():
    r = subprocess.run(["make", "-C", CSRC, "fps", "fps-resources"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stdout + r.stderr
    assert "tsdf_fps_kernel" in text
    scratch = [ln for ln in text.splitlines() if "ScratchSize" in ln]
    # the four loaders: crop, mapped crop, float32 cloud, float64 cloud
    assert len(scratch) == 4 and all(ln.split("]:")[1].split()[0] == "0" for ln in scratch), scratch
    vgprs = [int(ln.split("VGPRs:")[1].split()[0]) for ln in text.splitlines() if " VGPRs:" in ln]
    lds = [int(ln.split("]:")[1].split()[0]) for ln in text.splitlines() if "LDS Size" in ln]
    assert len(vgprs) == 4 and max(vgprs) <= 128          # 1024 lanes: four waves a SIMD
    assert lds == [12 * fr.RESIDENT + 16 * 16 + 4 * 16] * 4 and lds[0] <= 160 * 1024
    unit = open(os.path.join(CSRC, "tsdf_fps.hip")).read()
    assert sorted(re.findall(r'#include "(\w+\.inc)"', unit)) == ["device.inc", "fps_host.inc", "prim.inc"]
    body = unit.split("namespace {", 1)[1]
    assert not re.search(r"atomic(Add|Max|Min|CAS|Exch|And|Or|Xor)", body) and "__device__ int" not in unit   # no globals
    assert "__builtin_fma" not in unit and "fma(" not in body and "printf" not in unit
    exchange = body.split("fps_key fps_group_max(", 1)[1].split("\n}\n", 1)[0]
    assert exchange.count("__syncthreads()") == 1 and body.count("fps_group_max(key") == 2   # one barrier per iteration
    for loop in body.split("for (; j < M; ++j) {")[1:]:
        assert "__syncthreads" not in loop.split("\n    }\n" if "kFpsSlots" in loop.split("fps_group_max")[0] else "\n  }\n", 1)[0]
    recorded = open(os.path.join(ROOT, "profiles", "fps", "resources.txt")).read()
    assert recorded.count("ScratchSize [bytes/lane]: 0") >= 4 and f"VGPRs: {max(vgprs)}" in recorded


def test_the_library_includes_the_same_text():
    unit = open(os.path.join(CSRC, "tsdf_fps.hip")).read()
    inc, main = (open(os.path.join(CSRC, f)).read() for f in ("fps_host.inc", "fps_host_main.cc"))
    theirs = open(os.path.join(CSRC, "device.inc")).read().splitlines()
    (line,) = [ln for ln in main.splitlines() if re.search(r"\bbool misaligned\(", ln)]
    assert line in theirs and "misaligned(" in inc and not re.search(r"\bbool misaligned\(", inc)   # used, not restated
    assert "cam_ok(" in inc and "bool cam_ok" not in inc and "bool cam_ok" not in main and '#include "prim.inc"' in main
    order = [unit.index(f'#include "{f}"') for f in ("device.inc", "prim.inc", "fps_host.inc")]
    assert order == sorted(order)
    for name in ("fps_defect(", "fps_points_defect(", "fps_plan(", "fps_holds(", "fps_slots(", "fps_segment("):
        assert name in unit and name in main, name
    assert f"constexpr int kFpsResident = {fr.RESIDENT};" in inc


def test_host_code_under_sanitizers_as_a_stand_alone_program():
    subprocess.check_call(["make", "-C", CSRC, "-B", "fps-host-asan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "build", "fps_host_asan")
    env = dict(os.environ)
    env.update(ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert f"fps host code ok (1024 lanes, cap {fr.RESIDENT}, 160 forms, " in r.stdout, tail
    assert "Sanitizer" not in tail and "runtime error" not in tail and "FAILED" not in tail, tail


# ---- the plan ----
def test_plan(pkg):
    L = pkg._lib.load_fps()
    cap, work, lds = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int()
    for M in (1, 128, 1024, 65536):
        for capacity in (0, 1, 76800, 2 ** 31 - 1):
            for hint in (0, 1):
                assert L.tsdf_fps_plan(M, capacity, hint, cap, work, lds) == 0
                assert (cap.value, work.value, lds.value) == (fr.RESIDENT, 16 * capacity, 12 * fr.RESIDENT + 320)
                assert pkg.fps_plan(M, capacity, hint) == (fr.RESIDENT, 16 * capacity, lds.value)
    assert cap.value >= 8192 and lds.value <= 160 * 1024
    assert pkg.FPS_RESIDENT_POINTS == fr.RESIDENT and "FPS_RESIDENT_POINTS" in pkg.__all__
    for bad in ((0, 0, 0), (65537, 0, 0), (-1, 0, 0), (1024, -1, 0), (1024, 2 ** 31, 0), (1024, 0, 2), (1024, 0, -1)):
        assert L.tsdf_fps_plan(*bad, cap, work, lds) == INVALID, bad
        with pytest.raises(ValueError):
            pkg.fps_plan(*bad)
    assert L.tsdf_fps_plan(1024, 0, 0, None, work, lds) == INVALID and L.tsdf_fps_plan(1024, 0, 0, cap, work, None) == INVALID
    # the restated form rule is the library's (the stand-alone program checks the library's own)
    assert [fr.holds(c, k, f) for c, k, f in ((5, 0, 0), (5, 4, 1), (5, 5, 1), (fr.RESIDENT + 1, 0, 0),
                                              (fr.RESIDENT + 1, fr.RESIDENT + 1, 0), (fr.RESIDENT, BIG, 0))] == [1, 1, 2, 0, 2, 1]


# ---- refusals ----
null, one, odd8, odd4, odd2 = (ctypes.c_void_p(v) for v in (0, 64, 72, 68, 66))
nan, inf = float("nan"), float("inf")


def _entries(pkg):
    """The two entries on dummy pointers (64: aligned for every check), every argument good unless named."""
    L = pkg._lib.load_fps()

    def crop(depth=one, depth_len=100, offsets=one, headers=one, n_src=3, index=one, n=3, M=1024, focal=241.42, cx=160.0,
             cy=120.0, eps=1.0, trunc=3.0, capacity=100, hint=0, xforms=one, work=one, points=one, pixel=one, radius2=one,
             count=one, status=one):
        return L.tsdf_fps_hip(depth, depth_len, offsets, headers, n_src, index, n, M, focal, cx, cy, eps, trunc, capacity,
                              hint, null, xforms, work, points, pixel, radius2, count, status)

    def cloud(cloud=one, dtype=1, n=3, P=6000, M=1024, capacity=100, hint=0, work=one, points=one, pixel=one, radius2=one,
              count=one, status=one):
        return L.tsdf_fps_points_hip(cloud, dtype, n, P, M, capacity, hint, null, work, points, pixel, radius2, count, status)
    return crop, cloud


SHAPE = [dict(n=-1), dict(M=0), dict(M=-1), dict(M=65537), dict(hint=2), dict(hint=-1), dict(capacity=-1),
         dict(capacity=2 ** 31)]                                                       # refused whatever n is
OUTS = [dict(points=null), dict(pixel=null), dict(count=null), dict(status=null), dict(work=null), dict(capacity=0),
        dict(work=odd8), dict(work=odd4), dict(n=2 ** 22)]                             # ... with n > 0; n == 0 is a no-op
CROP = [dict(depth=null), dict(offsets=null), dict(headers=null), dict(depth_len=-1), dict(n_src=0), dict(n_src=-5),
        dict(index=null, n_src=4), dict(xforms=odd4),
        *[dict([(k, v)]) for k in ("focal", "eps", "trunc") for v in (0.0, -0.0, -1.0, nan, -inf)]]
CLOUD_FIRST = [dict(dtype=2), dict(dtype=-1), dict(P=0), dict(P=-1), dict(P=2 ** 31)]
CLOUD = [dict(cloud=null), dict(cloud=odd4), dict(cloud=odd2, dtype=0)]


def test_every_defect_is_refused_before_device_work(pkg):
    crop, cloud = _entries(pkg)
    for fn, first, later in ((crop, SHAPE, OUTS + CROP), (cloud, SHAPE + CLOUD_FIRST, OUTS + CLOUD)):
        for kw in first:
            assert fn(**kw) == INVALID, kw
            if "n" not in kw:
                assert fn(n=0, **kw) == INVALID, kw
        for kw in later:
            assert fn(**kw) == INVALID, kw
            if "n" not in kw:
                assert fn(n=0, **kw) == 0, kw
        assert fn(n=0) == 0


# Good arguments reach check_device.  On a machine WITH a device they would launch on the dummy pointers, so this row is
# checked where the device check answers -2.
@pytest.mark.skipif(torch.cuda.is_available(), reason="good arguments with dummy pointers must stop at the device check")
def test_good_arguments_get_as_far_as_the_device(pkg):
    crop, cloud = _entries(pkg)
    assert crop() == NO_DEVICE and cloud() == NO_DEVICE
    for M in (1, 128, 65536):
        for hint in (0, 1):
            assert crop(M=M, hint=hint) == NO_DEVICE and cloud(M=M, hint=hint) == NO_DEVICE
    assert crop(xforms=null) == NO_DEVICE and crop(radius2=null) == NO_DEVICE and crop(index=null) == NO_DEVICE
    assert crop(work=null, capacity=0) == NO_DEVICE and cloud(work=null, capacity=0) == NO_DEVICE
    assert crop(n=2 ** 22 - 1) == NO_DEVICE and crop(depth_len=0) == NO_DEVICE and crop(cx=nan, cy=-inf) == NO_DEVICE
    assert cloud(dtype=0, cloud=odd4) == NO_DEVICE and cloud(P=2 ** 31 - 1) == NO_DEVICE and cloud(radius2=null) == NO_DEVICE
    assert crop(capacity=2 ** 31 - 1) == NO_DEVICE


# ---- Python wrappers ----
@pytest.fixture()
def V():
    return importlib.import_module(PKG + ".voxelize")


def V_dev_check(name, t, dtype):
    """``_dev_check`` without "lives on the GPU": the rest of it is under test."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def test_public_names_and_refusals(pkg, V, monkeypatch):
    log = []
    monkeypatch.setattr(V, "_call", lambda *a, **kw: log.append(a))
    for name in ("farthest_points", "farthest_of", "FpsBatch", "fps_plan", "FPS_RESIDENT_POINTS"):
        assert name in pkg.__all__ and hasattr(pkg, name) and name in pkg.__doc__, name
    assert "tsdf_fps.h" in pkg.__doc__ and "libtsdf_fps.so" in pkg.__doc__ and "AugmentedStep(fps=" in pkg.__doc__
    assert list(inspect.signature(pkg.farthest_points).parameters) == [
        "depth", "offsets", "headers", "points", "cam", "xforms", "index", "capacity", "work", "out", "form"]
    assert list(inspect.signature(pkg.farthest_of).parameters) == ["cloud", "points", "capacity", "work", "out", "form"]
    assert inspect.signature(pkg.farthest_points).parameters["points"].default == 1024
    params = inspect.signature(pkg.AugmentedStep.__init__).parameters
    assert list(params)[-3:] == ["fps", "occupancy", "tsdf"] and params["fps"].default is None
    assert pkg.FpsBatch._fields == ("points", "pixel", "radius2", "count", "status")
    for word in ("obb_xforms(", "xforms=obb.xforms", "normalize_joints(fps.points.view(n, -1)"):
        assert word in pkg.farthest_points.__doc__, word
    pack = torch.rand(30), torch.tensor([0, 10, 20, 30]), torch.zeros((3, 6), dtype=torch.int32)
    cloud = torch.rand(3, 50, 3)
    # there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        pkg.farthest_points(*pack)
    with pytest.raises(ValueError, match="GPU"):
        pkg.farthest_of(cloud)
    # everything else, with the device check out of the way: judged before the launch
    monkeypatch.setattr(V, "_dev_check", lambda name, t, dtype, device=None, host_ok=False: V_dev_check(name, t, dtype))
    for fn in (lambda **kw: pkg.farthest_points(*pack, **kw), lambda **kw: pkg.farthest_of(cloud, **kw)):
        for bad in (0, -1, 65537, 128.0, True, "128", None):
            with pytest.raises(ValueError, match="points must be"):
                fn(points=bad)
        for bad in (2, -1, True, 0.0, "0", None):
            with pytest.raises(ValueError, match="form must be"):
                fn(form=bad)
        for bad in (0, -1, 2 ** 31, 100.0, True, "100"):
            with pytest.raises(ValueError, match="capacity must be"):
                fn(capacity=bad)
        for bad in (torch.zeros((3, 100, 3)), torch.zeros((2, 100, 4)), torch.zeros((3, 100, 4), dtype=torch.float64),
                    torch.zeros((3, 0, 4)), torch.zeros((300, 4)), torch.zeros((3, 101, 4))[:, 1:], "work"):
            with pytest.raises(ValueError):
                fn(work=bad)
        with pytest.raises(ValueError, match="is not work's"):
            fn(work=torch.zeros((3, 100, 4)), capacity=99)
        good = V._fps_out(None, 3, 16, torch.device("cpu"))
        for bad in (good._replace(points=torch.zeros((3, 16, 4))), good._replace(pixel=torch.zeros((3, 16))),
                    good._replace(radius2=torch.zeros((3, 15))), good._replace(count=torch.zeros(3)),
                    good._replace(status=torch.zeros(4, dtype=torch.int32)), tuple(good), "out"):
            with pytest.raises(ValueError):
                fn(points=16, out=bad)
    for kw in (dict(xforms=torch.rand(3, 24)), dict(xforms=torch.rand((3, 12), dtype=torch.float64)),
               dict(index=torch.tensor([[0, 1, 2]])), dict(index=torch.tensor([0, 1, 2], dtype=torch.int32)),
               dict(index=torch.tensor([0, 1]), xforms=torch.rand((3, 24), dtype=torch.float64))):
        with pytest.raises(ValueError):
            pkg.farthest_points(*pack, **kw)
    for bad in (pack[0].double(), pack[0].numpy(), None):                # not a float32 tensor: a ValueError all the same
        with pytest.raises(ValueError):
            pkg.farthest_points(bad, pack[1], pack[2])
    for bad in (cloud.half(), cloud.numpy(), None, torch.rand(3, 50, 2), torch.rand(50, 3), torch.rand(3, 0, 3), cloud.transpose(0, 1)):
        with pytest.raises(ValueError):
            pkg.farthest_of(bad)
    assert log == []                                                    # refused before anything is launched
    # a good call is one launch of the entry, the stream at position 15; without a capacity nothing but outputs exists
    xf, index = torch.rand((2, 24), dtype=torch.float64), torch.tensor([2, 0])
    out = pkg.farthest_points(*pack, points=7, xforms=xf, index=index)
    (dev, fn, args, stream_at), = log
    assert fn.__name__ == "tsdf_fps_hip" and stream_at == 15 and len(args) == 23 and args[15] is None
    assert args[4:8] == [3, index.data_ptr(), 2, 7] and args[8:13] == [241.42, 160.0, 120.0, 1.0, 3.0] and args[13:15] == [0, 0]
    assert args[16] == xf.data_ptr() and args[17] is None
    assert args[18:] == [t.data_ptr() for t in out] and isinstance(out, pkg.FpsBatch)
    assert [tuple(t.shape) for t in out] == [(2, 7, 3), (2, 7), (2, 7), (2,), (2,)]
    assert [t.dtype for t in out] == [torch.float32, torch.int32, torch.float32, torch.int32, torch.int32]
    del log[:]
    work = torch.zeros((3, 40, 4))
    again = pkg.farthest_points(*pack, points=7, work=work, form=1)
    args = log[0][2]
    assert args[13:15] == [40, 1] and args[17] == work.data_ptr() and args[16] is None and again.points.shape == (3, 7, 3)
    del log[:]
    pkg.farthest_points(*pack, points=7, capacity=55)
    assert log[0][2][13] == 55 and log[0][2][17] is not None
    # the cloud entry: the stream at position 7, the element type from the tensor
    for c, code in ((cloud, 0), (cloud.double(), 1)):
        del log[:]
        kept = V._fps_out(None, 3, 9, torch.device("cpu"))._replace(radius2=None)
        got = pkg.farthest_of(c, points=9, out=kept)
        (dev, fn, args, stream_at), = log
        assert fn.__name__ == "tsdf_fps_points_hip" and stream_at == 7 and len(args) == 14 and got is kept
        assert args[:7] == [c.data_ptr(), code, 3, 50, 9, 0, 0] and args[8] is None and args[11] is None
        assert args[9] == kept.points.data_ptr() and args[12:] == [kept.count.data_ptr(), kept.status.data_ptr()]
    # an empty batch launches nothing
    del log[:]
    empty = pkg.farthest_of(torch.zeros((0, 5, 3)), points=4)
    assert log == [] and empty.points.shape == (0, 4, 3)


# ---- AugmentedStep(fps=...) through stubbed primitives ----
N, R8 = 3, 8
BF16 = torch.bfloat16
STUBBED = ("aug_xforms_at", "map_step_head", "voxelize_indexed", "map_grids", "_map_grid_lowp", "_map_grid_accurate",
           "narrow_volumes", "transform_joints", "normalize_joints", "joint_heatmaps", "aabb", "_occupancy", "_fps_crop")


class Rec:
    """Recorders in the style of tests/test_occupancy_cpu.py: ``log`` holds (name, arguments by parameter name) of every
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
# what the step launches without fps=, configuration by configuration (AugmentedStep's docstring, option by option)
CONFIGS = {
    "plain": (dict(), ["aug_xforms_at", "voxelize_indexed"]),
    "dtype_gt": (dict(dtype=BF16, gt=True), ["aug_xforms_at", "map_grids", "_map_grid_lowp"] + LABELS),
    "head": (dict(fused_head=True, gt=True), ["map_step_head", "voxelize_indexed"]),
    "base_dtype": (dict(base=True, dtype=torch.float16, gt=True), ["map_step_head", "_map_grid_lowp"]),
    "accurate": (dict(tsdf="accurate"), ["aug_xforms_at", "map_grids", "_map_grid_accurate"]),
    "heatmap_occupancy": (dict(gt=True, heatmap=(12, 1.7), occupancy=(16,)),
                          ["aug_xforms_at", "voxelize_indexed", "joint_heatmaps", "_occupancy"]),
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
    assert rec.names() == want and s.cloud is None and s.cloud_pixel is None and s.cloud_status is None
    del rec.log[:]
    s, _ = _step(V, kw, fps=None)
    assert rec.names() == want                                          # fps=None: the launches there were
    for fps in ((64,), [1024]):
        del rec.log[:]
        s, pack = _step(V, kw, fps=fps)
        assert rec.names() == want + ["_fps_crop"]                      # one more, and it is the last
        a = rec.log[-1][1]
        assert all(a[k] is t for k, t in zip(("depth", "offsets", "headers"), pack))
        assert a["xforms"] is s.xforms and a["index"] is s.index and a["cam"] is None
        assert (a["points"], a["capacity"], a["work"], a["form"]) == (fps[0], None, None, 0)
        out = a["out"]
        assert out.points is s.cloud and out.pixel is s.cloud_pixel and out.radius2 is None
        assert out.count is s.cloud_count and out.status is s.cloud_status
        assert s.cloud.shape == (N, fps[0], 3) and s.cloud_pixel.shape == (N, fps[0]) and s.cloud_status.dtype is torch.int32
        del rec.log[:]
        s._run()                                                        # what a step without a graph issues
        assert rec.names() == want + ["_fps_crop"] and rec.log[-1][1]["out"].points is s.cloud


def test_augmented_step_refuses_a_bad_fps_before_anything(V, monkeypatch):
    rec = Rec(V, monkeypatch)
    for bad, what in (((), "fps must be"), (64, "fps must be"), ((64, 1), "fps must be"), ((0,), "points must be"),
                      ((65537,), "points must be"), ((None,), "points must be"), ((64.0,), "points must be")):
        with pytest.raises(ValueError, match=what):
            _step(V, {}, fps=bad)
    assert rec.log == []
