"""CPU tier of the hand locator (include/tsdf_locate.h): libtsdf_locate.so as far as it goes without a GPU — the build rule
and its resource report, the binding through _lib._EXTS, the version, every argument check before device work —, the
public names and their refusals, and the reference the GPU tier compares against (tests/locate_ref.py): the margin
condition on every input the GPU tier compares exactly, the round trip, the capacity bound, refine = 0, the cube row.
Nothing here touches a GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import locate_ref as lr  # noqa: E402
from abi_util import declared_functions, exported  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "handposeestimation-with-3d-cnns_amd", "csrc")
INVALID, NO_DEVICE = -1, -2
WANT = ["tsdf_locate_capacity", "tsdf_locate_hip", "tsdf_locate_version"]
NAN = float("nan")
# a good call with dummy pointers would launch on them where there is a device: "valid arguments get as far as the device
# check" is asserted where that check answers -2; the refusals are asserted everywhere (they return before the device)
NO_GPU = not torch.cuda.is_available()


# ---- build rule ----
def test_make_rules_cross_compile_for_gfx950_without_scratch():
    r = subprocess.run(["make", "-C", CSRC, "locate", "locate-resources"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stdout + r.stderr
    names = [ln for ln in text.splitlines() if "Function Name" in ln]
    # the locating kernel and the copy for float32 and uint16 frames, and the scan
    for kernel, times in (("tsdf_locate_kernel", 2), ("tsdf_locate_scan_kernel", 1), ("tsdf_locate_copy_kernel", 2)):
        assert sum(kernel in ln for ln in names) == times, (kernel, names)
    scratch = [ln for ln in text.splitlines() if "ScratchSize" in ln]
    assert len(scratch) == 5 and all(ln.split("]:")[1].split()[0] == "0" for ln in scratch), scratch
    # the committed report says the same
    report = open(os.path.join(ROOT, "profiles", "locate", "resources.txt")).read()
    committed = [ln for ln in report.splitlines() if "ScratchSize" in ln]
    assert len(committed) == 5 and all(ln.split("]:")[1].split()[0] == "0" for ln in committed), committed


# ---- binding ----
def test_row_binds_exactly_its_header_with_types(pkg):
    ext = pkg._lib._EXTS["locate"]
    assert isinstance(ext, pkg._lib._Ext)
    assert declared_functions("tsdf_locate.h") == WANT == sorted([ext.version_symbol, *ext.entries])
    funcs, named = exported(pkg._lib.LOCATE_LIB_PATH)
    assert funcs == WANT and named == WANT
    assert ext.path == pkg._lib.LOCATE_LIB_PATH and ext.version == pkg._lib.LOCATE_VERSION == 1
    L = pkg._lib.load_locate()
    assert L.tsdf_locate_version() == 1
    for entry in (ext.version_symbol, *ext.entries):
        fn = getattr(L, entry)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, entry
    vp, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    f64, f32 = ctypes.c_double, ctypes.c_float
    assert list(L.tsdf_locate_capacity.argtypes) == [i, i, f32, f32, f64, ctypes.POINTER(i64)]
    assert list(L.tsdf_locate_hip.argtypes) == [vp, i, i, i64, i, i, vp, i, f32, f32, f32, f32, i, i, f64, f64, f64, f32, f32,
                                                i64, vp] + [vp] * 9
    for name, args in ext.entries.items():
        assert list(getattr(L, name).argtypes) == args and args
    assert pkg._lib.load_locate() is L and L is not pkg._lib.load() and L is not pkg._lib.load_mapstep()
    # the header's own text: the camera comes by value, so no declaration of it names the camera struct
    text = open(os.path.join(ROOT, "include", "tsdf_locate.h")).read()
    assert "tsdf_cam" not in text
    assert (pkg._lib.TSDF_LOCATE_F32, pkg._lib.TSDF_LOCATE_U16) == (0, 1)
    assert "#define TSDF_LOCATE_F32 0" in text and "#define TSDF_LOCATE_U16 1" in text
    # the product beside it is what it was
    assert pkg._lib.load().tsdf_version() == 7


# ---- argument checks ----
def _caller(L):
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)

    def call(frames=one, frame_type=0, shift=0, n_src=1, H=30, W=41, index=null, n=1, near=100.0, far=1500.0, cube=250.0,
             band=150.0, refine=2, R=32, cam=(241.42, 160.0, 120.0, 1.0, 3.0), capacity=None, depth=one, offsets=one,
             headers=one, com=one, count=one, status=one, grid=one, max_l=one, mid_p=one):
        if capacity is None:
            capacity = max(n, 1) * 41 * 30
        return L.tsdf_locate_hip(frames, frame_type, shift, n_src, H, W, index, n, near, far, cube, band, refine, R, *cam,
                                 capacity, null, depth, offsets, headers, com, count, status, grid, max_l, mid_p)
    return call, null, one


def test_argument_validation_happens_before_device_work(pkg):
    L = pkg._lib.load_locate()
    call, null, one = _caller(L)
    odd2, odd4 = ctypes.c_void_p(66), ctypes.c_void_p(68)
    assert call(n=-1) == INVALID
    for ft in (-1, 2, 7):
        assert call(frame_type=ft) == INVALID, ft
    for shift in (-1, 8, 100):
        assert call(frame_type=1, shift=shift) == INVALID, shift
    for kw in (dict(H=0), dict(H=-3), dict(W=0), dict(W=-1)):
        assert call(**kw) == INVALID, kw
    assert call(n_src=0, index=one) == INVALID and call(n_src=-3, index=one) == INVALID
    assert call(n_src=2) == INVALID and call(n=2) == INVALID                # no index: n_src must equal n
    for kw in (dict(near=0.0), dict(near=-1.0), dict(near=NAN), dict(far=99.0), dict(far=NAN), dict(far=-5.0),
               dict(cube=0.0), dict(cube=-250.0), dict(cube=NAN), dict(band=-1.0), dict(band=NAN), dict(band=-1e-30)):
        assert call(**kw) == INVALID, kw
    for refine in (-1, 9, 100):
        assert call(refine=refine) == INVALID, refine
    for R in (0, 2, 3, 6, 30, 132, 256, -4):
        assert call(R=R) == INVALID, R
        assert call(R=R, grid=null, max_l=null, mid_p=null) == INVALID, R   # R is checked whether or not it is used
    # the camera comes by value and goes through the camera rule of every entry (csrc/prim.inc::cam_ok)
    for bad in ((0.0, 160.0, 120.0, 1.0, 3.0), (-1.0, 160.0, 120.0, 1.0, 3.0), (NAN, 160.0, 120.0, 1.0, 3.0),
                (241.42, 160.0, 120.0, 0.0, 3.0), (241.42, 160.0, 120.0, -1.0, 3.0), (241.42, 160.0, 120.0, NAN, 3.0),
                (241.42, 160.0, 120.0, 1.0, 0.0), (241.42, 160.0, 120.0, 1.0, NAN), (241.42, 160.0, 120.0, 1.0, -0.0)):
        assert call(cam=bad) == INVALID, bad
        assert call(cam=bad, grid=null, max_l=null, mid_p=null) == INVALID, bad
        assert call(cam=bad, n=0, n_src=0) == 0, bad
    for name in ("frames", "depth", "offsets", "headers", "com", "count", "status"):
        assert call(**{name: null}) == INVALID, name
    assert call(grid=null) == INVALID                                       # max_l and mid_p need the grid
    assert call(grid=null, max_l=null) == INVALID and call(grid=null, mid_p=null) == INVALID
    # alignment: the frames and the depth to their element, the centre and the offsets to 8 bytes
    assert call(frames=odd2) == INVALID and call(depth=odd2) == INVALID and call(depth=ctypes.c_void_p(65)) == INVALID
    assert call(frames=ctypes.c_void_p(65), frame_type=1) == INVALID
    assert call(com=odd4) == INVALID and call(offsets=odd4) == INVALID
    # the capacity rule: s = floor(250 * 241.42 / 100) + 2 = 605 exceeds both sides of a 41 x 30 frame
    assert call(capacity=41 * 30 - 1) == INVALID and call(capacity=0) == INVALID and call(capacity=-5) == INVALID
    assert call(n=3, n_src=3, capacity=3 * 41 * 30 - 1) == INVALID
    # ... and a small cube's is smaller than the frame: s = floor(10 * 30 / 100) + 2 = 5
    small = dict(cube=10.0, cam=(30.0, 20.3, 15.1, 1.0, 3.0))
    assert call(capacity=24, **small) == INVALID
    if NO_GPU:   # valid arguments get as far as the device, and there is none here
        assert call() == NO_DEVICE
        assert call(capacity=25, **small) == NO_DEVICE
        assert call(n=3, n_src=3, capacity=3 * 41 * 30) == NO_DEVICE
        assert call(frames=odd2, frame_type=1, shift=7) == NO_DEVICE        # uint16 frames are 2-byte aligned
        assert call(frame_type=0, shift=99) == NO_DEVICE                    # the shift belongs to uint16 frames
        assert call(grid=null, max_l=null, mid_p=null) == NO_DEVICE
        assert call(max_l=null, mid_p=null) == NO_DEVICE
        assert call(n_src=5, index=one, n=3, capacity=3 * 41 * 30) == NO_DEVICE
        assert call(near=100.0, far=100.0, band=0.0, refine=0) == NO_DEVICE and call(refine=8) == NO_DEVICE
        assert call(far=float("inf")) == NO_DEVICE
        for good in ((588.03, 320.5, 240.25, 0.5, 2.0), (241.42, NAN, -7.0, 1e-3, 8.0)):   # cx, cy are not judged
            assert call(cam=good) == NO_DEVICE, good
        for R in (4, 12, 64, 128):
            assert call(R=R) == NO_DEVICE, R
        assert call(H=2 ** 31 - 1, W=2 ** 31 - 1, capacity=605 * 605) == NO_DEVICE   # sizes are 64-bit throughout


def test_n_zero_is_a_no_op_whatever_else_is_passed(pkg):
    L = pkg._lib.load_locate()
    call, null, one = _caller(L)
    assert call(n=0, n_src=0) == 0
    assert call(n=0, frame_type=9, shift=-3, H=0, W=-1, near=NAN, cube=-1.0, refine=99, R=5, capacity=-1) == 0
    assert L.tsdf_locate_hip(null, 0, 0, 0, 0, 0, null, 0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, null, null, null,
                             null, null, null, null, null, null, null) == 0


def test_capacity_rule(pkg):
    L = pkg._lib.load_locate()
    per = ctypes.c_int64(-1)

    def cap(H, W, cube, near, focal):
        rc = L.tsdf_locate_capacity(H, W, cube, near, focal, ctypes.byref(per))
        return rc, per.value

    assert cap(240, 320, 250.0, 100.0, 241.42) == (0, 320 * 240)            # s = 605
    assert cap(480, 640, 250.0, 100.0, 588.04) == (0, 640 * 480)            # s = 1472
    assert cap(480, 640, 250.0, 400.0, 588.04) == (0, 369 * 369)            # s = floor(367.525) + 2
    assert cap(30, 41, 10.0, 100.0, 30.0) == (0, 25)
    assert cap(30, 41, 1e30, 1e-30, 1e300) == (0, 41 * 30)                  # an enormous quotient is the whole frame
    for H, W, cube, near, focal in ((240, 320, 250.0, 100.0, 241.42), (48, 64, 150.0, 100.0, 48.0), (30, 41, 77.7, 312.5, 30.0)):
        assert cap(H, W, cube, near, focal) == (0, lr.capacity(H, W, cube, near, focal))
    for bad in ((0, 41, 250.0, 100.0, 30.0), (30, -1, 250.0, 100.0, 30.0), (30, 41, 0.0, 100.0, 30.0), (30, 41, NAN, 100.0, 30.0),
                (30, 41, 250.0, 0.0, 30.0), (30, 41, 250.0, NAN, 30.0), (30, 41, 250.0, 100.0, 0.0), (30, 41, 250.0, 100.0, NAN)):
        assert cap(*bad)[0] == INVALID, bad
    assert L.tsdf_locate_capacity(30, 41, 250.0, 100.0, 30.0, None) == INVALID


# ---- public names and refusals ----
def test_public_names_and_refusals(pkg):
    for name in ("locate_hands", "voxelize_frames", "HandCrops"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
        assert name in pkg.__doc__ or name == "HandCrops", name   # (the docstring lists functions, not result types)
    assert "tsdf_locate.h" in pkg.__doc__
    assert pkg.HandCrops._fields == ("depth", "offsets", "headers", "com", "count", "status", "grid", "max_l", "mid_p")
    frames = torch.from_numpy(lr.frames_of("64x48")[:2])
    # there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        pkg.locate_hands(frames)
    with pytest.raises(ValueError, match="GPU"):
        pkg.voxelize_frames(frames)
    with pytest.raises(ValueError, match="GPU"):
        pkg.locate_hands(torch.zeros((2, 48, 64), dtype=torch.uint16), shift=3)
    # the wrong type, shape, layout in memory, encoding
    with pytest.raises(TypeError, match="float32 or torch.uint16"):
        pkg.locate_hands(frames.to(torch.float64))
    with pytest.raises(TypeError, match="float32 or torch.uint16"):
        pkg.locate_hands(frames.to(torch.int16), shift=0)
    with pytest.raises(TypeError, match="torch.Tensor"):
        pkg.locate_hands(lr.frames_of("64x48")[:2])
    with pytest.raises(ValueError, match=r"\[N, H, W\]"):
        pkg.locate_hands(frames[0])
    with pytest.raises(ValueError, match="contiguous"):
        pkg.locate_hands(frames[:, :, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        pkg.locate_hands(frames.transpose(1, 2))
    u16 = torch.zeros((2, 48, 64), dtype=torch.uint16)
    with pytest.raises(ValueError, match="shift"):
        pkg.locate_hands(u16)
    for shift in (-1, 8, 1.0, True):
        with pytest.raises(ValueError, match="shift"):
            pkg.locate_hands(u16, shift=shift)
    with pytest.raises(ValueError, match="shift"):
        pkg.locate_hands(frames, shift=3)
    with pytest.raises(ValueError, match="resolution"):
        pkg.locate_hands(frames, res=30)
    with pytest.raises(ValueError, match="placement"):
        pkg.voxelize_frames(frames, placement="obb")
    with pytest.raises(ValueError, match="layout"):
        pkg.voxelize_frames(frames, layout="xyz")
    with pytest.raises(ValueError, match="dtype"):
        pkg.voxelize_frames(frames, dtype=torch.float32)
    with pytest.raises(TypeError, match="grid and res"):
        pkg.voxelize_frames(frames, grid=False)


# ---- the reference, on the inputs of the GPU tier ----
def _all_references():
    """(label, reference dict) for every frame the GPU tier compares exactly."""
    for name in lr.SETS:
        for k, r in enumerate(lr.reference(name)):
            yield f"{name}[{k}]", r
    for k, r in enumerate(lr.reference("64x48", refine=0)):
        yield f"64x48 refine=0 [{k}]", r
    for k, r in lr.edge_reference().items():
        yield k, r
    for k, r in enumerate(lr.other_camera_reference()):
        yield f"other camera [{k}]", r
    p = dict(lr.PARAMS)
    for k, f in enumerate(lr.frames_q1()):
        yield f"q1[{k}]", lr.locate_frame(f, lr.CAM_MID, **p)


def test_margin_condition_holds_on_every_gpu_input():
    worst = min(((r["margin"], label) for label, r in _all_references()), key=lambda t: t[0])
    print(f"smallest decision margin over the GPU tier's inputs: {worst[0]:.3g} ({worst[1]})")
    for label, r in _all_references():
        assert r["margin"] >= lr.MARGIN, (label, r["margin"])


def test_round_trip_kept_set_is_the_hand_and_rectangle_holds_the_tight_box():
    for name, (H, W, cam, _) in lr.SETS.items():
        s = lr.capacity_side(lr.PARAMS["cube"], lr.PARAMS["near"], cam[0])
        for sc, r in zip(lr.scenes(name), lr.reference(name)):
            assert r["status"] == 0 and np.array_equal(r["keep"], sc["hand"]), name
            left, top, right, bottom = r["rect"]
            bl, bt, br, bb = sc["box"]
            assert left <= bl and top <= bt and right >= br and bottom >= bb, (name, r["rect"], sc["box"])
            # the projected centre is inside the rectangle, and no side exceeds the capacity bound
            u = r["com"][0] * cam[0] / -r["com"][2] + cam[1]
            v = -r["com"][1] * cam[0] / -r["com"][2] + cam[2]
            assert left <= u < right and top <= v < bottom
            assert right - left <= min(W, s) and bottom - top <= min(H, s)
            assert r["crop"].size == (right - left) * (bottom - top) <= lr.capacity(H, W, 250.0, 100.0, cam[0])
            # the crop is the hand's pixels where they were and +0 elsewhere: what a tight MSRA crop holds, in a larger box
            d, hdr = lr.tight_crop(sc)
            full = np.zeros((H, W), np.float32)
            full[hdr[3]:hdr[5], hdr[2]:hdr[4]] = d.reshape(hdr[5] - hdr[3], hdr[4] - hdr[2])
            assert np.array_equal(r["crop"].reshape(bottom - top, right - left), full[top:bottom, left:right])
    # corner scenes are among them: a rectangle clipped by the image
    assert any(r["rect"][0] == 0 or r["rect"][1] == 0 or r["rect"][2] == 41 or r["rect"][3] == 30 for r in lr.reference("41x30"))


def test_refine_zero_is_the_seed_centre_and_refinement_reaches_the_hand():
    for sc, r0, r2 in zip(lr.scenes("64x48"), lr.reference("64x48", refine=0), lr.reference("64x48")):
        d = sc["frame"]
        valid = lr.valid_mask(d, lr.CAM_MID)
        seed = valid & (d.astype(np.float64) <= np.float64(d[valid].min()) + 150.0)
        c, N, _ = lr.centre(d.astype(np.float64), seed, lr.CAM_MID)
        assert np.array_equal(r0["com"], c) and len(r0["centres"]) == 1 and r0["centres"][0][1] == N
        assert r0["rect"] == lr.rect_of(c, 48, 64, lr.CAM_MID)[0]
        assert len(r2["centres"]) == 3
    # background inside the seed band: the seed set holds the patch, the refined set is the hand
    sc, r = lr.scene_with_patch(), lr.edge_reference()["background inside the seed band"]
    assert r["centres"][0][1] == int(sc["hand"].sum()) + 16 and np.array_equal(r["keep"], sc["hand"])
    # seed_band == 0 is every valid pixel
    frame, _ = lr.edge_cases()["seed_band 0, refine 0"]
    r = lr.edge_reference()["seed_band 0, refine 0"]
    assert r["centres"][0][1] == int(lr.valid_mask(frame, lr.CAM_MID).sum())
    # the degenerate frames
    for k in ("all zero", "all NaN", "nearer than near", "beyond far"):
        r = lr.edge_reference()[k]
        assert r["status"] == 1 and r["rect"] == (0, 0, 1, 1) and r["count"] == 0 and r["crop"].tolist() == [0.0]


def test_cube_row_is_the_float32_glue_with_max_l_cube():
    # written out, operation by operation
    c = np.array([12.3456789, -45.678901, -432.10987], np.float64)
    for R, cube, tv in ((32, 250.0, 3.0), (16, 300.0, 2.0), (64, 187.3, 3.5)):
        row, max_l, mid = lr.glue_cube(c, cube, R, tv)
        f = np.float32
        vl = f(f(cube) / f(R))
        assert row.dtype == np.float32 and max_l == f(cube) and np.array_equal(mid, c.astype(f))
        assert row[3] == vl and row[4] == f(vl * f(tv)) and not row[5:].any()
        for k in range(3):
            assert row[k] == f(f(mid[k] - f(f(cube) / f(2))) + f(vl / f(2)))
    # and against the oracle's glue, where an AABB says exactly the same thing: extremes mid -+ cube / 2 with everything a
    # small integer, so that (mn + mx) / 2 and mx - mn are exact
    mid = np.array([40.0, -70.0, -432.0], np.float32)
    for R in (16, 32):
        for cam in (None, (241.42, 160.0, 120.0, 1.0, 2.0)):
            g, ori = oracle.glue(mid - np.float32(125.0), mid + np.float32(125.0), R, cam)
            row, max_l, m = lr.glue_cube(mid.astype(np.float64), 250.0, R, 3.0 if cam is None else cam[4])
            assert np.array_equal(g[:3], m) and g[3] == max_l
            assert np.array_equal(row[:3], ori) and np.array_equal(row[3:5], g[4:6])
