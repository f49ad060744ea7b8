"""CPU tier of the camera tests: the one camera rule (csrc/prim.inc::cam_ok) at every entry that takes a tsdf_cam, the
restatements that gained camera parameters against what they returned without them, and the conditions on the inputs of
tests/test_camera_gpu.py, asserted on the references.  Nothing here touches a GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auggrid_ref as ar  # noqa: E402
import camera_ref as cr  # noqa: E402
import obb_ref as ob  # noqa: E402

torch = pytest.importorskip("torch")

INVALID, NO_DEVICE = -1, -2
NAN = float("nan")
GOOD = cr.FRACTIONAL
# a non-NULL camera whose focal, invalid_eps or trunc_voxels is not > 0
BAD = {
    "focal=0": (0.0, 160.0, 120.0, 1.0, 3.0), "focal=-1": (-1.0, 160.0, 120.0, 1.0, 3.0),
    "focal=nan": (NAN, 160.0, 120.0, 1.0, 3.0),
    "eps=0": (241.42, 160.0, 120.0, 0.0, 3.0), "eps=-1": (241.42, 160.0, 120.0, -1.0, 3.0),
    "eps=nan": (241.42, 160.0, 120.0, NAN, 3.0),
    "trunc=0": (241.42, 160.0, 120.0, 1.0, 0.0), "trunc=nan": (241.42, 160.0, 120.0, 1.0, NAN),
}


def _entries(pkg):
    """{entry: (function, arguments(n, cam))} for every C entry that takes a tsdf_cam: dummy non-NULL pointers (64: aligned
    for every check), one frame, R = 32, everything an entry requires present — so that the camera is the only thing a
    call can be refused for.  The by-value index is real host memory (it is the one pointer the host may read)."""
    lib = pkg._lib
    L, D = lib.load(), lib.load_debug()
    one = ctypes.c_void_p(64)
    h_index = (ctypes.c_int64 * 1)(0)
    host = ctypes.cast(h_index, ctypes.c_void_p)
    lab = lib.TsdfLabels(64, 21, 1, 64, None)
    pca = lib.TsdfPca(64, 64, 10, 64)
    keep = (h_index, lab, pca)
    labp, pcap = ctypes.byref(lab), ctypes.byref(pca)
    outs = [one, one, one, one]

    def pack(n, cam):      # depth, depth_len, offsets, headers, n, R, cam, layout, stream
        return [one, 100, one, one, n, 32, cam, 0, None]

    def indexed(n, cam, index=one):   # ... headers, n_pack, index, n, R, cam, layout, stream
        return [one, 100, one, one, 1, index, n, 32, cam, 0, None]

    def src(n, cam):       # the extensions' source tables: ... headers, n_src, index, n, R, cam
        return [one, 100, one, one, n, None, n, 32, cam]

    table = {
        "tsdf_voxelize_hip": (L, lambda n, c: pack(n, c) + outs),
        "tsdf_voxelize_labels_hip": (L, lambda n, c: pack(n, c) + outs + [labp]),
        "tsdf_voxelize_grid_hip": (L, lambda n, c: pack(n, c) + [one, one, one]),
        "tsdf_voxelize_aug_hip": (L, lambda n, c: pack(n, c) + [one] + outs),
        "tsdf_voxelize_aug_labels_hip": (L, lambda n, c: pack(n, c) + [one] + outs + [labp]),
        "tsdf_voxelize_labels_pca_hip": (L, lambda n, c: pack(n, c) + [None] + outs + [labp, pcap]),
        "tsdf_aabb_hip": (L, lambda n, c: [one, 100, one, one, n, 32, c, None, one, one, one, one]),
        "tsdf_voxelize_indexed_hip": (L, lambda n, c: indexed(n, c) + outs + [None]),
        "tsdf_voxelize_indexed_host_hip": (L, lambda n, c: indexed(n, c, host) + outs + [labp]),
        "tsdf_voxelize_indexed_aug_hip": (L, lambda n, c: indexed(n, c) + [one] + outs + [labp]),
        "tsdf_voxelize_indexed_pca_hip": (L, lambda n, c: indexed(n, c) + [one] + outs + [labp, pcap]),
        "tsdf_voxelize_indexed_host_pca_hip": (L, lambda n, c: indexed(n, c, host) + outs + [labp, pcap]),
        "tsdf_debug_pixmap_hip": (D, lambda n, c: pack(n, c) + [None, one, one, one]),
        # the seven that do not go through run()
        "tsdf_point_clouds_hip": (L, lambda n, c: [one, 100, one, one, n, 8, c, 0, 0, None, None, one, one, one]),
        "tsdf_cloud_grid_hip": (L, lambda n, c: [one, n, 8, 32, c, None, one, one, one, one, one]),
        "tsdf_voxelize_aug_grid_hip": (lib.load_auggrid(), lambda n, c: pack(n, c) + [one, one, one, one]),
        "tsdf_obb_xforms_hip": (lib.load_obb(), lambda n, c: [one, 100, one, one, n, c, None, one, one, one]),
        "tsdf_voxelize_grid_lowp_hip": (lib.load_lowp(), lambda n, c: src(n, c) + [0, 2, None, one, one, one]),
        "tsdf_map_place_hip": (lib.load_maplowp(), lambda n, c: src(n, c) + [None, one, one, one, one, one]),
        "tsdf_voxelize_map_grid_lowp_hip": (lib.load_maplowp(), lambda n, c: src(n, c) + [0, 2, None, one, one, one, one]),
    }
    return {name: (getattr(L_, name), args) for name, (L_, args) in table.items()}, keep


def test_the_table_names_every_entry_that_takes_a_camera(pkg):
    """Every function of the product and of the extension table whose argtypes hold a tsdf_cam pointer is in _entries."""
    lib = pkg._lib
    entries, _ = _entries(pkg)
    cam_p = ctypes.POINTER(lib.TsdfCam)
    want = {"tsdf_default_cam"}        # fills a camera in; it takes no constants
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    declared = set()
    for h in sorted(os.listdir(inc)):
        text = open(os.path.join(inc, h)).read()
        for m in re.finditer(r"\b(?:int|void)\s+(tsdf_\w+)\s*\(([^;{]*?)\)\s*;", text, re.S):
            if "tsdf_cam" in m.group(2):
                declared.add(m.group(1))
    assert declared - want == set(entries), sorted(declared ^ set(entries))
    for name, (fn, args) in entries.items():
        assert cam_p in list(fn.argtypes), name
        assert len(args(1, None)) == len(fn.argtypes), name


# The calls below reach check_device when the camera is good.  On a machine WITH a device a good call would launch on the
# dummy pointers, so the pair (good -> not refused, bad -> refused) is checked where the device check answers -2.
@pytest.mark.skipif(torch.cuda.is_available(), reason="a good camera with dummy pointers must stop at the device check")
def test_a_bad_camera_is_refused_at_every_entry_and_a_good_one_is_not(pkg):
    lib = pkg._lib
    entries, keep = _entries(pkg)
    assert len(entries) == 20
    for name, (fn, args) in entries.items():
        good = lib.TsdfCam(*GOOD)
        # good -> not -1: here the device check's answer; NULL is the default camera
        assert fn(*args(1, ctypes.byref(good))) == NO_DEVICE, name
        assert fn(*args(1, None)) == NO_DEVICE, name
        for label, v in BAD.items():
            bad = lib.TsdfCam(*v)
            assert fn(*args(1, ctypes.byref(bad))) == INVALID, (name, label)
            # n == 0 stays a no-op whatever the camera
            assert fn(*args(0, ctypes.byref(bad))) == 0, (name, label)
        # the rule covers the whole struct: each field alone is enough, whichever fields the entry reads
        for field in ("focal", "invalid_eps", "trunc_voxels"):
            cam = lib.TsdfCam(*GOOD)
            setattr(cam, field, -0.0)
            assert fn(*args(1, ctypes.byref(cam))) == INVALID, (name, field)
    assert keep


@pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers: a call that is not refused must stop at the device check")
def test_the_refusal_is_reported_under_the_entrys_name(pkg):
    """What voxelize_grid_lowp(cam=bad) raises: the status of the entry, turned into a TsdfError by _lib.check as _call
    does it (CPU tensors are refused before any entry is called, so the entry is called here as the wrapper calls it).
    voxelize_lowp(cam=bad) used to be refused by its aabb half alone."""
    lib = pkg._lib
    bad = lib.TsdfCam(*BAD["eps=nan"])
    rc = lib.load_lowp().tsdf_voxelize_grid_lowp_hip(64, 100, 64, 64, 1, None, 1, 32, ctypes.byref(bad), 0, 2, None, 64, 64, 64)
    with pytest.raises(lib.TsdfError, match="tsdf_voxelize_grid_lowp_hip"):
        lib.check(rc, "tsdf_voxelize_grid_lowp_hip")


# ---- the restatements that gained camera parameters: the default-argument result is what it was -----------------------
def _old_obb_cloud(depth, hdr):
    """obb_ref.cloud as it was before it took a camera: the MSRA constants written out."""
    left, top, right, bottom = (int(v) for v in hdr[2:6])
    d = np.asarray(depth, np.float32).reshape(bottom - top, right - left)
    with np.errstate(invalid="ignore"):
        valid = np.abs(d) >= np.float32(1.0)
    i, j = np.nonzero(valid)
    d64 = d[i, j].astype(np.float64)
    s = d64 / 241.42
    return np.stack([((left + j).astype(np.float64) - 160.0) * s, -(((top + i).astype(np.float64) - 120.0) * s), -d64], axis=1)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def test_default_arguments_of_the_extended_restatements_are_what_they_were(pkg):
    depth, off, hdr = cr.batch_a()
    assert (ob.F, ob.CX, ob.CY, ob.EPS) == cr.DEFAULT[:4]
    # obb_ref: cloud against the formula with the constants written out; frame and batch on that cloud
    whole = ob.batch(depth, off, hdr)
    explicit = ob.batch(depth, off, hdr, None, 241.42, 160.0, 120.0, 1.0)
    for i in range(len(hdr)):
        d = depth[off[i]:off[i + 1]]
        old = _old_obb_cloud(d, hdr[i])
        assert np.array_equal(_bits(ob.cloud(d, hdr[i])), _bits(old))
        f = ob.frame(d, hdr[i])
        for g in (whole[i], explicit[i]):
            assert g["status"] == f["status"] and g["N"] == f["N"] == len(old)
            for key in ("mu", "C", "lam", "A", "xf", "pts"):
                assert np.array_equal(_bits(g[key]), _bits(f[key])), key
    # oracle.aabb / oracle.glue: the batch entry of the C oracle (which had its camera all along) on the same frames
    ref = oracle.voxelize(depth, off, hdr, R=16, want_tsdf=False, extras=True)
    for i in range(len(hdr)):
        nv, mn, mx = oracle.aabb(depth[off[i]:off[i + 1]], hdr[i])
        assert nv == cr.valid_counts(depth, off, 1.0)[i]
        assert np.array_equal(_bits(np.concatenate([mn, mx])), _bits(ref["aabb"][i]))
        g, ori = oracle.glue(mn, mx, 16)
        assert np.array_equal(_bits(g), _bits(ref["grid"][i])) and np.array_equal(_bits(ori), _bits(ref["ori"][i]))
    # auggrid_ref.pixel_grids: the placement of the C oracle's augmented batch entry, and aabb + glue as it called them
    xf = pkg.augment.random_affines(ref["grid"][:, :3].astype(np.float64), rng=3)[0]
    rows, max_l, mid_p = ar.pixel_grids(depth, off, hdr, xf, 16)
    va = oracle.voxelize_aug(depth, off, hdr, xf, R=16)
    assert not va["status"].any()
    assert np.array_equal(_bits(max_l), _bits(va["max_l"])) and np.array_equal(_bits(mid_p), _bits(va["mid_p"]))
    for i in range(len(hdr)):
        _, mn, mx = ar.aabb_aug(depth[off[i]:off[i + 1]], hdr[i], xf[i])
        g, ori = oracle.glue(mn, mx, 16)
        assert np.array_equal(_bits(rows[i]), _bits(np.concatenate([ori, g[4:6], np.zeros(3, np.float32)])))


def test_the_new_parameters_reach_the_arithmetic():
    """Each new parameter changes the result it belongs to (a parameter that is accepted and dropped would not)."""
    depth, off, hdr = cr.batch_b()
    d0, h0 = depth[off[0]:off[1]], hdr[0]
    base = ob.cloud(d0, h0)
    for kw in (dict(focal=300.0), dict(cx=150.5), dict(cy=118.25)):
        got = ob.cloud(d0, h0, **kw)
        assert got.shape == base.shape and not np.array_equal(got, base), kw
    assert len(ob.cloud(d0, h0, eps=420.5)) < len(base)
    assert ob.batch(depth, off, hdr, eps=420.5)[0]["N"] == cr.valid_counts(depth, off, 420.5)[0]
    for cam in cr.CAMS:
        nv, mn, mx = oracle.aabb(d0, h0, cam)
        ref = oracle.voxelize(d0, np.array([0, d0.size], np.int64), h0[None], R=32, want_tsdf=False, extras=True, cam=cam)
        assert nv == cr.valid_counts(depth, off, cam[3])[0]
        assert np.array_equal(_bits(np.concatenate([mn, mx])), _bits(ref["aabb"][0]))
        g, ori = oracle.glue(mn, mx, 32, cam)
        assert np.array_equal(_bits(g), _bits(ref["grid"][0])) and np.array_equal(_bits(ori), _bits(ref["ori"][0]))
        xf = ar.identity_xforms(1)
        rows, max_l, mid_p = ar.pixel_grids(d0, np.array([0, d0.size], np.int64), h0[None], xf, 32, cam)
        assert np.array_equal(_bits(rows[0, :5]), _bits(np.concatenate([ori, g[4:6]])))


# ---- the conditions on the inputs of tests/test_camera_gpu.py, on the references --------------------------------------
def test_cam_eps_splits_every_frame_of_batch_b_and_leaves_it_ok():
    depth, off, hdr = cr.batch_b()
    assert len(hdr) == 24 and all(int(h[4] - h[2]) % 2 == 1 for h in hdr)
    nz = depth[depth != 0]
    print(f"batch B: depths {nz.min():.1f} .. {nz.max():.1f} mm")
    assert 405.0 <= nz.min() and nz.max() <= 455.0
    full, part = cr.valid_counts(depth, off, 1.0), cr.valid_counts(depth, off, cr.CAM_EPS[3])
    share = part / full
    print(f"batch B under CAM_EPS keeps {100 * share.min():.1f} .. {100 * share.max():.1f} % of its valid pixels")
    assert (share >= 0.30).all() and (share <= 0.70).all()
    ref = oracle.voxelize(depth, off, hdr, R=32, want_tsdf=False, cam=cr.CAM_EPS)
    assert not ref["status"].any()
    # and the eps of the fourth camera does not discriminate on the seeded crops: why CAM_EPS exists
    a = cr.batch_a()
    assert np.array_equal(cr.valid_counts(a[0], a[1], 1.0)[:24], cr.valid_counts(a[0], a[1], 250.0)[:24])


def test_cam_eps_makes_crops_of_batch_a_degenerate():
    depth, off, hdr = cr.batch_a()
    st = oracle.voxelize(depth, off, hdr, R=32, want_tsdf=False, cam=cr.CAM_EPS)["status"][:24]
    print(f"batch A's crops under CAM_EPS: {(st == 1).sum()} degenerate, {(st == 0).sum()} OK")
    assert (st == 1).sum() >= 5 and (st == 0).sum() >= 10 and ((st == 0) | (st == 1)).all()
    obb = [f["status"] for f in ob.batch(depth, off, hdr, None, *cr.CAM_EPS[:4])][:24]
    assert sum(s == 1 for s in obb) >= 5 and sum(s == 0 for s in obb) >= 10


@pytest.mark.parametrize("cam", cr.CAMS, ids=cr.CAM_IDS)
def test_obb_restatements_input_conditions_hold_under_every_camera(cam):
    """Relative eigenvalue gaps >= 1e-3, |A[0,1]| >= 1e-6 and |A[2,2]| >= 1e-6 for every OK frame of A and B: no frame has
    to be left out of the axes comparison."""
    for name, (depth, off, hdr) in (("A", cr.batch_a()), ("B", cr.batch_b())):
        ref = ob.batch(depth, off, hdr, None, *cam[:4])
        ok = [f for f in ref if f["status"] == 0]
        assert len(ok) >= 10
        for f in ok:
            assert min(ob.rel_gaps(f["lam"])) >= 1e-3 and abs(f["A"][0, 1]) >= 1e-6 and abs(f["A"][2, 2]) >= 1e-6, name
