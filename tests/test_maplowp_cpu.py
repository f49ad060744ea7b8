"""CPU tier of the mapped low-precision volumes (include/tsdf_maplowp.h): libtsdf_maplowp.so as far as it goes without a
GPU — the build rule, the binding through _lib._EXTS, the version, the argument checks before device work —, the
public names and refusals, and the proof that the inputs of the GPU tier's volume tests are not trivial.  Nothing here
touches a GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auggrid_ref as ar  # noqa: E402
from abi_util import declared_functions, exported  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "handposeestimation-with-3d-cnns_amd", "csrc")
INVALID, NO_DEVICE = -1, -2
WANT = ["tsdf_map_place_hip", "tsdf_maplowp_version", "tsdf_voxelize_map_grid_lowp_hip"]


# ---- build rule ----
def test_make_rules_cross_compile_for_gfx950_without_scratch():
    r = subprocess.run(["make", "-C", CSRC, "maplowp", "maplowp-resources"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stdout + r.stderr
    assert "tsdf_map_place_kernel" in text and "tsdf_map_grid_lowp_kernel" in text
    scratch = [ln for ln in text.splitlines() if "ScratchSize" in ln]
    # the placement, and the voxel pass for 2 layouts x 2 dtypes x {8, 4} voxels a lane
    assert len(scratch) == 9 and all(ln.split("]:")[1].split()[0] == "0" for ln in scratch), scratch


# ---- binding ----
def test_row_binds_exactly_its_header_with_types(pkg):
    ext = pkg._lib._EXTS["maplowp"]
    assert isinstance(ext, pkg._lib._Ext)
    assert declared_functions("tsdf_maplowp.h") == WANT == sorted([ext.version_symbol, *ext.entries])
    funcs, named = exported(pkg._lib.MAPLOWP_LIB_PATH)
    assert funcs == WANT and named == WANT
    assert ext.path == pkg._lib.MAPLOWP_LIB_PATH and ext.version == pkg._lib.MAPLOWP_VERSION == 1
    L = pkg._lib.load_maplowp()
    assert L.tsdf_maplowp_version() == 1
    for entry in (ext.version_symbol, *ext.entries):
        fn = getattr(L, entry)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, entry
    vp, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    cam_p = ctypes.POINTER(pkg._lib.TsdfCam)
    assert list(L.tsdf_map_place_hip.argtypes) == [vp, i64, vp, vp, i64, vp, i, i, cam_p, vp, vp, vp, vp, vp, vp]
    assert list(L.tsdf_voxelize_map_grid_lowp_hip.argtypes) == [vp, i64, vp, vp, i64, vp, i, i, cam_p, i, i, vp, vp, vp, vp,
                                                                vp]
    for name, args in ext.entries.items():
        assert list(getattr(L, name).argtypes) == args and args
    assert pkg._lib.load_maplowp() is L and L is not pkg._lib.load() and L is not pkg._lib.load_lowp()
    # the product beside it is what it was
    assert pkg._lib.load().tsdf_version() == 7


# ---- argument checks ----
def test_argument_validation_happens_before_device_work(pkg):
    L = pkg._lib.load_maplowp()
    null, one, odd, odd4 = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(72), ctypes.c_void_p(68)

    def place(depth=one, depth_len=100, offsets=one, headers=one, n_src=1, index=null, n=1, R=32, xforms=one, grid=one,
              max_l=one, mid_p=one, status=one):
        return L.tsdf_map_place_hip(depth, depth_len, offsets, headers, n_src, index, n, R, None, null, xforms, grid,
                                    max_l, mid_p, status)

    def vox(depth=one, depth_len=100, offsets=one, headers=one, n_src=1, index=null, n=1, R=32, layout=0, dtype=2,
            xforms=one, grid=one, out=one, status=one):
        return L.tsdf_voxelize_map_grid_lowp_hip(depth, depth_len, offsets, headers, n_src, index, n, R, None, layout,
                                                 dtype, null, xforms, grid, out, status)

    for call in (place, vox):
        assert call(n=-1) == INVALID
        for name in ("depth", "offsets", "headers", "xforms", "grid"):
            assert call(**{name: null}) == INVALID, name
        assert call(depth_len=-1) == INVALID
        assert call(n_src=0, index=one) == INVALID and call(n_src=-3, index=one) == INVALID
        assert call(n_src=2) == INVALID and call(n=2) == INVALID          # no index: n_src must equal n
        for R in (0, 2, 3, 6, 30, 132, 256, -4):
            assert call(R=R) == INVALID, R
        assert call(xforms=odd4) == INVALID                                # 4-byte, not 8-byte aligned
        # valid arguments get as far as the device, and there is none here
        assert call() == NO_DEVICE
        assert call(status=null) == NO_DEVICE                              # the status is optional
        assert call(n_src=5, index=one, n=3) == NO_DEVICE
        assert call(xforms=odd) == NO_DEVICE                               # 8-byte aligned will do
        for R in (4, 12, 64, 128):
            assert call(R=R) == NO_DEVICE, R
        # n == 0 is a no-op
        assert call(n=0, n_src=0) == 0
        assert call(n=0, n_src=0, R=30) == INVALID                         # but R (layout, dtype) is judged before n == 0
    assert vox(n=0, n_src=0, layout=2) == INVALID and vox(n=0, n_src=0, dtype=3) == INVALID
    assert place(max_l=null, mid_p=null, status=null) == NO_DEVICE         # every scalar output is optional
    assert place(n=2 ** 31 - 1, n_src=2 ** 31 - 1) == NO_DEVICE            # the placement strides over any n
    assert L.tsdf_map_place_hip(null, 0, null, null, 0, null, 0, 32, None, null, null, null, null, null, null) == 0

    assert vox(out=null) == INVALID
    for layout in (-1, 2):
        assert vox(layout=layout) == INVALID
    for dtype in (0, 3, -1):
        assert vox(dtype=dtype) == INVALID
    assert vox(out=odd) == INVALID                                         # 8-byte, not 16-byte aligned
    # more than 2^32 work-items: at R = 128 a position is 128 workgroups of 256 lanes
    big = 2 ** 31 - 1
    assert vox(n=big, n_src=big, R=128) == INVALID
    assert vox(n=2 ** 17, n_src=2 ** 17, R=128) == INVALID                 # exactly 2^32
    assert vox(n=2 ** 17 - 1, n_src=2 ** 17 - 1, R=128) == NO_DEVICE
    for R in (4, 12, 64, 128):
        assert vox(R=R, dtype=1, layout=1) == NO_DEVICE, R
    assert L.tsdf_voxelize_map_grid_lowp_hip(null, 0, null, null, 0, null, 0, 32, None, 0, 1, null, null, null, null,
                                             null) == 0


# ---- public names and refusals ----
def test_public_names_and_refusals(pkg, synth):
    for name in ("map_grids", "MapGridBatch", "voxelize_map_grid_lowp", "voxelize_aug_lowp"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
        assert name in pkg.__doc__ or name == "MapGridBatch", name   # (the docstring lists functions, not result types)
    assert "tsdf_maplowp.h" in pkg.__doc__ and "AugmentedStep(dtype=" in pkg.__doc__
    assert pkg.MapGridBatch._fields == ("grid", "max_l", "mid_p", "status")
    doc = pkg.voxelize_aug_lowp.__doc__
    assert "two launches" in doc.lower() and "twice" in doc
    depth, off, hdr = (torch.from_numpy(x) for x in synth.synth_batch(2, "crop", seed0=3))
    xf = torch.from_numpy(pkg.augment.identity_affines(2))
    grid = torch.zeros((2, 8))
    for bad in (torch.float32, torch.float64, torch.int16, "bfloat16"):
        with pytest.raises(ValueError, match="float16 or torch.bfloat16"):
            pkg.voxelize_map_grid_lowp(depth, off, hdr, xf, grid, dtype=bad)
        with pytest.raises(ValueError, match="float16 or torch.bfloat16"):
            pkg.voxelize_aug_lowp(depth, off, hdr, xf, dtype=bad)
        with pytest.raises(ValueError, match="float16 or torch.bfloat16"):
            pkg.voxelize_obb(depth, off, hdr, dtype=bad)
        with pytest.raises(ValueError, match="float16 or torch.bfloat16"):
            pkg.process_batch_aug(depth, off, hdr, dtype=bad)
        with pytest.raises(ValueError, match="float16 or torch.bfloat16"):
            pkg.AugmentedStep(depth, off, hdr, 2, dtype=bad)
    for fn in (pkg.voxelize_map_grid_lowp, pkg.voxelize_aug_lowp):
        with pytest.raises(ValueError, match="float16 or torch.bfloat16"):
            fn(depth, off, hdr, xf, *([grid] if fn is pkg.voxelize_map_grid_lowp else []), dtype=None)
    # there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        pkg.map_grids(depth, off, hdr, xf)
    with pytest.raises(ValueError, match="GPU"):
        pkg.voxelize_map_grid_lowp(depth, off, hdr, xf, grid)
    with pytest.raises(ValueError, match="GPU"):
        pkg.voxelize_aug_lowp(depth, off, hdr, xf)
    with pytest.raises(ValueError, match="GPU"):
        pkg.voxelize_obb(depth, off, hdr, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="GPU"):
        pkg.process_batch_aug(depth, off, hdr, dtype=torch.float16)
    with pytest.raises(ValueError, match="GPU"):
        pkg.AugmentedStep(depth, off, hdr, 2, dtype=torch.bfloat16)
    # the loader still refuses a volume_dtype under a map (lifting that is a follow-up)
    d, o, h = synth.synth_batch(4, "crop", seed0=3)
    ds = pkg.MSRADepthDataset.from_packs([pkg.packing.PackedFrames(d, o, h, np.zeros((4, 63), np.float32))])
    bf = torch.bfloat16
    for kw in (dict(volume_dtype=bf, augment=True), dict(volume_dtype=bf, augment="device"),
               dict(volume_dtype=bf, frame="obb"), dict(volume_dtype=torch.float16, augment="device", graph=True)):
        with pytest.raises(ValueError):
            pkg.ResidentLoader(ds, batch_size=2, device="cuda", **kw)


# ---- the inputs of the GPU tier are not trivial ----
@pytest.mark.parametrize("R", [8, 12, 32])
def test_the_gpu_tiers_inputs_do_not_compare_zeros(pkg, synth, R):
    import oracle

    depth, off, hdr = synth.synth_batch(10, "crop", seed0=1200)
    plain = oracle.voxelize(depth, off, hdr, R=32, want_tsdf=False)
    assert not plain["status"].any()
    xf = pkg.augment.random_affines(plain["mid_p"].astype(np.float64), rng=5)[0]
    grid, max_l, mid_p = ar.pixel_grids(depth, off, hdr, xf, R)
    vol, st = ar.voxelize_aug_grid_ref(depth, off, hdr, xf, grid, R, "czyx")
    near, nonzero = ar.near_counts(vol)
    print(f"R={R}: fewest near voxels {near.min()}, fewest non-zero voxels {nonzero.min()}")
    assert not st.any() and near.min() >= 100
    # on the grid shifted by 0.75 max_l along x (the GPU tier's second grid) most voxels are rejected, some still near
    moved = grid.copy()
    moved[:, 0] += np.float32(0.75) * max_l
    vol2, st2 = ar.voxelize_aug_grid_ref(depth, off, hdr, xf, moved, R, "czyx")
    near2, _ = ar.near_counts(vol2)
    rejected = float((vol2 == 0).all(axis=1).mean())
    print(f"R={R} shifted: rejected {rejected:.3f}, near voxels in all {near2.sum()}")
    assert not st2.any() and rejected > 0.7 and near2.sum() > 0
