"""ctypes binding of libtsdf_hip.so (the C ABI declared in include/tsdf.h).

There is deliberately NO fallback: if the HIP library is missing or fails to load,
importing the voxelizer raises.  The product path never routes through a CPU
implementation (the oracle under oracle/ is test infrastructure only).
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_LIB = os.path.join(_HERE, "libtsdf_hip.so")


def _lib_path() -> str:
    """The product binary.  TSDF_HIP_LIB may name another build of the same ABI (diagnostic variants live in
    <repo>/build/), but only together with TSDF_ALLOW_LIB_OVERRIDE=1: a stale variable must not silently swap the
    library the tests and the bench believe they are measuring."""
    over = os.environ.get("TSDF_HIP_LIB")
    if not over or os.path.abspath(over) == _DEFAULT_LIB:
        return _DEFAULT_LIB
    if os.environ.get("TSDF_ALLOW_LIB_OVERRIDE") != "1":
        raise ImportError(f"TSDF_HIP_LIB={over} asks for a library other than {_DEFAULT_LIB}; set "
                          "TSDF_ALLOW_LIB_OVERRIDE=1 as well if that is intended (experiments only)")
    return over


LIB_PATH = _lib_path()

TSDF_LAYOUT_CZYX = 0
TSDF_LAYOUT_CXYZ = 1
LAYOUTS = {"czyx": TSDF_LAYOUT_CZYX, "cxyz": TSDF_LAYOUT_CXYZ}

TSDF_OK = 0
TSDF_FRAME_OK = 0
TSDF_FRAME_DEGENERATE = 1
TSDF_FRAME_BAD_HEADER = 2


class TsdfError(RuntimeError):
    """A tsdf_* entry point returned a negative status."""


class TsdfCam(ctypes.Structure):
    """``tsdf_cam`` of include/tsdf.h (defaults: pre/tsdf_numba.py:8-10)."""

    _fields_ = [
        ("focal", ctypes.c_double),
        ("cx", ctypes.c_double),
        ("cy", ctypes.c_double),
        ("invalid_eps", ctypes.c_float),
        ("trunc_voxels", ctypes.c_float),
    ]


class TsdfLabels(ctypes.Structure):
    """``tsdf_labels`` of include/tsdf.h: device pointers for the fused label normalisation."""

    _fields_ = [
        ("d_gt", ctypes.c_void_p),
        ("n_joints", ctypes.c_int),
        ("clamp", ctypes.c_int),
        ("d_out_gt_nor", ctypes.c_void_p),
        ("d_out_gt_aug", ctypes.c_void_p),
    ]


class TsdfPca(ctypes.Structure):
    """``tsdf_pca`` of include/tsdf.h: the joint-PCA basis (device pointers) and the projection's output."""

    _fields_ = [
        ("d_mean", ctypes.c_void_p),
        ("d_coeff", ctypes.c_void_p),
        ("n_components", ctypes.c_int),
        ("d_out_gt_pca", ctypes.c_void_p),
    ]


ABI_VERSION = 7
INLINE_INDEX_MAX = 32   # TSDF_INLINE_INDEX_MAX of include/tsdf.h

# The debug build of the same sources (make -C csrc debug: -DTSDF_DEBUG_HOOKS): everything the product exports plus the
# test hooks of include/tsdf_debug.h.  Never loaded unless somebody asks for a hook.
DEBUG_LIB_PATH = os.path.join(os.path.dirname(_HERE), "build", "libtsdf_hip_debug.so")

# The extension library of include/tsdf_augment.h (make -C csrc augment): the augmentation's draws and maps on the GPU.
# A binary of its own, because the ABI of libtsdf_hip.so is frozen.
AUGMENT_LIB_PATH = os.path.join(_HERE, "libtsdf_augment.so")
AUGMENT_VERSION = 1

# The extension library of include/tsdf_augstep.h (make -C csrc augstep): the same draws from a key and counters that
# live in device memory.  Again a binary of its own: libtsdf_augment.so is frozen at its two exports.
AUGSTEP_LIB_PATH = os.path.join(_HERE, "libtsdf_augstep.so")
AUGSTEP_VERSION = 1

# The extension library of include/tsdf_auggrid.h (make -C csrc auggrid): the augmented voxelization on a caller-supplied
# grid and the augmented labels on their own.  A binary of its own again: everything above is frozen.
AUGGRID_LIB_PATH = os.path.join(_HERE, "libtsdf_auggrid.so")
AUGGRID_VERSION = 1

# The extension library of include/tsdf_depth16.h (make -C csrc depth16): 16-bit depth (packing.py, TSDFPK02 packs) widened
# to the float32 buffer the voxelizer reads, and the 16-bit twin of the host gather.  A binary of its own once more.
DEPTH16_LIB_PATH = os.path.join(_HERE, "libtsdf_depth16.so")
DEPTH16_VERSION = 1
DEPTH16_MAX_SHIFT = 7   # TSDF_DEPTH16_MAX_SHIFT of include/tsdf_depth16.h

# The extension library of include/tsdf_obb.h (make -C csrc obb): per-frame principal-axis maps (the cloud's mean and
# covariance, a 3x3 eigen-decomposition, HandPointNet's signs) from the depth alone.  A binary of its own: all above is frozen.
OBB_LIB_PATH = os.path.join(_HERE, "libtsdf_obb.so")
OBB_VERSION = 1

# The extension library of include/tsdf_lowp.h (make -C csrc lowp): the plain voxel pass on a caller-supplied grid written
# as float16 / bfloat16 voxels, and the same narrowing for float32 values.  A binary of its own: all above is frozen.
LOWP_LIB_PATH = os.path.join(_HERE, "libtsdf_lowp.so")
LOWP_VERSION = 1
TSDF_LOWP_F16 = 1    # enum tsdf_lowp_dtype of include/tsdf_lowp.h
TSDF_LOWP_BF16 = 2

# The extension library of include/tsdf_maplowp.h (make -C csrc maplowp): the grid placement under a per-frame map on its
# own, and the augmented voxel pass on a caller-supplied grid written as float16 / bfloat16 voxels.  A binary of its own.
MAPLOWP_LIB_PATH = os.path.join(_HERE, "libtsdf_maplowp.so")
MAPLOWP_VERSION = 1

# The extension library of include/tsdf_mapstep.h (make -C csrc mapstep): two per-frame maps composed into one, and the head
# of the augmented step (draw, compose, placement, labels) as one launch.  A binary of its own.
MAPSTEP_LIB_PATH = os.path.join(_HERE, "libtsdf_mapstep.so")
MAPSTEP_VERSION = 1

# The extension library of include/tsdf_locate.h (make -C csrc locate): the hand located in raw depth frames (the nearest
# object's centre of mass, a fixed cube around it) and the crops packed as depth / offsets / headers.  A binary of its own.
LOCATE_LIB_PATH = os.path.join(_HERE, "libtsdf_locate.so")
LOCATE_VERSION = 1
TSDF_LOCATE_F32 = 0   # `frame_type` of include/tsdf_locate.h
TSDF_LOCATE_U16 = 1

# The extension library of include/tsdf_accurate.h (make -C csrc accurate): the accurate directional TSDF on a
# caller-supplied grid — per voxel the nearest surface point among all valid pixels of the crop.  A binary of its own.
ACCURATE_LIB_PATH = os.path.join(_HERE, "libtsdf_accurate.so")
ACCURATE_VERSION = 1

# The extension library of include/tsdf_mapaccurate.h (make -C csrc mapaccurate): the accurate directional TSDF under a
# per-frame map, on a caller-supplied grid.  A binary of its own: libtsdf_accurate.so is frozen at its two exports.
MAPACCURATE_LIB_PATH = os.path.join(_HERE, "libtsdf_mapaccurate.so")
MAPACCURATE_VERSION = 1

# The library of include/tsdf_heatmap.h (make -C csrc heatmap): per-joint Gaussian heatmap volumes from normalised labels,
# and per joint the peak of a volume back as normalised coordinates.  A binary of its own; its row is _HEATMAP below, not
# yet a row of _EXTS (tests/test_ext_table_cpu.py pins that table name by name).
HEATMAP_LIB_PATH = os.path.join(_HERE, "libtsdf_heatmap.so")
HEATMAP_VERSION = 1
TSDF_HEATMAP_F32 = 0   # the float32 element type of include/tsdf_heatmap.h; the 2-byte ones are TSDF_LOWP_*

# The library of include/tsdf_heatloss.h (make -C csrc heatloss): the squared error of a predicted heatmap volume against
# the Gaussian target of its label without that target in memory, a soft-argmax over the softmax of a whole volume, and
# the gradient of each.  A binary of its own; its row is _HEATLOSS below, outside _EXTS like _HEATMAP.
HEATLOSS_LIB_PATH = os.path.join(_HERE, "libtsdf_heatloss.so")
HEATLOSS_VERSION = 1

# The library of include/tsdf_occupancy.h (make -C csrc occupancy): one-channel occupancy volumes on a caller-placed grid,
# every pixel of the crop scattered into a bit mask in LDS.  A binary of its own; its row is _OCCUPANCY below, outside
# _EXTS like _HEATMAP.
OCCUPANCY_LIB_PATH = os.path.join(_HERE, "libtsdf_occupancy.so")
OCCUPANCY_VERSION = 1
OCCUPANCY_LDS_CAP = 64 * 1024   # bytes of bit mask per workgroup (kOccLdsCap of csrc/occupancy_host.inc)

# The library of include/tsdf_fps.h (make -C csrc fps): farthest-point sampled clouds from a packed crop or from a cloud,
# one workgroup per batch position running the chain of arg-max reductions on chip.  A binary of its own; its row is _FPS
# below, outside _EXTS like _HEATMAP.
FPS_LIB_PATH = os.path.join(_HERE, "libtsdf_fps.so")
FPS_VERSION = 1
TSDF_FPS_FRAME_OVER_CAPACITY = 3   # per-position status of include/tsdf_fps.h, next to TSDF_FRAME_*
FPS_MAX_POINTS = 65536             # TSDF_FPS_MAX_POINTS
TSDF_FPS_F32 = 0                   # the element types of tsdf_fps_points_hip's cloud
TSDF_FPS_F64 = 1

# The library of include/tsdf_group.h (make -C csrc group): kNN grouping and PCA surface normals of sampled clouds, a top-K
# selection per query over a cloud resident in LDS.  A binary of its own; its row is _GROUP below, outside _EXTS like
# _HEATMAP.
GROUP_LIB_PATH = os.path.join(_HERE, "libtsdf_group.so")
GROUP_VERSION = 1
GROUP_MAX_CLOUD = 12288            # TSDF_GROUP_MAX_CLOUD: rows of a cloud, the sampler's resident cap
GROUP_MAX_K = 128                  # TSDF_GROUP_MAX_K
GROUP_SWEEPS = 8                   # TSDF_GROUP_SWEEPS: the fixed number of Jacobi sweeps of the normals

# The library of include/tsdf_pointfield.h (make -C csrc pointfield): point-wise offset-field labels of sampled clouds — per
# point and joint a heat and a unit vector towards the joint — and their voting decode, a selection without a sort per
# joint over a cloud resident in LDS.  A binary of its own; its row is _POINTFIELD below, outside _EXTS like _HEATMAP.
POINTFIELD_LIB_PATH = os.path.join(_HERE, "libtsdf_pointfield.so")
POINTFIELD_VERSION = 1
POINTFIELD_MAX_CLOUD = 12288       # TSDF_POINTFIELD_MAX_CLOUD: rows of a cloud, GROUP_MAX_CLOUD
POINTFIELD_MAX_K = 12288           # TSDF_POINTFIELD_MAX_K: the encoder's nearest points per joint
POINTFIELD_MAX_VOTES = 128         # TSDF_POINTFIELD_MAX_VOTES: the decoder's voting points per joint
POINTFIELD_MAX_JOINTS = 65536      # TSDF_POINTFIELD_MAX_JOINTS
POINTFIELD_LAYOUTS = {"cp": 0, "pc": 1}   # TSDF_POINTFIELD_CP [n, 4J, P] / TSDF_POINTFIELD_PC [n, P, 4J]

# The library of include/tsdf_patch.h (make -C csrc patch): depth-image patches for the 2-D CNNs — a fixed-size patch
# resampled from the located cube's image rectangle under an optional in-plane map, the joints in the patch's (u, v, d)
# coordinates and the way back.  A binary of its own; its row is _PATCH below, outside _EXTS like _HEATMAP.
PATCH_LIB_PATH = os.path.join(_HERE, "libtsdf_patch.so")
PATCH_VERSION = 1
TSDF_PATCH_F32 = 0                 # the float32 element type of include/tsdf_patch.h; the 2-byte ones are TSDF_LOWP_*
PATCH_MIN_SIZE = 8                 # TSDF_PATCH_MIN_SIZE: a patch's edge is a multiple of 8 in 8..512
PATCH_MAX_SIZE = 512               # TSDF_PATCH_MAX_SIZE
PATCH_MAX_JOINTS = 65536           # TSDF_PATCH_MAX_JOINTS
PATCH_INTERPS = {"nearest": 0, "bilinear": 1}   # TSDF_PATCH_NEAREST / TSDF_PATCH_BILINEAR


class _Ext(NamedTuple):
    """A row of the extension table: libtsdf_<name>.so, built by ``make -C csrc <name>`` from include/tsdf_<name>.h."""
    path: str
    version_symbol: str
    version: int
    entries: dict   # {entry point: argtypes}; every entry returns a tsdf_status (int)


_vp, _i, _i64, _u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64

# The extension libraries of csrc/Makefile's `EXTS :=` line, in its order: tests/test_ext_table_cpu.py pins this table to
# exactly these and checks every row against its header and its binary.  Adding one is a row here, a name on that line
# (with what its tsdf_<name>.hip includes besides device.inc in <name>_DEPS), a one-line load_<name> below and a name in
# that test's list.
_EXTS = {
    "augment": _Ext(AUGMENT_LIB_PATH, "tsdf_augment_version", AUGMENT_VERSION, {
        # centres, n_src, index, n, key, counter0, stream, xforms, stretch, rot
        "tsdf_aug_draw_hip": [_vp, _i64, _vp, _i, _u64, _u64, _vp, _vp, _vp, _vp],
    }),
    "augstep": _Ext(AUGSTEP_LIB_PATH, "tsdf_augstep_version", AUGSTEP_VERSION, {
        # centres, n_src, index, n, state, counters, stream, xforms, stretch, rot
        "tsdf_aug_draw_at_hip": [_vp, _i64, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    }),
    "auggrid": _Ext(AUGGRID_LIB_PATH, "tsdf_auggrid_version", AUGGRID_VERSION, {
        # depth, depth_len, offsets, headers, n, R, cam, layout, stream, xforms, grid, tsdf, status
        "tsdf_voxelize_aug_grid_hip": [_vp, _i64, _vp, _vp, _i, _i, ctypes.POINTER(TsdfCam), _i, _vp, _vp, _vp, _vp, _vp],
        # gt, xforms, n, n_joints, stream, gt_aug
        "tsdf_transform_joints_hip": [_vp, _vp, _i, _i, _vp, _vp],
    }),
    "depth16": _Ext(DEPTH16_LIB_PATH, "tsdf_depth16_version", DEPTH16_VERSION, {
        # src, n_px, shift, dst, stream
        "tsdf_depth16_widen_hip": [_vp, _i64, _i, _vp, _vp],
        # src, src_len, src_offsets, n_src, index, n, dst, dst_len, dst_offsets, n_threads
        "tsdf_depth16_host_gather": [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i],
    }),
    "obb": _Ext(OBB_LIB_PATH, "tsdf_obb_version", OBB_VERSION, {
        # depth, depth_len, offsets, headers, n, cam, stream, xforms, moments, status
        "tsdf_obb_xforms_hip": [_vp, _i64, _vp, _vp, _i, ctypes.POINTER(TsdfCam), _vp, _vp, _vp, _vp],
    }),
    "lowp": _Ext(LOWP_LIB_PATH, "tsdf_lowp_version", LOWP_VERSION, {
        # depth, depth_len, offsets, headers, n_src, index, n, R, cam, layout, dtype, stream, grid, tsdf, status
        "tsdf_voxelize_grid_lowp_hip": [_vp, _i64, _vp, _vp, _i64, _vp, _i, _i, ctypes.POINTER(TsdfCam), _i, _i, _vp, _vp,
                                        _vp, _vp],
        # in, count, dtype, stream, out
        "tsdf_lowp_narrow_hip": [_vp, _i64, _i, _vp, _vp],
    }),
    "maplowp": _Ext(MAPLOWP_LIB_PATH, "tsdf_maplowp_version", MAPLOWP_VERSION, {
        # depth, depth_len, offsets, headers, n_src, index, n, R, cam, stream, xforms, grid, max_l, mid_p, status
        "tsdf_map_place_hip": [_vp, _i64, _vp, _vp, _i64, _vp, _i, _i, ctypes.POINTER(TsdfCam), _vp, _vp, _vp, _vp, _vp, _vp],
        # depth, depth_len, offsets, headers, n_src, index, n, R, cam, layout, dtype, stream, xforms, grid, tsdf, status
        "tsdf_voxelize_map_grid_lowp_hip": [_vp, _i64, _vp, _vp, _i64, _vp, _i, _i, ctypes.POINTER(TsdfCam), _i, _i, _vp, _vp,
                                            _vp, _vp, _vp],
    }),
    "mapstep": _Ext(MAPSTEP_LIB_PATH, "tsdf_mapstep_version", MAPSTEP_VERSION, {
        # outer, inner, n_inner, index, n, stream, out
        "tsdf_compose_xforms_hip": [_vp, _vp, _i64, _vp, _i, _vp, _vp],
        # depth, depth_len, offsets, headers, n_src, index, n, R, focal, cx, cy, invalid_eps, trunc_voxels (the camera by
        # value), centres, base, state, counters, gt, n_joints, clamp, stream, xforms, grid, max_l, mid_p, status, gt_aug,
        # gt_nor, stretch, rot
        "tsdf_map_step_head_hip": [_vp, _i64, _vp, _vp, _i64, _vp, _i, _i, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                   ctypes.c_float, ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp, _vp, _vp],
    }),
    "locate": _Ext(LOCATE_LIB_PATH, "tsdf_locate_version", LOCATE_VERSION, {
        # H, W, cube, near, focal, per_frame (an int64 in host memory)
        "tsdf_locate_capacity": [_i, _i, ctypes.c_float, ctypes.c_float, ctypes.c_double, ctypes.POINTER(_i64)],
        # frames, frame_type, shift, n_src, H, W, index, n, near, far, cube, seed_band, refine, R, focal, cx, cy, invalid_eps,
        # trunc_voxels (the camera by value), depth_capacity, stream, depth, offsets, headers, com, count, status, grid,
        # max_l, mid_p
        "tsdf_locate_hip": [_vp, _i, _i, _i64, _i, _i, _vp, _i, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                            ctypes.c_float, _i, _i, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_float,
                            ctypes.c_float, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    }),
    "accurate": _Ext(ACCURATE_LIB_PATH, "tsdf_accurate_version", ACCURATE_VERSION, {
        # depth, depth_len, offsets, headers, n_src, index, n, R, focal, cx, cy, invalid_eps, trunc_voxels (the camera by
        # value), layout, stream, grid, tsdf, nearest, status
        "tsdf_voxelize_grid_accurate_hip": [_vp, _i64, _vp, _vp, _i64, _vp, _i, _i, ctypes.c_double, ctypes.c_double,
                                            ctypes.c_double, ctypes.c_float, ctypes.c_float, _i, _vp, _vp, _vp, _vp, _vp],
    }),
    "mapaccurate": _Ext(MAPACCURATE_LIB_PATH, "tsdf_mapaccurate_version", MAPACCURATE_VERSION, {
        # depth, depth_len, offsets, headers, n_src, index, n, R, focal, cx, cy, invalid_eps, trunc_voxels (the camera by
        # value), layout, stream, xforms, grid, tsdf, nearest, status
        "tsdf_voxelize_map_grid_accurate_hip": [_vp, _i64, _vp, _vp, _i64, _vp, _i, _i, ctypes.c_double, ctypes.c_double,
                                                ctypes.c_double, ctypes.c_float, ctypes.c_float, _i, _vp, _vp, _vp, _vp, _vp,
                                                _vp],
    }),
}

# libtsdf_heatmap.so's row, of the same type and loaded by the same code (load_heatmap)
_HEATMAP = _Ext(HEATMAP_LIB_PATH, "tsdf_heatmap_version", HEATMAP_VERSION, {
    # u, status, n, n_joints, R, sigma, layout, dtype, stream, heat, valid
    "tsdf_joint_heatmaps_hip": [_vp, _vp, _i, _i, _i, ctypes.c_float, _i, _i, _vp, _vp, _vp],
    # heat, dtype, n, n_joints, R, layout, radius, stream, u, peak, arg
    "tsdf_heatmap_joints_hip": [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp],
})

# libtsdf_heatloss.so's row, of the same type and loaded by the same code (load_heatloss)
_HEATLOSS = _Ext(HEATLOSS_LIB_PATH, "tsdf_heatloss_version", HEATLOSS_VERSION, {
    # pred, dtype, u, status, n, n_joints, R, sigma, layout, stream, sse, valid
    "tsdf_heat_sse_hip": [_vp, _i, _vp, _vp, _i, _i, _i, ctypes.c_float, _i, _vp, _vp, _vp],
    # pred, dtype, u, status, w, n, n_joints, R, sigma, layout, stream, grad
    "tsdf_heat_sse_grad_hip": [_vp, _i, _vp, _vp, _vp, _i, _i, _i, ctypes.c_float, _i, _vp, _vp],
    # heat, dtype, n, n_joints, R, beta, layout, stream, u, stats
    "tsdf_soft_argmax_hip": [_vp, _i, _i, _i, _i, ctypes.c_float, _i, _vp, _vp, _vp],
    # heat, dtype, stats, grad_u, n, n_joints, R, beta, layout, stream, grad
    "tsdf_soft_argmax_grad_hip": [_vp, _i, _vp, _vp, _i, _i, _i, ctypes.c_float, _i, _vp, _vp],
})

# libtsdf_occupancy.so's row, of the same type and loaded by the same code (load_occupancy)
_OCCUPANCY = _Ext(OCCUPANCY_LIB_PATH, "tsdf_occupancy_version", OCCUPANCY_VERSION, {
    # R, slab_hint, slab, nslab, lds_bytes (three ints in host memory)
    "tsdf_occupancy_plan": [_i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)],
    # depth, depth_len, offsets, headers, n_src, index, n, R, focal, cx, cy, invalid_eps, trunc_voxels (the camera by
    # value), layout, dtype, slab_hint, stream, xforms, max_l, mid_p, occ, status
    "tsdf_occupancy_hip": [_vp, _i64, _vp, _vp, _i64, _vp, _i, _i, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                           ctypes.c_float, ctypes.c_float, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp],
})

# libtsdf_fps.so's row, of the same type and loaded by the same code (load_fps)
_FPS = _Ext(FPS_LIB_PATH, "tsdf_fps_version", FPS_VERSION, {
    # M, capacity, form_hint, resident_cap, work_bytes, lds_bytes (an int, an int64 and an int in host memory)
    "tsdf_fps_plan": [_i, _i64, _i, ctypes.POINTER(_i), ctypes.POINTER(_i64), ctypes.POINTER(_i)],
    # depth, depth_len, offsets, headers, n_src, index, n, M, focal, cx, cy, invalid_eps, trunc_voxels (the camera by
    # value), capacity, form_hint, stream, xforms, work, points, pixel, radius2, count, status
    "tsdf_fps_hip": [_vp, _i64, _vp, _vp, _i64, _vp, _i, _i, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                     ctypes.c_float, ctypes.c_float, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    # cloud, dtype, n, P, M, capacity, form_hint, stream, work, points, pixel, radius2, count, status
    "tsdf_fps_points_hip": [_vp, _i, _i, _i64, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
})

# libtsdf_group.so's row, of the same type and loaded by the same code (load_group)
_GROUP = _Ext(GROUP_LIB_PATH, "tsdf_group_version", GROUP_VERSION, {
    # P, C, K, lds_bytes, queries_per_group, groups_per_position (three ints in host memory)
    "tsdf_group_plan": [_i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)],
    # points, pitch, query, status_in, n, P, C, K, stream, index, dist2, offset, status
    "tsdf_knn_hip": [_vp, _i64, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp],
    # points, pitch, query, status_in, view, n, P, C, K, stream, normals, curvature, status
    "tsdf_normals_hip": [_vp, _i64, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp],
})

# libtsdf_pointfield.so's row, of the same type and loaded by the same code (load_pointfield)
_POINTFIELD = _Ext(POINTFIELD_LIB_PATH, "tsdf_pointfield_version", POINTFIELD_VERSION, {
    # P, J, K, lds_bytes, joints_per_group, groups_per_position (three ints in host memory)
    "tsdf_pointfield_plan": [_i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)],
    # points, pitch, joints, status_in, n, P, J, K, radius, layout, dtype, stream, field, valid, status
    "tsdf_pointfield_encode_hip": [_vp, _i64, _vp, _vp, _i, _i, _i, _i, ctypes.c_double, _i, _i, _vp, _vp, _vp, _vp],
    # points, pitch, field, status_in, n, P, J, M, radius, layout, dtype, stream, joints, weight, status
    "tsdf_pointfield_decode_hip": [_vp, _i64, _vp, _vp, _i, _i, _i, _i, ctypes.c_double, _i, _i, _vp, _vp, _vp, _vp],
})

# libtsdf_patch.so's row, of the same type and loaded by the same code (load_patch)
_dbl, _flt = ctypes.c_double, ctypes.c_float
_PATCH = _Ext(PATCH_LIB_PATH, "tsdf_patch_version", PATCH_VERSION, {
    # S, dtype, px_per_lane, rows_per_group, items_per_position (three ints in host memory)
    "tsdf_patch_plan": [_i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)],
    # frames, frame_type, shift, n_src, H, W, index, com, cube, cube_n, affine, status_in, n, S, interp, dtype, background,
    # focal, cx, cy, invalid_eps, trunc_voxels (the camera by value), stream, patch, status
    "tsdf_patch_frames_hip": [_vp, _i, _i, _i64, _i, _i, _vp, _vp, _flt, _vp, _vp, _vp, _i, _i, _i, _i, _flt, _dbl, _dbl, _dbl,
                              _flt, _flt, _vp, _vp, _vp],
    # depth, depth_len, offsets, headers, n_src, index, com, cube, cube_n, affine, status_in, n, S, interp, dtype, background,
    # focal, cx, cy, invalid_eps, trunc_voxels, stream, patch, status
    "tsdf_patch_crops_hip": [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _flt, _vp, _vp, _vp, _i, _i, _i, _i, _flt, _dbl, _dbl, _dbl,
                             _flt, _flt, _vp, _vp, _vp],
    # joints, com, cube, cube_n, affine, status_in, n, J, focal, cx, cy, invalid_eps, trunc_voxels, stream, uvd, valid, status
    "tsdf_patch_uvd_hip": [_vp, _vp, _flt, _vp, _vp, _vp, _i, _i, _dbl, _dbl, _dbl, _flt, _flt, _vp, _vp, _vp, _vp],
    # uvd, com, cube, cube_n, affine, status_in, n, J, focal, cx, cy, invalid_eps, trunc_voxels, stream, joints
    "tsdf_patch_joints_hip": [_vp, _vp, _flt, _vp, _vp, _vp, _i, _i, _dbl, _dbl, _dbl, _flt, _flt, _vp, _vp],
})

_lib = None
_debug_lib = None
_ext_libs = {}   # name -> the loaded extension library


def _declare(L, entries: dict) -> None:
    """``argtypes`` as given and ``restype`` int on every named entry point of a loaded library."""
    for name, argtypes in entries.items():
        fn = getattr(L, name)
        fn.restype = ctypes.c_int
        fn.argtypes = argtypes


def _bind(L, path: str, debug: bool = False):
    """Declare the argument / result types of every entry point of include/tsdf.h on a loaded library (``debug``: and of
    the hooks of include/tsdf_debug.h)."""
    vp = ctypes.c_void_p
    cam_p = ctypes.POINTER(TsdfCam)
    L.tsdf_version.restype = ctypes.c_int
    L.tsdf_version.argtypes = []
    if L.tsdf_version() != ABI_VERSION:
        raise ImportError(f"{path} has ABI version {L.tsdf_version()}, this package needs {ABI_VERSION}: rebuild it")
    L.tsdf_strerror.restype = ctypes.c_char_p
    L.tsdf_strerror.argtypes = [ctypes.c_int]
    L.tsdf_resolution_supported.restype = ctypes.c_int
    L.tsdf_resolution_supported.argtypes = [ctypes.c_int]
    L.tsdf_default_cam.restype = None
    L.tsdf_default_cam.argtypes = [cam_p]
    lab_p, pca_p = ctypes.POINTER(TsdfLabels), ctypes.POINTER(TsdfPca)
    i, i64 = ctypes.c_int, ctypes.c_int64
    pack = [vp, i64, vp, vp, i, i, cam_p, i, vp]              # depth, depth_len, offsets, headers, n, R, cam, layout, stream
    indexed = [vp, i64, vp, vp, i64, vp, i, i, cam_p, i, vp]  # ... headers, n_pack, index, n, R, cam, layout, stream
    outs = [vp, vp, vp, vp]                                   # tsdf, max_l, mid_p, status
    entries = {
            "tsdf_voxelize_hip": pack + outs,
            "tsdf_voxelize_labels_hip": pack + outs + [lab_p],
            "tsdf_voxelize_grid_hip": pack + [vp, vp, vp],                       # grid, tsdf, status
            "tsdf_voxelize_aug_hip": pack + [vp] + outs,                         # xforms
            "tsdf_voxelize_aug_labels_hip": pack + [vp] + outs + [lab_p],
            "tsdf_voxelize_labels_pca_hip": pack + [vp] + outs + [lab_p, pca_p],
            "tsdf_aabb_hip": pack[:7] + [vp] + [vp, vp, vp, vp],                 # no layout; aabb, grid, ori, status
            "tsdf_voxelize_indexed_hip": indexed + outs + [lab_p],
            "tsdf_voxelize_indexed_host_hip": indexed + outs + [lab_p],
            "tsdf_voxelize_indexed_aug_hip": indexed + [vp] + outs + [lab_p],
            "tsdf_voxelize_indexed_pca_hip": indexed + [vp] + outs + [lab_p, pca_p],
            "tsdf_voxelize_indexed_host_pca_hip": indexed + outs + [lab_p, pca_p],
            "tsdf_host_gather_frames": [vp, vp, i64, vp, i64, vp, i64, vp, i],
            "tsdf_host_gather_frames_n": [vp, i64, vp, i64, vp, i64, vp, i64, vp, i],
            "tsdf_normalize_joints_hip": [vp, vp, vp, i, i, i, vp, vp],
            "tsdf_denormalize_joints_hip": [vp, vp, vp, i, i, vp, vp],
            "tsdf_stream_release": [vp],
            "tsdf_project_joints_hip": [vp, vp, vp, i, i, pca_p, vp],
            "tsdf_pose_error_hip": [vp, pca_p, vp, vp, vp, i, i, vp, vp, vp, vp, vp],
            "tsdf_point_clouds_hip": pack[:4] + [i, i, cam_p, ctypes.c_uint64, i64, vp, vp, vp, vp, vp],
            "tsdf_cloud_grid_hip": [vp, i, i, i, cam_p, vp, vp, vp, vp, vp, vp],
            "tsdf_describe_launch": [i, i, i, i, ctypes.c_char_p, i],
            "tsdf_debug_pixmap_hip": pack + [vp, vp, vp, vp],                    # grid, tsdf, pixmap, status
            "tsdf_debug_set_queue_word": [vp, ctypes.c_uint64],
    }
    _declare(L, {k: v for k, v in entries.items() if debug or not k.startswith("tsdf_debug_")})
    return L


def load():
    """Load libtsdf_hip.so once; raise loudly if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C handposeestimation-with-3d-cnns_amd/csrc`. There is no CPU fallback."
        )
    _lib = _bind(ctypes.CDLL(LIB_PATH), LIB_PATH)
    return _lib


def load_debug():
    """The debug build (include/tsdf_debug.h): the whole ABI plus tsdf_debug_pixmap_hip / tsdf_debug_set_queue_word, and
    TSDF_XCHG_POLLS read from the environment.  A library image of its own, with its own device-side state."""
    global _debug_lib
    if _debug_lib is not None:
        return _debug_lib
    if not os.path.exists(DEBUG_LIB_PATH):
        raise ImportError(f"{DEBUG_LIB_PATH} not found: build it with `make -C handposeestimation-with-3d-cnns_amd/csrc debug` "
                          "(__graft_entry__.build() does)")
    L = _bind(ctypes.CDLL(DEBUG_LIB_PATH), DEBUG_LIB_PATH, debug=True)
    _debug_lib = L
    return L


def _load_row(name: str, ext: _Ext):
    """Load libtsdf_<name>.so as its row ``ext`` describes it, once: the file must exist, its entry points are declared,
    its version must be the row's, and the library is kept in ``_ext_libs`` under ``name``; raise loudly if it is not there."""
    L = _ext_libs.get(name)
    if L is not None:
        return L
    if not os.path.exists(ext.path):
        raise ImportError(f"{ext.path} not found: build it with `make -C handposeestimation-with-3d-cnns_amd/csrc "
                          f"{name}` (__graft_entry__.build() does). There is no CPU fallback.")
    L = ctypes.CDLL(ext.path)
    _declare(L, {ext.version_symbol: [], **ext.entries})
    have = getattr(L, ext.version_symbol)()
    if have != ext.version:
        raise ImportError(f"{ext.path} has version {have}, this package needs {ext.version}: rebuild it "
                          f"(`make -C handposeestimation-with-3d-cnns_amd/csrc {name}`)")
    _ext_libs[name] = L
    return L


def _load_ext(name: str):
    """Load libtsdf_<name>.so, a row of the table, once (:func:`_load_row`)."""
    return _load_row(name, _EXTS[name])


def load_heatmap():
    """libtsdf_heatmap.so, the library of include/tsdf_heatmap.h (its row is ``_HEATMAP``)."""
    return _load_row("heatmap", _HEATMAP)


def load_heatloss():
    """libtsdf_heatloss.so, the library of include/tsdf_heatloss.h (its row is ``_HEATLOSS``)."""
    return _load_row("heatloss", _HEATLOSS)


def load_occupancy():
    """libtsdf_occupancy.so, the library of include/tsdf_occupancy.h (its row is ``_OCCUPANCY``)."""
    return _load_row("occupancy", _OCCUPANCY)


def load_fps():
    """libtsdf_fps.so, the library of include/tsdf_fps.h (its row is ``_FPS``)."""
    return _load_row("fps", _FPS)


def load_group():
    """libtsdf_group.so, the library of include/tsdf_group.h (its row is ``_GROUP``)."""
    return _load_row("group", _GROUP)


def load_pointfield():
    """libtsdf_pointfield.so, the library of include/tsdf_pointfield.h (its row is ``_POINTFIELD``)."""
    return _load_row("pointfield", _POINTFIELD)


def load_patch():
    """libtsdf_patch.so, the library of include/tsdf_patch.h (its row is ``_PATCH``)."""
    return _load_row("patch", _PATCH)


def load_augment():
    """libtsdf_augment.so, the library of include/tsdf_augment.h."""
    return _load_ext("augment")


def load_augstep():
    """libtsdf_augstep.so, the library of include/tsdf_augstep.h."""
    return _load_ext("augstep")


def load_auggrid():
    """libtsdf_auggrid.so, the library of include/tsdf_auggrid.h."""
    return _load_ext("auggrid")


def load_depth16():
    """libtsdf_depth16.so, the library of include/tsdf_depth16.h."""
    return _load_ext("depth16")


def load_obb():
    """libtsdf_obb.so, the library of include/tsdf_obb.h."""
    return _load_ext("obb")


def load_lowp():
    """libtsdf_lowp.so, the library of include/tsdf_lowp.h."""
    return _load_ext("lowp")


def load_maplowp():
    """libtsdf_maplowp.so, the library of include/tsdf_maplowp.h."""
    return _load_ext("maplowp")


def load_mapstep():
    """libtsdf_mapstep.so, the library of include/tsdf_mapstep.h."""
    return _load_ext("mapstep")


def load_locate():
    """libtsdf_locate.so, the library of include/tsdf_locate.h."""
    return _load_ext("locate")


def load_accurate():
    """libtsdf_accurate.so, the library of include/tsdf_accurate.h."""
    return _load_ext("accurate")


def load_mapaccurate():
    """libtsdf_mapaccurate.so, the library of include/tsdf_mapaccurate.h."""
    return _load_ext("mapaccurate")


@contextlib.contextmanager
def using_debug_library():
    """Inside the block every call of this package goes through the debug build instead of the product (tests that need a
    hook and the launches it acts on in ONE library image).  Not thread-safe; objects that cached the library at
    construction (dataset loaders) keep theirs."""
    global _lib
    prev = _lib
    _lib = load_debug()
    try:
        yield _lib
    finally:
        _lib = prev


def check(status: int, what: str):
    if status != TSDF_OK:
        msg = load().tsdf_strerror(status).decode()
        raise TsdfError(f"{what}: {msg} (status {status})")


def default_cam() -> TsdfCam:
    c = TsdfCam()
    load().tsdf_default_cam(ctypes.byref(c))
    return c
