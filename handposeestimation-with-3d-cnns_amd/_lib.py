"""ctypes binding of libtsdf_hip.so (the C ABI declared in include/tsdf.h).

There is deliberately NO fallback: if the HIP library is missing or fails to load,
importing the voxelizer raises.  The product path never routes through a CPU
implementation (the oracle under oracle/ is test infrastructure only).
"""
from __future__ import annotations

import contextlib
import ctypes
import os

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

_lib = None
_debug_lib = None
_augment_lib = None
_augstep_lib = None
_auggrid_lib = None
_depth16_lib = None


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
    for name, argtypes in {
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
    }.items():
        if not name.startswith("tsdf_debug_") or debug:
            fn = getattr(L, name)
            fn.restype = i
            fn.argtypes = argtypes
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


def load_augment():
    """Load libtsdf_augment.so once and declare its two entry points; raise loudly if it is not there."""
    global _augment_lib
    if _augment_lib is not None:
        return _augment_lib
    if not os.path.exists(AUGMENT_LIB_PATH):
        raise ImportError(f"{AUGMENT_LIB_PATH} not found: build it with `make -C handposeestimation-with-3d-cnns_amd/csrc "
                          "augment` (__graft_entry__.build() does). There is no CPU fallback.")
    L = ctypes.CDLL(AUGMENT_LIB_PATH)
    L.tsdf_augment_version.restype = ctypes.c_int
    L.tsdf_augment_version.argtypes = []
    if L.tsdf_augment_version() != AUGMENT_VERSION:
        raise ImportError(f"{AUGMENT_LIB_PATH} has version {L.tsdf_augment_version()}, this package needs "
                          f"{AUGMENT_VERSION}: rebuild it")
    vp = ctypes.c_void_p
    L.tsdf_aug_draw_hip.restype = ctypes.c_int
    # centres, n_src, index, n, key, counter0, stream, xforms, stretch, rot
    L.tsdf_aug_draw_hip.argtypes = [vp, ctypes.c_int64, vp, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, vp, vp, vp, vp]
    _augment_lib = L
    return L


def load_augstep():
    """Load libtsdf_augstep.so once and declare its two entry points; raise loudly if it is not there."""
    global _augstep_lib
    if _augstep_lib is not None:
        return _augstep_lib
    if not os.path.exists(AUGSTEP_LIB_PATH):
        raise ImportError(f"{AUGSTEP_LIB_PATH} not found: build it with `make -C handposeestimation-with-3d-cnns_amd/csrc "
                          "augstep` (__graft_entry__.build() does). There is no CPU fallback.")
    L = ctypes.CDLL(AUGSTEP_LIB_PATH)
    L.tsdf_augstep_version.restype = ctypes.c_int
    L.tsdf_augstep_version.argtypes = []
    if L.tsdf_augstep_version() != AUGSTEP_VERSION:
        raise ImportError(f"{AUGSTEP_LIB_PATH} has version {L.tsdf_augstep_version()}, this package needs "
                          f"{AUGSTEP_VERSION}: rebuild it")
    vp = ctypes.c_void_p
    L.tsdf_aug_draw_at_hip.restype = ctypes.c_int
    # centres, n_src, index, n, state, counters, stream, xforms, stretch, rot
    L.tsdf_aug_draw_at_hip.argtypes = [vp, ctypes.c_int64, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    _augstep_lib = L
    return L


def load_auggrid():
    """Load libtsdf_auggrid.so once and declare its three entry points; raise loudly if it is not there."""
    global _auggrid_lib
    if _auggrid_lib is not None:
        return _auggrid_lib
    if not os.path.exists(AUGGRID_LIB_PATH):
        raise ImportError(f"{AUGGRID_LIB_PATH} not found: build it with `make -C handposeestimation-with-3d-cnns_amd/csrc "
                          "auggrid` (__graft_entry__.build() does). There is no CPU fallback.")
    L = ctypes.CDLL(AUGGRID_LIB_PATH)
    L.tsdf_auggrid_version.restype = ctypes.c_int
    L.tsdf_auggrid_version.argtypes = []
    if L.tsdf_auggrid_version() != AUGGRID_VERSION:
        raise ImportError(f"{AUGGRID_LIB_PATH} has version {L.tsdf_auggrid_version()}, this package needs "
                          f"{AUGGRID_VERSION}: rebuild it")
    vp, i = ctypes.c_void_p, ctypes.c_int
    L.tsdf_voxelize_aug_grid_hip.restype = i
    # depth, depth_len, offsets, headers, n, R, cam, layout, stream, xforms, grid, tsdf, status
    L.tsdf_voxelize_aug_grid_hip.argtypes = [vp, ctypes.c_int64, vp, vp, i, i, ctypes.POINTER(TsdfCam), i, vp, vp, vp, vp, vp]
    L.tsdf_transform_joints_hip.restype = i
    # gt, xforms, n, n_joints, stream, gt_aug
    L.tsdf_transform_joints_hip.argtypes = [vp, vp, i, i, vp, vp]
    _auggrid_lib = L
    return L


def load_depth16():
    """Load libtsdf_depth16.so once and declare its two entry points; raise loudly if it is not there."""
    global _depth16_lib
    if _depth16_lib is not None:
        return _depth16_lib
    if not os.path.exists(DEPTH16_LIB_PATH):
        raise ImportError(f"{DEPTH16_LIB_PATH} not found: build it with `make -C handposeestimation-with-3d-cnns_amd/csrc "
                          "depth16` (__graft_entry__.build() does). There is no CPU fallback.")
    L = ctypes.CDLL(DEPTH16_LIB_PATH)
    L.tsdf_depth16_version.restype = ctypes.c_int
    L.tsdf_depth16_version.argtypes = []
    if L.tsdf_depth16_version() != DEPTH16_VERSION:
        raise ImportError(f"{DEPTH16_LIB_PATH} has version {L.tsdf_depth16_version()}, this package needs "
                          f"{DEPTH16_VERSION}: rebuild it")
    vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    L.tsdf_depth16_widen_hip.restype = i
    # src, n_px, shift, dst, stream
    L.tsdf_depth16_widen_hip.argtypes = [vp, i64, i, vp, vp]
    L.tsdf_depth16_host_gather.restype = i
    # src, src_len, src_offsets, n_src, index, n, dst, dst_len, dst_offsets, n_threads
    L.tsdf_depth16_host_gather.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, vp, i]
    _depth16_lib = L
    return L


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
