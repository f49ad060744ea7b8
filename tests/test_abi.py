"""CPU tier: the C-ABI library loads and exports every symbol include/tsdf.h declares.
No compute call is made (there is no GPU here); argument validation that happens before any
device work is exercised."""
import ctypes
import os
import re

import pytest
from abi_util import declared_functions, exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER, DEBUG_HEADER = "tsdf.h", "tsdf_debug.h"   # under include/


def test_header_declares_expected_entry_points():
    names = declared_functions(HEADER)
    for must in ("tsdf_voxelize_hip", "tsdf_voxelize_grid_hip", "tsdf_aabb_hip", "tsdf_version",
                 "tsdf_strerror", "tsdf_default_cam", "tsdf_resolution_supported"):
        assert must in names


def test_library_exports_every_declared_symbol(pkg):
    L = pkg._lib.load()
    for name in declared_functions(HEADER):
        assert hasattr(L, name), f"libtsdf_hip.so does not export {name}"
    assert L.tsdf_version() == 7
    assert b"no CPU fallback" in L.tsdf_strerror(-2)
    # exactly the header, nothing else: no test hook in the shipping library (ABI v7)
    assert exported(pkg._lib.LIB_PATH)[1] == declared_functions(HEADER)
    assert not [n for n in exported(pkg._lib.LIB_PATH)[1] if "debug" in n]


def test_debug_build_exports_the_product_abi_plus_the_hooks(pkg):
    """build/libtsdf_hip_debug.so (-DTSDF_DEBUG_HOOKS): everything include/tsdf.h declares plus include/tsdf_debug.h."""
    hooks = sorted(set(declared_functions(DEBUG_HEADER)) - set(declared_functions(HEADER)))
    assert hooks == ["tsdf_debug_pixmap_hip", "tsdf_debug_set_queue_word"]
    L = pkg._lib.load_debug()
    assert L.tsdf_version() == 7
    assert exported(pkg._lib.DEBUG_LIB_PATH)[1] == sorted(declared_functions(HEADER) + hooks)
    with pkg._lib.using_debug_library() as D:
        assert pkg._lib.load() is D
    assert pkg._lib.load() is not L


def test_default_cam_matches_reference_constants(pkg):
    cam = pkg.default_cam()  # pre/tsdf_numba.py:8-10, :87, :146
    assert (cam.focal, cam.cx, cam.cy) == (241.42, 160.0, 120.0)
    assert cam.invalid_eps == 1.0 and cam.trunc_voxels == 3.0


def test_resolution_rule(pkg):
    L = pkg._lib.load()
    assert [r for r in range(0, 140) if L.tsdf_resolution_supported(r)] == list(range(4, 129, 4))


def test_argument_validation_happens_before_device_work(pkg):
    L = pkg._lib.load()
    null = ctypes.c_void_p(0)
    # n == 0 is a no-op
    assert L.tsdf_voxelize_hip(null, 0, null, null, 0, 32, None, 0, null, null, null, null, null) == 0
    # bad resolution / layout / null outputs -> TSDF_ERR_INVALID_ARG, never a crash
    one = ctypes.c_void_p(16)
    assert L.tsdf_voxelize_hip(one, 16, one, one, 1, 30, None, 0, null, one, one, one, null) == -1
    assert L.tsdf_voxelize_hip(one, 16, one, one, 1, 32, None, 7, null, one, one, one, null) == -1
    assert L.tsdf_voxelize_hip(one, 16, one, one, 1, 32, None, 0, null, null, one, one, null) == -1
    assert L.tsdf_voxelize_hip(one, 16, one, one, -1, 32, None, 0, null, one, one, one, null) == -1
    assert L.tsdf_voxelize_grid_hip(one, 16, one, one, 1, 32, None, 0, null, null, one, null) == -1


def test_product_package_does_not_import_the_oracle():
    """The oracle is test infrastructure: nothing under the product package may reference it."""
    pkg_dir = os.path.join(ROOT, "handposeestimation-with-3d-cnns_amd")
    for dirpath, _, files in os.walk(pkg_dir):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, fn)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", text, flags=re.M), fn
                assert "libtsdf_oracle" not in text, fn


# ---- every run()-backed entry x every argument defect: the status the library returns before any device work --------------
# One row per (entry, defect): start from arguments that would be valid, break one thing.  The expected statuses are
# literals, recorded from the library as it was before the per-entry checks were consolidated; a row is either refused
# (-1) or a no-op (0, with n == 0) — none may get as far as a launch, the pointers are dummies.
_PACK = ("depth", "depth_len", "offsets", "headers", "n", "R", "cam", "layout", "stream")
_IDX = ("depth", "depth_len", "offsets", "headers", "n_pack", "index", "n", "R", "cam", "layout", "stream")
_OUTS = ("tsdf", "max_l", "mid_p", "status")
ENTRY_ARGS = {
    "tsdf_voxelize_hip": _PACK + _OUTS,
    "tsdf_voxelize_labels_hip": _PACK + _OUTS + ("labels",),
    "tsdf_voxelize_indexed_hip": _IDX + _OUTS + ("labels",),
    "tsdf_voxelize_indexed_host_hip": _IDX + _OUTS + ("labels",),
    "tsdf_voxelize_indexed_aug_hip": _IDX + ("xforms",) + _OUTS + ("labels",),
    "tsdf_voxelize_grid_hip": _PACK + ("grid", "tsdf", "status"),
    "tsdf_voxelize_aug_hip": _PACK + ("xforms",) + _OUTS,
    "tsdf_voxelize_aug_labels_hip": _PACK + ("xforms",) + _OUTS + ("labels",),
    "tsdf_aabb_hip": ("depth", "depth_len", "offsets", "headers", "n", "R", "cam", "stream", "aabb", "grid_out", "ori",
                      "status"),
    "tsdf_voxelize_labels_pca_hip": _PACK + ("xforms",) + _OUTS + ("labels", "pca"),
    "tsdf_voxelize_indexed_pca_hip": _IDX + ("xforms",) + _OUTS + ("labels", "pca"),
    "tsdf_voxelize_indexed_host_pca_hip": _IDX + _OUTS + ("labels", "pca"),
    "tsdf_debug_pixmap_hip": _PACK + ("grid", "tsdf", "pixmap", "status"),
}


def _defects(pkg):
    """name -> (the argument it breaks, its broken value).  ``labels`` / ``pca`` / ``cam`` values are structs (passed by
    reference); None is a NULL struct pointer."""
    null, lib = ctypes.c_void_p(0), pkg._lib
    nan = float("nan")
    d = {name + "_null": (name, null) for name in ("depth", "offsets", "headers", "tsdf", "max_l", "mid_p", "grid", "pixmap",
                                                   "index", "xforms")}
    d.update({
        "n_pack_neg": ("n_pack", -1), "n_pack_zero": ("n_pack", 0), "n_33": ("n", 33), "n_neg": ("n", -1),
        "R_30": ("R", 30), "layout_7": ("layout", 7), "depth_len_neg": ("depth_len", -1),
        "xforms_misaligned": ("xforms", ctypes.c_void_p(12)), "tsdf_misaligned": ("tsdf", ctypes.c_void_p(24)),
        "labels_null": ("labels", None), "joints_0": ("labels", lib.TsdfLabels(16, 0, 0, 16, None)),
        "joints_171": ("labels", lib.TsdfLabels(16, 171, 0, 16, None)),
        "gt_null": ("labels", lib.TsdfLabels(None, 21, 0, 16, None)),
        "gt_nor_null": ("labels", lib.TsdfLabels(16, 21, 0, None, None)),
        "pca_null": ("pca", None), "pca_k0": ("pca", lib.TsdfPca(16, 16, 0, 16)), "pca_k64": ("pca", lib.TsdfPca(16, 16, 64, 16)),
        "pca_mean_null": ("pca", lib.TsdfPca(None, 16, 10, 16)), "pca_coeff_null": ("pca", lib.TsdfPca(16, None, 10, 16)),
        "pca_out_null": ("pca", lib.TsdfPca(16, 16, 10, None)),
        "focal_0": ("cam", lib.TsdfCam(0.0, 160.0, 120.0, 1.0, 3.0)), "focal_nan": ("cam", lib.TsdfCam(nan, 160.0, 120.0, 1.0, 3.0)),
        "eps_0": ("cam", lib.TsdfCam(241.42, 160.0, 120.0, 0.0, 3.0)),
    })
    return d


def entry_rows(pkg):
    """Yields (entry, row name, n, call): every defect that applies to the entry at n == 1, then ``n0`` (n == 0 with
    otherwise valid arguments) and ``n0+defect`` (n == 0 together with the defect)."""
    one, null, lib = ctypes.c_void_p(16), ctypes.c_void_p(0), pkg._lib
    host_index = (ctypes.c_int64 * 64)()   # the _host entries read it on the host: real memory
    valid = dict(depth=one, depth_len=16, offsets=one, headers=one, n=1, R=32, cam=None, layout=0, stream=null, n_pack=4,
                 index=one, tsdf=one, max_l=one, mid_p=one, status=null, xforms=one, grid=one, pixmap=one, aabb=one,
                 grid_out=one, ori=one, labels=lib.TsdfLabels(16, 21, 0, 16, None), pca=lib.TsdfPca(16, 16, 10, 16))
    defects = _defects(pkg)

    def call(fn, names, values):
        def go():
            return fn(*[ctypes.byref(values[k]) if isinstance(values[k], ctypes.Structure) else values[k] for k in names])
        return go

    for entry, names in ENTRY_ARGS.items():
        L = lib.load_debug() if "debug" in entry else lib.load()
        base = dict(valid, index=host_index) if "_host" in entry else valid
        for n0 in (False, True):
            if n0:
                yield entry, "n0", 0, call(getattr(L, entry), names, dict(base, n=0))
            for dname, (field, value) in defects.items():
                if field not in names or (n0 and field == "n"):
                    continue
                values = dict(base, **{field: value})
                if n0:
                    values["n"] = 0
                yield entry, ("n0+" if n0 else "") + dname, values["n"], call(getattr(L, entry), names, values)


# entry -> {status: "row names"}
ENTRY_STATUS = {
    "tsdf_voxelize_hip": {
        -1: "depth_null offsets_null headers_null tsdf_null max_l_null mid_p_null n_neg R_30 layout_7 "
            "depth_len_neg tsdf_misaligned focal_0 focal_nan eps_0 n0+R_30 n0+layout_7 ",
        0: "n0 n0+depth_null n0+offsets_null n0+headers_null n0+tsdf_null n0+max_l_null n0+mid_p_null "
            "n0+depth_len_neg n0+tsdf_misaligned n0+focal_0 n0+focal_nan n0+eps_0 ",
    },
    "tsdf_voxelize_labels_hip": {
        -1: "depth_null offsets_null headers_null tsdf_null max_l_null mid_p_null n_neg R_30 layout_7 "
            "depth_len_neg tsdf_misaligned labels_null joints_0 joints_171 gt_null gt_nor_null focal_0 focal_nan "
            "eps_0 n0+R_30 n0+layout_7 n0+labels_null n0+joints_0 n0+joints_171 ",
        0: "n0 n0+depth_null n0+offsets_null n0+headers_null n0+tsdf_null n0+max_l_null n0+mid_p_null "
            "n0+depth_len_neg n0+tsdf_misaligned n0+gt_null n0+gt_nor_null n0+focal_0 n0+focal_nan n0+eps_0 ",
    },
    "tsdf_voxelize_indexed_hip": {
        -1: "depth_null offsets_null headers_null tsdf_null max_l_null mid_p_null index_null n_pack_neg "
            "n_pack_zero n_neg R_30 layout_7 depth_len_neg tsdf_misaligned joints_0 joints_171 gt_null "
            "gt_nor_null focal_0 focal_nan eps_0 n0+n_pack_neg n0+R_30 n0+layout_7 n0+joints_0 n0+joints_171 ",
        0: "n0 n0+depth_null n0+offsets_null n0+headers_null n0+tsdf_null n0+max_l_null n0+mid_p_null "
            "n0+index_null n0+n_pack_zero n0+depth_len_neg n0+tsdf_misaligned n0+labels_null n0+gt_null "
            "n0+gt_nor_null n0+focal_0 n0+focal_nan n0+eps_0 ",
    },
    "tsdf_voxelize_indexed_host_hip": {
        -1: "depth_null offsets_null headers_null tsdf_null max_l_null mid_p_null index_null n_pack_neg "
            "n_pack_zero n_33 n_neg R_30 layout_7 depth_len_neg tsdf_misaligned joints_0 joints_171 gt_null "
            "gt_nor_null focal_0 focal_nan eps_0 n0+n_pack_neg n0+R_30 n0+layout_7 n0+joints_0 n0+joints_171 ",
        0: "n0 n0+depth_null n0+offsets_null n0+headers_null n0+tsdf_null n0+max_l_null n0+mid_p_null "
            "n0+index_null n0+n_pack_zero n0+depth_len_neg n0+tsdf_misaligned n0+labels_null n0+gt_null "
            "n0+gt_nor_null n0+focal_0 n0+focal_nan n0+eps_0 ",
    },
    "tsdf_voxelize_indexed_aug_hip": {
        -1: "depth_null offsets_null headers_null tsdf_null max_l_null mid_p_null index_null xforms_null "
            "n_pack_neg n_pack_zero n_neg R_30 layout_7 depth_len_neg xforms_misaligned tsdf_misaligned joints_0 "
            "joints_171 gt_null gt_nor_null focal_0 focal_nan eps_0 n0+n_pack_neg n0+R_30 n0+layout_7 "
            "n0+xforms_misaligned n0+joints_0 n0+joints_171 ",
        0: "n0 n0+depth_null n0+offsets_null n0+headers_null n0+tsdf_null n0+max_l_null n0+mid_p_null "
            "n0+index_null n0+xforms_null n0+n_pack_zero n0+depth_len_neg n0+tsdf_misaligned n0+labels_null "
            "n0+gt_null n0+gt_nor_null n0+focal_0 n0+focal_nan n0+eps_0 ",
    },
    "tsdf_voxelize_grid_hip": {
        -1: "depth_null offsets_null headers_null tsdf_null grid_null n_neg R_30 layout_7 depth_len_neg "
            "tsdf_misaligned focal_0 focal_nan eps_0 n0+R_30 n0+layout_7 ",
        0: "n0 n0+depth_null n0+offsets_null n0+headers_null n0+tsdf_null n0+grid_null n0+depth_len_neg "
            "n0+tsdf_misaligned n0+focal_0 n0+focal_nan n0+eps_0 ",
    },
    "tsdf_voxelize_aug_hip": {
        -1: "depth_null offsets_null headers_null tsdf_null max_l_null mid_p_null xforms_null n_neg R_30 layout_7 "
            "depth_len_neg xforms_misaligned tsdf_misaligned focal_0 focal_nan eps_0 n0+R_30 n0+layout_7 "
            "n0+xforms_misaligned ",
        0: "n0 n0+depth_null n0+offsets_null n0+headers_null n0+tsdf_null n0+max_l_null n0+mid_p_null "
            "n0+xforms_null n0+depth_len_neg n0+tsdf_misaligned n0+focal_0 n0+focal_nan n0+eps_0 ",
    },
    "tsdf_voxelize_aug_labels_hip": {
        -1: "depth_null offsets_null headers_null tsdf_null max_l_null mid_p_null xforms_null n_neg R_30 layout_7 "
            "depth_len_neg xforms_misaligned tsdf_misaligned labels_null joints_0 joints_171 gt_null gt_nor_null "
            "focal_0 focal_nan eps_0 n0+R_30 n0+layout_7 n0+xforms_misaligned n0+labels_null n0+joints_0 "
            "n0+joints_171 ",
        0: "n0 n0+depth_null n0+offsets_null n0+headers_null n0+tsdf_null n0+max_l_null n0+mid_p_null "
            "n0+xforms_null n0+depth_len_neg n0+tsdf_misaligned n0+gt_null n0+gt_nor_null n0+focal_0 n0+focal_nan "
            "n0+eps_0 ",
    },
    "tsdf_aabb_hip": {
        -1: "depth_null offsets_null headers_null n_neg R_30 depth_len_neg focal_0 focal_nan eps_0 n0+R_30 ",
        0: "n0 n0+depth_null n0+offsets_null n0+headers_null n0+depth_len_neg n0+focal_0 n0+focal_nan n0+eps_0 ",
    },
    "tsdf_voxelize_labels_pca_hip": {
        -1: "depth_null offsets_null headers_null tsdf_null max_l_null mid_p_null n_neg R_30 layout_7 "
            "depth_len_neg xforms_misaligned tsdf_misaligned labels_null joints_0 joints_171 gt_null gt_nor_null "
            "pca_null pca_k0 pca_k64 pca_mean_null pca_coeff_null pca_out_null focal_0 focal_nan eps_0 n0+R_30 "
            "n0+layout_7 n0+xforms_misaligned n0+labels_null n0+joints_0 n0+joints_171 n0+pca_null n0+pca_k0 "
            "n0+pca_k64 ",
        0: "n0 n0+depth_null n0+offsets_null n0+headers_null n0+tsdf_null n0+max_l_null n0+mid_p_null "
            "n0+xforms_null n0+depth_len_neg n0+tsdf_misaligned n0+gt_null n0+gt_nor_null n0+pca_mean_null "
            "n0+pca_coeff_null n0+pca_out_null n0+focal_0 n0+focal_nan n0+eps_0 ",
    },
    "tsdf_voxelize_indexed_pca_hip": {
        -1: "depth_null offsets_null headers_null tsdf_null max_l_null mid_p_null index_null n_pack_neg "
            "n_pack_zero n_neg R_30 layout_7 depth_len_neg xforms_misaligned tsdf_misaligned labels_null joints_0 "
            "joints_171 gt_null gt_nor_null pca_null pca_k0 pca_k64 pca_mean_null pca_coeff_null pca_out_null "
            "focal_0 focal_nan eps_0 n0+n_pack_neg n0+R_30 n0+layout_7 n0+xforms_misaligned n0+labels_null "
            "n0+joints_0 n0+joints_171 n0+pca_null n0+pca_k0 n0+pca_k64 ",
        0: "n0 n0+depth_null n0+offsets_null n0+headers_null n0+tsdf_null n0+max_l_null n0+mid_p_null "
            "n0+index_null n0+xforms_null n0+n_pack_zero n0+depth_len_neg n0+tsdf_misaligned n0+gt_null "
            "n0+gt_nor_null n0+pca_mean_null n0+pca_coeff_null n0+pca_out_null n0+focal_0 n0+focal_nan n0+eps_0 ",
    },
    "tsdf_voxelize_indexed_host_pca_hip": {
        -1: "depth_null offsets_null headers_null tsdf_null max_l_null mid_p_null index_null n_pack_neg "
            "n_pack_zero n_33 n_neg R_30 layout_7 depth_len_neg tsdf_misaligned labels_null joints_0 joints_171 "
            "gt_null gt_nor_null pca_null pca_k0 pca_k64 pca_mean_null pca_coeff_null pca_out_null focal_0 "
            "focal_nan eps_0 n0+n_pack_neg n0+R_30 n0+layout_7 n0+labels_null n0+joints_0 n0+joints_171 "
            "n0+pca_null n0+pca_k0 n0+pca_k64 ",
        0: "n0 n0+depth_null n0+offsets_null n0+headers_null n0+tsdf_null n0+max_l_null n0+mid_p_null "
            "n0+index_null n0+n_pack_zero n0+depth_len_neg n0+tsdf_misaligned n0+gt_null n0+gt_nor_null "
            "n0+pca_mean_null n0+pca_coeff_null n0+pca_out_null n0+focal_0 n0+focal_nan n0+eps_0 ",
    },
    "tsdf_debug_pixmap_hip": {
        -1: "depth_null offsets_null headers_null tsdf_null pixmap_null n_neg R_30 layout_7 depth_len_neg "
            "tsdf_misaligned focal_0 focal_nan eps_0 n0+R_30 n0+layout_7 ",
        0: "n0 n0+depth_null n0+offsets_null n0+headers_null n0+tsdf_null n0+grid_null n0+pixmap_null "
            "n0+depth_len_neg n0+tsdf_misaligned n0+focal_0 n0+focal_nan n0+eps_0 ",
    },
}


def test_every_entry_refuses_every_argument_defect_before_device_work(pkg):
    want = {(e, r): st for e, by in ENTRY_STATUS.items() for st, rows in by.items() for r in rows.split()}
    assert set(ENTRY_STATUS) == set(ENTRY_ARGS) and len(want) > 500
    seen = set()
    for entry, row, n, call in entry_rows(pkg):
        if (entry, row) not in want:
            continue   # (a defect in an argument the entry treats as optional: the call would be valid)
        seen.add((entry, row))
        st = want[entry, row]
        assert st == -1 or (st == 0 and n == 0), (entry, row)   # no row may reach a launch
        assert call() == st, (entry, row)
    assert seen == set(want)
    for entry, by in ENTRY_STATUS.items():   # the rows every entry must have
        rows = set(" ".join(by.values()).split())
        assert {"n0", "n_neg", "R_30", "n0+R_30", "depth_len_neg", "focal_0", "focal_nan"} <= rows, entry


ARGTYPE_CODES = {
    "tsdf_aabb_hip": "pqppiiCppppp",
    "tsdf_cloud_grid_hip": "piiiCpppppp",
    "tsdf_debug_pixmap_hip": "pqppiiCippppp",
    "tsdf_debug_set_queue_word": "pQ",
    "tsdf_default_cam": "C",
    "tsdf_denormalize_joints_hip": "pppiipp",
    "tsdf_describe_launch": "iiiisi",
    "tsdf_host_gather_frames": "ppqpqpqpi",
    "tsdf_host_gather_frames_n": "pqpqpqpqpi",
    "tsdf_normalize_joints_hip": "pppiiipp",
    "tsdf_point_clouds_hip": "pqppiiCQqppppp",
    "tsdf_pose_error_hip": "pPpppiippppp",
    "tsdf_project_joints_hip": "pppiiPp",
    "tsdf_resolution_supported": "i",
    "tsdf_stream_release": "p",
    "tsdf_strerror": "i",
    "tsdf_version": "",
    "tsdf_voxelize_aug_hip": "pqppiiCipppppp",
    "tsdf_voxelize_aug_labels_hip": "pqppiiCippppppL",
    "tsdf_voxelize_grid_hip": "pqppiiCipppp",
    "tsdf_voxelize_hip": "pqppiiCippppp",
    "tsdf_voxelize_indexed_aug_hip": "pqppqpiiCippppppL",
    "tsdf_voxelize_indexed_hip": "pqppqpiiCipppppL",
    "tsdf_voxelize_indexed_host_hip": "pqppqpiiCipppppL",
    "tsdf_voxelize_indexed_host_pca_hip": "pqppqpiiCipppppLP",
    "tsdf_voxelize_indexed_pca_hip": "pqppqpiiCippppppLP",
    "tsdf_voxelize_labels_hip": "pqppiiCipppppL",
    "tsdf_voxelize_labels_pca_hip": "pqppiiCippppppLP",
}


def _code(t, lib):
    return {ctypes.c_void_p: "p", ctypes.c_int64: "q", ctypes.c_int: "i", ctypes.c_uint64: "Q", ctypes.c_char_p: "s",
            ctypes.POINTER(lib.TsdfCam): "C", ctypes.POINTER(lib.TsdfLabels): "L", ctypes.POINTER(lib.TsdfPca): "P"}[t]


def test_bound_argument_types_are_the_recorded_ones(pkg):
    """_lib._bind builds the argtypes lists from shared prefixes; element by element they are what was spelled out per
    entry before (p void*, q int64, i int, Q uint64, s char*, C/L/P pointers to tsdf_cam / tsdf_labels / tsdf_pca)."""
    L, D = pkg._lib.load(), pkg._lib.load_debug()
    for name, codes in ARGTYPE_CODES.items():
        fn = getattr(D if "debug" in name else L, name)
        assert "".join(_code(t, pkg._lib) for t in fn.argtypes) == codes, name
        assert fn.restype is (None if name == "tsdf_default_cam" else ctypes.c_char_p if name == "tsdf_strerror"
                              else ctypes.c_int), name
    assert set(ARGTYPE_CODES) == set(declared_functions(HEADER) + declared_functions(DEBUG_HEADER))
