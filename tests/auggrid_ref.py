"""CPU reference of tsdf_voxelize_aug_grid_hip (include/tsdf_auggrid.h) for the tests: the oracle's own augmented voxel
arithmetic, ``tsdf_oracle_voxels_aug`` (oracle/tsdf_oracle.c), on a grid that is handed in, with the entry's status rules
applied in Python.  The two C functions used here are bound with ctypes in this file (oracle/ declares neither)."""
import ctypes

import numpy as np

import oracle

TOL = 1e-5    # the project's parity bound for the augmented entry (tests/test_parity_gpu.py::test_augmented_entry)
LAYOUTS = {"czyx": 0, "cxyz": 1, 0: 0, 1: 1}

_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = oracle.lib()
        fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
        dp, cp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(oracle.TsdfCam)
        # depth, header, ori, voxel_len, trunc_dis, R, cam, layout, xf, out
        L.tsdf_oracle_voxels_aug.restype = None
        L.tsdf_oracle_voxels_aug.argtypes = [fp, ip, fp, ctypes.c_float, ctypes.c_float, ctypes.c_int, cp, ctypes.c_int, dp,
                                             fp]
        # depth, header, cam, xf, min_p, max_p -> valid pixels
        L.tsdf_oracle_aabb_aug.restype = ctypes.c_long
        L.tsdf_oracle_aabb_aug.argtypes = [fp, ip, cp, dp, fp, fp]
        _bound = L
    return _bound


def _p(a, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct))


def identity_xforms(n):
    row = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] * 2, np.float64)
    return np.tile(row, (n, 1))


def header_ok(header, off0, off1, depth_len):
    """The voxelizer's header rule (oracle_frame / tests/cloud_grid_ref.py's callers) plus payload inside the buffer."""
    left, top, right, bottom = (int(v) for v in np.asarray(header)[2:6])
    bw, bh = right - left, bottom - top
    return 0 < bw <= 0x7fffffff and 0 < bh <= 0x7fffffff and bw * bh == off1 - off0 and off0 >= 0 and off1 <= depth_len


def grid_ok(row):
    """The grid row is usable: trunc_dis > 0 and voxel_len, trunc_dis, vox_ori all finite."""
    row = np.asarray(row, np.float32)
    return bool(row[4] > 0 and np.isfinite(row[:5]).all())


def voxels_aug(depth, header, ori, voxel_len, trunc_dis, R, layout, xf, cam=None):
    """tsdf_oracle_voxels_aug for one frame -> float32[3,R,R,R]."""
    depth = np.ascontiguousarray(depth, np.float32)
    header = np.ascontiguousarray(header, np.int32)
    ori = np.ascontiguousarray(ori, np.float32)
    xf = np.ascontiguousarray(xf, np.float64).reshape(24)
    out = np.empty((3, R, R, R), np.float32)
    _lib().tsdf_oracle_voxels_aug(_p(depth, ctypes.c_float), _p(header, ctypes.c_int32), _p(ori, ctypes.c_float),
                                  float(np.float32(voxel_len)), float(np.float32(trunc_dis)), int(R), oracle._cam(cam),
                                  LAYOUTS[layout], _p(xf, ctypes.c_double), _p(out, ctypes.c_float))
    return out


def aabb_aug(depth, header, xf, cam=None):
    """tsdf_oracle_aabb_aug for one frame -> (valid pixels, min float32[3], max float32[3])."""
    depth = np.ascontiguousarray(depth, np.float32)
    header = np.ascontiguousarray(header, np.int32)
    xf = np.ascontiguousarray(xf, np.float64).reshape(24)
    mn, mx = np.zeros(3, np.float32), np.zeros(3, np.float32)
    nv = _lib().tsdf_oracle_aabb_aug(_p(depth, ctypes.c_float), _p(header, ctypes.c_int32), oracle._cam(cam),
                                     _p(xf, ctypes.c_double), _p(mn, ctypes.c_float), _p(mx, ctypes.c_float))
    return int(nv), mn, mx


def pixel_grids(depth, off, hdr, xforms, R, cam=None):
    """float32[n,8] grid rows (vox_ori[3], voxel_len, trunc_dis, 0, 0, 0) that oracle.glue derives for the augmented AABB
    of all valid pixels — the placement of tsdf_voxelize_aug_hip —, and (max_l float32[n], mid_p float32[n,3]).  ``cam``
    (None, an oracle.TsdfCam or the five constants) goes to both: the AABB reads focal, cx, cy and invalid_eps, the glue
    trunc_voxels."""
    n = len(hdr)
    grid, max_l, mid_p = np.zeros((n, 8), np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    for i in range(n):
        nv, mn, mx = aabb_aug(depth[off[i]:off[i + 1]], hdr[i], xforms[i], cam)
        assert nv > 0
        g, ori = oracle.glue(mn, mx, R, cam)
        grid[i, :3], grid[i, 3], grid[i, 4] = ori, g[4], g[5]
        max_l[i], mid_p[i] = g[3], g[:3]
    return grid, max_l, mid_p


def voxelize_aug_grid_ref(depth, off, hdr, xforms, grid, R, layout, cam=None, depth_len=None):
    """(tsdf float32[n,3,R,R,R], status int32[n]) as tsdf_voxelize_aug_grid_hip defines them.  ``depth_len``: the length
    the entry is told (default: all of ``depth``); a frame whose payload is not inside it is a bad header."""
    depth = np.ascontiguousarray(depth, np.float32)
    off = np.asarray(off, np.int64)
    hdr = np.asarray(hdr, np.int32).reshape(-1, 6)
    xforms = np.asarray(xforms, np.float64).reshape(-1, 24)
    grid = np.asarray(grid, np.float32).reshape(-1, 8)
    n = hdr.shape[0]
    assert off.shape == (n + 1,) and xforms.shape[0] == n and grid.shape[0] == n
    depth_len = depth.size if depth_len is None else int(depth_len)
    tsdf = np.zeros((n, 3, R, R, R), np.float32)
    status = np.zeros(n, np.int32)
    for i in range(n):
        o0, o1 = int(off[i]), int(off[i + 1])
        if not header_ok(hdr[i], o0, o1, depth_len):
            status[i] = 2
        elif not grid_ok(grid[i]):
            status[i] = 1
        else:
            tsdf[i] = voxels_aug(depth[o0:o1], hdr[i], grid[i, :3], grid[i, 3], grid[i, 4], R, layout, xforms[i], cam)
    return tsdf, status


def near_counts(tsdf):
    """Per frame: voxels with a value strictly between 0 and 1 in magnitude (any channel), and non-zero voxels."""
    a = np.abs(np.asarray(tsdf))
    n = a.shape[0]
    near = ((a > 0) & (a < 1)).any(axis=1).reshape(n, -1).sum(axis=1)
    nonzero = (a != 0).any(axis=1).reshape(n, -1).sum(axis=1)
    return near, nonzero
