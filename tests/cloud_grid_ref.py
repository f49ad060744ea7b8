"""Numpy restatement of tsdf_cloud_grid_hip (include/tsdf.h, "Grid placement from a point cloud") for the tests: the
extremes of pre/tsdf_for.py::max_min_point (x and y over all points, z over the points with z != 0, each rounded to
float32) and the float32 glue of tsdf_f (pre/tsdf_for.py:11-16), one rounding per operation, plus the not-OK rule.
numpy's float32 scalar and elementwise operations round once each.  Also the reader of tests/golden/process_ref_<k>.npz."""
import glob
import os

import numpy as np

F32 = np.float32


def extremes(points):
    """points float64[n, P, 3] -> (mn float32[n,3], mx float32[n,3], any_z bool[n], nan bool[n]).  An axis without a value
    has (+inf, -inf); NaN is reported, not propagated."""
    p = np.asarray(points, np.float64)
    assert p.ndim == 3 and p.shape[2] == 3 and p.shape[1] >= 1
    keep = np.ones(p.shape, bool)
    keep[:, :, 2] = p[:, :, 2] != 0          # the float64 value: -0.0 is dropped, a denormal and a NaN are kept
    nan = (np.isnan(p) & keep).any(axis=(1, 2))
    with np.errstate(over="ignore", invalid="ignore"):
        f = p.astype(F32)                    # rounding to nearest is monotone: min/max commute with it
    use = keep & ~np.isnan(p)
    mn = np.where(use, f, F32(np.inf)).min(axis=1)
    mx = np.where(use, f, F32(-np.inf)).max(axis=1)
    return mn, mx, keep[:, :, 2].any(axis=1), nan


def glue(mn, mx, R=32, trunc_voxels=3.0):
    """pre/tsdf_for.py:11-16 on float32[3] extremes: dict(mid_p, max_l, voxel_len, trunc, vox_ori), float32."""
    mn, mx = np.asarray(mn, F32), np.asarray(mx, F32)
    with np.errstate(all="ignore"):
        mid = (mx + mn) / F32(2)
        max_l = np.max(mx - mn)
        voxel_len = max_l / F32(R)
        trunc = voxel_len * F32(trunc_voxels)
        ori = mid - max_l / F32(2) + voxel_len / F32(2)
    return dict(mid_p=mid.astype(F32), max_l=F32(max_l), voxel_len=F32(voxel_len), trunc=F32(trunc), vox_ori=ori.astype(F32))


def cloud_grids(points, R=32, trunc_voxels=3.0):
    """(grid float32[n,8], max_l float32[n], mid_p float32[n,3], aabb float32[n,6], status int32[n]) as the kernel
    computes them."""
    mn, mx, any_z, nan = extremes(points)
    n = mn.shape[0]
    grid, max_l, mid_p = np.zeros((n, 8), F32), np.zeros(n, F32), np.zeros((n, 3), F32)
    aabb, status = np.zeros((n, 6), F32), np.zeros(n, np.int32)
    for i in range(n):
        if nan[i] or not any_z[i]:
            status[i] = 1
            continue
        aabb[i, :3], aabb[i, 3:] = mn[i], mx[i]
        g = glue(mn[i], mx[i], R, trunc_voxels)
        mid_ok = bool(np.isfinite(g["mid_p"]).all())
        if not (g["max_l"] > 0) or not np.isfinite(g["max_l"]) or not mid_ok:
            status[i] = 1
            if mid_ok:
                mid_p[i] = g["mid_p"]
            continue
        grid[i, :3], grid[i, 3], grid[i, 4] = g["vox_ori"], g["voxel_len"], g["trunc"]
        max_l[i], mid_p[i] = g["max_l"], g["mid_p"]
    return grid, max_l, mid_p, aabb, status


def same_values(a, b) -> bool:
    """Equal as float32 values (+0 == -0), NaN by position."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]))


def recorded(golden_dir):
    """[(name, record)] of every process_ref fixture, in file order."""
    out = []
    files = sorted(glob.glob(os.path.join(golden_dir, "process_ref_*.npz")))
    assert files, "tests/golden/process_ref_*.npz missing (tools/make_goldens.py --only process)"
    for fn in files:
        z = np.load(fn)
        for i, name in enumerate(z["names"]):
            out.append((str(name), {k[len(f"f{i}_"):]: z[k] for k in z.files if k.startswith(f"f{i}_")}))
    return out


def frames_and_clouds(mg, golden_dir):
    """(name, header, depth, cloud, record): the fixtures' frames made again, their digests checked."""
    by_name = {name: (h, d) for name, h, d in mg.volume_frames()}
    for name, g in recorded(golden_dir):
        h, d = by_name[name.split("@")[0]]
        assert str(g["depth_sha256"]) == mg.depth_digest(d), f"{name}: the generator no longer makes the recorded frame"
        cloud = mg.process_cloud(h, d, int(g["P"]), int(g["seed"]))
        assert str(g["cloud_sha256"]) == mg.cloud_digest(cloud), f"{name}: the cloud rule no longer makes the recorded cloud"
        yield name, h, d, cloud, g
