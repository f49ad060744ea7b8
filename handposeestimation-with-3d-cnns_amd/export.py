"""Offline preprocessing in the reference's on-disk schema — one GPU launch per gesture.

The reference driver (pre/read_MSRA.py:37-140) walks ``<DB>/<subject>/<gesture>/``, voxelizes every
frame on the CPU (~0.2 s each) and writes, per subject directory under ``./result``:

    TSDF/<gesture>.npz          tsdf[n,3,32,32,32], max_l[n], mid_p[n,3]     (:119-120)
    ground_truth/<gesture>.npy  gt[n,63]                                      (:121-122)
    num/<gesture>.npy           n (scalar)                                    (:123-124)
    Point_Cloud/<gesture>.npy   [n,6000,3] random resample of the point cloud (:117-118)
    ../data_num-<subject>.npy   frames of the subject (scalar)                (:139)

and, with its AUG switch on, four twins of the augmented frames (:68-75,86-91,112-117,128-136):

    Point_Cloud_aug/<g>.npy     TSDF_aug/<g>.npz (tsdf, max_l, mid_p)     ground_truth_aug/<g>.npy     num_aug/<g>.npy

which is what ``3D_CNN/dataset.py:93-131`` reads back.  ``preprocess_tree`` writes the same files with the
voxelization done by the HIP kernel: a gesture (~500 frames) is packed (``packing.pack_bin_files``), uploaded
once and voxelized in one launch.

Differences from the reference writer, all deliberate, each with the switch that undoes it:
  * grid placement uses ALL valid pixels (the numba path), not the random 6000-point
    resample ``DataProcess.process()`` uses — the files do not depend on the draw.  ``placement="cloud"`` gives the
    reference's rule back: ``TSDF/<g>.npz`` is then voxelized on the grid of the very cloud that is written to
    ``Point_Cloud/<g>.npy`` (``voxelize.cloud_grids`` + ``voxelize_grid``), so the saved ``max_l`` / ``mid_p`` are a
    function of the saved cloud, as in the reference's files.  It needs ``point_clouds`` on.  The ``_aug`` twins have a
    switch of their own, independent of this one: with ``aug_placement="pixels"`` (the default) they keep the all-pixels
    placement of the fused augmented voxelizer; with ``aug_placement="cloud"`` ``TSDF_aug/<g>.npz`` is voxelized on the
    grid of the very cloud that is written to ``Point_Cloud_aug/<g>.npy`` (``voxelize.cloud_grids`` +
    ``voxelize_aug_grid``), so ``max_l_aug`` / ``mid_p_aug`` belong to the cloud saved next to them.  Either way their
    maps are centred on the plain ``mid_p`` that was written, and ``pca_dir`` uses the ``max_l`` / ``mid_p`` that were
    written;
  * arrays are float32 (the reader casts to float32 anyway, 3D_CNN/dataset.py:101-103); ``dtype=np.float64``
    gives the reference's ``np.empty`` default back;
  * layout is ``[c,x,y,z]`` — what the reference writer produced, since it went through the CPU loop
    (pre/tsdf_for.py:118-120); pass ``layout="czyx"`` for the numba layout;
  * a ``status`` array is added to the npz (0 ok / 1 degenerate / 2 bad header): the reference crashes or
    writes garbage for such frames;
  * ``gt_3d=True`` stores the labels as ``[n,21,3]`` WITH z NEGATED — the only form the reference reader handles
    (3D_CNN/dataset.py:107-109 negates z of 3-D label arrays, pairing with the commented-out writer lines
    pre/read_MSRA.py:81-82 that pre-negate it; for the ``[n,63]`` array its own writer saves, ``g_t`` is undefined).
    After the reader's flip the labels are back in the camera frame (z = -depth) that ``mid_p`` lives in.

``aug=True`` writes the twins too (``DataProcess(aug=True)`` re-specified, process.py): each frame's map comes from
``augment.random_affines`` centred on the frame's plain grid centre ``mid_p``; ``TSDF_aug`` is the fused augmented
voxelization under that map (``voxelize_aug``, same res / layout / dtype, plus ``status`` and the map itself as ``xform``
float64[n,24]; with ``aug_placement="cloud"`` the same map on the grid of the saved augmented cloud, ``voxelize_aug_grid``),
``ground_truth_aug`` the joints under the same map, ``Point_Cloud_aug`` the mapped cloud.
``data_num-<subject>.npy`` keeps counting plain frames, as the reference does.

Random draws.  ``rng`` feeds the plain files only and ``aug_rng`` the augmented ones, so ``aug=True`` leaves every
plain file byte-identical to an ``aug=False`` run with the same ``rng``.  Per gesture, in this order:
  * ``point_clouds="host"`` (or True): the plain cloud draws from ``rng`` (``resample_point_clouds``); the maps come
    from ``aug_rng``, then the augmented cloud draws from ``aug_rng``;
  * ``point_clouds="device"``: the plain cloud is ``voxelize.point_clouds(seed=rng.integers(0, 2**63))``; the maps
    come from ``aug_rng``, then the augmented cloud is ``point_clouds(seed=aug_rng.integers(0, 2**63), xforms=maps)``;
    both with ``frame_base=0``.  Replaying the two generators reproduces every file.
``aug_placement`` changes neither the draws nor their order: the voxelization draws nothing.

``pca_dir`` adds what ``read_MSRA.main()`` ends with (``joint_pca(aug=False)``, pre/joint_pca.py): the nine
leave-one-subject-out joint-PCA fits ``<pca_dir>/<fold>.npz``, fold t fitted on the normalised labels of every subject
but the t-th — re-specified (``pca.py``), from the max_l / mid_p / labels already in memory.  With ``aug=True`` also
``<fold>-aug.npz`` (``joint_pca(aug=True)``, pre/joint_pca.py:29-36): the same fold fitted on its plain labels stacked
over its augmented ones, the latter normalised with the ``TSDF_aug`` grid.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, Optional, Sequence

import numpy as np

from . import packing

_SUBDIRS = ("Point_Cloud", "TSDF", "ground_truth", "num")
_AUG_SUBDIRS = tuple(d + "_aug" for d in _SUBDIRS)


def _voxelize_pack(pk: packing.PackedFrames, res: int, layout: str, device, *, cloud: Optional[np.ndarray] = None,
                   xforms: Optional[np.ndarray] = None, gt: Optional[np.ndarray] = None, tsdf: str = "projective"):
    """The one body of the default hooks below: upload the pack (and ``xforms`` / ``cloud`` / ``gt``), place the grid, run
    the voxel pass, map the joints, combine the status, synchronise, copy to the host: ``(tsdf, max_l, mid_p, status)``,
    with ``gt`` a fifth, the joints under ``xforms``.  With ``cloud`` (host float64[n, P, 3]) the grid is placed on it
    (``voxelize.cloud_grids``), ``voxelize._grid_pass`` names the pass and ``status`` is the first non-zero of the two; without
    it the grid is on all valid pixels: the fused ``voxelize`` / ``voxelize_aug``, or ``voxelize_accurate``."""
    import torch

    from .voxelize import (TsdfBatch, _first_status, _grid_pass, cloud_grids, transform_joints, voxelize, voxelize_accurate,
                           voxelize_aug)

    if (xforms is None) != (gt is None) or (tsdf == "accurate" and xforms is not None):
        raise ValueError('xforms and gt come together, and not with tsdf="accurate": that pass is not reached from here')
    depth, offsets, headers = pk.to_torch(device, pin=True, non_blocking=True)

    def up(a, dtype):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(depth.device)
    xf, pts = up(xforms, np.float64), up(cloud, np.float64)
    g = up(None if gt is None else np.asarray(gt, np.float32).reshape(len(pk), -1), np.float32)
    gt_aug = None
    if pts is not None:
        cg = cloud_grids(pts, res=res)
        vol, st = _grid_pass(depth, offsets, headers, cg.grid, res=res, layout=layout, cam=None, xforms=xf, tsdf=tsdf)
        gt_aug = transform_joints(g, xf) if g is not None else None
        out = TsdfBatch(vol, cg.max_l, cg.mid_p, _first_status(cg.status, st))
    elif xf is not None:
        out, _, gt_aug = voxelize_aug(depth, offsets, headers, xf, res=res, layout=layout, gt=g)
    elif tsdf == "accurate":
        out = voxelize_accurate(depth, offsets, headers, res=res, layout=layout)
    else:
        out = voxelize(depth, offsets, headers, res=res, layout=layout)
    torch.cuda.synchronize(depth.device)
    return tuple(t.cpu().numpy() for t in (*out, gt_aug) if t is not None)


def _default_voxelize(pk: packing.PackedFrames, res: int, layout: str, device):
    """Upload + one launch; returns host arrays (tsdf, max_l, mid_p, status)."""
    return _voxelize_pack(pk, res, layout, device)


def _default_voxelize_accurate(pk: packing.PackedFrames, res: int, layout: str, device):
    """:func:`_default_voxelize` with the accurate directional TSDF (``voxelize.voxelize_accurate``): volumes alone differ."""
    return _voxelize_pack(pk, res, layout, device, tsdf="accurate")


def _default_voxelize_aug(pk: packing.PackedFrames, xforms: np.ndarray, gt: np.ndarray, res: int, layout: str, device):
    """Upload + one augmented launch with the labels: host arrays (tsdf, max_l, mid_p, status, gt_aug)."""
    return _voxelize_pack(pk, res, layout, device, xforms=xforms, gt=gt)


def _default_voxelize_cloud(pk: packing.PackedFrames, cloud: np.ndarray, res: int, layout: str, device):
    """Upload the pack and its clouds; grid placement from each cloud, then the volumes on that placement: host arrays
    (tsdf, max_l, mid_p, status), status being the first non-zero of the two stages."""
    return _voxelize_pack(pk, res, layout, device, cloud=cloud)


def _default_voxelize_cloud_accurate(pk: packing.PackedFrames, cloud: np.ndarray, res: int, layout: str, device):
    """:func:`_default_voxelize_cloud` with the accurate directional TSDF (``voxelize.voxelize_grid_accurate``) on the
    cloud's placement."""
    return _voxelize_pack(pk, res, layout, device, cloud=cloud, tsdf="accurate")


def _default_voxelize_aug_cloud(pk: packing.PackedFrames, xforms: np.ndarray, cloud_aug: np.ndarray, gt: np.ndarray,
                                res: int, layout: str, device):
    """:func:`_default_voxelize_cloud` under the maps (``voxelize.voxelize_aug_grid`` on the augmented cloud's placement), and
    the joints under them: host arrays (tsdf, max_l, mid_p, status, gt_aug)."""
    return _voxelize_pack(pk, res, layout, device, cloud=cloud_aug, xforms=xforms, gt=gt)


# the default plain hook of preprocess_tree by (tsdf, placement): module-level NAMES, resolved when it is called
_PLAIN_HOOKS = {("projective", "pixels"): "_default_voxelize", ("accurate", "pixels"): "_default_voxelize_accurate",
                ("projective", "cloud"): "_default_voxelize_cloud", ("accurate", "cloud"): "_default_voxelize_cloud_accurate"}


def device_point_clouds(pk: packing.PackedFrames, points_num: int, seed: int, xforms: Optional[np.ndarray] = None,
                        device="cuda") -> np.ndarray:
    """``voxelize.point_clouds`` on a pack (upload, one launch, ``frame_base=0``): host ``float64[n, points_num, 3]``."""
    import torch

    from .voxelize import point_clouds

    depth, offsets, headers = pk.to_torch(device, pin=True, non_blocking=True)
    xf = None if xforms is None else torch.from_numpy(np.ascontiguousarray(xforms, np.float64)).to(depth.device)
    out = point_clouds(depth, offsets, headers, points=points_num, seed=seed, xforms=xf)
    return out.points.cpu().numpy()


def _map_points(pts: np.ndarray, xform: np.ndarray) -> np.ndarray:
    """The forward map of ``tsdf_point_clouds_hip`` (include/tsdf.h): (A_i0 x + A_i1 y) + (A_i2 z + b_i), float64,
    products and sums rounded separately."""
    f = np.asarray(xform, np.float64).reshape(24)[:12].reshape(3, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([(f[k, 0] * x + f[k, 1] * y) + (f[k, 2] * z + f[k, 3]) for k in range(3)], axis=1)


def resample_point_clouds(pk: packing.PackedFrames, points_num: int = 6000,
                          rng: Optional[np.random.Generator] = None, xforms: Optional[np.ndarray] = None) -> np.ndarray:
    """``DataProcess.point_cloud`` + ``set_length`` (pre/process.py:30-84) for every frame of a pack:
    ``float64[n, points_num, 3]``.  Frames without any non-zero point give zeros.  ``xforms`` float64[n, 24]: each
    frame's cloud is mapped with its forward rows (as ``tsdf_point_clouds_hip`` maps them) before it is resampled."""
    from .process import DataProcess

    rng = rng if rng is not None else np.random.default_rng()
    n = len(pk)
    out = np.zeros((n, points_num, 3), np.float64)
    for i in range(n):
        header, depth = pk.frame(i)
        pts = DataProcess({"header": header, "depth": depth}, None, points_num).point_cloud()
        if xforms is not None:
            pts = _map_points(pts, xforms[i])
        m = pts.shape[0]
        if m == 0:
            continue
        if m < points_num:  # keep every point once, fill up with replacement (pre/process.py:74-79)
            idx = np.arange(points_num)
            idx[m:] = rng.integers(0, m, size=points_num - m)
        else:
            idx = rng.integers(0, m, size=points_num)
        out[i] = pts[idx]
    return out


def write_gesture(sub_dir: str, gesture: str, tsdf: np.ndarray, max_l: np.ndarray, mid_p: np.ndarray,
                  ground_truth: np.ndarray, status: Optional[np.ndarray] = None,
                  point_cloud: Optional[np.ndarray] = None, gt_3d: bool = False) -> None:
    """The four per-gesture files of pre/read_MSRA.py:117-124 (directories are created as needed)."""
    for d in _SUBDIRS:
        os.makedirs(os.path.join(sub_dir, d), exist_ok=True)
    n = int(tsdf.shape[0])
    extra = {} if status is None else {"status": np.asarray(status, np.int32)}
    np.savez(os.path.join(sub_dir, "TSDF", "%s.npz" % gesture), tsdf=tsdf, max_l=max_l, mid_p=mid_p, **extra)
    gt = np.asarray(ground_truth, np.float32).reshape(n, -1)
    if gt_3d:
        gt = gt.reshape(n, 21, 3).copy()
        gt[:, :, 2] = -gt[:, :, 2]  # the reference reader flips it back (3D_CNN/dataset.py:107-109)
    np.save(os.path.join(sub_dir, "ground_truth", "%s.npy" % gesture), gt)
    np.save(os.path.join(sub_dir, "num", "%s.npy" % gesture), n)
    if point_cloud is not None:
        np.save(os.path.join(sub_dir, "Point_Cloud", "%s.npy" % gesture), point_cloud)


def write_gesture_aug(sub_dir: str, gesture: str, tsdf: np.ndarray, max_l: np.ndarray, mid_p: np.ndarray,
                      ground_truth: np.ndarray, status: np.ndarray, xforms: np.ndarray,
                      point_cloud: Optional[np.ndarray] = None, gt_3d: bool = False) -> None:
    """The four augmented twins of pre/read_MSRA.py:112-117,128-136 (``TSDF_aug`` gains ``status`` and ``xform``)."""
    for d in _AUG_SUBDIRS:
        os.makedirs(os.path.join(sub_dir, d), exist_ok=True)
    n = int(tsdf.shape[0])
    np.savez(os.path.join(sub_dir, "TSDF_aug", "%s.npz" % gesture), tsdf=tsdf, max_l=max_l, mid_p=mid_p,
             status=np.asarray(status, np.int32), xform=np.asarray(xforms, np.float64).reshape(n, 24))
    gt = np.asarray(ground_truth, np.float32).reshape(n, -1)
    if gt_3d:
        gt = gt.reshape(n, 21, 3).copy()
        gt[:, :, 2] = -gt[:, :, 2]
    np.save(os.path.join(sub_dir, "ground_truth_aug", "%s.npy" % gesture), gt)
    np.save(os.path.join(sub_dir, "num_aug", "%s.npy" % gesture), n)
    if point_cloud is not None:
        np.save(os.path.join(sub_dir, "Point_Cloud_aug", "%s.npy" % gesture), point_cloud)


def preprocess_tree(db_dir: str, save_dir: str, *, res: int = 32, layout: str = "cxyz", dtype=np.float32,
                    points_num: int = 6000, point_clouds=True, gt_3d: bool = False,
                    subjects: Optional[Sequence[str]] = None, gestures: Optional[Sequence[str]] = None,
                    device="cuda", rng: Optional[np.random.Generator] = None,
                    voxelize_fn: Optional[Callable] = None, verbose: bool = False,
                    pca_dir: Optional[str] = None, aug: bool = False,
                    aug_rng: Optional[np.random.Generator] = None,
                    voxelize_aug_fn: Optional[Callable] = None, placement: str = "pixels",
                    voxelize_cloud_fn: Optional[Callable] = None, aug_placement: str = "pixels",
                    voxelize_aug_cloud_fn: Optional[Callable] = None, tsdf: str = "projective") -> Dict[str, int]:
    """Replacement for ``read_MSRA.main()`` (pre/read_MSRA.py:37-140): voxelize a whole MSRA tree into ``save_dir`` in
    the reference's schema (with ``aug=True`` its AUG=True schema).  Returns ``{subject: frames}``.

    ``voxelize_fn(pack, res, layout, device) -> (tsdf, max_l, mid_p, status)`` and
    ``voxelize_aug_fn(pack, xforms, gt, res, layout, device) -> (tsdf, max_l, mid_p, status, gt_aug)`` may replace the
    HIP calls (tests use them to check the file handling without a GPU); by default the HIP voxelizer runs and a
    missing library or device is an error.

    ``placement``: "pixels" (default: the grid on all valid pixels) or "cloud" (the reference's rule: the grid on the
    resampled cloud that is written to ``Point_Cloud``; needs ``point_clouds``).  With "cloud" the plain volumes come from
    ``voxelize_cloud_fn(pack, cloud, res, layout, device) -> (tsdf, max_l, mid_p, status)``, ``cloud`` being the host
    ``float64[n, points_num, 3]`` array that is saved (default: ``voxelize.cloud_grids`` + ``voxelize_grid``), and
    ``voxelize_fn`` is not called.  The random draws and their order are those of the module docstring either way.

    ``aug_placement`` (the ``_aug`` twins, independent of ``placement``): "pixels" (default: the fused augmented voxelizer,
    grid on all mapped valid pixels) or "cloud" (the grid on the augmented cloud that is written to ``Point_Cloud_aug``;
    needs ``aug=True`` and ``point_clouds``).  With "cloud" the augmented volumes and labels come from
    ``voxelize_aug_cloud_fn(pack, xforms, cloud_aug, gt, res, layout, device) -> (tsdf, max_l, mid_p, status, gt_aug)``,
    ``cloud_aug`` being the host array that is saved (default: ``voxelize.cloud_grids`` + ``voxelize_aug_grid`` +
    ``transform_joints``), and ``voxelize_aug_fn`` is not called.

    ``point_clouds``: True / "host" (``resample_point_clouds`` on the host), "device" (``voxelize.point_clouds``) or
    False (no cloud files).  The draws of each are in the module docstring.

    ``tsdf``: "projective" (default) or "accurate": the DEFAULT ``voxelize_fn`` / ``voxelize_cloud_fn`` write the accurate
    directional TSDF — per voxel the nearest surface point among all valid pixels (``voxelize.voxelize_accurate``;
    with ``placement="cloud"`` ``cloud_grids`` + ``voxelize_grid_accurate``) — into ``TSDF/<g>.npz``: the same schema, max_l,
    mid_p and status, so the tree is read by the reference's own train.py unchanged.  Hooks the caller passes are called as
    they are.  ``aug=True`` with ``tsdf="accurate"`` is a ``ValueError``: the accurate pass under a per-frame map is not
    there yet.

    ``pca_dir``: also write the joint-PCA fits of the first nine subjects' leave-one-out folds there (``pca.JointPCA``
    files, ``<fold>.npz``, and with ``aug=True`` ``<fold>-aug.npz``): the labels are normalised with each frame's own
    max_l / mid_p (no clamp) and frames whose status is not OK are left out."""
    if point_clouds is True:
        point_clouds = "host"
    if point_clouds not in (False, None, "host", "device"):
        raise ValueError('point_clouds must be True / "host", "device" or False')
    if placement not in ("pixels", "cloud"):
        raise ValueError('placement must be "pixels" or "cloud"')
    if placement == "cloud" and not point_clouds:
        raise ValueError('placement="cloud" places the grid on the saved cloud: it needs point_clouds="host" or "device"')
    if aug_placement not in ("pixels", "cloud"):
        raise ValueError('aug_placement must be "pixels" or "cloud"')
    if aug_placement == "cloud" and not (aug and point_clouds):
        raise ValueError('aug_placement="cloud" places the grid on the saved augmented cloud: it needs aug=True and '
                         'point_clouds="host" or "device"')
    if tsdf not in ("projective", "accurate"):
        raise ValueError('tsdf must be "projective" or "accurate"')
    if tsdf == "accurate" and aug:
        raise ValueError('tsdf="accurate" has no augmented twin yet (the accurate pass under a per-frame map): use aug=False')
    vox = voxelize_fn if voxelize_fn is not None else globals()[_PLAIN_HOOKS[tsdf, "pixels"]]
    vox_cloud = voxelize_cloud_fn if voxelize_cloud_fn is not None else globals()[_PLAIN_HOOKS[tsdf, "cloud"]]
    vox_aug = voxelize_aug_fn if voxelize_aug_fn is not None else _default_voxelize_aug
    vox_aug_cloud = voxelize_aug_cloud_fn if voxelize_aug_cloud_fn is not None else _default_voxelize_aug_cloud
    rng = rng if rng is not None else np.random.default_rng()
    if aug:
        aug_rng = aug_rng if aug_rng is not None else np.random.default_rng()
    os.makedirs(save_dir, exist_ok=True)
    subs = list(subjects) if subjects is not None else sorted(
        d for d in os.listdir(db_dir) if os.path.isdir(os.path.join(db_dir, d)))
    totals: Dict[str, int] = {}
    labels: Dict[str, list] = {}   # pca_dir: the normalised labels of the OK frames, per subject
    labels_aug: Dict[str, list] = {}   # ... and of the OK augmented frames (aug=True)
    for sub in subs:
        sub_in, sub_out = os.path.join(db_dir, sub), os.path.join(save_dir, sub)
        ges_list = list(gestures) if gestures is not None else sorted(
            g for g in os.listdir(sub_in) if os.path.isdir(os.path.join(sub_in, g)))
        total = 0
        for ges in ges_list:
            g_dir = os.path.join(sub_in, ges)
            bin_num, gt = packing.read_joint(g_dir)
            pk = packing.pack_bin_files(packing.gesture_bin_paths(g_dir, bin_num))
            if placement == "pixels":
                tsdf, max_l, mid_p, status = vox(pk, res, layout, device)
            pc = None
            if point_clouds == "host":
                pc = resample_point_clouds(pk, points_num, rng)
            elif point_clouds == "device":
                pc = device_point_clouds(pk, points_num, int(rng.integers(0, 2 ** 63)), device=device)
            if placement == "cloud":
                tsdf, max_l, mid_p, status = vox_cloud(pk, pc, res, layout, device)
            if pca_dir is not None:
                from .pca import normalize_labels_np
                ok = np.asarray(max_l, np.float32) > 0 if status is None else np.asarray(status) == 0
                labels.setdefault(sub, []).append(normalize_labels_np(gt, max_l, mid_p)[ok])
            write_gesture(sub_out, ges, np.asarray(tsdf, dtype), np.asarray(max_l, dtype),
                          np.asarray(mid_p, dtype), gt, status, pc, gt_3d)
            if aug:
                from .augment import random_affines
                xf = random_affines(np.asarray(mid_p, np.float64), rng=aug_rng)[0]
                if aug_placement == "pixels":
                    tsdf_a, max_l_a, mid_p_a, status_a, gt_a = vox_aug(pk, xf, gt, res, layout, device)
                pc_a = None
                if point_clouds == "host":
                    pc_a = resample_point_clouds(pk, points_num, aug_rng, xforms=xf)
                elif point_clouds == "device":
                    pc_a = device_point_clouds(pk, points_num, int(aug_rng.integers(0, 2 ** 63)), xf, device=device)
                if aug_placement == "cloud":
                    tsdf_a, max_l_a, mid_p_a, status_a, gt_a = vox_aug_cloud(pk, xf, pc_a, gt, res, layout, device)
                if pca_dir is not None:
                    from .pca import normalize_labels_np
                    ok = np.asarray(status_a) == 0
                    labels_aug.setdefault(sub, []).append(normalize_labels_np(gt_a, max_l_a, mid_p_a)[ok])
                write_gesture_aug(sub_out, ges, np.asarray(tsdf_a, dtype), np.asarray(max_l_a, dtype),
                                  np.asarray(mid_p_a, dtype), gt_a, status_a, xf, pc_a, gt_3d)
            total += bin_num
            if verbose:
                print("%s-%s files saved." % (sub, ges))
        np.save(os.path.join(save_dir, "data_num-%s.npy" % sub), total)
        totals[sub] = total
    if pca_dir is not None:
        from .pca import fit_labels
        folds = subs[:9]   # (pre/joint_pca.py:17: sorted(os.listdir(result))[:9])
        for t in range(len(folds)):
            u = [x for s in folds if s != folds[t] for x in labels.get(s, [])]
            fit_labels(np.concatenate(u) if u else np.zeros((0, 63), np.float32), fold=t).save(pca_dir)
            if aug:   # pre/joint_pca.py:29-36: the plain labels, then the augmented ones
                u += [x for s in folds if s != folds[t] for x in labels_aug.get(s, [])]
                fit_labels(np.concatenate(u) if u else np.zeros((0, 63), np.float32), fold=t, aug=True).save(pca_dir)
    return totals
