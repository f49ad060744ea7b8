"""Batched on-device voxelization on torch tensors (thin host layer over the C ABI).

``voxelize`` is the batched form of the reference's ``cal_tsdf_cuda``
(pre/tsdf_numba.py:119-161): depth crops in, ``(tsdf, max_l, mid_p)`` out — the
triple ``3D_CNN/dataset.py:73-79`` hands to the network — but for n frames in one
fused HIP launch on the caller's stream, with the results left on the GPU.
torch is used for device memory and the stream handle only.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional

import torch

from . import _lib


class TsdfBatch(NamedTuple):
    tsdf: torch.Tensor    # float32[n,3,R,R,R]
    max_l: torch.Tensor   # float32[n]
    mid_p: torch.Tensor   # float32[n,3]
    status: torch.Tensor  # int32[n]  (_lib.TSDF_FRAME_*)


_get_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _raw_stream(dev) -> int:
    """hipStream_t of torch's current stream on ``dev`` as an integer (without building a torch Stream object: at
    batch 16 the host side of a call is longer than the kernel, tools/exp_latency_parts.py)."""
    if _get_raw_stream is not None:
        return _get_raw_stream(dev.index)
    return torch.cuda.current_stream(dev).cuda_stream


class _Current:
    """``with _current(dev):`` — makes ``dev`` the current device, at no cost when it already is."""

    __slots__ = ("guard",)

    def __init__(self, dev):
        self.guard = None if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)

    def __enter__(self):
        if self.guard is not None:
            self.guard.__enter__()

    def __exit__(self, *exc):
        if self.guard is not None:
            self.guard.__exit__(*exc)
        return False


def _dev_check(name, t, dtype, device=None, host_ok=False):
    """``host_ok``: the per-frame metadata (offsets, headers, gt) may also be PAGE-LOCKED host memory, which the
    GPU reads over the link (include/tsdf.h) — a pinned CPU tensor then passes; pageable memory never does."""
    if t.__class__ is torch.Tensor and t.is_cuda and t.dtype is dtype and t.is_contiguous() and \
            (device is None or t.device == device):
        return   # the common case, in one expression: this runs seven times per call
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if host_ok and not t.is_cuda and t.is_pinned():
        device = None
    elif not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU" + (" or in page-locked host memory" if host_ok else "") +
                         f" (there is no CPU path); got device {t.device}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device}")


def _pack(L, depth, offsets, headers, res=None, layout="czyx"):
    """The one validation of a packed-frame triple; returns (device, n, R) — R is None without ``res``."""
    if layout not in _lib.LAYOUTS:
        raise ValueError("layout must be 'czyx' or 'cxyz'")
    _dev_check("depth", depth, torch.float32)
    dev = depth.device
    _dev_check("offsets", offsets, torch.int64, dev, host_ok=True)
    _dev_check("headers", headers, torch.int32, dev, host_ok=True)
    if headers.dim() != 2 or headers.shape[1] != 6:
        raise ValueError("headers must have shape [n, 6]")
    n = headers.shape[0]
    if offsets.numel() != n + 1:
        raise ValueError("offsets must have n+1 entries")
    if res is None:
        return dev, n, None
    if not L.tsdf_resolution_supported(int(res)):
        raise ValueError(f"unsupported grid resolution {res} (multiple of 4 in 4..128)")
    return dev, n, int(res)


def _coords(name, t, rows) -> int:
    """``t`` holds ``rows`` frames of 3*J float32 coordinates, 1 <= J <= 170, as [rows, 3J] or [rows, J, 3] (any trailing
    shape with 3*J elements): returns 3*J — or 0 for ``rows == 0``, where there is nothing to count and the caller has
    its own default."""
    if t.shape[0] != rows:
        raise ValueError(f"{name} must have shape [{rows}, 3*J] or [{rows}, J, 3]")
    nc = t.numel() // rows if rows else 0
    if rows and (nc % 3 or not 1 <= nc // 3 <= 170):
        raise ValueError(f"{name} must hold 1..170 joints of 3 coordinates per frame")
    return nc


def _shaped(name, t, shape, dtype, dev):
    """A caller's tensor whose data pointer goes straight to the kernel: device, dtype, contiguity, shape.  A per-frame
    vector (``shape`` [n]) is checked by its element count only, as it always was: [n, 1] passes."""
    _dev_check(name, t, dtype, dev)
    if tuple(t.shape) != shape and (len(shape) != 1 or t.numel() != shape[0]):
        raise ValueError(f"{name} must have shape {shape}")
    return t


def _out(name, t, shape, dtype, dev):
    """An output: allocated when ``t`` is None, else the caller's, validated."""
    return torch.empty(shape, dtype=dtype, device=dev) if t is None else _shaped(name, t, shape, dtype, dev)


def empty_batch(n: int, R: int, dev) -> TsdfBatch:
    """Uninitialised outputs of n frames at resolution R on ``dev`` (what ``out=`` of the voxelizers takes)."""
    return TsdfBatch(_out("tsdf", None, (n, 3, R, R, R), torch.float32, dev), _out("max_l", None, (n,), torch.float32, dev),
                     _out("mid_p", None, (n, 3), torch.float32, dev), _out("status", None, (n,), torch.int32, dev))


def _make_out(out, n, R, dev) -> "TsdfBatch":
    """Allocate the outputs, or validate caller-supplied ones.  (The latter is every step of a loader that reuses its
    buffers: what _shaped would do per field is written out, four calls and one expression.)"""
    if out is None:
        return empty_batch(n, R, dev)
    _dev_check("out.tsdf", out.tsdf, torch.float32, dev)
    _dev_check("out.max_l", out.max_l, torch.float32, dev)
    _dev_check("out.mid_p", out.mid_p, torch.float32, dev)
    _dev_check("out.status", out.status, torch.int32, dev)
    if tuple(out.tsdf.shape) != (n, 3, R, R, R) or out.max_l.numel() != n or \
            tuple(out.mid_p.shape) != (n, 3) or out.status.numel() != n:
        raise ValueError("out tensors have the wrong shape")
    return out


def _each(out, fields, dev) -> list:
    """Every output of the table ``fields`` of (name, shape, dtype): ``out``'s, validated, or allocated where it has none."""
    return [_out("out." + name, getattr(out, name, None), shape, dtype, dev) for name, shape, dtype in fields]


def _outs(cls, out, fields, dev):
    """An entry's outputs as the NamedTuple ``cls``: allocated from their table, or the caller's ``out``, every field validated."""
    if out is None:
        return cls(*[_out(name, None, shape, dtype, dev) for name, shape, dtype in fields])
    for name, shape, dtype in fields:
        _shaped("out." + name, getattr(out, name), shape, dtype, dev)
    return out


def _cam(cam):
    return ctypes.byref(cam) if cam is not None else None


def _cam5(cam) -> list:
    """The five camera constants by value, for the entries that take them so (``cam`` None: the MSRA defaults)."""
    c = cam if cam is not None else _lib.default_cam()
    return [c.focal, c.cx, c.cy, c.invalid_eps, c.trunc_voxels]


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _head(depth, offsets, headers, n, R, cam, layout) -> list:
    """The nine arguments every packed-frame entry starts with; the stream (position 8) is filled in by _call."""
    return [depth.data_ptr(), depth.numel(), offsets.data_ptr(), headers.data_ptr(), n, R, _cam(cam), _lib.LAYOUTS[layout],
            None]


def _call(dev, fn, args: list, stream_at: int) -> None:
    """The one place an entry is called: ``dev`` is made current, ``args[stream_at]`` becomes the raw handle of ITS current
    stream (read while it is current), and a failure is reported under the name of the entry that failed."""
    with _Current(dev):
        args[stream_at] = _raw_stream(dev)
        rc = fn(*args)
    _lib.check(rc, fn.__name__)


def _labels_struct(gt, n_src, n, dev, clamp, out_gt_nor=None, out_gt=None, want_gt=False):
    """Validate the label tensors and build the ``tsdf_labels`` struct (kept alive by the caller): ``gt`` holds the labels
    of ``n_src`` frames, the outputs those of the ``n`` frames of the batch (the same frames unless the entry is indexed).
    Returns (struct, gt_nor, gt written by the launch or None)."""
    _dev_check("gt", gt, torch.float32, dev, host_ok=True)
    nc = _coords("gt", gt, n_src) or 63
    shape = (n,) + tuple(gt.shape[1:])
    gt_nor = _out("out_gt_nor", out_gt_nor, shape, torch.float32, dev)
    gt_dev = _out("out_gt", out_gt, shape, torch.float32, dev) if want_gt or out_gt is not None else None
    return _lib.TsdfLabels(gt.data_ptr(), nc // 3, 1 if clamp else 0, gt_nor.data_ptr(), _ptr(gt_dev)), gt_nor, gt_dev


def voxelize(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, res: int = 32,
             layout: str = "czyx", cam: Optional[_lib.TsdfCam] = None,
             out: Optional[TsdfBatch] = None) -> TsdfBatch:
    """Voxelize n packed depth crops on the GPU.

    depth   float32[sum N_i]  crops packed back to back (payload of the MSRA .bin files)
    offsets int64[n+1]        element offsets of each crop in ``depth``
    headers int32[n,6]        W, H, left, top, right, bottom per frame
    res     grid resolution R (reference: 32)
    layout  "czyx" (numba kernel layout, default) or "cxyz" (CPU-loop layout)
    out     optional preallocated TsdfBatch to write into (no allocation, graph-capturable)

    Enqueues on ``torch.cuda.current_stream()`` and returns without synchronising.
    """
    L = _lib.load()
    dev, n, R = _pack(L, depth, offsets, headers, res, layout)
    out = _make_out(out, n, R, dev)
    if n:
        _call(dev, L.tsdf_voxelize_hip, _head(depth, offsets, headers, n, R, cam, layout) +
              [out.tsdf.data_ptr(), out.max_l.data_ptr(), out.mid_p.data_ptr(), out.status.data_ptr()], 8)
    return out


def voxelize_labels(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, gt: torch.Tensor,
                    res: int = 32, layout: str = "czyx", cam: Optional[_lib.TsdfCam] = None, clamp: bool = True,
                    out: Optional[TsdfBatch] = None, out_gt_nor: Optional[torch.Tensor] = None,
                    gt_copy: bool = False, pca=None, k: Optional[int] = None):
    """:func:`voxelize` plus the label normalisation of the same launch: ``(gt - mid_p) / max_l + 0.5`` per
    joint coordinate (pre/joint_nor.py:8-18), clamped to [0,1] as 3D_CNN/train.py:241-242 does (``clamp``).
    gt float32[n,63] (or [n,J,3]) on the GPU.  Returns ``(TsdfBatch, gt_nor)``; frames whose status is not 0
    get 0.5 everywhere.

    ``offsets``, ``headers`` and ``gt`` may be pinned CPU tensors (read by the kernel over the link; they must not
    change before the launch has finished); ``gt_copy=True`` then also returns the joints as a device tensor,
    written by the same launch: ``(TsdfBatch, gt_nor, gt_on_device)``.

    ``pca`` (a :class:`pca.JointPCA`) and ``k`` (default: every component it holds) add the joint-PCA projection of the
    unclamped labels to the same launch (``tsdf_voxelize_labels_pca_hip``): ``gt_pca`` float32[n, k] is appended to the
    returned tuple."""
    L = _lib.load()
    dev, n, R = _pack(L, depth, offsets, headers, res, layout)
    out = _make_out(out, n, R, dev)
    lab, gt_nor, gt_dev = _labels_struct(gt, n, n, dev, clamp, out_gt_nor, want_gt=gt_copy)
    pst = gt_pca = None
    if pca is not None:
        pst, gt_pca = _pca_struct(pca, k, n, lab.n_joints, dev)
    if n:
        head = _head(depth, offsets, headers, n, R, cam, layout)
        tail = [out.tsdf.data_ptr(), out.max_l.data_ptr(), out.mid_p.data_ptr(), out.status.data_ptr(), ctypes.byref(lab)]
        if pst is None:
            _call(dev, L.tsdf_voxelize_labels_hip, head + tail, 8)
        else:
            _call(dev, L.tsdf_voxelize_labels_pca_hip, head + [None] + tail + [ctypes.byref(pst)], 8)
    return ((out, gt_nor, gt_dev) if gt_copy else (out, gt_nor)) + ((gt_pca,) if pca is not None else ())


def voxelize_indexed(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, index: torch.Tensor,
                     gt: Optional[torch.Tensor] = None, res: int = 32, layout: str = "czyx",
                     cam: Optional[_lib.TsdfCam] = None, clamp: bool = True, out: Optional[TsdfBatch] = None,
                     gt_copy: bool = False, xforms: Optional[torch.Tensor] = None,
                     out_gt_nor: Optional[torch.Tensor] = None, out_gt: Optional[torch.Tensor] = None,
                     pca=None, k: Optional[int] = None):
    """A batch drawn by index from a pack that lives on the GPU (``tsdf_voxelize_indexed_hip``): ``depth`` /
    ``offsets[N+1]`` / ``headers[N,6]`` (and ``gt[N,3J]``) describe the whole pack, uploaded once; frame i of the batch is
    pack frame ``index[i]`` (int64[n], any order — a shuffled minibatch; device or pinned host memory; or, for
    n <= 32 without ``xforms``, an ordinary CPU tensor, which is read during the call and travels to the GPU inside the
    kernel arguments: ``tsdf_voxelize_indexed_host_hip``).  Outputs are in batch order.  Bit-identical to :func:`voxelize_labels` on the gathered frames.  Returns ``TsdfBatch`` without ``gt``,
    else ``(TsdfBatch, gt_nor)`` or, with ``gt_copy=True``, ``(TsdfBatch, gt_nor, gt_of_the_batch)``.
    ``xforms`` float64[n,24] on the GPU (one map per batch position, as for :func:`voxelize_aug`) adds the fused 3-D
    augmentation: the labels are then mapped with it, ``gt_of_the_batch`` is ``T(joints)``.
    ``out`` / ``out_gt_nor`` / ``out_gt`` (the latter implies ``gt_copy``): preallocated outputs of exactly the batch's
    shapes — a loader's ring buffers; nothing is allocated then.
    ``pca`` / ``k`` (needs ``gt``): the joint-PCA projection of the batch's unclamped labels by the same launch
    (``tsdf_voxelize_indexed_pca_hip`` / ``tsdf_voxelize_indexed_host_pca_hip``); ``gt_pca`` float32[n, k] is appended to
    the returned tuple."""
    L = _lib.load()
    by_value = isinstance(index, torch.Tensor) and not index.is_cuda and not index.is_pinned() and \
        index.dtype is torch.int64 and index.dim() == 1 and index.is_contiguous() and \
        index.numel() <= _lib.INLINE_INDEX_MAX and xforms is None
    if not by_value:   # (a small index in ordinary host memory travels inside the kernel arguments instead)
        _dev_check("index", index, torch.int64, depth.device if isinstance(depth, torch.Tensor) else None, host_ok=True)
    if index.dim() != 1:
        raise ValueError("index must have shape [n]")
    dev, n_pack, R = _pack(L, depth, offsets, headers, res, layout)
    n = index.numel()
    out = _make_out(out, n, R, dev)
    lab = gt_nor = gt_dev = None
    if xforms is not None:
        _dev_check("xforms", xforms, torch.float64, dev, host_ok=True)   # (page-locked host memory: read over the link)
        if xforms.numel() != 24 * n:
            raise ValueError("xforms must have shape [n, 24] (forward rows then inverse rows)")
    if gt is not None:
        _dev_check("gt", gt, torch.float32, dev, host_ok=True)
        # (the labels of a PACK are at least 2-D even when the pack is empty; every other site takes what _coords takes)
        if gt.dim() < 2:
            raise ValueError("gt must hold the labels of every frame of the pack: [N, 3*J] or [N, J, 3]")
        lab, gt_nor, gt_dev = _labels_struct(gt, n_pack, n, dev, clamp, out_gt_nor, out_gt, want_gt=gt_copy)
        gt_copy = gt_dev is not None
    pst = gt_pca = None
    if pca is not None:
        if gt is None:
            raise ValueError("pca= needs gt (the projection is of the batch's labels)")
        pst, gt_pca = _pca_struct(pca, k, n, lab.n_joints, dev)
    if n:
        head = _head(depth, offsets, headers, n, R, cam, layout)
        head[4:5] = [n_pack, index.data_ptr(), n]   # the indexed entries' prefix: the stream is at position 10
        tail = [out.tsdf.data_ptr(), out.max_l.data_ptr(), out.mid_p.data_ptr(), out.status.data_ptr(),
                ctypes.byref(lab) if lab is not None else None]
        if pst is not None:
            if by_value:
                _call(dev, L.tsdf_voxelize_indexed_host_pca_hip, head + tail + [ctypes.byref(pst)], 10)
            else:
                _call(dev, L.tsdf_voxelize_indexed_pca_hip, head + [_ptr(xforms)] + tail + [ctypes.byref(pst)], 10)
        elif by_value:
            _call(dev, L.tsdf_voxelize_indexed_host_hip, head + tail, 10)
        elif xforms is None:
            _call(dev, L.tsdf_voxelize_indexed_hip, head + tail, 10)
        else:
            _call(dev, L.tsdf_voxelize_indexed_aug_hip, head + [xforms.data_ptr()] + tail, 10)
    if gt is None:
        return out
    return ((out, gt_nor, gt_dev) if gt_copy else (out, gt_nor)) + ((gt_pca,) if pca is not None else ())


def _pca_struct(pca, k, n, n_joints, dev, out=None):
    """The ``tsdf_pca`` struct for ``pca`` (a :class:`pca.JointPCA`) with ``k`` components on ``dev``, and its output
    tensor float32[n, k] (kept alive by the caller)."""
    k = pca.check_k(k)
    if pca.n_coords != 3 * n_joints:
        raise ValueError(f"the PCA basis is for {pca.n_coords} coordinates, the labels have {3 * n_joints}")
    mean, coeff = pca.device_tensors(dev)
    out = _out("out", out, (n, k), torch.float32, dev)
    return _lib.TsdfPca(mean.data_ptr(), coeff.data_ptr(), k, out.data_ptr()), out


def _frames(name, x, max_l, mid_p):
    """``x`` float32[n, ...] on the GPU with the placement of its n frames: returns (device, n)."""
    _dev_check(name, x, torch.float32)
    dev, n = x.device, x.shape[0]
    _dev_check("max_l", max_l, torch.float32, dev)
    _dev_check("mid_p", mid_p, torch.float32, dev)
    if max_l.numel() != n or tuple(mid_p.shape) != (n, 3):
        raise ValueError("max_l must be [n] and mid_p [n,3]")
    return dev, n


def project_joints(gt: torch.Tensor, max_l: torch.Tensor, mid_p: torch.Tensor, pca, k: Optional[int] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Joint-PCA coefficients of world joints already on the GPU (``tsdf_project_joints_hip``): the labels are normalised
    with ``max_l`` / ``mid_p`` (no clamp; ``max_l == 0`` gives 0.5) and projected on the first ``k`` components of
    ``pca`` — bit-identical to the ``gt_pca`` the fused voxelizer entries write.  gt [n, 3J] or [n, J, 3] -> [n, k]."""
    L = _lib.load()
    dev, n = _frames("gt", gt, max_l, mid_p)
    nc = _coords("gt", gt, n) or pca.n_coords
    pst, out = _pca_struct(pca, k, n, nc // 3, dev, out)
    if n:
        _call(dev, L.tsdf_project_joints_hip, [gt.data_ptr(), max_l.data_ptr(), mid_p.data_ptr(), n, nc // 3,
                                               ctypes.byref(pst), None], 6)
    return out


class PoseError(NamedTuple):
    err: torch.Tensor                 # float32[n, J]  per-joint Euclidean error, mm
    frame_mean: torch.Tensor          # float32[n]     mean over the frame's joints
    frame_max: torch.Tensor           # float32[n]     worst joint of the frame
    joints: Optional[torch.Tensor]    # float32[n, 3J] the decoded prediction in mm (``joints=True``), else None


def pose_error(pred: torch.Tensor, gt: torch.Tensor, max_l: torch.Tensor, mid_p: torch.Tensor, pca=None,
               joints: bool = False) -> PoseError:
    """The per-batch evaluation of 3D_CNN/train.py (decode, denormalise, per-joint error: :219-227,325-333 and
    ``cal_out`` :410-427) in ONE launch (``tsdf_pose_error_hip``), without a host sync.

    pred   float32[n, K] PCA coefficients (``pca`` given: decoded as mu + p W[:, :K]^T) or float32[n, 3J] normalised
           coordinates (``pca=None``: the small mode's network output)
    gt     float32[n, 3J] (or [n, J, 3]) world joints in mm; max_l [n], mid_p [n, 3] of the frames' grids
    Returns :class:`PoseError`; :func:`joints_within` / :func:`frames_within` turn ``err`` into the usual scores."""
    L = _lib.load()
    _dev_check("pred", pred, torch.float32)
    dev = pred.device
    n = pred.shape[0]
    _dev_check("gt", gt, torch.float32, dev)
    _dev_check("max_l", max_l, torch.float32, dev)
    _dev_check("mid_p", mid_p, torch.float32, dev)
    if gt.shape[0] != n or max_l.numel() != n or tuple(mid_p.shape) != (n, 3):
        raise ValueError("pred, gt, max_l [n] and mid_p [n,3] must describe the same n frames")
    nc = _coords("gt", gt, n) or (pca.n_coords if pca is not None else 63)
    nj = nc // 3
    pst = None
    if pca is not None:
        if pred.dim() != 2:
            raise ValueError("pred must be [n, K] PCA coefficients")
        k = pca.check_k(pred.shape[1])
        if pca.n_coords != nc:
            raise ValueError(f"the PCA basis is for {pca.n_coords} coordinates, gt has {nc}")
        mean, coeff = pca.device_tensors(dev)
        pst = _lib.TsdfPca(mean.data_ptr(), coeff.data_ptr(), k, None)
    elif pred.numel() != n * nc:
        raise ValueError("pred must hold 3*J normalised coordinates per frame (or pass pca=)")
    res = PoseError(_out("err", None, (n, nj), torch.float32, dev), _out("frame_mean", None, (n,), torch.float32, dev),
                    _out("frame_max", None, (n,), torch.float32, dev),
                    _out("joints", None, (n, nc), torch.float32, dev) if joints else None)
    if n:
        _call(dev, L.tsdf_pose_error_hip,
              [pred.data_ptr(), ctypes.byref(pst) if pst is not None else None, max_l.data_ptr(), mid_p.data_ptr(),
               gt.data_ptr(), n, nj, None, res.err.data_ptr(), res.frame_mean.data_ptr(), res.frame_max.data_ptr(),
               _ptr(res.joints)], 7)
    return res


def joints_within(err: torch.Tensor, mm: float = 20.0) -> torch.Tensor:
    """The reference's "proportion" (``cal_out``, 3D_CNN/train.py:417-420): percent of joints whose error is below
    ``mm`` (strictly, as ``sqrt_sum < t``).  A 0-d float32 tensor on err's device (no host sync)."""
    return (err < mm).sum().to(torch.float32) / err.numel() * 100


def frames_within(err: torch.Tensor, mm: float) -> torch.Tensor:
    """Fraction of frames whose WORST joint is within ``mm`` (error <= mm) — the usual MSRA success curve.  ``err``
    float32[n, J] (``PoseError.err``); a 0-d float32 tensor."""
    return (err.amax(dim=1) <= mm).to(torch.float32).mean()


def normalize_joints(gt: torch.Tensor, max_l: torch.Tensor, mid_p: torch.Tensor, clamp: bool = True,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Labels into the voxel cube's [0,1] frame on their own (``tsdf_normalize_joints_hip``):
    ``(gt - mid_p) / max_l + 0.5`` (pre/joint_nor.py:8-18), clamped as 3D_CNN/train.py:241-242 unless
    ``clamp=False``; frames with ``max_l == 0`` give 0.5.  gt [n,63] or [n,21,3]; result has gt's shape."""
    return _norm_call(gt, max_l, mid_p, clamp, False, out)


def denormalize_joints(pred: torch.Tensor, max_l: torch.Tensor, mid_p: torch.Tensor,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Inverse of :func:`normalize_joints` for network outputs: ``(pred - 0.5) * max_l + mid_p``
    (3D_CNN/train.py:263-266)."""
    return _norm_call(pred, max_l, mid_p, False, True, out)


def _norm_call(x, max_l, mid_p, clamp, inverse, out):
    L = _lib.load()
    dev, n = _frames("joints", x, max_l, mid_p)
    nc = _coords("joints", x, n) or 63
    out = _out("out", out, tuple(x.shape), torch.float32, dev)
    if n:
        args = [x.data_ptr(), max_l.data_ptr(), mid_p.data_ptr(), n, nc // 3]
        if inverse:
            _call(dev, L.tsdf_denormalize_joints_hip, args + [None, out.data_ptr()], 5)
        else:
            _call(dev, L.tsdf_normalize_joints_hip, args + [1 if clamp else 0, None, out.data_ptr()], 6)
    return out


def release_stream(stream=None) -> None:
    """Tell the library that ``stream`` (default: the current one) is going away (``tsdf_stream_release``).  The
    stream is synchronised first: its work-queue word and mailboxes must not be handed to another stream while one of
    its launches is still running (include/tsdf.h, "stream ownership")."""
    L = _lib.load()
    s = stream if stream is not None else torch.cuda.current_stream()
    s.synchronize()
    L.tsdf_stream_release(s.cuda_stream)


def voxel_pixels(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, res: int = 32,
                 layout: str = "czyx", grid: Optional[torch.Tensor] = None, cam: Optional[_lib.TsdfCam] = None):
    """Diagnostic (``tsdf_debug_pixmap_hip``, include/tsdf_debug.h): the voxelizer together with the pixel every voxel
    gathers.  Runs in the DEBUG build of the library (``_lib.load_debug()``: the product does not carry the hook).
    Returns ``(tsdf, pixmap int32[n,R,R,R] indexed [z,y,x], status)``; pixmap values as in include/tsdf_debug.h."""
    L = _lib.load_debug()
    dev, n, R = _pack(L, depth, offsets, headers, res, layout)
    if grid is not None:
        _shaped("grid", grid, (n, 8), torch.float32, dev)
    tsdf = _out("tsdf", None, (n, 3, R, R, R), torch.float32, dev)
    pm = _out("pixmap", None, (n, R, R, R), torch.int32, dev)
    st = _out("status", None, (n,), torch.int32, dev)
    if n:
        _call(dev, L.tsdf_debug_pixmap_hip, _head(depth, offsets, headers, n, R, cam, layout) +
              [_ptr(grid), tsdf.data_ptr(), pm.data_ptr(), st.data_ptr()], 8)
    return tsdf, pm, st


class AabbBatch(NamedTuple):
    aabb: torch.Tensor    # float32[n,6] min xyz, max xyz
    grid: torch.Tensor    # float32[n,8] mid_p[3], max_l, voxel_len, trunc_dis, 0, 0
    ori: torch.Tensor     # float32[n,3] vox_ori
    status: torch.Tensor  # int32[n]


def aabb(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, res: int = 32,
         cam: Optional[_lib.TsdfCam] = None) -> AabbBatch:
    """Phase 1 + glue only: min_max_kernel + host numpy of pre/tsdf_numba.py:75-116,135-147."""
    L = _lib.load()
    dev, n, R = _pack(L, depth, offsets, headers, res)
    out = _outs(AabbBatch, None, (("aabb", (n, 6), torch.float32), ("grid", (n, 8), torch.float32),
                                  ("ori", (n, 3), torch.float32), ("status", (n,), torch.int32)), dev)
    if n:
        _call(dev, L.tsdf_aabb_hip, [depth.data_ptr(), depth.numel(), offsets.data_ptr(), headers.data_ptr(), n, R, _cam(cam),
                                     None, out.aabb.data_ptr(), out.grid.data_ptr(), out.ori.data_ptr(),
                                     out.status.data_ptr()], 7)
    return out


def voxelize_grid(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, grid: torch.Tensor,
                  res: int = 32, layout: str = "czyx", cam: Optional[_lib.TsdfCam] = None):
    """Phase 2 with caller-supplied grid placement: the batched form of the reference's
    ``tsdf_cal(data, vox_ori, voxel_len, truncation)`` (pre/tsdf_for.py:44-122).

    grid  float32[n,8] on the GPU: vox_ori[3], voxel_len, trunc_dis, 3 pad words per frame.
    Returns (tsdf float32[n,3,R,R,R], status int32[n]).
    """
    L = _lib.load()
    dev, n, R = _pack(L, depth, offsets, headers, res, layout)
    _shaped("grid", grid, (n, 8), torch.float32, dev)
    tsdf = _out("tsdf", None, (n, 3, R, R, R), torch.float32, dev)
    st = _out("status", None, (n,), torch.int32, dev)
    if n:
        _call(dev, L.tsdf_voxelize_grid_hip, _head(depth, offsets, headers, n, R, cam, layout) +
              [grid.data_ptr(), tsdf.data_ptr(), st.data_ptr()], 8)
    return tsdf, st


def voxelize_aug(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, xforms: torch.Tensor,
                 res: int = 64, layout: str = "czyx", cam: Optional[_lib.TsdfCam] = None,
                 out: Optional[TsdfBatch] = None, gt: Optional[torch.Tensor] = None, clamp: bool = True):
    """Voxelization with a per-frame 3-D affine augmentation fused into the kernel
    (BASELINE.json configs[4]; see ``tsdf_voxelize_aug_hip`` in include/tsdf.h for the contract).

    xforms  float64[n,24] on the GPU: forward map rows {A_i0,A_i1,A_i2,b_i} then the inverse map
            (``augment.random_affines`` / ``augment.pack_affine`` build them).
    gt      optional float32[n,63] labels: they are mapped with the frame's forward map and normalised in the
            augmented grid by the same launch (``tsdf_voxelize_aug_labels_hip``).
    Returns the same TsdfBatch as :func:`voxelize` (``max_l`` / ``mid_p`` in the mapped frame), or
    ``(TsdfBatch, gt_nor, gt_aug)`` when ``gt`` is given.
    """
    L = _lib.load()
    dev, n, R = _pack(L, depth, offsets, headers, res, layout)
    _shaped("xforms", xforms, (n, 24), torch.float64, dev)
    out = _make_out(out, n, R, dev)
    lab = gt_nor = gt_aug = None
    if gt is not None:
        lab, gt_nor, gt_aug = _labels_struct(gt, n, n, dev, clamp, want_gt=True)
    if n:
        args = _head(depth, offsets, headers, n, R, cam, layout) + \
            [xforms.data_ptr(), out.tsdf.data_ptr(), out.max_l.data_ptr(), out.mid_p.data_ptr(), out.status.data_ptr()]
        if lab is None:
            _call(dev, L.tsdf_voxelize_aug_hip, args, 8)
        else:
            _call(dev, L.tsdf_voxelize_aug_labels_hip, args + [ctypes.byref(lab)], 8)
    return out if gt is None else (out, gt_nor, gt_aug)


_NO_STATE = object()


def _draw_args(centres, n, index, counters, out, params, state=_NO_STATE):
    """The one validation of :func:`aug_xforms` and :func:`aug_xforms_at` (``state``, ``counters``: the latter's only):
    returns ``(device, n_src, n, xforms, stretch, rot)`` — the outputs allocated, or ``out`` validated; ``stretch`` and
    ``rot`` are None without ``params``."""
    _dev_check("centres", centres, torch.float32)
    dev = centres.device
    if centres.dim() != 2 or centres.shape[1] != 3:
        raise ValueError("centres must have shape [N, 3]")
    n_src = centres.shape[0]
    if state is not _NO_STATE:
        _dev_check("state", state, torch.int64, dev)
        if state.numel() != 2:
            raise ValueError("state must hold 2 elements: {key, counter0}")
    for name, t in (("index", index), ("counters", counters)):
        if t is None:
            continue
        _dev_check(name, t, torch.int64, dev, host_ok=True)
        if t.dim() != 1:
            raise ValueError(f"{name} must have shape [n]")
        if n is not None and int(n) != t.numel():
            raise ValueError(f"n must be the length of {name}" if t is index else "counters must have n entries")
        n = t.numel()
    n = n_src if n is None else int(n)
    if n < 0:
        raise ValueError("n must be >= 0")
    if n and n_src < 1:
        raise ValueError("centres holds no frame")
    xf = _out("out", out, (n, 24), torch.float64, dev)
    stretch = _out("stretch", None, (n,), torch.float64, dev) if params else None
    rot = _out("rot", None, (n, 2), torch.int32, dev) if params else None
    return dev, n_src, n, xf, stretch, rot


def aug_xforms(centres: torch.Tensor, n: Optional[int] = None, index: Optional[torch.Tensor] = None, key: int = 0,
               counter0: int = 0, out: Optional[torch.Tensor] = None, want_params: bool = False):
    """The maps of a batch of fused augmentations, drawn on the GPU (``tsdf_aug_draw_hip`` of libtsdf_augment.so, one small
    launch on the current stream; include/tsdf_augment.h has the contract).

    centres   float32[N,3] on the GPU: every frame's un-augmented grid centre (``aabb(...).grid[:, :3]`` / ``mid_p``)
    index     int64[n] (device or page-locked host memory): batch position i turns about ``centres[index[i]]``; without
              it position i uses frame i and ``n`` defaults to N
    key, counter0   position i draws from ``(key, counter0 + i)`` alone (integers mod 2^64;
              ``augment.device_draws_np(key, counter0 + arange(n))`` restates the draws, ``augment.device_key`` makes a key)
    out       optional float64[n,24] to write into (it is returned)
    Returns ``xforms`` float64[n,24] — what :func:`voxelize_aug` / :func:`voxelize_indexed` take —, or with ``want_params``
    ``(xforms, stretch float64[n], rot int32[n,2])``, rot = (rot_xy, rot_z) in degrees.  A position whose index is outside
    [0, N) gets the identity map and a NaN stretch."""
    A = _lib.load_augment()
    dev, n_src, n, xf, stretch, rot = _draw_args(centres, n, index, None, out, want_params)
    if n:
        m64 = (1 << 64) - 1
        _call(dev, A.tsdf_aug_draw_hip, [centres.data_ptr(), n_src, _ptr(index), n, int(key) & m64, int(counter0) & m64, None,
                                         xf.data_ptr(), _ptr(stretch), _ptr(rot)], 6)
    return (xf, stretch, rot) if want_params else xf


def _i64(v: int) -> int:
    """An integer mod 2^64 as the int64 with the same bits (torch has no arithmetic on uint64 tensors)."""
    v = int(v) & ((1 << 64) - 1)
    return v - (1 << 64) if v >> 63 else v


def aug_state(key: int, counter0: int = 0, device=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``{key, counter0}`` (integers mod 2^64) as the int64[2] tensor :func:`aug_xforms_at` reads on the device — a new one
    on ``device``, or written into ``out`` by a copy on the current stream (the launches queued before it on that stream
    still see the old state, those after it the new one)."""
    h = torch.tensor([_i64(key), _i64(counter0)], dtype=torch.int64)
    if out is None:
        return h.to(device)
    if out.dtype is not torch.int64 or out.numel() != 2:
        raise ValueError("state must be an int64 tensor of 2 elements")
    out.view(-1).copy_(h)
    return out


def aug_xforms_at(centres: torch.Tensor, state: torch.Tensor, n: Optional[int] = None,
                  index: Optional[torch.Tensor] = None, counters: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, return_params: bool = False):
    """:func:`aug_xforms` with the key and the counters read ON THE DEVICE (``tsdf_aug_draw_at_hip`` of libtsdf_augstep.so,
    one small launch on the current stream; include/tsdf_augstep.h has the contract): the same draws and maps for the same
    ``(key, counter)``, centre and index, bit for bit.

    centres   float32[N,3] on the GPU, as for :func:`aug_xforms`
    state     int64[2] on the GPU: ``{key, counter0}`` as 64-bit patterns (:func:`aug_state` makes one).  The KERNEL reads
              it: whatever was written to it earlier on the same stream is what the launch uses, so a launch captured into
              a graph draws anew at every replay whose state was rewritten before it (:class:`AugmentedStep`)
    index     int64[n] (device or page-locked host memory) or None, as for :func:`aug_xforms`
    counters  int64[n] (device or page-locked host memory) or None: position i draws from
              ``(key, counter0 + counters[i])`` mod 2^64 (negative values wrap) instead of ``(key, counter0 + i)`` — a batch
              of arbitrary frames, each with a draw of its own, in one launch
              (``augment.device_draws_np(key, counter0 + counters)`` restates the draws)
    out       optional float64[n,24] to write into (it is returned)
    ``n`` defaults to the length of ``index``, else of ``counters``, else N.  Returns ``xforms`` float64[n,24], or with
    ``return_params`` ``(xforms, stretch float64[n], rot int32[n,2])``.  A position whose index is outside [0, N) gets the
    identity map and a NaN stretch."""
    A = _lib.load_augstep()
    dev, n_src, n, xf, stretch, rot = _draw_args(centres, n, index, counters, out, return_params, state)
    if n:
        _call(dev, A.tsdf_aug_draw_at_hip, [centres.data_ptr(), n_src, _ptr(index), n, state.data_ptr(), _ptr(counters), None,
                                            xf.data_ptr(), _ptr(stretch), _ptr(rot)], 6)
    return (xf, stretch, rot) if return_params else xf


class AugmentedStep:
    """The augmented training step — :func:`aug_xforms_at` then :func:`voxelize_indexed` ``(..., xforms=...)`` — over static
    buffers, captured ONCE into a graph and replayed: a step's host side is one small copy (the batch's frame numbers and
    ``{key, counter0}``) and one graph launch instead of two C calls with their argument marshalling.

    One object serves one configuration: the resident pack ``depth`` / ``offsets`` / ``headers`` (``gt``: with labels), a
    batch of exactly ``n`` frames, ``res``, ``layout``, ``clamp``.  ``centres`` float32[N,3] are the frames' un-augmented grid
    centres (default: one :func:`aabb` launch over the pack).  It owns an int64[n] index, the int64[2] state, float64[n,24]
    maps and ONE set of outputs; ``step`` returns those outputs, so a step's results are valid until the next ``step``
    (queued on the same stream, the next step cannot overtake their readers; clone what you keep).

    The graph is the linear sequence of the two kernels on one stream: no branches, no copies inside, and the voxelizer
    takes the queue form it always takes under stream capture.  The draw kernel reads the state from device memory, which
    is what lets a replay draw anew.  ``graph=False`` issues the same two calls eagerly on the same buffers.

    ``dtype`` (torch.float16 / torch.bfloat16): the volume is written in that type.  The step is then
    :func:`aug_xforms_at`, :func:`map_grids`, :func:`voxelize_map_grid_lowp` and, with labels (``gt`` on the GPU), a gather of
    the batch's joints, :func:`transform_joints` and :func:`normalize_joints` — still one linear graph on one stream over
    static buffers, nothing allocated or copied inside; ``max_l`` / ``mid_p`` / ``status`` and the labels are those of the
    float32 step bit for bit.

    ``base`` float64[N,24] on the GPU, one map per pack frame (``obb_xforms(...).xforms``): position i is voxelized under
    ``draw_i o base[index[i]]`` — the augmentation about the frame's pose in ITS BASE FRAME, e.g. its principal axes.  The
    default ``centres`` are then the base-frame grid centres, ``map_grids(depth, offsets, headers, base).mid_p`` (one launch
    over the pack).  With ``base`` the step starts with :func:`map_step_head`: without ``dtype`` its maps alone
    (``place=False``) and then :func:`voxelize_indexed`; with ``dtype`` the whole head — maps, placement and labels in one
    launch — and then :func:`voxelize_map_grid_lowp`, two launches in all.  ``step`` leaves the composed maps in
    ``self.xforms``.  ``fused_head=True`` takes that two-launch form without a ``base`` as well; its results are those of
    the default step bit for bit.  The defaults ``base=None, fused_head=False`` issue exactly the launches listed above.

    ``tsdf="accurate"``: the volume is the accurate directional TSDF.  The step is the draw (:func:`aug_xforms_at`) and
    :func:`map_grids` — or, with ``base`` / ``fused_head``, the whole head in one launch —, then
    :func:`voxelize_map_grid_accurate` into a static float32 buffer, with ``dtype`` :func:`narrow_volumes` into the 2-byte
    volume, and without the head the labels as in the ``dtype`` step (``gt`` on the GPU, covering the pack).  One linear
    graph on one stream over static buffers again; ``max_l`` / ``mid_p`` / ``status``, ``xforms`` and the labels are the
    projective step's bit for bit.

    ``heatmap=(res, sigma)`` or ``(res, sigma, dtype)`` (needs ``gt``): the step also writes the voxel-to-voxel target, one
    Gaussian volume per joint, into ONE static buffer ``self.heat`` ``[n, J, res, res, res]`` (float32 unless ``dtype`` says
    otherwise; ``res`` is the heatmap's own resolution, in the step's ``layout``).  It is one more launch at the end of the
    same linear sequence — :func:`joint_heatmaps` of the step's ``gt_nor`` and ``status`` — and combines with every option
    above.  ``step`` returns exactly what it returns without it; ``heatmap=None`` issues exactly the launches listed above.

    ``occupancy=(res,)`` or ``(res, dtype)``: the step also writes the input of a voxel-to-voxel network, the one-channel
    occupancy volume of the batch under the step's maps, into ONE static buffer ``self.occ`` ``[n, 1, res, res, res]``
    (float32 unless ``dtype`` says otherwise; ``res`` is the occupancy's own resolution, in the step's ``layout``).  It is
    one more launch at the very end of the same linear sequence — :func:`occupancy_volumes` of the step's own ``index``,
    ``xforms``, ``out.max_l`` and ``out.mid_p`` — needs no ``gt`` and combines with every option above.  ``step`` returns
    exactly what it returns without it; ``occupancy=None`` issues exactly the launches listed above.

    ``fps=(M,)``: the step also writes the input of a point network, ``M`` farthest-point samples of each frame's cloud
    under the step's maps, into static buffers ``self.cloud`` float32[n, M, 3], ``self.cloud_pixel`` int32[n, M],
    ``self.cloud_count`` and ``self.cloud_status`` int32[n].  It is one more launch at the very end of the same linear
    sequence — :func:`farthest_points` of the step's own ``index`` and ``xforms``, in the resident form (a frame of more
    than ``FPS_RESIDENT_POINTS`` candidates gets status 3) — needs no ``gt`` and combines with every option above.
    ``step`` returns exactly what it returns without it; ``fps=None`` issues exactly the launches listed above.

    ``groups=((C, K), ...)`` and ``normals=k`` (both need ``fps=(M,)``): the step also writes what a point network reads
    next to the sampled cloud.  ``normals=k`` is one more launch after the sampling — :func:`point_normals` of
    ``self.cloud`` over ``k`` neighbours, the viewpoint the camera centre under the step's maps (one small copy takes it
    out of ``self.xforms``) — into the static :class:`NormalBatch` ``self.normals``.  ``groups`` is one launch per
    set-abstraction level after that — :func:`knn_groups` with ``offsets`` — into the static :class:`KnnBatch` es
    ``self.groups[l]``: level 0 groups the ``M`` sampled rows around their first ``C_0``, level ``l`` the first
    ``C_{l-1}`` rows around their first ``C_l``.  Positions the sampling gave a status are not read.  ``step`` returns
    exactly what it returns without them; without the two arguments the step issues exactly the launches listed above.

    ``fields=(K, radius)`` or ``(K, radius, dtype)`` (needs ``fps=(M,)`` and ``gt``): the step also writes the labels of a
    point-to-point regression network, per sampled point and joint a heat and a unit vector towards the joint, into ONE
    static buffer ``self.field`` ``[n, 4J, M]`` (layout "cp"; float32 unless ``dtype`` says otherwise) and
    ``self.field_valid`` int32[n, J].  It is one more launch after the sampling, and after normals / groups when they are
    given — :func:`point_fields` of ``self.cloud`` and the step's ``gt_aug`` with ``status=self.cloud_status``: joints and
    cloud are both in the step's mapped frame, in mm, which is ``radius``' unit.  ``step`` returns exactly what it returns
    without it; ``fields=None`` issues exactly the launches listed above."""

    def __init__(self, depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, n: int,
                 gt: Optional[torch.Tensor] = None, centres: Optional[torch.Tensor] = None, res: int = 32,
                 layout: str = "czyx", clamp: bool = True, cam: Optional[_lib.TsdfCam] = None, graph: bool = True,
                 dtype: Optional[torch.dtype] = None, base: Optional[torch.Tensor] = None, fused_head: bool = False,
                 heatmap: Optional[tuple] = None, fields: Optional[tuple] = None, groups: Optional[tuple] = None,
                 normals: Optional[int] = None, fps: Optional[tuple] = None, occupancy: Optional[tuple] = None,
                 tsdf: str = "projective"):
        self.accurate = _tsdf_kind(tsdf)
        self.heat = self._heatmap = None
        self.occ = self._occupancy = None
        self.cloud = self.cloud_pixel = self.cloud_count = self.cloud_status = self._fps = None
        if fps is not None:
            if not isinstance(fps, (tuple, list)) or len(fps) != 1:
                raise ValueError("fps must be (M,)")
            self._fps = _fps_points(fps[0])
        self.groups = self.normals = self._groups = self._normals_k = None
        if groups is not None or normals is not None:   # what a point network reads next to the sampled cloud
            if self._fps is None:
                raise ValueError("groups and normals need fps=(M,): they read the step's sampled cloud")
            if normals is not None:
                self._normals_k = _group_k(normals)
            if groups is not None:
                if not isinstance(groups, (tuple, list)) or not groups or \
                        not all(isinstance(g, (tuple, list)) and len(g) == 2 for g in groups):
                    raise ValueError("groups must be ((C, K), ...): one pair per set-abstraction level")
                if self._fps > _lib.GROUP_MAX_CLOUD:
                    raise ValueError(f"groups read a cloud of at most {_lib.GROUP_MAX_CLOUD} points")
                rows, self._groups = self._fps, []
                for C, K in groups:   # level l's cloud is the first C_{l-1} rows, level 0's the M sampled rows
                    self._groups.append((rows, _group_count("C", C, rows), _group_k(K)))
                    rows = C
            if self._normals_k is not None and self._fps > _lib.GROUP_MAX_CLOUD:
                raise ValueError(f"normals read a cloud of at most {_lib.GROUP_MAX_CLOUD} points")
        self.field = self.field_valid = self._fields = None
        if fields is not None:   # the point-wise labels of the sampled cloud
            if not isinstance(fields, (tuple, list)) or len(fields) not in (2, 3):
                raise ValueError("fields must be (K, radius) or (K, radius, dtype)")
            if self._fps is None or gt is None:
                raise ValueError("fields need fps=(M,) and gt: they are written from the step's sampled cloud and gt_aug")
            if self._fps > _lib.POINTFIELD_MAX_CLOUD:
                raise ValueError(f"fields read a cloud of at most {_lib.POINTFIELD_MAX_CLOUD} points")
            fdtype = fields[2] if len(fields) == 3 else torch.float32
            _heat_dtype(fdtype)
            self._fields = (_group_count("K", fields[0], _lib.POINTFIELD_MAX_K), _field_radius(fields[1]), fdtype)
        if occupancy is not None:
            if not isinstance(occupancy, (tuple, list)) or len(occupancy) not in (1, 2):
                raise ValueError("occupancy must be (res,) or (res, dtype)")
            odtype = occupancy[1] if len(occupancy) == 2 else torch.float32
            _heat_dtype(odtype)
            self._occupancy = (_heat_res(occupancy[0]), odtype)
        if heatmap is not None:
            if not isinstance(heatmap, (tuple, list)) or len(heatmap) not in (2, 3):
                raise ValueError("heatmap must be (res, sigma) or (res, sigma, dtype)")
            hdtype = heatmap[2] if len(heatmap) == 3 else torch.float32
            _heat_dtype(hdtype)
            self._heatmap = (_heat_res(heatmap[0]), _heat_sigma(heatmap[1]), hdtype)
            if gt is None:
                raise ValueError("heatmap needs gt: the volumes are written from the step's gt_nor")
        if graph not in (False, True):
            raise ValueError(f"graph must be False or True, got {graph!r}")
        if fused_head not in (False, True):
            raise ValueError(f"fused_head must be False or True, got {fused_head!r}")
        if dtype is not None:
            _lowp_dtype(dtype)
        self.dtype = dtype
        self.base = base
        self._head = bool(fused_head) or base is not None
        n = int(n)
        if n < 1:
            raise ValueError("n must be >= 1")
        dev, n_pack, R = _pack(_lib.load(), depth, offsets, headers, res, layout)
        self.n, self.res, self.layout, self.clamp, self.cam, self.device = n, R, layout, clamp, cam, dev
        self._pack_args = (depth, offsets, headers)
        self._gt = gt
        if base is not None:
            _shaped("base", base, (n_pack, 24), torch.float64, dev)
        if centres is not None:
            self.centres = centres
        elif base is not None:   # the un-augmented grid centre in the frame the volume is cut in
            self.centres = map_grids(depth, offsets, headers, base, res=R, cam=cam).mid_p
        else:
            self.centres = aabb(depth, offsets, headers, res=R, cam=cam).grid[:, :3].contiguous()
        _shaped("centres", self.centres, (n_pack, 3), torch.float32, dev)
        # index and state share one buffer, so that a step whose index comes from the host uploads both with one copy
        self._in = torch.zeros(n + 2, dtype=torch.int64, device=dev)
        self.index, self.state = self._in[:n], self._in[n:]
        self._h = [torch.zeros(n + 2, dtype=torch.int64).pin_memory() for _ in range(2)]   # staging, used in turn
        self._h_done = [None, None]   # the event after the copy that last read each staging buffer
        self._turn = 0
        self.xforms = torch.empty((n, 24), dtype=torch.float64, device=dev)
        self.out = empty_batch(n, R, dev)
        # the placed form of the step: a placement writes grid rows and a voxel pass runs on them (dtype, accurate)
        placed = self._placed = dtype is not None or self.accurate
        if self.accurate and dtype is not None:   # the accurate pass writes float32: narrow_volumes fills the 2-byte volume
            self._vol32 = self.out.tsdf
        if dtype is not None:   # the 2-byte volume
            self.out = self.out._replace(tsdf=torch.empty((n, 3, R, R, R), dtype=dtype, device=dev))
        if placed:   # the grid rows the placement hands to the voxel pass
            self._grid = MapGridBatch(torch.empty((n, 8), dtype=torch.float32, device=dev), *self.out[1:])
        self.gt_nor = self.gt_aug = None
        if gt is not None:
            _dev_check("gt", gt, torch.float32, dev, host_ok=not placed)
            if placed and gt.shape[0] != n_pack:
                raise ValueError("gt must hold the labels of every frame of the pack: [N, 3*J] or [N, J, 3]")
            shape = (n,) + tuple(gt.shape[1:])
            self.gt_nor = torch.empty(shape, dtype=torch.float32, device=dev)
            self.gt_aug = torch.empty(shape, dtype=torch.float32, device=dev)
            if placed and not self._head:   # the batch's frame numbers kept inside the pack, and its joints before the map
                self._sel = (torch.empty(n, dtype=torch.int64, device=dev), torch.empty(shape, dtype=torch.float32, device=dev))
            if self._heatmap is not None:   # the static target volumes, one per joint
                hres, _, hdtype = self._heatmap
                self.heat = torch.empty((n, _coords("gt", self.gt_nor, n) // 3, hres, hres, hres), dtype=hdtype, device=dev)
        if self._occupancy is not None:   # the static occupancy volume, at its own resolution
            ores, odtype = self._occupancy
            self.occ = torch.empty((n, 1, ores, ores, ores), dtype=odtype, device=dev)
        if self._fps is not None:   # the static sampled clouds
            self._cloud = _fps_out(None, n, self._fps, dev, radius2=False)
            self.cloud, self.cloud_pixel, _, self.cloud_count, self.cloud_status = self._cloud
        if self._groups is not None:   # the static groups, one KnnBatch per level
            self.groups = [_group_out(KnnBatch, None, (("index", (n, C, K), torch.int32), ("dist2", (n, C, K), torch.float32),
                                                       ("offsets", (n, C, K, 3), torch.float32), ("status", (n,), torch.int32)),
                                      {}, dev) for _, C, K in self._groups]
        if self._normals_k is not None:   # the static normals, and the viewpoint under the step's maps
            M = self._fps
            self.normals = _group_out(NormalBatch, None, (("normals", (n, M, 3), torch.float32), ("curvature", (n, M), torch.float32),
                                                          ("status", (n,), torch.int32)), {}, dev)
            self._view = torch.empty((n, 3), dtype=torch.float64, device=dev)
        if self._fields is not None:   # the static field, in layout "cp"
            J = _coords("gt", self.gt_aug, n) // 3
            self._field_out = PointFieldBatch(torch.empty((n, 4 * J, self._fps), dtype=self._fields[2], device=dev),
                                              torch.empty((n, J), dtype=torch.int32, device=dev),
                                              torch.empty((n,), dtype=torch.int32, device=dev))
            self.field, self.field_valid = self._field_out.field, self._field_out.valid
        if self._head:   # what map_step_head writes into: the object's own buffers
            g = self._grid if placed else MapGridBatch(None, None, None, None)
            self._head_out = MapStepBatch(self.xforms, g.grid, g.max_l, g.mid_p, g.status, self.gt_aug, self.gt_nor)
        self.graph = None
        self._run()                      # eagerly once: argument checks, library loads and the device check happen here
        if graph:
            torch.cuda.synchronize(dev)
            side = torch.cuda.Stream(dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                self._run()
            self.graph = g

    def _voxel_pass(self):
        """The voxel pass of the placed form on ``self._grid``'s rows, into the object's volume."""
        d, o, h = self._pack_args
        if not self.accurate:
            _map_grid_lowp(d, o, h, self.xforms, self._grid.grid, self.res, self.layout, self.dtype, self.cam, self.index,
                           self.out.tsdf, False)
            return
        vol32 = self.out.tsdf if self.dtype is None else self._vol32
        _map_grid_accurate(d, o, h, self.xforms, self._grid.grid, self.res, self.layout, self.cam, self.index, vol32, False)
        if self.dtype is not None:
            narrow_volumes(vol32, dtype=self.dtype, out=self.out.tsdf)

    def _run(self):
        self._step_launches()
        if self._heatmap is not None:   # one more launch at the end of the same linear sequence
            hres, sigma, hdtype = self._heatmap
            joint_heatmaps(self.gt_nor, hres, sigma, layout=self.layout, dtype=hdtype, status=self.out.status, out=self.heat)
        if self._occupancy is not None:   # and one more: the batch's points under the step's maps, binned into the step's cubes
            d, o, h = self._pack_args
            ores, odtype = self._occupancy
            _occupancy(d, o, h, self.out.max_l, self.out.mid_p, ores, self.layout, odtype, self.cam, self.xforms, self.index,
                       self.occ, 0, False)
        if self._fps is not None:   # and the last: the same points, farthest-point sampled
            d, o, h = self._pack_args
            _fps_crop(d, o, h, self._fps, self.cam, self.xforms, self.index, None, None, self._cloud, 0)
        if self._normals_k is not None:   # after it: a normal per sampled point, seen from the camera under the step's maps
            _normals(self.cloud, self._normals_k, None, self.cloud_status, _view_of(self.xforms, self.n, self._view), True,
                     self.normals)
        if self._groups is not None:   # and the levels' groups, each level's cloud a prefix of the sampled rows
            for (rows, C, K), out in zip(self._groups, self.groups):
                _knn(self.cloud[:, :rows], K, C, self.cloud_status, True, True, out)
        if self._fields is not None:   # and the point-wise labels: cloud and joints both in the step's mapped frame
            K, radius, fdtype = self._fields
            _point_fields(self.cloud, self.gt_aug, K, radius, "cp", fdtype, self.cloud_status, self._field_out)

    def _step_launches(self):
        d, o, h = self._pack_args
        if self._head:
            placed = self._placed
            map_step_head(d, o, h, self.centres, self.state, base=self.base, index=self.index,
                          gt=self._gt if placed else None, res=self.res, cam=self.cam, clamp=self.clamp, place=placed,
                          out=self._head_out)
            if placed:
                self._voxel_pass()
            else:
                voxelize_indexed(d, o, h, self.index, self._gt, res=self.res, layout=self.layout, cam=self.cam,
                                 clamp=self.clamp, out=self.out, xforms=self.xforms, out_gt_nor=self.gt_nor,
                                 out_gt=self.gt_aug)
            return
        aug_xforms_at(self.centres, self.state, index=self.index, out=self.xforms)
        if not self._placed:
            voxelize_indexed(d, o, h, self.index, self._gt, res=self.res, layout=self.layout, cam=self.cam, clamp=self.clamp,
                             out=self.out, xforms=self.xforms, out_gt_nor=self.gt_nor, out_gt=self.gt_aug)
            return
        map_grids(d, o, h, self.xforms, res=self.res, cam=self.cam, index=self.index, out=self._grid)
        self._voxel_pass()
        if self._gt is not None:
            _batch_labels(self._gt, self.index, h.shape[0], self.xforms, self.out.max_l, self.out.mid_p, self.clamp,
                          sel=self._sel, out_aug=self.gt_aug, out_nor=self.gt_nor)

    def step(self, index, key: int, counter0: int = 0):
        """Voxelize pack frames ``index`` (n frame numbers: an int64 tensor on the device or the host, or any sequence of
        integers), position i under the augmentation drawn from ``(key, counter0 + i)``.  Returns the object's outputs:
        ``TsdfBatch``, or ``(TsdfBatch, gt_nor, gt_of_the_batch)`` with labels.  Enqueues on the current stream and does not
        synchronise."""
        n = self.n
        k = self._turn & 1
        self._turn += 1
        h = self._h[k]
        if self._h_done[k] is not None:
            self._h_done[k].synchronize()     # the copy that read this staging buffer two steps ago
        hn = h.numpy()
        hn[n] = _i64(key)
        hn[n + 1] = _i64(counter0)
        with _Current(self.device):
            if isinstance(index, torch.Tensor) and index.is_cuda:
                _shaped("index", index, (n,), torch.int64, self.device)
                self.index.copy_(index)
                self.state.copy_(h[n:], non_blocking=True)
            else:
                src = index.numpy() if isinstance(index, torch.Tensor) else index
                if len(src) != n:
                    raise ValueError(f"index must hold {n} frame numbers")
                hn[:n] = src
                self._in.copy_(h, non_blocking=True)
            if self._h_done[k] is None:
                self._h_done[k] = torch.cuda.Event()
            self._h_done[k].record(torch.cuda.current_stream(self.device))
            if self.graph is not None:
                self.graph.replay()
            else:
                self._run()
        return self.out if self._gt is None else (self.out, self.gt_nor, self.gt_aug)


class PointCloudBatch(NamedTuple):
    points: torch.Tensor  # float64[n, P, 3]
    count: torch.Tensor   # int32[n]  valid pixels of the frame (m)
    status: torch.Tensor  # int32[n]  (_lib.TSDF_FRAME_*)


def point_clouds(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, points: int = 6000, seed: int = 0,
                 frame_base: int = 0, xforms: Optional[torch.Tensor] = None, cam: Optional[_lib.TsdfCam] = None,
                 out: Optional[PointCloudBatch] = None) -> PointCloudBatch:
    """``DataProcess.point_cloud`` + ``set_length`` (pre/process.py:30-84) for n packed frames in one launch
    (``tsdf_point_clouds_hip``; the contract is in include/tsdf.h): every pixel with d != 0 back-projected in float64,
    resampled to ``points`` points by a counter-based draw from ``seed`` and the frame's number ``frame_base + i``
    (so a batch split over several calls gives the same clouds as one call).

    xforms  optional float64[n, 24] on the GPU (``augment.random_affines``): the points are mapped with the forward rows.
    Returns :class:`PointCloudBatch`; frames that are not OK get all-zero rows.  Enqueues on the current stream and
    returns without synchronising."""
    L = _lib.load()
    dev, n, _ = _pack(L, depth, offsets, headers)
    P = int(points)
    if not 1 <= P <= 0x7fffffff:
        raise ValueError("points must be in 1..2^31-1")
    seed, frame_base = int(seed), int(frame_base)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in [0, 2^64)")
    if not -2 ** 63 <= frame_base < 2 ** 63:
        raise ValueError("frame_base must fit int64")
    if xforms is not None:
        _shaped("xforms", xforms, (n, 24), torch.float64, dev)
    out = _outs(PointCloudBatch, out, (("points", (n, P, 3), torch.float64), ("count", (n,), torch.int32),
                                       ("status", (n,), torch.int32)), dev)
    if n:
        _call(dev, L.tsdf_point_clouds_hip,
              [depth.data_ptr(), depth.numel(), offsets.data_ptr(), headers.data_ptr(), n, P, _cam(cam), seed, frame_base,
               _ptr(xforms), None, out.points.data_ptr(), out.count.data_ptr(), out.status.data_ptr()], 10)
    return out


class CloudGridBatch(NamedTuple):
    grid: torch.Tensor    # float32[n, 8]  vox_ori[3], voxel_len, trunc_dis, 0, 0, 0 (the ``grid`` of voxelize_grid)
    max_l: torch.Tensor   # float32[n]
    mid_p: torch.Tensor   # float32[n, 3]
    aabb: torch.Tensor    # float32[n, 6]  min xyz, max xyz of the cloud (z over the points with z != 0)
    status: torch.Tensor  # int32[n]  (_lib.TSDF_FRAME_*)


def cloud_grids(points: torch.Tensor, res: int = 32, cam: Optional[_lib.TsdfCam] = None) -> CloudGridBatch:
    """The grid placement ``tsdf_f(data, point_cloud)`` derives from the cloud it is handed (pre/tsdf_for.py:9-16 with
    ``max_min_point``, :23-41) for n clouds in one launch (``tsdf_cloud_grid_hip``; the contract is in include/tsdf.h):
    per-axis extremes as float32 (z over the points with z != 0), then the float32 glue.

    points  float64[n, P, 3] on the GPU — what :func:`point_clouds` returns, or any other cloud.
    Returns :class:`CloudGridBatch`; ``grid`` goes straight to :func:`voxelize_grid`.  A cloud without a z != 0, with a
    NaN, of non-finite or zero extent is TSDF_FRAME_DEGENERATE: zero grid row, ``max_l`` 0.  Enqueues on the current
    stream and returns without synchronising."""
    L = _lib.load()
    _dev_check("points", points, torch.float64)
    dev = points.device
    if points.dim() != 3 or points.shape[2] != 3:
        raise ValueError("points must have shape [n, P, 3]")
    n, P = int(points.shape[0]), int(points.shape[1])
    if not 1 <= P <= 0x7fffffff:
        raise ValueError("points must hold 1..2^31-1 points per frame")
    if not L.tsdf_resolution_supported(int(res)):
        raise ValueError(f"unsupported grid resolution {res} (multiple of 4 in 4..128)")
    out = _outs(CloudGridBatch, None, (("grid", (n, 8), torch.float32), ("max_l", (n,), torch.float32),
                                       ("mid_p", (n, 3), torch.float32), ("aabb", (n, 6), torch.float32),
                                       ("status", (n,), torch.int32)), dev)
    if n:
        _call(dev, L.tsdf_cloud_grid_hip, [points.data_ptr(), n, P, int(res), _cam(cam), None, out.grid.data_ptr(),
                                           out.max_l.data_ptr(), out.mid_p.data_ptr(), out.aabb.data_ptr(),
                                           out.status.data_ptr()], 5)
    return out


class ProcessBatch(NamedTuple):
    points: torch.Tensor  # float64[n, P, 3]  the resampled clouds
    tsdf: torch.Tensor    # float32[n, 3, R, R, R] (float16 / bfloat16 with process_batch(dtype=...))
    max_l: torch.Tensor   # float32[n]
    mid_p: torch.Tensor   # float32[n, 3]
    status: torch.Tensor  # int32[n]  the first non-zero status of the three stages
    count: torch.Tensor   # int32[n]  valid pixels of the frame


def process_batch(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, points: int = 6000, seed: int = 0,
                  frame_base: int = 0, res: int = 32, layout: str = "czyx",
                  cam: Optional[_lib.TsdfCam] = None, dtype: Optional[torch.dtype] = None) -> ProcessBatch:
    """``DataProcess.process()`` (pre/process.py:13-28) for n packed frames: back-project and resample the cloud
    (:func:`point_clouds`), place the grid on the AABB of THAT cloud (:func:`cloud_grids` — the reference's rule; every
    other batched path places it on all valid pixels) and voxelize with that placement (:func:`voxelize_grid`).  Three
    launches on the current stream, no synchronisation, nothing on the host in between.

    ``seed`` / ``frame_base`` as for :func:`point_clouds`: a batch split over several calls gives the same result.
    A frame that is not OK in any stage has a zero volume and ``max_l`` 0; ``status`` is the first non-zero status among
    the stages (cloud, grid, volume).

    ``dtype`` (torch.float16 / torch.bfloat16): the last stage is :func:`voxelize_grid_lowp` on the same rows and ``tsdf``
    has that type; every other field is unchanged."""
    pc, cg, tsdf, status = _process_half(depth, offsets, headers, points, seed, frame_base, res, layout, cam, dtype)
    return ProcessBatch(pc.points, tsdf, cg.max_l, cg.mid_p, status, pc.count)


def _process_half(depth, offsets, headers, points, seed, frame_base, res, layout, cam, dtype, xforms=None):
    """The three stages of ``process()`` — the resampled cloud (under ``xforms``), the grid on it, the volume on that grid
    (:func:`_grid_pass`) —: ``(PointCloudBatch, CloudGridBatch, volume, first non-zero status of the three)``."""
    if dtype is not None:
        _lowp_dtype(dtype)
    pc = point_clouds(depth, offsets, headers, points=points, seed=seed, frame_base=frame_base, xforms=xforms, cam=cam)
    cg = cloud_grids(pc.points, res=res, cam=cam)
    vol, st = _grid_pass(depth, offsets, headers, cg.grid, res=res, layout=layout, cam=cam, xforms=xforms, dtype=dtype)
    return pc, cg, vol, _first_status(pc.status, cg.status, st)


def voxelize_aug_grid(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, xforms: torch.Tensor,
                      grid: torch.Tensor, res: int = 32, layout: str = "czyx", cam: Optional[_lib.TsdfCam] = None):
    """:func:`voxelize_aug` on a grid the caller supplies — the augmented twin of :func:`voxelize_grid`
    (``tsdf_voxelize_aug_grid_hip`` of libtsdf_auggrid.so; include/tsdf_auggrid.h has the contract).

    xforms  float64[n,24] on the GPU: forward rows then inverse rows, as for :func:`voxelize_aug`
    grid    float32[n,8] on the GPU: vox_ori[3], voxel_len, trunc_dis, 3 pad words per frame, in the MAPPED frame — what
            :func:`cloud_grids` returns for the mapped cloud
    Returns ``(tsdf float32[n,3,R,R,R], status int32[n])``.  A frame with a bad header (2) or an unusable grid row (1:
    ``trunc_dis`` not positive, or anything non-finite) gets a zero volume; the crop is not scanned, so a frame without a
    valid pixel gets a zero volume with status 0.  One launch on the current stream, no synchronisation."""
    G = _lib.load_auggrid()
    dev, n, R = _pack(_lib.load(), depth, offsets, headers, res, layout)
    _shaped("xforms", xforms, (n, 24), torch.float64, dev)
    _shaped("grid", grid, (n, 8), torch.float32, dev)
    tsdf = _out("tsdf", None, (n, 3, R, R, R), torch.float32, dev)
    st = _out("status", None, (n,), torch.int32, dev)
    if n:
        _call(dev, G.tsdf_voxelize_aug_grid_hip, _head(depth, offsets, headers, n, R, cam, layout) +
              [xforms.data_ptr(), grid.data_ptr(), tsdf.data_ptr(), st.data_ptr()], 8)
    return tsdf, st


def transform_joints(gt: torch.Tensor, xforms: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The joints under each frame's forward map, on their own (``tsdf_transform_joints_hip`` of libtsdf_auggrid.so):
    ``fma(A_i0, x, fma(A_i1, y, fma(A_i2, z, b_i)))`` in float64, rounded to float32 — bit-identical to the ``gt_aug``
    :func:`voxelize_aug` ``(..., gt=)`` returns.  gt float32[n,3J] or [n,J,3] on the GPU, xforms float64[n,24]; the result
    has gt's shape (``out``: a preallocated tensor of that shape to write into)."""
    G = _lib.load_auggrid()
    _dev_check("gt", gt, torch.float32)
    if gt.dim() < 2:
        raise ValueError("gt must have shape [n, 3*J] or [n, J, 3]")
    dev, n = gt.device, gt.shape[0]
    nc = _coords("gt", gt, n)
    _shaped("xforms", xforms, (n, 24), torch.float64, dev)
    out = _out("gt_aug", out, tuple(gt.shape), torch.float32, dev)
    if n:
        _call(dev, G.tsdf_transform_joints_hip, [gt.data_ptr(), xforms.data_ptr(), n, nc // 3, None, out.data_ptr()], 4)
    return out


class ProcessAugBatch(NamedTuple):
    points: torch.Tensor       # float64[n, P, 3]  the resampled clouds
    tsdf: torch.Tensor         # float32[n, 3, R, R, R] (float16 / bfloat16 with process_batch_aug(dtype=...), and tsdf_aug)
    max_l: torch.Tensor        # float32[n]
    mid_p: torch.Tensor        # float32[n, 3]
    points_aug: torch.Tensor   # float64[n, P, 3]  the mapped clouds, resampled with their own draw
    tsdf_aug: torch.Tensor     # float32[n, 3, R, R, R]  on the grid of points_aug
    max_l_aug: torch.Tensor    # float32[n]
    mid_p_aug: torch.Tensor    # float32[n, 3]
    gt_aug: Optional[torch.Tensor]   # the joints under the map (gt's shape), or None without gt
    status: torch.Tensor       # int32[n]  first non-zero status of the plain stages
    status_aug: torch.Tensor   # int32[n]  first non-zero status of the augmented stages
    count: torch.Tensor        # int32[n]  valid pixels of the frame
    xforms: torch.Tensor       # float64[n, 24]  the maps that were used


def process_batch_aug(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor,
                      xforms: Optional[torch.Tensor] = None, gt: Optional[torch.Tensor] = None, points: int = 6000,
                      seed: int = 0, aug_seed: int = 0, key: int = 0, frame_base: int = 0, res: int = 32,
                      layout: str = "czyx", cam: Optional[_lib.TsdfCam] = None,
                      dtype: Optional[torch.dtype] = None) -> ProcessAugBatch:
    """``DataProcess(aug=True).process()`` (pre/process.py:13-28) for n packed frames: the nine entries of the reference's
    dictionary plus the bookkeeping, every stage on the current stream, no synchronisation, nothing on the host.

    The plain half is :func:`process_batch` (``points, tsdf, max_l, mid_p, status, count`` equal it bit for bit).  The
    augmented half (pre/process.py:19-24: data_aug, set_length, tsdf_f on the augmented resampled cloud):
      1. ``xforms`` (float64[n,24]) or, when None, ``aug_xforms(mid_p, key=key, counter0=frame_base)``: every frame is turned
         about its own plain cloud-grid centre, position i drawing from ``(key, frame_base + i)``;
      2. ``points_aug = point_clouds(..., seed=aug_seed, frame_base=frame_base, xforms=xforms)``;
      3. ``cloud_grids(points_aug)`` gives ``max_l_aug`` / ``mid_p_aug`` and the grid;
      4. ``tsdf_aug = voxelize_aug_grid(..., xforms, grid)``;
      5. ``gt_aug = transform_joints(gt, xforms)`` when ``gt`` (float32[n,3J] or [n,J,3]) is given.
    ``status_aug`` is the first non-zero status among the augmented cloud, grid and volume stages.  A batch split over
    several calls with ``frame_base`` gives the same result as one call.

    ``dtype`` (torch.float16 / torch.bfloat16): ``tsdf`` comes from :func:`process_batch` ``(dtype=)`` and ``tsdf_aug`` from
    :func:`voxelize_map_grid_lowp` on the same rows, both of that type; every other field is unchanged bit for bit."""
    pb = process_batch(depth, offsets, headers, points=points, seed=seed, frame_base=frame_base, res=res, layout=layout,
                       cam=cam, dtype=dtype)
    if xforms is None:
        xforms = aug_xforms(pb.mid_p, key=key, counter0=frame_base)
    pa, cg, tsdf_aug, status_aug = _process_half(depth, offsets, headers, points, aug_seed, frame_base, res, layout, cam, dtype,
                                                 xforms=xforms)
    gt_aug = transform_joints(gt, xforms) if gt is not None else None
    return ProcessAugBatch(pb.points, pb.tsdf, pb.max_l, pb.mid_p, pa.points, tsdf_aug, cg.max_l, cg.mid_p, gt_aug,
                           pb.status, status_aug, pb.count, xforms)


def widen_depth16(src_u16: torch.Tensor, shift: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """16-bit depth -> the float32 depth the voxelizers read: ``out[i] = float(src_u16[i]) * 2^-shift``, exact, by one
    launch on the current stream (``tsdf_depth16_widen_hip`` of libtsdf_depth16.so; include/tsdf_depth16.h has the
    contract, ``packing`` the encoding).  ``src_u16``: uint16 on the GPU, contiguous — any slice of a larger buffer, no
    alignment beyond the element's is asked; ``shift`` 0..7; ``out``: float32 of the same shape on the same device
    (allocated when None), likewise any slice.  No synchronisation."""
    D = _lib.load_depth16()
    _dev_check("src_u16", src_u16, torch.uint16)
    if isinstance(shift, bool) or not isinstance(shift, int) or not 0 <= shift <= _lib.DEPTH16_MAX_SHIFT:
        raise ValueError(f"shift must be an integer in 0..{_lib.DEPTH16_MAX_SHIFT}, got {shift!r}")
    dev = src_u16.device
    out = _out("out", out, tuple(src_u16.shape), torch.float32, dev)
    if src_u16.numel():
        _call(dev, D.tsdf_depth16_widen_hip, [src_u16.data_ptr(), src_u16.numel(), shift, out.data_ptr(), None], 4)
    return out


class ObbBatch(NamedTuple):
    xforms: torch.Tensor        # float64[n,24]  forward rows then inverse rows: what voxelize_aug / voxelize_indexed take
    status: torch.Tensor        # int32[n]       (_lib.TSDF_FRAME_*)
    count: torch.Tensor         # float64[n]     valid pixels N (an exact integer; a view of the moments row)
    mean: torch.Tensor          # float64[n,3]   the centroid mu
    cov: torch.Tensor           # float64[n,6]   xx xy xz yy yz zz, divisor N
    eigenvalues: torch.Tensor   # float64[n,3]   descending


def obb_xforms(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, cam: Optional[_lib.TsdfCam] = None,
               out: Optional[torch.Tensor] = None) -> ObbBatch:
    """The principal-axis (oriented-bounding-box) map of every frame, computed on the GPU (``tsdf_obb_xforms_hip`` of
    libtsdf_obb.so; include/tsdf_obb.h has the contract): the rotation about the cloud's centroid that turns its principal
    axes into x (largest extent), y and z (smallest), signs by HandPointNet's convention.  Feed ``xforms`` to
    :func:`voxelize_aug` and the volume, ``max_l`` / ``mid_p`` and the labels no longer depend on how the hand is turned
    in the image plane.  The map is rigid: distances between joints, and pose error, are what they are in the camera frame.

    depth / offsets / headers as for :func:`voxelize`; ``out``: optional float64[n,24] to write the maps into (it is
    ``ObbBatch.xforms`` then).  A frame with a bad header (status 2) or fewer than 3 valid pixels, non-finite or all-equal
    points (status 1) gets the identity map and zero moments.  ``count`` / ``mean`` / ``cov`` / ``eigenvalues`` are views
    of one float64[n,16] tensor.  One launch on the current stream, no synchronisation."""
    O = _lib.load_obb()
    dev, n, _ = _pack(_lib.load(), depth, offsets, headers)
    xf = _out("out", out, (n, 24), torch.float64, dev)
    mo = _out("moments", None, (n, 16), torch.float64, dev)
    st = _out("status", None, (n,), torch.int32, dev)
    if n:
        _call(dev, O.tsdf_obb_xforms_hip, [depth.data_ptr(), depth.numel(), offsets.data_ptr(), headers.data_ptr(), n,
                                           _cam(cam), None, xf.data_ptr(), mo.data_ptr(), st.data_ptr()], 6)
    return ObbBatch(xf, st, mo[:, 0], mo[:, 1:4], mo[:, 4:10], mo[:, 10:13])


def voxelize_obb(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, res: int = 32, layout: str = "czyx",
                 cam: Optional[_lib.TsdfCam] = None, gt: Optional[torch.Tensor] = None, clamp: bool = True,
                 dtype: Optional[torch.dtype] = None, tsdf: str = "projective"):
    """Volumes cut in every cloud's own principal axes: :func:`obb_xforms` followed by :func:`voxelize_aug` on the same
    stream, nothing on the host in between.  Returns ``(TsdfBatch, xforms)``, or with ``gt`` (float32[n,3J] on the GPU)
    ``(TsdfBatch, gt_nor, gt_obb, xforms)``: ``gt_obb`` are the joints in the mapped frame, ``gt_nor`` their labels;
    ``max_l`` / ``mid_p`` are in the mapped frame, as for :func:`voxelize_aug`.  Predictions go back to the camera frame
    with ``transform_joints(pred, invert_xforms(xforms))``.

    ``dtype`` (torch.float16 / torch.bfloat16): :func:`voxelize_aug_lowp` takes :func:`voxelize_aug`'s place and ``tsdf``
    has that type; everything else is unchanged bit for bit.

    ``tsdf="accurate"``: the accurate directional TSDF, :func:`voxelize_aug_accurate` in the voxelizer's place (with
    ``dtype``: narrowed afterwards); every other field is unchanged bit for bit."""
    accurate = _tsdf_kind(tsdf)
    if dtype is not None:
        _lowp_dtype(dtype)
    xf = obb_xforms(depth, offsets, headers, cam=cam).xforms
    if accurate:
        r = voxelize_aug_accurate(depth, offsets, headers, xf, res=res, layout=layout, dtype=dtype, cam=cam, gt=gt,
                                  clamp=clamp)
    elif dtype is None:
        r = voxelize_aug(depth, offsets, headers, xf, res=res, layout=layout, cam=cam, gt=gt, clamp=clamp)
    else:
        r = voxelize_aug_lowp(depth, offsets, headers, xf, res=res, layout=layout, dtype=dtype, cam=cam, gt=gt, clamp=clamp)
    return (r, xf) if gt is None else (r[0], r[1], r[2], xf)


def invert_xforms(xforms: torch.Tensor) -> torch.Tensor:
    """The same maps with the forward and inverse halves swapped (float64[n,24] -> float64[n,24]; a pure tensor
    operation, on whatever device ``xforms`` lives): ``transform_joints(x, invert_xforms(xf))`` carries joints of the mapped
    frame back to the camera's."""
    if not isinstance(xforms, torch.Tensor):
        raise TypeError("xforms must be a torch.Tensor")
    if xforms.dim() != 2 or xforms.shape[1] != 24:
        raise ValueError("xforms must have shape [n, 24] (forward rows then inverse rows)")
    return torch.cat([xforms[:, 12:], xforms[:, :12]], dim=1)


def _source(depth, offsets, headers, index, res, layout):
    """The one validation of the source tables with an optional index (int64[n] on the GPU: batch position i takes source
    frame index[i]; without it the batch is the n_src frames).  Returns (device, n_src, n, R)."""
    dev, n_src, R = _pack(_lib.load(), depth, offsets, headers, res, layout)
    n = n_src if index is None else _indexed(index, n_src, dev, "index needs at least one source frame")
    return dev, n_src, n, R


def _indexed(index, n_src, dev, nothing_to_index: str) -> int:
    """The one check of an index into ``n_src`` frames (int64[n] on ``dev``); returns the batch's n."""
    _dev_check("index", index, torch.int64, dev)
    if index.dim() != 1:
        raise ValueError("index must have shape [n]")
    n = int(index.shape[0])
    if n and not n_src:
        raise ValueError(nothing_to_index)
    return n


def _src_head(depth, offsets, headers, n_src, index, n, R) -> list:
    """The eight arguments every indexed extension entry starts with."""
    return [depth.data_ptr(), depth.numel(), offsets.data_ptr(), headers.data_ptr(), n_src, _ptr(index), n, R]


_LOWP_DTYPES = {torch.float16: _lib.TSDF_LOWP_F16, torch.bfloat16: _lib.TSDF_LOWP_BF16}


def _lowp_dtype(dtype) -> int:
    """enum tsdf_lowp_dtype of a torch dtype; anything but float16 / bfloat16 is a ValueError."""
    code = _LOWP_DTYPES.get(dtype) if isinstance(dtype, torch.dtype) else None
    if code is None:
        raise ValueError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype!r}")
    return code


def voxelize_grid_lowp(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, grid: torch.Tensor,
                       res: int = 32, layout: str = "czyx", dtype: torch.dtype = torch.bfloat16,
                       cam: Optional[_lib.TsdfCam] = None, index: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None):
    """:func:`voxelize_grid` written as float16 / bfloat16 voxels (``tsdf_voxelize_grid_lowp_hip`` of libtsdf_lowp.so;
    include/tsdf_lowp.h has the contract): every voxel is the float32 value of the plain pass narrowed by
    round-to-nearest-even in registers, so the volume is written once, at half the bytes.

    depth / offsets / headers   the n_src source frames, as for :func:`voxelize`
    grid    float32[n_src,8] on the GPU: vox_ori[3], voxel_len, trunc_dis, 3 pad words per SOURCE frame
    dtype   torch.float16 or torch.bfloat16
    index   optional int64[n] on the GPU: batch position i voxelizes source frame index[i] (repeats allowed; an entry
            outside [0, n_src) gives that position status 2 and a zero volume).  Without it the batch is the n_src frames
    out     optional preallocated ``dtype[n,3,R,R,R]`` (a contiguous view of a larger buffer will do) to write into
    Returns ``(tsdf dtype[n,3,R,R,R], status int32[n])``.  A bad header (2) or an unusable grid row (1: ``trunc_dis`` not
    positive, or anything non-finite) gives a zero volume; the crop is not scanned, so a frame without a valid pixel gets
    a zero volume with status 0.  One launch on the current stream, no synchronisation."""
    code = _lowp_dtype(dtype)
    P = _lib.load_lowp()
    dev, n_src, n, R = _source(depth, offsets, headers, index, res, layout)
    _shaped("grid", grid, (n_src, 8), torch.float32, dev)
    tsdf = _out("out", out, (n, 3, R, R, R), dtype, dev)
    st = _out("status", None, (n,), torch.int32, dev)
    if n:
        _call(dev, P.tsdf_voxelize_grid_lowp_hip,
              _src_head(depth, offsets, headers, n_src, index, n, R) +
              [_cam(cam), _lib.LAYOUTS[layout], code, None, grid.data_ptr(), tsdf.data_ptr(), st.data_ptr()], 11)
    return tsdf, st


def voxelize_lowp(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, res: int = 32, layout: str = "czyx",
                  dtype: torch.dtype = torch.bfloat16, cam: Optional[_lib.TsdfCam] = None) -> TsdfBatch:
    """:func:`voxelize` with a float16 / bfloat16 volume: :func:`aabb` places the grid, the rows are put together on the
    device and :func:`voxelize_grid_lowp` writes the volume.  Nothing runs on the host in between, but it is TWO launches
    and the crop is read twice (the fused float32 entry reads it once).  ``max_l`` / ``mid_p`` / ``status`` are
    :func:`aabb`'s, bit for bit those of :func:`voxelize`; ``tsdf`` is ``dtype[n,3,R,R,R]``."""
    _lowp_dtype(dtype)
    return _placed_pass(depth, offsets, headers, _place_aabb(depth, offsets, headers, res, cam), res=res, layout=layout,
                        cam=cam, dtype=dtype)


def narrow_volumes(tsdf32: torch.Tensor, dtype: torch.dtype = torch.bfloat16,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 values narrowed to float16 / bfloat16 by round-to-nearest-even (``tsdf_lowp_narrow_hip`` of libtsdf_lowp.so):
    the cast :func:`voxelize_grid_lowp` applies in registers, for volumes that are already float32.  ``tsdf32``: float32 on
    the GPU, contiguous, any shape, 16-byte aligned; ``out``: ``dtype`` of the same shape (allocated when None).  One launch
    on the current stream, no synchronisation."""
    code = _lowp_dtype(dtype)
    P = _lib.load_lowp()
    _dev_check("tsdf32", tsdf32, torch.float32)
    dev = tsdf32.device
    out = _out("out", out, tuple(tsdf32.shape), dtype, dev)
    if tsdf32.numel():
        _call(dev, P.tsdf_lowp_narrow_hip, [tsdf32.data_ptr(), tsdf32.numel(), code, None, out.data_ptr()], 3)
    return out


def voxelize_grid_accurate(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, grid: torch.Tensor,
                           res: int = 32, layout: str = "czyx", cam: Optional[_lib.TsdfCam] = None,
                           index: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                           nearest: bool = False):
    """The ACCURATE directional TSDF on a caller-supplied grid (``tsdf_voxelize_grid_accurate_hip`` of
    libtsdf_accurate.so; include/tsdf_accurate.h has the contract): per voxel the nearest surface point among ALL valid
    pixels of the crop, where :func:`voxelize_grid` takes the one pixel the voxel projects to and rejects the voxel when
    that pixel is empty.  A voxel within the truncation distance of some point gets ``min(|v - w| / trunc_dis, 1)`` per
    channel with the plain pass's sign (positive where the plain pass rejects); every other voxel keeps the plain value.

    depth / offsets / headers   the n_src source frames, as for :func:`voxelize`
    grid    float32[n_src,8] on the GPU: vox_ori[3], voxel_len, trunc_dis, 3 pad words per SOURCE frame
    cam     a :class:`TsdfCam` or None (the MSRA defaults); its five constants go to the entry by value
    index   optional int64[n] on the GPU: batch position i voxelizes source frame index[i] (repeats allowed; an entry
            outside [0, n_src) gives that position status 2 and a zero volume).  Without it the batch is the n_src frames
    out     optional preallocated ``float32[n,3,R,R,R]`` (a contiguous view of a larger buffer will do) to write into
    nearest True: also ``int32[n,R,R,R]``, per voxel the row-major crop index of its nearest pixel, -1 for a far voxel,
            in the index order of one channel of the volume
    Returns ``(tsdf float32[n,3,R,R,R], status int32[n])``, with ``nearest`` a third tensor.  A bad header (2) or an
    unusable grid row (1: ``trunc_dis`` not positive, or anything non-finite) gives a zero volume; a frame without a valid
    pixel gets a zero volume with status 0.  One launch on the current stream, no synchronisation.  A voxel within the
    truncation distance of the camera plane is searched over the whole crop: keep such grids to small crops."""
    A = _lib.load_accurate()
    dev, n_src, n, R = _source(depth, offsets, headers, index, res, layout)
    _shaped("grid", grid, (n_src, 8), torch.float32, dev)
    tsdf = _out("out", out, (n, 3, R, R, R), torch.float32, dev)
    st = _out("status", None, (n,), torch.int32, dev)
    near = _out("nearest", None, (n, R, R, R), torch.int32, dev) if nearest else None
    if n:
        _call(dev, A.tsdf_voxelize_grid_accurate_hip,
              _src_head(depth, offsets, headers, n_src, index, n, R) + _cam5(cam) +
              [_lib.LAYOUTS[layout], None, grid.data_ptr(), tsdf.data_ptr(), _ptr(near), st.data_ptr()], 14)
    return (tsdf, st, near) if nearest else (tsdf, st)


class MapGridBatch(NamedTuple):
    """A grid placement (:func:`map_grids`, :func:`_place_aabb`).  :class:`CloudGridBatch` and a :class:`HandCrops` with its
    cube have the same four fields by name: ``grid`` goes to :func:`_grid_pass`, the rest into a composed entry's result."""
    grid: torch.Tensor    # float32[n, 8]  vox_ori[3], voxel_len, trunc_dis, 0, 0, 0 (the ``grid`` of the voxel passes)
    max_l: torch.Tensor   # float32[n]     in the mapped frame
    mid_p: torch.Tensor   # float32[n, 3]
    status: torch.Tensor  # int32[n]  (_lib.TSDF_FRAME_*)


def _placement_fields(n):
    return (("grid", (n, 8), torch.float32), ("max_l", (n,), torch.float32), ("mid_p", (n, 3), torch.float32),
            ("status", (n,), torch.int32))


def _place_aabb(depth, offsets, headers, res=32, cam=None, rows: bool = True) -> MapGridBatch:
    """:func:`aabb`'s placement: the one place its columns (mid_p[3], max_l, voxel_len, trunc_dis; vox_ori apart) become the
    passes' grid rows, put together on the device.  ``rows=False``: no ``grid``, for who wants the labels' frame alone."""
    ab = aabb(depth, offsets, headers, res=res, cam=cam)
    grid = torch.cat([ab.ori, ab.grid[:, 4:6], torch.zeros_like(ab.ori)], dim=1) if rows else None
    return MapGridBatch(grid, ab.grid[:, 3].contiguous(), ab.grid[:, :3].contiguous(), ab.status)


def _first_status(*stages: torch.Tensor) -> torch.Tensor:
    """Per frame the first non-zero status of the stages, in their order."""
    status = stages[-1]
    for st in reversed(stages[:-1]):
        status = torch.where(st != 0, st, status)
    return status


_TSDF_KINDS = ("projective", "accurate")


def _tsdf_kind(tsdf) -> bool:
    """``tsdf=`` of a composed entry: True for the accurate volume; anything but the two names is a ValueError."""
    if tsdf not in _TSDF_KINDS:
        raise ValueError("tsdf must be 'projective' or 'accurate'")
    return tsdf == "accurate"


def _grid_pass(depth, offsets, headers, grid, *, res, layout, cam, xforms=None, dtype=None, tsdf="projective", index=None,
               out=None):
    """The voxel pass on the rows ``grid`` that (``xforms``, ``dtype``, ``tsdf``) name, ``(volume, status)`` — the one table
    of the passes there are ("Placement, pass, status"):
        projective   voxelize_grid | dtype: voxelize_grid_lowp | xforms: voxelize_aug_grid | both: voxelize_map_grid_lowp
        accurate     voxelize_grid_accurate, with dtype then narrow_volumes; under xforms a ValueError: the mapped accurate
                     pass is voxelize_map_grid_accurate, reached by the entries listed there (voxelize_aug_accurate,
                     voxelize_obb and AugmentedStep with tsdf="accurate"), not through this table
    ``index`` / ``out`` (with ``dtype``: the narrow volume) go to the entries whose ABI has them; the two float32 projective
    entries have neither and refuse them.  Every refusal comes before the first launch."""
    if dtype is not None:
        _lowp_dtype(dtype)
    accurate = _tsdf_kind(tsdf)
    pack = (depth, offsets, headers) if xforms is None else (depth, offsets, headers, xforms)
    kw = dict(res=res, layout=layout, cam=cam)
    if accurate:
        if xforms is not None:
            raise ValueError("tsdf='accurate' takes no xforms: the accurate pass under a per-frame map is "
                             "voxelize_map_grid_accurate, not reached through this table")
        vol, status = voxelize_grid_accurate(*pack, grid, index=index, out=out if dtype is None else None, **kw)
        return (vol if dtype is None else narrow_volumes(vol, dtype=dtype, out=out)), status
    if dtype is not None:
        entry = voxelize_grid_lowp if xforms is None else voxelize_map_grid_lowp
        return entry(*pack, grid, dtype=dtype, index=index, out=out, **kw)
    if index is not None or out is not None:
        raise ValueError(("voxelize_grid" if xforms is None else "voxelize_aug_grid") + " takes neither index nor out")
    return (voxelize_grid if xforms is None else voxelize_aug_grid)(*pack, grid, **kw)


def _placed_pass(depth, offsets, headers, place: MapGridBatch, **how) -> TsdfBatch:
    """:func:`_grid_pass` on the rows of ``place``, as a batch with the PLACEMENT's ``max_l`` / ``mid_p`` / ``status``."""
    vol, _ = _grid_pass(depth, offsets, headers, place.grid, **how)
    return TsdfBatch(vol, place.max_l, place.mid_p, place.status)


def voxelize_accurate(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, res: int = 32,
                      layout: str = "czyx", cam: Optional[_lib.TsdfCam] = None) -> TsdfBatch:
    """:func:`voxelize` with the accurate directional TSDF: :func:`aabb` places the grid, the rows are put together on the
    device and :func:`voxelize_grid_accurate` writes the volume.  Nothing runs on the host in between; it is two launches.
    ``max_l`` / ``mid_p`` / ``status`` are :func:`aabb`'s, bit for bit those of :func:`voxelize`."""
    return _placed_pass(depth, offsets, headers, _place_aabb(depth, offsets, headers, res, cam), res=res, layout=layout,
                        cam=cam, tsdf="accurate")


def map_grids(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, xforms: torch.Tensor, res: int = 32,
              cam: Optional[_lib.TsdfCam] = None, index: Optional[torch.Tensor] = None,
              out: Optional[MapGridBatch] = None) -> MapGridBatch:
    """The grid placement of :func:`voxelize_aug` on its own (``tsdf_map_place_hip`` of libtsdf_maplowp.so;
    include/tsdf_maplowp.h has the contract): the float32 AABB of every valid pixel's point under the frame's forward map,
    the float32 glue and the degenerate rule.  ``max_l`` / ``mid_p`` / ``status`` are those of :func:`voxelize_aug`, bit for
    bit; ``grid`` goes straight to :func:`voxelize_map_grid_lowp` or :func:`voxelize_aug_grid`.

    depth / offsets / headers   the n_src source frames, as for :func:`voxelize`
    xforms  float64[n,24] on the GPU: one map per BATCH POSITION, forward rows then inverse rows
    index   optional int64[n] on the GPU: batch position i places source frame index[i] (repeats allowed; an entry
            outside [0, n_src) gives that position status 2).  Without it the batch is the n_src frames
    out     optional preallocated :class:`MapGridBatch` to write into
    A position that is not OK gets an all-zero grid row and ``max_l`` 0.  One launch on the current stream, no
    synchronisation."""
    M = _lib.load_maplowp()
    dev, n_src, n, R = _source(depth, offsets, headers, index, res, "czyx")
    _shaped("xforms", xforms, (n, 24), torch.float64, dev)
    out = _outs(MapGridBatch, out, _placement_fields(n), dev)
    if n:
        _call(dev, M.tsdf_map_place_hip,
              _src_head(depth, offsets, headers, n_src, index, n, R) +
              [_cam(cam), None, xforms.data_ptr(), out.grid.data_ptr(), out.max_l.data_ptr(), out.mid_p.data_ptr(),
               out.status.data_ptr()], 9)
    return out


def _map_grid_lowp(depth, offsets, headers, xforms, grid, res, layout, dtype, cam, index, out, want_status):
    """:func:`voxelize_map_grid_lowp`; without ``want_status`` the launch writes no status and, given ``out``, the call
    allocates nothing.  Returns (volume, status or None)."""
    code = _lowp_dtype(dtype)
    M = _lib.load_maplowp()
    dev, n_src, n, R = _source(depth, offsets, headers, index, res, layout)
    _shaped("xforms", xforms, (n, 24), torch.float64, dev)
    _shaped("grid", grid, (n, 8), torch.float32, dev)
    tsdf = _out("out", out, (n, 3, R, R, R), dtype, dev)
    status = _out("status", None, (n,), torch.int32, dev) if want_status else None
    if n:
        _call(dev, M.tsdf_voxelize_map_grid_lowp_hip,
              _src_head(depth, offsets, headers, n_src, index, n, R) +
              [_cam(cam), _lib.LAYOUTS[layout], code, None, xforms.data_ptr(), grid.data_ptr(), tsdf.data_ptr(), _ptr(status)], 11)
    return tsdf, status


def voxelize_map_grid_lowp(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, xforms: torch.Tensor,
                           grid: torch.Tensor, res: int = 32, layout: str = "czyx", dtype: torch.dtype = torch.bfloat16,
                           cam: Optional[_lib.TsdfCam] = None, index: Optional[torch.Tensor] = None,
                           out: Optional[torch.Tensor] = None):
    """:func:`voxelize_aug_grid` written as float16 / bfloat16 voxels (``tsdf_voxelize_map_grid_lowp_hip`` of
    libtsdf_maplowp.so; include/tsdf_maplowp.h has the contract): every voxel is the float32 value of the augmented pass
    narrowed by round-to-nearest-even in registers, so the volume is written once, at half the bytes.

    depth / offsets / headers   the n_src source frames, as for :func:`voxelize`
    xforms  float64[n,24] on the GPU  }  per BATCH POSITION: position i voxelizes its source frame under map i on row i
    grid    float32[n,8] on the GPU   }  (vox_ori[3], voxel_len, trunc_dis, 3 pad words: what :func:`map_grids` returns)
    dtype   torch.float16 or torch.bfloat16
    index   optional int64[n] on the GPU: batch position i voxelizes source frame index[i] (repeats allowed; an entry
            outside [0, n_src) gives that position status 2 and a zero volume).  Without it the batch is the n_src frames
    out     optional preallocated ``dtype[n,3,R,R,R]`` (a contiguous view of a larger buffer will do) to write into
    Returns ``(tsdf dtype[n,3,R,R,R], status int32[n])``.  A bad header (2) or an unusable grid row (1) gives a zero volume;
    the crop is not scanned, so a frame without a valid pixel on a usable row gets a zero volume with status 0.  One launch
    on the current stream, no synchronisation."""
    return _map_grid_lowp(depth, offsets, headers, xforms, grid, res, layout, dtype, cam, index, out, True)


def _batch_labels(gt, index, n_src, xforms, max_l, mid_p, clamp, sel=None, out_aug=None, out_nor=None):
    """The labels of a batch under its maps: the batch's joints (``index``: gathered from the n_src source frames, an
    entry outside them reads the nearest frame and its position is not OK anyway), :func:`transform_joints`, then
    :func:`normalize_joints` in the mapped grid.  Returns (gt_nor, gt_aug)."""
    if index is not None:
        safe = index.clamp(0, n_src - 1) if sel is None else torch.clamp(index, 0, n_src - 1, out=sel[0])
        gt = gt.index_select(0, safe) if sel is None else torch.index_select(gt, 0, safe, out=sel[1])
    gt_aug = transform_joints(gt, xforms, out=out_aug)
    return normalize_joints(gt_aug, max_l, mid_p, clamp=clamp, out=out_nor), gt_aug


def _aug_placed(depth, offsets, headers, xforms, res, cam, gt, clamp, index, volume):
    """What :func:`voxelize_aug_lowp` and :func:`voxelize_aug_accurate` are around their pass: :func:`map_grids` places the
    grid under the maps, ``volume(rows)`` is the pass on the placement's rows, the batch has the PLACEMENT's ``max_l`` /
    ``mid_p`` / ``status``, and with ``gt`` the labels follow (:func:`_batch_labels`): ``(TsdfBatch, gt_nor, gt_aug)``."""
    mg = map_grids(depth, offsets, headers, xforms, res=res, cam=cam, index=index)
    batch = TsdfBatch(volume(mg.grid), mg.max_l, mg.mid_p, mg.status)
    if gt is None:
        return batch
    _dev_check("gt", gt, torch.float32, depth.device)
    gt_nor, gt_aug = _batch_labels(gt, index, headers.shape[0], xforms, mg.max_l, mg.mid_p, clamp)
    return batch, gt_nor, gt_aug


def voxelize_aug_lowp(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, xforms: torch.Tensor,
                      res: int = 32, layout: str = "czyx", dtype: torch.dtype = torch.bfloat16,
                      cam: Optional[_lib.TsdfCam] = None, gt: Optional[torch.Tensor] = None, clamp: bool = True,
                      index: Optional[torch.Tensor] = None):
    """:func:`voxelize_aug` with a float16 / bfloat16 volume: :func:`map_grids` places the grid under the maps and
    :func:`voxelize_map_grid_lowp` writes the volume on its rows, on one stream with nothing on the host in between.  It
    is TWO launches and the crop is read twice (the fused float32 entry reads it once).  ``max_l`` / ``mid_p`` / ``status``
    are the placement's, bit for bit those of :func:`voxelize_aug`; ``tsdf`` is ``dtype[n,3,R,R,R]``.

    xforms  float64[n,24] on the GPU, one map per batch position; ``index`` (int64[n] on the GPU) draws the batch from the
            source frames as for :func:`voxelize_map_grid_lowp`
    gt      optional float32[n_src,3J] (or [n_src,J,3]) on the GPU: returns ``(TsdfBatch, gt_nor, gt_aug)`` with
            ``gt_aug = transform_joints(gt of the batch, xforms)`` and ``gt_nor = normalize_joints(gt_aug, max_l, mid_p)``
            (two more small launches), the values the fused entry writes."""
    _lowp_dtype(dtype)
    return _aug_placed(depth, offsets, headers, xforms, res, cam, gt, clamp, index, lambda rows: _map_grid_lowp(
        depth, offsets, headers, xforms, rows, res, layout, dtype, cam, index, None, False)[0])


def _map_grid_accurate(depth, offsets, headers, xforms, grid, res, layout, cam, index, out, want_status, nearest=False):
    """:func:`voxelize_map_grid_accurate`; without ``want_status`` the launch writes no status and, given ``out`` (and no
    ``nearest``), the call allocates nothing.  Returns (volume, status or None, nearest or None)."""
    A = _lib.load_mapaccurate()
    dev, n_src, n, R = _source(depth, offsets, headers, index, res, layout)
    _shaped("xforms", xforms, (n, 24), torch.float64, dev)
    _shaped("grid", grid, (n, 8), torch.float32, dev)
    tsdf = _out("out", out, (n, 3, R, R, R), torch.float32, dev)
    status = _out("status", None, (n,), torch.int32, dev) if want_status else None
    near = _out("nearest", None, (n, R, R, R), torch.int32, dev) if nearest else None
    if n:
        _call(dev, A.tsdf_voxelize_map_grid_accurate_hip,
              _src_head(depth, offsets, headers, n_src, index, n, R) + _cam5(cam) +
              [_lib.LAYOUTS[layout], None, xforms.data_ptr(), grid.data_ptr(), tsdf.data_ptr(), _ptr(near), _ptr(status)], 14)
    return tsdf, status, near


def voxelize_map_grid_accurate(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, xforms: torch.Tensor,
                               grid: torch.Tensor, res: int = 32, layout: str = "czyx",
                               cam: Optional[_lib.TsdfCam] = None, index: Optional[torch.Tensor] = None,
                               out: Optional[torch.Tensor] = None, nearest: bool = False):
    """The ACCURATE directional TSDF under per-frame maps, on a caller-supplied grid (``tsdf_voxelize_map_grid_accurate_hip``
    of libtsdf_mapaccurate.so; include/tsdf_mapaccurate.h has the contract): per voxel the nearest MAPPED surface point
    among ALL valid pixels of the crop, where :func:`voxelize_aug_grid` takes the one pixel the voxel projects to and
    rejects the voxel when that pixel is empty.  It is :func:`voxelize_grid_accurate`'s search on
    :func:`voxelize_aug_grid`'s arithmetic: a voxel whose nearest pixel is its projected one has the projective pass's bits,
    a voxel with no mapped point within the truncation distance keeps the projective value.

    depth / offsets / headers   the n_src source frames, as for :func:`voxelize`
    xforms  float64[n,24] on the GPU  }  per BATCH POSITION: position i voxelizes its source frame under map i on row i
    grid    float32[n,8] on the GPU   }  (vox_ori[3], voxel_len, trunc_dis, 3 pad words: what :func:`map_grids` returns)
    cam     a :class:`TsdfCam` or None (the MSRA defaults); its five constants go to the entry by value
    index   optional int64[n] on the GPU: batch position i voxelizes source frame index[i] (repeats allowed; an entry
            outside [0, n_src) gives that position status 2 and a zero volume).  Without it the batch is the n_src frames
    out     optional preallocated ``float32[n,3,R,R,R]`` (a contiguous view of a larger buffer will do) to write into
    nearest True: also ``int32[n,R,R,R]``, per voxel the row-major crop index of its nearest pixel, -1 for a far voxel,
            in the index order of one channel of the volume
    Returns ``(tsdf float32[n,3,R,R,R], status int32[n])``, with ``nearest`` a third tensor.  A bad header (2) or an
    unusable grid row (1) gives a zero volume; a frame without a valid pixel gets a zero volume with status 0.  Only the
    forward rows of a map enter the distances and the search window; the inverse rows serve the projection that gives the
    sign.  One launch on the current stream, no synchronisation.  Float32 only: :func:`narrow_volumes` follows where
    2-byte voxels are wanted (the pass is bound by its search, not by its stores)."""
    tsdf, status, near = _map_grid_accurate(depth, offsets, headers, xforms, grid, res, layout, cam, index, out, True, nearest)
    return (tsdf, status, near) if nearest else (tsdf, status)


def voxelize_aug_accurate(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, xforms: torch.Tensor,
                          res: int = 32, layout: str = "czyx", dtype: Optional[torch.dtype] = None,
                          cam: Optional[_lib.TsdfCam] = None, gt: Optional[torch.Tensor] = None, clamp: bool = True,
                          index: Optional[torch.Tensor] = None):
    """:func:`voxelize_aug` with the accurate directional TSDF: :func:`map_grids` places the grid under the maps and
    :func:`voxelize_map_grid_accurate` writes the volume on its rows, on one stream with nothing on the host in between;
    with ``dtype`` (torch.float16 / torch.bfloat16) :func:`narrow_volumes` follows and ``tsdf`` has that type.
    ``max_l`` / ``mid_p`` / ``status`` are the placement's, bit for bit those of :func:`voxelize_aug`.

    xforms  float64[n,24] on the GPU, one map per batch position; ``index`` (int64[n] on the GPU) draws the batch from the
            source frames as for :func:`voxelize_map_grid_accurate`
    gt      optional float32[n_src,3J] (or [n_src,J,3]) on the GPU: returns ``(TsdfBatch, gt_nor, gt_aug)`` as
            :func:`voxelize_aug_lowp` does, the values the fused projective entry writes."""
    if dtype is not None:
        _lowp_dtype(dtype)

    def volume(rows):
        tsdf = _map_grid_accurate(depth, offsets, headers, xforms, rows, res, layout, cam, index, None, False)[0]
        return tsdf if dtype is None else narrow_volumes(tsdf, dtype=dtype)
    return _aug_placed(depth, offsets, headers, xforms, res, cam, gt, clamp, index, volume)


def compose_xforms(outer: torch.Tensor, inner: torch.Tensor, index: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Two sets of per-frame maps composed into one (``tsdf_compose_xforms_hip`` of libtsdf_mapstep.so;
    include/tsdf_mapstep.h has the contract): ``out[i] = outer[i] o inner[g]``, the map that applies ``inner[g]`` first and
    ``outer[i]`` second, ``g = index[i]`` (without ``index``: ``i``).  The forward rows are composed in that order and the
    inverse rows the other way round, in float64 with every product and sum rounded on its own; no matrix is inverted.

    outer   float64[n,24] on the GPU: one map per batch position (an augmentation: :func:`aug_xforms_at`)
    inner   float64[N,24] on the GPU: one map per source frame (a principal-axis map: :func:`obb_xforms`)
    index   optional int64[n] on the GPU; without it N must equal n.  An entry outside [0, N) gives ``out[i] = outer[i]``
    out     optional float64[n,24] to write into (it is returned; it may be ``outer``)
    One small launch on the current stream, no synchronisation."""
    S = _lib.load_mapstep()
    _dev_check("outer", outer, torch.float64)
    dev = outer.device
    if outer.dim() != 2 or outer.shape[1] != 24:
        raise ValueError("outer must have shape [n, 24] (forward rows then inverse rows)")
    n = outer.shape[0]
    _dev_check("inner", inner, torch.float64, dev)
    if inner.dim() != 2 or inner.shape[1] != 24:
        raise ValueError("inner must have shape [N, 24] (forward rows then inverse rows)")
    n_inner = inner.shape[0]
    if index is not None:
        _shaped("index", index, (n,), torch.int64, dev)
        if n and not n_inner:
            raise ValueError("index needs at least one inner map")
    elif n_inner != n:
        raise ValueError("without index, inner must hold one map per map of outer")
    out = _out("out", out, (n, 24), torch.float64, dev)
    if n:
        _call(dev, S.tsdf_compose_xforms_hip, [outer.data_ptr(), inner.data_ptr(), n_inner, _ptr(index), n, None,
                                               out.data_ptr()], 5)
    return out


class MapStepBatch(NamedTuple):
    xforms: torch.Tensor             # float64[n, 24]  the map of every batch position: the draw, composed with its base
    grid: Optional[torch.Tensor]     # float32[n, 8]   the placement's rows (None with place=False, as the three below)
    max_l: Optional[torch.Tensor]    # float32[n]      in the mapped frame
    mid_p: Optional[torch.Tensor]    # float32[n, 3]
    status: Optional[torch.Tensor]   # int32[n]  (_lib.TSDF_FRAME_*)
    gt_aug: Optional[torch.Tensor]   # the batch's joints under the maps (None without gt)
    gt_nor: Optional[torch.Tensor]   # their labels in the mapped grid


def map_step_head(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, centres: torch.Tensor,
                  state: torch.Tensor, *, base: Optional[torch.Tensor] = None, index: Optional[torch.Tensor] = None,
                  counters: Optional[torch.Tensor] = None, gt: Optional[torch.Tensor] = None, res: int = 32,
                  cam: Optional[_lib.TsdfCam] = None, clamp: bool = True, place: bool = True,
                  out: Optional[MapStepBatch] = None, return_params: bool = False):
    """Everything the augmented step does before its voxel pass, in ONE launch (``tsdf_map_step_head_hip`` of
    libtsdf_mapstep.so; include/tsdf_mapstep.h has the contract): the draw of :func:`aug_xforms_at`, its composition with
    the source frame's ``base`` map (:func:`compose_xforms`), the grid placement of :func:`map_grids` under the result and
    the batch's labels (:func:`transform_joints`, :func:`normalize_joints`) — every output bit for bit what that chain of
    five or six launches writes.

    depth / offsets / headers   the N source frames, as for :func:`voxelize`
    centres   float32[N,3] on the GPU: the centre each frame's augmentation turns about, in the frame the volume is cut in
    state     int64[2] on the GPU: ``{key, counter0}``, read by the kernel (:func:`aug_state`)
    base      optional float64[N,24] on the GPU: one map per SOURCE frame (``obb_xforms(...).xforms``); position i is
              voxelized under ``draw_i o base[index[i]]``
    index, counters   optional int64[n] (device or page-locked host memory), as for :func:`aug_xforms_at`
    gt        optional float32[N,3J] (or [N,J,3]) on the GPU: the joints of every source frame (needs ``place``)
    place     False: the maps alone — the depth is not read, and ``grid`` / ``max_l`` / ``mid_p`` / ``status`` are None
    out       optional preallocated :class:`MapStepBatch` to write into (fields that the call does not write are ignored)
    Returns :class:`MapStepBatch`, or with ``return_params`` ``(MapStepBatch, stretch float64[n], rot int32[n,2])``.
    ``xforms`` and ``grid`` go straight to :func:`voxelize_map_grid_lowp`, ``xforms`` alone to :func:`voxelize_indexed`."""
    S = _lib.load_mapstep()
    dev, n_src, R = _pack(_lib.load(), depth, offsets, headers, res)
    _, n_c, n, xf, stretch, rot = _draw_args(centres, None, index, counters, out.xforms if out is not None else None,
                                             return_params, state)
    if centres.device != dev:
        raise ValueError(f"centres is on {centres.device}, expected {dev}")
    if n_c != n_src:
        raise ValueError("centres must hold one centre per source frame: [N, 3]")
    if base is not None:
        _shaped("base", base, (n_src, 24), torch.float64, dev)
    grid = max_l = mid_p = status = gt_aug = gt_nor = None
    nj = 0
    if place:
        grid, max_l, mid_p, status = _each(out, _placement_fields(n), dev)
    if gt is not None:
        if not place:
            raise ValueError("gt needs place=True (the labels are normalised in the placed grid)")
        _dev_check("gt", gt, torch.float32, dev)
        if gt.dim() < 2:
            raise ValueError("gt must hold the labels of every source frame: [N, 3*J] or [N, J, 3]")
        nj = (_coords("gt", gt, n_src) or 63) // 3
        shape = (n,) + tuple(gt.shape[1:])
        gt_aug = _out("out.gt_aug", out.gt_aug if out is not None else None, shape, torch.float32, dev)
        gt_nor = _out("out.gt_nor", out.gt_nor if out is not None else None, shape, torch.float32, dev)
    if n:
        _call(dev, S.tsdf_map_step_head_hip,
              _src_head(depth, offsets, headers, n_src, index, n, R) + _cam5(cam) +
              [centres.data_ptr(), _ptr(base), state.data_ptr(), _ptr(counters), _ptr(gt), nj, 1 if clamp else 0, None,
               xf.data_ptr(), _ptr(grid), _ptr(max_l), _ptr(mid_p), _ptr(status), _ptr(gt_aug), _ptr(gt_nor), _ptr(stretch),
               _ptr(rot)], 20)
    batch = MapStepBatch(xf, grid, max_l, mid_p, status, gt_aug, gt_nor)
    return (batch, stretch, rot) if return_params else batch


class HandCrops(NamedTuple):
    depth: torch.Tensor              # float32[capacity]  the crops packed back to back; the tail past offsets[n] is unwritten
    offsets: torch.Tensor            # int64[n + 1]
    headers: torch.Tensor            # int32[n, 6]     W, H, left, top, right, bottom
    com: torch.Tensor                # float64[n, 3]   the centre c of the cube, camera frame, mm
    count: torch.Tensor              # int32[n]        pixels kept in the crop
    status: torch.Tensor             # int32[n]        0, 1 (no valid pixel), 2 (index outside the frames)
    grid: Optional[torch.Tensor]     # float32[n, 8]   the CUBE grid rows (None with grid=False, as the two below)
    max_l: Optional[torch.Tensor]    # float32[n]      cube
    mid_p: Optional[torch.Tensor]    # float32[n, 3]   float32(c)


_LOCATE_TYPES = {torch.float32: _lib.TSDF_LOCATE_F32, torch.uint16: _lib.TSDF_LOCATE_U16}


def locate_hands(frames: torch.Tensor, *, cube: float = 250.0, near: float = 100.0, far: float = 1500.0,
                 seed_band: float = 150.0, refine: int = 2, res: int = 32, cam: Optional[_lib.TsdfCam] = None,
                 shift: Optional[int] = None, index: Optional[torch.Tensor] = None, grid: bool = True,
                 out: Optional[HandCrops] = None) -> HandCrops:
    """The hand located in raw depth frames on the GPU (``tsdf_locate_hip`` of libtsdf_locate.so; include/tsdf_locate.h
    has the contract): per frame the nearest object's centre of mass — the valid pixels (finite, ``|d| >= invalid_eps``,
    ``near <= d <= far``) within ``seed_band`` mm of the nearest one —, a cube of edge ``cube`` mm about it, ``refine``
    rounds of "the centre of what is inside the cube", and the cube's pixels (everything else zeroed) packed as the
    ``depth / offsets / headers`` triple every entry here takes: :func:`voxelize`, :func:`voxelize_lowp`,
    :func:`voxelize_obb`, :func:`process_batch`, :class:`AugmentedStep`.  Nothing goes through the host.

    frames   float32[N,H,W] mm, or uint16[N,H,W] with ``shift`` (0..7): the depth is ``u * 2^-shift``, packing's encoding
    index    optional int64[n] on the GPU: batch position i is frame index[i] (outside [0, N): status 2)
    res      enters the cube grid rows alone
    grid     False: no ``grid`` / ``max_l`` / ``mid_p``
    out      optional preallocated :class:`HandCrops` to write into (capturable); ``out.depth`` must hold n times the
             capacity rule's pixels (``min(W, s) * min(H, s)``, ``s = floor(cube * focal / near) + 2``)
    A position without a valid pixel (status 1) or with a bad index (2) gets the header [W, H, 0, 0, 1, 1], one pixel of
    0 and zero rows: the voxelizers report their own status 1 for it.  ``grid`` goes to :func:`voxelize_grid`: the
    fixed-cube placement of DeepPrior++ / V2V-PoseNet, with ``max_l`` = cube and ``mid_p`` = the centre for the labels.
    Three small launches on the current stream, no synchronisation; two calls give identical bits."""
    K = _lib.load_locate()
    if not isinstance(frames, torch.Tensor):
        raise TypeError("frames must be a torch.Tensor")
    # what the frames ARE (type, shape, encoding) before where they live: each refusal names its own cause
    if frames.dtype not in _LOCATE_TYPES:
        raise TypeError(f"frames must be torch.float32 or torch.uint16, got {frames.dtype}")
    if frames.dim() != 3 or frames.shape[1] < 1 or frames.shape[2] < 1:
        raise ValueError("frames must have shape [N, H, W]")
    u16 = frames.dtype is torch.uint16
    if u16:
        if isinstance(shift, bool) or not isinstance(shift, int) or not 0 <= shift <= _lib.DEPTH16_MAX_SHIFT:
            raise ValueError(f"uint16 frames need shift, an integer in 0..{_lib.DEPTH16_MAX_SHIFT}; got {shift!r}")
    elif shift is not None:
        raise ValueError("shift belongs to uint16 frames")
    if not _lib.load().tsdf_resolution_supported(int(res)):
        raise ValueError(f"unsupported grid resolution {res} (multiple of 4 in 4..128)")
    if isinstance(refine, bool) or not isinstance(refine, int):
        raise TypeError("refine must be an integer")
    if not frames.is_contiguous():
        raise ValueError("frames must be contiguous")
    _dev_check("frames", frames, frames.dtype)
    dev = frames.device
    n_src, H, W = (int(v) for v in frames.shape)
    n = n_src if index is None else _indexed(index, n_src, dev, "index needs at least one frame")
    c5 = _cam5(cam)
    per = ctypes.c_int64(0)
    _lib.check(K.tsdf_locate_capacity(H, W, cube, near, c5[0], ctypes.byref(per)), "tsdf_locate_capacity")
    need = n * per.value
    if out is not None:
        _dev_check("out.depth", out.depth, torch.float32, dev)
        if out.depth.dim() != 1 or out.depth.numel() < need:
            raise ValueError(f"out.depth must be a vector of at least {need} elements ({n} frames of {per.value})")
        depth = out.depth
    else:
        depth = torch.empty((need,), dtype=torch.float32, device=dev)
    if n == 0:
        offsets = torch.zeros((1,), dtype=torch.int64, device=dev) if out is None else \
            _shaped("out.offsets", out.offsets, (1,), torch.int64, dev).zero_()
    else:
        offsets = _out("out.offsets", getattr(out, "offsets", None), (n + 1,), torch.int64, dev)
    fields = (("headers", (n, 6), torch.int32), ("com", (n, 3), torch.float64), ("count", (n,), torch.int32),
              ("status", (n,), torch.int32)) + (_placement_fields(n)[:3] if grid else ())
    headers, com, count, status, *cube_rows = _each(out, fields, dev)
    g, max_l, mid_p = cube_rows or (None, None, None)
    if n:
        _call(dev, K.tsdf_locate_hip,
              [frames.data_ptr(), _LOCATE_TYPES[frames.dtype], shift if u16 else 0, n_src, H, W, _ptr(index), n, near, far, cube,
               seed_band, refine, int(res), *c5, depth.numel(), None, depth.data_ptr(), offsets.data_ptr(), headers.data_ptr(),
               com.data_ptr(), count.data_ptr(), status.data_ptr(), _ptr(g), _ptr(max_l), _ptr(mid_p)], 20)
    return HandCrops(depth, offsets, headers, com, count, status, g, max_l, mid_p)


def voxelize_frames(frames: torch.Tensor, res: int = 32, *, placement: str = "aabb", dtype: Optional[torch.dtype] = None,
                    gt: Optional[torch.Tensor] = None, layout: str = "czyx", tsdf: str = "projective", **locate):
    """Raw depth frames to volumes: :func:`locate_hands` chained into the existing voxelizers on one stream, nothing on
    the host in between.  Returns ``(TsdfBatch, HandCrops)``, or with ``gt`` (float32[n,3J] or [n,J,3] on the GPU, the
    joints of every batch position, camera frame) ``(TsdfBatch, HandCrops, gt_nor)``.

    placement   "aabb": the grid on the located cloud's extremes, as the reference places it — :func:`voxelize` /
                :func:`voxelize_labels` (``dtype=None``) or :func:`voxelize_lowp`; the volumes, ``max_l`` and ``mid_p`` are
                exactly what those entries give for the located pack.
                "cube": the grid on the located cube — :func:`voxelize_grid` or :func:`voxelize_grid_lowp` on
                ``HandCrops.grid``; ``max_l`` / ``mid_p`` of the batch are the cube's (its edge and centre), so a frame's
                scale does not move with a finger, and the labels are ``normalize_joints(gt, max_l, mid_p)``.
    dtype       None (float32 volumes), torch.float16 or torch.bfloat16
    tsdf        "projective" (default: the entries above) or "accurate": the volumes are the accurate directional TSDF
                (:func:`voxelize_grid_accurate`) on the same placement — the AABB's rows or the cube's —, followed by
                :func:`narrow_volumes` with ``dtype``; ``max_l`` / ``mid_p`` / ``status`` and the labels do not change.
    **locate    :func:`locate_hands`' keywords (``cube``, ``near``, ``far``, ``seed_band``, ``refine``, ``cam``, ``shift``,
                ``index``, ``out``); ``cam`` goes to the voxelizer as well."""
    if placement not in ("aabb", "cube"):
        raise ValueError("placement must be 'aabb' or 'cube'")
    if layout not in _lib.LAYOUTS:
        raise ValueError("layout must be 'czyx' or 'cxyz'")
    if dtype is not None:
        _lowp_dtype(dtype)
    _tsdf_kind(tsdf)
    if "grid" in locate or "res" in locate:
        raise TypeError("voxelize_frames sets locate_hands' grid and res itself")
    cam = locate.get("cam")
    crops = locate_hands(frames, res=res, grid=placement == "cube", **locate)
    d, o, h = crops.depth, crops.offsets, crops.headers
    gt_nor = None
    how = dict(res=res, layout=layout, cam=cam)
    if placement == "cube":     # the cube's rows, and the status the PASS gives them
        vol, st = _grid_pass(d, o, h, crops.grid, dtype=dtype, tsdf=tsdf, **how)
        batch = TsdfBatch(vol, crops.max_l, crops.mid_p, st)
    elif dtype is not None or tsdf != "projective":
        batch = _placed_pass(d, o, h, _place_aabb(d, o, h, res, cam), dtype=dtype, tsdf=tsdf, **how)
    elif gt is not None:        # float32 projective on the AABB is the fused entry: one launch, not place plus pass
        batch, gt_nor = voxelize_labels(d, o, h, gt, **how)
    else:
        batch = voxelize(d, o, h, **how)
    if gt is None:
        return batch, crops
    if gt_nor is None:
        gt_nor = normalize_joints(gt, batch.max_l, batch.mid_p)
    return batch, crops, gt_nor


_HEAT_DTYPES = {torch.float32: _lib.TSDF_HEATMAP_F32, **_LOWP_DTYPES}


def _heat_dtype(dtype) -> int:
    """The dtype code of include/tsdf_heatmap.h of a torch dtype; anything but float32 / float16 / bfloat16 is a ValueError."""
    code = _HEAT_DTYPES.get(dtype) if isinstance(dtype, torch.dtype) else None
    if code is None:
        raise ValueError(f"dtype must be torch.float32, torch.float16 or torch.bfloat16, got {dtype!r}")
    return code


def _heat_res(res) -> int:
    """``res`` as an int the library voxelizes at (the rule of :func:`_pack`), else a ValueError."""
    try:
        ok = _lib.load().tsdf_resolution_supported(int(res))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"unsupported grid resolution {res!r} (multiple of 4 in 4..128)")
    return int(res)


def _heat_sigma(sigma) -> float:
    """``sigma`` as the float32 the entry takes: finite and > 0 as that float32, else a ValueError."""
    try:
        s = ctypes.c_float(sigma).value
    except TypeError:
        s = float("nan")
    if not 0.0 < s < float("inf"):
        raise ValueError(f"sigma must be a finite number > 0 (in voxels, as a float32), got {sigma!r}")
    return s


def _heat_layout(layout) -> int:
    if layout not in _lib.LAYOUTS:
        raise ValueError("layout must be 'czyx' or 'cxyz'")
    return _lib.LAYOUTS[layout]


def joint_heatmaps(gt_nor: torch.Tensor, res: int = 32, sigma: float = 1.7, layout: str = "czyx",
                   dtype: torch.dtype = torch.float32, status: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, return_valid: bool = False):
    """One Gaussian volume per joint, aligned voxel for voxel with the TSDF volume of the same frame at resolution ``res``
    (``tsdf_joint_heatmaps_hip`` of libtsdf_heatmap.so; include/tsdf_heatmap.h has the contract): the target of a
    voxel-to-voxel network, written once by one launch.

    gt_nor   float32[n,3J] or [n,J,3] on the GPU: the normalised labels ``(gt - mid_p) / max_l + 0.5`` — ``gt_nor`` of every
             entry that writes labels, of :func:`normalize_joints` and of :class:`AugmentedStep`.  A joint sits at voxel
             coordinate ``u * res - 0.5`` under every placement and every per-frame map, so the grid is not an argument
    sigma    the Gaussian's standard deviation in voxels of this grid; the peak is 1, there is no truncation window
    layout   the last three axes are z, y, x ("czyx") or x, y, z ("cxyz"): the volume's own
    dtype    torch.float32, torch.float16 or torch.bfloat16 (the float32 value narrowed by round-to-nearest-even)
    status   optional int32[n] on the GPU (a voxelizer's): the joints of a frame whose status is not 0 get zero volumes
    out      optional preallocated ``dtype[n,J,res,res,res]`` to write into (it is returned); every byte is written
    Returns ``heat``, or ``(heat, valid int32[n,J])`` with ``return_valid``: 0 for a joint with a non-finite coordinate or of
    a frame with a non-zero status (its volume is zero), else 1 — a joint outside the cube is valid and gets its tail.
    One launch on the current stream, no synchronisation."""
    R, s, lay, code = _heat_res(res), _heat_sigma(sigma), _heat_layout(layout), _heat_dtype(dtype)
    _dev_check("gt_nor", gt_nor, torch.float32)
    if gt_nor.dim() < 2:
        raise ValueError("gt_nor must have shape [n, 3*J] or [n, J, 3]")
    dev, n = gt_nor.device, gt_nor.shape[0]
    J = (_coords("gt_nor", gt_nor, n) or math.prod(gt_nor.shape[1:])) // 3   # (n == 0: nothing to count, J by the shape)
    if status is not None:
        _shaped("status", status, (n,), torch.int32, dev)
    heat = _out("out", out, (n, J, R, R, R), dtype, dev)
    valid = _out("valid", None, (n, J), torch.int32, dev) if return_valid else None
    if n:
        _call(dev, _lib.load_heatmap().tsdf_joint_heatmaps_hip,
              [gt_nor.data_ptr(), _ptr(status), n, J, R, s, lay, code, None, heat.data_ptr(), _ptr(valid)], 8)
    return (heat, valid) if return_valid else heat


class HeatmapJoints(NamedTuple):
    u: torch.Tensor      # float32[n,J,3]  normalised coordinates, columns x, y, z
    peak: torch.Tensor   # float32[n,J]    the maximum of the joint's volume
    arg: torch.Tensor    # int32[n,J]      its linear index within the volume, in memory order (-1: every value is a NaN)


def heatmap_joints(heat: torch.Tensor, layout: str = "czyx", radius: int = 0,
                   out: Optional[HeatmapJoints] = None) -> HeatmapJoints:
    """Per joint the peak of a (predicted) heatmap volume as normalised coordinates (``tsdf_heatmap_joints_hip`` of
    libtsdf_heatmap.so; include/tsdf_heatmap.h has the contract) — what :func:`denormalize_joints`,
    ``transform_joints(..., invert_xforms(...))`` and :func:`pose_error` take.

    heat     float32 / float16 / bfloat16 ``[n,J,R,R,R]`` on the GPU in ``layout``, R a multiple of 4 in 4..128
    radius   0: the centre of the maximal voxel.  1..3: the centre of mass of ``max(h, 0)`` over the (2·radius+1)³ window
             about it, clipped to the grid (the maximal voxel's centre where that mass is not a finite number > 0)
    out      optional preallocated :class:`HeatmapJoints` to write into (it is returned)
    The maximum is taken with ``>``: a NaN is never it, ties go to the lowest index in memory.  A volume of NaNs alone gives
    ``arg`` -1, ``peak`` NaN and ``u`` 0.5.  One launch on the current stream, no synchronisation."""
    lay = _heat_layout(layout)
    if not isinstance(radius, int) or isinstance(radius, bool) or not 0 <= radius <= 3:
        raise ValueError(f"radius must be 0, 1, 2 or 3, got {radius!r}")
    if not isinstance(heat, torch.Tensor):
        raise TypeError("heat must be a torch.Tensor")
    code = _heat_dtype(heat.dtype)
    _dev_check("heat", heat, heat.dtype)
    if heat.dim() != 5 or heat.shape[2] != heat.shape[3] or heat.shape[3] != heat.shape[4]:
        raise ValueError("heat must have shape [n, J, R, R, R]")
    n, J, R = heat.shape[0], heat.shape[1], _heat_res(heat.shape[2])
    if not 1 <= J <= 170:
        raise ValueError("heat must hold 1..170 joints per frame")
    dev = heat.device
    res = _outs(HeatmapJoints, out, (("u", (n, J, 3), torch.float32), ("peak", (n, J), torch.float32),
                                     ("arg", (n, J), torch.int32)), dev)
    if n:
        _call(dev, _lib.load_heatmap().tsdf_heatmap_joints_hip,
              [heat.data_ptr(), code, n, J, R, lay, radius, None, res.u.data_ptr(), res.peak.data_ptr(), res.arg.data_ptr()], 7)
    return res


def _heat_tensor(name, t, dtype, dev, shape=None):
    """An argument of the loss entries whose data pointer goes straight to a kernel: every defect is a ValueError."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (there is no CPU path); got device {t.device}")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name} is on {t.device}, expected {dev}")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != shape:
        raise ValueError(f"{name} must have shape {shape}")
    return t


def _heat_volume(name, t):
    """A volume ``[n,J,R,R,R]`` as libtsdf_heatloss.so reads it, in its own dtype: ``(dtype code, n, J, R)``."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch.Tensor")
    code = _heat_dtype(t.dtype)
    _heat_tensor(name, t, t.dtype, None)
    if t.dim() != 5 or t.shape[2] != t.shape[3] or t.shape[3] != t.shape[4]:
        raise ValueError(f"{name} must have shape [n, J, R, R, R]")
    n, J, R = t.shape[0], t.shape[1], _heat_res(t.shape[2])
    if not 1 <= J <= 170:
        raise ValueError(f"{name} must hold 1..170 joints per frame")
    if n * J >= 1 << 24:
        raise ValueError(f"{name} must hold fewer than 2^24 (frame, joint) pairs")
    if t.data_ptr() % 16:
        raise ValueError(f"{name} must be 16-byte aligned")
    return code, n, J, R


_HEAT_REDUCTIONS = ("mean", "sum", "none")


def _heat_reduce(sse, valid, R, reduction):
    """``(loss, factor)`` of the per-unit float64 ``sse`` and int32 ``valid``, both ``[n,J]``: the reduced loss in float64 and
    the float64 ``[n,J]`` factor that turns the loss's upstream gradient into the gradient kernel's per-unit ``w``
    (``d loss / d pred = factor * (pred - target)``).  Torch ops on the device; an invalid unit's sse is 0 already."""
    r3 = float(R) ** 3
    ok = valid.to(torch.float64)
    if reduction == "mean":       # over the voxels of the valid units; 0 when there is none (sse and valid are all 0 then)
        denom = (ok.sum() * r3).clamp_min(1.0)
        return sse.sum() / denom, (2.0 * ok) / denom
    if reduction == "sum":
        return sse.sum(), 2.0 * ok
    return sse / r3, (2.0 * ok) / r3


class _HeatSse(torch.autograd.Function):
    """``heatmap_mse_loss`` once its arguments are judged: tsdf_heat_sse_hip, the reduction; tsdf_heat_sse_grad_hip."""

    @staticmethod
    def forward(ctx, pred, gt_nor, status, sigma, lay, reduction, shape):
        code, n, J, R = shape
        dev = pred.device
        sse = torch.empty((n, J), dtype=torch.float64, device=dev)
        valid = torch.empty((n, J), dtype=torch.int32, device=dev)
        if n:
            _call(dev, _lib.load_heatloss().tsdf_heat_sse_hip,
                  [pred.data_ptr(), code, gt_nor.data_ptr(), _ptr(status), n, J, R, sigma, lay, None, sse.data_ptr(),
                   valid.data_ptr()], 9)
        loss, factor = _heat_reduce(sse, valid, R, reduction)
        ctx.save_for_backward(pred, gt_nor, status, factor)
        ctx.heat = (sigma, lay, shape)
        return loss.to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        pred, gt_nor, status, factor = ctx.saved_tensors
        sigma, lay, (code, n, J, R) = ctx.heat
        w = (grad_out.to(torch.float64) * factor).to(torch.float32).contiguous()
        grad = torch.empty_like(pred)
        if n:
            _call(pred.device, _lib.load_heatloss().tsdf_heat_sse_grad_hip,
                  [pred.data_ptr(), code, gt_nor.data_ptr(), _ptr(status), w.data_ptr(), n, J, R, sigma, lay, None,
                   grad.data_ptr()], 10)
        return grad, None, None, None, None, None, None


def heatmap_mse_loss(pred: torch.Tensor, gt_nor: torch.Tensor, sigma: float = 1.7, layout: str = "czyx",
                     status: Optional[torch.Tensor] = None, reduction: str = "mean") -> torch.Tensor:
    """The squared error of predicted heatmap volumes against the Gaussian targets of :func:`joint_heatmaps` — without the
    targets in memory: ``((pred - joint_heatmaps(gt_nor, R, sigma, layout, status=status)) ** 2)`` reduced, as a
    ``torch.autograd.Function`` over ``tsdf_heat_sse_hip`` / ``tsdf_heat_sse_grad_hip`` of libtsdf_heatloss.so
    (include/tsdf_heatloss.h has the contract).  Every target voxel is regenerated from the label in the kernel, bit for
    bit the encode's float32; differences, squares and sums are float64.

    pred       float32 / float16 / bfloat16 ``[n,J,R,R,R]`` on the GPU in ``layout``, taken in its own dtype; the only
               argument that receives a gradient (of pred's dtype; once differentiable)
    gt_nor     float32[n,3J] or [n,J,3] on the GPU, as :func:`joint_heatmaps` takes it; it gets no gradient
    status     optional int32[n] on the GPU (a voxelizer's)
    reduction  "mean": the sum over the valid units divided by (their count · R³), 0 when no unit is valid; "sum"; or
               "none": float32[n,J], every unit's own mean
    A unit with a non-finite label or of a frame whose status is not 0 is invalid: it adds nothing to the loss and its
    gradient is zero.  Returns a float32 tensor.  One launch and a few small torch ops on the current stream for the
    forward, the same for the backward; no host synchronisation anywhere."""
    if reduction not in _HEAT_REDUCTIONS:
        raise ValueError(f"reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
    s, lay = _heat_sigma(sigma), _heat_layout(layout)
    shape = _heat_volume("pred", pred)
    _, n, J, _ = shape
    dev = pred.device
    _heat_tensor("gt_nor", gt_nor, torch.float32, dev)
    if tuple(gt_nor.shape) not in ((n, 3 * J), (n, J, 3)):
        raise ValueError(f"gt_nor must have shape [{n}, {3 * J}] or [{n}, {J}, 3]: the labels of pred's joints")
    if status is not None:
        _heat_tensor("status", status, torch.int32, dev, (n,))
    return _HeatSse.apply(pred, gt_nor, status, s, lay, reduction, shape)


class _SoftArgmax(torch.autograd.Function):
    """``soft_argmax_joints`` once its arguments are judged: tsdf_soft_argmax_hip; tsdf_soft_argmax_grad_hip."""

    @staticmethod
    def forward(ctx, heat, beta, lay, shape):
        code, n, J, R = shape
        dev = heat.device
        u = torch.empty((n, J, 3), dtype=torch.float32, device=dev)
        stats = torch.empty((n, J, 5), dtype=torch.float64, device=dev)
        if n:
            _call(dev, _lib.load_heatloss().tsdf_soft_argmax_hip,
                  [heat.data_ptr(), code, n, J, R, beta, lay, None, u.data_ptr(), stats.data_ptr()], 7)
        ctx.save_for_backward(heat, stats)
        ctx.heat = (beta, lay, shape)
        return u

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_u):
        heat, stats = ctx.saved_tensors
        beta, lay, (code, n, J, R) = ctx.heat
        gu = grad_u.to(torch.float32).contiguous()
        grad = torch.empty_like(heat)
        if n:
            _call(heat.device, _lib.load_heatloss().tsdf_soft_argmax_grad_hip,
                  [heat.data_ptr(), code, stats.data_ptr(), gu.data_ptr(), n, J, R, beta, lay, None, grad.data_ptr()], 9)
        return grad, None, None, None


def soft_argmax_joints(pred: torch.Tensor, beta: float = 1.0, layout: str = "czyx") -> torch.Tensor:
    """Per joint the expectation of the voxel position under ``softmax(beta * pred)`` over the whole volume, as normalised
    coordinates (integral regression): the differentiable counterpart of :func:`heatmap_joints`, a
    ``torch.autograd.Function`` over ``tsdf_soft_argmax_hip`` / ``tsdf_soft_argmax_grad_hip`` of libtsdf_heatloss.so
    (include/tsdf_heatloss.h has the contract).

    pred     float32 / float16 / bfloat16 ``[n,J,R,R,R]`` on the GPU in ``layout``, taken in its own dtype
    beta     the softmax's inverse temperature, a finite number > 0 (as a float32)
    Returns float32[n,J,3], columns x, y, z — what :func:`denormalize_joints`, :func:`transform_joints`, :func:`pose_error`
    or an L1 loss against ``gt_nor`` take — differentiable (once) in ``pred``.  Sums are float64.  A volume that holds a NaN
    or whose maximum is not finite gives NaN for its joint alone.  One launch on the current stream each way, no
    synchronisation."""
    try:
        b = ctypes.c_float(beta).value
    except TypeError:
        b = float("nan")
    if not 0.0 < b < float("inf"):
        raise ValueError(f"beta must be a finite number > 0 (as a float32), got {beta!r}")
    lay = _heat_layout(layout)
    return _SoftArgmax.apply(pred, b, lay, _heat_volume("pred", pred))


def _occ_slab(slab) -> int:
    """``slab`` as the hint the entry takes: an int >= 0 (0: the library's plan), else a ValueError."""
    if isinstance(slab, bool) or not isinstance(slab, int) or not 0 <= slab < 2 ** 31:
        raise ValueError(f"slab must be an int >= 0 (slices per workgroup; 0: the library's plan), got {slab!r}")
    return slab


def _occupancy(depth, offsets, headers, max_l, mid_p, res, layout, dtype, cam, xforms, index, out, slab, want_status):
    """:func:`occupancy_volumes`; without ``want_status`` the launch writes no status and, given ``out``, the call
    allocates nothing.  Returns (volume, status or None)."""
    R, lay, code, hint = _heat_res(res), _heat_layout(layout), _heat_dtype(dtype), _occ_slab(slab)
    O = _lib.load_occupancy()
    try:
        dev, n_src, n, R = _source(depth, offsets, headers, index, R, layout)
        _shaped("max_l", max_l, (n,), torch.float32, dev)
        _shaped("mid_p", mid_p, (n, 3), torch.float32, dev)
        if xforms is not None:
            _shaped("xforms", xforms, (n, 24), torch.float64, dev)
        occ = _out("out", out, (n, 1, R, R, R), dtype, dev)
    except TypeError as e:   # a bad argument of this entry is a ValueError whatever is wrong with it
        raise ValueError(str(e)) from None
    status = _out("status", None, (n,), torch.int32, dev) if want_status else None
    if n:
        _call(dev, O.tsdf_occupancy_hip,
              _src_head(depth, offsets, headers, n_src, index, n, R) + _cam5(cam) +
              [lay, code, hint, None, _ptr(xforms), max_l.data_ptr(), mid_p.data_ptr(), occ.data_ptr(), _ptr(status)], 16)
    return occ, status


def occupancy_volumes(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, max_l: torch.Tensor,
                      mid_p: torch.Tensor, res: int = 32, layout: str = "czyx", dtype: torch.dtype = torch.float32,
                      cam: Optional[_lib.TsdfCam] = None, xforms: Optional[torch.Tensor] = None,
                      index: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, slab: int = 0):
    """One-channel occupancy volumes, the input of V2V-PoseNet and its family: a voxel is 1 if a point of the frame's
    back-projected cloud falls inside it, else 0 (``tsdf_occupancy_hip`` of libtsdf_occupancy.so; include/tsdf_occupancy.h
    has the contract).  A scatter — every pixel is pushed into its voxel — through a bit mask in LDS, one launch.

    depth / offsets / headers   the n_src source frames, as for :func:`voxelize`
    max_l   float32[n] on the GPU   }  the cube of ANY placement, per BATCH POSITION: ``aabb``'s, ``map_grids``'s (with the
    mid_p   float32[n,3]            }  same ``xforms``), ``cloud_grids``'s, the fixed cube of a :class:`HandCrops`.  The grid
            is that cube cut into ``res`` voxels a side, whatever resolution the placement itself was asked for: an 88^3
            occupancy goes with a 32^3 TSDF of the same frame, and sits voxel for voxel on :func:`joint_heatmaps` at ``res``
    dtype   torch.float32, torch.float16 or torch.bfloat16
    cam     a :class:`TsdfCam` or None (the MSRA defaults); its five constants go to the entry by value
    xforms  optional float64[n,24] on the GPU: one map per batch position, the points are mapped before they are binned
    index   optional int64[n] on the GPU: batch position i takes source frame index[i] (repeats allowed; an entry outside
            [0, n_src) gives that position status 2 and a zero volume).  Without it the batch is the n_src frames
    out     optional preallocated ``dtype[n,1,R,R,R]`` (a contiguous view of a larger buffer will do) to write into
    slab    0, or slices of the slowest axis per workgroup (clamped to what 64 KiB of LDS hold); the result never depends
            on it
    Returns ``(occ dtype[n,1,R,R,R], status int32[n])``.  A bad header (2) or an unusable ``max_l`` / ``mid_p`` row (1:
    ``max_l`` not positive, anything non-finite) gives a zero volume; a frame without a valid pixel gets a zero volume with
    status 0.  Every bad argument is a ValueError before anything is launched.  One launch on the current stream, no
    synchronisation."""
    return _occupancy(depth, offsets, headers, max_l, mid_p, res, layout, dtype, cam, xforms, index, out, slab, True)


def voxelize_occupancy(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, res: int = 32,
                       layout: str = "czyx", dtype: torch.dtype = torch.float32, cam: Optional[_lib.TsdfCam] = None,
                       xforms: Optional[torch.Tensor] = None) -> TsdfBatch:
    """:func:`occupancy_volumes` on the cloud's own cube: :func:`aabb` places it — :func:`map_grids` under ``xforms`` —
    and the occupancy pass bins the points into ``res`` voxels a side.  Two launches, nothing on the host in between.
    ``max_l`` / ``mid_p`` / ``status`` are the placement's, bit for bit those of :func:`voxelize` (:func:`voxelize_aug`);
    ``tsdf`` holds the occupancy, ``dtype[n,1,R,R,R]``.  (For the fixed cube of :func:`locate_hands` call
    :func:`occupancy_volumes` on the :class:`HandCrops`' ``max_l`` / ``mid_p``.)"""
    _heat_res(res), _heat_layout(layout), _heat_dtype(dtype)   # judged before the placement is launched
    if xforms is None:
        place = _place_aabb(depth, offsets, headers, res, cam, rows=False)
    else:
        place = map_grids(depth, offsets, headers, xforms, res=res, cam=cam)
    occ, _ = _occupancy(depth, offsets, headers, place.max_l, place.mid_p, res, layout, dtype, cam, xforms, None, None, 0,
                        False)
    return TsdfBatch(occ, place.max_l, place.mid_p, place.status)


class FpsBatch(NamedTuple):
    points: torch.Tensor   # float32[n, M, 3]  the sampled points, in sampling order
    pixel: torch.Tensor    # int32[n, M]       each sample's rank: its index in the crop (row-major in the bbox) or its row
    radius2: Optional[torch.Tensor]   # float32[n, M]  the squared distance at which each sample was chosen (row 0: +inf)
    count: torch.Tensor    # int32[n]  candidates of the frame
    status: torch.Tensor   # int32[n]  _lib.TSDF_FRAME_*, or _lib.TSDF_FPS_FRAME_OVER_CAPACITY (3)


def _fps_points(points) -> int:
    """``points`` as the M the entries take: an int in 1..65536, else a ValueError."""
    if isinstance(points, bool) or not isinstance(points, int) or not 1 <= points <= _lib.FPS_MAX_POINTS:
        raise ValueError(f"points must be an int in 1..{_lib.FPS_MAX_POINTS}, got {points!r}")
    return points


def _fps_form(form) -> int:
    if isinstance(form, bool) or not isinstance(form, int) or form not in (0, 1):
        raise ValueError(f"form must be 0 (the library's choice) or 1 (streaming wherever a workspace allows), got {form!r}")
    return int(form)


def fps_plan(points: int = 1024, capacity: int = 0, form: int = 0) -> tuple:
    """``tsdf_fps_plan`` (host code only): ``(resident_cap, work_bytes per batch position, lds_bytes)`` of a call with
    ``points`` samples and a workspace of ``capacity`` candidates per position."""
    M, hint = _fps_points(points), _fps_form(form)
    if isinstance(capacity, bool) or not isinstance(capacity, int) or not 0 <= capacity < 2 ** 31:
        raise ValueError(f"capacity must be an int in 0..2^31-1, got {capacity!r}")
    cap, work, lds = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int()
    _lib.check(_lib.load_fps().tsdf_fps_plan(M, capacity, hint, cap, work, lds), "tsdf_fps_plan")
    return cap.value, work.value, lds.value


def _fps_out(out, n, M, dev, radius2=True) -> FpsBatch:
    """The outputs of a sampling call: allocated (``radius2``: with that field), or the caller's ``out`` validated field by
    field — a :class:`FpsBatch` whose ``radius2`` may be None, which the launch then does not write."""
    fields = (("points", (n, M, 3), torch.float32), ("pixel", (n, M), torch.int32), ("radius2", (n, M), torch.float32),
              ("count", (n,), torch.int32), ("status", (n,), torch.int32))
    if out is None:
        return FpsBatch(*[_out(name, None, shape, dtype, dev) if radius2 or name != "radius2" else None
                          for name, shape, dtype in fields])
    if not isinstance(out, FpsBatch):
        raise ValueError("out must be an FpsBatch")
    for name, shape, dtype in fields:
        if name != "radius2" or out.radius2 is not None:
            _shaped("out." + name, getattr(out, name), shape, dtype, dev)
    return out


def _fps_work(n, capacity, work, dev):
    """``(capacity, work)`` as the entries take them: (0, None) without a workspace; with ``capacity`` alone the workspace
    is allocated; a caller's ``work`` float32[n, capacity, 4] is validated (and ``capacity``, if given too, must be its)."""
    if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, int) or not 1 <= capacity < 2 ** 31):
        raise ValueError(f"capacity must be None or an int in 1..2^31-1, got {capacity!r}")
    if work is None:
        if capacity is None:
            return 0, None
        return capacity, torch.empty((n, capacity, 4), dtype=torch.float32, device=dev)
    _dev_check("work", work, torch.float32, dev)
    if work.dim() != 3 or work.shape[0] != n or work.shape[1] < 1 or work.shape[2] != 4:
        raise ValueError(f"work must have shape [{n}, capacity, 4]")
    if capacity is not None and capacity != work.shape[1]:
        raise ValueError(f"capacity {capacity} is not work's, {work.shape[1]}")
    if work.data_ptr() % 16:
        raise ValueError("work must be 16-byte aligned")
    return int(work.shape[1]), work


def _fps_crop(depth, offsets, headers, points, cam, xforms, index, capacity, work, out, form) -> FpsBatch:
    """:func:`farthest_points`; given ``out`` (and ``work``, or no ``capacity``) the call allocates nothing."""
    M, hint = _fps_points(points), _fps_form(form)
    F = _lib.load_fps()
    try:
        dev, n_src, n, _ = _source(depth, offsets, headers, index, None, "czyx")
        if xforms is not None:
            _shaped("xforms", xforms, (n, 24), torch.float64, dev)
        cap, work = _fps_work(n, capacity, work, dev)
        out = _fps_out(out, n, M, dev)
    except TypeError as e:   # a bad argument of this entry is a ValueError whatever is wrong with it
        raise ValueError(str(e)) from None
    if n:
        _call(dev, F.tsdf_fps_hip,
              _src_head(depth, offsets, headers, n_src, index, n, M) + _cam5(cam) +
              [cap, hint, None, _ptr(xforms), _ptr(work), out.points.data_ptr(), out.pixel.data_ptr(), _ptr(out.radius2),
               out.count.data_ptr(), out.status.data_ptr()], 15)
    return out


def farthest_points(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, points: int = 1024,
                    cam: Optional[_lib.TsdfCam] = None, xforms: Optional[torch.Tensor] = None,
                    index: Optional[torch.Tensor] = None, capacity: Optional[int] = None,
                    work: Optional[torch.Tensor] = None, out: Optional[FpsBatch] = None, form: int = 0) -> FpsBatch:
    """Farthest-point sampled clouds, the input of a point network (HandPointNet, Point-to-Point Regression PointNet):
    ``points`` points of each frame's back-projected cloud, each the one farthest from all chosen before it
    (``tsdf_fps_hip`` of libtsdf_fps.so; include/tsdf_fps.h has the contract).  One launch, one workgroup per frame, the
    whole chain of ``points - 1`` arg-max reductions on chip.

    depth / offsets / headers   the n_src source frames, as for :func:`voxelize`
    points  M, 1..65536.  Sample 0 is the first valid pixel of the crop; the first k rows of an M-point result ARE the
            k-point result, so the 1024 / 512 / 128 hierarchy of a point network is ``fps.points[:, :512]`` ...
    cam     a :class:`TsdfCam` or None (the MSRA defaults); its five constants go to the entry by value
    xforms  optional float64[n,24] on the GPU: one map per batch position; the points are mapped in float64, rounded once
            to float32 and sampled in the mapped frame
    index   optional int64[n] on the GPU: batch position i takes source frame index[i] (repeats allowed; an entry outside
            [0, n_src) gives that position status 2).  Without it the batch is the n_src frames
    capacity  None: the resident form only — up to ``FPS_RESIDENT_POINTS`` valid pixels per frame, nothing allocated
            beyond the outputs; a frame with more gets status 3.  An int: frames above the resident cap stream through a
            workspace of that many candidates per frame, float32[n, capacity, 4], which the call allocates
    work    that workspace from the caller, for reuse and for graphs (``capacity`` is then its second extent)
    out     optional :class:`FpsBatch` to write into; its ``radius2`` may be None
    form    0, or 1: the streaming form wherever the workspace allows.  The result never depends on it
    Returns :class:`FpsBatch`.  A bad header (2), a frame without a valid pixel (1) and a frame over capacity (3, ``count``
    still true) give zero points, ``pixel`` -1 and ``radius2`` 0.  A frame of fewer than ``points`` valid pixels repeats
    its row 0.  Every bad argument is a ValueError before anything is launched.  Runs on the current stream, no
    synchronisation.

    The HandPointNet input, three launches and nothing on the host in between::

        obb = obb_xforms(depth, offsets, headers)
        fps = farthest_points(depth, offsets, headers, 1024, xforms=obb.xforms)
        place = map_grids(depth, offsets, headers, obb.xforms)          # the OBB frame's cube
        cloud = normalize_joints(fps.points.view(n, -1), place.max_l, place.mid_p).view(n, 1024, 3)
    """
    return _fps_crop(depth, offsets, headers, points, cam, xforms, index, capacity, work, out, form)


def farthest_of(cloud: torch.Tensor, points: int = 1024, capacity: Optional[int] = None,
                work: Optional[torch.Tensor] = None, out: Optional[FpsBatch] = None, form: int = 0) -> FpsBatch:
    """:func:`farthest_points` of clouds that exist already (``tsdf_fps_points_hip``): ``cloud`` is float32 or
    float64[n, P, 3] on the GPU — :func:`point_clouds`' output, or a network's own set-abstraction level.  float64 is
    rounded once to float32; a row with a non-finite coordinate is no candidate; ``pixel`` holds row numbers.  The other
    arguments and the returns are :func:`farthest_points`'s (status 2 does not occur)."""
    M, hint = _fps_points(points), _fps_form(form)
    F = _lib.load_fps()
    if not isinstance(cloud, torch.Tensor) or cloud.dtype not in (torch.float32, torch.float64):
        raise ValueError("cloud must be a float32 or float64 torch.Tensor")
    try:
        _dev_check("cloud", cloud, cloud.dtype)
        if cloud.dim() != 3 or cloud.shape[2] != 3 or not 1 <= cloud.shape[1] < 2 ** 31:
            raise ValueError("cloud must have shape [n, P, 3] with P >= 1")
        dev, n, P = cloud.device, int(cloud.shape[0]), int(cloud.shape[1])
        cap, work = _fps_work(n, capacity, work, dev)
        out = _fps_out(out, n, M, dev)
    except TypeError as e:
        raise ValueError(str(e)) from None
    if n:
        code = _lib.TSDF_FPS_F64 if cloud.dtype is torch.float64 else _lib.TSDF_FPS_F32
        _call(dev, F.tsdf_fps_points_hip,
              [cloud.data_ptr(), code, n, P, M, cap, hint, None, _ptr(work), out.points.data_ptr(), out.pixel.data_ptr(),
               _ptr(out.radius2), out.count.data_ptr(), out.status.data_ptr()], 7)
    return out


class KnnBatch(NamedTuple):
    index: torch.Tensor              # int32[n, C, k]       each neighbour's row in the cloud, nearest first
    dist2: Optional[torch.Tensor]    # float32[n, C, k]     its squared distance
    offsets: Optional[torch.Tensor]  # float32[n, C, k, 3]  neighbour - query, the very differences that were measured
    status: torch.Tensor             # int32[n]             _lib.TSDF_FRAME_*, or the input status copied through


class NormalBatch(NamedTuple):
    normals: torch.Tensor               # float32[n, C, 3]  unit normals turned towards the viewpoint
    curvature: Optional[torch.Tensor]   # float32[n, C]     l0 / (l0 + l1 + l2), the surface variation
    status: torch.Tensor                # int32[n]


def _group_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.GROUP_MAX_K:
        raise ValueError(f"k must be an int in 1..{_lib.GROUP_MAX_K}, got {k!r}")
    return k


def _group_count(name, v, most) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= most:
        raise ValueError(f"{name} must be an int in 1..{most}, got {v!r}")
    return v


def group_plan(P: int, C: int, K: int) -> tuple:
    """``tsdf_group_plan`` (host code only): ``(lds_bytes, queries per workgroup, workgroups per batch position)`` of a call
    with clouds of ``P`` rows, ``C`` queries and ``K`` neighbours."""
    P = _group_count("P", P, _lib.GROUP_MAX_CLOUD)
    C = _group_count("C", C, 2 ** 31 - 1)
    K = _group_k(K)
    lds, per, groups = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load_group().tsdf_group_plan(P, C, K, lds, per, groups), "tsdf_group_plan")
    return lds.value, per.value, groups.value


def _group_in(cloud, queries, status):
    """The input side both entries share, validated: ``(dev, n, P, pitch, C, query pointer, status pointer)``.  ``cloud``
    is float32[n, P, 3], contiguous or the leading rows ``big[:, :P]`` of a contiguous tensor (read in place: ``pitch`` is
    then ``big``'s rows)."""
    if not isinstance(cloud, torch.Tensor) or cloud.dtype is not torch.float32:
        raise ValueError("cloud must be a float32 torch.Tensor")
    if cloud.dim() != 3 or cloud.shape[2] != 3 or not 1 <= cloud.shape[1] <= _lib.GROUP_MAX_CLOUD:
        raise ValueError(f"cloud must have shape [n, P, 3] with P in 1..{_lib.GROUP_MAX_CLOUD}")
    n, P = int(cloud.shape[0]), int(cloud.shape[1])
    pitch = P
    if cloud.is_contiguous():
        _dev_check("cloud", cloud, torch.float32)
    else:
        s = cloud.stride()
        if n == 0 or s[2] != 1 or s[1] != 3 or s[0] % 3 or s[0] < 3 * P:
            raise ValueError("cloud must be contiguous, or the leading rows big[:, :P] of a contiguous tensor")
        pitch = s[0] // 3
        _dev_check("cloud", cloud[0, 0], torch.float32)
    dev = cloud.device
    if queries is None:
        C, qptr = P, None
    elif isinstance(queries, torch.Tensor):
        _dev_check("queries", queries, torch.float32, dev)
        if queries.dim() != 3 or queries.shape[0] != n or queries.shape[1] < 1 or queries.shape[2] != 3:
            raise ValueError(f"queries must have shape [{n}, C, 3] with C >= 1")
        C, qptr = int(queries.shape[1]), queries.data_ptr()
    else:
        C, qptr = _group_count("queries", queries, P), None   # the first C rows of the cloud itself
    if status is not None:
        _shaped("status", status, (n,), torch.int32, dev)
    return dev, n, P, pitch, C, qptr, _ptr(status)


def _group_out(cls, out, fields, optional, dev):
    """The outputs as the NamedTuple ``cls``: allocated from their table (an ``optional`` field only where its flag is
    set), or the caller's ``out`` validated field by field — its optional fields may be None, which the launch then does
    not write."""
    if out is None:
        return cls(*[_out(name, None, shape, dtype, dev) if optional.get(name, True) else None for name, shape, dtype in fields])
    if not isinstance(out, cls):
        raise ValueError(f"out must be a {cls.__name__}")
    for name, shape, dtype in fields:
        if name not in optional or getattr(out, name) is not None:
            _shaped("out." + name, getattr(out, name), shape, dtype, dev)
    return out


def _knn(cloud, k, queries, status, dist2, offsets, out) -> KnnBatch:
    """:func:`knn_groups`; given ``out`` the call allocates nothing."""
    K = _group_k(k)
    G = _lib.load_group()
    try:
        dev, n, P, pitch, C, qptr, sptr = _group_in(cloud, queries, status)
        out = _group_out(KnnBatch, out, (("index", (n, C, K), torch.int32), ("dist2", (n, C, K), torch.float32),
                                         ("offsets", (n, C, K, 3), torch.float32), ("status", (n,), torch.int32)),
                         {"dist2": bool(dist2), "offsets": bool(offsets)}, dev)
    except TypeError as e:   # a bad argument of this entry is a ValueError whatever is wrong with it
        raise ValueError(str(e)) from None
    if n:
        _call(dev, G.tsdf_knn_hip, [cloud.data_ptr(), pitch, qptr, sptr, n, P, C, K, None, out.index.data_ptr(),
                                    _ptr(out.dist2), _ptr(out.offsets), out.status.data_ptr()], 8)
    return out


def knn_groups(cloud: torch.Tensor, k: int, queries=None, status: Optional[torch.Tensor] = None, dist2: bool = True,
               offsets: bool = False, out: Optional[KnnBatch] = None) -> KnnBatch:
    """kNN grouping, what a set-abstraction level of a point network (HandPointNet, PointNet++) reads: for every query its
    ``k`` nearest neighbours in the cloud (``tsdf_knn_hip`` of libtsdf_group.so; include/tsdf_group.h has the contract).
    One launch, the cloud resident in LDS, one wave per query; the result is pinned bit for bit: distances in float32
    without fma by :func:`farthest_points`' expression, nearest first, ties to the LOWEST row.

    cloud    float32[n, P, 3] on the GPU, P in 1..12288: contiguous, or the leading rows ``big[:, :P]`` of a contiguous
             tensor (read in place).  A row with a non-finite coordinate is no candidate: NaN-padded ragged clouds work
    k        neighbours per query, 1..128.  With fewer than ``k`` candidates the trailing slots repeat slot 0
    queries  None: every row of the cloud is a query; an int C: rows 0..C-1 — after farthest point sampling the C-point
             sample, so the centres need no tensor of their own; or float32[n, C, 3] on the GPU.  A query of the cloud
             finds itself (or an equal row before it) in slot 0 at distance 0; a query with a non-finite coordinate gets
             index -1 and zeros
    status   optional int32[n] on the GPU (``fps.status``): a position whose status is not 0 is not read, gets index -1 and
             zeros, and its status is copied through
    dist2 / offsets  which optional outputs to allocate (``offsets``: neighbour - query, float32[n, C, k, 3])
    out      optional :class:`KnnBatch` to write into; its ``dist2`` / ``offsets`` may be None
    Returns :class:`KnnBatch`.  A cloud without a candidate has status 1.  Every bad argument is a ValueError before
    anything is launched.  Runs on the current stream, no synchronisation.

    The HandPointNet input — normals and two grouping levels — with nothing on the host in between::

        obb = obb_xforms(depth, offsets, headers)
        fps = farthest_points(depth, offsets, headers, 1024, xforms=obb.xforms)
        nrm = point_normals(fps.points, 30, xforms=obb.xforms, status=fps.status)
        g1 = knn_groups(fps.points, 64, queries=512, offsets=True)
        g2 = knn_groups(fps.points[:, :512], 64, queries=128, offsets=True)
    """
    return _knn(cloud, k, queries, status, dist2, offsets, out)


def _normals(cloud, k, queries, status, view, curvature, out) -> NormalBatch:
    """:func:`point_normals` with the viewpoint as a tensor or None; given ``out`` the call allocates nothing."""
    K = _group_k(k)
    G = _lib.load_group()
    try:
        dev, n, P, pitch, C, qptr, sptr = _group_in(cloud, queries, status)
        if view is not None:
            _shaped("view", view, (n, 3), torch.float64, dev)
        out = _group_out(NormalBatch, out, (("normals", (n, C, 3), torch.float32), ("curvature", (n, C), torch.float32),
                                            ("status", (n,), torch.int32)), {"curvature": bool(curvature)}, dev)
    except TypeError as e:
        raise ValueError(str(e)) from None
    if n:
        _call(dev, G.tsdf_normals_hip, [cloud.data_ptr(), pitch, qptr, sptr, _ptr(view), n, P, C, K, None,
                                        out.normals.data_ptr(), _ptr(out.curvature), out.status.data_ptr()], 9)
    return out


def _view_of(xforms, n, out=None):
    """The viewpoint under per-frame maps float64[n,24]: the image of the camera centre (the origin) under each map's
    forward rows, its translation column — float64[n,3] (``out``: written there, nothing allocated)."""
    col = xforms.view(n, 6, 4)[:, :3, 3]
    return col.contiguous() if out is None else out.copy_(col)


def point_normals(cloud: torch.Tensor, k: int = 30, queries=None, status: Optional[torch.Tensor] = None,
                  view: Optional[torch.Tensor] = None, xforms: Optional[torch.Tensor] = None, curvature: bool = True,
                  out: Optional[NormalBatch] = None) -> NormalBatch:
    """Surface normals by PCA over each query's ``k`` nearest neighbours (``tsdf_normals_hip`` of libtsdf_group.so): the
    neighbours are :func:`knn_groups`'s; their covariance is summed in float64 in a fixed tree order, its eigenvectors come
    from a fixed number of Jacobi sweeps, the normal is the eigenvector of the smallest eigenvalue turned towards the
    viewpoint, and ``curvature`` is l0 / (l0 + l1 + l2).  One launch; the result is pinned bit for bit.

    cloud / k / queries / status   as for :func:`knn_groups` (``queries`` None: a normal for every point)
    view     optional float64[n, 3] on the GPU: the viewpoint of each position, in the cloud's frame; None is the origin,
             the camera of an unmapped cloud
    xforms   instead of ``view``, the float64[n, 24] maps the cloud was sampled under (``obb.xforms``): the viewpoint is
             the image of the camera centre under each map's forward rows (one small copy builds it)
    curvature  False: no curvature output
    out      optional :class:`NormalBatch` to write into; its ``curvature`` may be None
    Returns :class:`NormalBatch`.  Fewer than 3 neighbours, a non-finite query and a position that is not read give a zero
    normal and zero curvature.  Every bad argument is a ValueError before anything is launched."""
    if view is not None and xforms is not None:
        raise ValueError("view and xforms are two ways to say the same thing: give one")
    if xforms is not None:
        try:
            _group_k(k)
            dev, n = _group_in(cloud, queries, status)[:2]   # every refusal comes before the copy below
            _shaped("xforms", xforms, (n, 24), torch.float64, dev)
        except TypeError as e:
            raise ValueError(str(e)) from None
        view = _view_of(xforms, n)
    return _normals(cloud, k, queries, status, view, curvature, out)


class PointFieldBatch(NamedTuple):
    field: torch.Tensor    # dtype[n, 4J, P] ("cp") or [n, P, 4J] ("pc"): channel j joint j's heat, J + 3j + a its vector
    valid: torch.Tensor    # int32[n, J]  1: a finite joint of a position that was read and has a candidate
    status: torch.Tensor   # int32[n]     _lib.TSDF_FRAME_*, or the input status copied through


class FieldJoints(NamedTuple):
    joints: torch.Tensor   # float32[n, J, 3]  the weighted vote, in the cloud's frame
    weight: torch.Tensor   # float32[n, J]     the sum of the votes' weights (0: no vote, a zero row)
    status: torch.Tensor   # int32[n]


def _field_radius(radius) -> float:
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not 0.0 < float(radius) < float("inf"):
        raise ValueError(f"radius must be a finite number > 0 (in the cloud's units), got {radius!r}")
    return float(radius)


def _field_layout(layout) -> int:
    if not isinstance(layout, str) or layout not in _lib.POINTFIELD_LAYOUTS:
        raise ValueError("layout must be 'cp' ([n, 4J, P]) or 'pc' ([n, P, 4J])")
    return _lib.POINTFIELD_LAYOUTS[layout]


def _field_shape(lay, n, J, P) -> tuple:
    return (n, 4 * J, P) if lay == 0 else (n, P, 4 * J)


def pointfield_plan(P: int, J: int, K: int) -> tuple:
    """``tsdf_pointfield_plan`` (host code only): ``(lds_bytes, joints per workgroup, workgroups per batch position)`` of a
    call with clouds of ``P`` rows, ``J`` joints and ``K`` nearest points (or votes)."""
    P = _group_count("P", P, _lib.POINTFIELD_MAX_CLOUD)
    J = _group_count("J", J, _lib.POINTFIELD_MAX_JOINTS)
    K = _group_count("K", K, _lib.POINTFIELD_MAX_K)
    lds, per, groups = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load_pointfield().tsdf_pointfield_plan(P, J, K, lds, per, groups), "tsdf_pointfield_plan")
    return lds.value, per.value, groups.value


def _point_fields(cloud, joints, k, radius, layout, dtype, status, out) -> PointFieldBatch:
    """:func:`point_fields`; given ``out`` the call allocates nothing."""
    K = _group_count("k", k, _lib.POINTFIELD_MAX_K)
    r, lay, code = _field_radius(radius), _field_layout(layout), _heat_dtype(dtype)
    F = _lib.load_pointfield()
    try:
        dev, n, P, pitch, _, _, sptr = _group_in(cloud, None, status)
        _dev_check("joints", joints, torch.float32, dev)
        if joints.dim() not in (2, 3) or (joints.dim() == 3 and joints.shape[2] != 3):
            raise ValueError(f"joints must have shape [{n}, 3*J] or [{n}, J, 3]")
        J = (_coords("joints", joints, n) or math.prod(joints.shape[1:])) // 3
        if J < 1:
            raise ValueError(f"joints must have shape [{n}, 3*J] or [{n}, J, 3]")
        out = _outs(PointFieldBatch, out, (("field", _field_shape(lay, n, J, P), dtype), ("valid", (n, J), torch.int32),
                                           ("status", (n,), torch.int32)), dev)
    except (TypeError, AttributeError) as e:   # a bad argument of this entry is a ValueError whatever is wrong with it
        raise ValueError(str(e)) from None
    if n:
        _call(dev, F.tsdf_pointfield_encode_hip, [cloud.data_ptr(), pitch, joints.data_ptr(), sptr, n, P, J, K, r, lay, code,
                                                  None, out.field.data_ptr(), out.valid.data_ptr(), out.status.data_ptr()], 11)
    return out


def point_fields(cloud: torch.Tensor, joints: torch.Tensor, k: int = 64, *, radius: float, layout: str = "cp",
                 dtype: torch.dtype = torch.float32, status: Optional[torch.Tensor] = None,
                 out: Optional[PointFieldBatch] = None) -> PointFieldBatch:
    """The labels of a point-to-point regression network (Ge, Ren, Yuan, ECCV 2018): for every point of a sampled cloud and
    every joint a heat value and a unit vector pointing at the joint, defined on the joint's ``k`` nearest points inside a
    ball (``tsdf_pointfield_encode_hip`` of libtsdf_pointfield.so; include/tsdf_pointfield.h has the contract).  One
    launch, the cloud resident in LDS, one wave per joint, a radix select instead of a sort; the result is pinned bit for
    bit: distances as :func:`knn_groups` forms them, ties to the LOWEST row, heat ``1 - d / radius`` and the vector
    ``(joint - point) / d`` in float64, each rounded once.

    cloud    float32[n, P, 3] on the GPU as for :func:`knn_groups` (``fps.points``); a non-finite row is no candidate
    joints   float32[n, 3J] or [n, J, 3] on the GPU, in the cloud's frame and units; a non-finite joint gets a zero field
    k        nearest points per joint, 1..12288; ``k >= P`` is the pure ball rule
    radius   the ball about a joint, in the cloud's units (no default: it depends on them)
    layout   "cp": ``[n, 4J, P]``, what a ``Conv1d`` head emits; "pc": ``[n, P, 4J]``.  Channel j is joint j's heat, channel
             ``J + 3j + a`` component a of its vector
    dtype    torch.float32, torch.float16 or torch.bfloat16 (the float32 value narrowed by round-to-nearest-even)
    status   optional int32[n] on the GPU (``fps.status``): a position whose status is not 0 is not read and gets zeros
    out      optional :class:`PointFieldBatch` to write into; every byte is written
    Returns :class:`PointFieldBatch`.  Every bad argument is a ValueError before anything is launched.  Runs on the current
    stream, no synchronisation."""
    return _point_fields(cloud, joints, k, radius, layout, dtype, status, out)


def field_joints(cloud: torch.Tensor, field: torch.Tensor, *, radius: float, points: int = 25, layout: str = "cp",
                 status: Optional[torch.Tensor] = None, out: Optional[FieldJoints] = None) -> FieldJoints:
    """Each joint back from a (predicted) offset field (``tsdf_pointfield_decode_hip`` of libtsdf_pointfield.so): the
    ``points`` candidates of greatest heat vote ``point + radius * (1 - w) * unit(vector)`` with weight
    ``w = clamp(heat, 0, 1)``; the weighted mean is summed in float64 in a fixed tree order, so the result is pinned bit for
    bit.  Ties go to the lowest row; a NaN heat never wins over a number.

    cloud    float32[n, P, 3] on the GPU as for :func:`point_fields`
    field    float32 / float16 / bfloat16 on the GPU, ``[n, 4J, P]`` ("cp") or ``[n, P, 4J]`` ("pc")
    radius   the ball the field was written with
    points   voting points per joint, 1..128
    status   optional int32[n] on the GPU: a position whose status is not 0 is not read and gets zero rows
    out      optional :class:`FieldJoints` to write into
    Returns :class:`FieldJoints`; a joint without a vote of positive weight is a zero row of weight 0."""
    M = _group_count("points", points, _lib.POINTFIELD_MAX_VOTES)
    r, lay = _field_radius(radius), _field_layout(layout)
    F = _lib.load_pointfield()
    try:
        dev, n, P, pitch, _, _, sptr = _group_in(cloud, None, status)
        if not isinstance(field, torch.Tensor):
            raise ValueError("field must be a torch.Tensor")
        code = _heat_dtype(field.dtype)
        _dev_check("field", field, field.dtype, dev)
        C = int(field.shape[1 if lay == 0 else 2]) if field.dim() == 3 else 0
        if C < 4 or C % 4 or tuple(field.shape) != _field_shape(lay, n, C // 4, P) or C // 4 > _lib.POINTFIELD_MAX_JOINTS:
            raise ValueError(f"field must have shape [{n}, 4*J, {P}] ('cp') or [{n}, {P}, 4*J] ('pc')")
        J = C // 4
        out = _outs(FieldJoints, out, (("joints", (n, J, 3), torch.float32), ("weight", (n, J), torch.float32),
                                       ("status", (n,), torch.int32)), dev)
    except (TypeError, AttributeError) as e:
        raise ValueError(str(e)) from None
    if n:
        _call(dev, F.tsdf_pointfield_decode_hip, [cloud.data_ptr(), pitch, field.data_ptr(), sptr, n, P, J, M, r, lay, code,
                                                  None, out.joints.data_ptr(), out.weight.data_ptr(), out.status.data_ptr()], 11)
    return out


class PatchBatch(NamedTuple):
    patch: torch.Tensor    # dtype[n, 1, S, S]  depth normalised by the cube: [-1, 1] inside it, ``background`` elsewhere
    status: torch.Tensor   # int32[n]           0, 1 (no usable cube: input status, centre, cube or map), 2 (no usable source)


class UvdBatch(NamedTuple):
    uvd: torch.Tensor      # float32[n, J, 3]   (a, b, w): column, row and depth in the patch's normalised coordinates
    valid: torch.Tensor    # int32[n, J]        0: a non-finite joint, one at or behind the camera, or a position with a status
    status: torch.Tensor   # int32[n]           0, or 1 (no usable cube, or a singular map)


def _patch_size(size) -> int:
    if isinstance(size, bool) or not isinstance(size, int) or size % 8 or not _lib.PATCH_MIN_SIZE <= size <= _lib.PATCH_MAX_SIZE:
        raise ValueError(f"size must be an integer multiple of 8 in {_lib.PATCH_MIN_SIZE}..{_lib.PATCH_MAX_SIZE}, got {size!r}")
    return size


def _patch_interp(interp) -> int:
    if not isinstance(interp, str) or interp not in _lib.PATCH_INTERPS:
        raise ValueError(f"interp must be 'nearest' or 'bilinear', got {interp!r}")
    return _lib.PATCH_INTERPS[interp]


def _patch_dtype(dtype):
    """(torch dtype, its code); None is float32."""
    dtype = torch.float32 if dtype is None else dtype
    return dtype, _heat_dtype(dtype)


def _patch_background(background) -> float:
    if isinstance(background, bool) or not isinstance(background, (int, float)):
        raise TypeError(f"background must be a number, got {background!r}")
    return float(background)


def patch_plan(size: int = 128, dtype: Optional[torch.dtype] = None) -> tuple:
    """``tsdf_patch_plan`` (host code only): ``(pixels per lane, rows per workgroup, work items per batch position)`` of a
    patch launch at edge ``size`` and element type ``dtype``."""
    S, (_, code) = _patch_size(size), _patch_dtype(dtype)
    px, rows, items = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load_patch().tsdf_patch_plan(S, code, px, rows, items), "tsdf_patch_plan")
    return px.value, rows.value, items.value


def _patch_cube(n, com, cube, affine, status, dev):
    """The arguments that fix every position's cube, validated: returns (com as float64[n, 3], the scalar cube, the cube
    tensor or None, affine, status) — what the four entries take after their source."""
    if not isinstance(com, torch.Tensor):
        raise TypeError("com must be a torch.Tensor")
    if com.dtype not in (torch.float64, torch.float32):
        raise TypeError(f"com must be torch.float64 (HandCrops.com) or torch.float32, got {com.dtype}")
    if tuple(com.shape) != (n, 3):
        raise ValueError(f"com must have shape [{n}, 3]")
    _dev_check("com", com, com.dtype, dev)
    if com.dtype is torch.float32:
        com = com.double()                                   # exact
    cube_n = None
    if isinstance(cube, torch.Tensor):
        cube_n = _shaped("cube", cube, (n,), torch.float32, dev)
        cube = 0.0
    elif isinstance(cube, bool) or not isinstance(cube, (int, float)) or not 0.0 < float(cube) < float("inf"):
        raise ValueError(f"cube must be a finite number > 0 (mm) or a float32 tensor [n], got {cube!r}")
    if affine is not None:
        if not isinstance(affine, torch.Tensor):
            raise TypeError("affine must be a torch.Tensor (patch_affines builds one)")
        _shaped("affine", affine, (n, 6), torch.float64, dev)
    if status is not None:
        if not isinstance(status, torch.Tensor):
            raise TypeError("status must be a torch.Tensor")
        _shaped("status", status, (n,), torch.int32, dev)
    return com, float(cube), cube_n, affine, status


def _patch_outs(out, n, S, dtype, dev) -> PatchBatch:
    return _outs(PatchBatch, out, (("patch", (n, 1, S, S), dtype), ("status", (n,), torch.int32)), dev)


def _patch_aligned(patch):
    if patch.data_ptr() % 16:
        raise ValueError("out.patch must be 16-byte aligned (a lane's pixels leave as one 16-byte store)")


def frame_patches(frames: torch.Tensor, com: torch.Tensor, *, size: int = 128, cube=250.0, interp: str = "nearest",
                  dtype: Optional[torch.dtype] = None, affine: Optional[torch.Tensor] = None, background: float = 1.0,
                  cam: Optional[_lib.TsdfCam] = None, shift: Optional[int] = None, index: Optional[torch.Tensor] = None,
                  status: Optional[torch.Tensor] = None, out: Optional[PatchBatch] = None) -> PatchBatch:
    """The input of a 2-D CNN that reads a depth image (DeepPrior++, A2J, DenseReg, Pose-REN): per batch position a
    ``size`` x ``size`` patch resampled from the image rectangle of the cube of edge ``cube`` mm about ``com``, straight
    from raw frames (``tsdf_patch_frames_hip`` of libtsdf_patch.so; include/tsdf_patch.h has the contract, pinned bit for
    bit).  A pixel's depth d becomes ``(d - cd) / (cube / 2)`` in [-1, 1]; a pixel whose tap is outside the frame, invalid
    or outside the cube in depth is ``background``.  One gather launch on the current stream, no synchronisation.

    frames   float32[N,H,W] mm, or uint16[N,H,W] with ``shift`` (0..7), as for :func:`locate_hands`
    com      float64[n,3] on the GPU, ``HandCrops.com``'s convention (camera frame, mm, ``z = -depth``); a float32 tensor
             (``aabb(...)``'s or a placement's ``mid_p``) is widened
    size     the patch's edge S, a multiple of 8 in 8..512
    cube     the cube's edge in mm: a float, or a float32 tensor [n] (scale augmentation of the cube is per frame)
    interp   "nearest": the tap ``floor(u + 0.5)``; "bilinear": the four neighbours, renormalised over the VALID ones, so the
             hand is never blended with the background (what ``grid_sample`` does at the silhouette)
    dtype    None / torch.float32, torch.float16 or torch.bfloat16
    affine   optional float64[n,6] on the GPU (:func:`patch_affines`): rows ``a00 a01 a02 a10 a11 a12`` mapping PATCH
             coordinates in [-1, 1]^2 to coordinates in the cube's rectangle; None is the identity
    index    optional int64[n] on the GPU: batch position i reads frame index[i] (outside [0, N): status 2)
    status   optional int32[n] on the GPU (``HandCrops.status``): a position with a non-zero entry is not read (status 1)
    out      optional :class:`PatchBatch` to write into (capturable); ``out.patch`` must be 16-byte aligned
    Returns :class:`PatchBatch`; every pixel of a position with a status is ``background``.  :func:`crop_patches` on
    :func:`locate_hands`' pack need NOT give the same patch at the crop's right and bottom edge (``floor(u + 0.5)`` can reach
    the crop's exclusive bound) or under an ``affine`` (this form sees pixels the crop never held)."""
    P = _lib.load_patch()
    S, lerp, (dtype, code), bg = _patch_size(size), _patch_interp(interp), _patch_dtype(dtype), _patch_background(background)
    if not isinstance(frames, torch.Tensor):
        raise TypeError("frames must be a torch.Tensor")
    if frames.dtype not in _LOCATE_TYPES:
        raise TypeError(f"frames must be torch.float32 or torch.uint16, got {frames.dtype}")
    if frames.dim() != 3 or frames.shape[1] < 1 or frames.shape[2] < 1:
        raise ValueError("frames must have shape [N, H, W]")
    u16 = frames.dtype is torch.uint16
    if u16:
        if isinstance(shift, bool) or not isinstance(shift, int) or not 0 <= shift <= _lib.DEPTH16_MAX_SHIFT:
            raise ValueError(f"uint16 frames need shift, an integer in 0..{_lib.DEPTH16_MAX_SHIFT}; got {shift!r}")
    elif shift is not None:
        raise ValueError("shift belongs to uint16 frames")
    _dev_check("frames", frames, frames.dtype)
    dev = frames.device
    n_src, H, W = (int(v) for v in frames.shape)
    n = n_src if index is None else _indexed(index, n_src, dev, "index needs at least one frame")
    com, cube, cube_n, affine, status = _patch_cube(n, com, cube, affine, status, dev)
    out = _patch_outs(out, n, S, dtype, dev)
    _patch_aligned(out.patch)
    if n:
        _call(dev, P.tsdf_patch_frames_hip,
              [frames.data_ptr(), _LOCATE_TYPES[frames.dtype], shift if u16 else 0, n_src, H, W, _ptr(index), com.data_ptr(), cube,
               _ptr(cube_n), _ptr(affine), _ptr(status), n, S, lerp, code, bg, *_cam5(cam), None, out.patch.data_ptr(),
               out.status.data_ptr()], 22)
    return out


def crop_patches(depth: torch.Tensor, offsets: torch.Tensor, headers: torch.Tensor, com: torch.Tensor, *, size: int = 128,
                 cube=250.0, interp: str = "nearest", dtype: Optional[torch.dtype] = None,
                 affine: Optional[torch.Tensor] = None, background: float = 1.0, cam: Optional[_lib.TsdfCam] = None,
                 index: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
                 out: Optional[PatchBatch] = None) -> PatchBatch:
    """:func:`frame_patches` on a pack — the ``depth / offsets / headers`` triple every entry here reads and
    :func:`locate_hands` writes (``tsdf_patch_crops_hip``: the same kernel and the same contract).  The source rectangle of
    a position is its header's ``[left, right) x [top, bottom)``; a header the voxelizers' header rule refuses, or an
    ``index`` outside the pack, gives status 2.  A tap outside the crop is invalid even where the frame the crop was cut
    from had a pixel there: at the crop's right and bottom edge (``floor(u + 0.5)`` can reach the exclusive bound) and under
    an ``affine`` this need NOT equal :func:`frame_patches` on the frames themselves.  The other arguments are
    :func:`frame_patches`'."""
    P = _lib.load_patch()
    S, lerp, (dtype, code), bg = _patch_size(size), _patch_interp(interp), _patch_dtype(dtype), _patch_background(background)
    dev, n_src, _ = _pack(_lib.load(), depth, offsets, headers)
    n = n_src if index is None else _indexed(index, n_src, dev, "index needs at least one source frame")
    com, cube, cube_n, affine, status = _patch_cube(n, com, cube, affine, status, dev)
    out = _patch_outs(out, n, S, dtype, dev)
    _patch_aligned(out.patch)
    if n:
        _call(dev, P.tsdf_patch_crops_hip,
              [depth.data_ptr(), depth.numel(), offsets.data_ptr(), headers.data_ptr(), n_src, _ptr(index), com.data_ptr(), cube,
               _ptr(cube_n), _ptr(affine), _ptr(status), n, S, lerp, code, bg, *_cam5(cam), None, out.patch.data_ptr(),
               out.status.data_ptr()], 21)
    return out


def _patch_joints(name, t):
    """float32[n, 3J] or [n, J, 3] on the GPU: returns (n, J)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    _dev_check(name, t, torch.float32)
    if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] != 3) or (t.dim() == 2 and t.shape[1] % 3):
        raise ValueError(f"{name} must have shape [n, 3*J] or [n, J, 3]")
    n, J = int(t.shape[0]), math.prod(t.shape[1:]) // 3
    if not 1 <= J <= _lib.PATCH_MAX_JOINTS:
        raise ValueError(f"{name} must hold 1..{_lib.PATCH_MAX_JOINTS} joints of 3 coordinates per frame")
    return n, J


def joints_to_uvd(gt: torch.Tensor, com: torch.Tensor, *, cube=250.0, affine: Optional[torch.Tensor] = None,
                  cam: Optional[_lib.TsdfCam] = None, status: Optional[torch.Tensor] = None,
                  out: Optional[UvdBatch] = None) -> UvdBatch:
    """The labels of a patch network: camera-frame joints ``gt`` (float32[n,3J] or [n,J,3] on the GPU, mm) in the normalised
    coordinates of the patch :func:`frame_patches` cuts with the same ``com`` / ``cube`` / ``affine`` / ``cam``
    (``tsdf_patch_uvd_hip``): ``(a, b)`` the column and row in [-1, 1] — pixel centre j is ``(2j + 1) / S - 1`` —, ``w`` the
    depth ``(-z - cd) / (cube / 2)``.  A joint inside the cube and the patch is in [-1, 1]^3; nothing is clamped.  Under an
    ``affine`` the inverse map is applied, so a singular one gives the position status 1.  Returns :class:`UvdBatch`; an
    invalid joint is a zero row.  One thread per joint, float64 arithmetic rounded once: pinned bit for bit."""
    P = _lib.load_patch()
    n, J = _patch_joints("gt", gt)
    dev = gt.device
    com, cube, cube_n, affine, status = _patch_cube(n, com, cube, affine, status, dev)
    out = _outs(UvdBatch, out, (("uvd", (n, J, 3), torch.float32), ("valid", (n, J), torch.int32), ("status", (n,), torch.int32)), dev)
    if n:
        _call(dev, P.tsdf_patch_uvd_hip,
              [gt.data_ptr(), com.data_ptr(), cube, _ptr(cube_n), _ptr(affine), _ptr(status), n, J, *_cam5(cam), None,
               out.uvd.data_ptr(), out.valid.data_ptr(), out.status.data_ptr()], 13)
    return out


def uvd_to_joints(uvd: torch.Tensor, com: torch.Tensor, *, cube=250.0, affine: Optional[torch.Tensor] = None,
                  cam: Optional[_lib.TsdfCam] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The way back (``tsdf_patch_joints_hip``): a network's ``uvd`` (float32[n,3J] or [n,J,3] on the GPU) as camera-frame
    joints float32[n,J,3] in mm, through the forward ``affine`` and the cube's rectangle.  A position without a usable
    cube gets zero rows.  ``uvd_to_joints(joints_to_uvd(x).uvd, ...)`` returns x to within the two float32 roundings."""
    P = _lib.load_patch()
    n, J = _patch_joints("uvd", uvd)
    dev = uvd.device
    com, cube, cube_n, affine, _ = _patch_cube(n, com, cube, affine, None, dev)
    out = _out("out", out, (n, J, 3), torch.float32, dev)
    if n:
        _call(dev, P.tsdf_patch_joints_hip,
              [uvd.data_ptr(), com.data_ptr(), cube, _ptr(cube_n), _ptr(affine), None, n, J, *_cam5(cam), None, out.data_ptr()], 13)
    return out


def patch_affines(angle: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
                  shift: Optional[torch.Tensor] = None, *, n: Optional[int] = None, device=None) -> torch.Tensor:
    """The in-plane augmentation of a patch network as the ``affine`` of :func:`frame_patches`: float64[n,6] rows
    ``a00 a01 a02 a10 a11 a12`` of the map from PATCH coordinates ``(a, b)`` in [-1, 1]^2 (a to the right, b DOWN, as image
    rows run) to coordinates ``(a', b')`` in the cube's rectangle:

        a' = s (cos t * a - sin t * b) + tx          b' = s (sin t * a + cos t * b) + ty

    angle  [n] radians, t.  The SAMPLING frame turns by t from the a axis towards the b axis — clockwise on a screen whose
           rows run down —, so the hand appears turned counter-clockwise by t in the patch.
    scale  [n], s.  s > 1 samples a LARGER part of the source: the hand appears smaller by 1 / s.
    shift  [n,2], (tx, ty) in half-patch units: the patch's centre reads the point (tx, ty) of the cube's rectangle, so
           the hand appears moved by (-tx, -ty); one patch pixel is 2 / S.
    Each is a per-frame tensor the caller has drawn (any floating type, on one device) or None (0, 1, (0, 0)); with all
    three None, ``n`` and ``device`` give the identity rows.  Built with torch ops in float64 on the tensors' device: no
    kernel of this package, nothing on the host.  The labels follow through :func:`joints_to_uvd` with the same rows."""
    given = [("angle", angle, 1), ("scale", scale, 1), ("shift", shift, 2)]
    for name, t, dim in given:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise TypeError(f"{name} must be a floating-point torch.Tensor")
        if t.dim() != dim or (dim == 2 and t.shape[1] != 2):
            raise ValueError(f"{name} must have shape {'[n]' if dim == 1 else '[n, 2]'}")
        if n is not None and t.shape[0] != n:
            raise ValueError(f"{name} has {t.shape[0]} rows, expected {n}")
        if device is not None and t.device != torch.device(device):
            raise ValueError(f"{name} is on {t.device}, expected {device}")
        n, device = int(t.shape[0]), t.device
    if n is None:
        raise ValueError("patch_affines needs a tensor or n")
    kw = dict(dtype=torch.float64, device=device)
    t = angle.double() if angle is not None else torch.zeros(n, **kw)
    s = scale.double() if scale is not None else torch.ones(n, **kw)
    sh = shift.double() if shift is not None else torch.zeros((n, 2), **kw)
    c, si = s * torch.cos(t), s * torch.sin(t)
    return torch.stack([c, -si, sh[:, 0], si, c, sh[:, 1]], dim=1).contiguous()


def patch_frames(frames: torch.Tensor, size: int = 128, *, gt: Optional[torch.Tensor] = None,
                 affine: Optional[torch.Tensor] = None, interp: str = "nearest", dtype: Optional[torch.dtype] = None,
                 background: float = 1.0, **locate):
    """Raw depth frames to the input and labels of a patch network: :func:`locate_hands` (``grid=False``), then
    :func:`frame_patches` on the SAME frames with ``crops.com`` and ``crops.status``, and with ``gt`` (float32[n,3J] or
    [n,J,3] on the GPU, camera frame) :func:`joints_to_uvd` — all on one stream, nothing on the host in between.  Returns
    ``(PatchBatch, HandCrops)`` or ``(PatchBatch, HandCrops, UvdBatch)``.

    **locate   :func:`locate_hands`' keywords (``cube``, ``near``, ``far``, ``seed_band``, ``refine``, ``cam``, ``shift``,
               ``index``, ``out``); ``cube``, ``cam``, ``shift`` and ``index`` go to the patch as well.
    A frame in which no hand is found (``crops.status`` 1) or whose index is outside the frames (2) gets a patch of
    ``background`` and status 1."""
    if "grid" in locate:
        raise TypeError("patch_frames sets locate_hands' grid itself")
    _patch_size(size), _patch_interp(interp), _patch_dtype(dtype), _patch_background(background)   # before the first launch
    crops = locate_hands(frames, grid=False, **locate)
    cube, cam = locate.get("cube", 250.0), locate.get("cam")
    patches = frame_patches(frames, crops.com, size=size, cube=cube, interp=interp, dtype=dtype, affine=affine,
                            background=background, cam=cam, shift=locate.get("shift"), index=locate.get("index"),
                            status=crops.status)
    if gt is None:
        return patches, crops
    return patches, crops, joints_to_uvd(gt, crops.com, cube=cube, affine=affine, cam=cam, status=crops.status)
