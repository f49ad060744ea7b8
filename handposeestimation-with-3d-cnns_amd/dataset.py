"""On-the-fly MSRA dataset: depth crops in, voxel grids out of the GPU — no preprocessed npz files.

The reference voxelizes every frame offline (pre/read_MSRA.py:37-140, ~0.2 s per frame), writes
``result/<subject>/TSDF/<gesture>.npz`` and then loads *all* of it into host RAM
(3D_CNN/dataset.py:35-38,99-117: ~76 k frames x 393 KB).  Here the dataset holds the raw frames
(``header``, ``depth`` crop, ``gt``) — straight from the ``.bin`` files, or, after one packing pass
(``packing.pack_tree``), from one memory-mapped ``.tsdfpk`` file per subject — and the loader packs a
batch, uploads it once and calls the HIP voxelizer on the training stream; what comes out is the tuple
the reference's ``__getitem__`` returns (3D_CNN/dataset.py:73-79), batched and already on the GPU:
``(tsdf[n,3,R,R,R], gt[n,63], max_l[n], mid_p[n,3])``.

Kept from the reference: directory layout ``<root>/<subject>/<gesture>/{joint.txt, 000000_depth.bin..}``
(pre/read_MSRA.py:46-50,79,99), leave-one-subject-out split (3D_CNN/dataset.py:44-53) and the
``small`` subset of 4 subjects x 5 gestures (:26-31).  Fixed: ``opt`` is honoured instead of being
ignored (:20-22).

Label sign convention (the "z flip", 3D_CNN/dataset.py:107-109).  MSRA's joint.txt stores joints in the
camera frame this pipeline uses throughout — the camera looks down -z, a point's z is MINUS its depth
(pre/process.py:46,58; pre/tsdf_numba.py:94) — so ``mid_p`` and the labels agree as they come from the file and
nothing is flipped here.  The reference reader negates z only for 3-D ``[n,21,3]`` label arrays, which pairs with
writer lines that are commented out (pre/read_MSRA.py:81-82: they would have stored z pre-negated); for the
``[n,63]`` arrays its writer really saves, the reader's branch is skipped (and ``g_t`` is then undefined — it
crashes, App. B#11).  ``export.write_gesture(gt_3d=True)`` therefore stores z pre-negated, so that the reference
reader's flip restores the camera-frame sign.
"""
from __future__ import annotations

import ctypes
import os
import sys
import queue
import threading
import warnings
from typing import Iterator, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.utils.data as data

from . import _lib, augment, packing, shard
from .pca import JointPCA, fit_joint_pca
from .voxelize import (AugmentedStep, TsdfBatch, _get_raw_stream, aabb, aug_state, aug_xforms, aug_xforms_at,  # noqa: F401
                       denormalize_joints, empty_batch, normalize_joints, obb_xforms, project_joints, voxelize,
                       voxelize_aug, voxelize_grid_lowp, voxelize_indexed, voxelize_labels, widen_depth16, _lowp_dtype,
                       _place_aabb)


def _common_depth_shift(packs: Sequence[packing.PackedFrames]) -> Optional[int]:
    """The one ``depth_shift`` of a dataset's packs (None: float32 depth).  Packs of different forms or shifts are
    refused: a batch is one buffer with one scale."""
    forms = sorted({-1 if pk.depth_shift is None else int(pk.depth_shift) for pk in packs})
    if len(forms) > 1:
        names = ", ".join("float32" if f < 0 else f"16-bit with shift {f}" for f in forms)
        raise ValueError(f"the packs of one dataset must share one depth form, these are {names}: repack them "
                         "(packing.pack_tree(..., depth16=None) or one forced shift, overwrite=True)")
    return None if not forms or forms[0] < 0 else forms[0]


def _subset(size: str) -> Tuple[int, int]:
    if size == "full":
        return 9, 17
    if size == "small":
        return 4, 5
    raise ValueError("size must be 'full' or 'small'")


class MSRADepthDataset(data.Dataset):
    """Raw MSRA frames: ``__getitem__ -> (header int32[6], depth float32[N], gt float32[63])``.

    root_path   the MSRA tree ``<root>/<subject>/<gesture>/...``
    packed_dir  directory of ``<subject>.tsdfpk`` packs (``packing.pack_tree``).  Given, frames come from the
                memory-mapped packs — one ``open()`` per subject instead of one per frame per epoch
                (pre/read_MSRA.py:98-106 re-reads ~8,500 files per subject); missing packs are built on first use
                when ``build_packs`` is true.
    """

    def __init__(self, root_path: str, train: bool = True, test_idx: int = 2, size: str = "full",
                 subjects: Optional[Sequence[str]] = None, packed_dir: Optional[str] = None,
                 build_packs: bool = True):
        n_sub, n_ges = _subset(size)
        self.root_path = root_path
        self.train = train
        self.test_idx = test_idx
        if subjects is not None:
            all_sub = list(subjects)
        elif root_path is not None and os.path.isdir(root_path):
            # subject directories (MSRA: P0..P8) — not a directory of packs that happens to live inside the tree
            skip = os.path.abspath(packed_dir) if packed_dir is not None else None
            all_sub = sorted(d for d in os.listdir(root_path) if os.path.isdir(os.path.join(root_path, d))
                             and os.path.abspath(os.path.join(root_path, d)) != skip)[:n_sub]
        elif packed_dir is not None:
            all_sub = sorted(f[:-7] for f in os.listdir(packed_dir) if f.endswith(".tsdfpk"))[:n_sub]
        else:
            raise ValueError("root_path is not a directory and no packed_dir was given")
        if not 0 <= test_idx < len(all_sub):
            raise ValueError("test_idx out of range")
        chosen = [s for i, s in enumerate(all_sub) if (i != test_idx) == train]
        self.subjects = chosen
        self.paths: List[str] = []
        self.packs: List[packing.PackedFrames] = []
        self._pack_of = np.zeros(0, np.int32)     # frame -> index into self.packs
        self._local = np.zeros(0, np.int64)       # frame -> frame index inside that pack
        gts: List[np.ndarray] = []
        if packed_dir is not None:
            pk_of, loc = [], []
            for sub in chosen:
                path = os.path.join(packed_dir, sub + ".tsdfpk")
                if not os.path.exists(path):
                    if not build_packs:
                        raise FileNotFoundError(path)
                    packing.pack_tree(root_path, packed_dir, subjects=[sub])
                pk = packing.PackedFrames.load(path, mmap=True)
                gs = pk.group_start if pk.group_start is not None else np.array([0, len(pk)])
                end = int(gs[min(n_ges, len(gs) - 1)])   # the first n_ges gestures (3D_CNN/dataset.py:26-31)
                self.packs.append(pk)
                pk_of.append(np.full(end, len(self.packs) - 1, np.int32))
                loc.append(np.arange(end, dtype=np.int64))
                gts.append(np.asarray(pk.gt[:end]) if pk.gt is not None else np.zeros((end, 63), np.float32))
            if pk_of:
                self._pack_of, self._local = np.concatenate(pk_of), np.concatenate(loc)
        else:
            for sub in chosen:
                sub_dir = os.path.join(root_path, sub)
                gestures = sorted(g for g in os.listdir(sub_dir) if os.path.isdir(os.path.join(sub_dir, g)))
                for ges in gestures[:n_ges]:
                    g_dir = os.path.join(sub_dir, ges)
                    bin_num, gt = packing.read_joint(g_dir)
                    self.paths += packing.gesture_bin_paths(g_dir, bin_num)
                    gts.append(gt)
        self.depth_shift = _common_depth_shift(self.packs)   # None: float32 depth; k: every pack holds uint16 * 2^-k
        self.ground_truth = np.concatenate(gts) if gts else np.zeros((0, 63), np.float32)

    @classmethod
    def from_packs(cls, packs: Sequence[packing.PackedFrames]) -> "MSRADepthDataset":
        """A dataset over packs that are already in memory (no directory walk, no split)."""
        self = cls.__new__(cls)
        self.root_path, self.train, self.test_idx, self.subjects, self.paths = None, True, -1, [], []
        self.packs = list(packs)
        self.depth_shift = _common_depth_shift(self.packs)
        self._pack_of = np.concatenate([np.full(len(pk), k, np.int32) for k, pk in enumerate(self.packs)])
        self._local = np.concatenate([np.arange(len(pk), dtype=np.int64) for pk in self.packs])
        self.ground_truth = np.concatenate([np.asarray(pk.gt) if pk.gt is not None else np.zeros((len(pk), 63), np.float32)
                                            for pk in self.packs])
        return self

    @property
    def packed(self) -> bool:
        return bool(self.packs)

    def __len__(self) -> int:
        return len(self._local) if self.packed else len(self.paths)

    def pixels(self) -> Optional[np.ndarray]:
        """Pixels per frame (int64[n]) when known without touching the files (packed datasets)."""
        if not self.packed:
            return None
        out = np.empty(len(self), np.int64)
        for k, pk in enumerate(self.packs):
            m = self._pack_of == k
            out[m] = pk.pixels[self._local[m]]
        return out

    def __getitem__(self, index: int):
        if self.packed:
            pk = self.packs[int(self._pack_of[index])]
            h, d = pk.frame(int(self._local[index]))
            return np.asarray(h), np.asarray(d), self.ground_truth[index]
        header, depth = packing.read_bin(self.paths[index])
        return header, depth, self.ground_truth[index]

    def pin_packs(self, limit_bytes: int = 32 << 30) -> bool:
        """Page-lock the packs' depth payloads (if they fit ``limit_bytes``) so that contiguous batches upload
        without a staging copy.  Returns whether the packs are pinned."""
        if not self.packed or sum(int(pk.depth.nbytes) for pk in self.packs) > limit_bytes:
            return False
        for pk in self.packs:
            pk.pin()
        return True

    def contiguous_source(self, idx: np.ndarray):
        """(pinned tensor slice — float32, or uint16 over 16-bit packs —, PackedFrames view) when ``idx`` is a run of
        consecutive frames of one pinned pack, else None."""
        idx = np.asarray(idx, np.int64)
        if not self.packed or idx.size == 0 or not (np.diff(idx) == 1).all():
            return None
        ks = self._pack_of[idx]
        pk = self.packs[int(ks[0])]
        if ks[0] != ks[-1] or getattr(pk, "_pinned", None) is None:
            return None
        a, b = int(self._local[idx[0]]), int(self._local[idx[-1]]) + 1
        view = pk.slice(a, b)
        view.gt = self.ground_truth[idx]
        return pk._pinned[int(pk.offsets[a]):int(pk.offsets[b])], view

    def take(self, idx: np.ndarray, depth_out: Optional[np.ndarray] = None) -> packing.PackedFrames:
        """Frames ``idx`` as one packed batch (with labels) in the dataset's depth form: uint16 over 16-bit packs
        (``depth_out`` is then uint16 too), else float32.  Packed datasets gather straight from the memory maps (one slice
        when the indices are consecutive inside a subject); otherwise the files are read."""
        idx = np.asarray(idx, np.int64)
        if self.packed and idx.size:
            ks = self._pack_of[idx]
            if (ks == ks[0]).all():
                out = self.packs[int(ks[0])].take(self._local[idx], depth_out)
                out.gt = self.ground_truth[idx]
                return out
            if self.depth_shift is not None:   # frames of several 16-bit packs (they share the shift): stay in 16 bits
                raw = [self.packs[int(k)].raw_frame(int(l)) for k, l in zip(ks, self._local[idx])]
                off = np.zeros(idx.size + 1, np.int64)
                np.cumsum([d.size for _, d in raw], out=off[1:])
                if depth_out is not None and depth_out.dtype != np.uint16:
                    raise TypeError(f"depth_out is {depth_out.dtype}, the dataset's packs hold uint16 depth")
                depth = depth_out[: off[-1]] if depth_out is not None else np.empty(int(off[-1]), np.uint16)
                for k, (_, d) in enumerate(raw):
                    depth[off[k]:off[k + 1]] = d
                return packing.PackedFrames(depth, off, np.stack([np.asarray(h) for h, _ in raw]), self.ground_truth[idx],
                                            depth_shift=self.depth_shift)
            pk = packing.pack_frames(self.packs[int(k)].frame(int(l)) for k, l in zip(ks, self._local[idx]))
            if depth_out is not None:
                depth_out[: pk.depth.size] = pk.depth
                pk.depth = depth_out[: pk.depth.size]
            pk.gt = self.ground_truth[idx]
            return pk
        pk = packing.pack_frames(self[int(i)][:2] for i in idx)
        if depth_out is not None:
            depth_out[: pk.depth.size] = pk.depth
            pk.depth = depth_out[: pk.depth.size]
        pk.gt = self.ground_truth[idx] if idx.size else np.zeros((0, 63), np.float32)
        return pk


def collate_frames(batch) -> Tuple[packing.PackedFrames, np.ndarray]:
    """[(header, depth, gt), ...] -> (PackedFrames, gt float32[n,63]) on the host."""
    pk = packing.pack_frames((h, d) for h, d, _ in batch)
    gt = np.stack([g for _, _, g in batch]).astype(np.float32) if batch else np.zeros((0, 63), np.float32)
    return pk, gt


def voxelize_batch(pk: packing.PackedFrames, gt: np.ndarray, device, res: int = 32, pin: bool = True):
    """Upload one packed batch and voxelize it on the current stream of ``device``.

    Returns ``(tsdf, gt, max_l, mid_p, status)`` as GPU tensors — the first four are the reference's
    per-item tuple (3D_CNN/dataset.py:73-79) batched."""
    depth, offsets, headers = pk.to_torch(device, pin=pin, non_blocking=True)
    tgt = torch.from_numpy(np.ascontiguousarray(gt))
    if pin:
        tgt = tgt.pin_memory()
    tgt = tgt.to(device, non_blocking=True)
    out: TsdfBatch = voxelize(depth, offsets, headers, res=res)
    return out.tsdf, tgt, out.max_l, out.mid_p, out.status


class VoxelBatch(NamedTuple):
    """What :class:`VoxelLoader` yields.  The first four fields are the reference's per-item tuple
    (3D_CNN/dataset.py:73-79) batched on the GPU; ``status`` tells degenerate / malformed frames apart (the
    reference returns None for them, tsdf_numba.py:162-171), ``gt_nor`` are the labels in the cube's [0,1] frame
    (pre/joint_nor.py:8-18 + the clamp of 3D_CNN/train.py:241-242), written by the voxelizer's own launch."""

    tsdf: torch.Tensor
    gt: torch.Tensor
    max_l: torch.Tensor
    mid_p: torch.Tensor
    status: torch.Tensor
    gt_nor: Optional[torch.Tensor]


def plan_batches(n: int, batch_size: int, rank: int = 0, world: int = 1, shuffle: bool = False, seed: int = 0,
                 epoch: int = 0, drop_last: bool = False, weights: Optional[np.ndarray] = None,
                 balance: Optional[str] = None) -> List[np.ndarray]:
    """The frame indices of every batch of one epoch for one rank.  Ranks own CONTIGUOUS shards of the frame range
    (``shard.shard_bounds``) — the split BASELINE.json configs[3] names; shuffling permutes inside the rank's shard.
    No collective is involved.

    balance  ``"frames"``: shards of equal frame count (sizes differ by at most one) and THE SAME BATCHES — number AND
             sizes — ON EVERY RANK: what a training loop that steps a gradient collective once per batch needs.  A rank
             whose shard is one frame short repeats one of its frames (the first of its epoch order) at the end of its
             index list BEFORE the batches are cut, as ``torch.utils.data.DistributedSampler`` pads samples — so no rank
             ever sees a one-frame batch (BatchNorm in train mode, full weight in a per-batch all-reduce); with
             ``drop_last`` every rank keeps ``min(shard) // batch_size`` full batches.  ``n < world`` is a ValueError
             (a rank without a frame has nothing to repeat, and a per-batch collective would hang).
             ``"pixels"``: cut points balance ``weights`` (pixels per frame; MSRA boxes vary ~3x in area): equal WORK per
             rank, for voxelization / export jobs that never synchronise per batch.  Frame and batch counts then differ
             between ranks (8 ranks over MSRA-like subjects: 7 to 15 batches of 1024).
             Default: ``"pixels"`` when ``weights`` is given, else ``"frames"``.
    """
    if balance is None:
        balance = "pixels" if weights is not None else "frames"
    if balance not in ("frames", "pixels"):
        raise ValueError("balance must be 'frames' or 'pixels'")
    if balance == "pixels" and weights is None:
        raise ValueError("balance='pixels' needs the per-frame weights")
    bounds = shard.shard_bounds(n, world, weights if balance == "pixels" else None)
    if not 0 <= rank < world:
        raise ValueError("rank out of range")
    a, b = bounds[rank]
    idx = np.arange(a, b, dtype=np.int64)
    if shuffle:
        np.random.default_rng((seed, epoch, rank)).shuffle(idx)
    if balance == "frames":
        if n < world:
            raise ValueError(f"balance='frames' needs at least one frame per rank (n={n}, world={world})")
        lens = [e - s for s, e in bounds]
        if not drop_last and idx.size < max(lens):
            idx = np.concatenate([idx, idx[:1]])      # pad at sample level: shard sizes differ by at most one
    batches = [idx[i:i + batch_size] for i in range(0, idx.size, batch_size)]
    if balance == "frames":
        if drop_last:
            batches = batches[: min(lens) // batch_size]
    elif drop_last and batches and batches[-1].size < batch_size:
        batches.pop()
    return batches


class _Staging:
    """One reusable set of pinned host buffers + device input tensors for a batch (two of them alternate)."""

    def __init__(self, max_px: int, bs: int, device, with_gt: bool, depth16: bool = False):
        # over 16-bit packs the pinned buffer and the upload's target are uint16 (half the bytes over the link); the widen
        # launch that follows the copy on the copy stream fills d_depth, and everything downstream is what it always was
        self.h_depth = torch.empty(max_px, dtype=torch.uint16 if depth16 else torch.float32).pin_memory()
        self.d_depth16 = torch.empty(max_px, dtype=torch.uint16, device=device) if depth16 else None
        self.h_off = torch.empty(bs + 1, dtype=torch.int64).pin_memory()
        self.h_hdr = torch.empty((bs, 6), dtype=torch.int32).pin_memory()
        self.h_gt = torch.empty((bs, 63), dtype=torch.float32).pin_memory() if with_gt else None
        self.d_depth = torch.empty(max_px, dtype=torch.float32, device=device)
        # offsets / headers / labels stay in the pinned buffers: the voxelizer reads them over the link (include/tsdf.h).
        # ONE copy per batch: a small copy between two big ones can halve the next big one's rate (the runtime's
        # choice of copy engine; tools/exp_loader_meta.py: 630 k vs 880 k crops/s with the same bytes).
        self.copied = torch.cuda.Event()
        self.consumed = torch.cuda.Event()
        self.filled = threading.Event()   # host side: the worker has packed a batch into the pinned buffers
        self.free = threading.Event()     # host side: the H2D copy out of the pinned buffers has been ISSUED (the
        self.free.set()                   # worker then waits for `copied` itself, off the consumer's path)
        self.used = False
        self.n = 0
        self.npx = 0
        self.src = None                   # pinned tensor to upload from (the staging buffer, or a slice of a pinned pack)


class _BatchLoader:
    """What :class:`VoxelLoader` and :class:`ResidentLoader` share: the arguments of :func:`plan_batches` and of the
    voxelizer's launch, and the epoch's batches."""

    def __init__(self, dataset: MSRADepthDataset, batch_size: int, device, res, shuffle, seed, drop_last, rank, world,
                 labels, clamp, layout, balance):
        self.balance = balance
        self.ds, self.bs, self.device, self.res = dataset, int(batch_size), torch.device(device), res
        self.shuffle, self.seed, self.drop_last = shuffle, seed, drop_last
        self.rank, self.world = rank, world
        self.labels, self.clamp, self.layout = labels, clamp, layout
        self.epoch = 0

    def _batches(self) -> List[np.ndarray]:
        return plan_batches(len(self.ds), self.bs, self.rank, self.world, self.shuffle, self.seed, self.epoch,
                            self.drop_last, self.ds.pixels() if self.balance == "pixels" else None, self.balance)

    def __len__(self) -> int:
        return len(self._batches())


class VoxelLoader(_BatchLoader):
    """Batches of voxel grids produced on the fly.

    A worker thread packs the next batch straight into one of TWO reusable pinned staging sets (no allocation
    and no ``pin_memory()`` per batch) while the GPU voxelizes and trains on the current one; uploads run on a
    side stream, the compute stream waits on an event, so H2D copies overlap the previous batch's kernels
    (BASELINE.json configs[2]).  Frames shard across ranks contiguously (:func:`plan_batches`).
    ``max_pixels`` bounds a batch's pixel count (default: ``batch_size`` full 320x240 frames).
    """

    def __init__(self, dataset: MSRADepthDataset, batch_size: int, device, res: int = 32,
                 shuffle: bool = False, seed: int = 0, drop_last: bool = False,
                 rank: int = 0, world: int = 1, labels: bool = True, clamp: bool = True,
                 max_pixels: Optional[int] = None, layout: str = "czyx", pin_packs: bool = True,
                 balance: str = "frames"):
        """``balance``: how ranks split the frames (:func:`plan_batches`): ``"frames"`` (default) gives every rank the same
        number of batches — required when the consumer synchronises per batch (DDP); ``"pixels"`` equalises the
        voxelization work instead (export jobs)."""
        super().__init__(dataset, batch_size, device, res, shuffle, seed, drop_last, rank, world, labels, clamp, layout,
                         balance)
        self.max_px = int(max_pixels) if max_pixels else self.bs * 320 * 240
        self.pin_packs = pin_packs
        self._sets: Optional[List[_Staging]] = None
        self._copy_stream = None

    def __iter__(self) -> Iterator[VoxelBatch]:
        batches = self._batches()
        self.epoch += 1
        if self._sets is None:
            self._sets = [_Staging(self.max_px, self.bs, self.device, True, getattr(self.ds, "depth_shift", None) is not None)
                          for _ in range(2)]
            if self.pin_packs:
                self.ds.pin_packs()
        sets = self._sets
        shift = getattr(self.ds, "depth_shift", None)   # 16-bit packs: upload uint16, widen on the copy stream
        for s in sets:
            if s.used:
                s.consumed.synchronize()   # an abandoned previous epoch may still be reading this set
            s.free.set()
            s.filled.clear()
            s.used = False
        err: "queue.Queue" = queue.Queue()
        stop = threading.Event()

        def work():
            try:
                for k, b in enumerate(batches):
                    s = sets[k & 1]
                    while not s.free.wait(0.05):
                        if stop.is_set():
                            return
                    s.free.clear()
                    if s.used:
                        s.consumed.synchronize()   # the kernel that read this set's pinned metadata (and therefore
                                                   # the upload out of its pinned depth buffer) is done
                    direct = self.ds.contiguous_source(b)
                    if direct is not None:            # DMA straight out of the pinned pack: no staging copy
                        s.src, pk = direct
                    else:
                        pk = self.ds.take(b, s.h_depth.numpy())
                        s.src = s.h_depth[: pk.depth.size]
                    if pk.depth.size > self.max_px:
                        raise ValueError(f"batch of {pk.depth.size} pixels exceeds max_pixels={self.max_px}")
                    s.n, s.npx = len(pk), int(pk.depth.size)
                    s.h_off.numpy()[: s.n + 1] = pk.offsets
                    s.h_hdr.numpy()[: s.n] = pk.headers
                    s.h_gt.numpy()[: s.n] = pk.gt
                    s.filled.set()
            except BaseException as e:  # surface I/O errors in the consumer
                err.put(e)
                for s in sets:
                    s.filled.set()

        t = threading.Thread(target=work, daemon=True)
        t.start()
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        copy_stream = self._copy_stream
        try:
            for k in range(len(batches)):
                # the stream the consumer is on NOW: a generator may be resumed under another torch.cuda.stream(...)
                # context than the one it was started in, and the launch below goes to whatever is current
                cur = torch.cuda.current_stream(self.device)
                s = sets[k & 1]
                s.filled.wait()
                if not err.empty():
                    raise err.get()
                s.filled.clear()
                n, npx = s.n, s.npx
                with torch.cuda.stream(copy_stream):
                    if k >= 2:
                        copy_stream.wait_event(s.consumed)   # the kernels that read this device set are done
                    if shift is None:
                        s.d_depth[:npx].copy_(s.src, non_blocking=True)
                    else:   # the one H2D copy at half the bytes, then the widen into d_depth, both on the copy stream
                        s.d_depth16[:npx].copy_(s.src, non_blocking=True)
                        widen_depth16(s.d_depth16[:npx], shift, out=s.d_depth[:npx])
                    s.copied.record(copy_stream)
                cur.wait_event(s.copied)
                # one launch: volumes, max_l / mid_p, normalised labels and the labels' device copy (which outlives the set)
                out, gt_nor, gt = voxelize_labels(s.d_depth[:npx], s.h_off[: n + 1], s.h_hdr[:n], s.h_gt[:n], res=self.res,
                                                  layout=self.layout, clamp=self.clamp, gt_copy=True)
                if not self.labels:
                    gt_nor = None
                s.consumed.record(cur)
                s.used = True
                s.free.set()   # issued: the worker may reuse the pinned buffers once `consumed` has fired
                yield VoxelBatch(out.tsdf, gt, out.max_l, out.mid_p, out.status, gt_nor)
        finally:
            stop.set()
            t.join()


class ResidentPacks:
    """The packs of a pack-backed dataset, uploaded to the GPU once: ``depth``, ``offsets[G+1]``, ``headers[G,6]``,
    ``gt[G,63]`` over the G frames of all packs back to back, and ``frame[d]`` = which of them dataset item d is."""

    def __init__(self, dataset: MSRADepthDataset, device):
        if not dataset.packed:
            raise ValueError("a resident dataset needs packs (packing.pack_tree + packed_dir=, or from_packs)")
        packs = dataset.packs
        px = np.array([int(pk.depth.size) for pk in packs], np.int64)
        nf = np.array([len(pk) for pk in packs], np.int64)
        pbase = np.concatenate([[0], np.cumsum(px)])
        fbase = np.concatenate([[0], np.cumsum(nf)])
        self.depth = torch.empty(int(pbase[-1]), dtype=torch.float32, device=device)
        with warnings.catch_warnings():      # (a memory-mapped pack is read-only: torch warns, and we only read)
            warnings.simplefilter("ignore", UserWarning)
            for k, pk in enumerate(packs):   # (a memory-mapped pack is read here, once)
                dst = self.depth[int(pbase[k]):int(pbase[k + 1])]
                if pk.depth_shift is None:
                    dst.copy_(torch.from_numpy(np.ascontiguousarray(pk.depth)))
                else:   # a 16-bit pack goes up as uint16 and is widened into its slice; the temporary is then dropped
                    tmp = torch.from_numpy(np.ascontiguousarray(pk.depth)).to(self.depth.device)
                    widen_depth16(tmp, pk.depth_shift, out=dst)
                    del tmp
        off = np.concatenate([np.asarray(pk.offsets[:-1], np.int64) + pbase[k] for k, pk in enumerate(packs)]
                             + [pbase[-1:]])
        hdr = np.concatenate([np.asarray(pk.headers, np.int32).reshape(-1, 6) for pk in packs])
        gt = np.concatenate([np.asarray(pk.gt, np.float32).reshape(len(pk), -1) if pk.gt is not None
                             else np.zeros((len(pk), 63), np.float32) for pk in packs])
        self.offsets = torch.from_numpy(off).to(device)
        self.headers = torch.from_numpy(np.ascontiguousarray(hdr)).to(device)
        self.gt = torch.from_numpy(np.ascontiguousarray(gt)).to(device)
        self.frame = fbase[dataset._pack_of] + dataset._local

    def nbytes(self) -> int:
        return 4 * self.depth.numel()


class ResidentLoader(_BatchLoader):
    """Batches of voxel grids from a dataset that LIVES ON THE GPU.

    All of MSRA is 76.5 k crops = 4.8 GB; an MI355X has 288 GB.  So instead of feeding crops over the link batch after
    batch (:class:`VoxelLoader`: PCIe-bound, and for shuffled batches bound by the host's gather) the packs are uploaded
    ONCE and every batch is drawn by index on the device (``tsdf_voxelize_indexed_hip``): a training step sends n frame
    indices, nothing else.  Same arguments, same batches (:func:`plan_batches`) and same :class:`VoxelBatch` as
    ``VoxelLoader``; the dataset must be pack-backed (``MSRADepthDataset(packed_dir=...)`` / ``from_packs``).

    ``prefetch=k`` (k > 1) takes the host out of the step for SMALL batches — the reference trains with batch 16
    (3D_CNN/train.py:36), where one launch per batch is bound by Python, not by the GPU: the epoch's permutation is
    uploaded once, ONE launch voxelizes k consecutive batches (k*batch_size frames: the fused kernel's regime) into a
    ring buffer, and the loader yields k prebuilt ``batch_size``-frame views of it.  The batches are the same frames in
    the same order with the same values as with ``prefetch=1``; what changes is their lifetime: a batch's tensors are
    views of a ring of ``ring`` blocks and are overwritten once ``(ring - 1) * k`` further batches have been drawn (on the
    stream that was current when the block was launched — a consumer on that stream can never observe the overwrite;
    clone what you keep).  ``augment=True`` draws its maps per batch exactly as without prefetch.  The ``augment`` draws
    use numpy's ``Generator`` seeded per (seed, epoch, rank, batch): the reference's distributions, not its legacy stream.

    ``augment="device"`` draws the maps on the GPU instead (:func:`voxelize.aug_xforms`, one small launch before the
    voxelizer's, on the same stream): the grid centres stay on the device, nothing is drawn, inverted or copied on the
    host.  Frame p of the rank's epoch (its position in the flat order of the epoch's batches) draws from
    ``(augment.device_key(seed, epoch, rank), p)``, so the batches do not depend on ``prefetch``.  Same distributions as
    ``augment=True``, another stream of draws.

    ``graph=True`` (with ``augment="device"`` and ``prefetch=1``) sends every full batch through one
    :class:`voxelize.AugmentedStep`: the two launches of the step are captured once and replayed, the batch's frame
    numbers and ``{key, counter}`` go up in one small copy.  The batches equal those of ``graph=False`` bit for bit; their
    tensors are the step's static outputs, valid until the next batch is drawn (clone what you keep).  The epoch's short
    last batch takes the eager path.

    ``frame="obb"`` cuts every volume in its cloud's own principal axes instead of the camera's (the oriented bounding box
    of hand-pose pipelines; include/tsdf_obb.h): the maps of all resident frames are computed once after the upload
    (:func:`voxelize.obb_xforms`, one launch) into the resident table ``loader.obb`` (float64[N,24], with
    ``loader.obb_status``), every batch gathers its rows by the batch's index on the device and goes through the indexed
    augmented entry.  The yielded ``gt`` are the joints in the mapped frame and ``gt_nor`` their labels, as with
    ``augment``; the map is rigid, so pose error is what it is in the camera frame, and
    ``transform_joints(pred, invert_xforms(loader.obb[index]))`` carries predictions back.  The default ``"camera"`` is the
    loader without it, bit for bit.  ``frame="obb"`` does not combine with ``augment`` or ``graph=True`` HERE: the
    augmentation in the principal-axis frame is ``voxelize.AugmentedStep(..., base=obb_xforms(...).xforms)`` on
    :class:`ResidentPacks` (the two maps composed on the device; include/tsdf_mapstep.h).

    ``volume_dtype=torch.float16`` / ``torch.bfloat16`` yields the volumes in that type, written once at half the bytes
    (:func:`voxelize.voxelize_grid_lowp`; include/tsdf_lowp.h) — what a network under autocast reads, and half the ring of a
    prefetching loader.  One :func:`voxelize.aabb` launch after the upload places every resident frame's grid into resident
    tables (grid rows, ``max_l``, ``mid_p``, ``status``); the epoch's permutation goes up once, every batch (``prefetch=k``:
    every block of k batches, into a ring of low-precision blocks) is one voxel launch with its slice of it, ``max_l`` /
    ``mid_p`` / ``status`` / ``gt`` are gathered by ``index_select`` and the labels come from :func:`normalize_joints`
    (0.5 for a frame that is not OK, as the fused entry writes).  Everything but ``tsdf`` equals the float32 loader's batch
    bit for bit; ``tsdf`` is the float32 volume narrowed by round-to-nearest-even, up to the contract's 1e-5.  It does not
    combine with ``augment``, ``frame="obb"`` or ``graph=True``.  The default ``None`` is the loader without it.
    """

    def __init__(self, dataset: MSRADepthDataset, batch_size: int, device, res: int = 32, shuffle: bool = False,
                 seed: int = 0, drop_last: bool = False, rank: int = 0, world: int = 1, labels: bool = True,
                 clamp: bool = True, layout: str = "czyx", augment: Union[bool, str] = False, balance: str = "frames",
                 prefetch: int = 1, ring: int = 2, graph: bool = False, frame: str = "camera",
                 volume_dtype: Optional[torch.dtype] = None):
        """``augment=True``: every frame of every batch gets a fresh 3-D augmentation with the reference's distributions
        (``augment.random_affines``, pre/process.py:209-216) about its own un-augmented grid centre, fused into the
        voxelizer (BASELINE configs[4]); the yielded ``gt`` are then the mapped joints, ``gt_nor`` their labels.
        ``augment="device"``: the same, with the maps drawn on the GPU (class docstring).
        ``balance``: see :func:`plan_batches` (``"frames"``: every rank yields the same number of batches)."""
        if frame not in ("camera", "obb"):
            raise ValueError(f"frame must be 'camera' or 'obb', got {frame!r}")
        if frame == "obb" and (augment or graph):
            raise ValueError("frame='obb' does not combine with augment or graph=True (the two maps are not composed)")
        if volume_dtype is not None:
            _lowp_dtype(volume_dtype)
            if augment or graph or frame == "obb":
                raise ValueError("volume_dtype does not combine with augment, frame='obb' or graph=True (the low-precision "
                                 "voxel pass is the plain one)")
        if not dataset.packed:
            raise ValueError("ResidentLoader needs a pack-backed dataset (packing.pack_tree + packed_dir=, or from_packs)")
        if prefetch < 1 or ring < 2:
            raise ValueError("prefetch must be >= 1 and ring >= 2")
        if isinstance(augment, str) and augment != "device":
            raise ValueError(f"augment must be False, True or 'device', got {augment!r}")
        if graph is not False and graph is not True:
            raise ValueError(f"graph must be False or True, got {graph!r}")
        if graph and (augment != "device" or prefetch != 1):
            raise ValueError("graph=True replays the augmented step: it needs augment='device' and prefetch=1")
        self.augment = bool(augment)
        self.device_draws = augment == "device"
        self.graph = graph
        self.frame = frame
        self.obb = None          # frame="obb": the maps of all resident frames, float64[N,24] on the device
        self.obb_status = None   # ... and their status, int32[N]
        self._step = None  # graph=True: the AugmentedStep of full batches
        self.volume_dtype = volume_dtype
        self._lowp = None        # volume_dtype: (grid rows, max_l, mid_p, status) of all resident frames
        self._lowp_ring = None   # ... and with prefetch > 1 the ring of low-precision volume blocks
        self._mapped = self.augment or frame == "obb"   # every launch takes one map per frame (_maps)
        self.prefetch, self.ring = int(prefetch), int(ring)
        super().__init__(dataset, batch_size, device, res, shuffle, seed, drop_last, rank, world, labels, clamp, layout,
                         balance)
        self._dev = None   # (depth, offsets, headers, gt) of all packs, on the device
        self._g = None     # dataset frame -> frame of the concatenated packs
        self._idx = None   # two pinned index buffers + the events of the launches that read them
        self._blocks = None  # prefetch > 1: the ring of output blocks and their prebuilt batch views

    def resident_bytes(self) -> int:
        return sum(4 * int(pk.depth.size) for pk in self.ds.packs)

    def _upload(self):
        rp = ResidentPacks(self.ds, self.device)
        self._dev = (rp.depth, rp.offsets, rp.headers, rp.gt)
        self._g = rp.frame
        # (batches of up to 32 frames hand their index over by value — tsdf_voxelize_indexed_host_hip —, which an ordinary
        # CPU tensor selects in voxelize_indexed; larger ones, and augmented ones, are read from page-locked memory)
        pin = self.bs > _lib.INLINE_INDEX_MAX or self._mapped
        self._idx = [(torch.empty(self.bs, dtype=torch.int64).pin_memory() if pin else torch.empty(self.bs, dtype=torch.int64),
                      torch.cuda.Event()) for _ in range(2)]
        self._used = [False, False]
        self._mid = None
        if self.frame == "obb":   # every resident frame's map, once: one launch over the pack
            ob = obb_xforms(rp.depth, rp.offsets, rp.headers)
            self.obb, self.obb_status = ob.xforms, ob.status
        if self.volume_dtype is not None:   # every resident frame's grid placement, once: one AABB launch over the pack
            self._lowp = _place_aabb(rp.depth, rp.offsets, rp.headers, self.res)
        if self.augment:   # the centres the maps turn about: every frame's own grid centre, one AABB launch over the pack
            mid = aabb(rp.depth, rp.offsets, rp.headers, res=self.res).grid[:, :3]
            if self.device_draws:   # the centres stay where the launch left them; one map buffer per launch in flight
                self._mid = mid.contiguous()
                self._xf = torch.empty((self.ring if self.prefetch > 1 else 2, self.bs * self.prefetch, 24),
                                       dtype=torch.float64, device=self.device)
            else:
                self._mid = mid.cpu().numpy().astype(np.float64)
                self._xf = [torch.empty((self.bs, 24), dtype=torch.float64).pin_memory() for _ in range(2)]

    def __iter__(self) -> Iterator[VoxelBatch]:
        batches = self._batches()
        self.epoch += 1
        if self._dev is None:
            self._upload()
        if self.volume_dtype is not None:
            return self._iter_lowp(batches)
        if self.prefetch > 1:
            return self._iter_blocks(batches, self.epoch)
        return self._iter_single(batches, self.epoch)

    def _iter_lowp(self, batches) -> Iterator[VoxelBatch]:
        """volume_dtype: one low-precision voxel launch per block of ``prefetch`` batches over the resident grid rows; the
        per-frame fields are gathered from the resident tables.  ``prefetch=1`` allocates every batch's volume, ``k > 1``
        writes into a ring of blocks whose batches are views (lifetime as in the class docstring)."""
        depth, off, hdr, gt = self._dev
        rows, max_l, mid_p, status = self._lowp
        if not batches:
            return
        bs, P, R = self.bs, self.prefetch, self.res
        if P > 1 and self._lowp_ring is None:
            self._lowp_ring = [torch.empty((bs * P, 3, R, R, R), dtype=self.volume_dtype, device=self.device)
                               for _ in range(self.ring)]
        d_idx = torch.from_numpy(np.ascontiguousarray(self._g[np.concatenate(batches)])).to(self.device)
        pos = 0
        for blk, k0 in enumerate(range(0, len(batches), P)):
            mine = batches[k0:k0 + P]
            nfr = int(sum(b.size for b in mine))
            idx = d_idx[pos:pos + nfr]
            pos += nfr
            out = self._lowp_ring[blk % self.ring][:nfr] if P > 1 else None
            tsdf, _ = voxelize_grid_lowp(depth, off, hdr, rows, res=R, layout=self.layout, dtype=self.volume_dtype,
                                         index=idx, out=out)
            ml, mp, st = max_l.index_select(0, idx), mid_p.index_select(0, idx), status.index_select(0, idx)
            g = gt.index_select(0, idx)
            gt_nor = None
            if self.labels:
                gt_nor = normalize_joints(g, ml, mp, clamp=self.clamp)
                bad = (st != _lib.TSDF_FRAME_OK).reshape((-1,) + (1,) * (g.dim() - 1))
                gt_nor = torch.where(bad, torch.full_like(gt_nor, 0.5), gt_nor)
            a = 0
            for b in mine:
                e = a + int(b.size)
                yield VoxelBatch(tsdf[a:e], g[a:e], ml[a:e], mp[a:e], st[a:e], gt_nor[a:e] if self.labels else None)
                a = e

    def _epoch_key(self, epoch: int) -> int:
        """augment="device": the key the epoch's frames draw under (their counters are their places in the epoch)."""
        return augment.device_key(self.seed, epoch, self.rank) if self.device_draws else 0

    def _host_draw(self, gidx: np.ndarray, batches, epoch: int, k0: int = 0) -> np.ndarray:
        """augment=True: the maps of batches ``k0, k0 + 1, ...`` of the epoch (``gidx``: their pack frames back to back),
        one generator per batch, so that a batch's maps do not depend on ``prefetch``."""
        xf = np.empty((gidx.size, 24), np.float64)
        pos = 0
        for k, b in enumerate(batches, k0):
            xf[pos:pos + b.size] = augment.random_affines(self._mid[gidx[pos:pos + b.size]],
                                                          rng=(self.seed, epoch, self.rank, k))[0]
            pos += b.size
        return xf

    def _maps(self, index: torch.Tensor, slot: int, key: int, pos: int, drawn: Optional[torch.Tensor]):
        """The maps of one launch over pack frames ``index``: its rows of the resident OBB table (``index`` on the device),
        a device draw into map buffer ``slot`` (on the launch stream; the buffer's last reader is the voxelizer launch
        before the slot came round again) with the counters of epoch positions ``pos, pos + 1, ...``, or what the host
        drew (``drawn``, on the device: the maps are read per voxel)."""
        if self.frame == "obb":
            return self.obb.index_select(0, index)
        if self.device_draws:
            return aug_xforms(self._mid, index=index, key=key, counter0=pos, out=self._xf[slot, :index.numel()])
        return drawn

    def _iter_single(self, batches, epoch) -> Iterator[VoxelBatch]:
        depth, off, hdr, gt = self._dev
        key, pos = self._epoch_key(epoch), 0
        for k, b in enumerate(batches):
            cur = torch.cuda.current_stream(self.device)   # (per batch: the consumer may have switched streams)
            h_idx, done = self._idx[k & 1]
            if self._used[k & 1]:
                done.synchronize()          # the launch that read this index buffer two batches ago
            n = int(b.size)
            gidx = self._g[b]
            if self.graph and n == self.bs:   # the captured step: index and {key, counter} in, its static outputs out
                if self._step is None:
                    self._step = AugmentedStep(depth, off, hdr, n, gt=gt, centres=self._mid, res=self.res,
                                               layout=self.layout, clamp=self.clamp)
                out, gt_nor, g = self._step.step(gidx, key, pos)
            else:
                h_idx.numpy()[:n] = gidx
                xf, idx = None, h_idx[:n]
                if self._mapped:
                    drawn = None
                    if self.frame == "obb":   # the table's rows are gathered by the batch's index on the device
                        idx = idx.to(self.device, non_blocking=True)
                    elif not self.device_draws:
                        h_xf = self._xf[k & 1]
                        h_xf.numpy()[:n] = self._host_draw(gidx, (b,), epoch, k)
                        drawn = h_xf[:n].to(self.device, non_blocking=True)
                    xf = self._maps(idx, k & 1, key, pos, drawn)
                out, gt_nor, g = voxelize_indexed(depth, off, hdr, idx, gt, res=self.res, layout=self.layout,
                                                  clamp=self.clamp, gt_copy=True, xforms=xf)
                done.record(cur)
                self._used[k & 1] = True
            pos += n
            yield VoxelBatch(out.tsdf, g, out.max_l, out.mid_p, out.status, gt_nor if self.labels else None)

    # ---- prefetch > 1: one launch per block of `prefetch` batches ----
    def _make_blocks(self):
        depth, off, hdr, gt = self._dev
        cap, R = self.bs * self.prefetch, self.res
        lab_shape = (cap,) + tuple(gt.shape[1:])
        blocks = []
        for _ in range(self.ring):
            out = empty_batch(cap, R, self.device)
            gt_nor = torch.empty(lab_shape, dtype=torch.float32, device=self.device)
            g = torch.empty(lab_shape, dtype=torch.float32, device=self.device)
            views = [self._view(out, gt_nor, g, j * self.bs, (j + 1) * self.bs) for j in range(self.prefetch)]
            blocks.append((out, gt_nor, g, views))
        return blocks

    def _view(self, out, gt_nor, g, a, b) -> VoxelBatch:
        return VoxelBatch(out.tsdf[a:b], g[a:b], out.max_l[a:b], out.mid_p[a:b], out.status[a:b],
                          gt_nor[a:b] if self.labels else None)

    def _iter_blocks(self, batches, epoch) -> Iterator[VoxelBatch]:
        depth, off, hdr, gt = self._dev
        if self._blocks is None:
            self._blocks = self._make_blocks()
        if not batches:
            return
        bs, P = self.bs, self.prefetch
        # the epoch's permutation goes up once; a launch reads its slice of it
        flat = np.concatenate(batches)
        gidx = self._g[flat]
        d_idx = torch.from_numpy(np.ascontiguousarray(gidx)).to(self.device)
        key = self._epoch_key(epoch)
        d_xf = None
        if self.augment and not self.device_draws:
            d_xf = torch.from_numpy(self._host_draw(gidx, batches, epoch)).to(self.device)
        pos = 0
        for blk, k0 in enumerate(range(0, len(batches), P)):
            mine = batches[k0:k0 + P]
            nfr = int(sum(b.size for b in mine))
            out, gt_nor, g, views = self._blocks[blk % self.ring]
            full = nfr == bs * P
            if full:
                o, gn, gg = out, gt_nor, g
            else:      # the epoch's last block: the leading part of the ring entry
                o = TsdfBatch(out.tsdf[:nfr], out.max_l[:nfr], out.mid_p[:nfr], out.status[:nfr])
                gn, gg = gt_nor[:nfr], g[:nfr]
            idx, xf = d_idx[pos:pos + nfr], None
            if self._mapped:
                xf = self._maps(idx, blk % self.ring, key, pos, None if d_xf is None else d_xf[pos:pos + nfr])
            voxelize_indexed(depth, off, hdr, idx, gt, res=self.res, layout=self.layout, clamp=self.clamp,
                             out=o, out_gt_nor=gn, out_gt=gg, xforms=xf)
            pos += nfr
            if full:
                yield from views
            else:
                a = 0
                for b in mine:
                    yield self._view(out, gt_nor, g, a, a + int(b.size))
                    a += int(b.size)


class PreBatched:
    """What :meth:`MSRA_Dataset.__getitems__` hands to torch's DataLoader: the batch, ALREADY batched.  torch's
    ``default_collate`` dispatches on the type of ``batch[0]``; this type is registered with it (below), so the list
    ``[PreBatched(batch)]`` collates to ``batch`` itself — no per-item views, no ``torch.stack``."""

    __slots__ = ("batch",)

    def __init__(self, batch):
        self.batch = batch


def _collate_prebatched(batch, *, collate_fn_map=None):
    return batch[0].batch


try:   # the documented extension point of torch.utils.data.default_collate
    from torch.utils.data._utils.collate import default_collate_fn_map as _collate_map
    _collate_map[PreBatched] = _collate_prebatched
except ImportError:   # pragma: no cover  (a torch without the map: MSRA_Dataset(prebatched=False) still works)
    _collate_map = None


class _SlotGuard:
    """Who else holds a ring slot's batch?  Two counts per tensor, compared with what they were when only the ring held
    the slot:

      * the Python reference count of the batch tuple and of each of its tensors — a consumer that keeps the tuple, one
        tensor object, or anything that keeps those objects alive (a dlpack capsule, a closure, a frame a debugger or
        ``sys.settrace`` hook holds on to);
      * the use count of each tensor's STORAGE (``torch._C._storage_Use_Count``) — every other tensor object over the same
        memory: a view (``t[:, 1]``), ``t.detach()``, ``t.data``, ``t.numpy()``, a tensor autograd saved for backward.
        (Round 4 relied on a live view bumping its base tensor's Python reference count — a torch-internal side effect —
        and did not see ``detach()`` / ``.data`` aliases at all: ADVICE round 4.)

    Equality with the baseline means "only the ring"; ANY difference means "held" and the slot gets fresh tensors, so an
    unexpected extra reference (a profiler, a different Python) costs an allocation, never a wrong batch.  What no count can
    see is a consumer that dropped every reference but still has work queued on ANOTHER stream: order that stream after
    the loader's (the usual rule for GPU tensors).  :func:`_slot_guard_works` checks the counting rules themselves once
    per process; a torch on which they do not hold makes the ring hand out fresh tensors for every batch."""

    __slots__ = ("batch", "_stor", "_cdata", "_base")

    def __init__(self, batch):
        self.batch = batch
        self._stor = tuple(t.untyped_storage() for t in batch)   # (kept: a wrapper's _cdata is only valid while it lives)
        self._cdata = tuple(s._cdata for s in self._stor)
        self._base = None

    def counts(self):
        rc, uc, b, c = sys.getrefcount, _storage_use_count, self.batch, self._cdata
        if len(c) == 5:   # (full mode: the batch also carries gt_pca, which a consumer may hold on its own)
            return (rc(b), rc(b[0]), rc(b[1]), rc(b[2]), rc(b[3]), rc(b[4]), uc(c[0]), uc(c[1]), uc(c[2]), uc(c[3]),
                    uc(c[4]))
        return (rc(b), rc(b[0]), rc(b[1]), rc(b[2]), rc(b[3]), uc(c[0]), uc(c[1]), uc(c[2]), uc(c[3]))

    def arm(self):
        """Call when every reference the ring itself keeps is in place and no local of the caller refers to the batch."""
        self._base = self.counts()

    def held(self) -> bool:
        return self.counts() != self._base


_storage_use_count = getattr(torch._C, "_storage_Use_Count", None)
_guard_ok: Optional[bool] = None


def _slot_guard_works() -> bool:
    """The counting rules _SlotGuard relies on, tried once on small CPU tensors: a kept tuple, a kept tensor, a view, a
    ``detach()`` alias, a ``.data`` alias and a numpy alias must each read as "held", and dropping them as "free"."""
    global _guard_ok
    if _guard_ok is None:
        ok = _storage_use_count is not None
        if ok:
            try:
                holder = [PreBatched(tuple(torch.zeros(2, 3) for _ in range(4)))]
                g = _SlotGuard(holder[0].batch)
                g.arm()
                ok = not g.held()
                for make in (lambda b: b, lambda b: b[1], lambda b: b[0][:, 1], lambda b: b[2].detach(), lambda b: b[3].data,
                             lambda b: b[0].numpy()):
                    ref = make(holder[0].batch)
                    ok = ok and g.held()
                    del ref
                    ok = ok and not g.held()
            except Exception:   # pragma: no cover  (an API that moved)
                ok = False
        _guard_ok = bool(ok)
    return _guard_ok


class MSRA_Dataset(data.Dataset):
    """The reference's dataset class with its constructor and item tuple (3D_CNN/dataset.py:16-79):

        MSRA_Dataset(root_path, opt, train=True, aug=False)[i] -> (tsdf[3,32,32,32], gt[63], max_l, mid_p)

    but ``root_path`` is the RAW MSRA tree (or a directory of packs, see ``packed_dir``), nothing is preprocessed
    and nothing but the depth crops is held in host memory: items are voxelized on the GPU in blocks of
    ``block`` consecutive frames the first time one of them is asked for, and returned as GPU tensors (the
    reference returns numpy rows that its training loop then moves with ``.cuda()``, train.py:200,232).
    ``opt.size`` / ``opt.test_index`` are honoured when present (the reference ignores ``opt`` and hard-codes
    ``'small'`` / 2, :20-22).

    ``aug=True`` (3D_CNN/dataset.py:57-62: "add augmentation dataset") appends an AUGMENTED rendition of every frame the
    dataset holds: items ``[n, 2n)`` are frames ``[0, n)`` under a fixed per-frame 3-D augmentation, drawn once with the
    reference's distributions (``augment.draw_params(n, aug_seed)``) about the frame's own un-augmented grid centre and
    FUSED into the voxelizer (the re-specified contract of ``tsdf_voxelize_aug_hip``; the reference's own ``_aug`` files
    cannot be produced — ``data_aug`` raises AxisError — and its loader reads the plain files again for them, SURVEY.md
    App. B#8,#11).  The item's ``gt`` are the joints under the same map, ``max_l`` / ``mid_p`` those of the augmented
    grid.  With ``aug=True`` every batch goes through the augmented entry — plain items with the identity map, whose
    volumes equal the plain entry's to the float32 rounding (grid, zero mask, sign and z component bit for bit).

    ``aug="device"``: the same items, with the maps drawn on the GPU.  The augmented twin of frame g draws from
    ``(augment.device_key(aug_seed, 0, 0), g)`` — a function of ``(aug_seed, g)`` alone, whatever batch the item appears in
    (``augment.device_draws_np(key, [g])`` restates it): the same distributions as ``aug=True``, another stream of draws.
    Nothing is drawn on the host and there is no table of maps: the grid centres stay on the device and one small launch
    per batch (:func:`voxelize.aug_xforms_at`, counters ``item mod n``) writes the batch's maps before the voxelizer's;
    plain items get the identity map from the same launch.

    Under the reference's own ``DataLoader(dataset, batch_size=B, shuffle=True)`` (train.py:36,86-91; ``num_workers=0``:
    the items are GPU tensors) the loader hands the batch's indices to :meth:`__getitems__`, which voxelizes exactly
    those B frames in ONE launch and returns them ALREADY BATCHED (``prebatched=True``, the default on a resident
    dataset): the indices go into a page-locked ring the kernel reads over the link, the outputs into a ring of
    preallocated batches, and the result is a :class:`PreBatched` that torch's ``default_collate`` unwraps — the host
    side of a step is one index conversion and one C call.  What the ``DataLoader`` yields is the reference's collated
    batch ``(tsdf[B,3,32,32,32], gt[B,63], max_l[B], mid_p[B,3])``, on the GPU.  The ring (``ring`` slots; default: as
    many batches as fit 2 GiB of volumes, between 2 and 256) recycles a slot's tensors only when the consumer holds no
    reference to that batch any more — a batch that is kept (``list(dl)``, collected outputs, a view of one tensor) keeps
    its tensors and the slot gets new ones, so the loader behaves like the reference's, which returns independent
    tensors.  With a custom ``collate_fn`` pass ``prebatched=False``: a list of
    item tuples, views into the batch's tensors, as torch documents for ``__getitems__``.
    A lone ``dataset[i]`` voxelizes frame i alone unless the access pattern is a sequential walk, which is served
    from a block.  For the highest throughput at small batch sizes use :class:`ResidentLoader` with ``prefetch``: it
    knows the epoch's permutation in advance, which nothing behind ``DataLoader`` can.
    """

    def __init__(self, root_path, opt=None, train=True, aug=False, device="cuda", block: int = 1024,
                 packed_dir: Optional[str] = None, resident: Optional[bool] = None, prebatched: Optional[bool] = None,
                 ring: Optional[int] = None, aug_seed: int = 0, _raw: Optional[MSRADepthDataset] = None, pca=None):
        if isinstance(aug, str) and aug != "device":
            raise ValueError(f"aug must be False, True or 'device', got {aug!r}")
        self.AUG = bool(aug)
        self.aug_device = aug == "device"
        self.aug_seed = aug_seed
        self.size = getattr(opt, "size", "small")
        self.test_idx = int(getattr(opt, "test_index", 2))
        self.PCA_SZ = int(getattr(opt, "PCA_SZ", 63))
        self.train = train
        self.raw = _raw if _raw is not None else MSRADepthDataset(root_path, train=train, test_idx=self.test_idx,
                                                                  size=self.size, packed_dir=packed_dir)
        self.device = torch.device(device)
        self.block = int(block)
        self._cache_block = -1
        self._cache: Optional[TsdfBatch] = None
        self._cache_gt: Optional[torch.Tensor] = None
        self._last = -1          # the last index served (a sequential walk is answered from blocks)
        # resident (default: whenever the dataset is pack-backed): the packs go to the GPU once and a batch is a list of
        # indices resolved on the device (tsdf_voxelize_indexed_hip) — no crop crosses the link after start-up
        self.resident = self.raw.packed if resident is None else bool(resident)
        self.prebatched = (self.resident and _collate_map is not None) if prebatched is None else bool(prebatched)
        if self.prebatched and not self.resident:
            raise ValueError("prebatched=True needs a resident (pack-backed) dataset")
        self._ring_req = ring
        self._rp: Optional[ResidentPacks] = None
        self._fast = None        # the ring of the pre-batched path (built on the first batch)
        self._n = len(self.raw)
        self._aug_params = None  # aug=True: (stretch, rot_xy, rot_z) of every frame, drawn once
        self._xf_table = None    # ... and, resident, the maps of all 2n items (identity for the first n), float64[2n,24]
        self._aug_key = 0        # aug="device": the key every augmented item draws under; its counter is the frame number
        self._aug_state = None   # ... {key, 0} on the device, and the grid centres of the resident packs' frames
        self._aug_mid = None
        if self.aug_device:
            self._aug_key = augment.device_key(aug_seed, 0, 0)
        elif self.AUG:
            self._aug_params = augment.draw_params(self._n, aug_seed)
        # full mode (3D_CNN/dataset.py:165-180): the joint-PCA basis, and gt_pca as the item's fifth element
        self.pca = None
        self._cache_pca: Optional[torch.Tensor] = None
        if pca is not None and pca is not False:
            if pca is True:
                if not train:
                    raise ValueError("pca=True fits on a TRAINING dataset; pass the training set's basis (its .pca, a "
                                     "JointPCA or a path) to a test dataset")
                basis = fit_joint_pca(self)
            elif isinstance(pca, JointPCA):
                basis = pca
            else:
                basis = JointPCA.load(os.fspath(pca))
            basis.check_k(self.PCA_SZ)
            self.pca = basis.to(self.device)
            # the shapes with which the reference's own decode, torch.addmm(PCA_mean.expand(b, C), est, PCA_coeff)
            # (3D_CNN/train.py:221-225), is mu + p W^T
            self.PCA_mean, self.PCA_coeff = basis.torch_decode_args(self.PCA_SZ, self.device)

    @classmethod
    def from_raw(cls, raw: MSRADepthDataset, device="cuda", **kw) -> "MSRA_Dataset":
        """The on-the-fly dataset over raw frames that are already open (``MSRADepthDataset`` / ``from_packs``)."""
        return cls(None, device=device, _raw=raw, **kw)

    def __len__(self):
        return 2 * self._n if self.AUG else self._n

    def _resident_packs(self) -> "ResidentPacks":
        if self._rp is None:
            self._rp = ResidentPacks(self.raw, self.device)
            if self.AUG:   # every frame's own grid centre (one AABB launch over the pack), then all maps at once
                rp = self._rp
                mid = aabb(rp.depth, rp.offsets, rp.headers).grid[:, :3]
                self._frame2 = np.ascontiguousarray(np.concatenate([rp.frame, rp.frame]))
                if self.aug_device:   # the centres stay on the device; an item's row of these two tables goes to the draw
                    self._aug_mid = mid.contiguous()
                    self._draw_frame = np.ascontiguousarray(np.concatenate([np.full(self._n, -1, np.int64), rp.frame]))
                    self._draw_counter = np.ascontiguousarray(np.tile(np.arange(self._n, dtype=np.int64), 2))
                else:
                    mid = mid.cpu().numpy().astype(np.float64)[rp.frame]
                    self._xf_table = np.ascontiguousarray(np.concatenate(
                        [augment.identity_affines(self._n), augment.affines_from_params(mid, *self._aug_params)]))
        return self._rp

    def _device_state(self) -> torch.Tensor:
        if self._aug_state is None:
            self._aug_state = aug_state(self._aug_key, 0, self.device)
        return self._aug_state

    def _device_maps(self, idx: np.ndarray) -> torch.Tensor:
        """aug="device", resident: the maps of items ``idx`` (identity for the plain ones), one launch."""
        return aug_xforms_at(self._aug_mid, self._device_state(),
                             index=torch.from_numpy(self._draw_frame[idx]).to(self.device),
                             counters=torch.from_numpy(self._draw_counter[idx]).to(self.device))

    def _voxelize_items(self, idx: np.ndarray, clamp: bool = True):
        """Items ``idx`` as device tensors, by one voxelizer launch: ``(TsdfBatch, gt, gt_nor, gt_pca)``.  ``gt_nor`` are the
        launch's labels (clamped unless ``clamp=False``; None from the plain entry, which writes none), ``gt_pca`` is None
        without a basis.  With ``aug`` the launch is the augmented entry — plain items under the identity map — and
        ``gt`` are the mapped joints."""
        dev = self.device
        kw = {} if self.pca is None else {"pca": self.pca, "k": self.PCA_SZ}
        if self.resident:   # the batch is drawn by index from the packs on the device
            rp = self._resident_packs()
            xf = None
            if self.aug_device:
                xf = self._device_maps(idx)
            elif self.AUG:
                xf = torch.from_numpy(self._xf_table[idx]).to(dev)
            frame = self._frame2 if self.AUG else rp.frame
            r = voxelize_indexed(rp.depth, rp.offsets, rp.headers, torch.from_numpy(frame[idx]).to(dev), rp.gt,
                                 clamp=clamp, gt_copy=True, xforms=xf, **kw)
            return r[0], r[2], r[1], (r[3] if kw else None)
        src = idx % self._n
        pk = self.raw.take(src)
        depth, offsets, headers = pk.to_torch(dev, pin=False, non_blocking=False)
        gt = torch.from_numpy(np.ascontiguousarray(pk.gt)).to(dev)
        if not self.AUG:
            if not kw:
                return voxelize(depth, offsets, headers, res=32), gt, None, None
            out, gt_nor, gt_pca = voxelize_labels(depth, offsets, headers, gt, res=32, clamp=clamp, **kw)
            return out, gt, gt_nor, gt_pca
        # one AABB launch for the frames' centres, the maps about them, then the augmented entry
        mid = aabb(depth, offsets, headers).grid[:, :3]
        if self.aug_device:   # the centres and the maps never leave the device
            pos = np.where(idx < self._n, -1, np.arange(idx.size)).astype(np.int64)   # plain items: the identity map
            xf = aug_xforms_at(mid.contiguous(), self._device_state(), index=torch.from_numpy(pos).to(dev),
                               counters=torch.from_numpy(np.ascontiguousarray(src, np.int64)).to(dev))
        else:
            xf = augment.affines_from_params(mid.cpu().numpy().astype(np.float64), *(p[src] for p in self._aug_params))
            plain = idx < self._n
            xf[plain] = augment.identity_affines(int(plain.sum()))
            xf = torch.from_numpy(xf).to(dev)
        out, gt_nor, gt_aug = voxelize_aug(depth, offsets, headers, xf, res=32, gt=gt, clamp=clamp)
        # (the augmented entry has no fused projection: project_joints gives the same bits from the launch's outputs)
        gt_pca = project_joints(gt_aug, out.max_l, out.mid_p, self.pca, self.PCA_SZ) if kw else None
        return out, gt_aug, gt_nor, gt_pca

    def _fit_labels(self) -> np.ndarray:
        """The normalised labels (no clamp) of every item whose frame status is OK, float32[N, C] on the host, in item
        order — what :func:`pca.fit_joint_pca` fits.  Plain items: the grid placement of the AABB launch (bit-identical
        to the voxelizer's); augmented items: the augmented entry's own labels."""
        n, dev, us = self._n, self.device, []
        if self.resident:
            rp = self._resident_packs()
            pl = _place_aabb(rp.depth, rp.offsets, rp.headers, rows=False)
            fr = torch.from_numpy(rp.frame).to(dev)
            u = normalize_joints(rp.gt[fr].contiguous(), pl.max_l[fr], pl.mid_p[fr], clamp=False)
            us.append(u[pl.status[fr] == 0].cpu().numpy())
        else:
            for a in range(0, n, self.block):
                pk = self.raw.take(np.arange(a, min(n, a + self.block)))
                depth, offsets, headers = pk.to_torch(dev, pin=False, non_blocking=False)
                pl = _place_aabb(depth, offsets, headers, rows=False)
                gt = torch.from_numpy(np.ascontiguousarray(pk.gt)).to(dev)
                u = normalize_joints(gt, pl.max_l, pl.mid_p, clamp=False)
                us.append(u[pl.status == 0].cpu().numpy())
        for a in range(n, len(self), self.block):   # (the augmented items, where there are any)
            out, _, u, _ = self._voxelize_items(np.arange(a, min(len(self), a + self.block)), clamp=False)
            us.append(u[out.status == 0].cpu().numpy())
        return np.concatenate(us) if us else np.zeros((0, 63), np.float32)

    def _tuples(self, out, gt, gt_pca, m: int):
        if gt_pca is None:
            return [(out.tsdf[k], gt[k], out.max_l[k], out.mid_p[k]) for k in range(m)]
        return [(out.tsdf[k], gt[k], out.max_l[k], out.mid_p[k], gt_pca[k]) for k in range(m)]

    def _load_block(self, blk: int):
        a, b = blk * self.block, min(len(self.raw), (blk + 1) * self.block)
        self._cache, self._cache_gt, _, self._cache_pca = self._voxelize_items(np.arange(a, b))
        self._cache_block = blk

    # ---- the pre-batched path: one C call per batch, nothing allocated, nothing sliced ----
    class _Fast:
        """Ring state for batches of (at most) ``bs`` frames: output slots, one prebuilt result per slot and the C call's
        constant arguments.  Batches of up to 32 plain frames hand their index to the GPU by value (``by_value``:
        ``tsdf_voxelize_indexed_host_hip``); larger ones, and ``aug=True`` datasets, write it into page-locked index slots
        the kernel reads over the link, with one event per ``kGroup`` index slots that tells when a group's words have been
        read (an index slot's words are rewritten ``iring`` batches later).

        A slot is RECYCLED only when nothing outside this object refers to its batch any more (:class:`_SlotGuard`: Python
        reference counts of the tuple and its tensors, storage use counts for views and ``detach()`` / ``.data`` / numpy
        aliases).  Every slot owns its tensors (separate allocations); a slot whose batch is still held is given fresh
        tensors instead (``replaced`` counts them) and the kept batch stays what it was — like the independent tensors the
        reference's loader returns (3D_CNN/train.py:86-91 over numpy rows).  ``list(DataLoader(...))``, an evaluation
        loop that collects outputs, a loss history: all safe.  What cannot be seen is a consumer that dropped every
        reference but still has work queued on ANOTHER stream: order that stream after the loader's (the usual rule for
        GPU tensors).  On a torch where the counting rules do not hold (``_slot_guard_works``) every batch gets fresh
        tensors: slower, never wrong."""

        kGroup = 16
        pca, k = None, 0   # (class defaults: full mode is set per instance)

        def __init__(self, rp: "ResidentPacks", bs: int, ring: int, device, frame=None, xf_table=None, pca=None, k=0,
                     draw=None):
            self._ctypes, self._lib = ctypes, _lib
            self.always_fresh = not _slot_guard_works()
            ring = max(2, int(ring))
            self.iring = -(-max(ring, self.kGroup) // self.kGroup) * self.kGroup   # index slots: whole event groups
            self.bs, self.ring, self.count, self.replaced = bs, ring, 0, 0
            self.L = _lib.load()
            self.pca, self.k = pca, int(k)   # full mode: the fused projection writes each slot's gt_pca too
            self.rp_gt = rp.gt
            self.nc = rp.gt.shape[1]
            d = torch.device(device)
            self.device = d if d.index is not None else torch.device("cuda", torch.cuda.current_device())
            self.dev_index = self.device.index
            self.h_idx = torch.empty((self.iring, bs), dtype=torch.int64).pin_memory()
            self.h_idx_np = self.h_idx.numpy()
            self.rows = [self.h_idx_np[k] for k in range(self.iring)]
            self.idx_ptrs = [self.h_idx[k].data_ptr() for k in range(self.iring)]
            self.head = (rp.depth.data_ptr(), rp.depth.numel(), rp.offsets.data_ptr(), rp.headers.data_ptr(),
                         int(rp.headers.shape[0]))
            self.slots = [None] * ring      # (tsdf, gt, max_l, mid_p, status, gt_nor) — the slot's own tensors
            self.labels = [None] * ring
            self.args = [None] * ring       # (tsdf, max_l, mid_p, status, byref(labels)[, byref(pca)]) of the C call
            self.pcas = [None] * ring       # full mode: the slot's tsdf_pca
            self.results = [None] * ring    # [PreBatched((tsdf, gt, max_l, mid_p))]
            self.guard = [None] * ring      # _SlotGuard of the slot's batch
            for k in range(ring):
                self._fresh(k)
            self.read = [torch.cuda.Event() for _ in range(self.iring // self.kGroup)]
            self.read_used = [False] * (self.iring // self.kGroup)
            self.raw_stream = _get_raw_stream if _get_raw_stream is not None else \
                (lambda i: torch.cuda.current_stream(i).cuda_stream)
            self.cur_dev = getattr(torch._C, "_cuda_getDevice", torch.cuda.current_device)
            self.fn = self.L.tsdf_voxelize_indexed_hip
            self.plain_xf = ()              # (the PCA entry of the page-locked path takes d_xforms = NULL first)
            if pca is not None:
                self.fn, self.plain_xf = self.L.tsdf_voxelize_indexed_pca_hip, (None,)
            self.take = (rp.frame if frame is None else frame).take   # dataset item -> frame of the resident packs
            # batches of at most INLINE_INDEX_MAX frames: the index goes to the GPU inside the kernel arguments
            # (tsdf_voxelize_indexed_host_hip reads it during the call) — no page-locked slot, no event, and the launch
            # does not start with a read over the link
            self.by_value = xf_table is None and draw is None and bs <= _lib.INLINE_INDEX_MAX
            self.fn_host = self.L.tsdf_voxelize_indexed_host_hip if pca is None else \
                self.L.tsdf_voxelize_indexed_host_pca_hip
            # ... and of both aug forms: one map per batch position, read by the kernel next to the index
            self.fn_aug = self.L.tsdf_voxelize_indexed_aug_hip if pca is None else self.L.tsdf_voxelize_indexed_pca_hip
            self.idx_buf = np.empty(bs, np.int64)
            self.idx_ptr = self.idx_buf.ctypes.data
            self.xf_take = None
            if xf_table is not None:   # aug=True: the maps in page-locked memory
                self.h_xf = torch.empty((self.iring, bs, 24), dtype=torch.float64).pin_memory()
                self.h_xf_np = self.h_xf.numpy()
                self.xf_rows = [self.h_xf_np[k] for k in range(self.iring)]
                self.xf_ptr = [self.h_xf[k].data_ptr() for k in range(self.iring)]
                self.xf_take = xf_table.take
            # aug="device": per index slot, the draw's frame numbers (-1: a plain item) and counters in page-locked memory
            # next to the voxelizer's index, and the slot's maps on the device; `draw` = (centres, state, frames, counters)
            self.draw = None
            if draw is not None:
                centres, state, frames, counters = draw
                self.fn_draw = _lib.load_augstep().tsdf_aug_draw_at_hip
                self.draw = (centres, state)      # (kept alive: the launches read them by raw pointer)
                self.draw_head = (centres.data_ptr(), int(centres.shape[0]))
                self.state_ptr = state.data_ptr()
                self.h_draw = torch.empty((self.iring, 2, bs), dtype=torch.int64).pin_memory()
                self.h_draw_np = self.h_draw.numpy()
                self.draw_rows = [(self.h_draw_np[k, 0], self.h_draw_np[k, 1]) for k in range(self.iring)]
                self.draw_ptrs = [(self.h_draw[k, 0].data_ptr(), self.h_draw[k, 1].data_ptr()) for k in range(self.iring)]
                self.d_xf = torch.empty((self.iring, bs, 24), dtype=torch.float64, device=self.device)
                self.xf_ptr = [self.d_xf[k].data_ptr() for k in range(self.iring)]
                self.frame_take, self.counter_take = frames.take, counters.take

        def _fresh(self, k: int) -> None:
            """New tensors for slot k (at start-up, and whenever its previous batch is still held by the consumer)."""
            self._alloc(k)
            self.guard[k].arm()      # (taken when _alloc's locals are gone: the ring's own references)

        def _alloc(self, k: int) -> None:
            R, bs, nc, dev = 32, self.bs, self.nc, self.device
            tsdf = torch.empty((bs, 3, R, R, R), dtype=torch.float32, device=dev)
            gt = torch.empty((bs, nc), dtype=torch.float32, device=dev)
            max_l = torch.empty(bs, dtype=torch.float32, device=dev)
            mid_p = torch.empty((bs, 3), dtype=torch.float32, device=dev)
            status = torch.empty(bs, dtype=torch.int32, device=dev)
            gt_nor = torch.empty((bs, nc), dtype=torch.float32, device=dev)
            self.slots[k] = (tsdf, gt, max_l, mid_p, status, gt_nor)
            self.labels[k] = self._lib.TsdfLabels(self.rp_gt.data_ptr(), nc // 3, 1, gt_nor.data_ptr(), gt.data_ptr())
            self.args[k] = (tsdf.data_ptr(), max_l.data_ptr(), mid_p.data_ptr(), status.data_ptr(),
                            self._ctypes.byref(self.labels[k]))
            batch = (tsdf, gt, max_l, mid_p)
            if self.pca is not None:
                gt_pca = torch.empty((bs, self.k), dtype=torch.float32, device=dev)
                mean, coeff = self.pca.device_tensors(dev)
                self.pcas[k] = self._lib.TsdfPca(mean.data_ptr(), coeff.data_ptr(), self.k, gt_pca.data_ptr())
                self.slots[k] = self.slots[k] + (gt_pca,)
                self.args[k] = self.args[k] + (self._ctypes.byref(self.pcas[k]),)
                batch = batch + (gt_pca,)
            self.results[k] = [PreBatched(batch)]
            self.guard[k] = _SlotGuard(self.results[k][0].batch)

        def held(self, k: int) -> bool:
            """Does anything outside the ring still refer to slot k's batch (the tuple, a tensor, any alias of one)?"""
            return self.always_fresh or self.guard[k].held()

        def next_slot(self) -> int:
            """The output slot of the next batch, free to be overwritten."""
            k = self.count % self.ring
            if self.held(k):
                self._fresh(k)
                self.replaced += 1
            return k

        def sync(self) -> None:
            """Everything queued through this ring has run (called before the ring is dropped: queued launches read its
            page-locked index words by raw pointer, which torch's pinned-memory allocator knows nothing about)."""
            torch.cuda.current_stream(self.device).synchronize()

    def _ring_size(self, n: int) -> int:
        """Output slots of the pre-batched ring: an explicit ``ring`` is honoured (at least 2); otherwise as many batches
        as fit 2 GiB of volumes, between 2 and 256 (batch 16: 256 slots = 1.6 GB; batch 1024: 5 slots = 2.0 GB)."""
        if self._ring_req:
            return max(2, int(self._ring_req))
        vol = n * (3 * 32 ** 3 * 4)
        return max(2, min(256, (2 << 30) // max(vol, 1)))

    def _fast_batch(self, indices):
        """One batch through the ring: ~4 us of Python around the C call (the HIP launch itself is the larger part)."""
        f = self._fast
        n = len(indices)
        if f is None or n > f.bs:
            if f is not None:
                f.sync()      # launches that read the old ring's page-locked words must be done before it goes away
            f = self._fast = MSRA_Dataset._Fast(self._rp, n, self._ring_size(n), self.device,
                                                frame=self._frame2 if self.AUG else None, xf_table=self._xf_table,
                                                pca=self.pca, k=self.PCA_SZ,
                                                draw=(self._aug_mid, self._device_state(), self._draw_frame,
                                                      self._draw_counter) if self.aug_device else None)
        k = f.next_slot()
        a = f.args[k]
        if f.by_value:                        # (the epoch's short last batch, or another current device)
            fn = f.fn_host
            f.idx_buf[:n] = f.take(indices)
            with torch.cuda.device(f.device):
                rc = fn(*f.head, f.idx_ptr, n, 32, None, 0, f.raw_stream(f.dev_index), *a)
        else:
            ki = f.count % f.iring            # the index words' slot (page-locked ring of whole event groups)
            within = ki & (f.kGroup - 1)
            if within == 0 and f.read_used[ki >> 4]:
                f.read[ki >> 4].synchronize()     # the launches that read this group's index words a ring ago are done
            # dataset item -> pack frame, written where the kernel will read it; numpy checks the range (IndexError) and,
            # like a Python list, counts negative indices from the end
            if n == f.bs:
                f.take(indices, out=f.rows[ki])
            else:
                f.h_idx_np[ki, :n] = f.take(indices)
            if f.draw is not None:        # aug="device": one launch draws the batch's maps, the next one reads them
                fr, cn = f.draw_rows[ki]
                if n == f.bs:
                    f.frame_take(indices, out=fr)
                    f.counter_take(indices, out=cn)
                else:
                    fr[:n] = f.frame_take(indices)
                    cn[:n] = f.counter_take(indices)
                with torch.cuda.device(f.device):
                    stream = f.raw_stream(f.dev_index)
                    fn = f.fn_draw
                    rc = fn(*f.draw_head, f.draw_ptrs[ki][0], n, f.state_ptr, f.draw_ptrs[ki][1], stream, f.xf_ptr[ki],
                            None, None)
                    if rc == 0:
                        fn = f.fn_aug
                        rc = fn(*f.head, f.idx_ptrs[ki], n, 32, None, 0, stream, f.xf_ptr[ki], *a)
            elif f.xf_take is not None:   # aug=True: the batch's maps next to its indices
                fn = f.fn_aug
                if n == f.bs:
                    f.xf_take(indices, axis=0, out=f.xf_rows[ki])
                else:
                    f.h_xf_np[ki, :n] = f.xf_take(indices, axis=0)
                with torch.cuda.device(f.device):
                    rc = fn(*f.head, f.idx_ptrs[ki], n, 32, None, 0, f.raw_stream(f.dev_index), f.xf_ptr[ki], *a)
            else:
                fn = f.fn
                if f.cur_dev() == f.dev_index:
                    rc = fn(*f.head, f.idx_ptrs[ki], n, 32, None, 0, f.raw_stream(f.dev_index), *f.plain_xf, *a)
                else:
                    with torch.cuda.device(f.device):
                        rc = fn(*f.head, f.idx_ptrs[ki], n, 32, None, 0, f.raw_stream(f.dev_index), *f.plain_xf, *a)
            if within == f.kGroup - 1:
                f.read[ki >> 4].record(torch.cuda.current_stream(f.device))
                f.read_used[ki >> 4] = True
        if rc != 0:
            _lib.check(rc, fn.__name__)
        f.count += 1
        if n == f.bs:
            return f.results[k]
        return [PreBatched(tuple(t[:n] for t in f.results[k][0].batch))]   # the epoch's short last batch

    def __getitems__(self, indices):
        """The frames of one batch, voxelized by one launch (torch's DataLoader calls this with the batch's indices
        when it exists).  ``prebatched``: ``[PreBatched(batch)]``, which ``default_collate`` turns into the batch; else a
        list of item tuples, views into the batch's tensors."""
        if data.get_worker_info() is not None:
            raise RuntimeError("MSRA_Dataset produces its items on the GPU: use it with num_workers=0 (the reference's "
                               "default, train.py:38), there is nothing for loader processes to do")
        f = self._fast
        if f is not None and f.by_value and len(indices) == f.bs and f.cur_dev() == f.dev_index:
            # the hot path of a training epoch, inlined (every microsecond here is 6 % of a batch of 16): a full batch of
            # plain items on the current device — item -> pack frame, one C call that takes the index by value, the
            # ring slot's prebuilt result
            k = f.next_slot()      # (a slot whose batch the consumer still holds gets fresh tensors)
            f.take(indices, out=f.idx_buf)
            a = f.args[k]
            rc = f.fn_host(*f.head, f.idx_ptr, f.bs, 32, None, 0, f.raw_stream(f.dev_index), *a)
            if rc != 0:
                _lib.check(rc, "tsdf_voxelize_indexed_host_hip")
            f.count += 1
            self._last = indices[-1]
            return f.results[k]
        if self.prebatched:
            if not indices:
                raise IndexError("empty batch")
            self._resident_packs()
            self._last = indices[-1]
            return self._fast_batch(indices)
        idx = np.asarray([int(i) for i in indices], np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError(int(idx.max() if idx.max() >= len(self) else idx.min()))
        self._last = int(idx[-1]) if idx.size else self._last
        out, gt, _, gt_pca = self._voxelize_items(idx)
        return self._tuples(out, gt, gt_pca, idx.size)

    def _items_of(self, indices):
        """``indices`` as a list of item tuples whatever ``prebatched`` says (single-item access)."""
        r = self.__getitems__(indices)
        if r and isinstance(r[0], PreBatched):
            b = r[0].batch
            return [tuple(t[k].clone() for t in b) for k in range(len(indices))]   # (out of the ring: the item outlives it)
        return r

    def __getitem__(self, index):
        index = int(index)
        if not 0 <= index < len(self):
            raise IndexError(index)
        if self.AUG:                                              # (no block cache: plain and augmented items mix)
            self._last = index
            return self._items_of([index])[0]
        blk = index // self.block
        if blk != self._cache_block:
            if index != self._last + 1 and index % self.block:   # random access: this frame alone
                return self._items_of([index])[0]
            self._load_block(blk)                                 # a sequential walk: the whole block at once
        self._last = index
        k = index - blk * self.block
        c = self._cache
        if self._cache_pca is not None:
            return c.tsdf[k], self._cache_gt[k], c.max_l[k], c.mid_p[k], self._cache_pca[k]
        return c.tsdf[k], self._cache_gt[k], c.max_l[k], c.mid_p[k]
