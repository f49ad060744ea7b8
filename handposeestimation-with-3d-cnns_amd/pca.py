"""Joint PCA of the normalised labels — what the reference's ``--size full`` mode regresses.

The reference trains on PCA coefficients of the normalised joints (3D_CNN/train.py:196-226, 3D_CNN/dataset.py:165-180),
fitted per leave-one-subject-out fold by pre/joint_pca.py.  None of those pieces runs as written, so the fit is
RE-SPECIFIED here (contract: include/tsdf.h, "Joint PCA and pose error"):

  * pre/joint_pca.py:34,39 hands the function ``joint_pca`` instead of the data to ``cal_pca``; :71 iterates over an int
    (``for i in len(...)``); :59 reads from ``/result``; ``np.savez('./PCA', '%s.npz' % test, ...)`` writes ``./PCA.npz``
    with the file name as a positional array.  The fit below is over the fold's normalised labels (item 1) with the
    MATLAB ``pca`` conventions the file's comment block uses: mean, covariance with the N-1 divisor, components by
    descending variance (``latent``), each column's largest-|.| entry positive.  Stored as ``<dir>/<fold>.npz`` /
    ``<fold>-aug.npz`` with the keys ``pca_mean``, ``coeff``, ``latent`` that 3D_CNN/dataset.py:171-175 reads.
  * 3D_CNN/dataset.py:176 subtracts the mean of NORMALISED joints from raw-mm joints: here the projection is of the
    normalised labels (the fused labels path, ``voxelize.project_joints``).
  * ``PCA_mean`` is 1-D but train.py:222 calls ``.size(1)`` on it, and ``PCA_coeff.transpose(0, 1)`` on a numpy array
    is the identity, so the decode at train.py:224 multiplies by W instead of W^T (right only for K = 63).
    ``MSRA_Dataset(pca=...)`` exposes ``PCA_mean`` float32[1, C] and ``PCA_coeff`` = W[:, :K]^T float32[K, C], with
    which the reference's unmodified ``torch.addmm(PCA_mean.expand(b, C), est, PCA_coeff)`` is mu + p W^T.

The fit is float64 numpy on the host (a C x C eigenproblem once per fold: not a hot path).
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import numpy as np


def normalize_labels_np(gt: np.ndarray, max_l: np.ndarray, mid_p: np.ndarray) -> np.ndarray:
    """Item 1 on the host, bit-identical to the device (float32 numpy operations round to nearest one at a time):
    ``(gt - mid_p) / max_l + 0.5`` without clamp; frames with ``max_l <= 0`` get 0.5.  gt [n, 3J] -> float32[n, 3J]."""
    gt = np.asarray(gt, np.float32)
    n = gt.shape[0]
    g3 = gt.reshape(n, -1, 3)
    ml = np.asarray(max_l, np.float32).reshape(n, 1, 1)
    mp = np.asarray(mid_p, np.float32).reshape(n, 1, 3)
    ok = ml > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (g3 - mp) / np.where(ok, ml, np.float32(1)) + np.float32(0.5)
    u = np.where(ok, u, np.float32(0.5)).astype(np.float32)
    return u.reshape(n, -1)


class JointPCA:
    """A fitted joint PCA: ``mean`` float32[C], ``coeff`` W float32[C, C] (all components; K is chosen at use),
    ``latent`` float64[C] (component variances, descending), ``n_frames`` and the fold / aug it was fitted for."""

    def __init__(self, mean, coeff, latent=None, n_frames: int = 0, fold: Optional[int] = None, aug: bool = False):
        self.mean = np.ascontiguousarray(np.asarray(mean, np.float32).reshape(-1))
        C = self.mean.size
        coeff = np.asarray(coeff, np.float32)
        if coeff.ndim != 2 or coeff.shape[0] != C or not 1 <= coeff.shape[1] <= C:
            raise ValueError(f"coeff must be [C, K<=C] with C = {C}, got {coeff.shape}")
        self.n_avail = int(coeff.shape[1])   # columns the file holds (a full fit: C)
        if self.n_avail < C:                 # (the device layout is [C][C]: unheld columns are zero and never read)
            coeff = np.concatenate([coeff, np.zeros((C, C - self.n_avail), np.float32)], axis=1)
        self.coeff = np.ascontiguousarray(coeff)
        self.latent = np.full(C, np.nan) if latent is None else np.asarray(latent, np.float64).reshape(-1)
        self.n_frames = int(n_frames)
        self.fold = fold
        self.aug = bool(aug)
        self._dev: Dict[str, tuple] = {}

    @property
    def n_coords(self) -> int:
        return int(self.mean.size)

    def check_k(self, k: Optional[int]) -> int:
        k = self.n_avail if k is None else int(k)
        if not 1 <= k <= self.n_avail:
            raise ValueError(f"k = {k} components requested, the basis holds 1..{self.n_avail}")
        return k

    def device_tensors(self, device):
        """(mean float32[C], coeff float32[C, C]) on ``device``, uploaded once per device."""
        import torch
        d = torch.device(device)
        if d.type == "cuda" and d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        key = str(d)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.mean).to(d), torch.from_numpy(self.coeff).to(d))
        return self._dev[key]

    def to(self, device) -> "JointPCA":
        """Upload the basis to ``device`` (kept with the object; returns self)."""
        self.device_tensors(device)
        return self

    def torch_decode_args(self, k: int, device):
        """``(PCA_mean float32[1, C], PCA_coeff float32[K, C])`` on ``device``: with these the reference's decode
        ``torch.addmm(PCA_mean.expand(b, C), est, PCA_coeff)`` (3D_CNN/train.py:221-225) is mu + p W[:, :K]^T."""
        k = self.check_k(k)
        mean, coeff = self.device_tensors(device)
        return mean.view(1, -1), coeff[:, :k].t().contiguous()

    def path(self, directory: str, fold: Optional[int] = None, aug: Optional[bool] = None) -> str:
        fold = self.fold if fold is None else fold
        aug = self.aug if aug is None else aug
        return os.path.join(directory, "%d%s.npz" % (int(fold), "-aug" if aug else ""))

    def save(self, directory: str, fold: Optional[int] = None, aug: Optional[bool] = None) -> str:
        """``<directory>/<fold>.npz`` (``<fold>-aug.npz``): ``pca_mean``, ``coeff``, ``latent`` — what
        3D_CNN/dataset.py:171-175 reads — plus ``n_frames`` / ``fold`` / ``aug``."""
        fold = self.fold if fold is None else fold
        if fold is None:
            raise ValueError("save() needs a fold")
        os.makedirs(directory, exist_ok=True)
        p = self.path(directory, fold, aug)
        np.savez(p, pca_mean=self.mean, coeff=self.coeff[:, :self.n_avail], latent=self.latent,
                 n_frames=np.int64(self.n_frames), fold=np.int64(fold), aug=np.bool_(self.aug if aug is None else aug))
        return p

    @classmethod
    def load(cls, path: str) -> "JointPCA":
        """A file written by :meth:`save`, or one in the reference's format (``pca_mean`` 1-D or [1, C], ``coeff``
        [C, K], ``latent`` optional, 1-D or [C, 1] — the MATLAB ``pca`` outputs its comment block saves)."""
        with np.load(path) as z:
            latent = z["latent"] if "latent" in z.files else None
            n_frames = int(z["n_frames"]) if "n_frames" in z.files else 0
            fold = int(z["fold"]) if "fold" in z.files else None
            aug = bool(z["aug"]) if "aug" in z.files else os.path.basename(path).endswith("-aug.npz")
            return cls(z["pca_mean"], z["coeff"], latent, n_frames, fold, aug)


def fit_labels(u: np.ndarray, fold: Optional[int] = None, aug: bool = False) -> JointPCA:
    """Item 2 of the contract on normalised labels ``u`` [N, C] (the OK frames of one training fold): float64 mean,
    covariance with the N-1 divisor, ``np.linalg.eigh``, components by descending eigenvalue, each column's largest-|.|
    entry positive (ties: the lowest index)."""
    x = np.asarray(u, np.float64)
    if x.ndim != 2 or x.shape[0] < 2:
        raise ValueError("a PCA fit needs at least two frames")
    mu = x.mean(axis=0)
    xc = x - mu
    cov = xc.T @ xc / (x.shape[0] - 1)
    w, v = np.linalg.eigh(cov)
    order = np.argsort(-w, kind="stable")
    w, v = w[order], v[:, order]
    big = np.argmax(np.abs(v), axis=0)          # (argmax returns the first maximum: ties go to the lowest index)
    v = v * np.where(v[big, np.arange(v.shape[1])] < 0, -1.0, 1.0)
    return JointPCA(mu.astype(np.float32), v.astype(np.float32), w, n_frames=x.shape[0], fold=fold, aug=aug)


def fit_joint_pca(dataset) -> JointPCA:
    """Fit on exactly the items of a TRAINING ``MSRA_Dataset`` (its subjects but ``test_index``; with ``aug=True`` its
    augmented items too), from the labels the device normalises with the max_l / mid_p the items carry.  Frames whose
    status is not OK are left out."""
    if not getattr(dataset, "train", True):
        raise ValueError("fit_joint_pca needs a training dataset: a test fold uses the training set's basis")
    u = dataset._fit_labels()
    return fit_labels(u, fold=getattr(dataset, "test_idx", None), aug=bool(getattr(dataset, "AUG", False)))
