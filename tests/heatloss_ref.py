"""The numpy restatement of include/tsdf_heatloss.h, float64 operation for operation, on top of tests/heatmap_ref.py (whose
``encode`` is the target): what the heatloss tests compare the GPU with, and the reductions of the Python wrapper.  Nothing
here touches a GPU or the library.  Volumes are float32 arrays (float32 holds a 2-byte value exactly)."""
import numpy as np

import heatmap_ref as hr

U = 2.0 ** -53      # the unit roundoff of float64


# ---- loss ----
def sse(pred, t32, valid):
    """``sse float64[n,J]``: per unit the sum of ``((double)pred - (double)t32)^2``; 0 for an invalid unit.  numpy sums
    pairwise: the order differs from the kernel's, which is what the comparison's 2^-31 allows for."""
    n, J = valid.shape
    with np.errstate(invalid="ignore", over="ignore"):
        d = pred.astype(np.float64) - t32.astype(np.float64)
        s = (d * d).reshape(n * J, -1).sum(axis=1).reshape(n, J)
    return np.where(valid != 0, s, 0.0)


def sse_grad(pred, t32, valid, w, exact=False):
    """``float32((double)w[unit] * d)`` per voxel, +0 in an invalid unit whatever ``w`` holds (``exact``: the float64
    product before its rounding)."""
    n, J = valid.shape
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        d = pred.astype(np.float64) - t32.astype(np.float64)
        g = np.asarray(w, np.float32).astype(np.float64).reshape(n, J, 1, 1, 1) * d
        g[valid == 0] = 0.0
        return g if exact else g.astype(np.float32)


def sse_bound(pred, t32, valid):
    """Per unit, how far the sse of a target correct to the encode's own bound (|t - t'| <= e = 2^-23 t + 2^-125 per voxel:
    two exp of 1 ulp each before one rounding to float32, tests/test_heatmap_gpu.py) may lie from the sse of ``t32``:
    |d'^2 - d^2| = |d' - d| |d' + d| <= e (2 |d| + e), summed over the unit; plus 2^-31 of the sum for its order."""
    n, J = valid.shape
    t = t32.astype(np.float64)
    d = np.abs(pred.astype(np.float64) - t)
    e = 2.0 ** -23 * t + 2.0 ** -125
    b = (e * (2.0 * d + e)).reshape(n * J, -1).sum(axis=1).reshape(n, J)
    return np.where(valid != 0, b + 2.0 ** -31 * sse(pred, t32, valid), 0.0)


def reduce(sse_, valid, R, reduction):
    """``(loss float64, factor float64[n,J])`` of the wrapper: the reduced loss and d loss / d sse[unit] times 2."""
    r3 = float(R) ** 3
    ok = (np.asarray(valid) != 0).astype(np.float64)
    if reduction == "mean":
        denom = max(ok.sum() * r3, 1.0)
        return sse_.sum() / denom, (2.0 * ok) / denom
    if reduction == "sum":
        return sse_.sum(), 2.0 * ok
    assert reduction == "none"
    return sse_ / r3, (2.0 * ok) / r3


def weights(grad_out, factor):
    """The gradient kernel's ``w float32[n,J]``: the upstream gradient times the reduction's factor, float64, then cast."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(grad_out, np.float64) * factor).astype(np.float32)


# ---- soft-argmax ----
def _indices(R, layout):
    """(i_x, i_y, i_z) of every voxel in memory order, float64[R^3] each."""
    slow, mid, fast = (a.reshape(-1).astype(np.float64) for a in np.indices((R, R, R)))
    return (fast, mid, slow) if layout == "czyx" else (slow, mid, fast)


def soft_argmax(h, R, beta, layout="czyx"):
    """``(u float32[n,J,3], stats float64[n,J,5])`` of ``h`` [n,J,R,R,R]: stats = (m, Z, c_x, c_y, c_z)."""
    assert layout in hr.LAYOUTS
    n, J = h.shape[:2]
    flat = h.reshape(n * J, -1).astype(np.float64)
    b = np.float64(np.float32(beta))
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        m = np.where(np.isnan(flat), -np.inf, flat).max(axis=1)      # under `>` from -inf: a NaN is never it
        z = np.exp(b * (flat - m[:, None]))
        Z = z.sum(axis=1)
        c = np.stack([(z * i).sum(axis=1) / Z for i in _indices(R, layout)], axis=1)
        u = ((c + 0.5) / np.float64(R)).astype(np.float32)
    stats = np.concatenate([m[:, None], Z[:, None], c], axis=1)
    return u.reshape(n, J, 3), stats.reshape(n, J, 5)


def soft_argmax_grad(h, stats, gu, R, beta, layout="czyx", exact=False):
    """``float32((z_i * k) * s_i)`` per voxel, k = beta / (Z * R), s_i = (gu_x (i_x - c_x) + gu_y (i_y - c_y)) + gu_z (i_z - c_z),
    z_i recomputed from h, m and beta (``exact``: before the rounding to float32)."""
    n, J = h.shape[:2]
    flat = h.reshape(n * J, -1).astype(np.float64)
    st = np.asarray(stats, np.float64).reshape(n * J, 5)
    g = np.asarray(gu, np.float32).astype(np.float64).reshape(n * J, 3)
    b = np.float64(np.float32(beta))
    ix, iy, iz = _indices(R, layout)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        z = np.exp(b * (flat - st[:, 0:1]))
        k = b / (st[:, 1] * np.float64(R))
        s = (g[:, 0:1] * (ix[None] - st[:, 2:3]) + g[:, 1:2] * (iy[None] - st[:, 3:4])) + g[:, 2:3] * (iz[None] - st[:, 4:5])
        out = (z * k[:, None]) * s
        out = out.reshape(h.shape)
        return out if exact else out.astype(np.float32)


def soft_argmax_grad_bound(h, stats, gu, R, beta, layout="czyx"):
    """The GPU comparison's bound per voxel: 2^-23 |ref| + beta q_i sum|gu_a| (R 2^-30) / R + one float32 denormal, where
    q_i = z_i / Z.  c_a carries the error of two sums of N <= 2^21 terms in another order and of exp to 1 ulp, N u + a few
    u relative to sums of at most R: below R 2^-30; it enters s_i times |gu_a|.  The relative errors of z_i, Z and the
    products (a few u, N u) and the final rounding to float32 (2^-24) are within the first term."""
    n, J = h.shape[:2]
    st = np.asarray(stats, np.float64).reshape(n * J, 5)
    b = np.float64(np.float32(beta))
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        q = np.exp(b * (h.reshape(n * J, -1).astype(np.float64) - st[:, 0:1])) / st[:, 1:2]
        ga = np.abs(np.asarray(gu, np.float32).astype(np.float64)).reshape(n * J, 3).sum(axis=1)
        ref = np.abs(soft_argmax_grad(h, stats, gu, R, beta, layout, exact=True)).reshape(n * J, -1)
        return (2.0 ** -23 * ref + b * q * ga[:, None] * (R * 2.0 ** -30) / R + 2.0 ** -149).reshape(h.shape)
