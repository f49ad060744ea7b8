"""Numpy restatement of the joint-PCA projection and the pose error (include/tsdf.h, "Joint PCA and pose error",
items 1, 3 and 4) for the tests: float32 operations one at a time, float64 sums as sequential loops in the stated
order (numpy's elementwise float64 multiply and add round once each, no FMA)."""
import numpy as np

f32 = np.float32


def normalize(gt, max_l, mid_p, ok=None):
    """Item 1: (gt - mid_p) / max_l + 0.5, no clamp; frames that are not OK (default: max_l <= 0) get 0.5."""
    gt = np.asarray(gt, f32)
    n = gt.shape[0]
    g = gt.reshape(n, -1, 3)
    ml = np.asarray(max_l, f32).reshape(n, 1, 1)
    mp = np.asarray(mid_p, f32).reshape(n, 1, 3)
    ok = (ml > 0) if ok is None else np.asarray(ok, bool).reshape(n, 1, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (g - mp) / np.where(ok, ml, f32(1)) + f32(0.5)
    return np.where(ok, u, f32(0.5)).astype(f32).reshape(n, -1)


def project(u, mean, W, k):
    """Item 3: t_j = fl32(u_j - mu_j); p_k = fl32(sum_j t_j W[j,k]) summed in float64 in ascending j."""
    t = (np.asarray(u, f32) - np.asarray(mean, f32)).astype(f32).astype(np.float64)
    W64 = np.asarray(W, f32).astype(np.float64)[:, :k]
    p = np.zeros((t.shape[0], k))
    for j in range(t.shape[1]):
        p = p + t[:, j:j + 1] * W64[j:j + 1, :]
    return p.astype(f32)


def decode(p, mean, W):
    """Item 4, first half: u^_j = fl32(mu_j + sum_k p_k W[j,k]), the float64 accumulator starting at mu_j, ascending k."""
    p64 = np.asarray(p, f32).astype(np.float64)
    k = p64.shape[1]
    W64 = np.asarray(W, f32).astype(np.float64)
    acc = np.broadcast_to(np.asarray(mean, f32).astype(np.float64), (p64.shape[0], W64.shape[0])).copy()
    for kk in range(k):
        acc = acc + p64[:, kk:kk + 1] * W64[None, :, kk]
    return acc.astype(f32)


def denormalize(uh, max_l, mid_p):
    n = uh.shape[0]
    u = np.asarray(uh, f32).reshape(n, -1, 3)
    ml = np.asarray(max_l, f32).reshape(n, 1, 1)
    mp = np.asarray(mid_p, f32).reshape(n, 1, 3)
    x = (u - f32(0.5)) * ml + mp
    return np.where(ml > 0, x, mp).astype(f32).reshape(n, -1)


def pose_error(pred, gt, max_l, mid_p, mean=None, W=None):
    """Item 4: (err[n,J], frame_mean[n], frame_max[n], joints[n,3J]).  pred: PCA coefficients with mean / W, else
    normalised coordinates."""
    uh = decode(pred, mean, W) if mean is not None else np.asarray(pred, f32)
    x = denormalize(uh, max_l, mid_p)
    n = x.shape[0]
    d = (x - np.asarray(gt, f32).reshape(n, -1)).reshape(n, -1, 3).astype(f32)
    sq = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    err = np.sqrt(sq.astype(f32)).astype(f32)
    s = np.zeros(n)
    mx = err[:, 0].copy()
    for j in range(err.shape[1]):
        s = s + err[:, j].astype(np.float64)
        mx = np.where((err[:, j] > mx) | np.isnan(err[:, j]), err[:, j], mx)
    return err, (s / err.shape[1]).astype(f32), mx.astype(f32), x


# ---- order-free float64 references: the exact sums, up to float64 rounding, whatever order a kernel adds in ----------
# A bug that the kernels and the restatement above share (W transposed, a wrong row or column) is far outside these
# bounds; a different summation order is well inside them.

def project64(u, mean, W, k):
    """(t @ W[:, :k] in float64, sum_j |t_j W[j,k]|) with t = fl32(u - mu) as item 3 defines it."""
    t = (np.asarray(u, f32) - np.asarray(mean, f32)).astype(f32).astype(np.float64)
    W64 = np.asarray(W, f32).astype(np.float64)[:, :k]
    return t @ W64, np.abs(t) @ np.abs(W64)


def decode64(p, mean, W):
    """(mu + p @ W[:, :K]^T in float64, |mu_j| + sum_k |p_k W[j,k]|), K = p.shape[1]."""
    p64 = np.asarray(p, f32).astype(np.float64)
    W64 = np.asarray(W, f32).astype(np.float64)[:, :p64.shape[1]]
    mu = np.asarray(mean, f32).astype(np.float64)
    return mu + p64 @ W64.T, np.abs(mu) + np.abs(p64) @ np.abs(W64.T)


def bound64(ref, scale, terms):
    """What a float32 result of a float64 sum of `terms` products may differ from ref by: the final float32 rounding
    (half an ulp, 2^-24 relative; 2^-149 for subnormals) plus `terms` float64 roundings on each side (2^-53 of the
    running |sum| <= scale each), doubled for slack."""
    return 2 * (np.abs(ref) * 2.0 ** -24 + 2.0 ** -149 + 2 * terms * scale * 2.0 ** -53)


def bits(a):
    """The bit patterns of a 4-byte array or tensor (a tensor is copied to the host).  Equality of these is
    bit-exactness, which np.array_equal / torch.equal are not: they take -0 for +0 and never match a NaN."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4, a.dtype
    return a.view(np.uint32)


def same_bits(a, b):
    x, y = bits(a), bits(b)
    return x.shape == y.shape and np.array_equal(x, y)
