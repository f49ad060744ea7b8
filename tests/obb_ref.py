"""numpy restatement of include/tsdf_obb.h for the tests: the point formula of the contract, two-pass moments and
``numpy.linalg.eigh`` (not the kernel's Jacobi: an independent decomposition), HandPointNet's signs and the map packed
with the contract's formulas.  Test infrastructure only."""
import math

import numpy as np

F, CX, CY, EPS = 241.42, 160.0, 120.0, 1.0
U = 2.0 ** -53


def header_ok(hdr, off0, off1, depth_len):
    left, top, right, bottom = (int(v) for v in hdr[2:6])
    bw, bh = right - left, bottom - top
    return bw > 0 and bh > 0 and bw * bh == off1 - off0 and off0 >= 0 and off1 <= depth_len


def cloud(depth, hdr, focal=F, cx=CX, cy=CY, eps=EPS):
    """float64[N,3]: the valid pixels of one crop (row-major order), by the contract's point formula under the camera
    constants ``focal``, ``cx``, ``cy`` and ``eps`` (tsdf_cam.invalid_eps)."""
    left, top, right, bottom = (int(v) for v in hdr[2:6])
    bw, bh = right - left, bottom - top
    d = np.asarray(depth, np.float32).reshape(bh, bw)
    with np.errstate(invalid="ignore"):
        valid = np.abs(d) >= np.float32(eps)          # NaN compares false
    i, j = np.nonzero(valid)
    d64 = d[i, j].astype(np.float64)
    s = d64 / focal
    x = ((left + j).astype(np.float64) - cx) * s
    y = -(((top + i).astype(np.float64) - cy) * s)
    return np.stack([x, y, -d64], axis=1)


_fma = getattr(math, "fma", lambda a, b, c: a * b + c)   # (a Python without math.fma: one more rounding, far inside every bound)


def pack_rotation(A, mu):
    """The contract's map: forward rows {A_i, mu_i - fma(A_i0, mu_x, fma(A_i1, mu_y, A_i2 mu_z))}, then A^T likewise."""
    def rows(M):
        out = np.empty(12)
        for i in range(3):
            out[4 * i:4 * i + 3] = M[i]
            out[4 * i + 3] = mu[i] - _fma(M[i, 0], mu[0], _fma(M[i, 1], mu[1], M[i, 2] * mu[2]))
        return out
    return np.concatenate([rows(A), rows(A.T)])


def identity():
    xf = np.zeros(24)
    xf[[0, 5, 10, 12, 17, 22]] = 1.0
    return xf


def frame(depth, hdr, focal=F, cx=CX, cy=CY, eps=EPS):
    """dict(status, N, mu, C [3,3], lam [3] descending, A [3,3] rows e1 e2 e3, xf [24], pts) of one crop whose header is
    good, under the camera constants of :func:`cloud`."""
    pts = cloud(depth, hdr, focal, cx, cy, eps)
    N = len(pts)
    out = dict(status=1, N=N, mu=np.zeros(3), C=np.zeros((3, 3)), lam=np.zeros(3), A=np.eye(3), xf=identity(), pts=pts)
    if N < 3:
        return out
    mu = pts.sum(axis=0) / N
    q = pts - mu
    C = (q.T @ q) / N
    if not (np.isfinite(mu).all() and np.isfinite(C).all()) or np.trace(C) == 0:
        return out
    w, V = np.linalg.eigh(C)                     # ascending
    lam = w[::-1].copy()
    e1, e3 = V[:, 2].copy(), V[:, 0].copy()
    if e1[1] < 0:
        e1 = -e1
    if e3[2] < 0:
        e3 = -e3
    e2 = np.cross(e3, e1)
    A = np.stack([e1, e2, e3])
    out.update(status=0, mu=mu, C=C, lam=lam, A=A, xf=pack_rotation(A, mu))
    return out


def batch(depth, offsets, headers, depth_len=None, focal=F, cx=CX, cy=CY, eps=EPS):
    """One :func:`frame` per frame of a packed batch (camera constants as for :func:`cloud`); a bad header gives status 2,
    N = 0 and the identity."""
    depth_len = len(depth) if depth_len is None else depth_len
    out = []
    for i, h in enumerate(np.asarray(headers).reshape(-1, 6)):
        o0, o1 = int(offsets[i]), int(offsets[i + 1])
        if not header_ok(h, o0, o1, depth_len):
            out.append(dict(status=2, N=0, mu=np.zeros(3), C=np.zeros((3, 3)), lam=np.zeros(3), A=np.eye(3), xf=identity(),
                            pts=np.zeros((0, 3))))
        else:
            out.append(frame(depth[o0:o1], h, focal, cx, cy, eps))
    return out


def cov6(C):
    return np.array([C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]])


def apply(xf, p, inverse=False):
    """T(p) (or T^-1) for points [k,3] in float64."""
    m = np.asarray(xf, np.float64).reshape(2, 3, 4)[1 if inverse else 0]
    return np.asarray(p, np.float64) @ m[:, :3].T + m[:, 3]


def rel_gaps(lam):
    """The two gaps between neighbouring eigenvalues, relative to the trace."""
    t = lam.sum()
    return (lam[0] - lam[1]) / t, (lam[1] - lam[2]) / t
