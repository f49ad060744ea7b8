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
    with np.errstate(invalid="ignore", over="ignore"):   # an infinite depth is a valid pixel: the mean is not finite
        mu = pts.sum(axis=0) / N
        if not np.isfinite(mu).all():                    # the contract's rule: degenerate, the count kept, zero moments
            return out
        q = pts - mu
        C = (q.T @ q) / N
    if not np.isfinite(C).all() or np.trace(C) == 0:
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


# ---- the spectrum list: crops whose covariance has tied, vanishing or ill-conditioned eigenvalues ----------------------
HUGE = 2.0 ** 91      # about 2.5e27: a depth of 400..600 mm times it is of magnitude 1e30, an exact scaling in float32


def _iso(a, b):
    """9 x 9 pixels centred on the principal point, depth 500 + a s + b t with s = +-1 by the parity of |u| + |v| and
    t = sign(|u| - |v|): symmetric under u -> -u and v -> -v, so the covariance is diagonal; a sets the spread in z, b
    makes the pixels far out in x deeper than those far out in y."""
    u = np.arange(-4, 5)
    uu, vv = np.meshgrid(u, u)
    s = np.where((np.abs(uu) + np.abs(vv)) % 2 == 0, 1.0, -1.0)
    return (500.0 + a * s + b * np.sign(np.abs(uu) - np.abs(vv))).astype(np.float32)


def _iso_gaps(a, b):
    C = frame(_iso(a, b).reshape(-1), np.array([320, 240, 156, 116, 165, 125], np.int32))["C"]
    return np.array([C[0, 0] - C[1, 1], C[1, 1] - C[2, 2]]) / np.trace(C)


def _near_isotropic(target=3e-5):
    """(a, b) of :func:`_iso` with Cxx - Cyy = Cyy - Czz = target * trace: Newton's method on the float32 depths."""
    x = np.array([5.35, 0.0])
    for _ in range(12):
        f = _iso_gaps(*x) - target
        h = 1e-2
        Jm = np.stack([(_iso_gaps(x[0] + h, x[1]) - target - f) / h, (_iso_gaps(x[0], x[1] + h) - target - f) / h], axis=1)
        x = x - np.linalg.solve(Jm, f)
    return x


_spectrum = None


def spectrum():
    """[(name, left, top, img float32[h, w])] in a 320 x 240 image under the default camera.  Made once, never modified;
    tests/test_obb_hard_cpu.py asserts on the restatement what each name claims."""
    global _spectrum
    if _spectrum is not None:
        return _spectrum
    rng = np.random.default_rng(20261022)
    inf = np.float32(np.inf)
    out = [("plane_const", 100, 80, np.full((9, 13), 500.0)),                    # fronto-parallel: lambda_3 = 0
           ("square_centred", 156, 116, np.full((9, 9), 500.0))]                 # and lambda_1 = lambda_2
    three = np.zeros((4, 7))
    three[1, [0, 3, 6]] = 500.0
    out.append(("three_collinear", 158, 30, three))
    tri = np.zeros((4, 7))
    tri[0, 1], tri[3, 0], tri[2, 6] = 480.0, 510.0, 495.0
    out.append(("three_triangle", 40, 50, tri))
    line = np.float32(500.0) + rng.integers(0, 33, (1, 300)).astype(np.float32) * np.float32(2.0 ** -15)   # ulps of 500
    out.append(("near_collinear", 10, 100, line))
    out.append(("near_isotropic", 156, 116, _iso(*_near_isotropic())))
    # a plane in space is linear in 1 / d over the pixels
    r, c = np.mgrid[0:20, 0:30]
    plane = 1.0 / (1.0 / 450.0 + 1.2e-5 * c - 0.9e-5 * r)
    out.append(("tilted_plane", 70, 60, plane))
    blob = 400.0 + 200.0 * rng.random((5, 7))
    blob[1, 2] = 0.0
    out.append(("huge", 120, 100, blob.astype(np.float32) * np.float32(HUGE)))
    one = (450.0 + 40.0 * rng.random((6, 5))).astype(np.float32)
    one[2, 3] = inf
    out.append(("one_inf", 200, 100, one))
    both = one.copy()
    both[4, 1] = -inf
    out.append(("pm_inf", 30, 150, both))
    _spectrum = tuple((name, left, top, np.ascontiguousarray(img, np.float32)) for name, left, top, img in out)
    for e in _spectrum:
        e[3].setflags(write=False)
    return _spectrum


def spectrum_pack():
    """(depth, offsets, headers) of :func:`spectrum`."""
    sp = spectrum()
    depth = np.concatenate([img.reshape(-1) for _, _, _, img in sp])
    off = np.concatenate([[0], np.cumsum([img.size for _, _, _, img in sp])]).astype(np.int64)
    hdr = np.array([[320, 240, left, top, left + img.shape[1], top + img.shape[0]] for _, left, top, img in sp], np.int32)
    return depth, off, hdr


def rescaled(f, s):
    """The restatement's frame ``f`` with every length multiplied by s (a power of two: exact)."""
    return dict(f, mu=f["mu"] * s, C=f["C"] * s * s, lam=f["lam"] * s * s, pts=f["pts"] * s, xf=None)
