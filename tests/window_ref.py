"""The SEARCH WINDOWS of the two accurate kernels restated in numpy float64, and the mistakes a window can carry.  Test
infrastructure only; nothing here is read from a library.

Both kernels discard, per item of 4 consecutive voxels of the fastest axis, every pixel outside a rectangle
[c0, c1) x [r0, r1) before they evaluate s; the heads of csrc/tsdf_accurate.hip and csrc/tsdf_mapaccurate.hip derive it.  A
rectangle that is too small silently returns a wrong ``nearest``, so the derivation is restated here operation for operation
— the union over the item's 4 voxels in both layouts, T' = T (1 + 2^-20), the four corner quotients, ``floor - 1`` /
``ceil + 2``, the clip to the crop; for the mapped kernel B by cofactors, h_a, ||B||_F, rho, the slack term, the trust
conditions and "no finite rectangle => the whole crop" — and ``mistake=`` names one way of getting it wrong:

    plain  (``plain_window``):   "no_union"      voxel 0's coordinate ranges stand for the item's
                                 "two_corners"   two of the four corner quotients: (lo, d_lo) and (hi, d_hi)
                                 "no_depth_T"    the depth interval without +-T'
                                 "T90"           0.90 T in place of T'
    mapped (``mapped_window``):  "no_union", "T90" as above
                                 "no_Hz"         the depth interval without H_z
                                 "col_norms"     h_a from B's columns instead of its rows
                                 "h1"            h_a = 1
    both:                        "shrink2"       every side 2 pixels further in

``lost`` counts what a window loses: the non-fragile near voxels whose reference-nearest pixel lies outside their item's
rectangle.  tests/test_window_cpu.py asserts that the kernels' formula loses none on any GPU input, and that the GPU inputs
are ADEQUATE: each listed mistake loses at least 8 voxels on them, so a kernel that made it would fail its GPU tier.

"shrink2" is not on that list and cannot be.  The first of its two pixels is the one the kernels add beyond floor / ceil:
a safety margin against the few roundings of the corner values (relative 2^-53 on pixel coordinates below 2^31) that no
correct input can reach, because a point within T of a voxel projects inside the UNROUNDED rectangle.  The second pixel
cuts into the unrounded rectangle, but that rectangle's extremes are those of the BOX |t_c| <= T' at its corners, and the
corners lie outside the ball |t| <= 1 a near pixel is in: the mistake lost nothing on any input tried, dense or sparse, so
the suite cannot be asked to see it.  It is offered for measuring only."""
import numpy as np

import accurate_ref as ar
import map_geom_ref as mg

PLAIN_MISTAKES = ("no_union", "two_corners", "no_depth_T", "T90")
MAPPED_MISTAKES = ("no_union", "no_Hz", "col_norms", "h1", "T90")
TW = 1.0 + 2.0 ** -20


def _union(a, axis, mistake):
    """(lo, hi) of ``a`` over the items of 4 along ``axis``, broadcast back to a's shape."""
    sh = list(a.shape)
    sh[axis] //= 4
    sh.insert(axis + 1, 4)
    r = a.reshape(sh)
    if mistake == "no_union":
        lo = hi = np.take(r, [0], axis=axis + 1)
    else:
        lo, hi = r.min(axis=axis + 1, keepdims=True), r.max(axis=axis + 1, keepdims=True)
    return np.broadcast_to(lo, sh).reshape(a.shape), np.broadcast_to(hi, sh).reshape(a.shape)


def _rectangle(xa, xb, ya, yb, dlo, dhi, header, cam, mistake):
    """The corner quotients, the outward rounding and the clip.  Every argument [z][y][x]; returns int64 (c0, c1, r0, r1) and
    ``finite`` — where it is False there is no rectangle and the four are the crop's."""
    F, cx, cy, eps, _ = ar._cam5(cam)
    left, top, right, bottom = (int(v) for v in np.asarray(header)[2:6])
    finite = (dlo >= eps) | (dhi <= -eps)
    with np.errstate(all="ignore"):
        i0, i1 = 1.0 / dlo, 1.0 / dhi
        if mistake == "two_corners":
            X, Y = np.stack([xa * i0, xb * i1]), np.stack([ya * i0, yb * i1])
        else:
            X, Y = np.stack([xa * i0, xa * i1, xb * i0, xb * i1]), np.stack([ya * i0, ya * i1, yb * i0, yb * i1])
        k = 2.0 if mistake == "shrink2" else 0.0
        c0 = np.floor(cx + F * X.min(0)) - 1.0 + k
        c1 = np.ceil(cx + F * X.max(0)) + 2.0 - k
        r0 = np.floor(cy - F * Y.max(0)) - 1.0 + k
        r1 = np.ceil(cy - F * Y.min(0)) + 2.0 - k
    out = []
    for b, lo, hi, whole in ((c0, left, right, left), (c1, left, right, right), (r0, top, bottom, top), (r1, top, bottom, bottom)):
        b = np.where(np.isnan(b), whole, np.clip(b, lo, hi))            # clip_lo / clip_hi: a NaN selects the whole side
        out.append(np.where(finite, b, whole).astype(np.int64))
    return (*out, finite)


def _grid3(R):
    return np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")      # zz, yy, xx


def plain_window(grid_row, header, R, layout, cam=None, mistake=None):
    """tsdf_grid_accurate_kernel's rectangle per voxel (that of its item), indexed [z][y][x]: (c0, c1, r0, r1, finite)."""
    assert mistake is None or mistake in PLAIN_MISTAKES + ("shrink2",)
    row = np.asarray(grid_row, np.float32)
    c = ar.centres(row[:3], row[3], R)
    T = float(row[4])
    Tw = 0.90 * T if mistake == "T90" else T * TW
    zz, yy, xx = _grid3(R)
    vx, vy, vz = c[0][xx], c[1][yy], c[2][zz]
    if ar.LAYOUTS[layout] == 0:                      # an item runs along x
        (xlo, xhi), (zlo, zhi) = _union(vx, 2, mistake), (vz, vz)
    else:                                            # ... along z
        (xlo, xhi), (zlo, zhi) = (vx, vx), _union(vz, 0, mistake)
    dT = 0.0 if mistake == "no_depth_T" else Tw
    return _rectangle(xlo - Tw, xhi + Tw, vy - Tw, vy + Tw, -zhi - dT, -zlo + dT, header, cam, mistake)


def window_consts(xf):
    """(B float64[3,3], h[3], ||B||_F, 2 rho' or NaN) as tsdf_mapaccurate.hip::window_consts has them: the inverse of the
    forward 3x3 by cofactors, in its order of operations."""
    a = np.asarray(xf, np.float64).reshape(24)[:12].reshape(3, 4)[:, :3]
    with np.errstate(all="ignore"):
        k00 = a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]
        k01 = a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2]
        k02 = a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0]
        det = (a[0, 0] * k00 + a[0, 1] * k01) + a[0, 2] * k02
        inv = np.float64(1.0) / det
        B = np.array([[k00 * inv, (a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2]) * inv, (a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]) * inv],
                      [k01 * inv, (a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0]) * inv, (a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]) * inv],
                      [k02 * inv, (a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1]) * inv, (a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]) * inv]])
        nA = np.sqrt((a * a).sum())
        h = np.sqrt((B * B).sum(axis=1))
        nB = np.sqrt((B * B).sum())
        res = np.array([[((B[i, 0] * a[0, j] + B[i, 1] * a[1, j]) + B[i, 2] * a[2, j]) - (1.0 if i == j else 0.0)
                         for j in range(3)] for i in range(3)])
        rho = np.sqrt((res * res).sum())
        trusted = bool(nA <= 2.0 ** 20 and nB <= 2.0 ** 20 and nA * nB <= 2.0 ** 16 and rho <= 2.0 ** -24)   # a NaN fails each
    return B, h, nB, (2.0 * (rho + 2.0 ** -30) if trusted else np.nan)


def mapped_window(grid_row, header, R, layout, xf, cam=None, mistake=None):
    """tsdf_map_grid_accurate_kernel's rectangle per voxel (that of its item), indexed [z][y][x]: (c0, c1, r0, r1, finite)."""
    assert mistake is None or mistake in MAPPED_MISTAKES + ("shrink2",)
    xf = np.asarray(xf, np.float64).reshape(24)
    left, top, right, bottom = (int(v) for v in np.asarray(header)[2:6])
    row = np.asarray(grid_row, np.float32)
    B, h, nB, rho2 = window_consts(xf)
    zz, yy, xx = _grid3(R)
    if not rho2 == rho2:                             # the inverse is not trusted: the whole crop for every item
        full = np.ones_like(zz)
        return left * full, right * full, top * full, bottom * full, np.zeros(zz.shape, bool)
    if mistake == "col_norms":
        h = np.sqrt((B * B).sum(axis=0))
    elif mistake == "h1":
        h = np.ones(3)
    T = float(row[4])
    Tw = 0.90 * T if mistake == "T90" else T * TW
    vx, vy, vz = mg.centres(row, R)
    wx, wy, wz = (vx - xf[3])[xx], (vy - xf[7])[yy], (vz - xf[11])[zz]               # v' - b
    c = np.stack([(B[i, 0] * wx + B[i, 1] * wy) + B[i, 2] * wz for i in range(3)])   # B (v' - b): [3][z][y][x]
    clo, chi = _union(c, 3 if ar.LAYOUTS[layout] == 0 else 1, mistake)
    c1n = np.maximum(np.abs(clo), np.abs(chi)).sum(axis=0)
    slack = rho2 * c1n + rho2 * (nB * Tw)            # 2 rho' (|c|_1 + ||B||_F T')
    H = [Tw * h[i] + slack for i in range(3)]
    Hz = 0.0 if mistake == "no_Hz" else H[2]
    return _rectangle(clo[0] - H[0], chi[0] + H[0], clo[1] - H[1], chi[1] + H[1], -chi[2] - Hz, -clo[2] + Hz, header, cam,
                      mistake)


def lost(ref, header, window):
    """(lost, counted): the non-fragile near voxels of a reference dict (accurate_ref.accurate_frame / mapaccurate_ref.frame,
    indexed [z][y][x]) whose nearest pixel lies outside ``window`` = (c0, c1, r0, r1, finite), and how many were looked at."""
    c0, c1, r0, r1, _ = window
    left, top, right, bottom = (int(v) for v in np.asarray(header)[2:6])
    bw = right - left
    sel = ref["near"] & ~ref["fragile"]
    nn = ref["nearest"].astype(np.int64)
    col, rw = left + nn % bw, top + nn // bw
    inside = (col >= c0) & (col < c1) & (rw >= r0) & (rw < r1)
    return int((sel & ~inside).sum()), int(sel.sum())
