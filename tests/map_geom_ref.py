"""Geometric reference of the mapped (augmented) voxel contract — numpy only, no ctypes, no oracle import.

include/tsdf.h defines the mapped volume in one sentence: "the truncated distances are those between v' and T(w), w the
surface point of the gathered pixel".  oracle/tsdf_oracle.c evaluates that sentence in a cheap algebraic form that never
forms w or T(w); the kernels follow the cheap form.  This module restates the SENTENCE: it forms w, then T(w), then
v' - T(w), in ``numpy.longdouble`` (asserted below to carry >= 63 mantissa bits: x87 extended precision), and rounds once
to float32.  Only the choice of the pixel follows the contract's float64 order, because which pixel a voxel gathers is
part of the definition and not of the arithmetic under test; numpy float64 never contracts a product into a sum, so that
restatement is exact.

What it offers: :func:`voxels` (volume, valid mask, fragile mask on a given grid row), :func:`placement` (the mapped
cloud's float32 AABB) with :func:`placement_bounds`, :func:`joints` with :func:`joint_bound`, and the named map family
:data:`MAPS` with :func:`xforms_for`.  Test infrastructure only.

The placement bound
-------------------
Let M be the largest |coordinate| of the mapped AABB and E the float32 spacing at M (E = 2^(floor(log2 M) - 23), so
M < 2^24 E and spacing(y) <= 2^-23 |y| < 2 E |y| / M for any y; a y with |y| <= 2M has spacing <= 2E).  The contract
rounds a float64 fma chain to float32, this module rounds the longdouble value: both are within 1e-12 mm of the exact
T(p), so the two float32 results are equal or neighbours, and since rounding is monotone the same holds for the min and
the max over the pixels: every one of the six extremes differs by at most E ("inherited" below).  The glue
(tsdf_oracle_glue, all float32, one rounding per operation) then gives, comparing two evaluations whose inputs differ by
d: |fl(a) - fl(b)| <= d + spacing/2 + spacing/2 ("own").

    mid_p     = (mn + mx) / 2       inherited 2E, |mn + mx| <= 2M so own 2 * (2E / 2) = 2E; halving is exact   -> 2 E
    len       = mx - mn             inherited 2E, |len| <= 2M so own 2E                                         -> 4 E
    max_l     = max(len)            max is 1-Lipschitz                                                          -> 4 E
    voxel_len = max_l / R           inherited 4E / R; voxel_len <= 2M / R has spacing < 4E / R, own 4E / R      -> 8 E / R
    vox_ori   = (mid_p - max_l / 2) + voxel_len / 2
                max_l / 2 exact (2E); the difference inherits 2E + 2E, |.| <= 2M so own 2E                       (6 E)
                voxel_len / 2 exact (4E / R); the sum inherits 6E + 4E / R, |vox_ori| <= 2M so own 2E           -> 8 E + 4 E / R

The label bound
---------------
T(joint): the contract's three fmas in float64 err by at most 3 * 2^-53 * S (S = sum_j |A_ij| |p_j| + |b_i|), this
module's longdouble by less.  Where that is below the float32 spacing at the result — asserted by :func:`joint_bound` —
the two float32 roundings are equal or neighbours: one float32 spacing at the result (double rounding).
"""
import numpy as np

import obb_ref

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "numpy.longdouble is not extended precision here"

DEFAULT_CAM = (241.42, 160.0, 120.0, 1.0, 3.0)     # focal, cx, cy, invalid_eps, trunc_voxels (include/tsdf.h)
FRAGILE = 2.0 ** -30
I32_MAX, I32_MIN = 2147483647.0, -2147483648.0


# ---- the map family ----------------------------------------------------------------------------------------------

def _rot(axis, deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    A = np.eye(3)
    A[i, i], A[i, j], A[j, i], A[j, j] = c, -s, s, c
    return A


_CYC = np.array([[0., 1, 0], [0, 0, 1], [1, 0, 0]])        # T(p) = (p_y, p_z, p_x)
# name -> 3x3 A (None: the frame's own principal-axis map, tests/obb_ref.py)
MATRICES = {
    "identity": np.eye(3),
    "rx100": _rot(0, 100), "ry-135": _rot(1, -135), "rz90": _rot(2, 90), "rz180": _rot(2, 180),
    "aniso": np.diag([0.5, 1.7, 1.2]),
    "shear": np.array([[1, .4, -.3], [.2, 1, .5], [-.35, .25, 1]]),
    "mirror": np.diag([-1., 1, 1]),
    "general": _rot(0, 40) @ np.diag([1.4, .7, 1.1]) @ _rot(2, -70) @ np.array([[1, .3, 0], [0, 1, .2], [0, 0, 1.]]),
    "obb": None,
    "half": 0.5 * np.eye(3), "x2": 2.0 * np.eye(3), "x4": 4.0 * np.eye(3),
    "cyc": _CYC, "cyc2": _CYC @ _CYC,
}
MAPS = tuple(MATRICES)                                      # 15 names, a fixed order
EXACT = ("identity", "half", "x2", "x4", "cyc", "cyc2")     # b = 0: related to the identity volume bit for bit
SCALES = {"half": 0.5, "x2": 2.0, "x4": 4.0}
# sigma of the cyclic maps: mapped axis a is camera axis CYCLES[name][a]
CYCLES = {"cyc": (1, 2, 0), "cyc2": (2, 0, 1)}


def pack(A, b):
    """float64[24]: forward rows {A_i0, A_i1, A_i2, b_i}, then the inverse map likewise (augment.pack_affine's layout and
    formulas, restated so that this module needs nothing but numpy)."""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    Ai = np.linalg.inv(A)
    bi = -np.einsum("...ij,...j->...i", Ai, b)
    return np.concatenate([np.concatenate([A, b[:, None]], 1).ravel(), np.concatenate([Ai, bi[:, None]], 1).ravel()])


def cloud(depth, header, cam=DEFAULT_CAM):
    """longdouble[N,3]: the back-projected point of every valid pixel, p = d * ((x - cx) / F, -(y - cy) / F, -1)."""
    F, cx, cy, eps = LD(cam[0]), LD(cam[1]), LD(cam[2]), np.float32(cam[3])
    left, top, right, bottom = (int(v) for v in np.asarray(header)[2:6])
    d = np.asarray(depth, np.float32).reshape(bottom - top, right - left)
    with np.errstate(invalid="ignore"):
        i, j = np.nonzero(np.abs(d) >= eps)
    dl = d[i, j].astype(LD)
    return np.stack([dl * (((left + j).astype(LD) - cx) / F), -(dl * (((top + i).astype(LD) - cy) / F)), -dl], 1)


def centre(depth, header, cam=DEFAULT_CAM):
    """float64[3]: the middle of the un-mapped cloud's AABB — the point the maps of :func:`xforms_for` are built about."""
    p = cloud(depth, header, cam)
    return ((p.min(0) + p.max(0)) / 2).astype(np.float64)


def xforms_for(names, depth, off, hdr, cam=DEFAULT_CAM, seed=20, ids=None):
    """float64[n,24]: frame i under the map ``names[i]``.  A is MATRICES[name], b = m - A m + delta with m the frame's
    :func:`centre` and delta ~ N(0, 30 mm) from a generator seeded per (seed, map, ids[i]) — ``ids`` (default 0..n-1) names
    the crops, so that a crop gets the same map wherever it stands in a batch; the EXACT family has b = 0; ``obb`` is the
    frame's own principal-axis map under ``cam`` as tests/obb_ref.py packs it."""
    out = np.empty((len(names), 24))
    ids = range(len(names)) if ids is None else ids
    for i, name in enumerate(names):
        d, h = depth[off[i]:off[i + 1]], hdr[i]
        if name == "obb":
            f = obb_ref.frame(d, h, cam[0], cam[1], cam[2], cam[3])
            assert f["status"] == 0
            out[i] = f["xf"]
            continue
        A = MATRICES[name]
        if name in EXACT:
            b = np.zeros(3)
        else:
            m = centre(d, h, cam)
            b = m - A @ m + np.random.default_rng([seed, MAPS.index(name), int(ids[i])]).normal(0, 30.0, 3)
        out[i] = pack(A, b)
    return out


# ---- the inputs both tiers use -----------------------------------------------------------------------------------

N_CROPS, SEED0 = 6, 1200


def take(depth, off, hdr, frames):
    """The frames ``frames`` (any order, repeats allowed) of a pack as a pack of their own."""
    parts = [depth[off[i]:off[i + 1]] for i in frames]
    o = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return np.concatenate(parts).astype(np.float32), o, np.asarray(hdr, np.int32).reshape(-1, 6)[list(frames)].copy()


def case_batch(synth, n, cam=DEFAULT_CAM, names=None):
    """n frames of the tests: position k holds crop (k mod 15) mod 6 of ``synth.synth_batch(6, "crop", seed0=1200)`` under
    the map MAPS[k mod 15] — a period of 15 positions, one per map —, or under ``names[k]`` when ``names`` is given (then
    crop k mod 6).  Returns (depth, off, hdr, names, xforms float64[n,24]); a crop's map depends on (map, crop) alone."""
    d6, o6, h6 = synth.synth_batch(N_CROPS, "crop", seed0=SEED0)
    if names is None:
        crops = [(k % len(MAPS)) % N_CROPS for k in range(n)]
        names = [MAPS[k % len(MAPS)] for k in range(n)]
    else:
        assert len(names) == n
        crops = [k % N_CROPS for k in range(n)]
    depth, off, hdr = take(d6, o6, h6, crops)
    return depth, off, hdr, list(names), xforms_for(names, depth, off, hdr, cam, ids=crops)


def all_pairs(synth, cam=DEFAULT_CAM):
    """Every (map, crop) pair as one batch of 15 * 6 frames, map-major: frame 6 * m + c is crop c under MAPS[m]."""
    d6, o6, h6 = synth.synth_batch(N_CROPS, "crop", seed0=SEED0)
    crops = [c for _ in MAPS for c in range(N_CROPS)]
    names = [m for m in MAPS for _ in range(N_CROPS)]
    depth, off, hdr = take(d6, o6, h6, crops)
    return depth, off, hdr, names, xforms_for(names, depth, off, hdr, cam, ids=crops)


# ---- the volume --------------------------------------------------------------------------------------------------

def trunc_i32(v):
    """int() of a float64 as the contract has it: toward zero, saturating, NaN -> 0."""
    with np.errstate(invalid="ignore"):
        t = np.where(np.isnan(v), 0.0, np.clip(np.trunc(v), I32_MIN, I32_MAX))
    return t.astype(np.int64)


def centres(grid_row, R):
    """float64 (vx, vy, vz), each [R]: v'_a = float64(ori_a) + idx * float64(voxel_len) (no half-voxel term)."""
    row = np.asarray(grid_row, np.float32)
    idx = np.arange(R, dtype=np.float64)
    return tuple(np.float64(row[a]) + idx * np.float64(row[3]) for a in range(3))


def camera_points(grid_row, R, xf):
    """float64 v = T^-1(v') per voxel, three arrays broadcastable to [z, y, x], from the xform's own inverse rows grouped
    (A_i0 x + A_i1 y) + (A_i2 z + b_i), every product and sum rounded separately."""
    inv = np.asarray(xf, np.float64).reshape(24)[12:].reshape(3, 4)
    vx, vy, vz = centres(grid_row, R)
    X, Y, Z = vx[None, None, :], vy[None, :, None], vz[:, None, None]
    return [(inv[i, 0] * X + inv[i, 1] * Y) + (inv[i, 2] * Z + inv[i, 3]) for i in range(3)]


def gather(depth, header, grid_row, R, xf, cam=DEFAULT_CAM):
    """The pixel every voxel gathers, float64 in the contract's order -> (valid bool[R,R,R], pix_x, pix_y, pd float32), all
    indexed [z, y, x]."""
    F, cx, cy = np.float64(cam[0]), np.float64(cam[1]), np.float64(cam[2])
    eps = np.float32(cam[3])
    left, top, right, bottom = (int(v) for v in np.asarray(header)[2:6])
    bw = right - left
    v = camera_points(grid_row, R, xf)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = -F / v[2]
        px = trunc_i32(v[0] * q + cx)
        py = trunc_i32((-v[1]) * q + cy)
    inside = (px >= left) & (px < right) & (py >= top) & (py < bottom)
    idx = np.where(inside, (py - top) * bw + (px - left), 0)
    pd = np.asarray(depth, np.float32)[idx]
    with np.errstate(invalid="ignore"):
        valid = inside & (np.abs(pd) >= eps)
    return valid, px, py, pd


def distances(valid, px, py, pd, grid_row, R, xf, cam=DEFAULT_CAM, fwd=None):
    """longdouble u = v' - T(w) [3,R,R,R] and t = u / trunc_dis for the gathered pixels (garbage where not valid).
    ``fwd`` (3x4) replaces the forward rows — the hook of the mutation tests, never used by the reference itself."""
    F, cx, cy = LD(cam[0]), LD(cam[1]), LD(cam[2])
    f = np.asarray(xf, np.float64).reshape(24)[:12].reshape(3, 4) if fwd is None else np.asarray(fwd, np.float64)
    f = f.astype(LD)
    pdl = np.where(valid, pd, np.float32(1)).astype(LD)
    w = [pdl * ((px.astype(LD) - cx) / F), -(pdl * ((py.astype(LD) - cy) / F)), -pdl]
    vx, vy, vz = centres(grid_row, R)
    vp = [vx.astype(LD)[None, None, :], vy.astype(LD)[None, :, None], vz.astype(LD)[:, None, None]]
    u = np.stack([np.broadcast_to(vp[i], valid.shape) - (f[i, 0] * w[0] + f[i, 1] * w[1] + f[i, 2] * w[2] + f[i, 3])
                  for i in range(3)])
    return u, u / LD(np.float32(np.asarray(grid_row, np.float32)[4]))


def finish(valid, u, t, layout="czyx", negative=None):
    """near iff |t|^2 <= 1; value near ? min(|t_i|, 1) : 1, negated iff u_z < 0; 0 where not valid; one rounding to float32.
    Returns (tsdf float32[3,R,R,R] in ``layout``, valid, fragile)."""
    s2 = t[0] * t[0] + t[1] * t[1] + t[2] * t[2]
    near = s2 <= 1
    val = np.where(near[None], np.minimum(np.abs(t), LD(1)), LD(1))
    neg = (u[2] < 0) if negative is None else negative
    val = np.where(neg[None], -val, val)
    out = np.where(valid[None], val, LD(0)).astype(np.float32)
    fragile = valid & ((np.abs(s2 - 1) <= FRAGILE) | (np.abs(t[2]) <= FRAGILE))
    if layout in ("cxyz", 1):
        out = np.ascontiguousarray(out.transpose(0, 3, 2, 1))
    return out, valid, fragile


def voxels(depth, header, grid_row, R, layout, xf, cam=DEFAULT_CAM):
    """The mapped volume of one frame on the grid row (vox_ori[3], voxel_len, trunc_dis, ...) by the definition.

    Returns (tsdf float32[3,R,R,R] in ``layout``, valid bool[R,R,R], fragile bool[R,R,R]); the two masks are indexed
    [z, y, x] whatever the layout.  ``fragile``: the valid voxels with | |t|^2 - 1 | <= 2^-30 or |t_z| <= 2^-30, the only
    places where a correctly rounded cheap form may land on the other side of a discontinuity."""
    g = gather(depth, header, grid_row, R, xf, cam)
    u, t = distances(*g, grid_row, R, xf, cam)
    return finish(g[0], u, t, layout)


def cyc_of_identity(vol, name, layout="czyx"):
    """What a cyclic map makes of the identity map's volume ``vol`` ([3,R,R,R] in ``layout``, numpy or torch): mapped axis a
    is camera axis s[a] (s = CYCLES[name]), so channel a is the identity's channel s[a] and mapped grid index j_a runs along
    the identity's grid axis s[a].  Signs are carried along as they are; compare magnitudes."""
    s = CYCLES[name]
    swap = (lambda v: v.permute(0, 3, 2, 1)) if hasattr(vol, "permute") else (lambda v: v.transpose(0, 3, 2, 1))
    w = swap(vol) if layout in ("czyx", 0) else vol                      # [channel, x, y, z]
    w = w[list(s)]
    w = w.permute(0, 1 + s[0], 1 + s[1], 1 + s[2]) if hasattr(w, "permute") else w.transpose(0, 1 + s[0], 1 + s[1], 1 + s[2])
    return swap(w) if layout in ("czyx", 0) else w


def mask_in(mask, layout):
    """A [z,y,x] mask as [1,...] in the volume's layout."""
    return (mask.transpose(2, 1, 0) if layout in ("cxyz", 1) else mask)[None]


# ---- placement and labels ----------------------------------------------------------------------------------------

def placement(depth, header, xf, R=None, cam=DEFAULT_CAM):
    """(min_p float32[3], max_p float32[3], M): the AABB of T(p) over the valid pixels, T(p) in longdouble rounded once to
    float32; M = the largest |coordinate| of that AABB.  (R is not needed for the AABB; it is accepted so that the call
    reads like the entry's.)"""
    f = np.asarray(xf, np.float64).reshape(24)[:12].reshape(3, 4).astype(LD)
    p = cloud(depth, header, cam)
    assert len(p)
    tp = (p @ f[:, :3].T + f[:, 3]).astype(np.float32)
    mn, mx = tp.min(0), tp.max(0)
    return mn, mx, float(max(np.abs(mn).max(), np.abs(mx).max()))


def placement_bounds(M, R):
    """dict of the derived bounds (module docstring) in mm for mid_p, max_l, voxel_len, vox_ori."""
    E = float(np.spacing(np.float32(M)))
    return dict(mid_p=2 * E, max_l=4 * E, voxel_len=8 * E / R, vox_ori=8 * E + 4 * E / R)


def joints(gt, xf):
    """T(joint) per frame in longdouble, rounded once to float32; gt float32[n,3J] or [n,J,3], xf float64[n,24]."""
    g = np.asarray(gt, np.float32)
    p = g.reshape(g.shape[0], -1, 3).astype(LD)
    f = np.asarray(xf, np.float64).reshape(-1, 2, 3, 4)[:, 0].astype(LD)
    out = (f[:, None, :, :3] * p[:, :, None, :]).sum(-1) + f[:, None, :, 3]
    return out.astype(np.float32).reshape(g.shape)


def joint_bound(gt, xf, ref):
    """One float32 spacing at every coordinate of ``ref`` (module docstring), after asserting its precondition."""
    g = np.asarray(gt, np.float32)
    p = np.abs(g.reshape(g.shape[0], -1, 3).astype(np.float64))
    f = np.abs(np.asarray(xf, np.float64).reshape(-1, 2, 3, 4)[:, 0])
    S = (f[:, None, :, :3] * p[:, :, None, :]).sum(-1) + f[:, None, :, 3]
    sp = np.spacing(np.abs(np.asarray(ref, np.float32))).astype(np.float64)
    assert (4 * 2.0 ** -53 * S.reshape(sp.shape) < sp).all(), "a joint maps too close to zero for the one-spacing bound"
    return sp
