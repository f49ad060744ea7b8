"""CPU reference of tsdf_voxelize_map_grid_accurate_hip (include/tsdf_mapaccurate.h) for the tests: the accurate directional
TSDF under a per-frame map restated by brute force in numpy float64 — T(w) of every valid pixel from the FORWARD rows, the
scaled squared distance s of EVERY (voxel, mapped point) pair, in chunks, its minimum (ties to the lowest row-major crop
index: numpy's argmin over pixels listed in that order; a NaN s counts as +inf, it wins no comparison) and the second best
over the other pixels —, with ``rejected`` and ``negative`` taken from the geometric reference of the mapped projective
pass, ``map_geom_ref.gather`` / ``distances`` with the xform's own INVERSE rows, and the entry's status rules applied in
Python as tests/accurate_ref.py does.

Next to the volume and ``nearest`` it returns the FRAGILE mask: ``|s(p*) - 1| <= 2^-30``, or near with
``second - s(p*) <= 2^-30``, or the projected pixel valid with ``|t_z| <= 2^-30`` (there the sign may fall either way).
Comparison is ``accurate_ref.compare`` unchanged: outside the fragile set ``nearest`` is equal and far values are bit-exact,
near values lie within 1e-5, and at most 1e-4 of a case's voxels may be fragile — a condition on the inputs, not a
measurement (an input that exceeds it is replaced, the cap is not).

The inputs both tiers use are listed here (``ALL``), computed once per process and never modified."""
import importlib

import numpy as np

import accurate_ref as ar
import map_geom_ref as mg
import oracle
from auggrid_ref import grid_ok, header_ok

FRAGILE_EPS = ar.FRAGILE_EPS
LD = np.longdouble


def cam5(cam):
    return ar._cam5(cam)


def mapped_points(depth, header, xf, cam=None):
    """(crop index int64[P], T(w) float64[P,3]) of the valid pixels of one crop, row-major, under the forward rows."""
    idx, w = ar.points(depth, header, cam)
    f = np.asarray(xf, np.float64).reshape(24)[:12].reshape(3, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        tw = np.stack([f[i, 0] * w[:, 0] + f[i, 1] * w[:, 1] + f[i, 2] * w[:, 2] + f[i, 3] for i in range(3)], axis=1)
    return idx, tw


def frame(depth, header, grid_row, R, xf, cam=None):
    """One position with a usable header and grid row, everything indexed [z][y][x] (layout czyx):
    dict(vol float32[3,R,R,R], nearest int32[R,R,R], fragile, near bool[R,R,R], s_best, s_second float64[R,R,R],
    proj float32[3,R,R,R] (the mapped projective volume by its definition), far float32[R,R,R] (a far voxel's value),
    valid bool (not rejected), negative bool, pix int64 (the projected pixel's crop index, -1 where rejected),
    s_proj float64 (the projected pixel's s where valid), tz float64 (its t_z))."""
    c5 = cam5(cam)
    depth = np.ascontiguousarray(depth, np.float32)
    header = np.ascontiguousarray(header, np.int32)
    row = np.asarray(grid_row, np.float32)
    xf = np.asarray(xf, np.float64).reshape(24)
    left, top, right, bottom = (int(v) for v in header[2:6])
    with np.errstate(all="ignore"):
        valid, px, py, pd = mg.gather(depth, header, row, R, xf, c5)
        u, t = mg.distances(valid, px, py, pd, row, R, xf, c5)
        proj, _, proj_fragile = mg.finish(valid, u, t)
        negative = valid & (u[2] < 0)
        s_proj = np.where(valid, (t[0] * t[0] + t[1] * t[1] + t[2] * t[2]).astype(np.float64), np.inf)
        tz = np.where(valid, t[2].astype(np.float64), np.inf)
    pix = np.where(valid, (py - top) * (right - left) + (px - left), -1)
    far = np.where(valid, np.where(negative, np.float32(-1), np.float32(1)), np.float32(0)).astype(np.float32)

    td = np.float64(row[4])
    vx, vy, vz = mg.centres(row, R)
    zz, yy, xx = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
    v = np.stack([vx[xx.ravel()], vy[yy.ravel()], vz[zz.ravel()]], axis=1)            # [R^3, 3] in z, y, x order
    idx, tw = mapped_points(depth, header, xf, cam)
    nv, P = v.shape[0], len(idx)
    s_best = np.full(nv, np.inf)
    s_second = np.full(nv, np.inf)
    arg = np.zeros(nv, np.int64)
    if P:
        step = max(1, ar.CHUNK_PAIRS // P)
        for b in range(0, nv, step):
            vb = v[b:b + step]
            with np.errstate(invalid="ignore", over="ignore"):
                s = (((vb[:, None, 0] - tw[None, :, 0]) / td) ** 2 + ((vb[:, None, 1] - tw[None, :, 1]) / td) ** 2 +
                     ((vb[:, None, 2] - tw[None, :, 2]) / td) ** 2)
            s[np.isnan(s)] = np.inf
            k = np.argmin(s, axis=1)
            rows = np.arange(len(vb))
            s_best[b:b + step] = s[rows, k]
            arg[b:b + step] = k
            if P > 1:
                s[rows, k] = np.inf
                s_second[b:b + step] = s.min(axis=1)
    near = s_best <= 1.0
    vol = np.repeat(far.reshape(1, nv), 3, axis=0).copy()
    nearest = np.full(nv, -1, np.int32)
    if P and near.any():
        with np.errstate(invalid="ignore", over="ignore"):
            m = np.minimum(np.abs(v - tw[arg]) / td, 1.0).astype(np.float32)          # [R^3, 3]
        sign = np.where(negative.ravel(), np.float32(-1), np.float32(1))
        vol[:, near] = (m * sign[:, None]).T[:, near]
        nearest[near] = idx[arg[near]].astype(np.int64).astype(np.int32)
    sh = (R, R, R)
    with np.errstate(invalid="ignore"):   # inf - inf where there is no candidate at all
        fragile = (np.abs(s_best - 1.0) <= FRAGILE_EPS) | (near & (s_second - s_best <= FRAGILE_EPS))
    fragile = fragile.reshape(sh) | (valid & (np.abs(tz) <= FRAGILE_EPS))
    return dict(vol=vol.reshape(3, R, R, R), nearest=nearest.reshape(sh), fragile=fragile, near=near.reshape(sh),
                s_best=s_best.reshape(sh), s_second=s_second.reshape(sh), proj=proj, proj_fragile=proj_fragile, far=far,
                valid=valid, negative=negative, pix=pix, s_proj=s_proj, tz=tz)


def voxelize_map_grid_accurate_ref(depth, off, hdr, xforms, grid, R, layout, cam=None, index=None, depth_len=None,
                                   frames=None):
    """(tsdf float32[n,3,R,R,R], status int32[n], nearest int32[n,R,R,R], fragile bool[n,R,R,R]) as
    tsdf_voxelize_map_grid_accurate_hip defines them: source tables by ``index``, ``xforms`` / ``grid`` per batch position.
    ``frames``: {position: frame() dict} computed elsewhere for positions that are OK (the tests' memoised cases)."""
    depth = np.ascontiguousarray(depth, np.float32)
    off = np.asarray(off, np.int64)
    hdr = np.asarray(hdr, np.int32).reshape(-1, 6)
    n_src = hdr.shape[0]
    index = np.arange(n_src) if index is None else np.asarray(index, np.int64)
    n = len(index)
    grid = np.asarray(grid, np.float32).reshape(n, 8)
    xforms = np.asarray(xforms, np.float64).reshape(n, 24)
    depth_len = depth.size if depth_len is None else int(depth_len)
    tsdf = np.zeros((n, 3, R, R, R), np.float32)
    nearest = np.full((n, R, R, R), -1, np.int32)
    fragile = np.zeros((n, R, R, R), bool)
    status = np.zeros(n, np.int32)
    for i, g in enumerate(index):
        g = int(g)
        if not 0 <= g < n_src:
            status[i] = 2
            continue
        o0, o1 = int(off[g]), int(off[g + 1])
        if not header_ok(hdr[g], o0, o1, depth_len):
            status[i] = 2
        elif not grid_ok(grid[i]):
            status[i] = 1
        else:
            r = frames[i] if frames is not None and i in frames else frame(depth[o0:o1], hdr[g], grid[i], R, xforms[i], cam)
            tsdf[i], (nearest[i], fragile[i]) = ar.to_layout(r["vol"], (r["nearest"], r["fragile"]), layout)
    return tsdf, status, nearest, fragile


# ---- the inputs both tiers use -------------------------------------------------------------------------------------
PKG = ar.PKG
NON_EXACT = tuple(m for m in mg.MAPS if m not in mg.EXACT)      # nine maps
CROPS_R12 = (0, 3)                                              # of map_geom_ref's six synthetic crops
CROP_R20 = 1
IDENTITY_INV = np.array([1., 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
_memo = {}


def _synth6():
    if "synth6" not in _memo:
        _memo["synth6"] = importlib.import_module(PKG + ".synth").synth_batch(mg.N_CROPS, "crop", seed0=mg.SEED0)
    return _memo["synth6"]


def source(kind, name):
    """(depth, header, id) of a named crop: ("synth", k) is crop k of map_geom_ref's six, ("golden", fixture) a fixture,
    ("camera", k) frame k of tests/camera_ref.py's batch A."""
    if kind == "synth":
        d6, o6, h6 = _synth6()
        return np.ascontiguousarray(d6[o6[name]:o6[name + 1]], np.float32), np.asarray(h6[name], np.int32), int(name)
    if kind == "camera":
        import camera_ref as cr
        d, o, h = cr.take(*cr.batch_a(), (name,))
        return np.ascontiguousarray(d, np.float32), np.asarray(h[0], np.int32), int(name)
    d, h = ar.frame_of("golden", name)
    return d, h, 0


def placement_row(depth, header, xf, R, cam=None):
    """The grid row (vox_ori[3], voxel_len, trunc_dis, 0, 0, 0) the glue places on the mapped cloud's float32 AABB, and max_l."""
    mn, mx, _ = mg.placement(depth, header, xf, cam=cam5(cam))
    g, ori = oracle.glue(mn, mx, R, cam)
    row = np.zeros(8, np.float32)
    row[:3], row[3], row[4] = ori, g[4], g[5]
    return row, g[3]


def xform(kind, name, map_name, cam=None):
    """float64[24] of a crop under a map of map_geom_ref.MAPS, or under one of the two broken forward parts: "singular"
    (A = diag(1, 1, 0)) and "nanfwd" (the shear with A_00 = NaN), both with the identity's inverse rows."""
    depth, header, cid = source(kind, name)
    off = np.array([0, depth.size], np.int64)
    if map_name in ("singular", "nanfwd"):
        A = np.diag([1.0, 1.0, 0.0]) if map_name == "singular" else mg.MATRICES["shear"].copy()
        if map_name == "nanfwd":
            A[0, 0] = np.nan
        m = mg.centre(depth, header, cam5(cam))
        b = np.array([5.0, -3.0, m[2]])
        return np.concatenate([np.concatenate([A, b[:, None]], 1).ravel(), IDENTITY_INV])
    return mg.xforms_for([map_name], depth, off, header[None], cam5(cam), ids=[cid])[0]


def case(kind, name, map_name, R, variant=None, cam=None):
    """A one-position case, computed once and never modified: dict(depth, off, hdr, xf float64[1,24], grid float32[1,8],
    ref = frame()'s dict).  The row is the pair's own placement (the broken maps stand on the identity's).  ``variant``:
    "shifted" — the row moved by 0.75 * max_l along x, so that most voxels are far; "wrong_inverse" — the inverse rows
    replaced by the identity's, so they are NOT the inverse of the forward rows."""
    key = (kind, name, map_name, R, variant, cam)
    if key not in _memo:
        depth, header, _ = source(kind, name)
        xf = xform(kind, name, map_name, cam)
        place_xf = xform(kind, name, "identity", cam) if map_name in ("singular", "nanfwd") else xf
        row, max_l = placement_row(depth, header, place_xf, R, cam)
        if variant == "shifted":
            row[0] += np.float32(0.75) * max_l
        elif variant == "wrong_inverse":
            xf = np.concatenate([xf[:12], IDENTITY_INV])
        else:
            assert variant is None
        _memo[key] = dict(depth=depth, off=np.array([0, depth.size], np.int64), hdr=header[None].copy(), xf=xf[None].copy(),
                          grid=row[None].copy(), ref=frame(depth, header, row, R, xf, cam))
    return _memo[key]


def camera():
    import camera_ref as cr
    return tuple(cr.FRACTIONAL)


# (label, key of case()) of every one-position case the GPU tier compares
PAIRS_R12 = [(f"{m} crop{c} R=12", ("synth", c, m, 12, None, None)) for m in mg.MAPS for c in CROPS_R12]
PAIRS_R20 = [(f"{m} crop{CROP_R20} R=20", ("synth", CROP_R20, m, 20, None, None)) for m in NON_EXACT]
SLAB_EDGES = [(f"general small_odd R={R}", ("golden", "small_odd", "general", R, None, None)) for R in (4, 64)]
NO_RECTANGLE = [(f"{m} {g} R=12", ("golden", g, m, 12, None, None)) for g in ("mixed_halves", "neg_all_flip")
                for m in ("rx100", "mirror")]
SHIFTED = [("general crop0 R=12 shifted", ("synth", 0, "general", 12, "shifted", None))]
WRONG_INVERSE = [("rx100 crop0 R=12 wrong inverse", ("synth", 0, "rx100", 12, "wrong_inverse", None))]
BROKEN = [(f"{m} crop0 R=12", ("synth", 0, m, 12, None, None)) for m in ("singular", "nanfwd")]


def camera_pairs():
    return [("shear camera0 R=12 f300", ("camera", 0, "shear", 12, None, camera()))]


def all_cases():
    return PAIRS_R12 + PAIRS_R20 + SLAB_EDGES + NO_RECTANGLE + SHIFTED + WRONG_INVERSE + BROKEN + camera_pairs()


def batch(keys):
    """The cases ``keys`` as one batch, every position its own source frame: (depth, off, hdr, xforms, grid, [case])."""
    cs = [case(*k) for k in keys]
    depth = np.concatenate([c["depth"] for c in cs])
    off = np.cumsum([0] + [c["depth"].size for c in cs]).astype(np.int64)
    return (depth, off, np.concatenate([c["hdr"] for c in cs]), np.concatenate([c["xf"] for c in cs]),
            np.concatenate([c["grid"] for c in cs]), cs)
