"""SPARSE FRAMES for the tests of the two accurate kernels: a crop with a handful of valid pixels, seeded.  Test
infrastructure only; everything is numpy.

Two uses.  A sparse frame under a long focal length reaches the ground on which a search window that is slightly too small
loses the nearest pixel (tests/window_ref.py, tests/test_window_cpu.py): on dense hand crops at the default focal length
the corner bound is wider than needed by about T / d and the one-pixel outward rounding hides the rest.  And the
brute-force references (tests/accurate_ref.py, tests/mapaccurate_ref.py) cost (voxels x valid pixels): a frame with 16 - 24
valid pixels makes them affordable at R = 128, which is what the resolution and large-buffer tests need.

``frame`` is the generator; ``PLAIN`` / ``MAPPED`` are the fixed lists of one-position cases of the search-window tests
(``plain_case`` / ``mapped_case``: computed once per process, never modified); ``res_sources`` are the k = 3 sources of the
resolution and large-buffer tests with their references at one R."""
import numpy as np

import accurate_ref as ar
import map_geom_ref as mg
import mapaccurate_ref as mr

IMG_W, IMG_H = 320, 240
FULL = (0, 0, IMG_W, IMG_H)
LONG2000 = (2000.0, 160.0, 120.0, 1.0, 3.0)        # focal, cx, cy, invalid_eps, trunc_voxels
LONG3000 = (3000.0, 150.5, 130.25, 1.0, 3.0)       # ... with a fractional principal point


def frame(seed, npts, dlo, dhi, sign=1.0, box=FULL):
    """(depth float32[bw * bh], header int32[6]): ``npts`` valid pixels drawn without replacement in the crop ``box`` =
    (left, top, right, bottom), depths ``sign`` * uniform(dlo, dhi), every other pixel 0."""
    left, top, right, bottom = box
    n = (right - left) * (bottom - top)
    rng = np.random.default_rng(seed)
    k = rng.choice(n, npts, replace=False)
    depth = np.zeros(n, np.float32)
    depth[k] = sign * rng.uniform(dlo, dhi, npts)
    return depth, np.array([IMG_W, IMG_H, left, top, right, bottom], np.int32)


# name -> (frame's arguments, camera (None: the default), R, trunc_dis in voxel lengths (None: the camera's))
PLAIN = {
    # the grid reaches within T of the camera plane: items without a finite rectangle next to windowed ones
    "camera_plane": ((5, 40, 80.0, 200.0), None, 24, 6.0),
    # T below an item's extent of 3 voxel lengths, at a wide angle: the union along z (layout cxyz) decides
    "thin_shell": ((6, 40, 150.0, 300.0), None, 24, 1.5),
    "f2000": ((11, 24, 900.0, 1000.0), LONG2000, 16, None),
    "f3000": ((12, 40, 1400.0, 1500.0), LONG3000, 24, 4.0),
    "f3000_negative": ((13, 40, 1400.0, 1500.0, -1.0), LONG3000, 24, 4.0),
    # a crop box inside the frame: the clip to the crop cuts windows on each of its four sides
    "boxed": ((21, 24, 300.0, 420.0, 1.0, (101, 67, 222, 170)), None, 16, None),
}

# name -> (frame's arguments, map of map_geom_ref.MAPS, camera, R, trunc_dis in voxel lengths)
MAPPED = {
    "shear_f2000": ((11, 24, 900.0, 1000.0), "shear", LONG2000, 16, None),
    "aniso_f3000": ((12, 40, 1400.0, 1500.0), "aniso", LONG3000, 24, 4.0),
    "general_f3000_negative": ((13, 40, 1400.0, 1500.0, -1.0), "general", LONG3000, 24, 4.0),
    "general_f2000": ((14, 32, 900.0, 1000.0), "general", LONG2000, 20, 4.0),
    "rx100_camera_plane": ((5, 40, 80.0, 200.0), "rx100", None, 24, 6.0),
    "shear_boxed": ((21, 24, 300.0, 420.0, 1.0, (101, 67, 222, 170)), "shear", None, 16, None),
}

_memo = {}


def _row_with(row, trunc_k):
    if trunc_k is not None:
        row[4] = np.float32(trunc_k) * row[3]
    return row


def plain_case(name):
    """dict(depth, off, hdr, grid float32[1,8], ref, cam, R) of a PLAIN case: the row is accurate_ref.glue_row's."""
    key = ("plain", name)
    if key not in _memo:
        args, cam, R, trunc_k = PLAIN[name]
        depth, header = frame(*args)
        row = _row_with(ar.glue_row(depth, header, R, cam)[0], trunc_k)
        ref = ar.accurate_frame(depth, header, row[:3], row[3], row[4], R, cam)
        _memo[key] = dict(depth=depth, off=np.array([0, depth.size], np.int64), hdr=header[None].copy(), grid=row[None].copy(),
                          ref=ref, cam=cam, R=R)
    return _memo[key]


def _xform(depth, header, map_name, cam, cid):
    off = np.array([0, depth.size], np.int64)
    return mg.xforms_for([map_name], depth, off, header[None], mr.cam5(cam), ids=[cid])[0]


def mapped_case(name):
    """dict(depth, off, hdr, xf float64[1,24], grid float32[1,8], ref, cam, R) of a MAPPED case: the row is
    mapaccurate_ref.placement_row's."""
    key = ("mapped", name)
    if key not in _memo:
        args, map_name, cam, R, trunc_k = MAPPED[name]
        depth, header = frame(*args)
        xf = _xform(depth, header, map_name, cam, args[0])
        row = _row_with(mr.placement_row(depth, header, xf, R, cam)[0], trunc_k)
        ref = mr.frame(depth, header, row, R, xf, cam)
        _memo[key] = dict(depth=depth, off=np.array([0, depth.size], np.int64), hdr=header[None].copy(), xf=xf[None].copy(),
                          grid=row[None].copy(), ref=ref, cam=cam, R=R)
    return _memo[key]


# ---- the sources of the resolution and large-buffer tests -----------------------------------------------------------
# k = 3 frames under the default camera at hand depths, <= 24 valid pixels each: a full frame, a crop box, negative depths
RES_FRAMES = ((31, 24, 300.0, 500.0), (32, 20, 400.0, 450.0, 1.0, (90, 60, 231, 191)), (33, 16, 250.0, 350.0, -1.0))
RES_MAPS = ("general", "shear", "rx100")
K_RES = len(RES_FRAMES)
KEEP_R = 128          # the references at this R stay (two test files use them); those of any other R go when R changes


def res_pack():
    """(depth, off, hdr) of the three sources as one pack."""
    if "res_pack" not in _memo:
        fr = [frame(*a) for a in RES_FRAMES]
        depth = np.concatenate([d for d, _ in fr])
        off = np.cumsum([0] + [d.size for d, _ in fr]).astype(np.int64)
        _memo["res_pack"] = (depth, off, np.stack([h for _, h in fr]))
    return _memo["res_pack"]


def res_xforms():
    """float64[3,24]: source i under RES_MAPS[i]."""
    if "res_xf" not in _memo:
        depth, off, hdr = res_pack()
        _memo["res_xf"] = np.stack([_xform(depth[off[i]:off[i + 1]], hdr[i], RES_MAPS[i], None, RES_FRAMES[i][0])
                                    for i in range(K_RES)])
    return _memo["res_xf"]


def res_sources(kind, R):
    """The three sources at R for ``kind`` in ("plain", "mapped"): dict(grid float32[3,8], vol float32[3,3,R,R,R],
    nearest int32[3,R,R,R], fragile bool[3,R,R,R], near int[3]), indexed [z][y][x] (layout czyx), by the brute-force
    references; the rows are those of ``plain_case`` / ``mapped_case``."""
    key = ("res", kind, R)
    if key not in _memo:
        for old in [k for k in _memo if isinstance(k, tuple) and k[0] == "res" and k[2] not in (R, KEEP_R)]:
            del _memo[old]
        depth, off, hdr = res_pack()
        xf = res_xforms()
        rows, refs = [], []
        for i in range(K_RES):
            d, h = depth[off[i]:off[i + 1]], hdr[i]
            if kind == "plain":
                row = ar.glue_row(d, h, R)[0]
                r = ar.accurate_frame(d, h, row[:3], row[3], row[4], R)
            else:
                row = mr.placement_row(d, h, xf[i], R)[0]
                r = mr.frame(d, h, row, R, xf[i])
            rows.append(row)
            refs.append((r["vol"], r["nearest"], r["fragile"], int(r["near"].sum())))
        _memo[key] = dict(grid=np.stack(rows), vol=np.stack([r[0] for r in refs]), nearest=np.stack([r[1] for r in refs]),
                          fragile=np.stack([r[2] for r in refs]), near=[r[3] for r in refs])
    return _memo[key]


def res_in_layout(src, layout):
    """(vol, nearest, fragile) of ``res_sources``' dict in the index order of ``layout``."""
    if ar.LAYOUTS[layout] == 0:
        return src["vol"], src["nearest"], src["fragile"]
    return (np.ascontiguousarray(src["vol"].transpose(0, 1, 4, 3, 2)), np.ascontiguousarray(src["nearest"].transpose(0, 3, 2, 1)),
            np.ascontiguousarray(src["fragile"].transpose(0, 3, 2, 1)))
