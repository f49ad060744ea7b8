"""The numpy restatement of include/tsdf_patch.h: the contract of a patch (rules 1-7), of the labels and the way back,
and the plan — what tests/test_patch_gpu.py compares libtsdf_patch.so with bit for bit, and what tests/test_patch_cpu.py
checks by hand-computed patches and by deliberate mistakes.  Every float64 operation is one numpy operation, in the
header's order; nothing is fused.  The input families of both tiers are here too (``families``, ``label_families``).

``mistake=`` names one deliberate departure from the contract:
    "trunc"          the nearest tap by truncation instead of floor(u + 0.5)
    "half_even"      the nearest tap by round-half-to-even instead of floor(u + 0.5)
    "no_half_pixel"  a = 2j * rS - 1: the half pixel of (2j + 1) dropped
    "no_renorm"      bilinear without the renormalisation by w at a silhouette
    "no_depth_test"  the cube's depth test missing
    "inclusive"      x <= right and y <= bottom
    "swap_affine"    the two rows of the map swapped
    "flip_y"         labels: the sign of y in the projection flipped
    "no_det"         labels: det ignored (the adjugate alone)
"""
import numpy as np

CAM = (241.42, 160.0, 120.0, 1.0, 3.0)   # focal, cx, cy, invalid_eps, trunc_voxels: the MSRA constants
F32, F16, BF16 = 0, 1, 2
MISTAKES = ("trunc", "half_even", "no_half_pixel", "no_renorm", "no_depth_test", "inclusive", "swap_affine")
LABEL_MISTAKES = ("flip_y", "no_det", "swap_affine")
WG, MAX_GROUPS = 256, 4096


def plan(S, dtype):
    """(pixels per lane, rows per workgroup, items per position): tsdf_patch_plan."""
    px = 4 if dtype == F32 else 8
    lpr = S // px
    rows = min(S, WG // lpr)
    return px, rows, -(-S // rows)


def widen(u16, shift):
    """uint16 with a shift: float32(u) * 2^-shift, exact."""
    return u16.astype(np.float32) * np.float32(2.0 ** -shift)


class Source:
    """A flat float32 buffer and per source index its rectangle: ``rect(g)`` is (base, left, top, right, bottom) or None."""

    def __init__(self, flat, rects):
        self.flat, self.rects = np.ascontiguousarray(flat, np.float32).reshape(-1), rects

    def __len__(self):
        return len(self.rects)

    def rect(self, g):
        return self.rects[g]


def frames_source(frames):
    n, H, W = frames.shape
    return Source(frames, [(g * H * W, 0, 0, W, H) for g in range(n)])


def pack_source(depth, offsets, headers):
    rects = []
    for g, hd in enumerate(np.asarray(headers, np.int64)):
        left, top, right, bottom = (int(v) for v in hd[2:6])
        off0, off1 = int(offsets[g]), int(offsets[g + 1])
        bw, bh = right - left, bottom - top
        ok = bw > 0 and bh > 0 and bw * bh == off1 - off0 and off0 >= 0 and off1 <= depth.size     # header_ok of prim.inc
        rects.append((off0, left, top, right, bottom) if ok else None)
    return Source(depth, rects)


def cube_of(com, cube, cam):
    """Rule 2: (u0, v0, du, dv, h, rh, cd), float64, every operation on its own."""
    F, cx, cy = np.float64(cam[0]), np.float64(cam[1]), np.float64(cam[2])
    c_x, c_y, cd = np.float64(com[0]), np.float64(com[1]), -np.float64(com[2])
    h = np.float64(np.float32(cube)) / np.float64(2.0)
    with np.errstate(all="ignore"):
        rh = np.float64(1.0) / h
        u0 = ((c_x - h) * F) / cd + cx
        u1 = ((c_x + h) * F) / cd + cx
        v0 = ((-(c_y + h)) * F) / cd + cy
        v1 = ((-(c_y - h)) * F) / cd + cy
    return u0, v0, u1 - u0, v1 - v0, h, rh, cd


def status1(com, cube, row, status_in):
    """Rule 1's status 1."""
    if status_in != 0 or not np.isfinite(np.asarray(com, np.float64)).all() or not -np.float64(com[2]) > 0:
        return True
    c = np.float32(cube)
    if not (np.isfinite(c) and c > 0):
        return True
    return row is not None and not np.isfinite(row).all()


def _forward(a, b, row, mistake):
    if row is None:
        return a, b
    r = row[[3, 4, 5, 0, 1, 2]] if mistake == "swap_affine" else row
    with np.errstate(all="ignore"):
        return (r[0] * a + r[1] * b) + r[2], (r[3] * a + r[4] * b) + r[5]


def _tap(src, rect, x, y, cd, h, eps, mistake):
    """Rule 4 on arrays of taps: (valid, float64 depth)."""
    base, left, top, right, bottom = rect
    with np.errstate(invalid="ignore"):
        if mistake == "inclusive":
            inside = (x >= left) & (x <= right) & (y >= top) & (y <= bottom)
        else:
            inside = (x >= left) & (x < right) & (y >= top) & (y < bottom)
    inside &= np.isfinite(x) & np.isfinite(y)
    xi, yi = np.where(inside, x, left).astype(np.int64), np.where(inside, y, top).astype(np.int64)
    e = base + (yi - top) * (right - left) + (xi - left)
    inside &= (e >= 0) & (e < src.flat.size)          # the contract never leaves the buffer; "inclusive" can
    d = src.flat[np.clip(e, 0, src.flat.size - 1)]
    with np.errstate(invalid="ignore"):
        ok = inside & np.isfinite(d) & (np.abs(d) >= np.float32(eps))
        d64 = d.astype(np.float64)
        if mistake != "no_depth_test":
            ok &= np.abs(d64 - cd) <= h
    return ok, d64


def patch_of(src, g, com, cube, row, S, interp, background, cam, status_in=0, mistake=None):
    """One position: (float32[S, S], status)."""
    out = np.full((S, S), np.float32(background), np.float32)
    if status1(com, cube, row, status_in):
        return out, 1
    rect = src.rect(g) if 0 <= g < len(src) else None
    if rect is None:
        return out, 2
    u0, v0, du, dv, h, rh, cd = cube_of(com, cube, cam)
    rS = np.float64(1.0) / np.float64(S)
    k = np.arange(S, dtype=np.float64)
    t = (2.0 * k if mistake == "no_half_pixel" else 2.0 * k + 1.0) * rS - 1.0
    a, b = np.broadcast_to(t[None, :], (S, S)), np.broadcast_to(t[:, None], (S, S))
    ap, bp = _forward(a, b, row, mistake)
    with np.errstate(all="ignore"):
        u = u0 + ((ap + 1.0) * 0.5) * du
        v = v0 + ((bp + 1.0) * 0.5) * dv
        if interp == 0:
            if mistake == "trunc":
                x, y = np.trunc(u), np.trunc(v)
            elif mistake == "half_even":
                x, y = np.rint(u), np.rint(v)
            else:
                x, y = np.floor(u + 0.5), np.floor(v + 0.5)
            ok, d = _tap(src, rect, x, y, cd, h, cam[3], mistake)
            z = (d - cd) * rh
        else:
            x0, y0 = np.floor(u), np.floor(v)
            fx, fy = u - x0, v - y0
            gx, gy = 1.0 - fx, 1.0 - fy
            s, w, have = np.zeros((S, S)), np.zeros((S, S)), np.zeros((S, S), np.int64)
            for x, y, wk in ((x0, y0, gx * gy), (x0 + 1.0, y0, fx * gy), (x0, y0 + 1.0, gx * fy), (x0 + 1.0, y0 + 1.0, fx * fy)):
                tap_ok, d = _tap(src, rect, x, y, cd, h, cam[3], mistake)
                s = np.where(tap_ok, s + wk * d, s)
                w = np.where(tap_ok, w + wk, w)
                have += tap_ok
            ok = (have != 0) & (w != 0.0)
            dbar = s if mistake == "no_renorm" else np.where(have == 4, s, s / w)
            z = (dbar - cd) * rh
        out[ok] = z[ok].astype(np.float32)
    return out, 0


def patches(src, com, *, S, cube=250.0, interp=0, affine=None, background=1.0, cam=CAM, index=None, status=None, mistake=None,
            positions=None):
    """(float32[n, S, S], int32[n]); ``positions``: only these batch positions are computed (the others stay zero)."""
    n = len(com)
    out, st = np.zeros((n, S, S), np.float32), np.zeros(n, np.int32)
    for i in (range(n) if positions is None else positions):
        g = int(index[i]) if index is not None else i
        out[i], st[i] = patch_of(src, g, com[i], cube[i] if np.ndim(cube) else cube, None if affine is None else affine[i], S,
                                 interp, background, cam, 0 if status is None else int(status[i]), mistake)
    return out, st


def bits(x32, dtype):
    """The bit patterns the library writes: int32 for float32, int16 for the 2-byte types (round-to-nearest-even)."""
    x32 = np.ascontiguousarray(x32, np.float32)
    if dtype == F32:
        return x32.view(np.int32)
    if dtype == F16:
        with np.errstate(over="ignore"):
            return x32.astype(np.float16).view(np.int16)
    u = x32.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16).view(np.int16)     # no NaN among the values here


def uvd(joints, com, *, cube=250.0, affine=None, cam=CAM, status=None, mistake=None):
    """The labels: (float32[n, J, 3], int32[n, J], int32[n])."""
    joints = np.asarray(joints, np.float32)
    n, J = joints.shape[:2]
    out, valid, st = np.zeros((n, J, 3), np.float32), np.zeros((n, J), np.int32), np.zeros(n, np.int32)
    F, cx, cy = np.float64(cam[0]), np.float64(cam[1]), np.float64(cam[2])
    for i in range(n):
        row = None if affine is None else np.asarray(affine[i], np.float64)
        cube_i = cube[i] if np.ndim(cube) else cube
        if status1(com[i], cube_i, row, 0 if status is None else int(status[i])):
            st[i] = 1
            continue
        if row is not None and mistake == "swap_affine":
            row = row[[3, 4, 5, 0, 1, 2]]
        det = np.float64(1.0)
        if row is not None:
            with np.errstate(all="ignore"):
                det = row[0] * row[4] - row[1] * row[3]
            if mistake != "no_det" and (det == 0 or not np.isfinite(det)):
                st[i] = 1
                continue
        u0, v0, du, dv, h, rh, cd = cube_of(com[i], cube_i, cam)
        X, Y, Z = (joints[i, :, k].astype(np.float64) for k in range(3))
        dj = -Z
        with np.errstate(all="ignore"):
            ok = np.isfinite(joints[i]).all(axis=1) & (dj > 0)
            u = (X * F) / dj + cx
            v = ((Y if mistake == "flip_y" else -Y) * F) / dj + cy
            ap = ((u - u0) / du) * 2.0 - 1.0
            bp = ((v - v0) / dv) * 2.0 - 1.0
            a, b = ap, bp
            if row is not None:
                ta, tb = ap - row[2], bp - row[5]
                a, b = row[4] * ta - row[1] * tb, row[0] * tb - row[3] * ta
                if mistake != "no_det":
                    a, b = a / det, b / det
            w = (dj - cd) * rh
            res = np.stack([a, b, w], axis=1).astype(np.float32)
        out[i][ok] = res[ok]
        valid[i] = ok
    return out, valid, st


def joints_back(uvd_, com, *, cube=250.0, affine=None, cam=CAM, status=None):
    """The way back: float32[n, J, 3]."""
    uvd_ = np.asarray(uvd_, np.float32)
    n, J = uvd_.shape[:2]
    out = np.zeros((n, J, 3), np.float32)
    F, cx, cy = np.float64(cam[0]), np.float64(cam[1]), np.float64(cam[2])
    for i in range(n):
        row = None if affine is None else np.asarray(affine[i], np.float64)
        cube_i = cube[i] if np.ndim(cube) else cube
        if status1(com[i], cube_i, row, 0 if status is None else int(status[i])):
            continue
        u0, v0, du, dv, h, rh, cd = cube_of(com[i], cube_i, cam)
        a, b, w = (uvd_[i, :, k].astype(np.float64) for k in range(3))
        with np.errstate(all="ignore"):
            depth = w * h + cd
            ap, bp = _forward(a, b, row, None)
            u = u0 + ((ap + 1.0) * 0.5) * du
            v = v0 + ((bp + 1.0) * 0.5) * dv
            X = ((u - cx) * depth) / F
            Y = -(((v - cy) * depth) / F)
            out[i] = np.stack([X, Y, -depth], axis=1).astype(np.float32)
    return out


def affines(angle=None, scale=None, shift=None, n=None):
    """patch_affines' rows in numpy: a' = s (cos t a - sin t b) + tx, b' = s (sin t a + cos t b) + ty."""
    n = n if n is not None else len(next(v for v in (angle, scale, shift) if v is not None))
    t = np.zeros(n) if angle is None else np.asarray(angle, np.float64)
    s = np.ones(n) if scale is None else np.asarray(scale, np.float64)
    sh = np.zeros((n, 2)) if shift is None else np.asarray(shift, np.float64)
    c, si = s * np.cos(t), s * np.sin(t)
    return np.stack([c, -si, sh[:, 0], si, c, sh[:, 1]], axis=1)


# ---- the inputs of both tiers ----
def com_at(px, py, d, cam=CAM):
    """The camera-frame centre whose projection is pixel (px, py) at depth d."""
    return np.array([(px - cam[1]) * d / cam[0], -(py - cam[2]) * d / cam[0], -d], np.float64)


def synth_frame(H, W, seed, depth=450.0):
    """A hand-like blob (a palm and four fingers, depth sloping over it) before a far wall, with holes of every invalid
    kind: 0, below invalid_eps, negative, NaN, +-inf."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    cx, cy, r = W * 0.5, H * 0.55, min(H, W) * 0.18
    hand = ((x - cx) / r) ** 2 + ((y - cy) / (1.2 * r)) ** 2 <= 1.0
    for k in range(4):
        fx = cx + (k - 1.5) * r * 0.5
        hand |= (np.abs(x - fx) <= r * 0.15) & (y <= cy) & (y >= cy - 2.6 * r + abs(k - 1.5) * r * 0.3)
    f = np.where(x < W * 0.7, 1300.0, 0.0)                         # a wall on the left, nothing on the right
    f = np.where(hand, depth + 0.35 * (x - cx) - 0.2 * (y - cy) + 6.0 * rng.standard_normal((H, W)), f)
    f = f.astype(np.float32)
    holes = rng.integers(0, H * W, size=max(6, H * W // 40))
    kinds = np.array([0.0, 0.5, -300.0, np.nan, np.inf, -np.inf], np.float32)
    f.reshape(-1)[holes] = kinds[np.arange(holes.size) % kinds.size]
    return f


def pack_of(crops):
    """A pack of [(array2d, left, top, W, H)]: depth, offsets, headers."""
    depth = np.concatenate([np.asarray(c[0], np.float32).reshape(-1) for c in crops])
    offsets = np.concatenate([[0], np.cumsum([c[0].size for c in crops])]).astype(np.int64)
    headers = np.array([[c[3], c[4], c[1], c[2], c[1] + c[0].shape[1], c[2] + c[0].shape[0]] for c in crops], np.int32)
    return depth, offsets, headers


def small_pack(seed=3):
    """The sources 1 x 1, 1 x 7, 7 x 1, 3 x 3 and a 37 x 29 crop of a 320 x 240 frame as one pack, and the cube centres
    on them: (depth, offsets, headers, com float64[5, 3], cube float32[5])."""
    rng = np.random.default_rng(seed)
    frame = synth_frame(240, 320, seed)
    crops, com, cube = [], [], []
    for (bh, bw, left, top) in ((1, 1, 10, 12), (1, 7, 150, 100), (7, 1, 0, 0), (3, 3, 317, 237)):
        a = (450.0 + 20.0 * rng.standard_normal((bh, bw))).astype(np.float32)
        crops.append((a, left, top, 320, 240))
        com.append(com_at(left + (bw - 1) / 2.0, top + (bh - 1) / 2.0, 452.0))
        cube.append(np.float32((max(bw, bh) + 1.3) * 452.0 / CAM[0]))      # the rectangle a little larger than the crop
    left, top = 141, 110
    crops.append((frame[top:top + 29, left:left + 37], left, top, 320, 240))
    com.append(com_at(160.3, 126.8, 455.0))
    cube.append(np.float32(70.0))
    return (*pack_of(crops), np.array(com), np.array(cube, np.float32))


def affine_family():
    """name -> float64[6]: the maps of the affine family (the NaN and the singular one included)."""
    d = {
        "identity": [1, 0, 0, 0, 1, 0],
        "rot90": affines([np.pi / 2])[0], "rot180": affines([np.pi])[0], "rot45": affines([np.pi / 4])[0],
        "half": affines(scale=[0.5])[0], "double": affines(scale=[2.0])[0],
        "reflect": [-1, 0, 0, 0, 1, 0], "pixel": [1, 0, 2.0 / 64, 0, 1, -2.0 / 64], "shear": [1, 0.4, 0.05, -0.2, 1, 0],
        "nan": [1, 0, float("nan"), 0, 1, 0], "huge": [1e30, 0, 0, 0, 1e30, 0], "huge_shift": [1, 0, 1e30, 0, 1, -1e30],
        "singular": [1, 2, 0.1, 2, 4, -0.1],
    }
    return {k: np.asarray(v, np.float64) for k, v in d.items()}


def joints_family(seed=11, n=6, J=21, depth=450.0):
    """Camera-frame joints about the centres ``com`` (returned): inside and outside the cube, a NaN, an inf, Z >= 0."""
    rng = np.random.default_rng(seed)
    want, n = n, max(n, 6)
    com = np.stack([com_at(160 + 30 * rng.standard_normal(), 120 + 30 * rng.standard_normal(), depth + 40 * rng.standard_normal())
                    for _ in range(n)])
    j = (com[:, None, :] + 90.0 * rng.standard_normal((n, J, 3))).astype(np.float32)
    j[0, 1, 0] = np.nan
    j[1, 2, 2] = np.inf
    j[2, 3, 2] = 0.0
    j[3, 4, 2] = 25.0
    j[4, 5] = com[4].astype(np.float32)
    return j[:want], com[:want]


def noise_frame(H, W, seed, depth=450.0, sigma=8.0):
    """A small frame valid nearly everywhere: depth + noise, with one hole of every invalid kind where there is room."""
    rng = np.random.default_rng(seed)
    f = (depth + sigma * rng.standard_normal((H, W))).astype(np.float32)
    kinds = np.array([0.0, 0.5, -300.0, np.nan, np.inf, -np.inf], np.float32)
    if H * W >= 24:
        f.reshape(-1)[rng.choice(H * W, kinds.size, replace=False)] = kinds
    return f


EXACT_CAM = (256.0, 1.5, 1.5, 1.0, 3.0)   # cd = F = 256 and cube = 8: u0 = -2.5, du = 8, so at S = 8 pixel (i, j) is source (j - 2, i - 2)


def exact_source():
    """The 4 x 4 source of the hand-computed patches, cd = 256, h = 4: cd - h and cd + h (kept), one float32 step beyond
    each (dropped), every invalid kind, and a valid pixel right of an invalid one."""
    lo, hi = np.float32(252.0), np.float32(260.0)
    return np.array([[lo, np.nextafter(lo, np.float32(0)), 256.0, 258.0],
                     [hi, np.nextafter(hi, np.float32(1e9)), np.nan, np.inf],
                     [0.5, -256.0, 254.0, 255.0],
                     [257.0, 259.0, 253.0, 256.0]], np.float32)


def case(kind, source, com, **kw):
    """One input family: ``kind`` "frames" (``source`` float32[N, H, W]) or "crops" (``source`` (depth, offsets, headers))."""
    c = dict(kind=kind, source=source, com=np.asarray(com, np.float64).reshape(-1, 3), cube=250.0, affine=None, index=None,
             status=None, cam=CAM, background=1.0)
    c.update(kw)
    return c


def source_of(c):
    return frames_source(c["source"]) if c["kind"] == "frames" else pack_source(*c["source"])


def reference(c, S, interp, mistake=None, positions=None):
    """The restatement on a family: (float32[n, S, S], int32[n])."""
    return patches(source_of(c), c["com"], S=S, cube=c["cube"], interp=interp, affine=c["affine"], background=c["background"],
                   cam=c["cam"], index=c["index"], status=c["status"], mistake=mistake, positions=positions)


def families():
    """name -> case: the inputs of the GPU tier, on which the CPU tier shows that each mistake is seen."""
    out = {}
    depth, off, hdr, com, cube = small_pack()
    out["pack"] = case("crops", (depth, off, hdr), com, cube=cube)
    out["tiny"] = case("frames", noise_frame(12, 16, 5)[None], com_at(7.3, 5.6, 450.0), cube=np.float32(25.0))
    frame = synth_frame(240, 320, 7)
    out["frame"] = case("frames", frame[None], com_at(160.4, 131.7, 452.0))
    out["up"] = case("frames", frame[None], com_at(161.2, 132.4, 452.0), cube=np.float32(5.0 * 452.0 / CAM[0]))
    out["down"] = case("frames", frame[None], com_at(160.0, 120.0, 452.0), cube=np.float32(300.0 * 452.0 / CAM[0]))
    # the centre near each border and corner, so that the rectangle leaves the frame on every side, and wholly outside it
    at = [(2.0, 120.0), (318.0, 120.0), (160.0, 1.0), (160.0, 238.5), (0.0, 0.0), (319.0, 0.0), (0.0, 239.0), (319.0, 239.0),
          (-400.0, 120.0), (160.0, 900.0), (160.0, 131.0)]
    yy, xx = np.mgrid[0:240, 0:320]
    wall = (440.0 + (xx * 7 + yy * 13) % 17).astype(np.float32)       # valid everywhere but at the frame's non-finite holes
    wall[~np.isfinite(frame)] = frame[~np.isfinite(frame)]
    out["borders"] = case("frames", wall[None], [com_at(px, py, 450.0) for px, py in at], cube=120.0,
                          index=np.zeros(len(at), np.int64))
    aff = affine_family()
    out["affine"] = case("frames", frame[None], [com_at(160.4, 131.7, 452.0)] * len(aff), affine=np.stack(list(aff.values())),
                         index=np.zeros(len(aff), np.int64))
    out["exact"] = case("frames", exact_source()[None], [[0.0, 0.0, -256.0]], cube=8.0, cam=EXACT_CAM, background=7.0)
    out["exact_half"] = case("frames", exact_source()[None], [[0.0, 0.0, -256.0]], cube=8.0, cam=(256.0, 1.0, 1.0, 1.0, 3.0),
                             background=7.0)
    frames3 = np.stack([frame, synth_frame(240, 320, 8, depth=520.0), synth_frame(240, 320, 9, depth=380.0)])
    com3 = [com_at(160.4, 131.7, 452.0), com_at(158.0, 130.0, 520.0), com_at(163.0, 133.0, 380.0)]
    # a per-position cube, a status passed through, an index with duplicates, a negative and a too-large entry, bad centres
    idx = np.array([2, 0, 0, -1, 3, 1, 1, 2, 0], np.int64)
    comi = np.stack([com3[g] if 0 <= g < 3 else com3[0] for g in idx])
    comi[7] = [0.0, 0.0, 10.0]            # behind the camera
    comi[8, 1] = np.nan
    out["batch"] = case("frames", frames3, comi, cube=np.array([250, 200, 300, 250, 250, float("inf"), 150, 250, 250], np.float32),
                        index=idx, status=np.array([0, 0, 5, 0, 0, 0, 0, 0, 0], np.int32))
    out["cam"] = case("frames", frames3, com3, cam=(588.03, 170.5, 110.25, 2.0, 3.0), cube=180.0)
    # packs: a header the rule refuses (payload of another size), one whose payload lies beyond depth_len, a negative offset
    d2, o2, h2 = pack_of([(frame[100:130, 140:180], 140, 100, 320, 240), (frame[90:120, 150:170], 150, 90, 320, 240),
                          (frame[100:140, 130:190], 130, 100, 320, 240)])
    h2 = h2.copy()
    h2[1, 4] += 1                          # a wider crop than its payload
    out["badpack"] = case("crops", (d2[:-5].copy(), o2, h2), [com_at(160.0, 115.0, 452.0)] * 3, cube=120.0)
    return out


def label_families():
    """name -> (joints, com, keywords of uvd): the inputs of the label tier."""
    j, com = joints_family()
    aff = affine_family()
    names = ["rot45", "shear", "half", "reflect", "singular", "nan"]
    out = {"plain": (j, com, dict(cube=250.0)),
           "cubes": (j, com, dict(cube=np.array([250, 200, 0, 300, float("nan"), 180], np.float32), status=np.array([0, 3, 0, 0, 0, 0], np.int32))),
           "mapped": (j, com, dict(cube=220.0, affine=np.stack([aff[k] for k in names]))),
           "cam": (j, com, dict(cube=250.0, cam=(588.03, 170.5, 110.25, 2.0, 3.0), affine=np.stack([aff["rot90"]] * 6)))}
    return out
