"""numpy restatement of include/tsdf_locate.h, the reference of tests/test_locate_cpu.py and tests/test_locate_gpu.py:
float64 in the contract's operation order (np.sum's own order for the sums: the contract leaves the tree to the kernel),
independent of the kernel.  Besides the outputs it returns a frame's smallest DECISION MARGIN: the distance of u0, u1,
v0, v1 from the nearest integer at every pass and of |d - cd| from h over the frame's valid pixels at every pass.  A float64
sum in another order moves c by parts in 1e-11, so kernel and reference pick identical rectangles and sets whenever the
margin is well above that: the GPU tier compares exactly only frames whose margin is >= MARGIN (asserted in the CPU tier
on the very inputs the GPU tier uses).  Also here: the seeded blob scenes both tiers use."""
import numpy as np

U = 2.0 ** -53                       # unit roundoff of float64
MARGIN = 1e-6
DEFAULT_CAM = (241.42, 160.0, 120.0, 1.0, 3.0)   # focal, cx, cy, invalid_eps, trunc_voxels: the MSRA constants
PARAMS = dict(cube=250.0, near=100.0, far=1500.0, seed_band=150.0, refine=2)
f32, f64 = np.float32, np.float64


def capacity_side(cube, near, focal):
    """s of the capacity rule: floor(cube * focal / near) + 2, float64 on the float32 parameters."""
    return int(min(np.floor((f64(f32(cube)) * f64(focal)) / f64(f32(near))) + 2.0, 2 ** 31 - 1))


def capacity(H, W, cube, near, focal):
    s = capacity_side(cube, near, focal)
    return min(W, s) * min(H, s)


def valid_mask(d, cam=DEFAULT_CAM, near=100.0, far=1500.0):
    """Step 1: finite, |d| >= eps, near <= d <= far, float32 compares; a NaN is invalid."""
    d = np.asarray(d, f32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (np.abs(d) >= f32(cam[3])) & (d >= f32(near)) & (d <= f32(far))


def centre(d64, S, cam):
    """Step 4 -> (c, N, the sums of the absolute values of the terms of sd, sx, sy: what a rounding bound needs)."""
    F, cx, cy = (f64(v) for v in cam[:3])
    H, W = d64.shape
    tx = d64 * (np.arange(W, dtype=f64) - cx)[None, :]     # each product rounded on its own
    ty = d64 * (np.arange(H, dtype=f64) - cy)[:, None]
    N = f64(int(S.sum()))
    sd, sx, sy = d64[S].sum(), tx[S].sum(), ty[S].sum()
    c = np.array([(sx / F) / N, -((sy / F) / N), -(sd / N)], f64)
    return c, int(N), np.array([np.abs(tx[S]).sum(), np.abs(ty[S]).sum(), np.abs(d64[S]).sum()], f64)


def _clamp_floor(v, lo, hi):
    f = np.floor(v)
    if not f >= lo:
        return int(lo)
    return int(hi) if f > hi else int(f)


def rect_of(c, H, W, cam=DEFAULT_CAM, cube=250.0, near=100.0):
    """Step 5 -> ((left, top, right, bottom), the distance of u0, u1, v0, v1 from the nearest integer)."""
    F, cx, cy = (f64(v) for v in cam[:3])
    h = f64(f32(cube)) / 2.0
    c_x, c_y, cd = c[0], c[1], -c[2]
    u0 = ((c_x - h) * F) / cd + cx
    u1 = ((c_x + h) * F) / cd + cx
    v0 = ((-(c_y + h)) * F) / cd + cy
    v1 = ((-(c_y - h)) * F) / cd + cy
    left = _clamp_floor(u0, 0, W - 1)
    right = _clamp_floor(np.floor(u1) + 1.0, left + 1, W)
    top = _clamp_floor(v0, 0, H - 1)
    bottom = _clamp_floor(np.floor(v1) + 1.0, top + 1, H)
    s = capacity_side(cube, near, F)
    right = min(right, left + min(W, s))
    bottom = min(bottom, top + min(H, s))
    uv = np.array([u0, u1, v0, v1], f64)
    return (left, top, right, bottom), float(np.abs(uv - np.round(uv)).min())


def cube_mask(d, valid, c, rect, cube=250.0):
    """The valid pixels inside the rectangle with |d - cd| <= h -> (mask over the whole frame, margin over the valid pixels)."""
    h = f64(f32(cube)) / 2.0
    dist = np.abs(np.asarray(d, f32).astype(f64) - (-c[2]))
    left, top, right, bottom = rect
    inside = np.zeros(valid.shape, bool)
    inside[top:bottom, left:right] = True
    with np.errstate(invalid="ignore"):
        keep = valid & inside & (dist <= h)
    margin = float(np.abs(dist[valid] - h).min()) if valid.any() else np.inf
    return keep, margin


def glue_cube(c, cube=250.0, R=32, trunc_voxels=3.0):
    """Step 8: the reference's float32 glue with max_l := cube, mid_p := float32(c) -> (grid row f32[8], max_l, mid_p)."""
    mid = np.asarray(c, f64).astype(f32)
    max_l = f32(cube)
    vl = f32(max_l / f32(R))
    td = f32(vl * f32(trunc_voxels))
    ori = ((mid - f32(max_l / f32(2))).astype(f32) + f32(vl / f32(2))).astype(f32)
    return np.concatenate([ori, [vl, td, 0, 0, 0]]).astype(f32), max_l, mid


def crop_of(d, keep, rect):
    left, top, right, bottom = rect
    return np.where(keep, np.asarray(d, f32), f32(0))[top:bottom, left:right].ravel()


def locate_frame(d, cam=DEFAULT_CAM, cube=250.0, near=100.0, far=1500.0, seed_band=150.0, refine=2, R=32):
    """One frame through the whole contract -> dict(status, com, rect, keep, count, crop, grid, max_l, mid_p, margin,
    centres: the (c, N, abs-sums) of every pass that moved c)."""
    d = np.asarray(d, f32)
    H, W = d.shape
    valid = valid_mask(d, cam, near, far)
    if not valid.any():
        return dict(status=1, com=np.zeros(3), rect=(0, 0, 1, 1), keep=np.zeros((H, W), bool), count=0,
                    crop=np.zeros(1, f32), grid=np.zeros(8, f32), max_l=f32(0), mid_p=np.zeros(3, f32), margin=np.inf,
                    centres=[])
    d64 = d.astype(f64)
    d_min = d[valid].min()
    with np.errstate(invalid="ignore"):
        S = valid & (d64 <= f64(d_min) + f64(f32(seed_band))) if f32(seed_band) != 0 else valid
    c, N, ab = centre(d64, S, cam)
    centres = [(c, N, ab)]
    rect, margin = rect_of(c, H, W, cam, cube, near)
    for _ in range(refine):
        S, m = cube_mask(d, valid, c, rect, cube)
        margin = min(margin, m)
        if not S.any():
            break
        c, N, ab = centre(d64, S, cam)
        centres.append((c, N, ab))
        rect, m = rect_of(c, H, W, cam, cube, near)
        margin = min(margin, m)
    keep, m = cube_mask(d, valid, c, rect, cube)
    margin = min(margin, m)
    grid, max_l, mid_p = glue_cube(c, cube, R, cam[4])
    return dict(status=0, com=c, rect=rect, keep=keep, count=int(keep.sum()), crop=crop_of(d, keep, rect), grid=grid,
                max_l=max_l, mid_p=mid_p, margin=margin, centres=centres)


def downstream(d, com, cam=DEFAULT_CAM, cube=250.0, near=100.0, far=1500.0, R=32):
    """Everything after the centre, from a GIVEN centre (the kernel's own): rectangle, mask, crop, count, cube row."""
    d = np.asarray(d, f32)
    H, W = d.shape
    rect, _ = rect_of(com, H, W, cam, cube, near)
    keep, _ = cube_mask(d, valid_mask(d, cam, near, far), com, rect, cube)
    grid, max_l, mid_p = glue_cube(com, cube, R, cam[4])
    return dict(rect=rect, keep=keep, count=int(keep.sum()), crop=crop_of(d, keep, rect), grid=grid, max_l=max_l, mid_p=mid_p)


def pack(frames_out, H, W):
    """Per-frame results (dicts with rect / crop) -> (depth, offsets, headers) as the kernel packs them."""
    hdr = np.array([[W, H, *f["rect"]] for f in frames_out], np.int32).reshape(-1, 6)
    sizes = (hdr[:, 4] - hdr[:, 2]).astype(np.int64) * (hdr[:, 5] - hdr[:, 3])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    depth = np.concatenate([f["crop"] for f in frames_out]).astype(f32) if frames_out else np.zeros(0, f32)
    return depth, off, hdr


def com_bound(centres, cam=DEFAULT_CAM):
    """An a-priori bound on |c_kernel - c_reference| per coordinate for a frame whose every pass summed the SAME set in
    both (the margin condition).  A float64 sum of K terms in ANY order is off by at most (K - 1) u sum|t| to first
    order (Higham, gamma_{K-1}); the terms themselves (one rounded product each) are the same numbers on both sides, so
    two sums of the same terms differ by at most 2 (K - 1) u sum|t| (1 + K u).  The two quotients that follow add 2 u |c|
    on each side.  A later pass takes its set from the earlier centre but, the set being the same, not its value — so
    the bound of the LAST pass is the bound of the result."""
    c, N, ab = centres[-1]
    F = f64(cam[0])
    sums = 2.0 * max(N - 1, 0) * U * (1.0 + N * U) * ab / np.array([F * N, F * N, N], f64)
    return sums * (1.0 + 8 * U) + 4.0 * U * np.abs(c)


# ---- the seeded blob scenes -------------------------------------------------------------------------------------------
def scene(H, W, cam, seed, corner=False, quant=8, behind=400.0):
    """A hand — the near face of a sphere 35..70 mm in radius at 300..600 mm — in front of a noisy body plane ``behind`` mm
    behind it, a fifth of the frame empty; depth exact in 1/quant mm.  -> dict(frame f32[H,W], hand: its pixel mask,
    box: the hand's tight (left, top, right, bottom))."""
    F, cx, cy = cam[:3]
    rng = np.random.default_rng(seed)
    z0 = rng.uniform(300.0, 600.0)
    rad = rng.uniform(35.0, 70.0)
    rp = rad * F / z0                                     # the hand's radius in pixels
    if corner:                                            # the centre near a corner: the cube's rectangle is clipped
        px = rng.uniform(0.6 * rp, 1.2 * rp) if rng.random() < 0.5 else W - 1 - rng.uniform(0.6 * rp, 1.2 * rp)
        py = rng.uniform(0.6 * rp, 1.2 * rp) if rng.random() < 0.5 else H - 1 - rng.uniform(0.6 * rp, 1.2 * rp)
    else:
        px = rng.uniform(min(rp + 1, W / 2), max(W - 2 - rp, W / 2))
        py = rng.uniform(min(rp + 1, H / 2), max(H - 2 - rp, H / 2))
    yy, xx = np.mgrid[0:H, 0:W].astype(f64)
    r2 = ((xx - px) ** 2 + (yy - py) ** 2) * (z0 / F) ** 2
    hand = r2 < rad ** 2
    frame = z0 + behind + rng.normal(0.0, 5.0, (H, W))
    empty_from = int(rng.uniform(0.0, 0.8) * W)           # a fifth of the columns holds nothing
    frame[:, empty_from:empty_from + W // 5] = 0.0
    frame[hand] = (z0 - np.sqrt(np.maximum(rad ** 2 - r2, 0.0)) + rng.normal(0.0, 0.5, (H, W)))[hand]
    frame = (np.round(frame * quant) / quant).astype(f32)
    ys, xs = np.nonzero(hand)
    return dict(frame=frame, hand=hand, box=(int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1), z0=z0)


def tight_crop(sc):
    """The scene's hand as an MSRA-style crop: (depth f32[bw*bh], header int32[6]) — the pixels of the tight box, everything
    that is not hand zeroed."""
    H, W = sc["frame"].shape
    left, top, right, bottom = sc["box"]
    d = np.where(sc["hand"], sc["frame"], f32(0))[top:bottom, left:right]
    return d.ravel().astype(f32), np.array([W, H, left, top, right, bottom], np.int32)


# the cameras and frame counts of the GPU tier's input sets: name -> (H, W, camera, seeds)
CAM_SMALL = (30.0, 20.3, 15.1, 1.0, 3.0)
CAM_MID = (48.0, 31.5, 23.5, 1.0, 3.0)
CAM_VGA = (588.04, 320.0, 240.0, 1.0, 3.0)
SETS = {
    "41x30": (30, 41, CAM_SMALL, range(1000, 1300)),     # n = 1, 3, 17 and 300 are cut from these
    "64x48": (48, 64, CAM_MID, range(2000, 2017)),
    "320x240": (240, 320, DEFAULT_CAM, range(3000, 3002)),
    "640x480": (480, 640, CAM_VGA, range(4000, 4001)),
}
_cache = {}


def scenes(name):
    """The scenes of one input set (every fourth a corner scene), built once."""
    if name not in _cache:
        H, W, cam, seeds = SETS[name]
        _cache[name] = [scene(H, W, cam, s, corner=(k % 4 == 3)) for k, s in enumerate(seeds)]
    return _cache[name]


def frames_of(name):
    return np.stack([sc["frame"] for sc in scenes(name)])


_ref_cache = {}


def reference(name, **kw):
    """locate_frame over one input set with PARAMS (overridden by kw), computed once per (set, kw)."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _ref_cache:
        p = dict(PARAMS, **kw)
        cam = SETS[name][2]
        _ref_cache[key] = [locate_frame(sc["frame"], cam, **p) for sc in scenes(name)]
    return _ref_cache[key]


# ---- the edge frames and the other inputs of the GPU tier -------------------------------------------------------------
CAM_OTHER = (55.5, 30.25, 25.75, 350.0, 2.0)   # another focal, centre, eps (it invalidates what is nearer than 350 mm) and trunc


def scene_with_patch(seed=5003):
    """A 64x48 scene with a 4x4 patch of background 60 mm behind the centre of the hand's sphere — inside the seed band
    of 150 mm behind the hand's nearest point, outside a cube of 150 mm about the hand — on the side of the image the hand
    is not on."""
    sc = scene(48, 64, CAM_MID, seed)
    frame = sc["frame"].copy()
    x0 = 2 if sc["box"][0] > 32 else 58
    frame[2:6, x0:x0 + 4] = f32(np.round(sc["z0"] + 60.0))
    return dict(sc, frame=frame)


def edge_cases():
    """name -> (frame f32[48,64], parameters): the GPU tier's edge frames, all under CAM_MID; the reference decides what
    each one gives.  Built once."""
    if "edge" in _cache:
        return _cache["edge"]
    H, W = 48, 64
    base = scene(H, W, CAM_MID, 5001)["frame"]
    one = np.zeros((H, W), f32)
    one[17, 41] = 432.125
    specials = base.copy()
    specials[::7, ::5] = np.inf
    specials[3::7, 2::5] = -np.inf
    specials[5::7, 1::5] = np.nan
    cases = {
        "all zero": (np.zeros((H, W), f32), {}),
        "all NaN": (np.full((H, W), np.nan, f32), {}),
        "one valid pixel": (one, {}),
        "nearer than near": (np.full((H, W), 60.5, f32), {}),
        "beyond far": (np.full((H, W), 1800.25, f32), {}),
        "inf and NaN among the pixels": (specials, {}),
        "far = inf": (specials, dict(far=np.inf)),
        "hand in the corner": (scene(H, W, CAM_MID, 5002, corner=True)["frame"], {}),
        "the cube's rectangle is the whole image": (base, dict(cube=4000.0, far=3000.0)),
        "background inside the seed band": (scene_with_patch()["frame"], dict(cube=150.0)),
        "refine 0": (base, dict(refine=0)),
        "refine 8": (scene(H, W, CAM_MID, 5003, behind=100.0)["frame"], dict(cube=150.0, refine=8)),
        "seed_band 0": (base, dict(seed_band=0.0)),
        "seed_band 0, refine 0": (base, dict(seed_band=0.0, refine=0)),
    }
    _cache["edge"] = cases
    return cases


def edge_reference():
    if "edge" not in _ref_cache:
        _ref_cache["edge"] = {k: locate_frame(f, CAM_MID, **dict(PARAMS, **kw)) for k, (f, kw) in edge_cases().items()}
    return _ref_cache["edge"]


def frames_q1():
    """The 64x48 scenes once more with depth in whole millimetres: what a uint16 frame with shift 0 holds."""
    if "q1" not in _cache:
        H, W, cam, seeds = SETS["64x48"]
        _cache["q1"] = np.stack([scene(H, W, cam, s, corner=(k % 4 == 3), quant=1)["frame"] for k, s in enumerate(seeds)])
    return _cache["q1"]


def other_camera_reference():
    """The 64x48 frames under CAM_OTHER."""
    if "other" not in _ref_cache:
        _ref_cache["other"] = [locate_frame(sc["frame"], CAM_OTHER, **PARAMS) for sc in scenes("64x48")]
    return _ref_cache["other"]
