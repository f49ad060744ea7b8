"""The position tables of the grid-stride tests: which kind of frame sits at which batch position when a launch has more
positions than the per-position kernels have workgroups, and the inputs built from them.  Test infrastructure only: a plain
module, no fixtures.  tests/test_stride_cpu.py shows that the tables and the packs are what they claim,
tests/test_stride_gpu.py runs them through tsdf_obb_kernel, tsdf_map_place_kernel, tsdf_map_step_head_kernel and the three
kernels of tsdf_locate.hip.

Those kernels give one workgroup to a batch position and cap the grid at GRID workgroups; workgroup b then takes the
positions b, b + GRID, b + 2 GRID, ... and reuses its LDS partials from one to the next.  What a position leaves behind
depends on its KIND — an OK crop goes through every barrier, a bad header or a bad index through none, a degenerate one
through some —, so a table puts every kind behind every kind (and, with three turns, between OK and between not-OK
neighbours).

Everything is built from a small set of K <= 64 distinct source frames, so that a launch of the K frames alone — one
position per workgroup, the path the other test files hold to their references — says what every position of the big
launch must hold, bit for bit."""
import functools
from typing import NamedTuple

import numpy as np
import torch

import locate_ref as lr

GRID = 65536                       # kObbMaxBlocks, kPlaceMaxBlocks, kHeadMaxBlocks, kLocMaxBlocks (1 << 16 each)
N2 = GRID + 4096                   # the first 4096 workgroups take two positions
N3 = 2 * GRID + 257                # the first 257 take three, the others two
SCAN_NS = (1023, 1024, 1025, 2047, 2049, 3 * 1024 + 1)   # the scan kernel's chunks: 1, 1, 2, 2, 3, 4

KINDS = ("ok_small", "ok_rows", "ok_wide", "degenerate", "bad_header", "bad_index")
OK_KINDS = KINDS[:3]
OBB_KINDS = KINDS[:5]              # obb_xforms takes no index
LOCATE_KINDS = KINDS[:4] + KINDS[5:]   # a raw frame has no header to be bad
MIN_PAIRS = 8
IMG_W, IMG_H = 320, 240


def is_ok(kind):
    return kind in OK_KINDS


def table(n, seed, kinds=KINDS):
    """The kind of every position of a launch of n > GRID positions, as indices into ``kinds``: int8[n].

    A workgroup's positions are its COLUMN c, c + GRID, c + 2 GRID.  Columns of two positions cycle (in a seeded order)
    through every ordered pair of kinds; columns of three cycle through every kind in the middle between two OK kinds and
    between two kinds that are not OK; columns of one are drawn at random."""
    assert GRID < n <= 3 * GRID
    rng = np.random.default_rng(seed)
    k = len(kinds)
    ok = [j for j, name in enumerate(kinds) if is_ok(name)]
    bad = [j for j, name in enumerate(kinds) if not is_ok(name)]
    t = rng.integers(0, k, n).astype(np.int8)
    three = max(n - 2 * GRID, 0)                       # columns [0, three) hold three positions
    two = np.arange(three, min(n - GRID, GRID))        # columns of exactly two
    pair = rng.permutation(len(two)) % (k * k)
    t[two], t[two + GRID] = pair // k, pair % k
    c = np.arange(three)
    mid = rng.permutation(three) % (2 * k)
    flank = np.where(mid[:, None] < k, rng.choice(ok, (three, 2)), rng.choice(bad, (three, 2)))
    t[c], t[c + GRID], t[c + 2 * GRID] = flank[:, 0], mid % k, flank[:, 1]
    return t


def pair_counts(t, k):
    """[k, k]: how often kind a at position i is followed by kind b at i + GRID."""
    a, b = t[:-GRID].astype(np.int64), t[GRID:].astype(np.int64)
    return np.bincount(a * k + b, minlength=k * k).reshape(k, k)


def middle_counts(t, kinds):
    """([k], [k]): how often each kind is the middle of a triple (i, i + GRID, i + 2 GRID) between two OK kinds, and
    between two kinds that are not OK."""
    k = len(kinds)
    ok = np.array([is_ok(name) for name in kinds])
    a, m, b = t[:-2 * GRID], t[GRID:-GRID], t[2 * GRID:]
    both_ok, both_bad = ok[a] & ok[b], ~ok[a] & ~ok[b]
    return np.bincount(m[both_ok], minlength=k), np.bincount(m[both_bad], minlength=k)


# ---- the source crops of obb_xforms, map_grids and map_step_head -------------------------------------------------------

class Crop(NamedTuple):
    kind: str              # for map_grids and map_step_head
    obb_kind: str          # for obb_xforms, where two valid pixels are degenerate as well
    img: np.ndarray        # float32[bh, bw]: the payload
    header: tuple          # W, H, left, top, right, bottom
    name: str


SMALL = ((2, 2), (3, 1), (1, 3), (2, 3), (3, 3), (4, 1), (5, 2), (3, 2))        # a few pixels, 1-3 columns
ROWS = ((17, 1), (18, 3), (33, 2), (40, 5), (64, 4), (100, 3), (236, 5), (19, 7))   # more than 16 rows: every wave has work
WIDE = ((2, 257), (2, 261), (3, 258), (4, 300), (2, 299), (3, 260), (4, 257), (2, 264))   # a lane's second group of a row


@functools.lru_cache(maxsize=None)
def crops():
    """The K source crops.  OK crops: depth seeded uniform in [400, 900] mm, about a sixth of the pixels 0 and one NaN in
    the larger ones, the first three pixels valid (so none is degenerate, for obb neither).  Made once, never modified."""
    rng = np.random.default_rng(20261021)
    out = []

    def add(kind, img, name, obb_kind=None, header=None):
        img = np.ascontiguousarray(img, np.float32)
        bh, bw = img.shape
        left, top = int(rng.integers(0, IMG_W - bw + 1)), int(rng.integers(0, IMG_H - bh + 1))
        hdr = [IMG_W, IMG_H, left, top, left + bw, top + bh]
        if header is not None:
            header(hdr)
        img.setflags(write=False)
        out.append(Crop(kind, obb_kind or kind, img, tuple(hdr), name))

    def blob(bh, bw):
        d = rng.uniform(400.0, 900.0, (bh, bw)).astype(np.float32)
        if bh * bw > 6:
            d[rng.random((bh, bw)) < 0.16] = 0.0
            d.reshape(-1)[int(rng.integers(3, bh * bw))] = np.nan
        d.reshape(-1)[:3] = rng.uniform(400.0, 900.0, 3).astype(np.float32)[:min(3, bh * bw)]
        return d

    for kind, shapes in (("ok_small", SMALL), ("ok_rows", ROWS), ("ok_wide", WIDE)):
        for bh, bw in shapes:
            add(kind, blob(bh, bw), "%s_%dx%d" % (kind, bh, bw))
    two = np.zeros((3, 3), np.float32)
    two[0, 1], two[2, 2] = 480.0, 510.0
    add("ok_small", two, "two_valid_pixels", obb_kind="degenerate")          # an extent for the placement, no plane for obb
    add("degenerate", np.zeros((3, 3)), "all_zero")
    add("degenerate", np.full((2, 5), np.nan), "all_nan")
    add("degenerate", np.full((18, 2), 0.5), "below_eps_18_rows")
    add("degenerate", np.zeros((2, 260)), "all_zero_wide")
    add("degenerate", [[0.0, 0.0], [650.0, 0.0]], "one_valid_pixel")          # N = 1: no extent either

    def wider(h):
        h[4] += 1

    def shorter(h):
        h[5] -= 1

    def empty(h):
        h[4] = h[2]

    add("bad_header", blob(3, 3), "right_plus_1", header=wider)
    add("bad_header", blob(20, 3), "bottom_minus_1", header=shorter)
    add("bad_header", blob(2, 5), "right_is_left", header=empty)
    add("bad_header", blob(2, 258), "wide_right_plus_1", header=wider)
    assert len(out) <= 64
    return tuple(out)


@functools.lru_cache(maxsize=None)
def crop_pack():
    """(depth, offsets, headers) of the K crops, payloads back to back: a bad header is one whose area is not its
    payload.  Read-only."""
    cs = crops()
    depth = np.concatenate([c.img.reshape(-1) for c in cs])
    off = np.concatenate([[0], np.cumsum([c.img.size for c in cs])]).astype(np.int64)
    hdr = np.array([c.header for c in cs], np.int32)
    for a in (depth, off, hdr):
        a.setflags(write=False)
    return depth, off, hdr


def sources_of(kinds, obb=False):
    """Per kind of ``kinds`` the indices of the crops of that kind (none for bad_index)."""
    cs = crops()
    return [np.array([j for j, c in enumerate(cs) if (c.obb_kind if obb else c.kind) == name], np.int64) for name in kinds]


def draw_sources(t, by_kind, n_src, seed):
    """The source frame of every position of table ``t``: drawn among the kind's sources; a bad_index position (a kind
    without sources) gets -1 and n_src in turn.  int64[n]."""
    rng = np.random.default_rng(seed)
    src = np.empty(len(t), np.int64)
    for j, pool in enumerate(by_kind):
        at = np.flatnonzero(t == j)
        src[at] = pool[rng.integers(0, len(pool), len(at))] if len(pool) else np.where(np.arange(len(at)) % 2, n_src, -1)
    return src


def small_row(index, n_src):
    """Where a position's row is found in the launch of the n_src sources followed by the two bad indices -1 and n_src
    (:func:`small_index`)."""
    return torch.where(index < 0, n_src, torch.where(index >= n_src, n_src + 1, index))


def small_index(n_src):
    return np.concatenate([np.arange(n_src), [-1, n_src]]).astype(np.int64)


def tile(depth, offsets, headers, src):
    """obb_xforms' pack: position i holds a copy of source frame src[i] — its payload and its header as they are, the
    offsets cumulative.  Torch tensors on any one device in, (depth, offsets, headers) on it out."""
    sizes = (offsets[1:] - offsets[:-1])[src]
    off = torch.zeros(len(src) + 1, dtype=torch.int64, device=src.device)
    off[1:] = torch.cumsum(sizes, 0)
    shift = offsets[:-1][src] - off[:-1]                       # a payload element's source, relative to its own place
    at = torch.arange(int(off[-1]), device=src.device) + torch.repeat_interleave(shift, sizes)
    return depth[at], off, headers[src].contiguous()


# ---- the source frames of locate_hands ---------------------------------------------------------------------------------

LOC_H, LOC_W = 18, 24
LOC_CAM = (18.0, 11.6, 8.7, 1.0, 3.0)      # focal, cx, cy, invalid_eps, trunc_voxels of a 24 x 18 image
LOC_SHIFT = 3                               # every depth below is a multiple of 1/8 mm: exact as uint16 with shift 3
LOC_SEEDS = range(7000, 7018)


@functools.lru_cache(maxsize=None)
def locate_frames():
    """(frames float32[K, 18, 24], kinds): the seeded scenes of tests/locate_ref.py at 24 x 18 — ok_rows a hand inside the
    image, ok_wide one in a corner (a clipped rectangle) —, ok_small two or three valid pixels in one to three columns,
    and the degenerate frames: all 0, all below ``near``, all beyond ``far``.  Read-only."""
    frames, kinds = [], []
    for k, s in enumerate(LOC_SEEDS):
        corner = k % 3 == 2
        frames.append(lr.scene(LOC_H, LOC_W, LOC_CAM, s, corner=corner)["frame"])
        kinds.append("ok_wide" if corner else "ok_rows")
    for k, pix in enumerate((((4, 7, 432.125), (5, 7, 440.5)), ((11, 20, 300.25), (12, 21, 310.0), (12, 22, 305.5)),
                             ((0, 0, 500.0), (1, 0, 501.0), (2, 0, 502.0)), ((17, 23, 700.125), (17, 22, 690.0)))):
        f = np.zeros((LOC_H, LOC_W), np.float32)
        for y, x, d in pix:
            f[y, x] = d
        frames.append(f)
        kinds.append("ok_small")
    for fill in (0.0, 60.5, 1800.25):
        frames.append(np.full((LOC_H, LOC_W), fill, np.float32))
        kinds.append("degenerate")
    frames = np.stack(frames)
    frames.setflags(write=False)
    return frames, tuple(kinds)


def locate_frames_u16():
    f = locate_frames()[0].astype(np.float64) * 2 ** LOC_SHIFT
    assert (f == np.round(f)).all() and f.min() >= 0 and f.max() < 65536
    return f.astype(np.uint16)


def locate_sources(kinds=LOCATE_KINDS):
    fk = locate_frames()[1]
    return [np.array([j for j, name in enumerate(fk) if name == kind], np.int64) for kind in kinds]
