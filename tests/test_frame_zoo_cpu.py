"""CPU tier of the frame zoo (tests/frame_zoo.py): the zoo is what it claims — every height x width class is present, the
``pool`` pairs lie on the two sides of the pool's size, valid pixels reach the rows and columns they should, the numbers of
frames per status are the stated ones, the split plans give the band counts the GPU tier relies on, the maps of the
augmented runs leave the zoo a zoo, and the oracle's plain and identity-map placements agree bit for bit."""
import numpy as np
import pytest

import frame_zoo as fz
import oracle
import plan_ref

CUS = 256                                  # an MI355X
SPLIT_N = (16, min(CUS // 2, 128))         # the split-sized batches of tests/test_frame_zoo_gpu.py

N_OK, N_DEGENERATE = 226, 4                # status 0 / status 1 frames of the zoo (nothing else occurs)
DEGENERATE = ("rowdeal_1x1_0", "rowdeal_2x1_13", "rowdeal_48x129_194", "rowdeal_24x257_195")


@pytest.fixture(scope="module")
def zoo():
    return fz.zoo()


@pytest.fixture(scope="module")
def plain(zoo):
    ref = oracle.voxelize(*fz.master(len(zoo)), R=32, n_threads=8, extras=True)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _shapes(zoo, cls):
    return {e.img.shape for e in zoo if cls in e.classes}


def _valid(img):
    with np.errstate(invalid="ignore"):
        return np.abs(img) >= fz.INVALID_EPS


def test_every_height_and_width_class_is_present(zoo):
    assert len(zoo) == 230 and len({e.name for e in zoo}) == len(zoo)
    assert _shapes(zoo, "short") == {(h, w) for h in fz.SHORT_H for w in fz.SHORT_W}
    assert _shapes(zoo, "tall") == {(h, w) for h in fz.TALL_H for w in fz.TALL_W}
    assert {s[1] for s in _shapes(zoo, "wide")} == set(fz.WIDE_W)
    assert _shapes(zoo, "rowdeal") >= {(h, w) for h in fz.HEIGHTS for w in fz.WIDTHS}
    # the thresholds of csrc/common.inc (kMaxRows = 256, kMaxCapW = 320) have a frame on either side and one on them
    assert {255, 256, 257} <= {e.img.shape[0] for e in zoo} and {319, 320, 321} <= {e.img.shape[1] for e in zoo}
    for e in zoo:
        assert e.img.dtype == np.float32 and not e.img.flags.writeable
        assert e.img.shape[0] <= fz.IMG_H and e.img.shape[1] <= fz.IMG_W     # "inside a 640 x 480 image"


def test_valid_pixels_reach_the_edges_they_should(zoo):
    for e in zoo:
        v = _valid(e.img)
        if "tall" in e.classes:
            assert v[0].any() and v[-1].any(), e.name
        if "wide" in e.classes:
            assert v[:, 0].any() and v[:, -1].any(), e.name
    # the frames that came with the row deal's test stay: one edge row / column only, all invalid, sub-threshold with
    # NaNs, NaN-laden
    only = [e for e in zoo if "rowdeal" in e.classes][169:194]
    assert len(only) == 25
    kinds = set()
    for e in only:
        v = _valid(e.img)
        rows, cols = np.nonzero(v.any(axis=1))[0], np.nonzero(v.any(axis=0))[0]
        assert len(rows) == 1 or len(cols) == 1, e.name
        kinds.add(("row", int(rows[0]) == 0, int(rows[0]) == e.img.shape[0] - 1) if len(rows) == 1 else
                  ("col", int(cols[0]) == 0, int(cols[0]) == e.img.shape[1] - 1))
    assert kinds == {("row", True, False), ("row", False, True), ("row", False, False),
                     ("col", True, False), ("col", False, True)}
    by_name = {e.name: e for e in zoo}
    assert not _valid(by_name["rowdeal_48x129_194"].img).any() and not by_name["rowdeal_48x129_194"].img.any()
    sub = by_name["rowdeal_24x257_195"].img
    assert not _valid(sub).any() and np.isnan(sub).any() and (sub == 0.5).any()
    nan = by_name["rowdeal_240x320_196"].img
    assert np.isnan(nan[100]).all() and np.isnan(nan).mean() > 0.04 and _valid(nan).sum() > 1000


def test_pool_frames_straddle_the_pool(zoo):
    pool = {e.name: e.img for e in zoo if "pool" in e.classes}
    assert len(pool) == 8
    for (sw4, sh), over in zip(fz.POOL_RECTS, (False, True, False, True)):
        img = pool["pool_rect_%dx%d" % (sw4, sh)]
        c0, r0, sw, h = fz.valid_rect(img)
        assert ((sw + 3) & ~3, h) == (sw4, sh) and fz.rect_floats(img) == sw4 * sh
        assert (sw4 * sh > fz.POOL_FLOATS) == over
        v = _valid(img)
        assert v[r0, c0] and v[r0, c0 + sw - 1] and v[r0 + h - 1, c0] and v[r0 + h - 1, c0 + sw - 1]     # the corners
        assert 0 < c0 and c0 + sw < img.shape[1] and 0 < r0 and r0 + h < img.shape[0]                    # strictly inside
    assert 248 * 141 == fz.POOL_FLOATS and 248 * 142 == 35216 and 320 * 109 == 34880 and 320 * 110 == 35200
    dense = pool["pool_dense_320x240"]
    assert _valid(dense).all() and fz.rect_floats(dense) == 76800          # beyond every pool, every capture region
    assert _valid(pool["pool_small_80x80"]).any() and fz.box_floats(pool["pool_small_80x80"]) == 6400
    a, b = pool["pool_box_fits_rect_small"], pool["pool_box_over_rect_fits"]
    assert fz.box_floats(a) <= fz.POOL_FLOATS and 10 * fz.rect_floats(a) < fz.box_floats(a)
    assert fz.box_floats(b) > fz.POOL_FLOATS >= fz.rect_floats(b)          # the diagnostic build gathers from memory


def test_a_tenth_hang_off_or_start_at_odd_offsets(zoo):
    off_image = [e for e in zoo if "off_image" in e.classes]
    assert 10 * len(off_image) >= len(zoo) == 230
    cx, cy = 160.0, 120.0                  # the principal point (include/tsdf.h)
    sides = set()
    outside = 0
    for e in off_image:
        left, top = e.place
        right, bottom = left + e.img.shape[1], top + e.img.shape[0]
        sides |= {s for s, c in (("l", right <= cx), ("r", left > cx), ("a", bottom <= cy), ("b", top > cy)) if c}
        outside += left < 0 or top < 0 or right > fz.IMG_W or bottom > fz.IMG_H
    assert sides == {"l", "r", "a", "b"} and outside >= 3
    for e in zoo:
        if "off_image" not in e.classes:
            left, top = e.place
            assert 0 <= left and left + e.img.shape[1] <= fz.IMG_W and 0 <= top and top + e.img.shape[0] <= fz.IMG_H
    off = fz.master(len(zoo))[1]
    assert (off[:-1] % 4 != 0).sum() >= len(zoo) // 10


def test_status_counts_are_exact(zoo, plain):
    st = plain["status"]
    assert (int((st == 0).sum()), int((st == 1).sum()), int((st > 1).sum())) == (N_OK, N_DEGENERATE, 0)
    assert tuple(zoo[i].name for i in np.nonzero(st == 1)[0]) == DEGENERATE
    # the padding of a batch is real work: every fresh draw is a status 0 frame
    more = oracle.voxelize(*fz.master(2 * CUS + 5), R=32, n_threads=8, want_tsdf=False)
    assert (more["status"][len(zoo):] == 0).all()
    np.testing.assert_array_equal(more["status"][:len(zoo)], st)
    for k in ("max_l", "mid_p"):
        np.testing.assert_array_equal(more[k][:len(zoo)].view(np.uint32), plain[k].view(np.uint32))


def test_oracle_rectangle_is_the_valid_rectangle(zoo, plain):
    """The oracle's extras against the zoo's own account of where the valid pixels are: the float32 extents of the cloud
    over the pixels of valid_rect() alone equal the AABB the oracle reports, so no valid pixel lies outside it."""
    for i, e in enumerate(zoo):
        r = fz.valid_rect(e.img)
        if r is None:
            assert plain["status"][i] == 1
            continue
        c0, r0, sw, sh = r
        sub = np.ascontiguousarray(e.img[r0:r0 + sh, c0:c0 + sw])
        left, top = e.place[0] + c0, e.place[1] + r0
        nv, mn, mx = oracle.aabb(sub, np.array([fz.IMG_W, fz.IMG_H, left, top, left + sw, top + sh], np.int32))
        assert nv == int(_valid(e.img).sum())
        np.testing.assert_array_equal(np.concatenate([mn, mx]).view(np.uint32), plain["aabb"][i].view(np.uint32), e.name)


def test_split_plans_have_more_bands_than_short_frames_have_rows():
    """At 16 frames the split kernel runs S = 8 workgroups a frame at R = 32 and S = 16 at R = 64; the short frames of 1,
    2, 3 and 7 rows (at S = 16: of 9 rows too) then leave row bands without a row.  At CUs/2 frames the plan is S = 2:
    there only the one-row frames leave a band empty."""
    assert SPLIT_N == (16, 128)
    assert plan_ref.split_plan(16, 32, CUS)[0] == 8 and plan_ref.split_plan(16, 64, CUS)[0] == 16
    assert plan_ref.split_plan(16, 48, CUS)[0] >= 8
    assert [h for h in fz.SHORT_H if h < 8] == [1, 2, 3, 7] and all(h < 16 for h in fz.SHORT_H)
    for R in (32, 48, 64):
        assert plan_ref.split_plan(128, R, CUS)[0] == 2
        assert plan_ref.split_plan(129, R, CUS)[0] == 0
    for R, lay, aug in ((32, 0, False), (32, 1, True), (64, 0, True), (48, 0, False)):
        assert plan_ref.describe(16, R, lay, aug, CUS).startswith("tsdf_split_kernel<%d, %d, " % (R if R != 48 else 0, lay))
    # a geometry batch of either size holds every class, and the smaller one holds short frames
    short = set(fz.subset("short"))
    for n in SPLIT_N:
        sel = fz.geometry_batch(n, 5)
        assert len(sel) == n
        for c in fz.GEOMETRY:
            assert len(set(sel.tolist()) & set(fz.subset(c))) >= min(n // 4, len(fz.subset(c)))
        assert set(sel.tolist()) & short
    every = set(fz.geometry_batch(128, 5).tolist())
    assert every >= set(fz.subset("tall", "wide", "pool")) and every >= short


def test_whole_batches_hold_the_whole_zoo(zoo):
    for n in (len(zoo), CUS + 5, 2 * CUS + 5):
        sel = fz.whole_batch(n, 3)
        assert sorted(sel.tolist()) == list(range(n))
    d, o, h = fz.master(CUS + 5)
    big = fz.master(2 * CUS + 5)
    assert np.array_equal(big[1][:CUS + 6], o) and np.array_equal(big[2][:CUS + 5], h)
    assert np.array_equal(big[0][:o[-1]].view(np.uint32), d.view(np.uint32))
    sel = np.array([7, 0, 229, 7])
    td, to, th = fz.take(big, sel)
    for k, i in enumerate(sel):
        assert np.array_equal(td[to[k]:to[k + 1]].view(np.uint32), zoo[i].img.reshape(-1).view(np.uint32))
        assert th[k].tolist() == [640, 480, zoo[i].place[0], zoo[i].place[1], zoo[i].place[0] + zoo[i].img.shape[1],
                                  zoo[i].place[1] + zoo[i].img.shape[0]]


def test_augmented_zoo_is_still_a_zoo(zoo, plain):
    parts = fz.master(len(zoo))
    xf = fz.aug_maps(plain["mid_p"])
    ident = fz.aug_maps(np.zeros((5, 3)))[0]
    assert (xf[::5] == ident).all() and not (xf[1::5] == ident).all(axis=1).any()
    aug = oracle.voxelize_aug(*parts, xf, R=32, n_threads=8)
    assert (aug["status"] == 0).sum() >= 0.9 * len(zoo)
    np.testing.assert_array_equal(aug["status"], plain["status"])
    # the oracle's plain and identity-map placements agree bit for bit (and so do, here, the volumes)
    every5 = slice(0, None, 5)
    for k in ("max_l", "mid_p"):
        np.testing.assert_array_equal(aug[k][every5].view(np.uint32), plain[k][every5].view(np.uint32))
    alli = oracle.voxelize_aug(*parts, np.tile(ident, (len(zoo), 1)), R=32, n_threads=8)
    np.testing.assert_array_equal(alli["status"], plain["status"])
    for k in ("max_l", "mid_p"):
        np.testing.assert_array_equal(alli[k].view(np.uint32), plain[k].view(np.uint32))
    assert float(np.abs(alli["tsdf"] - plain["tsdf"]).max()) <= 1e-5
    # a general map moves the grid
    assert (aug["max_l"][1::5] != plain["max_l"][1::5]).mean() > 0.9
