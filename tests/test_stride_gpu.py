"""GPU tier of the grid-stride loops: tsdf_obb_kernel, tsdf_map_place_kernel, tsdf_map_step_head_kernel, tsdf_locate_kernel
and tsdf_locate_copy_kernel with more batch positions than workgroups (GRID = 65536), so that a workgroup takes a second
and a third position and reuses its LDS partials; and tsdf_locate_scan_kernel with more than one header per thread.

Every entry runs at N2 = GRID + 4096 and N3 = 2 GRID + 257 positions whose kinds tests/stride_ref.py lays out (every kind
behind every kind), into sentinel-filled outputs, three times: twice into the same buffers and once on a side stream.
After each run every row of every output is compared, on the device and on the bits, with the row of the same source frame
in a launch of the K source frames alone — one position per workgroup, the path the other test files hold to their
references.  That small launch is itself held to its reference here with the helpers and bounds of tests/test_obb_gpu.py,
tests/test_place_gpu.py, tests/test_mapstep_gpu.py and tests/test_locate_gpu.py.  No position is skipped and nothing
here has a tolerance of its own."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_zoo as fz  # noqa: E402
import locate_ref as lr  # noqa: E402
import obb_ref as ob  # noqa: E402
import stride_ref as sr  # noqa: E402
import test_locate_gpu as tlg  # noqa: E402
import test_mapstep_gpu as tmg  # noqa: E402
import test_obb_gpu as tog  # noqa: E402
import test_place_gpu as tpg  # noqa: E402

pytestmark = pytest.mark.gpu

PKG = "handposeestimation-with-3d-cnns_amd"
R = 8
KEY = 0x5712DE0FACE0FF1C
NS = (sr.N2, sr.N3)
VIEW = {torch.float64: torch.int64, torch.float32: torch.int32}


def dev():
    return torch.device("cuda")


def up(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the shared inputs are read-only)


def bits(t):
    v = VIEW.get(t.dtype)
    return t.contiguous().view(v) if v is not None else t


def same(a, b):
    return a.dtype is b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def sentinel(shape, dtype):
    """NaN for floats, -7 for integers."""
    return torch.full(shape, float("nan") if dtype.is_floating_point else -7, dtype=dtype, device=dev())


def untouched(t):
    return bool(torch.isnan(t).all()) if t.dtype.is_floating_point else bool((t == -7).all())


def no_sentinel(t):
    return not bool(torch.isnan(t).any()) if t.dtype.is_floating_point else not bool((t == -7).any())


def three_runs(launch, check):
    """Twice into the same buffers, then once on a side stream: ``check`` after each."""
    for _ in range(2):
        launch()
        torch.cuda.synchronize()
        check()
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    side.synchronize()
    check()


def vx():
    return importlib.import_module(PKG + ".voxelize")


@pytest.fixture(scope="module", autouse=True)
def _release_device_caches():
    """The cached inputs and small launches live on the device for this module alone."""
    yield
    for f in (crop_pack, obb_small, obb_big, source_maps, index_of, place_small, head_sources, head_small, loc_frames,
              loc_index, loc_small):
        f.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def crop_pack():
    return tuple(up(a) for a in sr.crop_pack())


# ---- obb_xforms --------------------------------------------------------------------------------------------------------

def raw_obb(pkg, d, o, h, xf, mo, st):
    """tsdf_obb_xforms_hip with caller-owned outputs; ``mo`` and ``st`` may be None."""
    v = vx()
    v._call(d.device, pkg._lib.load_obb().tsdf_obb_xforms_hip,
            [d.data_ptr(), d.numel(), o.data_ptr(), h.data_ptr(), h.shape[0], None, None, xf.data_ptr(), v._ptr(mo),
             v._ptr(st)], 6)


@functools.lru_cache(maxsize=None)
def obb_small(pkg):
    """The K crops alone -> (xforms [K, 24], moments [K, 16], status [K]), sentinel-free."""
    d, o, h = crop_pack()
    K = h.shape[0]
    xf, mo, st = sentinel((K, 24), torch.float64), sentinel((K, 16), torch.float64), sentinel((K,), torch.int32)
    raw_obb(pkg, d, o, h, xf, mo, st)
    torch.cuda.synchronize()
    assert no_sentinel(xf) and no_sentinel(mo) and no_sentinel(st)
    return xf, mo, st


@functools.lru_cache(maxsize=None)
def obb_big(n):
    """The tiled pack of n positions on the device and the source of every position."""
    depth, off, hdr = (torch.from_numpy(a.copy()) for a in sr.crop_pack())
    t = sr.table(n, 11, sr.OBB_KINDS)
    src = torch.from_numpy(sr.draw_sources(t, sr.sources_of(sr.OBB_KINDS, obb=True), len(hdr), 12))
    return tuple(a.to(dev()) for a in sr.tile(depth, off, hdr, src)) + (src.to(dev()),)


def test_obb_small_launch_against_the_restatement(pkg):
    depth, off, hdr = sr.crop_pack()
    xf, mo, st = (t.cpu().numpy() for t in obb_small(pkg))
    got = pkg.ObbBatch(xf, st, mo[:, 0], mo[:, 1:4], mo[:, 4:10], mo[:, 10:13])
    ref = ob.batch(depth, off, hdr)
    assert st.tolist() == [f["status"] for f in ref] and mo[:, 0].tolist() == [f["N"] for f in ref]
    assert sorted(set(st.tolist())) == [0, 1, 2]
    for i, f in enumerate(ref):
        if f["status"] == 0:
            tog.check_frame(got, i, f, compare_axes=False)        # rank-deficient crops among them: ties at 0
        else:   # the identity map with the contract's moments: N (0 under a bad header), then zeros
            assert np.array_equal(xf[i], ob.identity()) and not mo[i, 1:].any() and not np.signbit(mo[i]).any(), i
        assert not mo[i, 13:].any()


@pytest.mark.parametrize("optional", ["moments+status", "moments", "status", "neither"])
@pytest.mark.parametrize("n", NS)
def test_obb_every_position_equals_its_frame_alone(pkg, n, optional):
    d, o, h, src = obb_big(n)
    small_xf, small_mo, small_st = obb_small(pkg)
    xf = sentinel((n, 24), torch.float64)
    mo = sentinel((n, 16), torch.float64) if "moments" in optional else None
    st = sentinel((n,), torch.int32) if "status" in optional else None

    def check():
        assert same(xf, small_xf[src])
        assert mo is None or same(mo, small_mo[src])
        assert st is None or same(st, small_st[src])

    three_runs(lambda: raw_obb(pkg, d, o, h, xf, mo, st), check)
    assert int(h.shape[0]) == n and set(small_st[src].unique().tolist()) == {0, 1, 2}


# ---- map_grids ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def source_maps():
    """float64[K, 24] on the device: seeded random_affines about a seeded centre per source frame, the identity for every
    fifth frame; and the centres, float32[K, 3]."""
    aug = importlib.import_module(PKG + ".augment")
    K = len(sr.crops())
    centres = (np.random.default_rng(21).normal(0, 100, (K, 3)) + [0, 0, -650]).astype(np.float32)
    xf = aug.random_affines(centres.astype(np.float64), rng=22)[0].copy()
    xf[::5] = aug.identity_affines(len(xf[::5]))
    return up(xf), up(centres)


@functools.lru_cache(maxsize=None)
def index_of(n, seed=31):
    """int64[n] on the device: the source frame of every position, -1 and K at the bad_index positions."""
    K = len(sr.crops())
    if n <= sr.GRID:
        return up(sr.small_index(K))
    return up(sr.draw_sources(sr.table(n, seed, sr.KINDS), sr.sources_of(sr.KINDS), K, seed + 1))


def raw_place(pkg, index, xf, grid, max_l, mid_p, status):
    """tsdf_map_place_hip on the K crops with caller-owned outputs; all but ``grid`` may be None."""
    v = vx()
    d, o, h = crop_pack()
    n = index.shape[0]
    v._call(d.device, pkg._lib.load_maplowp().tsdf_map_place_hip,
            v._src_head(d, o, h, h.shape[0], index, n, R) +
            [None, None, xf.data_ptr(), grid.data_ptr(), v._ptr(max_l), v._ptr(mid_p), v._ptr(status)], 9)


def place_outputs(n, optional=("max_l", "mid_p", "status")):
    return (sentinel((n, 8), torch.float32), sentinel((n,), torch.float32) if "max_l" in optional else None,
            sentinel((n, 3), torch.float32) if "mid_p" in optional else None,
            sentinel((n,), torch.int32) if "status" in optional else None)


@functools.lru_cache(maxsize=None)
def place_small(pkg):
    """The K crops and the two bad indices: K + 2 positions, one workgroup each."""
    K = len(sr.crops())
    index = index_of(K + 2)
    xf = source_maps()[0][index.clamp(0, K - 1)].contiguous()
    outs = place_outputs(K + 2)
    raw_place(pkg, index, xf, *outs)
    torch.cuda.synchronize()
    assert all(no_sentinel(t) for t in outs)
    return outs


def test_place_small_launch_against_the_oracle(pkg):
    cs = sr.crops()
    K = len(cs)
    ok = [j for j, c in enumerate(cs) if sr.is_ok(c.kind)]
    d, o, h = fz.take(sr.crop_pack(), ok)
    xf = source_maps()[0][up(np.array(ok))].contiguous()
    mg = pkg.map_grids(up(d), up(o), up(h), xf, res=R)
    torch.cuda.synchronize()
    tpg.assert_placed_as_the_oracle(mg, d, o, h, xf.cpu().numpy())
    grid, max_l, mid_p, status = place_small(pkg)
    for a, b in zip(mg, (grid, max_l, mid_p, status)):
        assert same(a, b[up(np.array(ok))])                       # the rows of the launch the big ones are compared with
    want = [0 if sr.is_ok(c.kind) else 1 if c.kind == "degenerate" else 2 for c in cs] + [2, 2]
    assert status.tolist() == want
    bad = status != 0
    assert not bool(grid[bad].any()) and not bool(max_l[bad].any()) and not bool(mid_p[status == 2].any())


@pytest.mark.parametrize("optional", [("max_l", "mid_p", "status"), ("status",), ("max_l",), ("mid_p",), ()],
                         ids=["all", "status", "max_l", "mid_p", "grid_only"])
@pytest.mark.parametrize("n", NS)
def test_place_every_position_equals_its_frame_alone(pkg, n, optional):
    K = len(sr.crops())
    index = index_of(n)
    row = sr.small_row(index, K)
    xf = source_maps()[0][index.clamp(0, K - 1)].contiguous()
    outs = place_outputs(n, optional)
    small = place_small(pkg)

    def check():
        for got, want in zip(outs, small):
            assert got is None or same(got, want[row])

    three_runs(lambda: raw_place(pkg, index, xf, *outs), check)
    assert set(small[3][row].unique().tolist()) == {0, 1, 2}


# ---- map_step_head -----------------------------------------------------------------------------------------------------

J = 21


@functools.lru_cache(maxsize=None)
def head_sources(pkg):
    """base float64[K, 24] (the crops' own principal-axis maps; the identity where there is none) and gt float32[K, J, 3]."""
    d, o, h = crop_pack()
    base = pkg.obb_xforms(d, o, h).xforms
    centres = source_maps()[1]
    gt = centres[:, None, :] + up(np.random.default_rng(23).normal(0, 80, (h.shape[0], J, 3)).astype(np.float32))
    torch.cuda.synchronize()
    return base, gt.contiguous()


def head_kw(pkg, with_gt, with_base):
    base, gt = head_sources(pkg)
    return dict(base=base if with_base else None, gt=gt if with_gt else None, res=R)


def head_into(pkg, n, state, index, counters, with_gt, with_base):
    """(launch, fields): tsdf_map_step_head_hip on the K crops with EVERY output caller-owned and sentinel-filled —
    map_step_head itself allocates ``stretch`` and ``rot``, and a fresh allocation may hold the previous run's values."""
    v = vx()
    d, o, h = crop_pack()
    kw = head_kw(pkg, with_gt, with_base)
    out = tmg.sentinel_out(pkg, n, gt_shape=(J, 3) if with_gt else None)
    got = dict(zip(tmg.FIELDS, (*out, sentinel((n,), torch.float64), sentinel((n, 2), torch.int32))))
    args = (v._src_head(d, o, h, h.shape[0], index, n, R) + v._cam5(None) +
            [source_maps()[1].data_ptr(), v._ptr(kw["base"]), state.data_ptr(), v._ptr(counters), v._ptr(kw["gt"]),
             J if with_gt else 0, 1, None] + [v._ptr(got[k]) for k in tmg.FIELDS])

    def launch(keep=(state, index, counters, kw)):   # (the arguments are raw pointers: their tensors live as long as this)
        v._call(d.device, pkg._lib.load_mapstep().tsdf_map_step_head_hip, list(args), 20)

    return launch, got


@functools.lru_cache(maxsize=None)
def head_small(pkg, with_gt, with_base):
    """K + 2 positions (the crops, then the bad indices -1 and K), counters = index."""
    K = len(sr.crops())
    index = index_of(K + 2)
    launch, got = head_into(pkg, K + 2, pkg.aug_state(KEY, 5, device=dev()), index, index, with_gt, with_base)
    launch()
    torch.cuda.synchronize()
    assert all(no_sentinel(got[k]) for k in ("xforms", "grid", "max_l", "mid_p", "status", "rot"))
    assert not with_gt or (no_sentinel(got["gt_aug"]) and no_sentinel(got["gt_nor"]))
    return got


@pytest.mark.parametrize("with_base", [True, False], ids=["base", "nobase"])
@pytest.mark.parametrize("with_gt", [True, False], ids=["gt", "nogt"])
def test_head_small_launch_against_the_chain(pkg, with_gt, with_base):
    d, o, h = crop_pack()
    K = h.shape[0]
    index = index_of(K + 2)
    got = head_small(pkg, with_gt, with_base)
    want = tmg.chain(pkg, d, o, h, source_maps()[1], pkg.aug_state(KEY, 5, device=dev()), index=index, counters=index,
                     **head_kw(pkg, with_gt, with_base))
    torch.cuda.synchronize()
    tmg.assert_same(got, want)
    assert same(got["status"], place_small(pkg)[3])                # the kinds are the placement's


@pytest.mark.parametrize("with_base", [True, False], ids=["base", "nobase"])
@pytest.mark.parametrize("with_gt", [True, False], ids=["gt", "nogt"])
@pytest.mark.parametrize("n", NS)
def test_head_every_position_equals_its_frame_alone(pkg, n, with_gt, with_base):
    """(a) counters[i] = index[i]: position i draws what the small launch's row of the same source frame drew."""
    K = len(sr.crops())
    index = index_of(n)
    row = sr.small_row(index, K)
    small = head_small(pkg, with_gt, with_base)
    launch, got = head_into(pkg, n, pkg.aug_state(KEY, 5, device=dev()), index, index, with_gt, with_base)

    def check():
        for name in tmg.FIELDS:
            if small[name] is None:
                assert got[name] is None
            else:
                assert same(got[name], small[name][row]), name

    three_runs(launch, check)


@pytest.mark.parametrize("with_base", [True, False], ids=["base", "nobase"])
@pytest.mark.parametrize("with_gt", [True, False], ids=["gt", "nogt"])
@pytest.mark.parametrize("n", NS)
def test_head_equals_the_chain_past_the_grid(pkg, n, with_gt, with_base):
    """(b) default counters (counter0 + i, wrapping mod 2^64 inside the batch): every output against the chain of entries
    that tests/test_mapstep_gpu.py::test_head_equals_the_chain_on_every_output uses."""
    d, o, h = crop_pack()
    index = index_of(n)
    state = pkg.aug_state(KEY + n, (1 << 64) - sr.GRID - 40, device=dev())
    want = tmg.chain(pkg, d, o, h, source_maps()[1], state, index=index, **head_kw(pkg, with_gt, with_base))
    launch, got = head_into(pkg, n, state, index, None, with_gt, with_base)
    three_runs(launch, lambda: tmg.assert_same(got, want))
    assert no_sentinel(got["xforms"]) and no_sentinel(got["grid"]) and no_sentinel(got["status"])
    assert not with_gt or no_sentinel(got["gt_nor"])


# ---- locate_hands ------------------------------------------------------------------------------------------------------

LOC_FIELDS = ("headers", "com", "count", "status", "grid", "max_l", "mid_p")


def hip_cam(pkg):
    return pkg.TsdfCam(*sr.LOC_CAM)


@functools.lru_cache(maxsize=None)
def loc_frames(u16):
    return up(sr.locate_frames_u16() if u16 else sr.locate_frames()[0])


@functools.lru_cache(maxsize=None)
def loc_index(n):
    K = len(sr.locate_frames()[0])
    if n <= sr.GRID and n == K + 2:
        return up(sr.small_index(K))
    if n <= sr.GRID:     # the scan sizes: every source in turn, a bad index every 37th position
        idx = np.arange(n, dtype=np.int64) * 7 % K
        idx[::37] = np.where(np.arange(len(idx[::37])) % 2, K, -1)
        return up(idx)
    return up(sr.draw_sources(sr.table(n, 41, sr.LOCATE_KINDS), sr.locate_sources(), K, 42))


def loc_kw(pkg, u16, refine, band):
    return dict(cam=hip_cam(pkg), refine=refine, seed_band=band, res=R, shift=sr.LOC_SHIFT if u16 else None)


def loc_sentinel(pkg, n):
    per = lr.capacity(sr.LOC_H, sr.LOC_W, 250.0, 100.0, sr.LOC_CAM[0])
    return pkg.HandCrops(sentinel((n * per,), torch.float32), sentinel((n + 1,), torch.int64), sentinel((n, 6), torch.int32),
                         sentinel((n, 3), torch.float64), sentinel((n,), torch.int32), sentinel((n,), torch.int32),
                         sentinel((n, 8), torch.float32), sentinel((n,), torch.float32), sentinel((n, 3), torch.float32))


@functools.lru_cache(maxsize=None)
def loc_small(pkg, u16, refine, band):
    K = len(sr.locate_frames()[0])
    out = loc_sentinel(pkg, K + 2)
    got = pkg.locate_hands(loc_frames(u16), index=loc_index(K + 2), out=out, **loc_kw(pkg, u16, refine, band))
    torch.cuda.synchronize()
    assert all(no_sentinel(getattr(got, k)) for k in LOC_FIELDS + ("offsets",))
    return got


def loc_check(got, small, row):
    """Every field of every position, the crops and the offsets against the small launch's rows ``row``; nothing written
    at or beyond offsets[n]."""
    for k in LOC_FIELDS:
        assert same(getattr(got, k), getattr(small, k)[row]), k
    want_depth, want_off, _ = sr.tile(small.depth, small.offsets, small.headers, row)
    hdr = got.headers.cpu().numpy().astype(np.int64)
    sizes = (hdr[:, 4] - hdr[:, 2]) * (hdr[:, 5] - hdr[:, 3])
    assert np.array_equal(got.offsets.cpu().numpy(), np.concatenate([[0], np.cumsum(sizes)]))      # exactly
    assert torch.equal(got.offsets, want_off)
    total = int(want_off[-1])
    assert same(got.depth[:total], want_depth)
    assert untouched(got.depth[total:])


@pytest.mark.parametrize("band", [0.0, 150.0], ids=["band0", "band150"])
@pytest.mark.parametrize("refine", [0, 1, 2])
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_locate_small_launch_against_the_reference(pkg, u16, refine, band):
    frames = sr.locate_frames()[0]
    K = len(frames)
    small = loc_small(pkg, u16, refine, band)
    out = {k: getattr(small, k).cpu().numpy() for k in tlg.FIELDS}
    out["depth"] = small.depth.cpu().numpy()[:int(out["offsets"][-1])]
    p = tlg.params(refine=refine, seed_band=band)
    refs = [lr.locate_frame(f, sr.LOC_CAM, R=R, **p) for f in frames] + [dict(status=2)] * 2
    padded = np.concatenate([frames, np.zeros((2,) + frames.shape[1:], np.float32)])
    tlg.check(out, padded, refs, sr.LOC_CAM, p, R=R)
    assert sorted(set(out["status"].tolist())) == [0, 1, 2]


@pytest.mark.parametrize("band", [0.0, 150.0], ids=["band0", "band150"])
@pytest.mark.parametrize("refine", [0, 1, 2])
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
@pytest.mark.parametrize("n", NS)
def test_locate_every_position_equals_its_frame_alone(pkg, n, u16, refine, band):
    K = len(sr.locate_frames()[0])
    index = loc_index(n)
    row = sr.small_row(index, K)
    small = loc_small(pkg, u16, refine, band)
    out = loc_sentinel(pkg, n)
    kw = loc_kw(pkg, u16, refine, band)
    three_runs(lambda: pkg.locate_hands(loc_frames(u16), index=index, out=out, **kw), lambda: loc_check(out, small, row))
    assert set(out.status.unique().tolist()) == {0, 1, 2}


@pytest.mark.parametrize("n", sr.SCAN_NS)
def test_scan_kernel_with_more_than_one_header_per_thread(pkg, n):
    """tsdf_locate_scan_kernel alone decides the offsets: thread t sums and then writes the chunk of ceil(n / 1024) headers
    that starts at t * chunk, so these sizes give chunks of 1, 1, 2, 2, 3 and 4 with empty trailing chunks."""
    K = len(sr.locate_frames()[0])
    index = loc_index(n)
    small = loc_small(pkg, False, 2, 150.0)
    out = loc_sentinel(pkg, n)
    kw = loc_kw(pkg, False, 2, 150.0)
    three_runs(lambda: pkg.locate_hands(loc_frames(False), index=index, out=out, **kw),
               lambda: loc_check(out, small, sr.small_row(index, K)))
    assert -(-n // 1024) == {1023: 1, 1024: 1, 1025: 2, 2047: 2, 2049: 3, 3073: 4}[n]
    assert set(out.status.unique().tolist()) == {0, 1, 2}
