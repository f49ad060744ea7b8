"""GPU tier: every kernel on buffers that pass the 32-bit range — an element index >= 2^31 or a byte offset >= 2^32.

The smallest shape at which a 32-bit index can fail is 2^31 elements, so the buffers here are that size and no larger:
 (a) a 7-frame pack whose crops sit at element offsets around 2^30 (byte 2^32) and 2^31, every entry that reads a pack
     (``ENTRIES`` and voxelize_indexed; the two accurate entries voxelize_grid_accurate and voxelize_map_grid_accurate
     among them, with their ``nearest``) against the same entry on a compact pack of the same crops, bit for bit;
 (b) 344 volumes at 128^3 (8.65 GB of float32, 4.3 GB of 16-bit voxels) from voxelize, voxelize_aug, voxelize_aug_grid,
     voxelize_grid_lowp and voxelize_map_grid_lowp, every position against the oracle; and 513 volumes at 128^3 with
     their ``nearest`` (17.3 GiB) from each accurate entry, on sparse frames, against the brute-force reference;
 (c) widen_depth16 and narrow_volumes over 2^31 + 4099 elements against torch's own arithmetic;
 (d) locate_hands on 699,060 frames of 64 x 48 (more than 2^31 pixels), uint16 and float32, against a compact tensor.
Each test states its need of device memory, asks the device first and skips (with both figures) if that plus 2 GiB is not
free, and frees what it made.  Each entry is a case of its own; once a case has left the device in an error state the
later ones fail at once instead of launching."""
import functools
import importlib
import os
import sys
import time
import types

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accurate_ref as acr  # noqa: E402
import auggrid_ref as ar  # noqa: E402
import locate_ref as lr  # noqa: E402
import plan_ref as pr  # noqa: E402
import sparse_ref as sp  # noqa: E402
from test_lowp_gpu import in_band  # noqa: E402
from test_resolutions_gpu import accurate_launch, accurate_sources, cu_count, cycle, dev, up, worst_error  # noqa: E402

pytestmark = pytest.mark.gpu

PKG = pr.PKG
TOL = 1e-5
GIB = 1 << 30
P31 = 1 << 31
N_STREAM = P31 + 4099           # (c): elements of the streams
VIEW = {torch.float64: torch.int64, torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}

_state = {"faulted": None, "base": 0}


@pytest.fixture(autouse=True)
def _stop_after_a_fault(request):
    """A case that leaves the device in an error state is the last one that launches anything."""
    if _state["faulted"]:
        pytest.fail("not launched: the device was left in an error state by " + _state["faulted"])
    yield
    try:
        torch.cuda.synchronize()
    except Exception:     # noqa: BLE001 — whatever the runtime raises, nothing more may be launched
        _state["faulted"] = request.node.name
        raise


def need_memory(gib):
    """The memory rule: skip, with both figures in the reason, unless ``gib`` + 2 GiB of device memory is free."""
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(dev())[0]
    if free < (gib + 2) * GIB:
        pytest.skip(f"needs {gib} GiB + 2 GiB of free device memory, {free / GIB:.1f} GiB is free")
    torch.cuda.reset_peak_memory_stats(dev())
    _state["base"] = torch.cuda.memory_allocated(dev())


def report_peak(what):
    """The test's own peak: above what the module's fixtures held when it began."""
    print(f"{what}: peak device memory {(torch.cuda.max_memory_allocated(dev()) - _state['base']) / GIB:.2f} GiB")


def same(a, b):
    """Equal on the bits (NaN by pattern, -0 != +0)."""
    if a.dtype is not b.dtype or a.shape != b.shape:
        return False
    v = VIEW.get(a.dtype)
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v)) if v is not None else torch.equal(a, b)


# ---- (a) pack offsets beyond 2^31 --------------------------------------------------------------------------------------
R_A = 16
KS = (0, 2, 4, 5)                     # the table's positions of crops K0..K3
FILLERS = (1, 3, 6)
INDEX = (4, 5, 2, 0, 5)               # K2, K3, K1, K0, K3
INDEX4 = (2, 3, 1, 0, 3)              # the same frames in the 4-frame pack
BIG_LEN = P31 + (1 << 22)
BIG_K1, BIG_K2 = (1 << 30) - 5001, P31 - 7003


@functools.lru_cache(maxsize=None)
def _crops():
    """K0..K3: the four seeded crops of the resolution tests."""
    return importlib.import_module(PKG + ".synth").synth_batch(4, "crop", seed0=42)


def _table(k1, k2, total):
    """offsets int64[8] and headers int32[7,6] of the 7-frame table: K0 at 0, K1 at k1, K2 at k2, K3 behind it, fillers
    in between and up to ``total``.  A filler's header says one pixel, its slot holds another count: a bad header."""
    depth, off, hdr = _crops()
    s = [int(off[i + 1] - off[i]) for i in range(4)]
    k3 = k2 + s[2]
    offsets = np.array([0, s[0], k1, k1 + s[1], k2, k3, k3 + s[3], total], np.int64)
    assert (np.diff(offsets) > 1).all()
    headers = np.tile(np.array([320, 240, 0, 0, 1, 1], np.int32), (7, 1))
    headers[list(KS)] = hdr
    return offsets, headers


def _fill(buf, offsets):
    depth, off, _ = _crops()
    for j, p in enumerate(KS):
        buf[int(offsets[p]):int(offsets[p + 1])] = torch.from_numpy(depth[off[j]:off[j + 1]]).to(buf.device)


@pytest.fixture(scope="module")
def packs():
    """The big pack (needs 8.1 GiB: float32[2^31 + 2^22], zeros but for the four crops) and the compact one: the same
    seven table positions — so that what depends on a frame's NUMBER (point_clouds' draw, the step head's counters) is the
    same in both — with fillers of a few elements, every crop at the same address modulo 256 bytes as in the big pack (so
    that only the address range differs, not the alignment).  Plus the inputs both share: one map, one grid row under it
    and one plain row per table position, from the oracle.  And ``four``: the plain 4-frame pack of the same crops (other
    addresses modulo 16 bytes), which the crops' results must equal as well."""
    need_memory(8.1)
    depth, off, hdr = _crops()
    s = [int(off[i + 1] - off[i]) for i in range(4)]
    k1 = s[0] + 8
    k1 += (BIG_K1 - k1) % 64
    k2 = k1 + s[1] + 8
    k2 += (BIG_K2 - k2) % 64
    assert k1 % 64 == BIG_K1 % 64 and k2 % 64 == BIG_K2 % 64 and BIG_K1 % 4 != 0
    small_o, small_h = _table(k1, k2, k2 + s[2] + s[3] + 8)
    big_o, big_h = _table(BIG_K1, BIG_K2, BIG_LEN)
    # K1 straddles byte 2^32, K2 element 2^31, K3 lies beyond it
    assert big_o[2] * 4 < (1 << 32) < big_o[3] * 4 and big_o[4] < P31 < big_o[5] and big_o[5] > P31
    assert np.array_equal(big_h, small_h)
    out = {}
    for name, o, h in (("big", big_o, big_h), ("small", small_o, small_h)):
        buf = torch.zeros(int(o[-1]), dtype=torch.float32, device=dev())
        _fill(buf, o)
        to, th = up(o, h)
        out[name] = types.SimpleNamespace(d=buf, o=to, h=th)
    # the shared inputs, from the oracle on the four crops
    plain = oracle.voxelize(depth, off, hdr, R=R_A, n_threads=4, extras=True)
    assert not plain["status"].any()
    aug = importlib.import_module(PKG + ".augment")
    xf4 = aug.random_affines(plain["mid_p"].astype(np.float64), rng=31)[0]
    xf = aug.identity_affines(7)
    rows, arows, centres = np.zeros((7, 8), np.float32), np.zeros((7, 8), np.float32), np.zeros((7, 3), np.float32)
    ks = list(KS)
    xf[ks] = xf4
    rows[ks, :3], rows[ks, 3], rows[ks, 4] = plain["ori"], plain["grid"][:, 4], plain["grid"][:, 5]
    arows[ks] = ar.pixel_grids(depth, off, hdr, xf4, R_A)[0]
    centres[ks] = plain["mid_p"]
    t = up(xf, rows, arows, centres)
    out["aux"] = types.SimpleNamespace(xf=t[0], rows=t[1], arows=t[2], centres=t[3], oracle=plain, pos=None)
    # the compact pack as packing makes it: the four crops back to back, and their rows of the shared inputs; ``pos`` says
    # which table position each of its frames holds in the big pack
    fd, fo, fh = up(depth, off, hdr)
    out["four"] = types.SimpleNamespace(d=fd, o=fo, h=fh)
    kt = torch.tensor(ks, dtype=torch.int64, device=dev())
    out["aux4"] = types.SimpleNamespace(xf=t[0][kt].contiguous(), rows=t[1][kt].contiguous(), arows=t[2][kt].contiguous(),
                                        centres=t[3][kt].contiguous(), oracle=plain, pos=kt)
    torch.cuda.synchronize()
    yield types.SimpleNamespace(**out)
    out.clear()
    torch.cuda.empty_cache()


def _batch(b):
    return dict(tsdf=b.tsdf, max_l=b.max_l, mid_p=b.mid_p, status=b.status)


def _voxelize(pkg, P, A, idx):
    return _batch(pkg.voxelize(P.d, P.o, P.h, res=R_A))


def _voxelize_indexed(pkg, P, A, idx):
    return _batch(pkg.voxelize_indexed(P.d, P.o, P.h, idx, res=R_A))


def _voxelize_aug(pkg, P, A, idx):
    return _batch(pkg.voxelize_aug(P.d, P.o, P.h, A.xf, res=R_A))


def _aabb(pkg, P, A, idx):
    return pkg.aabb(P.d, P.o, P.h, res=R_A)._asdict()


def _voxelize_grid(pkg, P, A, idx):
    tsdf, st = pkg.voxelize_grid(P.d, P.o, P.h, A.rows, res=R_A)
    return dict(tsdf=tsdf, status=st)


def _per_frame(P, A, call):
    """An entry whose draw depends on the frame's NUMBER, on the 4-frame pack: frame j alone, numbered as in the table."""
    parts = [call(P.d, P.o[j:j + 2], P.h[j:j + 1], int(A.pos[j]))._asdict() for j in range(len(A.pos))]
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


def _point_clouds(pkg, P, A, idx):
    call = lambda d, o, h, base: pkg.point_clouds(d, o, h, points=1000, seed=5, frame_base=base)    # noqa: E731
    return call(P.d, P.o, P.h, 0)._asdict() if A.pos is None else _per_frame(P, A, call)


def _obb_xforms(pkg, P, A, idx):
    return pkg.obb_xforms(P.d, P.o, P.h)._asdict()


def _voxelize_aug_grid(pkg, P, A, idx):
    tsdf, st = pkg.voxelize_aug_grid(P.d, P.o, P.h, A.xf, A.arows, res=R_A)
    return dict(tsdf=tsdf, status=st)


def _voxelize_grid_lowp(pkg, P, A, idx):
    out = {}
    for kind, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        tsdf, st = pkg.voxelize_grid_lowp(P.d, P.o, P.h, A.rows, res=R_A, dtype=dt, index=idx)
        out["tsdf_" + kind], out["status_" + kind] = tsdf, st
    return out


def _map_grids_and_lowp(pkg, P, A, idx):
    xf = A.xf if idx is None else A.xf.index_select(0, idx)
    mg = pkg.map_grids(P.d, P.o, P.h, xf, res=R_A, index=idx)
    out = dict(grid=mg.grid, max_l=mg.max_l, mid_p=mg.mid_p, status=mg.status)
    for kind, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        tsdf, st = pkg.voxelize_map_grid_lowp(P.d, P.o, P.h, xf, mg.grid, res=R_A, dtype=dt, index=idx)
        out["tsdf_" + kind], out["status_" + kind] = tsdf, st
    return out


def _voxelize_grid_accurate(pkg, P, A, idx):
    tsdf, st, nn = pkg.voxelize_grid_accurate(P.d, P.o, P.h, A.rows, res=R_A, index=idx, nearest=True)     # rows of SOURCES
    return dict(tsdf=tsdf, status=st, nearest=nn)


def _voxelize_map_grid_accurate(pkg, P, A, idx):
    xf, arows = (A.xf, A.arows) if idx is None else (A.xf.index_select(0, idx), A.arows.index_select(0, idx))
    tsdf, st, nn = pkg.voxelize_map_grid_accurate(P.d, P.o, P.h, xf, arows, res=R_A, index=idx, nearest=True)
    return dict(tsdf=tsdf, status=st, nearest=nn)


def _map_step_head(pkg, P, A, idx):
    # (position i draws from counter0 + i: the 4-frame pack's frames are given the table positions as their counters)
    counters = A.pos if idx is None else None
    b = pkg.map_step_head(P.d, P.o, P.h, A.centres, pkg.aug_state(77, 9, device=dev()), index=idx, counters=counters,
                          res=R_A)
    return dict(xforms=b.xforms, grid=b.grid, max_l=b.max_l, mid_p=b.mid_p, status=b.status)


def _process_batch(pkg, P, A, idx):
    call = lambda d, o, h, base: pkg.process_batch(d, o, h, points=1000, seed=5, frame_base=base, res=R_A)    # noqa: E731
    return call(P.d, P.o, P.h, 0)._asdict() if A.pos is None else _per_frame(P, A, call)


# entry -> (runner, takes an index, the outputs that are all-zero for a frame that is not OK)
ENTRIES = {
    "voxelize": (_voxelize, False, ("tsdf",)),
    "voxelize_aug": (_voxelize_aug, False, ("tsdf",)),
    "aabb": (_aabb, False, ()),
    "voxelize_grid": (_voxelize_grid, False, ("tsdf",)),
    "point_clouds": (_point_clouds, False, ("points",)),
    "obb_xforms": (_obb_xforms, False, ()),
    "voxelize_aug_grid": (_voxelize_aug_grid, False, ("tsdf",)),
    "voxelize_grid_lowp": (_voxelize_grid_lowp, True, ("tsdf_bf16", "tsdf_f16")),
    "map_grids_and_voxelize_map_grid_lowp": (_map_grids_and_lowp, True, ("grid", "tsdf_bf16", "tsdf_f16")),
    "voxelize_grid_accurate": (_voxelize_grid_accurate, True, ("tsdf",)),
    "voxelize_map_grid_accurate": (_voxelize_map_grid_accurate, True, ("tsdf",)),
    "map_step_head": (_map_step_head, True, ("grid",)),
    "process_batch": (_process_batch, False, ("points", "tsdf")),
}


def _compare(big, small, what):
    assert big.keys() == small.keys()
    for k in big:
        assert same(big[k], small[k]), (what, k)


def _status_keys(res):
    return [k for k in res if k.startswith("status")]


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_pack_offsets_beyond_2_31(pkg, packs, entry):
    """(a) The whole 7-frame table through the entry: every output equal, bit for bit, to the same entry on the compact
    table, and at K0..K3 to the same entry on the compact 4-frame pack; the crops OK and not empty, the fillers status 2
    with zero volumes / rows."""
    run, _, zero = ENTRIES[entry]
    big, small = run(pkg, packs.big, packs.aux, None), run(pkg, packs.small, packs.aux, None)
    four = run(pkg, packs.four, packs.aux4, None)
    torch.cuda.synchronize()
    _compare(big, small, entry)
    ks, fl = list(KS), list(FILLERS)
    _compare({k: v[ks] for k, v in big.items()}, four, entry + " (4-frame pack)")
    for k in _status_keys(big):
        assert big[k][ks].tolist() == [0] * 4 and big[k][fl].tolist() == [2] * 3, (entry, k, big[k].tolist())
    for k in zero:
        assert not bool(big[k][fl].float().abs().sum() != 0) and not bool(torch.isnan(big[k].float()).any()), (entry, k)
        assert all(bool((big[k][p] != 0).any()) for p in ks), (entry, k)
    if "nearest" in big:       # the accurate entries: a filler names no pixel, every crop has near voxels
        assert bool((big["nearest"][fl] == -1).all()) and all(bool((big["nearest"][p] >= 0).any()) for p in ks), entry
    if entry == "voxelize":    # once: the big pack's volumes against the oracle itself
        depth, off, hdr = _crops()
        ref = oracle.voxelize(depth, off, hdr, R=R_A, n_threads=4)
        got = big["tsdf"][ks]
        err = float(worst_error(got, up(ref["tsdf"])[0]))
        assert err <= TOL, err
        assert np.array_equal(big["max_l"][ks].cpu().numpy().view(np.uint32), ref["max_l"].view(np.uint32))
        assert np.array_equal(big["mid_p"][ks].cpu().numpy().view(np.uint32), ref["mid_p"].view(np.uint32))
        print(f"voxelize on the big pack: max |hip - oracle| = {err:.3g}")


@pytest.mark.parametrize("entry", [e for e, v in ENTRIES.items() if v[1]])
def test_pack_offsets_beyond_2_31_through_an_index(pkg, packs, entry):
    """(a) The entries that draw a batch by index, with [4, 5, 2, 0, 5]: K2, K3, K1, K0, K3."""
    run = ENTRIES[entry][0]
    idx = torch.tensor(INDEX, dtype=torch.int64, device=dev())
    big, small = run(pkg, packs.big, packs.aux, idx), run(pkg, packs.small, packs.aux, idx)
    four = run(pkg, packs.four, packs.aux4, torch.tensor(INDEX4, dtype=torch.int64, device=dev()))
    torch.cuda.synchronize()
    _compare(big, small, entry)
    _compare(big, four, entry + " (4-frame pack)")
    for k in _status_keys(big):
        assert big[k].tolist() == [0] * 5, (entry, k)
    for k in big:
        if k.startswith("tsdf") or k in ("grid", "nearest"):
            assert all(bool((big[k][p] != 0).any()) for p in range(5)), (entry, k)
            # positions 1 and 4 are both K3 (under the same map; the step head draws a map per position)
            assert same(big[k][1], big[k][4]) == (entry != "map_step_head") and not same(big[k][0], big[k][1]), (entry, k)


@pytest.mark.parametrize("size", ["5", "C/2+4", "2C+8"])
def test_voxelize_indexed_beyond_2_31(pkg, packs, size):
    """(a) voxelize_indexed at n = 5 (the split kernel) and, through the same index cycled, at C/2 + 4 (the fused kernel
    dealing by position) and 2C + 8 (its work queue and tail help)."""
    C = cu_count()
    n = {"5": 5, "C/2+4": C // 2 + 4, "2C+8": 2 * C + 8}[size]
    idx = cycle(torch.tensor(INDEX, dtype=torch.int64, device=dev()), n)
    big, small = _voxelize_indexed(pkg, packs.big, packs.aux, idx), _voxelize_indexed(pkg, packs.small, packs.aux, idx)
    four = _voxelize_indexed(pkg, packs.four, packs.aux4, cycle(torch.tensor(INDEX4, dtype=torch.int64, device=dev()), n))
    torch.cuda.synchronize()
    _compare(big, small, size)
    _compare(big, four, size + " (4-frame pack)")
    assert not bool(big["status"].any())
    # against the oracle as well: position i holds crop (2, 3, 1, 0, 3)[i % 5]
    ref = packs.aux.oracle
    order = list(INDEX4)
    err = float(worst_error(big["tsdf"], up(ref["tsdf"][order])[0]))
    assert err <= TOL, (size, err)
    assert np.array_equal(big["max_l"][:5].cpu().numpy().view(np.uint32), ref["max_l"][order].view(np.uint32))


# ---- (b) volume outputs beyond 2^31 elements ---------------------------------------------------------------------------
R_B, N_B, REPS = 128, 344, 86
VOL = 3 * R_B ** 3                     # elements of one position: 25 MB of float32


@pytest.fixture(scope="module")
def big_batch():
    """The four crops 86 times over (344 frames, about 20 MB), one map and one grid row per position, and the oracle's four
    plain and four mapped volumes at 128^3 on the device (0.2 GiB)."""
    need_memory(0.5)
    assert N_B == 4 * REPS and 85 * VOL * 4 < P31 <= 86 * VOL * 4 and 170 * VOL * 4 < (1 << 32) <= 171 * VOL * 4
    assert 341 * VOL < P31 < 342 * VOL and N_B * VOL > P31
    depth, off, hdr = _crops()
    plain = oracle.voxelize(depth, off, hdr, R=R_B, n_threads=4, extras=True)
    aug = importlib.import_module(PKG + ".augment")
    xf4 = aug.random_affines(plain["mid_p"].astype(np.float64), rng=31)[0]
    mapped = oracle.voxelize_aug(depth, off, hdr, xf4, R=R_B, n_threads=4)
    assert not plain["status"].any() and not mapped["status"].any()
    rows = np.zeros((4, 8), np.float32)
    rows[:, :3], rows[:, 3], rows[:, 4] = plain["ori"], plain["grid"][:, 4], plain["grid"][:, 5]
    arows = ar.pixel_grids(depth, off, hdr, xf4, R_B)[0]
    d, o, h = up(*pr.cycled(N_B, (depth, off, hdr)))
    t = up(xf4, rows, arows, plain["tsdf"], mapped["tsdf"])
    b = types.SimpleNamespace(d=d, o=o, h=h, xf=cycle(t[0], N_B), rows=cycle(t[1], N_B), arows=cycle(t[2], N_B), plain=t[3],
                              mapped=t[4], plain_np=plain, mapped_np=mapped)
    yield b
    del b, t, d, o, h
    torch.cuda.empty_cache()


def _copies_identical(vol):
    """Are all 86 copies of every crop's volume the same bits?  (reported, not asserted)"""
    v = vol.view(REPS, 4 * VOL).view(VIEW[vol.dtype])
    return all(bool((v[c0:c0 + 8] == v[0]).all()) for c0 in range(0, REPS, 8))


def _band_all(vol, ref):
    """in_band over every position, eight cycles of the four crops at a time."""
    v = vol.view(REPS, 4, 3, R_B, R_B, R_B)
    return all(in_band(v[c0:c0 + 8], ref, TOL) for c0 in range(0, REPS, 8))


def _nan_left(vol):
    return any(bool(torch.isnan(vol[p0:p0 + 32]).any()) for p0 in range(0, N_B, 32))


@pytest.mark.parametrize("entry", ["voxelize", "voxelize_aug", "voxelize_aug_grid", "voxelize_grid_lowp",
                                   "voxelize_map_grid_lowp"])
def test_volume_outputs_beyond_2_31(pkg, big_batch, record_property, entry):
    """(b) 344 positions at 128^3: position 85 crosses byte 2^31, position 170 byte 2^32, position 341 element 2^31.  Every
    position against the oracle's volume of its crop (float32: 1e-5; 16-bit: in_band), no NaN left of the pre-fill.
    Needs 8.1 GiB for a float32 output (4.1 GiB for a 16-bit one) and about 1.5 GiB for the comparison."""
    b = big_batch
    lowp = entry in ("voxelize_grid_lowp", "voxelize_map_grid_lowp")
    need_memory(6 if lowp else 10)
    shape = (N_B, 3, R_B, R_B, R_B)
    results = []
    if entry == "voxelize":
        out = pkg.empty_batch(N_B, R_B, dev())
        out.tsdf.fill_(float("nan"))
        got = pkg.voxelize(b.d, b.o, b.h, res=R_B, out=out)
        results.append(("float32", got.tsdf, b.plain))
        torch.cuda.synchronize()
        assert not bool(got.status.any())
        assert np.array_equal(got.max_l.cpu().numpy().view(np.uint32), np.tile(b.plain_np["max_l"], REPS).view(np.uint32))
    elif entry == "voxelize_aug":
        out = pkg.empty_batch(N_B, R_B, dev())
        out.tsdf.fill_(float("nan"))
        got = pkg.voxelize_aug(b.d, b.o, b.h, b.xf, res=R_B, out=out)
        results.append(("float32", got.tsdf, b.mapped))
        torch.cuda.synchronize()
        assert not bool(got.status.any())
        assert np.array_equal(got.max_l.cpu().numpy().view(np.uint32), np.tile(b.mapped_np["max_l"], REPS).view(np.uint32))
    elif entry == "voxelize_aug_grid":      # (the entry allocates its own output: no pre-fill)
        tsdf, st = pkg.voxelize_aug_grid(b.d, b.o, b.h, b.xf, b.arows, res=R_B)
        results.append(("float32", tsdf, b.mapped))
        torch.cuda.synchronize()
        assert not bool(st.any())
    else:
        for kind, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
            out = torch.full(shape, float("nan"), dtype=dt, device=dev())
            if entry == "voxelize_grid_lowp":
                tsdf, st = pkg.voxelize_grid_lowp(b.d, b.o, b.h, b.rows, res=R_B, dtype=dt, out=out)
                ref = b.plain
            else:
                tsdf, st = pkg.voxelize_map_grid_lowp(b.d, b.o, b.h, b.xf, b.arows, res=R_B, dtype=dt, out=out)
                ref = b.mapped
            torch.cuda.synchronize()
            assert tsdf.data_ptr() == out.data_ptr() and not bool(st.any())
            assert not _nan_left(tsdf), (entry, kind)
            assert _band_all(tsdf, ref), (entry, kind)
            ident = _copies_identical(tsdf)
            print(f"{entry} {kind}: repeated crops bit-identical: {ident}")
            record_property(f"copies_identical_{kind}", ident)
            del out, tsdf
            torch.cuda.empty_cache()
    for kind, tsdf, ref in results:
        assert tsdf.numel() > P31 and tsdf.shape == shape
        assert not _nan_left(tsdf), entry
        err = float(worst_error(tsdf, ref))
        assert err <= TOL, (entry, err)
        ident = _copies_identical(tsdf)
        print(f"{entry}: max |hip - oracle| = {err:.3g} over {N_B} positions; repeated crops bit-identical: {ident}")
        record_property("max_err", err)
        record_property("copies_identical", ident)
    report_peak(entry)
    del results
    torch.cuda.empty_cache()


N_ACC = 513                            # positions of the accurate entries' case: 171 cycles of the three sparse sources


@pytest.mark.parametrize("kind,layout", [("plain", "czyx"), ("mapped", "cxyz")], ids=["voxelize_grid_accurate", "voxelize_map_grid_accurate"])
def test_accurate_outputs_beyond_2_31(pkg, record_property, kind, layout):
    """(b) The two accurate entries at 128^3 with 513 positions cycling over the three sparse sources of
    tests/sparse_ref.py (a dense crop puts their brute-force reference out of reach at this R): the volume holds 3.2e9
    elements — position 170 crosses byte 2^32, position 341 element 2^31 — and ``nearest`` 4.30e9 bytes: its last position
    begins at byte 2^32.  Positions 0..2 against the reference under accurate_ref.compare, every later position equal to
    position i % 3 bit for bit, in chunks on the device.  One layout each: the in-volume index is the same int64 expression
    in both kernels.  Needs 17.3 GiB of outputs (12.9 GiB of volumes, 4.3 GiB of ``nearest``) and 0.7 GiB to compare."""
    need_memory(18)
    k, R3 = sp.K_RES, R_B ** 3
    cycles = N_ACC // k
    assert N_ACC == cycles * k and N_ACC * VOL > P31 and 170 * VOL * 4 < (1 << 32) < 171 * VOL * 4 and 341 * VOL < P31 < 342 * VOL
    assert (N_ACC - 1) * R3 * 4 == 1 << 32 and pr.accurate_plan(N_ACC, R_B) == (1, R_B, 0)
    t0 = time.perf_counter()
    a = accurate_sources(kind, R_B)
    t1 = time.perf_counter()
    tsdf, st, nn = accurate_launch(pkg, a, N_ACC, layout)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    assert tsdf.shape == (N_ACC, 3, R_B, R_B, R_B) and nn.shape == (N_ACC, R_B, R_B, R_B) and not bool(st.any())
    wv, wn, wf = sp.res_in_layout(a.ref, layout)
    acr.compare(tsdf[:k].cpu().numpy(), nn[:k].cpu().numpy(), wv, wn, wf, f"{kind} R={R_B} {layout} n={N_ACC}")
    v, q = tsdf.view(cycles, k * VOL).view(torch.int32), nn.view(cycles, k * R3)
    for c0 in range(1, cycles, 8):
        assert bool((v[c0:c0 + 8] == v[0]).all()), (kind, "volume", c0)
        assert bool((q[c0:c0 + 8] == q[0]).all()), (kind, "nearest", c0)
    t3 = time.perf_counter()
    print(f"{kind} {N_ACC} x {R_B}^3: reference {t1 - t0:.2f} s, launch {t2 - t1:.2f} s, comparison {t3 - t2:.2f} s")
    record_property("launch_seconds", t2 - t1)
    report_peak(f"accurate {kind}")
    del a, tsdf, st, nn, v, q
    torch.cuda.empty_cache()


# ---- (c) element streams beyond 2^31 -----------------------------------------------------------------------------------
CH = 1 << 27    # elements per comparison chunk


def _chunks(n):
    return [(c0, min(n, c0 + CH)) for c0 in range(0, n, CH)]


def test_widen_depth16_beyond_2_31(pkg):
    """(c) 2^31 + 4099 random uint16 widened with shift 3 (4 GiB in, 8 GiB out), then once more into a destination one
    float further on, so that the unaligned head path runs: equal, chunk by chunk, to float(src) * 2^-3.  Needs 14 GiB (12 GiB of
    buffers, the rest for the comparison's chunks)."""
    need_memory(14)
    n, d = N_STREAM, dev()
    gen = torch.Generator(device=d).manual_seed(16)
    src16 = torch.empty(n, dtype=torch.int16, device=d)                 # the same bits as uint16
    for c0, c1 in _chunks(n):
        src16[c0:c1] = torch.randint(-32768, 32768, (c1 - c0,), dtype=torch.int16, device=d, generator=gen)
    src = src16.view(torch.uint16)
    buf = torch.full((n + 1,), float("nan"), dtype=torch.float32, device=d)
    for shift_by in (0, 1):
        out = buf[shift_by:shift_by + n]
        got = pkg.widen_depth16(src, 3, out=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and got.numel() > P31
        for c0, c1 in _chunks(n):
            want = (src16[c0:c1].to(torch.int32) & 0xFFFF).to(torch.float32) * 2.0 ** -3
            assert torch.equal(out[c0:c1], want), (shift_by, c0)
        if shift_by == 0:
            assert bool(torch.isnan(buf[n]))                            # nothing written past the end
            buf.fill_(float("nan"))
        else:
            assert bool(torch.isnan(buf[0]))                            # nor before the start
    report_peak("widen_depth16")
    del src, src16, buf, out, got, want
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_narrow_volumes_beyond_2_31(pkg, kind):
    """(c) 2^31 + 4099 float32 narrowed (8 GiB in, 4 GiB out): equal, chunk by chunk, to torch's own cast.  Needs 13 GiB."""
    need_memory(13)
    dt = {"f16": torch.float16, "bf16": torch.bfloat16}[kind]
    n, d = N_STREAM, dev()
    gen = torch.Generator(device=d).manual_seed(17)
    src = torch.empty(n, dtype=torch.float32, device=d)
    for c0, c1 in _chunks(n):
        src[c0:c1] = torch.randn(c1 - c0, dtype=torch.float32, device=d, generator=gen)
    src *= 3.0                                                          # |v| < 1 and |v| > 1: both sides of the surface
    out = torch.full((n,), float("nan"), dtype=dt, device=d)
    got = pkg.narrow_volumes(src, dtype=dt, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.numel() > P31
    for c0, c1 in _chunks(n):
        assert torch.equal(out[c0:c1].view(torch.int16), src[c0:c1].to(dt).view(torch.int16)), (kind, c0)
    report_peak("narrow_volumes " + kind)
    del src, out, got
    torch.cuda.empty_cache()


# ---- (d) frames beyond 2^31 pixels -------------------------------------------------------------------------------------
N_FRAMES = 699060
PLACED = (0, 349525, 699051, N_FRAMES - 1)      # the 64 x 48 scenes 0..3 are written here
EMPTY = 123457                                  # an all-zero frame


@pytest.mark.parametrize("kind", ["uint16", "float32"])
def test_locate_hands_beyond_2_31_pixels(pkg, kind):
    """(d) 699,060 frames of 64 x 48: byte 2^31 of the uint16 tensor falls inside frame 349,525, frame 699,051 is the first
    entirely beyond element 2^31.  Located through the index [699051, 0, N-1, 349525, 699051]: every output row and crop
    equal, bit for bit, to those of the same four frames in a compact [4, 48, 64] tensor; one all-zero frame, added to the
    index once, has status 1.  Needs 4.1 GiB (uint16) or 8.1 GiB (float32)."""
    H, W, cam, _ = lr.SETS["64x48"]
    px = H * W
    assert N_FRAMES * px > P31 and PLACED[1] * px * 2 < P31 < (PLACED[1] + 1) * px * 2
    assert (PLACED[2] - 1) * px < P31 <= PLACED[2] * px
    need_memory(4.1 if kind == "uint16" else 8.1)
    scenes = lr.frames_of("64x48")[:4]
    if kind == "uint16":        # the scenes are exact in 1/8 mm: shift 3
        q = scenes * np.float32(8)
        assert np.array_equal(q, np.round(q)) and q.max() < 32768
        small, = up(q.astype(np.int16))
        frames = torch.zeros((N_FRAMES, H, W), dtype=torch.int16, device=dev())
        kw = dict(shift=3)
    else:
        small, = up(scenes)
        frames = torch.zeros((N_FRAMES, H, W), dtype=torch.float32, device=dev())
        kw = {}
    for j, g in enumerate(PLACED):
        frames[g] = small[j]
    if kind == "uint16":
        frames, small = frames.view(torch.uint16), small.view(torch.uint16)
    assert frames.numel() > P31
    hc = pkg.TsdfCam(*cam)
    order = [2, 0, 3, 1, 2]
    idx = torch.tensor([PLACED[j] for j in order] + [EMPTY], dtype=torch.int64, device=dev())
    big = pkg.locate_hands(frames, cam=hc, index=idx, **kw, **lr.PARAMS)
    ref = pkg.locate_hands(small, cam=hc, index=torch.tensor(order, dtype=torch.int64, device=dev()), **kw, **lr.PARAMS)
    torch.cuda.synchronize()
    assert ref.status.tolist() == [0] * 5 and big.status.tolist() == [0] * 5 + [1]
    for k in ("headers", "com", "count", "status", "grid", "max_l", "mid_p"):
        assert same(getattr(big, k)[:5], getattr(ref, k)), (kind, k)
    assert torch.equal(big.offsets[:6], ref.offsets)
    end = int(ref.offsets[5])
    assert end > 5 and same(big.depth[:end], ref.depth[:end]) and bool((ref.depth[:end] != 0).any())
    assert bool((big.count[:5] > 0).all()) and same(big.com[0], big.com[4]) and not same(big.com[0], big.com[1])
    # the all-zero frame: the empty row
    assert big.headers[5].tolist() == [W, H, 0, 0, 1, 1] and int(big.count[5]) == 0
    assert int(big.offsets[6] - big.offsets[5]) == 1 and float(big.depth[end]) == 0.0
    assert not bool(big.grid[5].any()) and float(big.max_l[5]) == 0.0
    report_peak("locate_hands " + kind)
    del frames, big, ref, small
    torch.cuda.empty_cache()
