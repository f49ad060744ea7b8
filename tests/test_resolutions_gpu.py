"""GPU tier: every kernel that takes a resolution, at ALL 32 of them (multiples of 4 from 4 to 128), against the oracle.

One parametrized case is one R with both layouts.  The six source frames, their maps and the batch sizes come from
tests/plan_ref.py, whose CPU tier (tests/test_resolutions_cpu.py) shows which branches of split_plan, of the voxel pass and
of slab_plan the list reaches and that every oracle volume used here holds rejected voxels and voxels near the surface.
Every position of every batch is compared (on the device) with the oracle's result for its source: volumes within the
contract's 1e-5 (include/tsdf.h), max_l / mid_p / status bit for bit, pixel maps equal, 16-bit volumes by the in_band rule
of tests/test_lowp_gpu.py, grid rows bit for bit with their restatements.

The entries, each called below: voxelize, voxelize_aug (the product kernels), voxel_pixels, voxelize_grid,
voxelize_aug_grid, voxelize_grid_lowp, voxelize_map_grid_lowp, map_grids, map_step_head, cloud_grids, locate_hands(res=R),
and the two accurate entries voxelize_grid_accurate and voxelize_map_grid_accurate.  The accurate ones have a reference of
their own, brute force over (voxel, valid pixel) pairs, which a dense crop puts out of reach at R = 128: they run on the
three sparse sources of tests/sparse_ref.py, one parametrized case per (R, kernel), at the batch sizes of
``plan_ref.accurate_batch_sizes`` (their halving loop's regimes), under ``accurate_ref.compare``."""
import ctypes
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
import cloud_grid_ref as cg  # noqa: E402
import locate_ref as lr  # noqa: E402
import plan_ref as pr  # noqa: E402
import sparse_ref as sp  # noqa: E402
from test_lowp_gpu import in_band  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-5                      # include/tsdf.h: per-voxel bound against the oracle, plain and augmented
LAYOUTS = ("czyx", "cxyz")
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
CHUNK_BYTES = 1 << 30           # the device comparison's temporaries stay below this


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def up(*arrays):
    return tuple(torch.from_numpy(np.array(a, order="C")).to(dev()) for a in arrays)    # (a copy: the shared inputs are read-only)


def fbits(t):
    return t.contiguous().view(torch.int32)


def cu_count():
    return torch.cuda.get_device_properties(dev()).multi_processor_count


def cycle(t, n):
    """Rows of t (one per source) cycled to n positions."""
    k = t.shape[0]
    return t.repeat((n + k - 1) // k, *([1] * (t.dim() - 1)))[:n].contiguous()


def worst_error(vol, ref):
    """max |vol[i] - ref[i % k]| over every position i, on the device (a NaN anywhere comes out as NaN): the positions as
    whole cycles [cycles, k, ...] against ref broadcast, then the remainder positions against ref's first rows."""
    n, k = vol.shape[0], ref.shape[0]
    full, rem = divmod(n, k)
    worst = torch.zeros((), dtype=torch.float32, device=vol.device)
    step = max(1, CHUNK_BYTES // (ref.numel() * 4))
    for c0 in range(0, full, step):
        c1 = min(full, c0 + step)
        blk = vol[c0 * k:c1 * k].view(c1 - c0, k, *ref.shape[1:])
        worst = torch.maximum(worst, (blk - ref).abs_().amax())
    if rem:
        worst = torch.maximum(worst, (vol[full * k:] - ref[:rem]).abs_().amax())
    return worst


@pytest.fixture(scope="module")
def src():
    """The six sources and their maps on the device, once."""
    depth, off, hdr = pr.sources()
    xf = pr.source_maps()
    t = up(depth, off, hdr, xf)
    yield types.SimpleNamespace(depth=t[0], off=t[1], hdr=t[2], xf=t[3])
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", params=pr.RES, ids=lambda R: "R%d" % R)
def case(request):
    """The oracle's results of the six sources at one R: per layout the plain and the mapped volumes (uploaded once, never
    modified), the placement, and the grid rows of both placements.  Module-scoped and parametrized: every test of this file
    runs at one R before the next R is computed."""
    R = request.param
    depth, off, hdr = pr.sources()
    xf = pr.source_maps()
    c = types.SimpleNamespace(R=R, plain={}, mapped={})
    for lay, layout in enumerate(LAYOUTS):
        p = oracle.voxelize(depth, off, hdr, R=R, layout=lay, n_threads=6, extras=True)
        m = oracle.voxelize_aug(depth, off, hdr, xf, R=R, layout=lay, n_threads=6)
        assert not p["status"].any() and not m["status"].any()
        for store, res in ((c.plain, p), (c.mapped, m)):
            store[layout] = types.SimpleNamespace(tsdf=up(res["tsdf"])[0], max_l=up(res["max_l"])[0], mid_p=up(res["mid_p"])[0],
                                                  status=up(res["status"])[0])
        if lay == 0:
            c.extras = p
            rows = np.zeros((pr.N_SRC, 8), np.float32)
            rows[:, :3], rows[:, 3], rows[:, 4] = p["ori"], p["grid"][:, 4], p["grid"][:, 5]
            c.rows = rows
            c.mapped_np = m
    c.arows, c.amax_l, c.amid_p = ar.pixel_grids(depth, off, hdr, xf, R)
    yield c
    del c
    torch.cuda.empty_cache()


def check_batch(got, ref, n, what):
    """A TsdfBatch of n cycled positions against the oracle's six: status, max_l, mid_p on the bits, every volume within
    TOL, no NaN left.  Returns the largest error."""
    torch.cuda.synchronize()
    assert torch.equal(got.status, cycle(ref.status, n)), what
    assert torch.equal(fbits(got.max_l), fbits(cycle(ref.max_l, n))), what
    assert torch.equal(fbits(got.mid_p), fbits(cycle(ref.mid_p, n))), what
    err = float(worst_error(got.tsdf, ref.tsdf))
    assert not bool(torch.isnan(got.tsdf).any()), what
    assert err <= TOL, (what, err)
    return err


def test_product_entries_at_every_batch_size(pkg, src, case):
    """voxelize and voxelize_aug: n in {1, 3, 40, C/2} (the split kernel where split_plan splits), C/2 + 4 (the fused kernel
    dealing by position) and the queue-driven size (work queue; tail help among R < 48), both layouts.  The library must
    say it launches what plan_ref predicts, and every position must come out as the oracle's volume of its source."""
    R, C = case.R, cu_count()
    L = pkg._lib.load()
    buf = ctypes.create_string_buffer(160)
    worst = {"plain": 0.0, "mapped": 0.0}
    named = set()
    for n, kind in pr.batch_sizes(C, R):
        d, o, h = up(*pr.cycled(n))
        xf = cycle(src.xf, n)
        # the volumes end inside a larger buffer: a slice written past the last position lands in the guard
        vol, guard = n * 3 * R ** 3, 16 * R * R
        flat = torch.empty(vol + guard, dtype=torch.float32, device=dev())
        out = pkg.TsdfBatch(flat[:vol].view(n, 3, R, R, R), torch.empty(n, device=dev()), torch.empty((n, 3), device=dev()),
                            torch.empty(n, dtype=torch.int32, device=dev()))
        for lay, layout in enumerate(LAYOUTS):
            for aug, name in ((0, "plain"), (1, "mapped")):
                what = (R, n, kind, layout, name)
                assert L.tsdf_describe_launch(n, R, lay, aug, buf, 160) == 0
                assert buf.value.decode() == pr.describe(n, R, lay, aug, C), what
                named.add(buf.value.decode().split("<")[0])
                for t in (flat, out.max_l, out.mid_p):
                    t.fill_(float("nan"))
                out.status.fill_(-7)
                if aug:
                    got = pkg.voxelize_aug(d, o, h, xf, res=R, layout=layout, out=out)
                else:
                    got = pkg.voxelize(d, o, h, res=R, layout=layout, out=out)
                assert got.tsdf.data_ptr() == out.tsdf.data_ptr()
                ref = (case.mapped if aug else case.plain)[layout]
                worst[name] = max(worst[name], check_batch(got, ref, n, what))
                assert bool(torch.isnan(flat[vol:]).all()), what
        del out, got, flat, d, o, h, xf
        torch.cuda.empty_cache()
    assert "tsdf_fused_kernel" in named and (("tsdf_split_kernel" in named) == any(
        pr.split_plan(n, R, C)[0] for n, _ in pr.batch_sizes(C, R)))
    print(f"R={R}: max |hip - oracle| plain {worst['plain']:.3g}, mapped {worst['mapped']:.3g}")


def test_pixel_maps_equal_the_oracles(pkg, src, case):
    """voxel_pixels (the DBG instantiation) at n = 6, both layouts: the pixel every voxel gathers equals the oracle's."""
    R = case.R
    depth, off, hdr = pr.sources()
    want = [oracle.voxels(depth[off[i]:off[i + 1]], hdr[i], case.rows[i, :3], case.rows[i, 3], case.rows[i, 4], R=R,
                          want_pixmap=True)[1] for i in range(pr.N_SRC)]
    want, = up(np.stack(want))
    assert bool((want >= 0).any()) and bool((want < 0).any())
    for layout in LAYOUTS:
        t, pm, st = pkg.voxel_pixels(src.depth, src.off, src.hdr, res=R, layout=layout)
        torch.cuda.synchronize()
        assert not bool(st.any()), (R, layout)
        assert torch.equal(pm, want), (R, layout, int((pm != want).sum()))
        err = float(worst_error(t, case.plain[layout].tsdf))
        assert err <= TOL, (R, layout, err)


def test_slab_kernels_on_the_oracles_rows(pkg, src, case):
    """voxelize_grid, voxelize_aug_grid, voxelize_grid_lowp and voxelize_map_grid_lowp (float16 and bfloat16) at n = 6 on
    the rows the oracle's glue places: float32 volumes within TOL of the oracle, 16-bit ones inside the band of the
    narrowed contract; every status 0; nothing left of a NaN pre-fill where the entry takes ``out=``."""
    R = case.R
    rows, arows = up(case.rows, case.arows)
    n = pr.N_SRC
    report = []
    for layout in LAYOUTS:
        o, oa = case.plain[layout].tsdf, case.mapped[layout].tsdf
        v, st = pkg.voxelize_grid(src.depth, src.off, src.hdr, rows, res=R, layout=layout)
        va, sta = pkg.voxelize_aug_grid(src.depth, src.off, src.hdr, src.xf, arows, res=R, layout=layout)
        torch.cuda.synchronize()
        assert not bool(st.any()) and not bool(sta.any()), (R, layout)
        e, ea = float(worst_error(v, o)), float(worst_error(va, oa))
        assert e <= TOL and ea <= TOL, (R, layout, e, ea)
        report.append(f"{layout}: grid {e:.3g}, aug_grid {ea:.3g}")
        for kind, dt in DTYPES.items():
            out = torch.full((n, 3, R, R, R), float("nan"), dtype=dt, device=dev())
            g, gst = pkg.voxelize_grid_lowp(src.depth, src.off, src.hdr, rows, res=R, layout=layout, dtype=dt, out=out)
            outm = torch.full((n, 3, R, R, R), float("nan"), dtype=dt, device=dev())
            gm, gmst = pkg.voxelize_map_grid_lowp(src.depth, src.off, src.hdr, src.xf, arows, res=R, layout=layout, dtype=dt,
                                                  out=outm)
            torch.cuda.synchronize()
            assert g.data_ptr() == out.data_ptr() and gm.data_ptr() == outm.data_ptr()
            assert not bool(gst.any()) and not bool(gmst.any()), (R, layout, kind)
            assert not bool(torch.isnan(g).any()) and not bool(torch.isnan(gm).any()), (R, layout, kind)
            assert in_band(g, o, TOL), (R, layout, kind, "voxelize_grid_lowp")
            assert in_band(gm, oa, TOL), (R, layout, kind, "voxelize_map_grid_lowp")
            assert in_band(g, v, 2 * TOL) and in_band(gm, va, 2 * TOL), (R, layout, kind)
    print(f"R={R}: max |hip - oracle| " + "; ".join(report))


def test_grid_rows_equal_their_restatements(pkg, src, case):
    """The rows map_grids, map_step_head, cloud_grids and locate_hands(res=R) write, bit for bit: the oracle's placement
    under the maps (tests/auggrid_ref.py::pixel_grids), the numpy cloud glue (tests/cloud_grid_ref.py) and the cube glue
    (tests/locate_ref.py::glue_cube)."""
    R = case.R
    depth, off, hdr = pr.sources()

    def same_rows(got, rows, max_l, mid_p, what):
        assert not bool(got.status.any()), what
        assert np.array_equal(got.grid.cpu().numpy().view(np.uint32), rows.view(np.uint32)), what
        assert np.array_equal(got.max_l.cpu().numpy().view(np.uint32), max_l.view(np.uint32)), what
        assert np.array_equal(got.mid_p.cpu().numpy().view(np.uint32), mid_p.view(np.uint32)), what

    mg = pkg.map_grids(src.depth, src.off, src.hdr, src.xf, res=R)
    torch.cuda.synchronize()
    same_rows(mg, case.arows, case.amax_l, case.amid_p, (R, "map_grids"))
    assert np.array_equal(case.amax_l.view(np.uint32), case.mapped_np["max_l"].view(np.uint32))
    # the step head: its own draw about every source's plain centre, placed under the maps it reports
    centres, = up(case.extras["mid_p"])
    head = pkg.map_step_head(src.depth, src.off, src.hdr, centres, pkg.aug_state(0x5EED + R, 3, device=dev()), res=R)
    torch.cuda.synchronize()
    T = head.xforms.cpu().numpy()
    assert np.isfinite(T).all() and not np.array_equal(T, pkg.augment.identity_affines(pr.N_SRC))
    same_rows(head, *ar.pixel_grids(depth, off, hdr, T, R), (R, "map_step_head"))
    # the cloud's placement
    pc = pkg.point_clouds(src.depth, src.off, src.hdr, points=1000, seed=R)
    got = pkg.cloud_grids(pc.points, res=R)
    torch.cuda.synchronize()
    assert not bool(pc.status.any())
    want = cg.cloud_grids(pc.points.cpu().numpy(), R=R)
    for name, w in zip(("grid", "max_l", "mid_p", "aabb", "status"), want):
        assert cg.same_values(getattr(got, name).cpu().numpy(), w) if name != "status" else \
            np.array_equal(got.status.cpu().numpy(), w), (R, "cloud_grids", name)
    assert not want[4].any() and (want[1] > 0).all()
    # the located cube's rows
    H, W, cam, _ = lr.SETS["64x48"]
    frames = lr.frames_of("64x48")
    crops = pkg.locate_hands(up(frames)[0], cam=pkg.TsdfCam(*cam), res=R, **lr.PARAMS)
    torch.cuda.synchronize()
    assert not bool(crops.status.any())
    com = crops.com.cpu().numpy()
    grid, max_l, mid_p = (getattr(crops, k).cpu().numpy() for k in ("grid", "max_l", "mid_p"))
    for i in range(len(frames)):
        wg, wl, wm = lr.glue_cube(com[i], lr.PARAMS["cube"], R, cam[4])
        assert np.array_equal(grid[i].view(np.uint32), wg.view(np.uint32)), (R, "locate_hands", i)
        assert max_l[i].view(np.uint32) == np.float32(wl).view(np.uint32), (R, "locate_hands", i)
        assert np.array_equal(mid_p[i].view(np.uint32), wm.view(np.uint32)), (R, "locate_hands", i)


# ---- the two accurate entries ----
def accurate_sources(kind, R):
    """The three sparse sources of tests/sparse_ref.py on the device with their rows (and maps) at R, and their brute-force
    references (numpy, indexed [z][y][x])."""
    s = sp.res_sources(kind, R)
    depth, off, hdr = sp.res_pack()
    t = up(depth, off, hdr, s["grid"], sp.res_xforms())
    return types.SimpleNamespace(kind=kind, R=R, ref=s, depth=t[0], off=t[1], hdr=t[2], grid=t[3], xf=t[4])


def accurate_launch(pkg, a, n, layout):
    """n positions cycling over the three sources (position i holds source i % 3) -> (tsdf, status, nearest)."""
    idx = torch.arange(n, dtype=torch.int64, device=dev()) % sp.K_RES
    if a.kind == "plain":       # rows of SOURCES
        return pkg.voxelize_grid_accurate(a.depth, a.off, a.hdr, a.grid, res=a.R, layout=layout, index=idx, nearest=True)
    return pkg.voxelize_map_grid_accurate(a.depth, a.off, a.hdr, cycle(a.xf, n), cycle(a.grid, n), res=a.R, layout=layout,
                                          index=idx, nearest=True)      # maps and rows of POSITIONS


@pytest.mark.parametrize("kind", ["plain", "mapped"])
@pytest.mark.parametrize("R", pr.RES, ids=lambda R: "R%d" % R)
def test_accurate_entries_at_every_resolution(pkg, R, kind):
    """voxelize_grid_accurate / voxelize_map_grid_accurate (three maps, one of them ``general``) at n = 1, at the smallest n
    at which their slab is halved once less than at n = 1 (where R has such a state: R <= 28) and at the smallest n at which
    it is not halved at all, both layouts.  Positions 0..2 against the brute-force reference under accurate_ref.compare; every
    later position equal to position i % 3 bit for bit in volume, ``nearest`` and status, and position 0 the same bits in
    every launch: a voxel's bits depend on neither its slab nor its batch position."""
    t0 = time.perf_counter()
    a = accurate_sources(kind, R)
    t_ref = time.perf_counter() - t0
    k = sp.K_RES
    for layout in LAYOUTS:
        wv, wn, wf = sp.res_in_layout(a.ref, layout)
        first = None
        for n, regime in pr.accurate_batch_sizes(R):
            tsdf, st, nn = accurate_launch(pkg, a, n, layout)
            torch.cuda.synchronize()
            what = (kind, R, layout, n, regime, pr.accurate_plan(n, R))
            assert tsdf.shape == (n, 3, R, R, R) and nn.shape == (n, R, R, R) and not bool(st.any()), what
            m = min(n, k)
            acr.compare(tsdf[:m].cpu().numpy(), nn[:m].cpu().numpy(), wv[:m], wn[:m], wf[:m],
                        f"{kind} R={R} {layout} n={n} ({regime}: slab {what[5][0]})")
            if n > k:
                assert torch.equal(fbits(tsdf), fbits(cycle(tsdf[:k], n))) and torch.equal(nn, cycle(nn[:k], n)), what
            if first is None:
                first = (tsdf[0].clone(), nn[0].clone())
            else:
                assert torch.equal(fbits(tsdf[0]), fbits(first[0])) and torch.equal(nn[0], first[1]), what
            del tsdf, st, nn
    print(f"{kind} R={R}: {time.perf_counter() - t0:.2f} s in all, {t_ref:.2f} s of it the reference")
    torch.cuda.empty_cache()
