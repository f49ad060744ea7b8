"""GPU tier of the low-precision volumes (include/tsdf_lowp.h): the narrowing on chosen bit patterns against the device's own
casts, tsdf_grid_lowp_kernel against the oracle and against the product's float32 volume, status and edge frames, the
index, independence of the batch and determinism, voxelize_lowp, process_batch(dtype=), ResidentLoader(volume_dtype=) and
capture into a graph.

The volume checks have no tolerance of their own: with o the oracle's float32 volume and TOL = 1e-5 the project's contract
figure (include/tsdf.h), the output g must satisfy (o - TOL).to(dtype) <= g <= (o + TOL).to(dtype) — rounding is monotone,
so that is exactly "g is the narrowing of some float32 within the contract of the oracle".  Against the product's own
float32 volume v (itself within TOL of the oracle) the band is 2 * TOL."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lowp_ref as lp  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-5
W, H = 320, 240
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


def dev():
    return torch.device("cuda")


def up(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev()) for a in arrays)


def concat(parts):
    """[(depth, offsets, headers), ...] -> one packed batch."""
    depth = np.concatenate([p[0] for p in parts])
    base = np.cumsum([0] + [len(p[0]) for p in parts])
    off = np.concatenate([np.asarray(p[1][:-1], np.int64) + base[k] for k, p in enumerate(parts)] + [base[-1:]])
    hdr = np.concatenate([np.asarray(p[2], np.int32).reshape(-1, 6) for p in parts])
    return depth.astype(np.float32), off.astype(np.int64), hdr


def bits(t):
    return t.contiguous().view(torch.int16)


def in_band(g, ref, tol):
    """(ref - tol).to(dtype) <= g <= (ref + tol).to(dtype), element-wise; ref float32, g the low-precision volume."""
    lo, hi = (ref - tol).to(g.dtype).float(), (ref + tol).to(g.dtype).float()
    gf = g.float()
    return bool(((lo <= gf) & (gf <= hi)).all())


@functools.lru_cache(maxsize=None)
def _frames():
    synth = importlib.import_module("handposeestimation-with-3d-cnns_amd.synth")
    crops = synth.synth_batch(10, "crop", seed0=42)
    fd, fo, fh = synth.synth_batch(12, "full", seed0=42)
    return concat([crops, (fd[:fo[2]], fo[:3], fh[:2])])


def grid_rows(depth, off, hdr, R):
    """The rows the oracle's own glue places on every frame's valid pixels: vox_ori[3], voxel_len, trunc_dis, 0, 0, 0."""
    rows = np.zeros((len(hdr), 8), np.float32)
    for i in range(len(hdr)):
        nv, mn, mx = oracle.aabb(depth[off[i]:off[i + 1]], hdr[i])
        assert nv > 0
        g, ori = oracle.glue(mn, mx, R)
        rows[i, :3], rows[i, 3], rows[i, 4] = ori, g[4], g[5]
    return rows


@functools.lru_cache(maxsize=None)
def _case(R, layout):
    """(rows, oracle volume float32[n,3,R,R,R]) of the test frames (12, or the first 2 crops at R = 64): computed once,
    shared by both dtypes, never modified."""
    depth, off, hdr = _frames()
    n = 2 if R == 64 else len(hdr)
    rows = grid_rows(depth, off, hdr, R)[:n]
    vol = np.stack([oracle.voxels(depth[off[i]:off[i + 1]], hdr[i], rows[i, :3], rows[i, 3], rows[i, 4], R=R,
                                  layout=0 if layout == "czyx" else 1) for i in range(n)])
    return rows, vol


# ---- narrowing ----
@pytest.mark.parametrize("kind", lp.KINDS)
def test_narrowing_equals_the_devices_cast_bit_for_bit(pkg, kind):
    dt = DTYPES[kind]
    x = lp.neighbourhoods(kind)
    want_ref = lp.narrow_bits(x, kind)
    tx, = up(x)
    got = pkg.narrow_volumes(tx, dtype=dt)
    torch.cuda.synchronize()
    assert got.dtype is dt and got.shape == tx.shape
    assert torch.equal(bits(got), bits(tx.to(dt)))
    assert np.array_equal(bits(got).cpu().numpy().view(np.uint16), want_ref)
    # counts that are no multiple of 8 (the element-wise tail), into a caller's buffer whose rest must stay untouched
    for count in (1, 7, 9, 1027):
        part = tx[5000:5000 + 1032][:count].clone()
        buf = torch.full((1040,), -3.0, dtype=dt, device=dev())
        r = pkg.narrow_volumes(part, dtype=dt, out=buf[:count])
        torch.cuda.synchronize()
        assert r.data_ptr() == buf.data_ptr()
        assert torch.equal(bits(buf[:count]), bits(part.to(dt))), count
        assert bool((buf[count:] == -3.0).all()), count
    # infinity stays, NaN stays a NaN, and the shape is kept
    sp = torch.tensor([[np.inf, -np.inf, np.nan], [1.0, -0.0, 3e38]], dtype=torch.float32, device=dev())
    r = pkg.narrow_volumes(sp, dtype=dt)
    assert r.shape == sp.shape and bool(torch.isnan(r[0, 2]))
    assert torch.equal(bits(r).flatten()[[0, 1, 3, 4]], bits(sp.to(dt)).flatten()[[0, 1, 3, 4]])
    assert pkg.narrow_volumes(tx[:0], dtype=dt).shape == (0,)


# ---- volumes against the oracle and against the product ----
@pytest.mark.parametrize("kind", lp.KINDS)
@pytest.mark.parametrize("layout", ["czyx", "cxyz"])
@pytest.mark.parametrize("R", [8, 12, 16, 32, 64])
def test_volumes_against_the_oracle_and_the_product(pkg, R, layout, kind):
    dt = DTYPES[kind]
    depth, off, hdr = _frames()
    rows, vol = _case(R, layout)
    n = len(rows)
    td, to, th, tr, o = up(depth[:off[n]], off[:n + 1], hdr[:n], rows, vol)
    g, st = pkg.voxelize_grid_lowp(td, to, th, tr, res=R, layout=layout, dtype=dt)
    v, vst = pkg.voxelize_grid(td, to, th, tr, res=R, layout=layout)
    torch.cuda.synchronize()
    assert g.dtype is dt and g.shape == (n, 3, R, R, R) and st.dtype is torch.int32
    assert not bool(st.any()) and not bool(vst.any())
    assert bool((o != 0).any()) and bool((o.abs() < 1).logical_and(o != 0).any())    # near voxels exist
    assert in_band(g, o, TOL)
    assert in_band(g, v, 2 * TOL)
    assert torch.equal(torch.signbit(g), torch.signbit(v))
    differ = int((bits(g) != bits(v.to(dt))).sum())
    print(f"R={R} {layout} {kind}: {differ} of {g.numel()} voxels differ from the product's volume cast")


# ---- status and edge frames ----
def test_status_and_edge_frames(pkg, synth):
    R, dt = 16, torch.bfloat16
    depth, off, hdr = synth.synth_batch(3, "crop", seed0=42)
    rows = grid_rows(depth, off, hdr, R)
    td, to, th, tr = up(depth, off, hdr, rows)
    clean, st = pkg.voxelize_grid_lowp(td, to, th, tr, res=R, dtype=dt)
    assert st.tolist() == [0, 0, 0] and all(bool(clean[i].any()) for i in range(3))
    # a bad header in the middle of the batch: its neighbours are untouched
    for edit in ("area", "empty", "payload"):
        h2 = hdr.copy()
        d2 = td
        if edit == "area":
            h2[1, 4] += 1
        elif edit == "empty":
            h2[1, 4] = h2[1, 2]
        else:
            h2, d2 = hdr[:2], td[:off[2] - 5]              # frame 1's payload ends past the buffer
        n2 = len(h2)
        out = torch.full((n2, 3, R, R, R), 7.0, dtype=dt, device=dev())
        g, st = pkg.voxelize_grid_lowp(d2, to[:n2 + 1], up(h2)[0], tr[:n2], res=R, dtype=dt, out=out)
        assert g.data_ptr() == out.data_ptr()
        assert st.tolist() == [0, 2, 0][:n2], edit
        assert not bool(bits(g[1]).any()), edit
        assert torch.equal(bits(g[0]), bits(clean[0])) and (n2 < 3 or torch.equal(bits(g[2]), bits(clean[2]))), edit
    # unusable grid rows: trunc_dis = 0, a NaN origin, an infinite voxel_len, a negative trunc_dis
    r2 = rows.copy()
    r2[0, 4] = 0.0
    r2[2, 1] = np.nan
    g, st = pkg.voxelize_grid_lowp(td, to, th, up(r2)[0], res=R, dtype=dt)
    assert st.tolist() == [1, 0, 1]
    assert not bool(bits(g[0]).any()) and not bool(bits(g[2]).any()) and torch.equal(bits(g[1]), bits(clean[1]))
    r3 = rows.copy()
    r3[0, 3] = np.inf
    r3[1, 4] = -1.0
    g, st = pkg.voxelize_grid_lowp(td, to, th, up(r3)[0], res=R, layout="cxyz", dtype=torch.float16)
    assert st.tolist() == [1, 1, 0] and not bool(bits(g[:2]).any()) and bool(g[2].any())
    # a crop of all-zero depth: nothing is scanned, so status 0 and zeros (also 0.5 and NaN are invalid pixels)
    for fill in (0.0, 0.5, np.nan):
        dz = depth.copy()
        dz[off[1]:off[2]] = fill
        g, st = pkg.voxelize_grid_lowp(up(dz)[0], to, th, tr, res=R, dtype=dt)
        assert st.tolist() == [0, 0, 0] and not bool(bits(g[1]).any())
        assert torch.equal(bits(g[0]), bits(clean[0])) and torch.equal(bits(g[2]), bits(clean[2]))
    # indices outside the source tables
    idx = torch.tensor([2, -1, 0, 3, 1], dtype=torch.int64, device=dev())
    g, st = pkg.voxelize_grid_lowp(td, to, th, tr, res=R, dtype=dt, index=idx)
    torch.cuda.synchronize()
    assert st.tolist() == [0, 2, 0, 2, 0]
    assert not bool(bits(g[1]).any()) and not bool(bits(g[3]).any())
    for k, s in ((0, 2), (2, 0), (4, 1)):
        assert torch.equal(bits(g[k]), bits(clean[s]))
    # the wrapper's own refusals, and the empty batch
    with pytest.raises(ValueError):
        pkg.voxelize_grid_lowp(td, to, th, tr[:2], res=R)
    with pytest.raises(TypeError):
        pkg.voxelize_grid_lowp(td, to, th, tr, res=R, out=torch.empty((3, 3, R, R, R), dtype=torch.float16, device=dev()))
    with pytest.raises(ValueError):
        pkg.voxelize_grid_lowp(td, to, th, tr, res=R, out=clean[:2])
    with pytest.raises(ValueError):
        pkg.voxelize_grid_lowp(td, to, th, tr, res=10)
    g, st = pkg.voxelize_grid_lowp(td, to, th, tr, res=R, index=idx[:0])
    assert g.shape == (0, 3, R, R, R) and st.shape == (0,)


# ---- index, independence of the batch, determinism ----
@pytest.mark.parametrize("R,layout,kind", [(32, "czyx", "bf16"), (12, "cxyz", "f16")])
def test_index_batch_independence_and_determinism(pkg, synth, R, layout, kind):
    dt = DTYPES[kind]
    depth, off, hdr = synth.synth_batch(10, "crop", seed0=42)
    rows = grid_rows(depth, off, hdr, R)
    td, to, th, tr = up(depth, off, hdr, rows)
    kw = dict(res=R, layout=layout, dtype=dt)
    whole, st = pkg.voxelize_grid_lowp(td, to, th, tr, **kw)
    again, _ = pkg.voxelize_grid_lowp(td, to, th, tr, **kw)
    torch.cuda.synchronize()
    assert not bool(st.any()) and torch.equal(bits(whole), bits(again))
    perm = torch.tensor([7, 3, 3, 9, 0, 1, 7, 2, 8, 4, 6, 5, 0, 9, 9, 3, 7], dtype=torch.int64, device=dev())
    g, st = pkg.voxelize_grid_lowp(td, to, th, tr, index=perm, **kw)
    torch.cuda.synchronize()
    assert g.shape[0] == 17 and not bool(st.any())
    assert torch.equal(bits(g), bits(whole[perm]))
    for i in range(10):
        alone, st = pkg.voxelize_grid_lowp(*up(depth[off[i]:off[i + 1]], np.array([0, off[i + 1] - off[i]], np.int64),
                                               hdr[i:i + 1], rows[i:i + 1]), **kw)
        assert st.tolist() == [0] and torch.equal(bits(alone[0]), bits(whole[i])), i


# ---- voxelize_lowp ----
@pytest.mark.parametrize("kind", lp.KINDS)
def test_voxelize_lowp_equals_voxelize_but_for_the_volumes_type(pkg, synth, kind):
    dt = DTYPES[kind]
    parts = [synth.synth_batch(6, "crop", seed0=42), (np.zeros(12, np.float32), np.array([0, 12], np.int64),
                                                      np.array([[W, H, 50, 60, 54, 63]], np.int32))]
    depth, off, hdr = concat(parts)
    hdr[2, 5] += 1                                            # a bad header as well
    td, to, th = up(depth, off, hdr)
    for R, layout in ((32, "czyx"), (12, "cxyz")):
        want = pkg.voxelize(td, to, th, res=R, layout=layout)
        got = pkg.voxelize_lowp(td, to, th, res=R, layout=layout, dtype=dt)
        torch.cuda.synchronize()
        assert isinstance(got, pkg.TsdfBatch) and got.tsdf.dtype is dt
        assert want.status.tolist() == [0, 0, 2, 0, 0, 0, 1]
        assert torch.equal(got.max_l, want.max_l) and torch.equal(got.mid_p, want.mid_p)
        assert torch.equal(got.status, want.status)
        assert in_band(got.tsdf, want.tsdf, 2 * TOL)
        assert not bool(bits(got.tsdf[2]).any()) and not bool(bits(got.tsdf[6]).any())


# ---- process_batch(dtype=...) ----
def test_process_batch_with_a_dtype(pkg, synth):
    depth, off, hdr = synth.synth_batch(12, "crop", seed0=42)
    td, to, th = up(depth, off, hdr)
    kw = dict(points=512, seed=5, res=12)
    want = pkg.process_batch(td, to, th, **kw)
    assert not bool(want.status.any())
    for dt in DTYPES.values():
        got = pkg.process_batch(td, to, th, dtype=dt, **kw)
        torch.cuda.synchronize()
        for name, x, y in zip(want._fields, want, got):
            if name == "tsdf":
                assert y.dtype is dt and in_band(y, x, 2 * TOL)
                assert torch.equal(torch.signbit(x), torch.signbit(y))
            else:
                assert torch.equal(x, y), name
    none = pkg.process_batch(td, to, th, dtype=None, **kw)
    for x, y in zip(want, none):
        assert x.dtype is y.dtype and torch.equal(x, y)


# ---- ResidentLoader(volume_dtype=...) ----
def _batch_tensors(b):
    return [t.clone() for t in b if t is not None]


def test_resident_loader_with_a_volume_dtype(pkg, synth):
    d, dt = dev(), torch.bfloat16
    N = 10
    depth, off, hdr = synth.synth_batch(N, "crop", seed0=9100)
    depth = depth.copy()
    depth[off[4]:off[5]] = 0.0                                # one degenerate frame: no valid pixel
    gt = np.random.default_rng(3).normal(0, 90, (N, 63)).astype(np.float32)
    ds = pkg.MSRADepthDataset.from_packs([pkg.packing.PackedFrames(depth, off, hdr, gt)])
    kw = dict(batch_size=4, device=d, shuffle=True, seed=4)
    f32 = [_batch_tensors(b) for b in pkg.ResidentLoader(ds, **kw)]
    got = {}
    for prefetch in (1, 2):
        ld = pkg.ResidentLoader(ds, prefetch=prefetch, volume_dtype=dt, **kw)
        got[prefetch] = [_batch_tensors(b) for b in ld]
        second = [_batch_tensors(b) for b in ld]              # the next epoch draws other batches from the same tables
        assert len(second) == 3 and ld._lowp[0].shape == (N, 8)
    torch.cuda.synchronize()
    assert [len(b[0]) for b in f32] == [4, 4, 2]
    names = pkg.VoxelBatch._fields
    seen = 0
    for want, a, b in zip(f32, got[1], got[2]):
        assert len(want) == len(a) == len(b) == 6
        for name, x, y, z in zip(names, want, a, b):
            assert torch.equal(bits(y) if name == "tsdf" else y, bits(z) if name == "tsdf" else z), name
            if name == "tsdf":
                assert y.dtype is dt and in_band(y, x, 2 * TOL)
            else:
                assert torch.equal(x, y), name
        deg = want[4] == 1
        seen += int(deg.sum())
        assert bool((a[5][deg] == 0.5).all()) and not bool(bits(a[0][deg]).any())
    assert seen == 1 and sum(int((w[4] != 0).sum()) for w in f32) == 1
    # the default is the loader as it is without the argument
    today = [_batch_tensors(b) for b in pkg.ResidentLoader(ds, volume_dtype=None, **kw)]
    for x, y in zip(f32, today):
        assert all(torch.equal(u, v) and u.dtype is v.dtype for u, v in zip(x, y))


# ---- graph capture ----
def test_capture_into_a_graph(pkg, synth):
    d, dt = dev(), torch.float16
    n, R = 8, 32
    depth, off, hdr = synth.synth_batch(n, "crop", seed0=42)
    rows = grid_rows(depth, off, hdr, R)
    changed = (depth * 1.03 * (depth != 0)).astype(np.float32)
    td, to, th, tr = up(depth, off, hdr, rows)
    idx = torch.tensor([3, 1, 7, 7, 0, 2], dtype=torch.int64, device=d)
    out = torch.empty((6, 3, R, R, R), dtype=dt, device=d)

    def step():
        return pkg.voxelize_grid_lowp(td, to, th, tr, res=R, dtype=dt, index=idx, out=out)

    step()                                   # eagerly once: library loads and the device check happen here
    torch.cuda.synchronize()
    first = out.clone()
    side = torch.cuda.Stream(d)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _, st = step()
    td.copy_(torch.from_numpy(changed))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    have, have_st = out.clone(), st.clone()
    eager, eager_st = pkg.voxelize_grid_lowp(td, to, th, tr, res=R, dtype=dt, index=idx)
    torch.cuda.synchronize()
    assert torch.equal(bits(have), bits(eager)) and torch.equal(have_st, eager_st)
    assert not torch.equal(bits(have), bits(first))           # the depth did change the volumes
