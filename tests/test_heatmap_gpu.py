"""GPU tier of the voxel heatmap labels (include/tsdf_heatmap.h): tsdf_heat_encode_kernel against the numpy restatement
(tests/heatmap_ref.py) on every voxel, at every resolution class, plan shape, layout and dtype; tsdf_heat_decode_kernel
against the same restatement on uploaded values — argmax, ties, NaNs, window clipping, fallback —; the round trip; graph
capture of both; AugmentedStep(heatmap=...).

Bounds.  Encode, float32: |got - ref| <= 2^-23 ref + 2^-125 — one float32 ulp, all that two float64 exp correct to 1 ulp can
differ by after the one rounding to float32, plus the width of the flush threshold for a product that straddles it.  The
2-byte outputs are the float32 output narrowed, bit for bit.  Decode: arg, peak and the radius-0 u are exact; with a radius
the float64 sums differ by their order (about 1e-13) before one rounding to a float32 in [0, 1]: 2^-23."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heatmap_ref as hr  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAN = float("nan")
SHAPES = [(1, 1), (3, 21), (17, 5), (2, 170)]
CASES = [(R, n, J) for R in (4, 8, 12, 20, 32, 44, 64) for n, J in SHAPES] + [(128, 1, 2)]
COMBOS = [(layout, sigma) for sigma in (0.5, 1.7, 4.0) for layout in hr.LAYOUTS]
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def dev():
    return torch.device("cuda:0")


def test_the_cases_reach_every_plan_shape_and_item_class():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    shapes = {hr.plan_class(n * J, R, cus) for R, n, J in CASES}
    print(f"{cus} CUs: plan shapes {sorted(shapes)}")
    assert shapes == {"one", "equal", "ragged"}
    assert {R % 8 == 0 for R, _, _ in CASES} == {False, True}            # both 2-byte item classes


def centre_u(R):
    """A label that sits on a voxel centre exactly: c = u R - 0.5 is a whole number in float64."""
    return 0.125 if R % 8 else (R // 2 - 0.5) / R


def labels(R, n, J, k):
    """float32[n,J,3] labels and int32[n] statuses: interior points, then the special joints from the front (all of them
    where the batch holds them; one of them, in turn, in a batch of one joint), in frames whose status is 0."""
    rng = np.random.default_rng(1000 + k)
    u = rng.uniform(0.05, 0.95, size=(n * J, 3)).astype(np.float32)
    cu = centre_u(R)
    special = [(cu, cu, cu),                       # an exact voxel centre
               (0.25, cu, 0.75),                   # exact half-voxel ties on x and z: c = R/4 - 0.5, 3R/4 - 0.5
               (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 1.0, 0.5),
               (-0.3, 0.5, 0.5), (1.4, 0.2, 0.9),  # outside the cube: valid, the tail
               (50.0, 0.5, 0.5),                   # far outside: all zero by the flush rule, valid
               (NAN, 0.5, 0.5), (0.5, float("inf"), 0.5), (0.5, 0.5, float("-inf"))]
    if n * J == 1:
        u[0] = special[k % len(special)]
    else:
        m = min(len(special), n * J)
        u[:m] = np.float32(special[:m])
    status = np.zeros(n, np.int32)
    if n == 2:
        status[1] = 1
    elif n == 3:
        status[1:] = (1, 2)
    elif n > 3:
        status[5], status[11] = 1, 2
    u = u.reshape(n, J, 3)
    c = u.astype(np.float64) * R - 0.5
    assert n * J == 1 or (c[0, 0] == np.rint(c[0, 0])).all()
    assert n * J == 1 or ((c[0, 1, [0, 2]] % 1) == 0.5).all()
    return u, status


def guarded(shape, dtype, fill=NAN):
    """A prefilled buffer with a guard of 64 elements after the end: ``(out, guard)``."""
    count = int(np.prod(shape))
    buf = torch.full((count + 64,), fill, dtype=dtype, device=dev())
    return buf[:count].view(shape), buf[count:]


def intact(guard, fill=NAN):
    return bool(torch.isnan(guard).all()) if fill != fill else bool((guard == fill).all())


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def within(got, ref):
    """Every voxel of a float32 volume within 2^-23 ref + 2^-125 of the restatement (float64 on the GPU)."""
    g, r = got.double(), ref.double()
    bad = (g - r).abs() > 2.0 ** -23 * r + 2.0 ** -125
    return not bool(bad.any()) and not bool(torch.isnan(got).any())


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"R{R}-n{n}-J{J}" for R, n, J in CASES])
def test_encode_every_voxel_against_the_restatement(pkg, k):
    R, n, J = CASES[k]
    u, status = labels(R, n, J, k)
    tu, ts = torch.from_numpy(u).to(dev()), torch.from_numpy(status).to(dev())
    for layout, sigma in COMBOS:
        ref, ref_valid = hr.encode(u, status, R, sigma, layout)
        out, guard = guarded((n, J, R, R, R), torch.float32)
        got, valid = pkg.joint_heatmaps(tu.reshape(n, 3 * J), R, sigma, layout=layout, status=ts, out=out, return_valid=True)
        torch.cuda.synchronize()
        assert got is out and intact(guard)
        tref = torch.from_numpy(ref).to(dev())
        worst = float(((got.double() - tref.double()).abs() / tref.double().clamp_min(2.0 ** -100)).max()) * 2.0 ** 23
        print(f"R={R} n={n} J={J} {layout} sigma={sigma}: worst {worst:.3f} ulp, {int((got != tref).sum())} voxels differ, "
              f"peak {float(got.max()):.6f}")
        assert within(got, tref)
        assert np.array_equal(valid.cpu().numpy(), ref_valid) and valid.dtype is torch.int32
        bad = torch.from_numpy(ref_valid == 0).to(dev())
        assert not bool(bits(got[bad]).any())                       # +0 in every voxel of an invalid joint
        if n * J > 1:
            assert float(got[0, 0].max()) == 1.0                    # the joint on a voxel centre: the peak is 1
            assert int((got[0, 1] == got[0, 1].max()).sum()) == 4   # ties on two axes: four maximal voxels
        if n * J >= 8:
            assert not bool(got.reshape(n * J, -1)[7].any()) and ref_valid.reshape(-1)[7] == 1   # u = 50: flushed, valid
        # the 2-byte outputs are this volume narrowed, bit for bit
        for dt in DTYPES[1:]:
            low, lguard = guarded((n, J, R, R, R), dt)
            pkg.joint_heatmaps(tu, R, sigma, layout=layout, dtype=dt, status=ts, out=low)
            torch.cuda.synchronize()
            assert intact(lguard) and torch.equal(low, got.to(dt)), dt
        # without a status every frame counts; a frame alone gives the bits it has in the batch; two calls give the same bits
        i = n - 1 if status[n - 1] == 0 else 0
        alone = pkg.joint_heatmaps(tu[i:i + 1].contiguous(), R, sigma, layout=layout)
        again = pkg.joint_heatmaps(tu, R, sigma, layout=layout, status=ts)
        free, fvalid = pkg.joint_heatmaps(tu, R, sigma, layout=layout, return_valid=True)
        torch.cuda.synchronize()
        assert torch.equal(bits(alone[0]), bits(got[i])) and torch.equal(bits(again), bits(got))
        assert np.array_equal(fvalid.cpu().numpy(), np.isfinite(u).all(axis=2).astype(np.int32))
        ok = torch.from_numpy(status == 0).to(dev())
        assert torch.equal(bits(free[ok]), bits(got[ok]))
        if (status != 0).any():
            assert bool(free[~ok].any())


def planted(R, n, J, k):
    """Standard-normal float32 volumes with, volume by volume in turn: nothing; a duplicated maximum; the maximum at the last
    element; at each of the eight corners; sprinkled NaN and -inf; NaN alone; a constant; negative values alone."""
    rng = np.random.default_rng(2000 + k)
    v = rng.standard_normal(size=(n * J, R, R, R), dtype=np.float32)
    kinds = []
    for q in range(n * J):
        kind = (q + k) % 15 if n * J > 1 else k % 15
        kinds.append(kind)
        x = v[q]
        flat = x.reshape(-1)
        if kind == 1:
            a, b = sorted(rng.choice(R ** 3, 2, replace=False))
            flat[a] = flat[b] = 9.0
        elif kind == 2:
            flat[-1] = 9.0
        elif 3 <= kind <= 10:
            c = kind - 3
            x[(R - 1) * (c & 1), (R - 1) * ((c >> 1) & 1), (R - 1) * ((c >> 2) & 1)] = 9.0
        elif kind == 11:
            flat[rng.random(R ** 3) < 0.05] = np.nan
            flat[rng.random(R ** 3) < 0.05] = -np.inf
        elif kind == 12:
            flat[:] = np.nan
        elif kind == 13:
            flat[:] = 0.25
        elif kind == 14:
            flat[:] = -np.abs(flat) - 1.0
    return v.reshape(n, J, R, R, R), np.array(kinds).reshape(n, J)


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"R{R}-n{n}-J{J}" for R, n, J in CASES])
def test_decode_against_the_restatement_on_the_same_values(pkg, k):
    R, n, J = CASES[k]
    v32, kinds = planted(R, n, J, k)
    host = torch.from_numpy(v32)
    for dt in DTYPES:
        h = host.to(dt)                                   # narrowed on the host: the GPU and the restatement read the same values
        seen = h.float().numpy()
        found = hr.peaks(seen)
        d = h.to(dev())
        rp, ra = found
        assert (ra[kinds == 12] == -1).all() and (ra[kinds == 13] == 0).all() and (ra[kinds == 2] == R ** 3 - 1).all()
        assert (rp[kinds == 14] < 0).all()
        for layout in hr.LAYOUTS:
            for radius in range(4):
                ru, _, _ = hr.decode(seen, R, layout, radius, found)
                outs = [guarded((n, J, 3), torch.float32), guarded((n, J), torch.float32), guarded((n, J), torch.int32, -7)]
                got = pkg.heatmap_joints(d, layout=layout, radius=radius, out=pkg.HeatmapJoints(*[o for o, _ in outs]))
                torch.cuda.synchronize()
                assert intact(outs[0][1]) and intact(outs[1][1]) and intact(outs[2][1], -7)
                gu, gp, ga = got.u.cpu().numpy(), got.peak.cpu().numpy(), got.arg.cpu().numpy()
                assert np.array_equal(ga, ra), (dt, layout, radius)
                assert np.array_equal(gp.view(np.int32)[ra >= 0], rp.view(np.int32)[ra >= 0]) and np.isnan(gp[ra < 0]).all()
                assert not np.isnan(gu).any()
                if radius == 0:
                    assert np.array_equal(gu, ru), (dt, layout)
                else:
                    err = float(np.abs(gu.astype(np.float64) - ru).max())
                    assert err <= 2.0 ** -23, (dt, layout, radius, err)
                    low = kinds == 14                      # negative values alone: the argmax voxel's centre
                    assert np.array_equal(gu[low], hr.decode(seen, R, layout, 0, found)[0][low])
        if dt is torch.float32:                            # without the optional outputs
            only = pkg.heatmap_joints(d, radius=2)
            torch.cuda.synchronize()
            assert only.u.shape == (n, J, 3) and only.peak.shape == (n, J) and only.arg.dtype is torch.int32


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"R{R}-n{n}-J{J}" for R, n, J in CASES])
def test_round_trip_lands_within_half_a_voxel(pkg, k):
    """decode(radius 0) of the encoder's own output.  The nearest voxel is within half a voxel of c; two voxels whose float32
    values tie or swap within one ulp lie within 2^-22 sigma^2 voxels of equidistant; the division by R and the rounding of
    u follow: |u_dec - u| <= (0.5 + 2^-20 max(1, sigma^2)) / R + 2^-23 per axis."""
    R, n, J = CASES[k]
    u, status = labels(R, n, J, k)
    tu = torch.from_numpy(u).to(dev())
    for layout, sigma in COMBOS:
        for dt in DTYPES:
            heat, valid = pkg.joint_heatmaps(tu, R, sigma, layout=layout, dtype=dt, return_valid=True)
            back = pkg.heatmap_joints(heat, layout=layout)
            torch.cuda.synchronize()
            c = u.astype(np.float64) * R - 0.5
            inside = ((c >= -0.5) & (c <= R - 0.5)).all(axis=2) & (valid.cpu().numpy() == 1)
            err = np.abs(back.u.cpu().numpy().astype(np.float64) - u.astype(np.float64))[inside]
            if dt is torch.float32:
                bound = (0.5 + 2.0 ** -20 * max(1.0, sigma * sigma)) / R + 2.0 ** -23
                assert inside.sum() == 0 or err.max() <= bound, (layout, sigma, err.max(), bound)
            assert (back.arg.cpu().numpy()[inside] >= 0).all() and (back.peak.cpu().numpy()[inside] > 0).all()


def test_both_entries_are_captured_and_replayed(pkg):
    n, J, R = 3, 21, 12
    rng = np.random.default_rng(3)
    gt = torch.from_numpy(rng.uniform(0, 1, (n, J, 3)).astype(np.float32)).to(dev())
    st = torch.zeros(n, dtype=torch.int32, device=dev())
    heat = torch.empty((n, J, R, R, R), dtype=torch.bfloat16, device=dev())
    valid_u = pkg.HeatmapJoints(torch.empty((n, J, 3), device=dev()), torch.empty((n, J), device=dev()),
                                torch.empty((n, J), dtype=torch.int32, device=dev()))

    def run():
        pkg.joint_heatmaps(gt, R, 1.0, layout="cxyz", dtype=torch.bfloat16, status=st, out=heat)
        pkg.heatmap_joints(heat, layout="cxyz", radius=1, out=valid_u)

    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev())):
        run()
    for seed in (4, 5):
        new = torch.from_numpy(np.random.default_rng(seed).uniform(0, 1, (n, J, 3)).astype(np.float32)).to(dev())
        gt.copy_(new)
        st.copy_(torch.tensor([0, seed % 2, 0], dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        replayed = (heat.clone(), *[t.clone() for t in valid_u])
        eager_heat = pkg.joint_heatmaps(new, R, 1.0, layout="cxyz", dtype=torch.bfloat16, status=st)
        eager = pkg.heatmap_joints(eager_heat, layout="cxyz", radius=1)
        torch.cuda.synchronize()
        assert torch.equal(bits(replayed[0]), bits(eager_heat)) and bool(eager_heat.any())
        for x, y in zip(replayed[1:], eager):
            assert torch.equal(x, y)


@pytest.mark.parametrize("dtype", [None, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_augmented_step_writes_the_heatmaps_of_its_labels(pkg, dtype, graph):
    synth = importlib.import_module(pkg.__name__ + ".synth")
    n, R, J = 3, 16, 21
    depth, off, hdr = synth.synth_batch(5, "crop", seed0=77)
    depth = depth.copy()
    depth[off[4]:off[5]] = 0                      # a frame without a valid pixel: status 1, zero heatmaps
    td, to, th = (torch.from_numpy(x).to(dev()) for x in (depth, off, hdr))
    mid_p = pkg.voxelize(td, to, th, res=R).mid_p          # joints scattered about every frame's grid centre
    noise = torch.from_numpy(np.random.default_rng(9).normal(0, 40, (5, J, 3)).astype(np.float32)).to(dev())
    gt = (mid_p[:, None, :] + noise).reshape(5, 3 * J).contiguous()
    kw = dict(gt=gt, res=R, graph=graph, dtype=dtype)
    with_h = pkg.AugmentedStep(td, to, th, n, heatmap=(44, 1.7), **kw)
    without = pkg.AugmentedStep(td, to, th, n, **kw)
    assert with_h.heat.shape == (n, J, 44, 44, 44) and with_h.heat.dtype is torch.float32 and without.heat is None
    assert (with_h.graph is not None) == graph
    for index, key, c0 in (([0, 4, 2], 0xBEEF, 0), ([3, 1, 4], 0xBEEF, 3), ([2, 2, 0], 7, 1 << 33)):
        a = with_h.step(index, key, c0)
        b = without.step(index, key, c0)
        torch.cuda.synchronize()
        assert len(a) == len(b) == 3
        for x, y in zip((*a[0], a[1], a[2]), (*b[0], b[1], b[2])):
            assert x.dtype is y.dtype and torch.equal(bits(x), bits(y))
        out, nor, _ = a
        want = pkg.joint_heatmaps(nor, 44, 1.7, status=out.status)
        torch.cuda.synchronize()
        assert torch.equal(bits(with_h.heat), bits(want))
        assert out.status.tolist() == [1 if i == 4 else 0 for i in index]
        for i, f in enumerate(index):
            assert bool(with_h.heat[i].any()) == (f != 4)
    low = pkg.AugmentedStep(td, to, th, n, heatmap=(12, 0.5, torch.float16), layout="cxyz", **kw)
    out, nor, _ = low.step([1, 0, 3], 5, 0)
    torch.cuda.synchronize()
    assert low.heat.dtype is torch.float16 and low.heat.shape == (n, J, 12, 12, 12)
    assert torch.equal(bits(low.heat), bits(pkg.joint_heatmaps(nor, 12, 0.5, layout="cxyz", dtype=torch.float16, status=out.status)))


def test_shape_refusals_are_value_errors_before_any_launch(pkg, monkeypatch):
    """Every tensor-shape refusal of the two wrappers, on device tensors (a CPU tensor stops at "must live on the GPU"
    before its shape is looked at), with the one place an entry is called made to fail: nothing is launched."""
    V = importlib.import_module(pkg.__name__ + ".voxelize")

    def no_call(*a, **kw):
        raise AssertionError("an entry was called")

    monkeypatch.setattr(V, "_call", no_call)
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev())   # noqa: E731
    n, J, R = 2, 21, 8
    good = z(n, 3 * J)
    for bad in (z(n, 64), z(n), z(n, 1), z(n, 2, 2), z(n, 171, 3), z(n, 3 * 171), z(n, 0), torch.zeros((), device=dev())):
        with pytest.raises(ValueError, match="gt_nor"):
            pkg.joint_heatmaps(bad, R)
    for bad in (z(n + 1, dtype=torch.int32), z(n, 2, dtype=torch.int32), z(0, dtype=torch.int32)):
        with pytest.raises(ValueError, match="status"):
            pkg.joint_heatmaps(good, R, status=bad)
    for bad in (z(n, J, R, R, R + 4), z(n, J + 1, R, R, R), z(n + 1, J, R, R, R), z(n, J, R * R * R), z(n * J, R, R, R),
                z(n, J, 12, 12, 12)):
        with pytest.raises(ValueError, match="out"):
            pkg.joint_heatmaps(good, R, out=bad)
    with pytest.raises(ValueError, match="out"):
        pkg.joint_heatmaps(z(n, J, 3), R, out=z(n, 3 * J, R, R, R))
    for bad in (z(n, J, R, R), z(J, R, R, R), z(n, J, R, R, R, 1), z(n, J, R, R, 12), z(n, J, R, 12, R), z(n, J, 12, R, R),
                z(n, J, 6, 6, 6), z(n, J, 2, 2, 2), z(1, 171, 4, 4, 4), z(1, 0, 4, 4, 4)):
        with pytest.raises(ValueError, match="heat|resolution"):
            pkg.heatmap_joints(bad)
    heat = z(n, J, R, R, R)
    fields = dict(u=z(n, J, 3), peak=z(n, J), arg=z(n, J, dtype=torch.int32))
    wrong = dict(u=(z(n, 3 * J), z(n, J, 4), z(n + 1, J, 3)), peak=(z(n, J, 1), z(n * J), z(n, J + 1)),
                 arg=(z(n, J, 3, dtype=torch.int32), z(n * J, dtype=torch.int32), z(J, n, dtype=torch.int32)))
    for name, bads in wrong.items():
        for bad in bads:
            with pytest.raises(ValueError, match="out." + name):
                pkg.heatmap_joints(heat, out=pkg.HeatmapJoints(**{**fields, name: bad}))
    # and with the entry reachable again the good shapes pass
    monkeypatch.undo()
    out = pkg.heatmap_joints(pkg.joint_heatmaps(good + 0.5, R, status=z(n, dtype=torch.int32), out=heat),
                             out=pkg.HeatmapJoints(**fields))
    torch.cuda.synchronize()
    assert out.arg.tolist() == [[(3 * R + 3) * R + 3] * J] * n        # c = 3.5 on every axis: eight maximal voxels, the first in memory
