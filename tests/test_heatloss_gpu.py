"""GPU tier of the voxel heatmap training entries (include/tsdf_heatloss.h): the four kernels of libtsdf_heatloss.so at every
resolution class, plan shape, layout and dtype, and the two autograd wrappers on top of them.

The loss is compared twice.  Against the MERGED encode (joint_heatmaps on the GPU, float32 — a separately tested kernel): the
gradient bit for bit, the sum to its order.  And against the numpy restatement alone (tests/heatloss_ref.py over
tests/heatmap_ref.py, numpy's exp), with the encode's own bound propagated.  The soft-argmax is compared with the
restatement.  Every bound is derived in the docstring of the test that uses it; none was tuned on the code under test.

Shapes are those of tests/test_heatmap_gpu.py.  A case runs every (layout, scalar) combination while it is small and a
rotating one or two of them when its volumes pass 2^21 / 2^23 elements, so that the numpy side of a case stays within a few
seconds; the cases together meet every combination at every resolution class."""
import importlib
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heatloss_ref as lr  # noqa: E402
import heatmap_ref as hr  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAN = float("nan")
SHAPES = [(1, 1), (3, 21), (17, 5), (2, 170)]
CASES = [(R, n, J) for R in (4, 8, 12, 20, 32, 44, 64) for n, J in SHAPES if not (R > 32 and J == 170)] + [(128, 1, 2)]
IDS = [f"R{R}-n{n}-J{J}" for R, n, J in CASES]
SIGMAS, BETAS = (0.5, 1.7, 4.0), (0.5, 1.0, 8.0)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
MANT = {torch.float16: (10, -24), torch.bfloat16: (7, -133)}     # explicit mantissa bits, log2 of the least subnormal


def dev():
    return torch.device("cuda:0")


def combos(k, R, n, J, scalars):
    """The (layout, scalar) combinations case ``k`` runs: all six while n J R^3 <= 2^21, two up to 2^23, else one."""
    every = [(layout, s) for s in scalars for layout in hr.LAYOUTS]
    elems = n * J * R ** 3
    count = 6 if elems <= 2 ** 21 else 2 if elems <= 2 ** 23 else 1
    return [every[(k + 3 * i + i) % 6] for i in range(count)] if count < 6 else every


def test_the_cases_reach_every_plan_shape_item_class_and_combination():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    shapes = {hr.plan_class(n * J, R, cus) for R, n, J in CASES}
    print(f"{cus} CUs: plan shapes {sorted(shapes)}")
    assert shapes == {"one", "equal", "ragged"}                      # the gradient kernels' three plan shapes
    assert {R % 8 == 0 for R, _, _ in CASES} == {False, True}        # both 2-byte item classes
    for scalars in (SIGMAS, BETAS):
        for big in (False, True):                                    # every combination below and above the row-straddling sizes
            seen = {c for k, (R, n, J) in enumerate(CASES) if (R > 20) == big for c in combos(k, R, n, J, scalars)}
            assert len(seen) == 6, (scalars, big, seen)


def centre_u(R):
    """A label that sits on a voxel centre exactly: c = u R - 0.5 is a whole number in float64."""
    return 0.125 if R % 8 else (R // 2 - 0.5) / R


def labels(R, n, J, k):
    """tests/test_heatmap_gpu.py's labels, restated: float32[n,J,3] and int32[n] statuses — interior points, then the special
    joints from the front (one of them, in turn, in a batch of one joint), and frames whose status is not 0."""
    rng = np.random.default_rng(1000 + k)
    u = rng.uniform(0.05, 0.95, size=(n * J, 3)).astype(np.float32)
    cu = centre_u(R)
    special = [(cu, cu, cu),                       # an exact voxel centre
               (0.25, cu, 0.75),                   # exact half-voxel ties on x and z
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
    return u.reshape(n, J, 3), status


def guarded(shape, dtype, fill=NAN):
    """A prefilled buffer with a guard of 64 elements after the end: ``(out, guard)``."""
    count = int(np.prod(shape))
    buf = torch.full((count + 64,), fill, dtype=dtype, device=dev())
    return buf[:count].view(shape), buf[count:]


def intact(guard, fill=NAN):
    return bool(torch.isnan(guard).all()) if fill != fill else bool((guard == fill).all())


def bits(t):
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class Entries:
    """The four C entries on device tensors, through the package's one calling place."""

    def __init__(self, pkg):
        self.V = importlib.import_module(pkg.__name__ + ".voxelize")
        self.L = pkg._lib.load_heatloss()
        self.lay = pkg._lib.LAYOUTS

    @staticmethod
    def _p(t):
        return None if t is None else t.data_ptr()

    def sse(self, pred, u, status, sigma, layout, sse, valid):
        n, J, R = pred.shape[:3]
        self.V._call(pred.device, self.L.tsdf_heat_sse_hip, [pred.data_ptr(), CODES[pred.dtype], u.data_ptr(), self._p(status), n, J, R,
                                                             sigma, self.lay[layout], None, sse.data_ptr(), self._p(valid)], 9)

    def sse_grad(self, pred, u, status, w, sigma, layout, out):
        n, J, R = pred.shape[:3]
        self.V._call(pred.device, self.L.tsdf_heat_sse_grad_hip, [pred.data_ptr(), CODES[pred.dtype], u.data_ptr(), self._p(status),
                                                                  w.data_ptr(), n, J, R, sigma, self.lay[layout], None, out.data_ptr()], 10)

    def soft(self, heat, beta, layout, u, stats):
        n, J, R = heat.shape[:3]
        self.V._call(heat.device, self.L.tsdf_soft_argmax_hip, [heat.data_ptr(), CODES[heat.dtype], n, J, R, beta, self.lay[layout], None,
                                                                u.data_ptr(), stats.data_ptr()], 7)

    def soft_grad(self, heat, stats, gu, beta, layout, out):
        n, J, R = heat.shape[:3]
        self.V._call(heat.device, self.L.tsdf_soft_argmax_grad_hip, [heat.data_ptr(), CODES[heat.dtype], stats.data_ptr(), gu.data_ptr(),
                                                                     n, J, R, beta, self.lay[layout], None, out.data_ptr()], 9)


@pytest.fixture(scope="module")
def ent(pkg):
    return Entries(pkg)


def prediction(t32, seed):
    """Standard-normal values plus the target, float32 on the device."""
    g = torch.Generator(device=dev())
    g.manual_seed(seed)
    return torch.randn(t32.shape, generator=g, device=dev(), dtype=torch.float32) + t32


def loss_outputs(n, J):
    return guarded((n, J), torch.float64), guarded((n, J), torch.int32, -7)


def check_loss_determinism(ent, pred, tu, ts, tw, status, sigma, layout, sse, grad):
    """A second call, a frame alone, a unit alone and the in-place gradient give the bits of the first call."""
    n, J = pred.shape[:2]
    (sse2, _), (valid2, _) = loss_outputs(n, J)
    ent.sse(pred, tu, ts, sigma, layout, sse2, valid2)
    grad2 = torch.empty_like(pred)
    ent.sse_grad(pred, tu, ts, tw, sigma, layout, grad2)
    i = n - 1 if status[n - 1] == 0 else 0
    one = [t[i:i + 1].contiguous() for t in (pred, tu, ts, tw)]
    (sse1, _), (valid1, _) = loss_outputs(1, J)
    ent.sse(one[0], one[1], one[2], sigma, layout, sse1, valid1)
    grad1 = torch.empty_like(one[0])
    ent.sse_grad(one[0], one[1], one[2], one[3], sigma, layout, grad1)
    place = pred.clone()
    ent.sse_grad(place, tu, ts, tw, sigma, layout, place)
    j = J - 1                                                   # and ONE (frame, joint) cut out of the batch: n = 1, J = 1
    unit = [t[i:i + 1, j:j + 1].contiguous() for t in (pred, tu, tw)]
    (sse0, _), (valid0, _) = loss_outputs(1, 1)
    ent.sse(unit[0], unit[1], one[2], sigma, layout, sse0, valid0)
    grad0 = torch.empty_like(unit[0])
    ent.sse_grad(unit[0], unit[1], one[2], unit[2], sigma, layout, grad0)
    torch.cuda.synchronize()
    assert same(sse2, sse) and same(grad2, grad) and same(sse1[0], sse[i]) and same(grad1[0], grad[i]) and same(place, grad)
    assert same(sse0[0, 0], sse[i, j]) and same(grad0[0, 0], grad[i, j]) and int(valid0) == int(valid2[i, j])


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_loss_against_the_merged_encode(pkg, ent, k):
    """The target is joint_heatmaps(..., float32) on the GPU.  grad: bit for bit float32(w (pred - t32)) formed in numpy
    float64 (each a single correctly rounded operation on both sides); a 2-byte output equals that narrowed.  sse: the
    float64 squares are the same numbers on both sides, so the error is the summation order's alone: N <= 2^21 non-negative
    terms, u = 2^-53, any order within N u = 2^-32 relative of the exact sum — 2^-31 sse asked.  math.fsum gives the exact
    sum for EVERY unit of a case of up to 2^21 elements and for three units of a larger one (the first two, the last),
    whose other units are held to numpy's pairwise float64 sum, itself within 21 u < 2^-48 of exact, with
    (2^-31 - 2^-47) sse — which implies the bound against the exact sum."""
    R, n, J = CASES[k]
    u, status = labels(R, n, J, k)
    tu, ts = torch.from_numpy(u).to(dev()), torch.from_numpy(status).to(dev())
    rng = np.random.default_rng(3000 + k)
    for ci, (layout, sigma) in enumerate(combos(k, R, n, J, SIGMAS)):
        t32, valid = pkg.joint_heatmaps(tu, R, sigma, layout=layout, status=ts, return_valid=True)
        pred32 = prediction(t32, 7 * k + ci)
        T, ok = t32.cpu().numpy(), valid.cpu().numpy()
        w = rng.standard_normal((n, J)).astype(np.float32)
        w[ok == 0] = NAN                                       # an invalid unit: +0 whatever w holds
        tw = torch.from_numpy(w).to(dev())
        for dt in DTYPES:
            pred = pred32.to(dt)
            P = pred.float().cpu().numpy()
            (sse, g1), (gvalid, g2) = loss_outputs(n, J)
            grad, g3 = guarded(pred.shape, dt)
            ent.sse(pred, tu, ts, sigma, layout, sse, gvalid)
            ent.sse_grad(pred, tu, ts, tw, sigma, layout, grad)
            torch.cuda.synchronize()
            assert intact(g1) and intact(g2, -7) and intact(g3)
            got, ref = sse.cpu().numpy(), lr.sse(P, T, ok)
            assert np.array_equal(gvalid.cpu().numpy(), ok) and not np.isnan(got).any()
            assert (got[ok == 0] == 0).all() and not np.signbit(got).any()
            rel = np.abs(got - ref) / np.where(ref > 0, ref, 1.0)
            print(f"R={R} n={n} J={J} {layout} sigma={sigma} {dt}: sse worst {float(rel.max()) / lr.U:.1f} u")
            assert (np.abs(got - ref) <= (2.0 ** -31 - 2.0 ** -47) * ref).all()
            for q in range(n * J) if n * J * R ** 3 <= 2 ** 21 else sorted({0, min(1, n * J - 1), n * J - 1}):
                i, j = divmod(q, J)
                if ok[i, j]:
                    d = P[i, j].astype(np.float64).ravel() - T[i, j].astype(np.float64).ravel()
                    exact = math.fsum(d * d)
                    assert abs(got[i, j] - exact) <= 2.0 ** -31 * exact
            want = lr.sse_grad(P, T, ok, w)
            if dt is torch.float32:
                assert np.array_equal(grad.cpu().numpy().view(np.int32), want.view(np.int32))
            else:
                assert torch.equal(grad.cpu(), torch.from_numpy(want).to(dt))
            bad = torch.from_numpy(ok == 0).to(dev())
            assert not bool(bits(grad[bad]).any())             # +0 in every voxel of an invalid unit, under a NaN w
            if ci == 0 and (dt is DTYPES[k % 3] or n * J * R ** 3 <= 2 ** 21):
                check_loss_determinism(ent, pred, tu, ts, tw, status, sigma, layout, sse, grad)
        if n * J > 1:       # without a status every frame counts
            (sse, _), (gvalid, _) = loss_outputs(n, J)
            ent.sse(pred32, tu, None, sigma, layout, sse, None)
            ent.sse(pred32, tu, None, sigma, layout, sse.clone(), gvalid)
            torch.cuda.synchronize()
            assert np.array_equal(gvalid.cpu().numpy(), np.isfinite(u).all(axis=2).astype(np.int32))
            if (status != 0).any():
                assert bool((sse[torch.from_numpy(status != 0).to(dev())] > 0).any())


@pytest.mark.parametrize("R", [4, 12, 32, 44])
def test_loss_of_the_targets_themselves_is_exactly_zero(pkg, R):
    """heatmap_mse_loss(joint_heatmaps(gt_nor), gt_nor): the kernel regenerates the encode's float32 bit for bit, so every
    d is 0 exactly, the loss is 0 exactly under every reduction and the gradient is zero bits up to sign."""
    n, J = 3, 21
    u, status = labels(R, n, J, R)
    tu, ts = torch.from_numpy(u).to(dev()), torch.from_numpy(status).to(dev())
    for layout, sigma in [(layout, s) for s in SIGMAS for layout in hr.LAYOUTS]:
        heat = pkg.joint_heatmaps(tu, R, sigma, layout=layout, status=ts)
        for reduction in ("mean", "sum", "none"):
            pred = heat.clone().requires_grad_()
            loss = pkg.heatmap_mse_loss(pred, tu, sigma=sigma, layout=layout, status=ts, reduction=reduction)
            loss.sum().backward()
            torch.cuda.synchronize()
            assert loss.dtype is torch.float32 and not bool(bits(loss).any()), (layout, sigma, reduction)
            assert not bool((bits(pred.grad) & 0x7fffffff).any())
        assert bool(heat.any())


@pytest.mark.parametrize("k", [k for k, (R, n, J) in enumerate(CASES) if n * J * R ** 3 <= 2 ** 23], ids=lambda k: IDS[k])
def test_loss_against_the_restatement_alone(pkg, ent, k):
    """No GPU target here: t32 is heatmap_ref.encode's (numpy exp).  The encode kernel is within e = 2^-23 t + 2^-125 of it
    per voxel (tests/test_heatmap_gpu.py's bound); through d and d^2 that is e (2 |d| + e) per voxel, summed per unit, plus
    2^-31 sse for the order: heatloss_ref.sse_bound.  The gradient: |w| e per voxel before one rounding to float32,
    2^-24 |w d| more."""
    R, n, J = CASES[k]
    u, status = labels(R, n, J, k)
    tu, ts = torch.from_numpy(u).to(dev()), torch.from_numpy(status).to(dev())
    layout, sigma = combos(k, R, n, J, SIGMAS)[0] if n * J * R ** 3 > 2 ** 21 else [(la, s) for s in SIGMAS for la in hr.LAYOUTS][k % 6]
    T, ok = hr.encode(u, status, R, sigma, layout)
    pred32 = prediction(torch.from_numpy(T).to(dev()), 11 * k)
    w = np.random.default_rng(k).standard_normal((n, J)).astype(np.float32)
    tw = torch.from_numpy(w).to(dev())
    for dt in DTYPES:
        pred = pred32.to(dt)
        P = pred.float().cpu().numpy()
        (sse, g1), (gvalid, g2) = loss_outputs(n, J)
        grad, g3 = guarded(pred.shape, torch.float32 if dt is torch.float32 else dt)
        ent.sse(pred, tu, ts, sigma, layout, sse, gvalid)
        ent.sse_grad(pred, tu, ts, tw, sigma, layout, grad)
        torch.cuda.synchronize()
        assert intact(g1) and intact(g2, -7) and intact(g3)
        got, ref, bound = sse.cpu().numpy(), lr.sse(P, T, ok), lr.sse_bound(P, T, ok)
        print(f"R={R} n={n} J={J} {layout} sigma={sigma} {dt}: {int((got != ref).sum())} of {n * J} units differ at all, "
              f"worst error / bound {float((np.abs(got - ref) / np.where(bound > 0, bound, 1.0)).max()):.3g}")
        assert np.array_equal(gvalid.cpu().numpy(), ok) and (np.abs(got - ref) <= bound).all()
        if dt is torch.float32:
            exact = lr.sse_grad(P, T, ok, w, exact=True)
            e = 2.0 ** -23 * T.astype(np.float64) + 2.0 ** -125
            tol = np.abs(w.astype(np.float64)).reshape(n, J, 1, 1, 1) * e + 2.0 ** -24 * np.abs(exact) + 2.0 ** -149
            assert (np.abs(grad.cpu().numpy().astype(np.float64) - exact) <= tol).all()


def test_a_non_finite_prediction_stays_in_its_unit(pkg, ent):
    n, J, R = 2, 3, 12
    u = np.random.default_rng(1).uniform(0.1, 0.9, (n, J, 3)).astype(np.float32)
    tu = torch.from_numpy(u).to(dev())
    for dt in DTYPES:
        for layout in hr.LAYOUTS:
            pred = torch.zeros((n, J, R, R, R), dtype=dt, device=dev())
            pred[0, 1, 3, 7, 11] = NAN
            pred[1, 2, 11, 11, 11] = float("inf")
            pred[1, 0, 0, 0, 0] = float("-inf")
            (sse, _), (valid, _) = loss_outputs(n, J)
            ent.sse(pred, tu, None, 1.7, layout, sse, valid)
            torch.cuda.synchronize()
            got = sse.cpu().numpy()
            assert np.isnan(got[0, 1]) and got[1, 2] == np.inf and got[1, 0] == np.inf
            assert np.isfinite(got[[0, 0, 1], [0, 2, 1]]).all() and bool((valid == 1).all())
            loss = pkg.heatmap_mse_loss(pred, tu, layout=layout, reduction="none")
            assert torch.isnan(loss[0, 1]) and int(torch.isfinite(loss).sum()) == 3


# ---- soft-argmax ----
def volumes(R, n, J, k):
    """Standard-normal float32 volumes scaled by 3 with, volume by volume in turn: nothing; the one-hot-like volume (0
    everywhere but 40 at one voxel); a NaN somewhere; -inf alone; a +inf somewhere; NaN alone; a constant."""
    rng = np.random.default_rng(4000 + k)
    v = 3.0 * rng.standard_normal(size=(n * J, R, R, R), dtype=np.float32)
    kinds = []
    for q in range(n * J):
        kind = (q + k) % 9
        kinds.append(kind)
        flat = v[q].reshape(-1)
        at = int(rng.integers(R ** 3))
        if kind == 1:
            flat[:] = 0.0
            flat[at] = 40.0
        elif kind == 2:
            flat[at] = np.nan
        elif kind == 3:
            flat[:] = -np.inf
        elif kind == 4:
            flat[at] = np.inf
        elif kind == 5:
            flat[:] = np.nan
        elif kind == 6:
            flat[:] = 0.25
    return v.reshape(n, J, R, R, R), np.array(kinds).reshape(n, J)


def ulp_of(x, dt):
    """One unit in the last place of the 2-byte dtype at the float values ``x`` of that dtype (numpy float64)."""
    mant, least = MANT[dt]
    _, e = np.frexp(np.abs(x))                      # |x| = f 2^e, f in [0.5, 1)
    return np.exp2(np.maximum(e - 1 - mant, least).astype(np.float64))


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_soft_argmax_and_its_gradient_against_the_restatement(pkg, ent, k):
    """Both sides form beta (h - m) by the same two float64 operations, so exp meets the same argument; it is correct to
    1 ulp on either side: 4 u between them per term.  Z and the three moments are sums of N = R^3 <= 2^21 non-negative
    terms in different orders, N u each way: |dZ| <= (2 N + 4) u Z, and with the division |dc_a| <= (4 N + 10) u c_a —
    below 2^-30 c_a, so u_a = float32((c_a + 0.5) / R) in [0, 1] moves by less than 2^-31 before ONE rounding to float32:
    2^-23 asked, the decode's radius bound.  m is exact.  A volume with a NaN, of -inf alone or with a +inf is NaN in u, Z
    and c, that unit alone.  Gradient: heatloss_ref.soft_argmax_grad_bound; a 2-byte output within one ulp of that dtype
    of the narrowed restatement OF THE STATS THE ENTRY WAS HANDED (the forward's own output, held to its bounds above):
    s_i and k are then the same float64 bits on both sides, the two results differ by exp's ulp alone, which is the
    same float32 or its neighbour and so the same 2-byte value or its neighbour — the peak voxel of the one-hot-like
    volume, where s_i cancels to next to nothing, included."""
    R, n, J = CASES[k]
    N = R ** 3
    v32, kinds = volumes(R, n, J, k)
    host = torch.from_numpy(v32)
    finite = ~np.isin(kinds, (2, 3, 4, 5))
    gu = np.random.default_rng(5000 + k).standard_normal((n, J, 3)).astype(np.float32)
    tgu = torch.from_numpy(gu).to(dev())
    for ci, (layout, beta) in enumerate(combos(k, R, n, J, BETAS)):
        for dt in DTYPES:
            hd = host.to(dt)                               # narrowed on the host: both sides read the same values
            seen = hd.float().numpy()
            d = hd.to(dev())
            (gu_, g1), (gs_, g2) = guarded((n, J, 3), torch.float32), guarded((n, J, 5), torch.float64)
            grad, g3 = guarded(d.shape, dt)
            ent.soft(d, beta, layout, gu_, gs_)
            ent.soft_grad(d, gs_, tgu, beta, layout, grad)
            torch.cuda.synchronize()
            assert intact(g1) and intact(g2) and intact(g3)
            ru, rs = lr.soft_argmax(seen, R, beta, layout)
            got_u, got_s = gu_.cpu().numpy(), gs_.cpu().numpy()
            assert np.array_equal(np.isnan(got_u), np.isnan(ru)) and np.array_equal(np.isnan(got_s), np.isnan(rs))
            assert np.isnan(got_u[~finite]).all() and np.isnan(got_s[~finite][:, 1:]).all() and not np.isnan(got_u[finite]).any()
            assert np.array_equal(got_s[..., 0], rs[..., 0])                                      # m, exactly
            f = finite
            err_u = np.abs(got_u[f].astype(np.float64) - ru[f]).max() if f.any() else 0.0
            assert err_u <= 2.0 ** -23, (dt, layout, beta, err_u)
            if f.any():
                assert (np.abs(got_s[f][:, 1] - rs[f][:, 1]) <= (2 * N + 4) * lr.U * rs[f][:, 1]).all()
                assert (np.abs(got_s[f][:, 2:] - rs[f][:, 2:]) <= (4 * N + 10) * lr.U * rs[f][:, 2:]).all()
            hot = kinds == 1
            if hot.any() and beta == 8.0:                  # u of the one-hot-like volume is the radius-0 decode's, to 2^-23
                dec = pkg.heatmap_joints(d, layout=layout).u.cpu().numpy()
                assert np.abs(got_u[hot].astype(np.float64) - dec[hot]).max() <= 2.0 ** -23
            # gradient
            gg = grad.float().cpu().numpy()
            assert np.isnan(gg[~finite]).all() and not np.isnan(gg[finite]).any()
            if f.any():
                if dt is torch.float32:
                    bound = lr.soft_argmax_grad_bound(seen[f][None], rs[f][None], gu[f][None], R, beta, layout)[0]
                    exact = lr.soft_argmax_grad(seen[f][None], rs[f][None], gu[f][None], R, beta, layout, exact=True)[0]
                    err = np.abs(gg[f].astype(np.float64) - exact)
                    print(f"R={R} n={n} J={J} {layout} beta={beta}: u err {err_u:.3g}, grad worst error / bound {float((err / bound).max()):.3g}")
                    assert (err <= bound).all()
                else:
                    same_stats = lr.soft_argmax_grad(seen[f][None], got_s[f][None], gu[f][None], R, beta, layout)[0]
                    narrowed = torch.from_numpy(same_stats).to(dt).float().numpy().astype(np.float64)
                    assert (np.abs(gg[f].astype(np.float64) - narrowed) <= ulp_of(narrowed, dt)).all(), (dt, layout, beta)
            if ci == 0 and (dt is DTYPES[k % 3] or n * J * N <= 2 ** 21):
                # a second call, a frame alone, a unit alone and the in-place gradient give the bits of the first call
                u2, s2 = torch.empty_like(gu_), torch.empty_like(gs_)
                ent.soft(d, beta, layout, u2, s2)
                grad2 = torch.empty_like(d)
                ent.soft_grad(d, s2, tgu, beta, layout, grad2)
                i = n - 1
                one = d[i:i + 1].contiguous()
                u1, s1 = torch.empty((1, J, 3), device=dev()), torch.empty((1, J, 5), dtype=torch.float64, device=dev())
                ent.soft(one, beta, layout, u1, s1)
                grad1 = torch.empty_like(one)
                ent.soft_grad(one, s1, tgu[i:i + 1].contiguous(), beta, layout, grad1)
                place = d.clone()
                ent.soft_grad(place, gs_, tgu, beta, layout, place)
                j = J - 1                                   # and ONE (frame, joint) cut out of the batch: n = 1, J = 1
                cut = d[i:i + 1, j:j + 1].contiguous()
                u0, s0 = torch.empty((1, 1, 3), device=dev()), torch.empty((1, 1, 5), dtype=torch.float64, device=dev())
                ent.soft(cut, beta, layout, u0, s0)
                grad0 = torch.empty_like(cut)
                ent.soft_grad(cut, s0, tgu[i:i + 1, j:j + 1].contiguous(), beta, layout, grad0)
                torch.cuda.synchronize()
                assert same(u2, gu_) and same(s2, gs_) and same(grad2, grad) and same(place, grad)
                assert same(u1[0], gu_[i]) and same(s1[0], gs_[i]) and same(grad1[0], grad[i])
                assert same(u0[0, 0], gu_[i, j]) and same(s0[0, 0], gs_[i, j]) and same(grad0[0, 0], grad[i, j])


# ---- the wrappers ----
def mixed_batch(R, n, J, seed, dt):
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.1, 0.9, (n, J, 3)).astype(np.float32)
    u[0, 1, 2] = NAN
    status = np.zeros(n, np.int32)
    status[1] = 2
    pred = torch.from_numpy(rng.standard_normal((n, J, R, R, R)).astype(np.float32)).to(dev()).to(dt)
    return u, status, pred


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f16", "bf16"])
def test_autograd_end_to_end(pkg, ent, dt):
    """pred.grad is the C entry's gradient with the wrapper's own w (torch.equal); the loss is the restatement's float64
    value rounded to float32, 2 float32 ulps allowed (sse within 2^-31, the reduction's sum and division within a few u,
    one rounding to float32: half an ulp and a little); gt_nor gets no gradient."""
    R, n, J, sigma, layout = 12, 3, 4, 1.7, "cxyz"
    u, status, pred = mixed_batch(R, n, J, 21, dt)
    tu, ts = torch.from_numpy(u).to(dev()).requires_grad_(), torch.from_numpy(status).to(dev())
    T, ok = hr.encode(u, status, R, sigma, layout)
    P = pred.float().cpu().numpy()
    ref_sse = lr.sse(P, T, ok)
    assert ok.sum() == n * J - J - 1
    up = torch.from_numpy(np.random.default_rng(2).uniform(0.5, 2.0, (n, J)).astype(np.float32)).to(dev())
    for reduction in ("mean", "sum", "none"):
        p = pred.clone().requires_grad_()
        loss = pkg.heatmap_mse_loss(p, tu, sigma=sigma, layout=layout, status=ts, reduction=reduction)
        assert loss.dtype is torch.float32 and loss.shape == ((n, J) if reduction == "none" else ())
        (loss * up).sum().backward() if reduction == "none" else (3.0 * loss).backward()
        rl, factor = lr.reduce(ref_sse, ok, R, reduction)
        w = lr.weights(up.cpu().numpy() if reduction == "none" else 3.0, factor)
        want = torch.empty_like(pred)
        ent.sse_grad(pred, tu.detach(), ts, torch.from_numpy(w).to(dev()), sigma, layout, want)
        torch.cuda.synchronize()
        assert p.grad.dtype is dt and torch.equal(bits(p.grad), bits(want)) and bool(p.grad.any()), reduction
        rl32 = np.asarray(rl, np.float64).astype(np.float32)
        assert (np.abs(loss.detach().cpu().numpy().astype(np.float64) - rl32) <= 2 * np.spacing(np.abs(rl32))).all(), reduction
        assert tu.grad is None
    # no valid unit: 0 loss, 0 gradient
    p = pred.clone().requires_grad_()
    loss = pkg.heatmap_mse_loss(p, tu, sigma=sigma, layout=layout, status=torch.ones_like(ts))
    loss.backward()
    assert float(loss.detach()) == 0.0 and not bool(bits(p.grad).any())
    # soft-argmax, then an L1 against the labels
    beta = 1.0
    p = pred.clone().requires_grad_()
    su = pkg.soft_argmax_joints(p, beta=beta, layout=layout)
    target = torch.nan_to_num(tu.detach(), nan=0.5)
    (su - target).abs().sum().backward()
    ru, rs = lr.soft_argmax(P, R, beta, layout)
    assert su.shape == (n, J, 3) and np.abs(su.detach().cpu().numpy().astype(np.float64) - ru).max() <= 2.0 ** -23
    u2, stats = torch.empty((n, J, 3), device=dev()), torch.empty((n, J, 5), dtype=torch.float64, device=dev())
    ent.soft(pred, beta, layout, u2, stats)
    want = torch.empty_like(pred)
    ent.soft_grad(pred, stats, torch.sign(u2 - target).contiguous(), beta, layout, want)
    torch.cuda.synchronize()
    assert same(su.detach(), u2) and torch.equal(bits(p.grad), bits(want)) and bool(p.grad.any())
    back = pkg.denormalize_joints(su.detach().reshape(n, 3 * J), torch.ones(n, device=dev()), torch.zeros((n, 3), device=dev()))
    assert back.shape[0] == n


def test_forward_and_gradient_are_captured_and_replayed(pkg):
    n, J, R = 3, 5, 12
    gen = np.random.default_rng(3)
    pred = torch.zeros((n, J, R, R, R), dtype=torch.bfloat16, device=dev())
    gt = torch.zeros((n, J, 3), device=dev())
    st = torch.zeros(n, dtype=torch.int32, device=dev())
    outs = {}

    def run(p, g, s):
        a = p.detach().clone().requires_grad_()
        loss = pkg.heatmap_mse_loss(a, g, sigma=1.0, layout="cxyz", status=s)
        loss.backward()
        b = p.detach().clone().requires_grad_()
        su = pkg.soft_argmax_joints(b, beta=2.0, layout="cxyz")
        (su - g).abs().sum().backward()
        return loss.detach(), a.grad, su.detach(), b.grad

    def fill(seed):
        r = np.random.default_rng(seed)
        pred.copy_(torch.from_numpy(r.standard_normal(tuple(pred.shape)).astype(np.float32)).to(dev()))
        gt.copy_(torch.from_numpy(r.uniform(0, 1, (n, J, 3)).astype(np.float32)).to(dev()))
        st.copy_(torch.tensor([0, seed % 2, 0], dtype=torch.int32))

    fill(int(gen.integers(100)))
    side = torch.cuda.Stream(dev())
    with torch.cuda.stream(side):
        run(pred, gt, st)                                   # warm-up on the capture stream
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        outs["replay"] = run(pred, gt, st)
    for seed in (4, 5):
        fill(seed)
        g.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in outs["replay"]]
        eager = run(pred, gt, st)
        torch.cuda.synchronize()
        for x, y in zip(replayed, eager):
            assert same(x, y) and bool(y.any())


def test_the_training_line_without_a_target_volume(pkg):
    """AugmentedStep(dtype=bfloat16) WITHOUT heatmap= feeds gt_nor and status to heatmap_mse_loss, batch 3 at R = 12, against
    ((pred.float() - joint_heatmaps(gt_nor, 12, sigma, status=status)) ** 2) reduced in float64: the sse bound (2^-31
    relative, the order of the sums) and the wrapper's rounding of the result to float32 (2^-24)."""
    synth = importlib.import_module(pkg.__name__ + ".synth")
    n, R, J, sigma = 3, 12, 21, 1.7
    depth, off, hdr = synth.synth_batch(5, "crop", seed0=77)
    depth = depth.copy()
    depth[off[4]:off[5]] = 0                      # a frame without a valid pixel: status 1
    td, to, th = (torch.from_numpy(x).to(dev()) for x in (depth, off, hdr))
    mid_p = pkg.voxelize(td, to, th, res=R).mid_p
    noise = torch.from_numpy(np.random.default_rng(9).normal(0, 40, (5, J, 3)).astype(np.float32)).to(dev())
    gt = (mid_p[:, None, :] + noise).reshape(5, 3 * J).contiguous()
    step = pkg.AugmentedStep(td, to, th, n, gt=gt, res=R, dtype=torch.bfloat16)
    assert step.heat is None
    for index in ([0, 4, 2], [3, 1, 0]):
        out, gt_nor, _ = step.step(index, 0xBEEF, 0)
        assert out.tsdf.dtype is torch.bfloat16
        pred = torch.randn((n, J, R, R, R), device=dev()).to(torch.bfloat16).requires_grad_()     # a network's output
        loss = pkg.heatmap_mse_loss(pred, gt_nor, sigma=sigma, status=out.status)
        loss.backward()
        heat, valid = pkg.joint_heatmaps(gt_nor, R, sigma, status=out.status, return_valid=True)
        sq = ((pred.detach().float().double() - heat.double()) ** 2).reshape(n, J, -1).sum(dim=2)
        count = int(valid.sum())
        want = float((sq * valid).sum()) / (count * R ** 3)
        torch.cuda.synchronize()
        assert count == J * (n - index.count(4)) and abs(float(loss.detach()) - want) <= (2.0 ** -31 + 2.0 ** -24) * want
        assert pred.grad.dtype is torch.bfloat16 and bool(pred.grad.any())
        assert not bool(pred.grad[out.status != 0].any())


def test_shape_refusals_are_value_errors_before_any_launch(pkg, monkeypatch):
    """Every tensor refusal of the two wrappers on device tensors, with the one place an entry is called made to fail."""
    V = importlib.import_module(pkg.__name__ + ".voxelize")

    def no_call(*a, **kw):
        raise AssertionError("an entry was called")

    monkeypatch.setattr(V, "_call", no_call)
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev())   # noqa: E731
    n, J, R = 2, 21, 8
    pred, good = z(n, J, R, R, R), z(n, 3 * J)
    for bad in (z(n, J, R, R), z(J, R, R, R), z(n, J, R, R, R, 1), z(n, J, R, R, 12), z(n, J, R, 12, R), z(n, J, 12, R, R),
                z(n, J, 6, 6, 6), z(n, J, 2, 2, 2), z(1, 171, 4, 4, 4), z(1, 0, 4, 4, 4), z(n, J, R, R, 2 * R)[..., ::2],
                z(n * J * R ** 3 + 8)[1:1 + n * J * R ** 3].view(n, J, R, R, R), z(n, J, R, R, R, dtype=torch.float64)):
        with pytest.raises(ValueError, match="pred|resolution|dtype"):
            pkg.heatmap_mse_loss(bad, good)
        with pytest.raises(ValueError, match="pred|resolution|dtype"):
            pkg.soft_argmax_joints(bad)
    with pytest.raises(ValueError, match="16-byte aligned"):
        pkg.soft_argmax_joints(z(n * J * R ** 3 + 8, dtype=torch.bfloat16)[2:2 + n * J * R ** 3].view(n, J, R, R, R))
    for bad in (z(n, 64), z(n), z(n + 1, 3 * J), z(n, J + 1, 3), z(3 * J, n), z(n, 3 * J, dtype=torch.float64), z(n, 6 * J)[:, ::2], z(n, 3, J), z(n, 3 * J, 1),
                torch.zeros((n, 3 * J))):
        with pytest.raises(ValueError, match="gt_nor"):
            pkg.heatmap_mse_loss(pred, bad)
    for bad in (z(n + 1, dtype=torch.int32), z(n, 2, dtype=torch.int32), z(0, dtype=torch.int32), z(n, dtype=torch.int64), z(n),
                z(2 * n, dtype=torch.int32)[::2], torch.zeros(n, dtype=torch.int32), z(1, n, dtype=torch.int32),
                z(n, 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="status"):
            pkg.heatmap_mse_loss(pred, good, status=bad)
    with pytest.raises(ValueError, match="reduction"):
        pkg.heatmap_mse_loss(pred, good, reduction="max")
    # and with the entry reachable again the good shapes pass: the loss of an all-zero prediction is the targets' mean square
    monkeypatch.undo()
    loss = pkg.heatmap_mse_loss(pred, good + 0.5, status=z(n, dtype=torch.int32))
    heat = pkg.joint_heatmaps(good + 0.5, R)
    assert abs(float(loss) - float((heat.double() ** 2).mean())) <= 2.0 ** -23 * float(loss) and float(loss) > 0
    assert pkg.soft_argmax_joints(pred).tolist() == [[[0.5, 0.5, 0.5]] * J] * n     # a constant volume: the cube's centre
