"""CPU tier of the voxel heatmap training entries (include/tsdf_heatloss.h): libtsdf_heatloss.so as far as it goes without a
GPU — the build rule, the loader's row against header and binary, the version, every argument refusal before device work —,
the properties of the numpy restatement the GPU tier compares with (tests/heatloss_ref.py), the public names and refusals,
and the library's host-only code under the CPU sanitizers as a child process.  Nothing here touches a GPU."""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heatloss_ref as lr  # noqa: E402
import heatmap_ref as hr  # noqa: E402
from abi_util import declared_functions, exported  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "handposeestimation-with-3d-cnns_amd", "csrc")
INVALID, NO_DEVICE = -1, -2
WANT = ["tsdf_heat_sse_grad_hip", "tsdf_heat_sse_hip", "tsdf_heatloss_version", "tsdf_soft_argmax_grad_hip", "tsdf_soft_argmax_hip"]
OTHERS = ["augment", "augstep", "auggrid", "depth16", "obb", "lowp", "maplowp", "mapstep", "locate", "accurate", "mapaccurate"]


# ---- library pins ----
def test_row_binds_exactly_its_header_with_types(pkg):
    lib = pkg._lib
    ext = lib._HEATLOSS
    assert isinstance(ext, lib._Ext) and "heatloss" not in lib._EXTS
    assert declared_functions("tsdf_heatloss.h") == WANT == sorted([ext.version_symbol, *ext.entries])
    funcs, named = exported(lib.HEATLOSS_LIB_PATH)
    assert funcs == WANT and named == WANT
    assert ext.path == lib.HEATLOSS_LIB_PATH and ext.version == lib.HEATLOSS_VERSION == 1
    L = lib.load_heatloss()
    assert L.tsdf_heatloss_version() == 1
    for entry in (ext.version_symbol, *ext.entries):
        fn = getattr(L, entry)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, entry
    vp, i, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert list(L.tsdf_heatloss_version.argtypes) == []
    assert list(L.tsdf_heat_sse_hip.argtypes) == [vp, i, vp, vp, i, i, i, f32, i, vp, vp, vp]
    assert list(L.tsdf_heat_sse_grad_hip.argtypes) == [vp, i, vp, vp, vp, i, i, i, f32, i, vp, vp]
    assert list(L.tsdf_soft_argmax_hip.argtypes) == [vp, i, i, i, i, f32, i, vp, vp, vp]
    assert list(L.tsdf_soft_argmax_grad_hip.argtypes) == [vp, i, vp, vp, i, i, i, f32, i, vp, vp]
    for name, args in ext.entries.items():
        assert list(getattr(L, name).argtypes) == args and args
    # one object, distinct from every other loader's
    assert lib.load_heatloss() is L and L is not lib.load() and L is not lib.load_heatmap()
    assert all(L is not getattr(lib, "load_" + other)() for other in OTHERS)
    text = open(os.path.join(ROOT, "include", "tsdf_heatloss.h")).read()
    assert "tsdf_cam" not in text and "#define TSDF_HEATLOSS_VERSION 1" in text
    assert "d_out_grad == d_pred (in place) is allowed" in text
    assert lib.load().tsdf_version() == 7 and lib.load_heatmap().tsdf_heatmap_version() == 1   # what was there is what it was


def test_wrong_version_and_missing_library_raise_import_error(pkg, monkeypatch):
    lib = pkg._lib
    row = lib._HEATLOSS
    monkeypatch.delitem(lib._ext_libs, "heatloss", raising=False)
    monkeypatch.setattr(lib, "_HEATLOSS", row._replace(version=row.version + 1))
    with pytest.raises(ImportError, match="version 1.*csrc heatloss"):
        lib.load_heatloss()
    monkeypatch.setattr(lib, "_HEATLOSS", row._replace(path=os.path.join(ROOT, "build", "no_such_libtsdf_heatloss.so")))
    with pytest.raises(ImportError, match="csrc heatloss"):
        lib.load_heatloss()


# ---- build pins ----
def test_makefile_builds_it_outside_the_pinned_table():
    lines = open(os.path.join(CSRC, "Makefile")).read().splitlines()
    assert "heatloss_DEPS := narrow.inc heatmap_host.inc heatloss_host.inc ../../include/tsdf_heatmap.h ../../include/tsdf_lowp.h" in lines
    assert "$(eval $(call EXT_RULES,heatloss))" in lines and "$(eval $(call EXT_RULES,heatmap))" in lines
    (all_line,) = [ln for ln in lines if ln.startswith("all:")]
    (phony,) = [ln for ln in lines if ln.startswith(".PHONY:")]
    assert "heatloss" in all_line.split()
    for name in ("heatloss", "heatloss-resources", "heatloss-asm", "heatloss-host-asan"):
        assert name in phony.split(), name
    clean = lines[lines.index("clean:") + 1]
    assert "../libtsdf_heatloss.so" in clean.split()
    (src,) = [ln for ln in lines if ln.startswith("SRC :=")]
    assert "heatloss_host.inc" in src.split("$(filter-out", 1)[1].split(",", 1)[0].split()   # not a part of the product
    (exts,) = [ln for ln in lines if re.match(r"^EXTS := ", ln)]
    assert exts.split(":=")[1].split() == OTHERS


def test_make_rules_cross_compile_for_gfx950_without_scratch():
    r = subprocess.run(["make", "-C", CSRC, "heatloss", "heatloss-resources"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stdout + r.stderr
    names = ("tsdf_heat_sse_kernel", "tsdf_heat_sse_grad_kernel", "tsdf_soft_argmax_kernel", "tsdf_soft_argmax_grad_kernel")
    count = {k: len([ln for ln in text.splitlines() if "Function Name" in ln and re.search(rf"\d{k}I", ln)]) for k in names}
    # forward: 2 layouts x 3 dtypes; gradient: 2 layouts x (float32, and 2 dtypes x {8, 4} voxels a lane)
    assert count == {names[0]: 6, names[1]: 10, names[2]: 6, names[3]: 10}, count
    scratch = [ln for ln in text.splitlines() if "ScratchSize" in ln]
    assert len(scratch) == 32 and all(ln.split("]:")[1].split()[0] == "0" for ln in scratch), scratch
    src = open(os.path.join(CSRC, "tsdf_heatloss.hip")).read()
    assert sorted(re.findall(r'#include "(\w+\.inc)"', src)) == ["device.inc", "heatloss_host.inc", "heatmap_host.inc", "narrow.inc"]
    assert "atomic" not in src.split("namespace {", 1)[1] and "__device__ int" not in src   # no atomics, no device globals
    assert not re.search(r"^\s*(static\s+)?__(device|constant|managed)__\s+[\w:<> ]+\s+\w+\s*(\[|=|;)", src, flags=re.M)
    assert "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read()


# ---- refusals ----
null, one, odd8, odd4, odd2 = (ctypes.c_void_p(v) for v in (0, 64, 72, 68, 66))
nan, inf = float("nan"), float("inf")


def _calls(pkg):
    """The four entries on dummy pointers (64: aligned for every check), every argument good unless named."""
    L = pkg._lib.load_heatloss()

    def sse(pred=one, dtype=0, u=one, status=one, n=3, J=21, R=32, scalar=1.7, layout=0, out=one, valid=one):
        return L.tsdf_heat_sse_hip(pred, dtype, u, status, n, J, R, scalar, layout, null, out, valid)

    def sse_grad(pred=one, dtype=0, u=one, status=one, w=one, n=3, J=21, R=32, scalar=1.7, layout=0, out=one):
        return L.tsdf_heat_sse_grad_hip(pred, dtype, u, status, w, n, J, R, scalar, layout, null, out)

    def soft(pred=one, dtype=0, n=3, J=21, R=32, scalar=1.0, layout=0, u=one, out=one):
        return L.tsdf_soft_argmax_hip(pred, dtype, n, J, R, scalar, layout, null, u, out)

    def soft_grad(pred=one, dtype=0, stats=one, u=one, n=3, J=21, R=32, scalar=1.0, layout=0, out=one):
        return L.tsdf_soft_argmax_grad_hip(pred, dtype, stats, u, n, J, R, scalar, layout, null, out)

    return L, sse, sse_grad, soft, soft_grad


def test_every_defect_is_refused_before_device_work(pkg):
    L, sse, sse_grad, soft, soft_grad = _calls(pkg)
    shared = [dict(n=-1), *[dict(R=R) for R in (0, 2, 3, 6, 30, 132, 256, -4)], dict(J=0), dict(J=171), dict(J=-1),
              dict(layout=2), dict(layout=-1), dict(dtype=3), dict(dtype=-1), dict(n=2 ** 24, J=1), dict(n=98690, J=170),
              *[dict(scalar=s) for s in (0.0, -0.0, -1.0, nan, inf, -inf, 1e-50)],
              dict(pred=null), dict(pred=odd8), dict(u=null), dict(u=odd2), dict(out=null)]
    defects = {
        sse: shared + [dict(out=odd4), dict(status=odd2), dict(valid=odd2)],
        sse_grad: shared + [dict(out=odd8), dict(status=odd2), dict(w=null), dict(w=odd2)],
        soft: shared + [dict(out=odd4)],
        soft_grad: shared + [dict(out=odd8), dict(stats=null), dict(stats=odd4)],
    }
    for call, rows in defects.items():
        for kw in rows:
            assert call(**kw) == INVALID, (call.__name__, kw)
            if "n" not in kw:      # n == 0 is a no-op whatever comes after it in the order
                assert call(n=0, **kw) == 0, (call.__name__, kw)
        assert call(n=0) == 0 and call(n=0, J=0, R=5) == 0
    assert L.tsdf_heat_sse_hip(null, 9, null, null, 0, 0, 0, nan, 9, null, null, null) == 0
    assert L.tsdf_heat_sse_grad_hip(null, 9, null, null, null, 0, 0, 0, nan, 9, null, null) == 0
    assert L.tsdf_soft_argmax_hip(null, 9, 0, 0, 0, nan, 9, null, null, null) == 0
    assert L.tsdf_soft_argmax_grad_hip(null, 9, null, null, 0, 0, 0, nan, 9, null, null) == 0


# The header's order, pair by pair: of two defects the earlier rule's is the one that decides.  Every refusal answers
# INVALID, so the order shows where a later defect is paired with n == 0 (above) and, on this side of the ABI, in the
# stand-alone program, which sees the rule's own name (test_host_code_under_sanitizers_as_a_stand_alone_program).
# Good arguments reach check_device.  On a machine WITH a device they would launch on the dummy pointers, so this row is
# checked where the device check answers -2.
@pytest.mark.skipif(torch.cuda.is_available(), reason="good arguments with dummy pointers must stop at the device check")
def test_good_arguments_get_as_far_as_the_device(pkg):
    L, sse, sse_grad, soft, soft_grad = _calls(pkg)
    for call in (sse, sse_grad, soft, soft_grad):
        assert call() == NO_DEVICE
        for R in (4, 12, 64, 128):
            for dtype in (0, 1, 2):
                for layout in (0, 1):
                    assert call(R=R, dtype=dtype, layout=layout) == NO_DEVICE
        assert call(J=1) == NO_DEVICE and call(J=170) == NO_DEVICE and call(n=98688, J=170) == NO_DEVICE
        assert call(pred=ctypes.c_void_p(80), u=odd4) == NO_DEVICE
        for s in (1e-30, 0.5, 4.0, 8.0, 3e38):
            assert call(scalar=s) == NO_DEVICE
    assert sse(status=null, valid=null) == NO_DEVICE and sse_grad(status=null) == NO_DEVICE      # the optional ones
    assert sse(out=odd8) == NO_DEVICE and soft(out=odd8) == NO_DEVICE and soft_grad(stats=odd8) == NO_DEVICE   # 8 bytes do
    assert sse_grad(out=one, pred=one) == NO_DEVICE and soft_grad(out=one, pred=one) == NO_DEVICE  # in place
    P = pkg._lib.load()
    for R in range(-8, 264):
        assert (sse(R=R) == INVALID) == (soft_grad(R=R) == INVALID) == (not P.tsdf_resolution_supported(R)), R


# ---- sanitizer child ----
def test_host_code_under_sanitizers_as_a_stand_alone_program():
    subprocess.check_call(["make", "-C", CSRC, "-B", "heatloss-host-asan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "build", "heatloss_host_asan")
    env = dict(os.environ)
    env.update(ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    # every quad of every volume, R = 4..128 in steps of 4, as 4- and as 8-element pieces: 2 * sum(R^3) / 4
    assert f"heatloss host code ok ({sum(R ** 3 for R in range(4, 129, 4)) // 2} quads)" in r.stdout, tail
    assert "Sanitizer" not in tail and "runtime error" not in tail and "FAILED" not in tail, tail


def test_the_library_includes_the_same_text():
    """The library and the stand-alone program compile ONE text of the rules: heatloss_host.inc on top of heatmap_host.inc,
    which takes the three tests that exist already (bad_res, misaligned, bad_dtype) from its includer."""
    unit = open(os.path.join(CSRC, "tsdf_heatloss.hip")).read()
    inc, main = (open(os.path.join(CSRC, f)).read() for f in ("heatloss_host.inc", "heatloss_host_main.cc"))
    theirs = open(os.path.join(CSRC, "device.inc")).read().splitlines() + open(os.path.join(CSRC, "narrow.inc")).read().splitlines()
    for name in ("bad_res", "misaligned", "bad_dtype"):
        (line,) = [ln for ln in main.splitlines() if re.search(rf"\bbool {name}\(", ln)]
        assert line in theirs, name
        assert not re.search(rf"\bbool {name}\(", inc), name
    order = [unit.index(f'#include "{f}"') for f in ("device.inc", "narrow.inc", "heatmap_host.inc", "heatloss_host.inc")]
    assert order == sorted(order)
    assert main.index('#include "heatmap_host.inc"') < main.index('#include "heatloss_host.inc"')
    for name in ("heat_defect_sse(", "heat_defect_sse_grad(", "heat_defect_soft_argmax(", "heat_defect_soft_argmax_grad(",
                 "heat_quad(", "heat_plan(", "heat_item("):
        assert name in unit and name in main, name
    assert "#include" not in inc and "__global__" not in inc and "hipLaunch" not in inc           # plain C++, no device code


# ---- restatement properties ----
def _torch_target(u, status, R, sigma, layout):
    heat, valid = hr.encode(u, status, R, sigma, layout)
    return heat, valid


@pytest.mark.parametrize("R", [4, 12])
def test_loss_gradient_is_the_autograd_of_its_forward(R):
    """sse_grad against torch CPU float64 autograd of L = sum_units c_unit * sum((pred - t)^2).  autograd forms
    c * (2 * d) or (c * 2) * d where the restatement forms (2 c) * d with d the same float64 difference: 2 c is exact, so
    the two differ by at most one rounding of a product, |delta| <= 2^-52 |ref| (2 u), taken as 4 u for the order autograd
    may choose.  The forward: sum in another order, N u relative with N = R^3."""
    n, J = 2, 3
    rng = np.random.default_rng(R)
    for layout in hr.LAYOUTS:
        u = rng.uniform(0.1, 0.9, (n, J, 3)).astype(np.float32)
        u[1, 2, 0] = np.nan
        t32, valid = _torch_target(u, None, R, 1.3, layout)
        pred = (rng.standard_normal((n, J, R, R, R)).astype(np.float32) + t32).astype(np.float32)
        c = rng.uniform(0.5, 2.0, (n, J)).astype(np.float32).astype(np.float64)     # so that w = 2 c is a float32 exactly
        w = (2.0 * c).astype(np.float32)
        p = torch.from_numpy(pred).double().requires_grad_()
        ok = torch.from_numpy(valid != 0)
        per = ((p - torch.from_numpy(t32).double()) ** 2).reshape(n, J, -1).sum(dim=2)
        per = torch.where(ok, per, torch.zeros_like(per))
        (per * torch.from_numpy(c)).sum().backward()
        ref = lr.sse_grad(pred, t32, valid, w, exact=True)
        got = p.grad.numpy()
        assert (np.abs(got - ref) <= 4 * lr.U * np.abs(ref)).all()
        assert not ref[1, 2].any() and ref[0, 0].any()
        s = lr.sse(pred, t32, valid)
        assert (np.abs(s - per.detach().numpy()) <= R ** 3 * lr.U * s).all() and s[1, 2] == 0
        assert np.array_equal(lr.sse_grad(pred, t32, valid, w), ref.astype(np.float32))
        assert not lr.sse_grad(pred, t32, valid, np.full((n, J), np.nan))[1, 2].any()      # +0 under a NaN w


@pytest.mark.parametrize("R", [4, 12])
def test_soft_argmax_gradient_is_the_autograd_of_its_forward(R):
    """soft_argmax_grad against torch CPU float64 autograd of u = (sum(softmax(beta h) i_a) + 0.5) / R contracted with gu.
    Both are float64; they differ by the order of sums of N = R^3 <= 1728 terms (N u relative in Z and in the moments, so
    N u R absolute in c_a) and by autograd's own form i_a q_i - c_a q_i, whose cancellation leaves an ABSOLUTE error of a
    few u (i_a + c_a) q_i.  Hence per voxel |delta| <= 4 (N + 16) u * beta q_i sum_a |gu_a| (i_a + c_a + 1) / R — about
    1e-12 relative to the gradient's own scale beta q_i |gu| — and u itself within 4 N u."""
    n, J, N = 2, 3, R ** 3
    rng = np.random.default_rng(100 + R)
    for layout in hr.LAYOUTS:
        for beta in (0.5, 1.0, 8.0):
            h = rng.standard_normal((n, J, R, R, R)).astype(np.float32)
            gu = rng.standard_normal((n, J, 3)).astype(np.float32)
            u, stats = lr.soft_argmax(h, R, beta, layout)
            ref = lr.soft_argmax_grad(h, stats, gu, R, beta, layout, exact=True)
            idx = [torch.from_numpy(i) for i in lr._indices(R, layout)]
            t = torch.from_numpy(h).double().requires_grad_()
            q = torch.softmax(float(np.float32(beta)) * t.reshape(n * J, -1), dim=1)
            tu = torch.stack([((q * i).sum(dim=1) + 0.5) / R for i in idx], dim=1).reshape(n, J, 3)
            (tu * torch.from_numpy(gu).double()).sum().backward()
            assert np.abs(tu.detach().numpy() - u.astype(np.float64)).max() <= 2.0 ** -24 + 4 * N * lr.U
            qn = q.detach().numpy().reshape(n * J, -1)
            c = stats.reshape(n * J, 5)[:, 2:]
            scale = sum(np.abs(gu.reshape(n * J, 3)[:, a:a + 1].astype(np.float64)) * (lr._indices(R, layout)[a][None] + c[:, a:a + 1] + 1)
                        for a in range(3))
            tol = 4 * (N + 16) * lr.U * float(np.float32(beta)) * qn * scale / R
            err = np.abs(t.grad.numpy().reshape(n * J, -1) - ref.reshape(n * J, -1))
            print(f"R={R} {layout} beta={beta}: worst error / bound {float((err / tol).max()):.3g}")
            assert (err <= tol).all()
            assert np.array_equal(lr.soft_argmax_grad(h, stats, gu, R, beta, layout), ref.astype(np.float32))


def test_non_finite_volumes_and_empty_batches_of_the_restatement():
    R = 4
    h = np.zeros((1, 5, R, R, R), np.float32)
    h[0, 0, 1, 2, 3] = np.nan                  # one NaN
    h[0, 1] = -np.inf                          # all -inf: the maximum is not finite
    h[0, 2, 0, 0, 0] = np.inf                  # a +inf
    h[0, 3] = np.nan                           # NaNs alone: m = -inf
    h[0, 4, 3, 1, 2] = 40.0                    # hand-checkable
    for layout in hr.LAYOUTS:
        u, stats = lr.soft_argmax(h, R, 8.0, layout)
        assert np.isnan(u[0, :4]).all() and np.isnan(stats[0, :4, 1:]).all()
        assert stats[0, 0, 0] == 0.0 and stats[0, 1, 0] == -np.inf and stats[0, 2, 0] == np.inf and stats[0, 3, 0] == -np.inf
        want = ((np.array([2, 1, 3] if layout == "czyx" else [3, 1, 2]) + 0.5) / R).astype(np.float32)
        assert np.array_equal(u[0, 4], want) and stats[0, 4, 0] == 40.0     # exp(-320) vanishes against 1
        assert np.array_equal(u[0, 4], hr.decode(h[:, 4:5], R, layout, 0)[0][0, 0])
    # "mean" over no valid unit: 0 loss, 0 w; over some: the valid ones' voxels
    sse, valid = np.zeros((2, 3)), np.zeros((2, 3), np.int32)
    loss, factor = lr.reduce(sse, valid, 8, "mean")
    assert loss == 0.0 and not factor.any() and not lr.weights(1.0, factor).any()
    sse, valid = np.array([[512.0, 0.0, 1024.0]]), np.array([[1, 0, 1]], np.int32)
    loss, factor = lr.reduce(sse, valid, 8, "mean")
    assert loss == 1.5 and np.array_equal(factor, [[2 / 1024, 0, 2 / 1024]])
    assert lr.reduce(sse, valid, 8, "sum")[0] == 1536.0 and np.array_equal(lr.reduce(sse, valid, 8, "sum")[1], [[2, 0, 2]])
    per, factor = lr.reduce(sse, valid, 8, "none")
    assert np.array_equal(per, [[1.0, 0.0, 2.0]]) and np.array_equal(lr.weights(np.ones((1, 3)), factor), np.float32([[2 / 512, 0, 2 / 512]]))


def test_wrapper_reduction_is_the_restatements(pkg):
    """_heat_reduce (torch ops; here on the CPU) against lr.reduce: the same float64 operations."""
    V = importlib.import_module(pkg.__name__ + ".voxelize")
    rng = np.random.default_rng(8)
    for valid in (np.zeros((3, 4), np.int32), (rng.random((3, 4)) < 0.7).astype(np.int32)):
        sse = rng.uniform(1, 100, (3, 4)) * valid
        for reduction in ("mean", "sum", "none"):
            loss, factor = V._heat_reduce(torch.from_numpy(sse), torch.from_numpy(valid), 12, reduction)
            rl, rf = lr.reduce(sse, valid, 12, reduction)
            assert np.allclose(loss.numpy(), rl, rtol=4 * lr.U, atol=0) and np.array_equal(factor.numpy(), rf), reduction
            assert loss.dtype is torch.float64 and factor.shape == (3, 4)


# ---- Python wrappers ----
def test_public_names_and_refusals(pkg, monkeypatch):
    V = importlib.import_module(pkg.__name__ + ".voxelize")

    def no_call(*a, **kw):
        raise AssertionError("an entry was called")

    monkeypatch.setattr(V, "_call", no_call)
    for name in ("heatmap_mse_loss", "soft_argmax_joints"):
        assert name in pkg.__all__ and hasattr(pkg, name) and name in pkg.__doc__, name
    assert "tsdf_heatloss.h" in pkg.__doc__ and "libtsdf_heatloss.so" in pkg.__doc__
    pred = torch.zeros((2, 3, 8, 8, 8))
    u = torch.full((2, 9), 0.5)
    # there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        pkg.heatmap_mse_loss(pred, u)
    with pytest.raises(ValueError, match="GPU"):
        pkg.soft_argmax_joints(pred)
    # and everything else is judged before anything could be launched
    for bad in (pred.double(), pred.to(torch.int16)):
        with pytest.raises(ValueError, match="float32, torch.float16 or torch.bfloat16"):
            pkg.heatmap_mse_loss(bad, u)
        with pytest.raises(ValueError, match="float32, torch.float16 or torch.bfloat16"):
            pkg.soft_argmax_joints(bad)
    for bad in (0, 0.0, -1.0, nan, inf, 1e-50, "1.7", None):
        with pytest.raises(ValueError, match="sigma"):
            pkg.heatmap_mse_loss(pred, u, sigma=bad)
        with pytest.raises(ValueError, match="beta"):
            pkg.soft_argmax_joints(pred, beta=bad)
    for fn in (lambda: pkg.heatmap_mse_loss(pred, u, layout="xyzc"), lambda: pkg.soft_argmax_joints(pred, layout="xyzc")):
        with pytest.raises(ValueError, match="layout"):
            fn()
    for bad in ("avg", "", None, "Mean", 0):
        with pytest.raises(ValueError, match="reduction"):
            pkg.heatmap_mse_loss(pred, u, reduction=bad)
    for fn in (lambda: pkg.soft_argmax_joints(pred.numpy()), lambda: pkg.heatmap_mse_loss(pred.numpy(), u),
               lambda: pkg.heatmap_mse_loss(pred, u.numpy()), lambda: pkg.heatmap_mse_loss(pred, u, status=[0, 0])):
        with pytest.raises(ValueError, match="torch.Tensor|GPU"):
            fn()
