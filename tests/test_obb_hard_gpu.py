"""GPU tier of the principal-axis maps on hard inputs: tsdf_obb_kernel on the frame zoo (tests/frame_zoo.py: frames of 1-3
rows, one column, rows of up to 640 columns — a lane's second and third group —, 480 rows, N = 1 and 2) and on the spectrum
list of tests/obb_ref.py (tied, vanishing and ill-conditioned eigenvalues, three valid pixels, depths of 1e30, infinite
depths), which tests/test_obb_gpu.py asserts its own inputs away from.

Where eigenvalues tie, the axes within the eigenspace are anybody's; what is asserted holds whatever axes the kernel picks:
the bounds of tests/test_obb_gpu.py::check_frame (moments, Weyl, orthonormality, det and signs, the diagonalised covariance,
inverse = transpose, the centroid a fixed point), and the Davis-Kahan comparison of the axes themselves only where the
relative gaps are at least 1e-3.  Then the map the GPU chose is used: voxelize_obb against the oracle under that very map,
and the joints' round trip.  No bound is restated here."""
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_zoo as fz  # noqa: E402
import obb_ref as ob  # noqa: E402
from test_obb_gpu import TOL, check_frame, run, up  # noqa: E402

pytestmark = pytest.mark.gpu


def check_every_frame(got, ref, names):
    """Status and count exact; every OK frame through check_frame, its axes compared where the gaps allow."""
    assert got.status.tolist() == [f["status"] for f in ref]
    assert got.count.tolist() == [f["N"] for f in ref]
    compared = 0
    for i, f in enumerate(ref):
        if f["status"] != 0:
            assert np.array_equal(got.xforms[i], ob.identity()), names[i]
            assert not got.mean[i].any() and not got.cov[i].any() and not got.eigenvalues[i].any(), names[i]
            continue
        axes = min(ob.rel_gaps(f["lam"])) >= 1e-3
        compared += axes
        print(names[i], end=": ")
        check_frame(got, i, f, compare_axes=bool(axes))
    return compared


def test_the_zoo_through_obb_xforms(pkg):
    z = fz.zoo()
    depth, off, hdr = (a.copy() for a in fz.master(len(z)))          # (the master batch is read-only)
    ref = ob.batch(depth, off, hdr)
    # what the zoo brings, on the reference
    shapes = [e.img.shape for e in z]
    assert {f["N"] for f in ref if f["status"] == 1} & {1, 2}
    assert any(f["status"] == 0 and bh == 1 for f, (bh, bw) in zip(ref, shapes))            # one row: rank <= 2
    assert any(f["status"] == 0 and bw == 1 for f, (bh, bw) in zip(ref, shapes))            # one column
    assert any(f["status"] == 0 and 321 <= bw <= 640 for f, (bh, bw) in zip(ref, shapes))   # a second g += 64 visit
    assert any(f["status"] == 0 and bh == 480 for f, (bh, bw) in zip(ref, shapes))
    assert any(f["status"] == 0 and bh <= 3 for f, (bh, bw) in zip(ref, shapes))
    got = run(pkg, depth, off, hdr)                                                         # all 230 frames, one launch
    compared = check_every_frame(got, ref, [e.name for e in z])
    ok = sum(f["status"] == 0 for f in ref)
    print(f"zoo: {ok} OK frames, axes compared on {compared}")
    assert 0 < compared < ok                                                                # both branches ran


@pytest.fixture(scope="module")
def spectrum(pkg):
    depth, off, hdr = ob.spectrum_pack()
    return depth, off, hdr, ob.batch(depth, off, hdr), run(pkg, depth, off, hdr)


def test_the_spectrum_list_through_obb_xforms(pkg, spectrum):
    depth, off, hdr, ref, got = spectrum
    names = [e[0] for e in ob.spectrum()]
    k = names.index("huge")
    # the 1e30 frame in millimetres of its own: every length times 2^-91, exactly, so that check_frame's one absolute
    # figure (the fixed point within 1e-9) means what it means for every other frame
    s = 1.0 / ob.HUGE
    xf = got.xforms.copy()
    xf[k, 3::4] *= s
    mean, cov, lam = got.mean.copy(), got.cov.copy(), got.eigenvalues.copy()
    mean[k], cov[k], lam[k] = mean[k] * s, cov[k] * s * s, lam[k] * s * s
    assert np.isfinite(got.xforms[k]).all() and np.abs(got.mean[k, 2]) > 1e29
    scaled = pkg.ObbBatch(xf, got.status, got.count, mean, cov, lam)
    ref = list(ref)
    ref[k] = ob.rescaled(ref[k], s)
    compared = check_every_frame(scaled, ref, names)
    assert compared >= 3
    # the ties the kernel broke: one axis carries the line, the constant-depth plane has no extent along its third axis
    i = names.index("three_collinear")
    assert got.eigenvalues[i, 1] <= 64 * ob.U * got.eigenvalues[i, 0] and abs(got.xforms[i, 0]) >= 1 - 64 * ob.U
    for name in ("plane_const", "square_centred"):
        i = names.index(name)
        assert abs(got.xforms[i, 10]) >= 1 - 64 * ob.U and got.eigenvalues[i, 2] <= 64 * ob.U * got.eigenvalues[i, 0]


@pytest.mark.parametrize("R", [8, 20])
def test_the_map_the_gpu_chose_is_used(pkg, spectrum, R):
    depth, off, hdr, ref, got = spectrum
    n = len(hdr)
    mu = np.stack([f["mu"] for f in ref])
    gt = (mu[:, None, :] + np.random.default_rng(9).normal(0, 40, (n, 21, 3))).astype(np.float32).reshape(n, 63)
    td, to, th = up(depth, off, hdr)
    out, nor, gobb, xf = pkg.voxelize_obb(td, to, th, res=R, gt=up(gt)[0])
    torch.cuda.synchronize()
    assert np.array_equal(xf.cpu().numpy().view(np.uint64), got.xforms.view(np.uint64))
    want = oracle.voxelize_aug(depth, off, hdr, got.xforms, R=R, layout=0, n_threads=8)
    status = out.status.cpu().numpy()
    print(f"R={R}: status {status.tolist()}")
    np.testing.assert_array_equal(status, want["status"])
    np.testing.assert_array_equal(out.max_l.cpu().numpy(), want["max_l"])
    np.testing.assert_array_equal(out.mid_p.cpu().numpy(), want["mid_p"])
    err = np.abs(out.tsdf.cpu().numpy() - want["tsdf"]).reshape(n, -1).max(axis=1)
    print(f"R={R}: max volume error per frame {err}")
    assert err.max() <= TOL
    assert (status[[f["status"] == 0 and np.abs(f["mu"]).max() < 1e6 for f in ref]] == 0).all()
    np.testing.assert_array_equal(gobb.cpu().numpy(), oracle.transform_joints(gt, got.xforms))
    # the round trip of the joints through the map and its inverse, float64
    # (the 1e30 frame in its own millimetres, as above)
    for i, f in enumerate(ref):
        if f["status"] == 0:
            s = 1.0 / ob.HUGE if np.abs(f["mu"]).max() > 1e6 else 1.0
            m = got.xforms[i].copy()
            m[3::4] *= s
            j = gt[i].reshape(21, 3).astype(np.float64) * s
            back = ob.apply(m, ob.apply(m, j), inverse=True)
            assert np.abs(back - j).max() <= 1e-9, i
