"""GPU tier of the principal-axis maps (include/tsdf_obb.h): tsdf_obb_kernel against the numpy restatement
(tests/obb_ref.py) within a-priori bounds, the edge frames and their status, independence of the batch and determinism,
the volumes of voxelize_obb against voxelize_aug and the oracle, the round trip, ResidentLoader(frame="obb") and capture
into a graph."""
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obb_ref as ob  # noqa: E402

pytestmark = pytest.mark.gpu

U = ob.U
TOL = 1e-5          # volumes against the oracle: the tolerance of tests/test_parity_gpu.py::test_augmented_entry
W, H = 320, 240


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
    return depth, off.astype(np.int64), hdr


def run(pkg, depth, off, hdr, **kw):
    """obb_xforms on numpy inputs; every field as a numpy array."""
    r = pkg.obb_xforms(*up(depth, off, hdr), **kw)
    torch.cuda.synchronize()
    return pkg.ObbBatch(*(t.cpu().numpy() for t in r))


@pytest.fixture(scope="module")
def crops(synth):
    return synth.synth_batch(24, "crop", seed0=42)


@pytest.fixture(scope="module")
def frames27(synth, crops):
    """The 24 crops (odd widths: unaligned rows and frames) and 3 of the full frames (320 columns: more than one visit
    per wave), their restatement and joints near every centroid."""
    fd, fo, fh = synth.synth_batch(12, "full", seed0=42)
    depth, off, hdr = concat([crops, (fd[:fo[3]], fo[:4], fh[:3])])
    ref = ob.batch(depth, off, hdr)
    mu = np.stack([f["mu"] for f in ref])
    gt = (mu[:, None, :] + np.random.default_rng(7).normal(0, 40, (len(ref), 21, 3))).astype(np.float32).reshape(-1, 63)
    return depth, off, hdr, ref, gt


def check_frame(got, i, f, compare_axes=True):
    """The a-priori bounds of one OK frame: u = 2^-53, N the valid count.  Any-order float64 summation of N terms is within
    gamma_N ~ N u of the exact sum; 4 N u leaves a factor for the centring and the products (and the restatement's own
    error)."""
    N, tr = f["N"], np.trace(f["C"])
    assert got.status[i] == 0 and f["status"] == 0
    assert got.count[i] == N
    scale = np.abs(f["pts"]).max()
    err_mu = np.abs(got.mean[i] - f["mu"]).max()
    tolC = 4 * N * U * tr
    err_C = np.abs(got.cov[i] - ob.cov6(f["C"])).max()
    err_l = np.abs(got.eigenvalues[i] - f["lam"]).max()
    A = got.xforms[i, :12].reshape(3, 4)[:, :3]
    err_o = np.abs(A @ A.T - np.eye(3)).max()
    print(f"frame {i}: N {N} mu {err_mu:.3g}/{4 * N * U * scale:.3g} C {err_C:.3g}/{tolC:.3g} lam {err_l:.3g} orth {err_o / U:.3g} u")
    assert err_mu <= 4 * N * U * scale
    assert err_C <= tolC
    assert err_l <= 3 * tolC + 64 * U * tr                       # Weyl
    assert err_o <= 256 * U                                      # at most 36 rotations of a few u each, with a margin
    assert np.linalg.det(A) > 0 and A[0, 1] >= 0 and A[2, 2] >= 0
    assert list(got.eigenvalues[i]) == sorted(got.eigenvalues[i], reverse=True)
    # the map is the rotation about the centroid, and the second half its inverse
    Ai = got.xforms[i, 12:].reshape(3, 4)[:, :3]
    assert np.array_equal(Ai, A.T)
    assert np.abs(ob.apply(got.xforms[i], got.mean[i][None]) - got.mean[i]).max() <= 1e-9
    # A diagonalises the covariance: Jacobi stops at an off-diagonal norm of u trace, its <= 36 rotations each add a few
    # u trace, and C itself is within tolC
    D = A @ f["C"] @ A.T
    assert np.abs(D - np.diag(np.diag(D))).max() <= 6 * tolC + 1024 * U * tr
    if compare_axes:
        g1, g2 = f["lam"][0] - f["lam"][1], f["lam"][1] - f["lam"][2]
        gap = min(g1, g2)
        err_A = np.abs(A - f["A"]).max()
        print(f"         axes {err_A:.3g}/{6 * tolC / gap:.3g}")
        assert err_A <= 6 * tolC / gap                           # Davis-Kahan


def test_moments_and_maps_against_the_restatement(pkg, frames27):
    depth, off, hdr, ref, gt = frames27
    # conditions on the inputs, asserted on the restatement
    for f in ref:
        assert f["status"] == 0
        assert min(ob.rel_gaps(f["lam"])) >= 1e-3 and abs(f["A"][0, 1]) >= 1e-6 and abs(f["A"][2, 2]) >= 1e-6
    assert sum(int(h[4] - h[2]) % 4 != 0 for h in hdr) >= 10 and sum(int(o) % 4 != 0 for o in off[:-1]) >= 10
    got = run(pkg, depth, off, hdr)
    for i, f in enumerate(ref):
        check_frame(got, i, f)
        j = gt[i].reshape(21, 3).astype(np.float64)
        back = ob.apply(got.xforms[i], ob.apply(got.xforms[i], j), inverse=True)
        assert np.abs(back - j).max() <= 1e-9


def _crop(left, top, img):
    img = np.asarray(img, np.float32)
    h, w = img.shape
    return img.reshape(-1), np.array([0, h * w], np.int64), np.array([[W, H, left, top, left + w, top + h]], np.int32)


def test_edge_frames(pkg):
    rng = np.random.default_rng(11)
    nan = np.float32(np.nan)
    two = np.zeros((3, 3), np.float32)
    two[0, 1], two[2, 2] = 480.0, 510.0
    mixed = (450.0 + 40.0 * rng.random((9, 11))).astype(np.float32)
    mixed.reshape(-1)[::3] = [0.0, 0.5, -0.99, nan] * 8 + [0.0]
    parts = [
        _crop(100, 90, [[500.0]]),                                              # 0  1 x 1: N = 1
        _crop(40, 50, two),                                                     # 1  2 valid pixels
        _crop(158, 30, [[500.0, 0.0, 500.0, 0.0, 500.0]]),                      # 2  3 collinear points: rank 1, OK
        _crop(7, 121, 400.0 + 100.0 * rng.random((1, 17))),                     # 3  one row
        _crop(301, 5, 400.0 + 100.0 * rng.random((13, 1))),                     # 4  one column
        _crop(120, 100, mixed),                                                 # 5  valid pixels among 0, 0.5, -0.99, NaN
        _crop(10, 10, np.array([[0.0, 0.5, nan], [-0.99, 0.0, 0.25]])),         # 6  all invalid
        _crop(60, 60, np.full((4, 5), nan)),                                    # 7  area != payload (header edited below)
        _crop(80, 80, np.full((3, 3), nan)),                                    # 8  right <= left (edited below)
        _crop(200, 100, 450.0 + 30.0 * rng.random((6, 7))),                     # 9  payload outside depth_len
    ]
    depth, off, hdr = concat(parts)
    hdr[7, 4] += 1
    hdr[8, 4] = hdr[8, 2]
    cut = depth[:off[9] + 5]                                                    # frame 9's payload ends past the buffer
    want_status = [1, 1, 0, 0, 0, 0, 1, 2, 2, 2]
    want_N = [1, 2, 3, 17, 13, 99 - 33, 0, 0, 0, 0]
    got = run(pkg, cut, off, hdr)
    assert list(got.status) == want_status
    assert list(got.count) == want_N
    ref = ob.batch(depth, off, hdr, depth_len=len(cut))
    assert [f["status"] for f in ref] == want_status and [f["N"] for f in ref] == want_N
    ident = ob.identity()
    for i, st in enumerate(want_status):
        if st:
            assert np.array_equal(got.xforms[i], ident), i
            assert not got.mean[i].any() and not got.cov[i].any() and not got.eigenvalues[i].any(), i
        else:
            # a line or a plane has eigenvalues that coincide (at 0): the axes within that eigenspace are anybody's, so
            # the properties are checked, not the restatement's choice
            check_frame(got, i, ref[i], compare_axes=False)
    # the collinear frame: one direction carries everything, and it is the first axis
    assert got.eigenvalues[2, 1] <= 64 * U * got.eigenvalues[2, 0] and abs(got.xforms[2, 0]) >= 1 - 64 * U


def test_independence_of_the_batch_and_determinism(pkg, crops):
    depth, off, hdr = crops
    n0 = len(hdr)
    alone = []
    for i in range(n0):
        r = pkg.obb_xforms(*up(depth[off[i]:off[i + 1]], np.array([0, off[i + 1] - off[i]], np.int64), hdr[i:i + 1]))
        alone.append(r)
    reps = [(depth, off, hdr)] * 13
    bd, bo, bh = concat(reps)
    n = 300                                                    # more frames than the device has CUs
    bd, bo, bh = bd[:bo[n]], bo[:n + 1], bh[:n]
    td, to, th = up(bd, bo, bh)
    big = pkg.obb_xforms(td, to, th)
    again = pkg.obb_xforms(td, to, th)
    torch.cuda.synchronize()
    assert not bool(big.status.any())
    pick = torch.arange(n, device=dev()) % n0

    def bits(t):
        t = t.contiguous()
        return t.view(torch.int64) if t.dtype is torch.float64 else t

    for k, name in enumerate(big._fields):
        want = torch.cat([a[k] for a in alone])[pick]           # every copy: the frame computed alone
        assert torch.equal(bits(big[k]), bits(want)), name
        assert torch.equal(bits(big[k]), bits(again[k])), name
    out = torch.full((n, 24), -7.0, dtype=torch.float64, device=dev())
    r = pkg.obb_xforms(td, to, th, out=out)
    torch.cuda.synchronize()
    assert r.xforms is out and torch.equal(out, big.xforms)
    with pytest.raises(ValueError):
        pkg.obb_xforms(td, to, th, out=out[:5])
    empty = pkg.obb_xforms(td[:0], to[:1], th[:0])
    assert empty.xforms.shape == (0, 24) and empty.cov.shape == (0, 6)


def test_volumes_labels_and_round_trip(pkg, frames27):
    depth, off, hdr, _, gt = frames27
    depth, off, hdr, gt = depth[:off[24]], off[:25], hdr[:24], gt[:24]       # the crops
    td, to, th, tg = up(depth, off, hdr, gt)
    xf = pkg.obb_xforms(td, to, th).xforms
    xf_np = xf.cpu().numpy()
    want_obb = oracle.transform_joints(gt, xf_np)
    for R in (32, 16):
        for layout in ("czyx", "cxyz"):
            out, nor, gobb, xf2 = pkg.voxelize_obb(td, to, th, res=R, layout=layout, gt=tg)
            want, want_nor, want_g = pkg.voxelize_aug(td, to, th, xf, res=R, layout=layout, gt=tg)
            bare, xf3 = pkg.voxelize_obb(td, to, th, res=R, layout=layout)
            torch.cuda.synchronize()
            assert torch.equal(xf2, xf) and torch.equal(xf3, xf)
            for a, b, c in zip(out, want, bare):
                assert torch.equal(a, b) and torch.equal(a, c)
            assert torch.equal(nor, want_nor) and torch.equal(gobb, want_g)
            ref = oracle.voxelize_aug(depth, off, hdr, xf_np, R=R, layout=0 if layout == "czyx" else 1, n_threads=8)
            np.testing.assert_array_equal(out.status.cpu().numpy(), ref["status"])
            assert not ref["status"].any()
            np.testing.assert_array_equal(out.max_l.cpu().numpy(), ref["max_l"])
            np.testing.assert_array_equal(out.mid_p.cpu().numpy(), ref["mid_p"])
            err = np.abs(out.tsdf.cpu().numpy() - ref["tsdf"]).max()
            print(f"R={R} {layout}: max volume error {err:.3g}")
            assert err <= TOL
            np.testing.assert_array_equal(gobb.cpu().numpy(), want_obb)
            np.testing.assert_array_equal(nor.cpu().numpy(), oracle.normalize_joints(want_obb, ref["max_l"], ref["mid_p"]))
    # a rigid map: the distances between joints are those of the camera frame, to the float32 rounding of the mapped
    # coordinates (|coordinate| < 1024 mm: 2^-24 * 1024 each, two of them per difference, three differences per distance)
    a = gt.reshape(24, 21, 3).astype(np.float64)
    b = want_obb.reshape(24, 21, 3).astype(np.float64)
    assert np.abs(b).max() < 1024
    da = np.linalg.norm(a[:, :, None] - a[:, None], axis=-1)
    db = np.linalg.norm(b[:, :, None] - b[:, None], axis=-1)
    assert np.abs(da - db).max() <= 2 * np.sqrt(3) * 2.0 ** -24 * 1024
    # round trip to the camera frame
    back = pkg.transform_joints(gobb, pkg.invert_xforms(xf))
    assert float((back - tg).abs().max()) <= 1e-3


def _batch_tensors(b):
    return [t.clone() for t in b if t is not None]


@pytest.mark.parametrize("prefetch", [1, 2])
def test_resident_loader_in_the_obb_frame(pkg, synth, prefetch):
    d = dev()
    N = 40
    depth, off, hdr = synth.synth_batch(N, "crop", seed0=9100)
    gt = np.random.default_rng(3).normal(0, 90, (N, 63)).astype(np.float32)
    pk = pkg.packing.PackedFrames(depth, off, hdr, gt)
    ds = pkg.MSRADepthDataset.from_packs([pk])
    ld = pkg.ResidentLoader(ds, batch_size=16, device=d, shuffle=True, seed=4, prefetch=prefetch, frame="obb")
    plan = ld._batches()
    got = [_batch_tensors(b) for b in ld]
    torch.cuda.synchronize()
    assert [len(b) for b in plan] == [16, 16, 8] and len(got) == 3
    whole = pkg.obb_xforms(*up(depth, off, hdr))
    assert torch.equal(ld.obb, whole.xforms) and torch.equal(ld.obb_status, whole.status)
    assert ld.obb.shape == (N, 24) and not bool(ld.obb_status.any())
    for b, have in zip(plan, got):
        sub = pk.take(ld._g[b])
        sd, so, sh, sg = up(sub.depth, sub.offsets, sub.headers, sub.gt)
        out, nor, gobb, xf = pkg.voxelize_obb(sd, so, sh, res=32, gt=sg)
        assert torch.equal(xf, ld.obb[torch.from_numpy(ld._g[b]).to(d)])
        want = pkg.VoxelBatch(out.tsdf, gobb, out.max_l, out.mid_p, out.status, nor)
        for name, x, y in zip(want._fields, want, have):
            assert torch.equal(x, y), name
    # frame="camera" is the loader as it is without the argument
    cam = [_batch_tensors(b) for b in pkg.ResidentLoader(ds, batch_size=16, device=d, shuffle=True, seed=4,
                                                         prefetch=prefetch, frame="camera")]
    today = [_batch_tensors(b) for b in pkg.ResidentLoader(ds, batch_size=16, device=d, shuffle=True, seed=4,
                                                           prefetch=prefetch)]
    for b, x, y in zip(plan, cam, today):
        sub = pk.take(ld._g[b])
        sd, so, sh, sg = up(sub.depth, sub.offsets, sub.headers, sub.gt)
        out, nor = pkg.voxelize_labels(sd, so, sh, sg)
        for u, v in zip(x, y):
            assert torch.equal(u, v)
        assert torch.equal(x[0], out.tsdf) and torch.equal(x[1], sg) and torch.equal(x[5], nor)
    assert not torch.equal(cam[0][0], got[0][0])               # the other frame is another volume


def test_capture_into_a_graph(pkg, synth):
    """obb_xforms then voxelize_aug, a straight chain of two launches, captured once and replayed on new depth."""
    d = dev()
    n, R = 8, 32
    depth, off, hdr = synth.synth_batch(n, "crop", seed0=42)
    rng = np.random.default_rng(5)
    variants = [depth, (depth * (1 + 0.05 * rng.random(depth.shape)) * (depth != 0)).astype(np.float32),
                (depth + 25.0 * (depth != 0)).astype(np.float32)]
    td, to, th = up(depth, off, hdr)
    xf = torch.empty((n, 24), dtype=torch.float64, device=d)
    out = pkg.empty_batch(n, R, d)

    def step():
        pkg.voxelize_aug(td, to, th, pkg.obb_xforms(td, to, th, out=xf).xforms, res=R, out=out)

    step()                                   # eagerly once: library loads and the device check happen here
    torch.cuda.synchronize()
    side = torch.cuda.Stream(d)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    for v in variants[1:]:
        td.copy_(torch.from_numpy(v))
        g.replay()
        torch.cuda.synchronize()
        have = [t.clone() for t in (xf, *out)]
        e_xf = pkg.obb_xforms(td, to, th).xforms
        e_out = pkg.voxelize_aug(td, to, th, e_xf, res=R)
        torch.cuda.synchronize()
        for x, y in zip(have, (e_xf, *e_out)):
            assert torch.equal(x, y)
    assert not torch.equal(have[0], pkg.obb_xforms(*up(depth, off, hdr)).xforms)   # the depth did change the maps
