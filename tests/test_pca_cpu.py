"""CPU tier: the joint-PCA fit, its file formats, the projection / decode restatement (tests/pca_ref.py), the
cal_out pin, argument validation of the new C entries before any device work, and export's nine fold fits."""
import ctypes
import importlib
import os

import numpy as np
import pytest

import pca_ref

PKG = "handposeestimation-with-3d-cnns_amd"


@pytest.fixture(scope="module")
def P():
    return importlib.import_module(PKG + ".pca")


def _separated(n=400, C=63, seed=0):
    """Data with well-separated component variances."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(C, C)))
    scales = 0.2 * 0.9 ** np.arange(C)
    z = rng.normal(size=(n, C)) * scales
    return (0.5 + z @ q.T).astype(np.float32)


def test_fit_matches_svd_up_to_sign_rule(P):
    u = _separated()
    pca = P.fit_labels(u, fold=3)
    x = u.astype(np.float64)
    xc = x - x.mean(0)
    _, s, vt = np.linalg.svd(xc, full_matrices=False)
    v = vt.T
    big = np.argmax(np.abs(v), axis=0)
    v = v * np.where(v[big, np.arange(v.shape[1])] < 0, -1.0, 1.0)
    np.testing.assert_allclose(pca.latent, s ** 2 / (x.shape[0] - 1), rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(pca.coeff.astype(np.float64), v, atol=1e-6)   # (stored float32)
    # the float64 fit itself, before the float32 store
    w, vv = np.linalg.eigh(xc.T @ xc / (x.shape[0] - 1))
    vv = vv[:, np.argsort(-w, kind="stable")]
    big = np.argmax(np.abs(vv), axis=0)
    vv = vv * np.where(vv[big, np.arange(vv.shape[1])] < 0, -1.0, 1.0)
    np.testing.assert_allclose(vv, v, atol=1e-9)
    assert np.all(np.diff(pca.latent) <= 0)
    assert pca.mean.dtype == np.float32 and pca.coeff.shape == (63, 63) and pca.n_frames == 400 and pca.fold == 3
    # sign rule: each column's largest-|.| entry is positive
    cols = np.arange(63)
    assert (pca.coeff[np.argmax(np.abs(pca.coeff), axis=0), cols] > 0).all()


def test_decode_of_project_is_identity_at_full_rank(P):
    pca = P.fit_labels(_separated(seed=1))
    u = _separated(n=32, seed=2)
    p = pca_ref.project(u, pca.mean, pca.coeff, 63)
    back = pca_ref.decode(p, pca.mean, pca.coeff)
    np.testing.assert_allclose(back, u, rtol=0, atol=4 * np.finfo(np.float32).eps)
    # fewer components: the reconstruction error grows, never shrinks
    e = [np.abs(pca_ref.decode(pca_ref.project(u, pca.mean, pca.coeff, k), pca.mean, pca.coeff[:, :k]) - u).max()
         for k in (8, 32)]
    assert e[0] >= e[1] > 0


def test_save_load_roundtrip_and_reference_format(P, tmp_path):
    pca = P.fit_labels(_separated(seed=3), fold=4, aug=True)
    path = pca.save(str(tmp_path))
    assert os.path.basename(path) == "4-aug.npz"
    z = np.load(path)
    assert {"pca_mean", "coeff", "latent"} <= set(z.files)
    np.testing.assert_array_equal(z["coeff"][:, :10], pca.coeff[:, :10])   # what 3D_CNN/dataset.py:173 reads
    back = P.JointPCA.load(path)
    for a in ("mean", "coeff", "latent"):
        np.testing.assert_array_equal(getattr(back, a), getattr(pca, a))
    assert (back.fold, back.aug, back.n_frames) == (4, True, pca.n_frames)
    # the reference's format: MATLAB pca outputs ([1,C] mean, [C,1] latent), or cal_pca's (no latent)
    ref = str(tmp_path / "2.npz")
    np.savez(ref, pca_mean=pca.mean.reshape(1, 63).astype(np.float64), coeff=pca.coeff.astype(np.float64),
             latent=pca.latent.reshape(63, 1))
    r = P.JointPCA.load(ref)
    np.testing.assert_array_equal(r.mean, pca.mean)
    np.testing.assert_array_equal(r.coeff, pca.coeff)
    assert r.aug is False and r.check_k(63) == 63
    np.savez(ref, pca_mean=pca.mean, coeff=pca.coeff[:, :20])
    r = P.JointPCA.load(ref)
    assert r.n_avail == 20 and np.isnan(r.latent).all()
    with pytest.raises(ValueError):
        r.check_k(21)


def test_host_normalisation_equals_restatement(P):
    rng = np.random.default_rng(5)
    ml = rng.uniform(100, 300, 20).astype(np.float32)
    ml[3] = 0
    mp = rng.normal(0, 50, (20, 3)).astype(np.float32)
    gt = (mp[:, None] + rng.normal(0, 80, (20, 21, 3))).astype(np.float32).reshape(20, 63)
    u = P.normalize_labels_np(gt, ml, mp)
    np.testing.assert_array_equal(u, pca_ref.normalize(gt, ml, mp))
    assert (u[3] == 0.5).all() and (u < 0).any() and (u > 1).any()   # no clamp


def test_restatement_reproduces_reference_cal_out(golden_dir):
    g = np.load(os.path.join(golden_dir, "cal_out_ref.npz"))
    err, fmean, fmax, x = pca_ref.pose_error(g["pred"], g["gt"], g["max_l"], g["mid_p"])
    np.testing.assert_array_equal(x, g["output"])
    np.testing.assert_allclose(err, g["err"], rtol=2e-7, atol=0)
    t = float(g["threshold"])
    assert np.float32((err < t).sum()) / np.float32(err.size) * np.float32(100) == pytest.approx(float(g["proportion"]),
                                                                                               abs=1e-4)
    assert float(fmean.astype(np.float64).sum()) == pytest.approx(float(g["err_mean"]), rel=1e-6)
    assert (fmax == err.max(1)).all()


def test_new_entries_validate_arguments_without_a_device(pkg):
    L = pkg._lib.load()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)
    lab = pkg._lib.TsdfLabels(16, 21, 0, 16, None)
    good = pkg._lib.TsdfPca(16, 16, 10, 16)
    for bad in (pkg._lib.TsdfPca(16, 16, 0, 16), pkg._lib.TsdfPca(16, 16, 64, 16), pkg._lib.TsdfPca(None, 16, 10, 16),
                pkg._lib.TsdfPca(16, 16, 10, None)):
        assert L.tsdf_voxelize_labels_pca_hip(one, 16, one, one, 1, 32, None, 0, null, null, one, one, one, null,
                                              ctypes.byref(lab), ctypes.byref(bad)) == -1
        assert L.tsdf_voxelize_indexed_pca_hip(one, 16, one, one, 4, one, 1, 32, None, 0, null, null, one, one, one, null,
                                               ctypes.byref(lab), ctypes.byref(bad)) == -1
        assert L.tsdf_project_joints_hip(one, one, one, 1, 21, ctypes.byref(bad), null) == -1
    idx = (ctypes.c_int64 * 1)(0)
    # pca and labels are required by the fused entries; n > 32 is refused by the inline-index one
    assert L.tsdf_voxelize_labels_pca_hip(one, 16, one, one, 1, 32, None, 0, null, null, one, one, one, null,
                                          None, ctypes.byref(good)) == -1
    assert L.tsdf_voxelize_labels_pca_hip(one, 16, one, one, 1, 32, None, 0, null, null, one, one, one, null,
                                          ctypes.byref(lab), None) == -1
    assert L.tsdf_voxelize_indexed_host_pca_hip(one, 16, one, one, 4, idx, 33, 32, None, 0, null, one, one, one, null,
                                                ctypes.byref(lab), ctypes.byref(good)) == -1
    assert L.tsdf_voxelize_labels_pca_hip(one, 16, one, one, 1, 32, None, 0, null, ctypes.c_void_p(12), one, one, one,
                                          null, ctypes.byref(lab), ctypes.byref(good)) == -1   # misaligned xforms
    # n == 0 is a no-op
    assert L.tsdf_voxelize_labels_pca_hip(null, 0, null, null, 0, 32, None, 0, null, null, null, null, null, null,
                                          ctypes.byref(lab), ctypes.byref(good)) == 0
    assert L.tsdf_project_joints_hip(null, null, null, 0, 21, ctypes.byref(good), null) == 0
    assert L.tsdf_pose_error_hip(null, None, null, null, null, 0, 21, null, null, null, null, null) == 0
    # J outside 1..170, NULL outputs
    assert L.tsdf_pose_error_hip(one, None, one, one, one, 1, 0, null, one, one, one, null) == -1
    assert L.tsdf_pose_error_hip(one, None, one, one, one, 1, 171, null, one, one, one, null) == -1
    assert L.tsdf_project_joints_hip(one, one, one, 1, 171, ctypes.byref(good), null) == -1
    for outs in ((null, one, one), (one, null, one), (one, one, null)):
        assert L.tsdf_pose_error_hip(one, None, one, one, one, 1, 21, null, *outs, null) == -1
    assert L.tsdf_pose_error_hip(one, ctypes.byref(pkg._lib.TsdfPca(16, 16, 64, None)), one, one, one, 1, 21, null,
                                 one, one, one, null) == -1
    assert L.tsdf_pose_error_hip(one, None, one, one, one, -1, 21, null, one, one, one, null) == -1


def test_preprocess_tree_writes_nine_leave_one_out_fits(pkg, synth, tmp_path, P):
    export = importlib.import_module(PKG + ".export")
    db = str(tmp_path / "db")
    synth.synth_msra_tree(db, n_sub=9, n_ges=2, n_frames=6, seed=1)
    rng = np.random.default_rng(0)
    seen = {}

    def stub(pk, res, layout, device):   # placement from the labels themselves: no GPU here
        n = len(pk)
        g = np.asarray(pk.gt if pk.gt is not None else np.zeros((n, 63)), np.float32)
        mid = rng.normal(0, 20, (n, 3)).astype(np.float32)
        ml = rng.uniform(150, 250, n).astype(np.float32)
        st = np.zeros(n, np.int32)
        ml[0], st[0] = 0, 1   # one degenerate frame per gesture: left out of the fit
        return np.zeros((n, 3, 4, 4, 4), np.float32), ml, mid, st

    def spy(pk, res, layout, device):
        out = stub(pk, res, layout, device)
        seen.setdefault("calls", []).append(out[1:])
        return out

    out_dir, pca_dir = str(tmp_path / "result"), str(tmp_path / "PCA")
    export.preprocess_tree(db, out_dir, res=4, point_clouds=False, voxelize_fn=spy, pca_dir=pca_dir)
    assert sorted(os.listdir(pca_dir)) == ["%d.npz" % t for t in range(9)]
    subs = sorted(os.listdir(db))
    # rebuild each subject's normalised labels from what was written, and refit without the held-out subject
    per = {}
    for s in subs:
        us = []
        for ges in sorted(os.listdir(os.path.join(out_dir, s, "TSDF"))):
            z = np.load(os.path.join(out_dir, s, "TSDF", ges))
            gt = np.load(os.path.join(out_dir, s, "ground_truth", ges[:-4] + ".npy"))
            us.append(pca_ref.normalize(gt, z["max_l"], z["mid_p"])[z["status"] == 0])
        per[s] = np.concatenate(us)
    for t in range(9):
        f = P.JointPCA.load(os.path.join(pca_dir, "%d.npz" % t))
        u = np.concatenate([per[s] for s in subs if s != subs[t]])
        assert f.n_frames == len(u) == 8 * 2 * 5
        np.testing.assert_array_equal(f.mean, u.astype(np.float64).mean(0).astype(np.float32))
        assert not np.array_equal(f.mean, P.JointPCA.load(os.path.join(pca_dir, "%d.npz" % ((t + 1) % 9))).mean)


def test_restatement_within_order_free_bound_at_170_joints(P):
    """The sequential restatement at C = 510 against the float64 matmul (pca_ref.project64 / decode64): within the
    rounding bound, and a transposed basis — a bug the restatement and a kernel could share — far outside it."""
    C = 510
    pca = P.fit_labels(_separated(n=600, C=C, seed=7))
    rng = np.random.default_rng(8)
    u = _separated(n=16, C=C, seed=9)
    u[3] = 0.5   # a frame that is not OK
    assert (pca.coeff < 0).any() and (pca.coeff > 0).any()
    for k in (1, 65, C - 1, C):
        p = pca_ref.project(u, pca.mean, pca.coeff, k)
        ref, scale = pca_ref.project64(u, pca.mean, pca.coeff, k)
        assert (np.abs(p - ref) <= pca_ref.bound64(ref, scale, C)).all()
        q = (p + rng.normal(0, 0.05, p.shape)).astype(np.float32)
        uh = pca_ref.decode(q, pca.mean, pca.coeff[:, :k])
        ref, scale = pca_ref.decode64(q, pca.mean, pca.coeff)
        assert (np.abs(uh - ref) <= pca_ref.bound64(ref, scale, k + 1)).all()
    ref, scale = pca_ref.project64(u, pca.mean, pca.coeff.T, C)
    assert (np.abs(pca_ref.project(u, pca.mean, pca.coeff, C) - ref) > pca_ref.bound64(ref, scale, C)).mean() > 0.9
