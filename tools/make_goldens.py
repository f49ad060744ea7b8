#!/usr/bin/env python3
"""Generate tests/golden/*.npz by RUNNING the reference's own code.

Runs only in the build container (it imports /root/reference/pre/tsdf_for.py and
pre/process.py, which need nothing but numpy).  The reference never travels to the
GPU box; only the small .npz fixtures written here do.  Re-run with
    python tools/make_goldens.py
and commit the result; tests/test_oracle_golden.py consumes it.

What each fixture pins:
  loop32  pre/tsdf_for.py::tsdf_f -> tsdf_cal exactly as it runs today (numpy 2:
          float32 scalar arithmetic), fed a 2-point cloud {min_p, max_p} so that its
          own glue (tsdf_for.py:11-16) is evaluated on the full-pixel AABB.  Pins the
          grid placement (max_l, mid_p) and the per-voxel formula.
  loop64  the SAME reference function tsdf_cal fed float64-typed copies of the float32
          parameters and depth.  Every operation then runs in float64, which is what
          numba infers for pre/tsdf_numba.py:15-72 (FOCAL is a Python float) — this is
          the numba typing evaluated by the reference's own code.  The parity target.
  pc_*    pre/process.py::DataProcess.point_cloud + max_min_point on ALL valid points
          (no 6000-point resample): the CPU analogue of min_max_kernel.  It computes
          x,y in float32, so it may differ from the numba typing by 1 ulp (App. A.1);
          stored as a witness with that tolerance.
  aug_ref pre/process.py::DataProcess.data_aug run on [1,M,3] clouds with np.random seeded: pins the stretch /
          rotation conventions and the draw order that handposeestimation-with-3d-cnns_amd/augment.py restates.
  joint_nor_ref  pre/joint_nor.py::normalize (:8-18) RUN on [n,21,3] float32 labels (the one shape it does not raise
          on: for the [n,63] arrays its callers hold, `joint_nor[i] = ...` cannot broadcast (21,3) into (63,)) with the
          goldens' own max_l / mid_p plus seeded extra frames: pins the label formula of SURVEY.md 8(f)#4.
  io_ref  pre/read_MSRA.py::read_bin / read_joint (:143-164) RUN on tiny .bin / joint.txt files written here with plain
          numpy / text: the file bytes and exactly what the reference returned (dtype, shape, values).  Pins row a1.
  dataset_ref  3D_CNN/dataset.py::MSRA_Dataset (:16-117) RUN — train=True and train=False — on a 4-subject x 5-gesture
          x 2-frame synthetic MSRA tree (synth.synth_msra_tree, regenerated from its seed by the tests) exported in the
          reference's on-disk schema with the ORACLE as the voxelizer (no GPU here): length, item order, dtypes, shapes,
          gt / max_l / mid_p of every item, the volumes of a few.  Pins row f1 to the class instead of to a reading of it.
  unseen_ref_<k>  run_reference on 33 more seeded frames that no volume fixture holds (unseen_frames): what the
          reference computed for them, for tests/test_reference_live.py.
  cal_out_ref  3D_CNN/train.py::cal_out (:410-427) RUN (train.py imported with a stub tqdm, from a scratch directory
          holding an empty result/) on seeded small-mode predictions decoded as train.py:263-266 does: inputs, per-joint
          errors (the torch.sqrt it takes), the proportion and err_mean.  Pins pose_error / joints_within.
  process_ref_<k>  DataProcess.process()'s placement rule (pre/process.py:13-28): for every volume fixture's frame the
          cloud of tests/point_cloud_ref.py (P = 6000, seed 7; its sha256 is kept, not the cloud) handed to
          pre/tsdf_for.py::tsdf_f(data, cloud) — the grid on the AABB of the RESAMPLED cloud — with the tsdf_cal spy, and
          the loop again on float64-typed parameters; max_min_point's own return values beside them.  A few frames
          with P = 500 and P = 20000 carry the grid values only.  Pins tsdf_cloud_grid_hip / process_batch.
  aabb_*  the numba-typing AABB (pre/tsdf_numba.py:84-96,140-141) from
          oracle/tsdf_oracle_np.py — a restatement, not a run (min_max_kernel cannot
          be executed here: no usable numba, no params.py).
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_PRE = "/root/reference/pre"
sys.path.insert(0, ROOT)

synth = importlib.import_module("handposeestimation-with-3d-cnns_amd.synth")
from oracle import tsdf_oracle_np as onp  # noqa: E402


def _reference():
    """The reference's own pre/tsdf_for.py, pre/process.py and pre/joint_nor.py, imported by the steps that run them and
    by nothing else: the tests import this module for its frame lists and loop32_emulation, without the reference."""
    if REF_PRE not in sys.path:
        sys.path.insert(0, REF_PRE)
    import joint_nor as ref_joint_nor
    import process as ref_process
    import tsdf_for
    return tsdf_for, ref_process, ref_joint_nor


def special_frames():
    """Hand-built edge cases on top of the seeded generator."""
    out = []
    # bbox touching the image border, blob cut by the bbox edge
    h, d = synth.synth_frame(100, "full")
    l, t, r, b = 0, 0, 140, 120
    crop = d.reshape(240, 320)[t:b, l:r].copy()
    out.append(("border_cut", np.array([320, 240, l, t, r, b], np.int32), crop.reshape(-1)))
    # small odd-sized bbox (17 wide): rows are not 16-byte aligned
    h, d = synth.synth_frame(101, "full")
    img = d.reshape(240, 320)
    ys, xs = np.nonzero(img)
    cy, cx = int(ys.mean()), int(xs.mean())
    l, t = cx - 8, cy - 12
    r, b = l + 17, t + 25
    crop = img[t:b, l:r].copy()
    out.append(("small_odd", np.array([320, 240, l, t, r, b], np.int32), crop.reshape(-1)))
    return out


def run_reference(header, depth):
    tsdf_for, ref_process, _ = _reference()
    nv, mn, mx = onp.aabb(depth, header)
    assert nv > 0
    data32 = {"header": header, "depth": depth}

    captured = {}
    orig = tsdf_for.tsdf_cal

    def spy(data, vox_ori, voxel_len, truncation):
        captured["p"] = (np.array(vox_ori), voxel_len, truncation)
        return orig(data, vox_ori, voxel_len, truncation)

    tsdf_for.tsdf_cal = spy
    try:
        pc2 = np.stack([mn, mx]).astype(np.float32)
        loop32, max_l, mid_p = tsdf_for.tsdf_f(data32, pc2)  # reference glue + loop, as it runs today
    finally:
        tsdf_for.tsdf_cal = orig
    vox_ori, voxel_len, truncation = captured["p"]
    assert vox_ori.dtype == np.float32 and np.asarray(voxel_len).dtype == np.float32

    # numba typing through the reference's own loop: float64-typed copies of float32 values
    data64 = {"header": header, "depth": depth.astype(np.float64)}
    loop64 = orig(data64, vox_ori.astype(np.float64), np.float64(voxel_len), np.float64(truncation))

    # CPU analogue of the AABB on all valid points (process.py:30-68,102-120)
    dp = ref_process.DataProcess({"header": header, "depth": depth}, np.zeros(63, np.float32))
    pts = dp.point_cloud()
    pmax, pmin = dp.max_min_point(pts)

    # loop layout [c,x,y,z] -> numba layout [c,z,y,x]
    l32 = np.ascontiguousarray(loop32.transpose(0, 3, 2, 1)).astype(np.float32)
    l64 = np.ascontiguousarray(loop64.transpose(0, 3, 2, 1)).astype(np.float32)
    assert np.array_equal(l32.astype(np.float64), loop32.transpose(0, 3, 2, 1)), "loop32 holds f32 values"
    return dict(
        header=header, depth=depth,
        aabb_min=mn, aabb_max=mx, n_valid=np.int64(nv),
        pc_min=pmin, pc_max=pmax, pc_n=np.int64(pts.shape[0]),
        max_l=np.float32(max_l), mid_p=np.asarray(mid_p, np.float32),
        vox_ori=vox_ori, voxel_len=np.float32(voxel_len), trunc=np.float32(truncation),
        loop32=l32, loop64=l64,
        n_flip=np.int64((np.abs(l32 - l64) > 1e-5).any(axis=0).sum()),
    )


def run_reference_aug(outdir):
    """aug_ref.npz: the reference's own DataProcess.data_aug (pre/process.py:202-261) run on [1,M,3] clouds —
    the one input shape it does not raise AxisError on — with np.random seeded.  Stores the
    inputs, the seeds and what the reference returned; nothing else (the draws are not observable from outside:
    tests re-draw them with augment.reference_draw and must reproduce these outputs)."""
    _, ref_process, _ = _reference()
    rng = np.random.default_rng(4242)
    seeds = np.array([0, 1, 7, 12345, 20261004], np.int64)
    M = 64
    pcs = rng.normal(0, 60, (len(seeds), 1, M, 3))
    pcs[..., 2] -= 400.0  # in front of the camera, z = -depth
    gts = rng.normal(0, 70, (len(seeds), 63))
    gts[:, 2::3] -= 400.0
    pc_aug = np.empty_like(pcs)
    gt_aug = np.empty((len(seeds), 63))
    for i, sd in enumerate(seeds):
        dp = ref_process.DataProcess({"header": np.array([320, 240, 0, 0, 4, 4], np.int32),
                                      "depth": np.zeros(16, np.float32)}, gts[i].copy(), aug=True)
        np.random.seed(int(sd))
        pa, ga = dp.data_aug(pcs[i].copy())
        pc_aug[i] = pa
        gt_aug[i] = ga.reshape(63)
    np.savez_compressed(os.path.join(outdir, "aug_ref.npz"), seeds=seeds, pc=pcs, gt=gts, pc_aug=pc_aug, gt_aug=gt_aug)
    print(f"aug_ref: {len(seeds)} seeded data_aug runs on [1,{M},3] clouds")


def run_reference_joint_nor(outdir, golden_scales):
    """joint_nor_ref.npz: the reference's own normalize (pre/joint_nor.py:8-18) run on float32 [n,21,3] labels.
    The first frames use the max_l / mid_p the reference's tsdf_f produced for the volume goldens (same order as
    MANIFEST.txt), the rest seeded scales; some joints lie outside the cube so that the clamp of
    3D_CNN/train.py:241-242 (applied by the test to these reference values) has something to do.  The reference
    stores its float32 results in a float64 array; they are kept as float64 here, untouched."""
    _, _, ref_joint_nor = _reference()
    rng = np.random.default_rng(777)
    n_extra = 24
    max_l = np.concatenate([np.array([g[0] for g in golden_scales], np.float32),
                            rng.uniform(80, 400, n_extra).astype(np.float32)])
    mid_p = np.concatenate([np.stack([g[1] for g in golden_scales]).astype(np.float32),
                            (rng.normal(0, 80, (n_extra, 3)) + [0, 0, -420]).astype(np.float32)])
    n = len(max_l)
    gt = (mid_p[:, None, :] + rng.normal(0, 0.35, (n, 21, 3)) * max_l[:, None, None]).astype(np.float32)
    want = ref_joint_nor.normalize(gt.copy(), max_l, mid_p)
    assert want.shape == (n, 21, 3) and want.dtype == np.float64
    assert (want < 0).any() and (want > 1).any()
    np.savez_compressed(os.path.join(outdir, "joint_nor_ref.npz"), gt=gt, max_l=max_l, mid_p=mid_p, joint_nor=want)
    # the [n,63] form its callers hold (pre/joint_nor.py:42-45 feeds np.load of ground_truth/*.npy) does not run:
    try:
        ref_joint_nor.normalize(gt.reshape(n, 63).copy(), max_l, mid_p)
        raise AssertionError("normalize accepted [n,63]")
    except ValueError:
        pass
    print(f"joint_nor_ref: {n} frames x 21 joints through pre/joint_nor.py::normalize "
          f"({int((want < 0).sum())} coordinates < 0, {int((want > 1).sum())} > 1)")


def run_reference_io(outdir):
    """io_ref.npz: the reference's own read_bin / read_joint (pre/read_MSRA.py:143-164) on files written here.
    Stored: every file's bytes (uint8) and what the reference returned for it.  read_joint returns a 1-D array for a
    one-frame gesture (np.loadtxt squeezes); the fixture keeps that shape — packing.read_joint documents its [1,63]."""
    import tempfile

    sys.path.insert(0, REF_PRE)
    import read_MSRA as ref_io  # noqa: E402  (the reference; pulls scipy.io, process, joint_pca — all importable)

    rng = np.random.default_rng(31337)
    bins = {}
    # odd width (rows not 16-byte aligned), zeros and sub-threshold values inside
    d = rng.uniform(250, 600, 17 * 5).astype(np.float32)
    d[rng.random(d.size) < 0.3] = 0.0
    d[3] = 0.5
    bins["odd_17x5"] = (np.array([320, 240, 100, 60, 117, 65], np.int32), d)
    # one pixel
    bins["one_pixel"] = (np.array([320, 240, 7, 9, 8, 10], np.int32), np.array([431.25], np.float32))
    # a whole 320x240 frame (the synthetic generator's)
    bins["full_frame"] = synth.synth_frame(3, "full")
    # payload bytes a text-mode read could mangle (the reference opens the file with 'r', :157): CR, LF, CR LF, ^Z, 0xFF
    raw = np.frombuffer(bytes([0x0d, 0x0a, 0x0d, 0x0a, 0x1a, 0x00, 0x0a, 0x43, 0xff, 0xfe, 0x0d, 0x44, 0x0a, 0x0a, 0x0a,
                               0x44] * 3), dtype=np.float32).copy()
    bins["text_mode_bytes"] = (np.array([320, 240, 0, 0, 4, 3], np.int32), raw)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (h, dep) in bins.items():
            fn = os.path.join(tmp, name + ".bin")
            with open(fn, "wb") as f:
                f.write(np.asarray(h, np.int32).tobytes())
                f.write(np.asarray(dep, np.float32).tobytes())
            rh, rd = ref_io.read_bin(fn)
            assert rh.dtype == np.int32 and rd.dtype == np.float32
            out["bin_%s_bytes" % name] = np.fromfile(fn, dtype=np.uint8)
            out["bin_%s_header" % name] = rh
            out["bin_%s_depth" % name] = rd
        for n in (1, 3):
            gdir = os.path.join(tmp, "ges%d" % n)
            os.makedirs(gdir)
            rows = rng.normal(0, 80, (n, 63))
            rows[:, 2::3] -= 400.0
            with open(os.path.join(gdir, "joint.txt"), "w") as f:
                f.write("%d\n" % n)
                for r in rows:   # MSRA's own files separate with single spaces; mixed precision on purpose
                    f.write(" ".join(("%.6f" if k % 2 else "%.3f") % v for k, v in enumerate(r)) + "\n")
            cnt, gt = ref_io.read_joint(gdir)
            assert gt.dtype == np.float32
            out["joint%d_bytes" % n] = np.fromfile(os.path.join(gdir, "joint.txt"), dtype=np.uint8)
            out["joint%d_count" % n] = np.int64(cnt)
            out["joint%d_gt" % n] = gt
    out["bin_names"] = np.array(sorted(bins))
    np.savez_compressed(os.path.join(outdir, "io_ref.npz"), **out)
    print("io_ref: %d .bin files + 2 joint.txt through pre/read_MSRA.py::read_bin / read_joint "
          "(joint.txt with one frame -> shape %s)" % (len(bins), out["joint1_gt"].shape,))


DATASET_TREE = dict(n_sub=4, n_ges=5, n_frames=2, seed=0, kind="crop")


def run_reference_dataset(outdir):
    """dataset_ref.npz: the reference's own MSRA_Dataset (3D_CNN/dataset.py:16-117) over an export of a synthetic tree.
    The export is this project's export.preprocess_tree with the ORACLE as the voxelizer and gt_3d=True (the one label
    form the reference reader does not crash on, App. B#11); the class is run in a child interpreter (it sets
    CUDA_VISIBLE_DEVICES at import, :12-13)."""
    import hashlib
    import subprocess
    import tempfile

    import oracle
    pkg = importlib.import_module("handposeestimation-with-3d-cnns_amd")

    def vox(pk, res, layout, device):
        r = oracle.voxelize(pk.depth, pk.offsets, pk.headers, R=res, layout=0 if layout == "czyx" else 1)
        return r["tsdf"], r["max_l"], r["mid_p"], r["status"]

    with tempfile.TemporaryDirectory() as tmp:
        db, res = os.path.join(tmp, "db"), os.path.join(tmp, "result")
        total = synth.synth_msra_tree(db, **DATASET_TREE)
        pkg.export.preprocess_tree(db, res, gt_3d=True, point_clouds=False, voxelize_fn=vox)
        child = r"""
import sys, numpy as np
sys.path.insert(0, "/root/reference/3D_CNN")
import dataset as ref_ds
out = {}
for name, train in (("train", True), ("test", False)):
    ds = ref_ds.MSRA_Dataset(sys.argv[1], None, train=train)
    n = len(ds)
    items = [ds[i] for i in range(n)]
    assert all(len(it) == 4 for it in items)
    out[name + "_len"] = np.int64(n)
    out[name + "_tsdf"] = np.stack([it[0] for it in items])
    out[name + "_gt"] = np.stack([it[1] for it in items])
    out[name + "_max_l"] = np.stack([it[2] for it in items])
    out[name + "_mid_p"] = np.stack([it[3] for it in items])
    out[name + "_item_types"] = np.array([type(x).__name__ + ":" + str(np.asarray(x).dtype) + ":" + str(np.asarray(x).shape) for x in items[0]])
np.savez(sys.argv[2], **out)
"""
        raw = os.path.join(tmp, "ref_items.npz")
        subprocess.run([sys.executable, "-c", child, res, raw], check=True, cwd=tmp, stdout=subprocess.DEVNULL)
        z = np.load(raw)
        out = {"tree": np.array(["%s=%s" % kv for kv in sorted(DATASET_TREE.items())]), "total_frames": np.int64(total)}
        keep = {"train": [0, 1, 9, 10, 19, 29], "test": [0, 9]}   # volumes kept whole; every item keeps a digest
        for name in ("train", "test"):
            n = int(z[name + "_len"])
            tsdf = z[name + "_tsdf"]
            assert tsdf.dtype == np.float32 and tsdf.shape == (n, 3, 32, 32, 32)
            for k in ("gt", "max_l", "mid_p", "item_types", "len"):
                out["%s_%s" % (name, k)] = z["%s_%s" % (name, k)]
            out[name + "_tsdf_sha256"] = np.array([hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for v in tsdf])
            idx = np.array([i for i in keep[name] if i < n], np.int64)
            out[name + "_kept"] = idx
            out[name + "_tsdf_kept"] = tsdf[idx]
        np.savez_compressed(os.path.join(outdir, "dataset_ref.npz"), **out)
        print("dataset_ref: 3D_CNN/dataset.py::MSRA_Dataset over a %d-frame export: len(train)=%d len(test)=%d, item %s"
              % (total, int(z["train_len"]), int(z["test_len"]), list(z["train_item_types"])))


# Frames outside the two benchmark distributions (synth.synth_variant): name -> (seed, parameters).  The *_flip seeds
# were FOUND by scanning seeds 0..39 of each family with a vectorised float32 emulation of the loop (bit-identical to
# the reference's loop32 on every fixture: checked below) for frames on which the loop as it runs today (float32
# scalars) and the numba typing (float64) disagree by more than 1e-5 somewhere — a pixel index `int(v_x*q + 160)`
# (pre/tsdf_numba.py:31-32), the `> 1` truncation test or the sign test falling the other way (hard part
# #1).  About one frame in fifty has such voxels.  They are carried with the float64 expectation (loop64) AND the
# float32 one (loop32); n_flip counts the voxels that differ.
VARIANTS = [
    ("near_150", 0, dict(bbox=(40, 20, 300, 230), base=150.0, rad=100.0, bulge=30.0)),          # a hand at the lens
    ("far_1500", 0, dict(bbox=(130, 90, 190, 150), base=1500.0, rad=18.0, bulge=25.0)),         # across the room
    ("far_1500_flip", 4, dict(bbox=(130, 90, 190, 150), base=1500.0, rad=18.0, bulge=25.0)),
    ("corner_tl", 0, dict(bbox=(0, 0, 110, 100), base=380.0, rad=45.0)),                        # far off the principal point
    ("corner_tl_flip", 11, dict(bbox=(0, 0, 110, 100), base=380.0, rad=45.0)),
    ("corner_br_flip", 1, dict(bbox=(200, 130, 320, 240), base=520.0, rad=50.0)),
    ("sparse_1pct", 0, dict(bbox=(60, 40, 260, 200), base=420.0, rad=75.0, keep=0.012)),        # ~1 % of the blob valid
    ("sparse_1pct_flip", 27, dict(bbox=(60, 40, 260, 200), base=420.0, rad=75.0, keep=0.012)),
    ("dense", 0, dict(bbox=(100, 70, 220, 170), base=400.0, rad=200.0, keep=1.0)),              # every bbox pixel valid
    ("neg_all_flip", 2, dict(bbox=(80, 60, 240, 200), base=450.0, rad=60.0, sign="neg")),       # z = +d: behind the camera
    # mixed-sign depths: the grid straddles z = 0, q = -F / v_z changes sign inside it (pre/tsdf_numba.py:30-41)
    ("mixed_halves", 0, dict(bbox=(90, 50, 230, 190), base=300.0, rad=60.0, sign="halves")),
    ("mixed_checker", 0, dict(bbox=(90, 50, 230, 190), base=250.0, rad=55.0, sign="checker")),
    ("mixed_halves_near", 3, dict(bbox=(120, 80, 200, 160), base=40.0, rad=35.0, bulge=10.0, sign="halves")),
]
FLIP_CROP_SEED = 20     # synth_frame(20, "crop"): the one flip frame among seeds 0..59 of the benchmark distributions


def loop32_emulation(depth, header, vox_ori, voxel_len, trunc):
    """The reference loop as it runs under numpy 2 (float32 scalar arithmetic), vectorised — ONLY a search tool for
    flip frames and a cross-check of itself against the reference's loop32 below; nothing is pinned to it."""
    F = np.float32(241.42)
    l, t, r, b = [int(v) for v in header[2:6]]
    step = (np.arange(32) * np.float32(voxel_len)).astype(np.float32)
    X, Y, Z = np.meshgrid(vox_ori[0] + step, vox_ori[1] + step, vox_ori[2] + step, indexing="ij")
    with np.errstate(all="ignore"):
        coeff = -F / Z
        px = np.trunc(X * coeff + np.float32(160)).astype(np.int64)
        py = np.trunc(-Y * coeff + np.float32(120)).astype(np.int64)
    ok = (px >= l) & (px < r) & (py >= t) & (py < b)
    pd = depth[np.where(ok, (py - t) * (r - l) + px - l, 0)]
    ok &= np.abs(pd) >= 1
    c1 = pd / F
    wx, wy, wz = (px - 160).astype(np.float32) * c1, (-(py - 120)).astype(np.float32) * c1, -pd
    tx, ty, tz = np.abs(X - wx) / trunc, np.abs(Y - wy) / trunc, np.abs(Z - wz) / trunc
    far = np.sqrt(tx * tx + ty * ty + tz * tz) > 1
    sgn = np.where(wz > Z, -1, 1)
    out = np.stack([np.where(far, 1, np.minimum(v, 1)) * sgn for v in (tx, ty, tz)]).astype(np.float32) * ok
    return np.ascontiguousarray(out.transpose(0, 3, 2, 1))


def volume_frames():
    frames = []
    for s in (0, 1, 2):
        h, d = synth.synth_frame(s, "full")
        frames.append((f"full_{s}", h, d))
    for s in (10, 11, 12):
        h, d = synth.synth_frame(s, "crop")
        frames.append((f"crop_{s}", h, d))
    frames += special_frames()
    h, d = synth.synth_frame(FLIP_CROP_SEED, "crop")
    frames.append((f"crop_{FLIP_CROP_SEED}_flip", h, d))
    for name, seed, kw in VARIANTS:
        h, d = synth.synth_variant(seed, **kw)
        frames.append((name, h, d))
    return frames


def run_volumes(outdir):
    names = []
    scales = []
    for name, h, d in volume_frames():
        g = run_reference(h, d)
        emu = loop32_emulation(d, h, g["vox_ori"], g["voxel_len"], g["trunc"])
        assert np.array_equal(emu, g["loop32"]), f"{name}: the search emulation is not the reference's loop32"
        assert (int(g["n_flip"]) > 0) == name.endswith("_flip"), (name, int(g["n_flip"]))
        scales.append((g["max_l"], g["mid_p"]))
        np.savez_compressed(os.path.join(outdir, f"{name}.npz"), **g)
        names.append(name)
        dd = np.abs(g["loop32"] - g["loop64"])
        print(f"{name}: bbox {h[4]-h[2]}x{h[5]-h[3]} valid {int(g['n_valid'])} of {d.size} max_l {float(g['max_l']):.4f} "
              f"mid_z {float(g['mid_p'][2]):.1f} nonzero voxels {int((g['loop64'] != 0).any(axis=0).sum())} "
              f"flips(f32 vs f64 loop) {int(g['n_flip'])} |loop32-loop64|max(non-flip) {float(dd[dd <= 1e-5].max()):.2e}")
    run_reference_joint_nor(outdir, scales)
    with open(os.path.join(outdir, "MANIFEST.txt"), "w") as f:
        f.write("# written by tools/make_goldens.py from /root/reference/pre/{tsdf_for,process,joint_nor}.py\n")
        f.write("# numpy %s\n" % np.__version__)
        f.write("# *_flip: frames on which the float32 loop and the float64 (numba-typed) loop disagree somewhere (n_flip > 0)\n")
        for n in names:
            f.write(n + "\n")


def unseen_frames():
    """33 seeded frames that are NOT among the volume fixtures, of every family — benchmark distributions, near / far
    hands, corner bboxes, sparse, dense, negative and mixed-sign depths: (name, header, depth)."""
    out = []
    for s in (40, 41):
        out.append((f"full_{s}", *synth.synth_frame(s, "full")))
    for s in (60, 61, 62, 63):
        out.append((f"crop_{s}", *synth.synth_frame(s, "crop")))
    for name, _, kw in VARIANTS:                        # two unseen seeds of every family the fixtures hold
        for s in (200, 201):
            out.append((f"{name}#{s}", *synth.synth_variant(s, **kw)))
    # mixed signs at two different distances: the camera plane off the grid's centre
    h, d = synth.synth_variant(202, bbox=(60, 30, 260, 210), base=500.0, rad=80.0)
    xs = np.arange(d.size) % 200
    out.append(("mixed_two_distances", h, np.where(xs < 100, -0.3 * d, d).astype(np.float32)))
    return out


UNSEEN_PER_FILE = 6     # unseen_ref_<k>.npz: frames [6k, 6k+6) of unseen_frames(), each file well under 1 MiB


def depth_digest(depth):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(depth, np.float32).tobytes()).hexdigest()


def run_unseen(outdir):
    """unseen_ref_<k>.npz: run_reference on unseen_frames(), for tests/test_reference_live.py.  The depths are not stored
    (the seeded generator makes them again; their sha256 is kept so that a drift of the generator is caught); loop64 is
    stored whole, loop32 as the voxels where its bits differ from loop64 (flat index + value)."""
    frames = unseen_frames()
    for k in range(0, len(frames), UNSEEN_PER_FILE):
        out = {"names": np.array([f[0] for f in frames[k:k + UNSEEN_PER_FILE]])}
        for i, (name, h, d) in enumerate(frames[k:k + UNSEEN_PER_FILE]):
            with np.errstate(all="ignore"):
                g = run_reference(h, d)
            emu = loop32_emulation(d, h, g["vox_ori"], g["voxel_len"], g["trunc"])
            assert np.array_equal(emu, g["loop32"]), f"{name}: the search emulation is not the reference's loop32"
            diff = np.flatnonzero(g["loop32"].view(np.uint32) != g["loop64"].view(np.uint32))
            rec = {key: g[key] for key in ("header", "aabb_min", "aabb_max", "n_valid", "pc_min", "pc_max", "pc_n", "max_l",
                                           "mid_p", "vox_ori", "voxel_len", "trunc", "loop64", "n_flip")}
            rec.update(depth_sha256=np.array(depth_digest(d)), loop32_diff_index=diff.astype(np.int64),
                       loop32_diff_value=g["loop32"].reshape(-1)[diff])
            out.update({f"f{i}_{key}": v for key, v in rec.items()})
        fn = os.path.join(outdir, f"unseen_ref_{k // UNSEEN_PER_FILE}.npz")
        np.savez_compressed(fn, **out)
        print(f"{os.path.basename(fn)}: {len(out['names'])} frames, {os.path.getsize(fn)} bytes")


PROCESS_PER_FILE = 8    # process_ref_<k>.npz: frames [8k, 8k+8) of volume_frames(), each file under 1 MiB
PROCESS_P, PROCESS_SEED = 6000, 7
PROCESS_GRID_ONLY = [("full_0", 500), ("crop_10", 500), ("sparse_1pct", 500), ("full_1", 20000), ("small_odd", 20000),
                     ("mixed_halves", 20000)]     # (frame, P): grid values only, no volumes


def process_cloud(header, depth, P, seed=PROCESS_SEED):
    """The frame's resampled cloud float64[P,3] as tsdf_point_clouds_hip is specified (tests/point_cloud_ref.py)."""
    tests = os.path.join(ROOT, "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    import point_cloud_ref
    off = np.array([0, depth.size], np.int64)
    pts, _, st = point_cloud_ref.point_clouds(depth, off, np.asarray(header, np.int32).reshape(1, 6), P, seed=seed)
    assert st[0] == 0
    return pts[0]


def cloud_digest(cloud):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(cloud, np.float64).tobytes()).hexdigest()


def run_reference_process(header, depth, cloud, volumes=True):
    """tsdf_f(data, cloud) of the reference, RUN: what it returned and what it passed to tsdf_cal; with ``volumes`` the
    loop as it runs today (loop32) and on float64-typed parameters (loop64), both as float32 in [c,z,y,x]."""
    tsdf_for, _, _ = _reference()
    captured = {}
    orig = tsdf_for.tsdf_cal

    def spy(data, vox_ori, voxel_len, truncation):
        captured["p"] = (np.array(vox_ori), voxel_len, truncation)
        return orig(data, vox_ori, voxel_len, truncation) if volumes else None

    tsdf_for.tsdf_cal = spy
    try:
        loop32, max_l, mid_p = tsdf_for.tsdf_f({"header": header, "depth": depth}, cloud)
    finally:
        tsdf_for.tsdf_cal = orig
    vox_ori, voxel_len, truncation = captured["p"]
    assert vox_ori.dtype == np.float32 and np.asarray(voxel_len).dtype == np.float32
    assert np.asarray(max_l).dtype == np.float32 and np.asarray(mid_p).dtype == np.float32
    pmax, pmin = tsdf_for.max_min_point(cloud)
    g = dict(header=np.asarray(header, np.int32), point_max=pmax, point_min=pmin, max_l=np.float32(max_l),
             mid_p=np.asarray(mid_p, np.float32), vox_ori=vox_ori, voxel_len=np.float32(voxel_len),
             trunc=np.float32(truncation))
    if volumes:
        data64 = {"header": header, "depth": depth.astype(np.float64)}
        loop64 = orig(data64, vox_ori.astype(np.float64), np.float64(voxel_len), np.float64(truncation))
        l32 = np.ascontiguousarray(loop32.transpose(0, 3, 2, 1)).astype(np.float32)
        l64 = np.ascontiguousarray(loop64.transpose(0, 3, 2, 1)).astype(np.float32)
        assert np.array_equal(l32.astype(np.float64), loop32.transpose(0, 3, 2, 1)), "loop32 holds f32 values"
        diff = np.flatnonzero(l32.view(np.uint32) != l64.view(np.uint32))
        g.update(loop64=l64, loop32_diff_index=diff.astype(np.int64), loop32_diff_value=l32.reshape(-1)[diff],
                 n_flip=np.int64((np.abs(l32 - l64) > 1e-5).any(axis=0).sum()))
    return g


def run_process(outdir):
    """process_ref_<k>.npz.  Touches no other fixture and not MANIFEST.txt."""
    frames = volume_frames()
    by_name = {name: (h, d) for name, h, d in frames}
    recs = []
    for name, h, d in frames:
        cloud = process_cloud(h, d, PROCESS_P)
        with np.errstate(all="ignore"):
            g = run_reference_process(h, d, cloud)
        g.update(P=np.int64(PROCESS_P), seed=np.int64(PROCESS_SEED), depth_sha256=np.array(depth_digest(d)),
                 cloud_sha256=np.array(cloud_digest(cloud)))
        recs.append((name, g))
        print(f"{name}: valid {int((d != 0).sum())} max_l {float(g['max_l']):.4f} loop32 != loop64 on "
              f"{g['loop32_diff_index'].size} voxels ({int(g['n_flip'])} by more than 1e-5)")
    k = 0
    for k in range(0, len(recs), PROCESS_PER_FILE):
        part = recs[k:k + PROCESS_PER_FILE]
        out = {"names": np.array([name for name, _ in part])}
        for i, (_, g) in enumerate(part):
            out.update({f"f{i}_{key}": v for key, v in g.items()})
        fn = os.path.join(outdir, f"process_ref_{k // PROCESS_PER_FILE}.npz")
        np.savez_compressed(fn, **out)
        print(f"{os.path.basename(fn)}: {len(part)} frames, {os.path.getsize(fn)} bytes")
    out = {"names": np.array([f"{name}@P{P}" for name, P in PROCESS_GRID_ONLY])}
    for i, (name, P) in enumerate(PROCESS_GRID_ONLY):
        h, d = by_name[name]
        cloud = process_cloud(h, d, P)
        g = run_reference_process(h, d, cloud, volumes=False)
        g.update(P=np.int64(P), seed=np.int64(PROCESS_SEED), depth_sha256=np.array(depth_digest(d)),
                 cloud_sha256=np.array(cloud_digest(cloud)))
        out.update({f"f{i}_{key}": v for key, v in g.items()})
    fn = os.path.join(outdir, f"process_ref_{k // PROCESS_PER_FILE + 1}.npz")
    np.savez_compressed(fn, **out)
    print(f"{os.path.basename(fn)}: {len(PROCESS_GRID_ONLY)} frames (grid values only), {os.path.getsize(fn)} bytes")


def run_reference_cal_out(outdir):
    """cal_out_ref.npz: the reference's own evaluation (3D_CNN/train.py::cal_out) on seeded normalised predictions of
    16 frames, decoded to mm with the reference's small-mode expression (train.py:263-266) in float32 torch."""
    import tempfile
    import types

    import torch
    ref_cnn = os.path.join(os.path.dirname(REF_PRE), "3D_CNN")
    if ref_cnn not in sys.path:
        sys.path.insert(0, ref_cnn)
    sys.modules.setdefault("tqdm", types.SimpleNamespace(tqdm=lambda x, *a, **k: x))
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "result"))
        os.chdir(tmp)
        try:
            import train as ref_train   # (train.py:28 lists ./result/ at import)
        finally:
            os.chdir(cwd)
    threshold = 20
    ref_train.opt = types.SimpleNamespace(threshold=threshold)
    rng = np.random.default_rng(4242)
    b = 16
    max_l = rng.uniform(120, 260, b).astype(np.float32)
    mid_p = (rng.normal(0, 60, (b, 3)) + [0, 0, -400]).astype(np.float32)
    gt = (mid_p[:, None, :] + rng.normal(0, 0.3, (b, 21, 3)) * max_l[:, None, None]).astype(np.float32).reshape(b, 63)
    gt_nor = ((gt.reshape(b, 21, 3) - mid_p[:, None, :]) / max_l[:, None, None] + np.float32(0.5)).reshape(b, 63)
    pred = (gt_nor + rng.normal(0, 0.09, (b, 63))).astype(np.float32)   # errors of a few mm to ~60 mm
    est = torch.from_numpy(pred)
    ml, mp = torch.from_numpy(max_l).unsqueeze(1), torch.from_numpy(mid_p).unsqueeze(1)
    output = ((est - 0.5) * ml).view(b, -1, 3) + mp   # train.py:263-266
    seen = []

    class _SpyTorch:   # the per-joint errors: what cal_out's torch.sqrt returns
        def __getattr__(self, k):
            return getattr(torch, k)

        def sqrt(self, x):
            r = torch.sqrt(x)
            seen.append(r.clone())
            return r

    ref_train.torch = _SpyTorch()
    try:
        good, err_mean = ref_train.cal_out(output, torch.from_numpy(gt), b)
    finally:
        ref_train.torch = torch
    err = seen[0].numpy()
    assert err.shape == (b, 21) and 0 < (err < threshold).mean() < 1
    np.savez_compressed(os.path.join(outdir, "cal_out_ref.npz"), pred=pred, max_l=max_l, mid_p=mid_p, gt=gt,
                        output=output.numpy().reshape(b, 63), err=err, threshold=np.float32(threshold),
                        proportion=np.float32(good.item()), err_mean=np.float32(err_mean.item()))
    print(f"cal_out_ref: {b} frames, proportion {good.item():.3f} %, err_mean {err_mean.item():.3f}")


def main(only=None):
    outdir = os.path.join(ROOT, "tests", "golden")
    os.makedirs(outdir, exist_ok=True)
    steps = {"aug": run_reference_aug, "io": run_reference_io, "dataset": run_reference_dataset, "volumes": run_volumes,
             "unseen": run_unseen, "cal_out": run_reference_cal_out, "process": run_process}
    for name in (only or list(steps)):   # --only: some of the fixtures, the others untouched (npz files carry time stamps)
        steps[name](outdir)


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description="Regenerate tests/golden/*.npz by running the reference's own code "
                                             "(needs /root/reference).")
    ap.add_argument("--only", default="", help="comma list of aug,io,dataset,volumes,unseen,cal_out,process: just these fixtures")
    main([x for x in ap.parse_args().only.split(",") if x])
