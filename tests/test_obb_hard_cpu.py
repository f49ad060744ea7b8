"""CPU tier of the principal-axis maps on hard inputs: the spectrum list of tests/obb_ref.py is what each name claims, on
the numpy restatement; and the frame zoo brings the principal-axis kernel the frames tests/test_obb_hard_gpu.py says it
does.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_zoo as fz  # noqa: E402
import obb_ref as ob  # noqa: E402

U = ob.U


def _ref():
    depth, off, hdr = ob.spectrum_pack()
    return {name: f for (name, _, _, _), f in zip(ob.spectrum(), ob.batch(depth, off, hdr))}


def test_spectrum_list_is_what_it_claims():
    ref = _ref()
    assert len(ref) == len(ob.spectrum()) == 10
    tr = {k: f["lam"].sum() for k, f in ref.items()}
    for k in ("plane_const", "square_centred", "three_collinear", "three_triangle", "near_collinear", "near_isotropic",
              "tilted_plane", "huge"):
        assert ref[k]["status"] == 0, k
    # a constant depth in front of the camera: no extent along z
    for k in ("plane_const", "square_centred"):
        assert abs(ref[k]["lam"][2]) <= 64 * U * tr[k] and not ref[k]["C"][2].any()
    assert ob.rel_gaps(ref["plane_const"]["lam"])[0] >= 1e-3
    assert abs(ob.rel_gaps(ref["square_centred"]["lam"])[0]) <= 1e-12            # a tie
    # exactly three valid pixels
    for k in ("three_collinear", "three_triangle"):
        assert ref[k]["N"] == 3 and abs(ref[k]["lam"][2]) <= 64 * U * tr[k]
    assert abs(ref["three_collinear"]["lam"][1]) <= 64 * U * tr["three_collinear"]
    assert ref["three_triangle"]["lam"][1] >= 1e-3 * tr["three_triangle"]
    # nearly collinear: the second eigenvalue is there, ten orders below the first
    lam = ref["near_collinear"]["lam"]
    assert 1e-16 * lam[0] < lam[1] <= 1e-10 * lam[0]
    g = ob.rel_gaps(ref["near_isotropic"]["lam"])
    assert 1e-6 <= g[0] <= 1e-4 and 1e-6 <= g[1] <= 1e-4
    f = ref["tilted_plane"]
    assert abs(f["lam"][2]) <= 1e-9 * f["lam"][0] and min(ob.rel_gaps(f["lam"])) >= 1e-3 and abs(f["A"][2, 2]) < 0.999
    f = ref["huge"]
    assert np.isfinite(f["C"]).all() and np.isfinite(f["lam"]).all() and 1e29 < np.abs(f["pts"][:, 2]).min() < 1e31
    # an infinite depth is a valid pixel, the mean is not finite: degenerate with the count kept
    img = {name: im for name, _, _, im in ob.spectrum()}
    assert np.isposinf(img["one_inf"]).sum() == 1 and not np.isneginf(img["one_inf"]).any()
    assert np.isposinf(img["pm_inf"]).sum() == 1 and np.isneginf(img["pm_inf"]).sum() == 1
    for k in ("one_inf", "pm_inf"):
        f = ref[k]
        assert f["status"] == 1 and f["N"] == img[k].size and not f["mu"].any() and np.array_equal(f["xf"], ob.identity())


def test_rescaled_is_the_frame_of_the_rescaled_depth():
    """What the GPU tier relies on for the 1e30 frame: a power of two scales the restatement exactly."""
    name, left, top, img = next(e for e in ob.spectrum() if e[0] == "huge")
    hdr = np.array([320, 240, left, top, left + img.shape[1], top + img.shape[0]], np.int32)
    big = ob.frame(img.reshape(-1), hdr)
    small = ob.frame((img / np.float32(ob.HUGE)).reshape(-1), hdr)
    r = ob.rescaled(big, 1.0 / ob.HUGE)
    assert np.array_equal(r["mu"], small["mu"]) and np.array_equal(r["C"], small["C"]) and np.array_equal(r["pts"], small["pts"])
    assert np.abs(r["lam"] - small["lam"]).max() <= 64 * U * small["lam"].sum()


def test_the_zoo_brings_the_hard_shapes():
    z = fz.zoo()
    assert len(z) == 230
    shapes = [e.img.shape for e in z]
    assert any(bh == 1 and bw > 1 for bh, bw in shapes) and any(bw == 1 and bh > 1 for bh, bw in shapes)
    assert any(321 <= bw <= 640 for _, bw in shapes) and any(bw == 640 for _, bw in shapes)
    assert any(bh == 480 for bh, _ in shapes) and any(1 <= bh <= 3 for bh, _ in shapes)
