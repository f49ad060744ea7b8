"""CPU tier of the search windows of the two accurate kernels (tests/window_ref.py), on every one-position input their GPU
tiers compare: the existing lists ``accurate_ref.all_cases()`` / ``mapaccurate_ref.all_cases()`` and the sparse frames of
tests/sparse_ref.py, in both layouts.

 1. The restated rectangle contains the reference-nearest pixel of every non-fragile near voxel.  That checks the
    derivation in the kernels' heads, and the restatement against the brute-force references.
 2. The inputs are ADEQUATE — a condition on the inputs, not a measurement: each listed mistake of a window loses at least
    ``ADEQUATE`` = 8 voxels over all GPU inputs of its kernel (both layouts summed), "no_union" at least one in each
    layout, and the mapped kernel's "T90" and "no_Hz" reach 8 on the sparse frames alone.  A kernel that made one of these
    mistakes would therefore return a wrong ``nearest`` on its GPU tier.  An input that does not help is replaced; the 8
    stays.
 3. Every new case keeps its fragile share within ``accurate_ref.FRAGILE_CAP`` by the reference alone, and the three
    frames the GPU tiers ask for by name are what they are asked to be."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accurate_ref as ar  # noqa: E402
import mapaccurate_ref as mr  # noqa: E402
import sparse_ref as sp  # noqa: E402
import window_ref as wr  # noqa: E402

ADEQUATE = 8
LAYOUTS = (0, 1)

# label -> a function returning (case dict, R, camera); the dicts are the memoised ones of the reference modules
PLAIN_INPUTS = {label: (lambda k=(kind, name, R, sh): (ar.case(*k), k[2], None)) for label, kind, name, R, sh in ar.all_cases()}
PLAIN_INPUTS.update({"sparse " + n: (lambda n=n: (sp.plain_case(n), sp.PLAIN[n][2], sp.PLAIN[n][1])) for n in sp.PLAIN})
MAPPED_INPUTS = {label: (lambda k=key: (mr.case(*k), k[3], k[5])) for label, key in mr.all_cases()}
MAPPED_INPUTS.update({"sparse " + n: (lambda n=n: (sp.mapped_case(n), sp.MAPPED[n][3], sp.MAPPED[n][2])) for n in sp.MAPPED})

_counts = {}


def counts(kind, label):
    """{(mistake, layout): voxels lost} of one input, computed once."""
    if (kind, label) not in _counts:
        c, R, cam = (PLAIN_INPUTS if kind == "plain" else MAPPED_INPUTS)[label]()
        hdr, row = c["hdr"][0], c["grid"][0]
        out = {}
        for m in (None,) + (wr.PLAIN_MISTAKES if kind == "plain" else wr.MAPPED_MISTAKES):
            for lay in LAYOUTS:
                w = wr.plain_window(row, hdr, R, lay, cam, m) if kind == "plain" else \
                    wr.mapped_window(row, hdr, R, lay, c["xf"][0], cam, m)
                out[m, lay] = wr.lost(c["ref"], hdr, w)[0]
        _counts[kind, label] = out
    return _counts[kind, label]


def ids(d):
    return [k.replace(" ", "_") for k in d]


# ---- 1. the kernels' formula loses nothing ----
@pytest.mark.parametrize("label", list(PLAIN_INPUTS), ids=ids(PLAIN_INPUTS))
def test_plain_window_holds_every_nearest_pixel(label):
    c, R, cam = PLAIN_INPUTS[label]()
    got = counts("plain", label)
    assert int((c["ref"]["near"] & ~c["ref"]["fragile"]).sum()) > 0
    assert got[None, 0] == 0 and got[None, 1] == 0, (label, got)


@pytest.mark.parametrize("label", list(MAPPED_INPUTS), ids=ids(MAPPED_INPUTS))
def test_mapped_window_holds_every_nearest_pixel(label):
    got = counts("mapped", label)
    assert got[None, 0] == 0 and got[None, 1] == 0, (label, got)


def test_untrusted_inverses_have_no_rectangle():
    # diag(1, 1, 0) has no inverse and a NaN entry makes every norm a NaN: the whole crop, for every item
    for m in ("singular", "nanfwd"):
        c = mr.case("synth", 0, m, 12)
        assert not (wr.window_consts(c["xf"][0])[3] == wr.window_consts(c["xf"][0])[3])
        c0, c1, r0, r1, finite = wr.mapped_window(c["grid"][0], c["hdr"][0], 12, 0, c["xf"][0])
        left, top, right, bottom = c["hdr"][0][2:6]
        assert not finite.any() and (c0 == left).all() and (c1 == right).all() and (r0 == top).all() and (r1 == bottom).all()
    B, h, nB, rho2 = wr.window_consts(mr.case("synth", 0, "general", 12)["xf"][0])
    A = mr.case("synth", 0, "general", 12)["xf"][0][:12].reshape(3, 4)[:, :3]
    assert np.abs(B - np.linalg.inv(A)).max() <= 1e-14 and 2.0 ** -29 <= rho2 <= 2.0 ** -28
    assert np.allclose(h, np.linalg.norm(B, axis=1), rtol=1e-14) and np.isclose(nB, np.linalg.norm(B), rtol=1e-14)


# ---- 2. the inputs are adequate ----
def _totals(kind, labels):
    tot = {}
    for label in labels:
        for k, v in counts(kind, label).items():
            tot[k] = tot.get(k, 0) + v
    return tot


def test_plain_inputs_are_adequate():
    tot = _totals("plain", PLAIN_INPUTS)
    print("plain kernel, voxels lost per (mistake, layout):", tot)
    for m in wr.PLAIN_MISTAKES:
        assert tot[m, 0] + tot[m, 1] >= ADEQUATE, (m, tot)
    assert tot["no_union", 0] >= 1 and tot["no_union", 1] >= 1, tot


def test_mapped_inputs_are_adequate():
    tot = _totals("mapped", MAPPED_INPUTS)
    print("mapped kernel, voxels lost per (mistake, layout):", tot)
    for m in wr.MAPPED_MISTAKES:
        assert tot[m, 0] + tot[m, 1] >= ADEQUATE, (m, tot)
    assert tot["no_union", 0] >= 1 and tot["no_union", 1] >= 1, tot
    new = _totals("mapped", [k for k in MAPPED_INPUTS if k.startswith("sparse ")])
    print("... on the sparse frames alone:", new)
    for m in ("T90", "no_Hz"):
        assert new[m, 0] + new[m, 1] >= ADEQUATE, (m, new)


# ---- 3. the new cases ----
@pytest.mark.parametrize("name", list(sp.PLAIN))
def test_sparse_plain_case_is_not_fragile(name):
    r = sp.plain_case(name)["ref"]
    print(f"{name}: {int(r['fragile'].sum())} fragile, {int(r['near'].sum())} near of {r['near'].size}")
    assert r["fragile"].mean() <= ar.FRAGILE_CAP and r["near"].any() and not r["near"].all()
    assert (r["nearest"][r["near"]] >= 0).all() and (r["nearest"][~r["near"]] == -1).all()
    far = ~r["near"]
    assert np.array_equal(r["vol"][:, far].view(np.uint32), r["plain"][:, far].view(np.uint32))


@pytest.mark.parametrize("name", list(sp.MAPPED))
def test_sparse_mapped_case_is_not_fragile(name):
    r = sp.mapped_case(name)["ref"]
    print(f"{name}: {int(r['fragile'].sum())} fragile, {int(r['near'].sum())} near of {r['near'].size}")
    assert r["fragile"].mean() <= ar.FRAGILE_CAP and r["near"].any() and not r["near"].all()
    assert (r["nearest"][r["near"]] >= 0).all() and (r["nearest"][~r["near"]] == -1).all()
    far = ~r["near"]
    assert np.array_equal(r["vol"][:, far].view(np.uint32), np.repeat(r["far"][None], 3, 0)[:, far].view(np.uint32))


@pytest.mark.parametrize("R", [4, 8, 20, 28, 44, 64])
def test_resolution_sources_are_not_fragile(R):
    # (the GPU tier meets the same cap at every R through accurate_ref.compare; these are the resolutions of its slab regimes)
    for kind in ("plain", "mapped"):
        s = sp.res_sources(kind, R)
        assert s["fragile"].reshape(sp.K_RES, -1).mean(axis=1).max() <= ar.FRAGILE_CAP, (kind, R)
        assert min(s["near"]) > 0 and s["vol"].shape == (3, 3, R, R, R) and (s["grid"][:, 4] > 0).all()
    depth, off, hdr = sp.res_pack()
    with np.errstate(invalid="ignore"):
        assert all(0 < int((np.abs(depth[off[i]:off[i + 1]]) >= 1).sum()) <= 24 for i in range(sp.K_RES))


def _unclipped(window_of, hdr):
    """A window function's bounds with the crop taken away: the header's box replaced by one no window reaches."""
    wide = hdr.copy()
    wide[2:6] = (-10 ** 7, -10 ** 7, 10 ** 7, 10 ** 7)
    return window_of(wide)


def test_the_named_frames_are_what_the_gpu_tier_asks_for():
    # a negative-depth frame, plain and mapped
    for c in (sp.plain_case("f3000_negative"), sp.mapped_case("general_f3000_negative")):
        d = c["depth"]
        assert (d[d != 0] < 0).all() and (d != 0).sum() == 40 and c["ref"]["near"].any()
    # voxels within T of the camera plane: items with no finite rectangle next to windowed items, near voxels in both
    for lay in LAYOUTS:
        c = sp.plain_case("camera_plane")
        fin = wr.plain_window(c["grid"][0], c["hdr"][0], c["R"], lay, c["cam"])[4]
        m = sp.mapped_case("rx100_camera_plane")
        mfin = wr.mapped_window(m["grid"][0], m["hdr"][0], m["R"], lay, m["xf"][0], m["cam"])[4]
        for f, near in ((fin, c["ref"]["near"]), (mfin, m["ref"]["near"])):
            assert (near & f).any() and (near & ~f).any() and (~near & f).any(), lay
    # a crop box inside the frame: among the items that hold a near voxel the clip cuts windows on each of the four sides
    # (and leaves others whole on that side)
    for lay in LAYOUTS:
        c = sp.plain_case("boxed")
        m = sp.mapped_case("shear_boxed")
        for case, fn in ((c, lambda h: wr.plain_window(c["grid"][0], h, c["R"], lay, c["cam"])),
                         (m, lambda h: wr.mapped_window(m["grid"][0], h, m["R"], lay, m["xf"][0], m["cam"]))):
            hdr = case["hdr"][0]
            left, top, right, bottom = (int(v) for v in hdr[2:6])
            assert 0 < left and 0 < top and right < sp.IMG_W and bottom < sp.IMG_H
            c0, c1, r0, r1, finite = _unclipped(fn, hdr)
            near = case["ref"]["near"] & finite
            for cut in (c0 < left, c1 > right, r0 < top, r1 > bottom):
                assert (near & cut).any() and (near & ~cut).any(), lay
