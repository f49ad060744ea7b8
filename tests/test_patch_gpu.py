"""GPU tier of the depth-image patches (include/tsdf_patch.h): libtsdf_patch.so compared BIT FOR BIT with the numpy
restatement tests/patch_ref.py — patches as int32 / int16 patterns, uvd, valid and status equal — on the input families
of that file, at the smallest shapes at which the kernel can go wrong: every plan shape (a band that is the whole patch, a
short last band, idle lanes), both interpolations, the three element types, frames and packs, rectangles that leave the
source on every side, every invalid depth, every map of the affine family, indices, statuses and cameras."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patch_ref as pr  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIZES = (8, 16, 24, 40, 64, 96, 128, 176, 512)
DTYPES = ((pr.F32, torch.float32), (pr.F16, torch.float16), (pr.BF16, torch.bfloat16))
INTERPS = ((0, "nearest"), (1, "bilinear"))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fam():
    return pr.families()


def to(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def cam_of(pkg, cam):
    return None if cam == pr.CAM else pkg.TsdfCam(*cam)


def host_bits(t):
    """A patch tensor as the integer patterns patch_ref.bits gives."""
    return (t.view(torch.int32) if t.dtype is torch.float32 else t.view(torch.int16)).cpu().numpy()


class Device:
    """A family's arrays on the GPU, uploaded once."""

    def __init__(self, pkg, dev, c):
        self.pkg, self.c = pkg, c
        self.source = [to(dev, c["source"])] if c["kind"] == "frames" else [to(dev, a) for a in c["source"]]
        self.com = to(dev, c["com"])
        self.cube = to(dev, c["cube"]) if np.ndim(c["cube"]) else float(c["cube"])
        self.kw = dict(affine=to(dev, c["affine"]), index=to(dev, c["index"]), status=to(dev, c["status"]), cam=cam_of(pkg, c["cam"]),
                       background=c["background"])

    def run(self, S, interp, dtype, **over):
        fn = self.pkg.frame_patches if self.c["kind"] == "frames" else self.pkg.crop_patches
        kw = dict(self.kw, size=S, cube=self.cube, interp=interp, dtype=dtype)
        kw.update(over)
        return fn(*self.source, kw.pop("com", self.com), **kw)


def check(pkg, dev, c, sizes, interps=INTERPS, dtypes=DTYPES):
    """The family at every given size, interpolation and element type against the restatement."""
    d = Device(pkg, dev, c)
    for S in sizes:
        for code, name in interps:
            want, want_st = pr.reference(c, S, code)
            for dcode, dtype in dtypes:
                got = d.run(S, name, dtype)
                assert got.patch.shape == (len(c["com"]), 1, S, S) and got.patch.dtype is dtype
                assert np.array_equal(got.status.cpu().numpy(), want_st), (S, name, dtype)
                bad = np.flatnonzero((host_bits(got.patch)[:, 0] != pr.bits(want, dcode)).reshape(len(want), -1).any(axis=1))
                assert bad.size == 0, (S, name, dtype, bad.tolist())
    return d


# ---- every plan shape, on the seven small sources ----
@pytest.mark.parametrize("S", SIZES)
def test_every_size_type_and_interpolation_on_the_small_sources(pkg, dev, fam, S):
    """1 x 1, 1 x 7, 7 x 1, 3 x 3 and a 37 x 29 crop as one pack; a 16 x 12 frame; one 320 x 240 frame."""
    for name in ("pack", "tiny", "frame"):
        check(pkg, dev, fam[name], (S,))
    for dcode, dtype in DTYPES:
        assert pkg.patch_plan(S, dtype) == pr.plan(S, dcode)


def test_up_and_down_sampling(pkg, dev, fam):
    check(pkg, dev, fam["up"], (64,))        # a 5-pixel rectangle
    check(pkg, dev, fam["down"], (8,))       # a 300-pixel rectangle


def test_the_rectangle_leaves_the_frame_on_every_side(pkg, dev, fam):
    d = check(pkg, dev, fam["borders"], (40,), dtypes=DTYPES[:1])
    got = d.run(40, "nearest", torch.float32)
    assert (got.patch[8:10] == 1.0).all() and (got.patch[:8] != 1.0).flatten(1).any(dim=1).all()


def test_depths_at_the_cube_faces_half_integer_taps_and_zero_weight(pkg, dev, fam):
    """exact: cd +- h kept, one float32 step beyond dropped, every invalid kind, fx == 0 with only the right-hand tap valid;
    exact_half: u on exact half-integers."""
    for name in ("exact", "exact_half"):
        d = check(pkg, dev, fam[name], (8,))
    got = Device(pkg, dev, fam["exact"]).run(8, "bilinear", torch.float32).patch[0, 0].cpu().numpy()
    assert got[2, 2] == -1.0 and got[3, 2] == 1.0 and got[2, 3] == 7.0 and got[3, 3] == 7.0 and (got[:2] == 7.0).all()
    assert d is not None


# ---- the affine family ----
def test_the_affine_family(pkg, dev, fam):
    c = fam["affine"]
    names = list(pr.affine_family())
    d = check(pkg, dev, c, (64,), dtypes=(DTYPES[0], DTYPES[2]))
    for _, interp in INTERPS:
        got = d.run(64, interp, torch.float32)
        plain = d.run(64, interp, torch.float32, affine=None)
        assert torch.equal(got.patch[names.index("identity")].view(torch.int32), plain.patch[0].view(torch.int32))   # bits equal to None
        assert got.status.tolist() == [1 if k == "nan" else 0 for k in names]
        assert (got.patch[names.index("huge")] == 1.0).all() and (got.patch[names.index("nan")] == 1.0).all()
        assert (got.patch[names.index("singular")] != 1.0).any()                     # the patch is fine; the labels are not
    j, com = pr.joints_family(n=len(names))
    com[:] = c["com"]
    lab = pkg.joints_to_uvd(to(dev, j), to(dev, com), affine=to(dev, c["affine"]))
    want = pr.uvd(j, com, affine=c["affine"])
    assert [np.array_equal(a.cpu().numpy().view(np.int32), b.view(np.int32)) for a, b in zip(lab, want)] == [True] * 3
    assert lab.status.tolist() == [1 if k in ("nan", "singular") else 0 for k in names]


# ---- batches: cubes, statuses, indices ----
def test_per_position_cubes_statuses_and_indices(pkg, dev, fam):
    c = fam["batch"]
    d = check(pkg, dev, c, (24, 96))
    got = d.run(96, "bilinear", torch.float32)
    assert got.status.tolist() == [0, 0, 1, 2, 2, 1, 0, 1, 1]
    assert torch.equal(got.patch[1], got.patch[1]) and (got.patch[2:6] == 1.0).all()
    # a per-position cube against the scalar; a position alone against the same position in the batch
    for i in (0, 1, 6):
        alone = pkg.frame_patches(d.source[0], d.com[i:i + 1], size=96, cube=float(c["cube"][i]), interp="bilinear",
                                  index=d.kw["index"][i:i + 1])
        assert torch.equal(alone.patch[0].view(torch.int32), got.patch[i].view(torch.int32)) and alone.status.tolist() == [0]
    # index with duplicates: positions 1 and 2 read frame 0, 5 and 6 frame 1
    assert c["index"].tolist() == [2, 0, 0, -1, 3, 1, 1, 2, 0]


def test_float32_centres_are_widened(pkg, dev, fam):
    c = fam["frame"]
    d = Device(pkg, dev, c)
    com32 = c["com"].astype(np.float32)
    got = d.run(64, "bilinear", torch.float32, com=to(dev, com32))
    want, _ = pr.patches(pr.source_of(c), com32.astype(np.float64), S=64, interp=1)
    assert np.array_equal(host_bits(got.patch)[:, 0], pr.bits(want, pr.F32))


def test_uint16_frames_at_every_shift_equal_the_float32_frames_of_the_same_values(pkg, dev, fam):
    frame = fam["frame"]["source"][0]
    com = to(dev, fam["frame"]["com"])
    for shift in range(8):
        seen = np.isfinite(frame) & (frame > 0)
        q = np.minimum(np.rint(np.where(seen, frame, 0).astype(np.float64) * 2 ** shift), 65535).astype(np.uint16)
        wide = pr.widen(q, shift)
        assert wide.dtype == np.float32 and np.array_equal(wide.astype(np.float64) * 2 ** shift, q.astype(np.float64))
        want, _ = pr.patches(pr.frames_source(wide[None]), fam["frame"]["com"], S=40, interp=1)
        a = pkg.frame_patches(to(dev, q[None]), com, size=40, interp="bilinear", shift=shift)
        b = pkg.frame_patches(to(dev, wide[None]), com, size=40, interp="bilinear")
        assert np.array_equal(host_bits(a.patch)[:, 0], pr.bits(want, pr.F32)) and torch.equal(a.patch, b.patch), shift
        if shift <= 5:                                                # beyond, 452 mm saturates the 16 bits
            assert (a.patch != 1.0).any()
        a = pkg.frame_patches(to(dev, q[None]), com, size=40, shift=shift, dtype=torch.float16)
        assert np.array_equal(host_bits(a.patch)[:, 0], pr.bits(pr.patches(pr.frames_source(wide[None]), fam["frame"]["com"], S=40)[0], pr.F16))


def test_packs_with_a_refused_header_and_a_payload_beyond_the_buffer(pkg, dev, fam):
    d = check(pkg, dev, fam["badpack"], (16, 64), dtypes=DTYPES[:2])
    got = d.run(64, "nearest", torch.float32)
    assert got.status.tolist() == [0, 2, 2] and (got.patch[1:] == 1.0).all() and (got.patch[0] != 1.0).any()


def test_a_non_default_camera(pkg, dev, fam):
    check(pkg, dev, fam["cam"], (40, 128), dtypes=DTYPES[:1])


# ---- the labels ----
def test_labels_and_the_way_back(pkg, dev):
    for name, (j, com, kw) in pr.label_families().items():
        dkw = {k: (cam_of(pkg, v) if k == "cam" else to(dev, v) if np.ndim(v) else v) for k, v in kw.items()}
        lab = pkg.joints_to_uvd(to(dev, j), to(dev, com), **dkw)
        want = pr.uvd(j, com, **kw)
        for a, b, what in zip(lab, want, ("uvd", "valid", "status")):
            assert np.array_equal(a.cpu().numpy().view(np.int32), b.view(np.int32)), (name, what)
        dkw.pop("status", None)
        back = pkg.uvd_to_joints(lab.uvd, to(dev, com), **dkw)
        want_back = pr.joints_back(want[0], com, **{k: v for k, v in kw.items() if k != "status"})
        assert np.array_equal(back.cpu().numpy().view(np.int32), want_back.view(np.int32)), name
        flat = pkg.joints_to_uvd(to(dev, j.reshape(len(j), -1)), to(dev, com), **dict(dkw, status=dkw.get("status")))
        assert flat.uvd.shape == lab.uvd.shape
    j, com, _ = pr.label_families()["plain"]
    lab = pkg.joints_to_uvd(to(dev, j), to(dev, com))
    assert lab.valid[0, 1] == 0 and lab.valid[2, 3] == 0 and lab.valid[3, 4] == 0 and not lab.uvd[0, 1].any()      # NaN, Z == 0, Z > 0


# ---- determinism, buffers ----
def test_two_calls_out_buffers_and_a_misaligned_out(pkg, dev, fam):
    c = fam["batch"]
    d = Device(pkg, dev, c)
    a, b = d.run(40, "bilinear", torch.bfloat16), d.run(40, "bilinear", torch.bfloat16)
    assert torch.equal(a.patch.view(torch.int16), b.patch.view(torch.int16)) and torch.equal(a.status, b.status)
    out = pkg.PatchBatch(torch.full_like(a.patch, 9.0), torch.full_like(a.status, 9))
    got = d.run(40, "bilinear", torch.bfloat16, out=out)
    assert got is out and torch.equal(out.patch.view(torch.int16), a.patch.view(torch.int16)) and torch.equal(out.status, a.status)
    n = len(c["com"])
    buf = torch.zeros(n * 40 * 40 + 4, dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="16-byte aligned"):
        d.run(40, "bilinear", torch.bfloat16, out=pkg.PatchBatch(buf[1:n * 1600 + 1].view(n, 1, 40, 40), a.status.clone()))
    assert not buf.any()
    lab = pkg.joints_to_uvd(*[to(dev, t) for t in pr.joints_family()[:2]])
    out = pkg.UvdBatch(torch.full_like(lab.uvd, 9.0), torch.full_like(lab.valid, 9), torch.full_like(lab.status, 9))
    again = pkg.joints_to_uvd(*[to(dev, t) for t in pr.joints_family()[:2]], out=out)
    assert again is out and all(torch.equal(x, y) for x, y in zip(out, lab))


# ---- the chain ----
def test_patch_frames_equals_its_explicit_chain(pkg, dev, fam):
    frames = to(dev, fam["batch"]["source"])
    j, _ = pr.joints_family(n=3)
    gt = to(dev, j)
    aff = pkg.patch_affines(torch.tensor([0.2, -0.4, 0.0], device=dev), torch.tensor([1.1, 0.9, 1.0], device=dev),
                            torch.tensor([[0.05, 0.0], [0.0, -0.1], [0.0, 0.0]], device=dev))
    patches, crops, lab = pkg.patch_frames(frames, 96, gt=gt, affine=aff, interp="bilinear", dtype=torch.float16, cube=220.0)
    want_crops = pkg.locate_hands(frames, cube=220.0, grid=False)
    used = int(crops.offsets[-1])                                      # the tail of the packed depth is unwritten
    assert all(torch.equal(a, b) for a, b in zip(crops[1:6], want_crops[1:6])) and crops.grid is None
    assert torch.equal(crops.depth[:used], want_crops.depth[:used])
    assert crops.status.tolist() == [0, 0, 0]
    want = pkg.frame_patches(frames, crops.com, size=96, cube=220.0, interp="bilinear", dtype=torch.float16, affine=aff, status=crops.status)
    assert torch.equal(patches.patch.view(torch.int16), want.patch.view(torch.int16)) and torch.equal(patches.status, want.status)
    want_lab = pkg.joints_to_uvd(gt, crops.com, cube=220.0, affine=aff, status=crops.status)
    assert all(torch.equal(a, b) for a, b in zip(lab, want_lab))
    # and the restatement on the located centres
    ref, ref_st = pr.patches(pr.frames_source(fam["batch"]["source"]), crops.com.cpu().numpy(), S=96, cube=220.0, interp=1,
                             affine=aff.cpu().numpy())
    assert np.array_equal(host_bits(patches.patch)[:, 0], pr.bits(ref, pr.F16)) and patches.status.tolist() == ref_st.tolist()
    assert (patches.patch.float() != 1.0).flatten(1).any(dim=1).all()
    two = pkg.patch_frames(frames, 96)
    assert len(two) == 2 and two[0].patch.dtype is torch.float32 and tuple(two[0].patch.shape) == (3, 1, 96, 96)


def test_a_graph_replay_after_the_centres_and_maps_changed_in_place(pkg, dev, fam):
    c = fam["cam"]
    frames, cam = to(dev, c["source"]), cam_of(pkg, c["cam"])
    com, aff = to(dev, c["com"]).clone(), pkg.patch_affines(n=3, device=dev)
    j, _ = pr.joints_family(n=3)
    gt = to(dev, j)
    out = pkg.PatchBatch(torch.zeros((3, 1, 64, 64), device=dev), torch.zeros(3, dtype=torch.int32, device=dev))
    lab = pkg.UvdBatch(torch.zeros((3, 21, 3), device=dev), torch.zeros((3, 21), dtype=torch.int32, device=dev),
                       torch.zeros(3, dtype=torch.int32, device=dev))
    pkg.frame_patches(frames, com, size=64, cube=180.0, interp="bilinear", affine=aff, cam=cam, out=out)     # loads the library
    pkg.joints_to_uvd(gt, com, cube=180.0, affine=aff, cam=cam, out=lab)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
        pkg.frame_patches(frames, com, size=64, cube=180.0, interp="bilinear", affine=aff, cam=cam, out=out)
        pkg.joints_to_uvd(gt, com, cube=180.0, affine=aff, cam=cam, out=lab)
    new_com = c["com"] + np.array([[3.0, -2.0, 5.0], [-4.0, 1.0, -6.0], [0.5, 0.25, 0.0]])
    new_aff = pr.affines([0.3, -0.2, 3.0], [1.2, 0.8, 1.0], [[0.1, 0.0], [0.0, 0.1], [-0.05, 0.05]])
    com.copy_(to(dev, new_com))
    aff.copy_(to(dev, new_aff))
    for t in (*out, *lab):
        t.zero_()
    g.replay()
    torch.cuda.synchronize(dev)
    want, want_st = pr.patches(pr.frames_source(c["source"]), new_com, S=64, cube=180.0, interp=1, affine=new_aff, cam=c["cam"])
    assert np.array_equal(host_bits(out.patch)[:, 0], pr.bits(want, pr.F32)) and out.status.tolist() == want_st.tolist()
    for a, b in zip(lab, pr.uvd(j, new_com, cube=180.0, affine=new_aff, cam=c["cam"])):
        assert np.array_equal(a.cpu().numpy().view(np.int32), b.view(np.int32))
