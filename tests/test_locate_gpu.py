"""GPU tier of the hand locator (include/tsdf_locate.h): locate_hands against tests/locate_ref.py — the centre within a
rounding bound derived from the terms summed, everything downstream of the centre on the bits —, the round trip through
the existing voxelizers, uint16 frames, the index, independence of the batch, determinism, sentinel-filled outputs, edge
frames, another camera, graph capture, and the composites voxelize_frames / AugmentedStep on a located pack.

The only tolerances: lr.com_bound (a priori, from the number of terms and the sum of their absolute values) for the
centre, and the project's contract figure 1e-5 where a cube-placed volume is compared with the oracle.  Everything else
is equality of bits.  Exact comparisons with the REFERENCE's rectangles and sets rest on the margin condition, which
tests/test_locate_cpu.py asserts on these very inputs."""
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import locate_ref as lr  # noqa: E402

pytestmark = pytest.mark.gpu

VIEW = {torch.float64: torch.int64, torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
FIELDS = ("headers", "offsets", "com", "count", "status", "grid", "max_l", "mid_p")


def dev():
    return torch.device("cuda")


def up(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the shared frames are read-only)


def same(a, b):
    """Equal shapes, types and BITS (a NaN equals itself, -0 is not +0)."""
    if a is None or b is None:
        return a is None and b is None
    if a.dtype is not b.dtype or a.shape != b.shape:
        return False
    v = VIEW.get(a.dtype)
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v)) if v is not None else torch.equal(a, b)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def hip_cam(pkg, cam):
    return pkg.TsdfCam(*cam)


def params(**kw):
    return dict(lr.PARAMS, **kw)


def locate(pkg, frames, cam, **kw):
    """locate_hands on numpy (or device) frames -> (HandCrops, its fields as numpy, the pack cut at offsets[n])."""
    t = frames if isinstance(frames, torch.Tensor) else up(frames)
    crops = pkg.locate_hands(t, cam=hip_cam(pkg, cam), **kw)
    torch.cuda.synchronize()
    assert isinstance(crops, pkg.HandCrops)
    out = {k: (getattr(crops, k).cpu().numpy() if getattr(crops, k) is not None else None) for k in FIELDS}
    out["depth"] = crops.depth.cpu().numpy()[:int(out["offsets"][-1])]
    return crops, out


def same_outputs(a, b, rows_a=None, rows_b=None):
    """Two numpy output dicts equal on the bits, field by field (optionally some rows of each), crops included."""
    ra = range(len(a["status"])) if rows_a is None else rows_a
    rb = range(len(b["status"])) if rows_b is None else rows_b
    assert len(ra) == len(rb)
    for i, j in zip(ra, rb):
        for k in ("headers", "com", "count", "status", "grid", "max_l", "mid_p"):
            assert np.array_equal(bits(a[k][i]), bits(b[k][j])), (k, i, j)
        ca = a["depth"][a["offsets"][i]:a["offsets"][i + 1]]
        cb = b["depth"][b["offsets"][j]:b["offsets"][j + 1]]
        assert np.array_equal(bits(ca), bits(cb)), ("crop", i, j)


def check_offsets(out):
    hdr = out["headers"]
    sizes = (hdr[:, 4] - hdr[:, 2]).astype(np.int64) * (hdr[:, 5] - hdr[:, 3])
    assert out["offsets"].dtype == np.int64 and np.array_equal(out["offsets"], np.concatenate([[0], np.cumsum(sizes)]))


def check_empty_row(out, i, H, W, status):
    assert out["status"][i] == status and out["headers"][i].tolist() == [W, H, 0, 0, 1, 1] and out["count"][i] == 0
    crop = out["depth"][out["offsets"][i]:out["offsets"][i + 1]]
    assert crop.size == 1 and bits(crop)[0] == 0                       # one pixel of +0
    for k in ("com", "grid", "max_l", "mid_p"):
        assert not bits(out[k][i]).any(), k


def check(out, frames, refs, cam, p, R=32):
    """Cases 1 and 2 of the issue for every frame: the centre within the rounding bound of the reference's; headers,
    offsets, count, the packed crop and the cube row recomputed in numpy from the KERNEL'S OWN centre, equal; and
    headers, offsets, count equal to the reference's (the margin condition makes that legitimate)."""
    H, W = frames.shape[1:]
    assert len(out["status"]) == len(refs)
    check_offsets(out)
    worst = 0.0
    for i, r in enumerate(refs):
        if r["status"] != 0:
            check_empty_row(out, i, H, W, r["status"])
            continue
        assert out["status"][i] == 0, i
        com = out["com"][i]
        bound = lr.com_bound(r["centres"], cam)
        err = np.abs(com - r["com"])
        assert (err <= bound).all(), (i, err, bound)
        worst = max(worst, float((err / bound).max()))
        ds = lr.downstream(frames[i], com, cam, p["cube"], p["near"], p["far"], R)
        assert out["headers"][i].tolist() == [W, H, *ds["rect"]], i
        assert out["count"][i] == ds["count"], i
        crop = out["depth"][out["offsets"][i]:out["offsets"][i + 1]]
        assert np.array_equal(bits(crop), bits(ds["crop"])), i
        assert np.array_equal(bits(out["grid"][i]), bits(ds["grid"])), i
        assert bits(out["max_l"][i]) == bits(ds["max_l"]) and np.array_equal(bits(out["mid_p"][i]), bits(ds["mid_p"])), i
        assert ds["rect"] == r["rect"] and ds["count"] == r["count"], i
    return worst


# ---- cases 1, 2: against the reference ----
@pytest.mark.parametrize("n", [1, 3, 17, 300])
def test_small_frames_against_the_reference(pkg, n):
    H, W, cam, _ = lr.SETS["41x30"]
    frames = lr.frames_of("41x30")[:n]
    _, out = locate(pkg, frames, cam)
    worst = check(out, frames, lr.reference("41x30")[:n], cam, params())
    print(f"41x30, n = {n}: largest |c - c_ref| / bound = {worst:.3g}")


@pytest.mark.parametrize("name", ["64x48", "320x240", "640x480"])
def test_larger_frames_against_the_reference(pkg, name):
    H, W, cam, _ = lr.SETS[name]
    frames = lr.frames_of(name)
    _, out = locate(pkg, frames, cam)
    worst = check(out, frames, lr.reference(name), cam, params())
    print(f"{name}, n = {len(frames)}: largest |c - c_ref| / bound = {worst:.3g}")
    if name == "64x48":
        _, out0 = locate(pkg, frames, cam, refine=0)
        check(out0, frames, lr.reference(name, refine=0), cam, params(refine=0))
        _, out16 = locate(pkg, frames, cam, res=16)
        for i in range(len(frames)):
            assert np.array_equal(bits(out16["grid"][i]), bits(lr.glue_cube(out16["com"][i], 250.0, 16, cam[4])[0]))
        _, nogrid = locate(pkg, frames, cam, grid=False)
        assert nogrid["grid"] is None and nogrid["max_l"] is None and nogrid["mid_p"] is None
        for k in ("headers", "offsets", "com", "count", "status", "depth"):
            assert np.array_equal(bits(nogrid[k]), bits(out[k])), k


# ---- case 3: the round trip against what exists ----
@pytest.mark.parametrize("name", ["64x48", "320x240"])
def test_round_trip_through_the_voxelizers(pkg, name):
    H, W, cam, _ = lr.SETS[name]
    hc = hip_cam(pkg, cam)
    tight = [lr.tight_crop(sc) for sc in lr.scenes(name)]
    td = up(np.concatenate([d for d, _ in tight]))
    to = up(np.concatenate([[0], np.cumsum([d.size for d, _ in tight])]).astype(np.int64))
    th = up(np.stack([h for _, h in tight]))
    crops, out = locate(pkg, lr.frames_of(name), cam)
    assert (out["status"] == 0).all()
    assert (out["headers"][:, 4] - out["headers"][:, 2] > (th[:, 4] - th[:, 2]).cpu().numpy()).any()   # not the same boxes
    for R in (16, 32):
        for layout in ("czyx", "cxyz"):
            want = pkg.voxelize(td, to, th, res=R, layout=layout, cam=hc)
            got = pkg.voxelize(crops.depth, crops.offsets, crops.headers, res=R, layout=layout, cam=hc)
            torch.cuda.synchronize()
            assert not bool(want.status.any()) and bool(want.tsdf.any())
            for k in ("tsdf", "max_l", "mid_p", "status"):
                assert same(getattr(got, k), getattr(want, k)), (R, layout, k)
        for dtype in (torch.bfloat16, torch.float16):
            want = pkg.voxelize_lowp(td, to, th, res=R, dtype=dtype, cam=hc)
            got = pkg.voxelize_lowp(crops.depth, crops.offsets, crops.headers, res=R, dtype=dtype, cam=hc)
            torch.cuda.synchronize()
            for k in ("tsdf", "max_l", "mid_p", "status"):
                assert same(getattr(got, k), getattr(want, k)), (R, dtype, k)


# ---- case 4: uint16 frames ----
@pytest.mark.parametrize("shift", [0, 3])
def test_uint16_frames_give_the_bits_of_the_float32_frames(pkg, shift):
    cam = lr.CAM_MID
    frames = lr.frames_of("64x48") if shift == 3 else lr.frames_q1()
    u = frames.astype(np.float64) * 2 ** shift
    assert (u == np.round(u)).all() and u.max() < 65536 and u.min() >= 0
    u16 = u.astype(np.uint16)
    assert np.array_equal(u16.astype(np.float32) * np.float32(2.0 ** -shift), frames)
    _, a = locate(pkg, frames, cam)
    _, b = locate(pkg, u16, cam, shift=shift)
    assert (a["status"] == 0).all()
    same_outputs(a, b)
    assert np.array_equal(a["offsets"], b["offsets"])
    if shift == 3:                                          # the wrong shift is another depth
        _, c = locate(pkg, u16, cam, shift=2)
        assert not np.array_equal(a["com"], c["com"])
    # a slice that starts on an odd element: 2-byte alignment is all uint16 frames need
    flat = torch.zeros(u16.size + 1, dtype=torch.uint16, device=dev())
    flat[1:] = up(u16).reshape(-1)
    _, d = locate(pkg, flat[1:].view(u16.shape), cam, shift=shift)
    same_outputs(a, d)


# ---- case 5: the index ----
def test_index_repeats_and_entries_outside_the_frames(pkg):
    H, W, cam, _ = lr.SETS["64x48"]
    frames = lr.frames_of("64x48")
    n_src = len(frames)
    idx = np.array([3, 3, -1, 0, n_src, 16, 5, 3, -(2 ** 40), 2 ** 40], np.int64)
    _, whole = locate(pkg, frames, cam)
    _, got = locate(pkg, frames, cam, index=up(idx))
    check_offsets(got)
    ok = (idx >= 0) & (idx < n_src)
    assert got["status"].tolist() == [0 if v else 2 for v in ok]
    same_outputs(got, whole, np.nonzero(ok)[0], idx[ok])
    for i in np.nonzero(~ok)[0]:
        check_empty_row(got, i, H, W, 2)
    # the voxelizers report their own status 1 for such a row, and a zero volume
    crops = pkg.locate_hands(up(frames), cam=hip_cam(pkg, cam), index=up(idx))
    b = pkg.voxelize(crops.depth, crops.offsets, crops.headers, res=16, cam=hip_cam(pkg, cam))
    torch.cuda.synchronize()
    assert b.status.cpu().tolist() == [0 if v else 1 for v in ok] and not bool(b.tsdf[2].any())


# ---- cases 6, 7: a frame alone, and twice ----
def test_every_frame_alone_equals_its_row_in_the_batch(pkg):
    for name in ("64x48", "320x240"):
        cam = lr.SETS[name][2]
        frames = lr.frames_of(name)
        _, whole = locate(pkg, frames, cam)
        for i in range(len(frames)):
            _, alone = locate(pkg, frames[i:i + 1], cam)
            same_outputs(alone, whole, [0], [i])


def test_two_calls_give_identical_bits(pkg):
    cam = lr.SETS["41x30"][2]
    t = up(lr.frames_of("41x30"))
    _, a = locate(pkg, t, cam)
    _, b = locate(pkg, t, cam)
    same_outputs(a, b)
    assert np.array_equal(a["offsets"], b["offsets"])


# ---- case 8: sentinel-filled outputs ----
def test_nothing_outside_the_documented_fields_is_written(pkg):
    H, W, cam, _ = lr.SETS["64x48"]
    frames = np.concatenate([lr.frames_of("64x48")[:5], np.zeros((1, H, W), np.float32)])      # and one degenerate frame
    n = len(frames)
    _, want = locate(pkg, frames, cam)
    cap = n * lr.capacity(H, W, 250.0, 100.0, cam[0])
    nan = float("nan")

    def backing(rows, dtype, fill, *tail):
        return torch.full((rows + 2,) + tail, fill, dtype=dtype, device=dev())

    # every output is a slice of a larger sentinel-filled buffer; the depth starts one float in: 4-byte alignment only
    B = dict(depth=torch.full((cap + 40,), nan, device=dev()), offsets=backing(n + 1, torch.int64, -7),
             headers=backing(n, torch.int32, -7, 6), com=backing(n, torch.float64, nan, 3), count=backing(n, torch.int32, -7),
             status=backing(n, torch.int32, -7), grid=backing(n, torch.float32, nan, 8), max_l=backing(n, torch.float32, nan),
             mid_p=backing(n, torch.float32, nan, 3))
    before = {k: v.clone() for k, v in B.items()}
    out = pkg.HandCrops(B["depth"][1:1 + cap], *(B[k][1:-1] for k in pkg.HandCrops._fields[1:]))
    got = pkg.locate_hands(up(frames), cam=hip_cam(pkg, cam), out=out)
    torch.cuda.synchronize()
    assert all(getattr(got, k).data_ptr() == getattr(out, k).data_ptr() for k in pkg.HandCrops._fields)
    g = {k: getattr(got, k).cpu().numpy() for k in FIELDS}
    total = int(g["offsets"][-1])
    g["depth"] = got.depth.cpu().numpy()[:total]
    same_outputs(g, want)
    assert np.array_equal(g["offsets"], want["offsets"]) and g["status"].tolist() == [0] * 5 + [1]
    # nothing at or beyond offsets[n], nothing in front of the buffers, nothing behind them
    assert same(B["depth"][1 + total:], before["depth"][1 + total:]) and same(B["depth"][:1], before["depth"][:1])
    assert total < cap
    for k in pkg.HandCrops._fields[1:]:
        assert same(B[k][:1], before[k][:1]) and same(B[k][-1:], before[k][-1:]), k
    # a depth buffer below the capacity rule is refused before anything is launched
    with pytest.raises(ValueError, match="out.depth"):
        pkg.locate_hands(up(frames), cam=hip_cam(pkg, cam), out=out._replace(depth=B["depth"][1:cap]))


# ---- case 9: edge frames ----
@pytest.mark.parametrize("case", list(lr.edge_cases()))
def test_edge_frames(pkg, case):
    frame, kw = lr.edge_cases()[case]
    r = lr.edge_reference()[case]
    _, out = locate(pkg, frame[None], lr.CAM_MID, **kw)
    check(out, frame[None], [r], lr.CAM_MID, params(**kw))
    if case == "the cube's rectangle is the whole image":
        assert out["headers"][0].tolist() == [64, 48, 0, 0, 64, 48]
    if case == "hand in the corner":
        assert 0 in out["headers"][0][2:4].tolist() or out["headers"][0][4] == 64 or out["headers"][0][5] == 48
    if case == "background inside the seed band":
        assert np.array_equal(out["depth"] != 0, lr.scene_with_patch()["hand"][r["rect"][1]:r["rect"][3],
                                                                                r["rect"][0]:r["rect"][2]].ravel())


def test_edge_frames_in_one_batch_with_good_ones(pkg):
    """Degenerate positions between good ones: one pixel each in the pack, the offsets exact, the neighbours untouched."""
    H, W, cam, _ = lr.SETS["64x48"]
    good = lr.frames_of("64x48")
    cases = lr.edge_cases()
    frames = np.stack([good[0], cases["all zero"][0], good[1], cases["all NaN"][0], cases["beyond far"][0], good[2]])
    refs = [lr.reference("64x48")[0], lr.edge_reference()["all zero"], lr.reference("64x48")[1],
            lr.edge_reference()["all NaN"], lr.edge_reference()["beyond far"], lr.reference("64x48")[2]]
    _, out = locate(pkg, frames, cam)
    check(out, frames, refs, cam, params())
    assert out["status"].tolist() == [0, 1, 0, 1, 1, 0]


# ---- case 10: another camera ----
def test_another_camera_gives_that_cameras_results(pkg):
    frames = lr.frames_of("64x48")
    _, other = locate(pkg, frames, lr.CAM_OTHER)
    check(other, frames, lr.other_camera_reference(), lr.CAM_OTHER, params())
    _, mid = locate(pkg, frames, lr.CAM_MID)
    assert not np.array_equal(other["com"], mid["com"]) and not np.array_equal(other["grid"][:, 4], mid["grid"][:, 4])
    assert (other["count"] != mid["count"]).any()            # eps = 350 mm invalidates the nearer hands' pixels
    # the default camera is the MSRA one
    f320 = up(lr.frames_of("320x240"))
    a = pkg.locate_hands(f320)
    b = pkg.locate_hands(f320, cam=hip_cam(pkg, lr.DEFAULT_CAM))
    torch.cuda.synchronize()
    assert all(same(x, y) for x, y in zip(a[1:], b[1:]))


# ---- case 11: capture ----
def test_captured_launches_replayed_over_changed_frames_equal_the_eager_call(pkg):
    H, W, cam, _ = lr.SETS["64x48"]
    hc = hip_cam(pkg, cam)
    sets = [lr.frames_of("64x48")[:8], lr.frames_of("64x48")[8:16], lr.frames_q1()[:8]]
    static = up(sets[0])
    n = 8
    cap = n * lr.capacity(H, W, 250.0, 100.0, cam[0])
    out = pkg.HandCrops(torch.zeros(cap, device=dev()), torch.zeros(n + 1, dtype=torch.int64, device=dev()),
                        torch.zeros((n, 6), dtype=torch.int32, device=dev()), torch.zeros((n, 3), dtype=torch.float64, device=dev()),
                        torch.zeros(n, dtype=torch.int32, device=dev()), torch.zeros(n, dtype=torch.int32, device=dev()),
                        torch.zeros((n, 8), device=dev()), torch.zeros(n, device=dev()), torch.zeros((n, 3), device=dev()))
    pkg.locate_hands(static, cam=hc, out=out)             # eagerly once: library loads and the device check happen here
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        pkg.locate_hands(static, cam=hc, out=out)
    for frames in (sets[1], sets[2], sets[0]):
        static.copy_(up(frames))
        g.replay()
        torch.cuda.synchronize()
        got = {k: getattr(out, k).cpu().numpy() for k in FIELDS}
        got["depth"] = out.depth.cpu().numpy()[:int(got["offsets"][-1])]
        _, want = locate(pkg, frames, cam)
        same_outputs(got, want)
        assert np.array_equal(got["offsets"], want["offsets"])


# ---- case 12: the composites ----
def _joints(com, seed):
    """21 joints about every centre (sigma 60 mm: some labels leave the cube and are clamped)."""
    rng = np.random.default_rng(seed)
    return (com[:, None, :] + rng.normal(0.0, 60.0, (len(com), 21, 3))).astype(np.float32).reshape(len(com), 63)


def test_voxelize_frames_cube_placement(pkg):
    H, W, cam, _ = lr.SETS["64x48"]
    hc = hip_cam(pkg, cam)
    frames = np.concatenate([lr.frames_of("64x48")[:7], np.zeros((1, H, W), np.float32)])
    t = up(frames)
    _, ref_out = locate(pkg, frames, cam)
    gt = up(_joints(ref_out["com"], 7))
    batch, crops, gt_nor = pkg.voxelize_frames(t, 32, placement="cube", gt=gt, cam=hc)
    tsdf, st = pkg.voxelize_grid(crops.depth, crops.offsets, crops.headers, crops.grid, res=32, cam=hc)
    torch.cuda.synchronize()
    assert isinstance(batch, pkg.TsdfBatch) and isinstance(crops, pkg.HandCrops)
    assert same(batch.tsdf, tsdf) and same(batch.status, st) and batch.max_l is crops.max_l and batch.mid_p is crops.mid_p
    assert st.cpu().tolist() == [0] * 7 + [1] and not bool(tsdf[7].any()) and bool(tsdf[:7].any())
    assert same(gt_nor, pkg.normalize_joints(gt, crops.max_l, crops.mid_p))
    nor = gt_nor.cpu().numpy()
    assert (nor[7] == 0.5).all() and 0.0 <= nor.min() and nor.max() <= 1.0 and (nor[:7] != 0.5).any()
    assert batch.max_l.cpu().tolist() == [250.0] * 7 + [0.0]
    # what the placement means: the oracle's voxel loop on the located crop and the cube's row
    for i in (0, 3):
        o0, o1 = int(ref_out["offsets"][i]), int(ref_out["offsets"][i + 1])
        row = ref_out["grid"][i]
        want = oracle.voxels(ref_out["depth"][o0:o1], ref_out["headers"][i], row[:3], row[3], row[4], R=32, cam=cam)
        assert np.abs(batch.tsdf[i].cpu().numpy() - want).max() <= 1e-5, i
    # the 2-byte forms, and the other layout
    for dtype in (torch.bfloat16, torch.float16):
        b2, c2 = pkg.voxelize_frames(t, 32, placement="cube", dtype=dtype, layout="cxyz", cam=hc)
        t2, s2 = pkg.voxelize_grid_lowp(c2.depth, c2.offsets, c2.headers, c2.grid, res=32, layout="cxyz", dtype=dtype, cam=hc)
        torch.cuda.synchronize()
        assert b2.tsdf.dtype is dtype and same(b2.tsdf, t2) and same(b2.status, s2) and same(c2.grid, crops.grid)


def test_voxelize_frames_aabb_placement(pkg):
    H, W, cam, _ = lr.SETS["64x48"]
    hc = hip_cam(pkg, cam)
    t = up(lr.frames_of("64x48")[:7])
    crops = pkg.locate_hands(t, cam=hc, grid=False)
    d, o, h = crops.depth, crops.offsets, crops.headers
    want = pkg.voxelize(d, o, h, res=16, cam=hc)
    gt = up(_joints(want.mid_p.cpu().numpy().astype(np.float64), 8))
    batch, c1 = pkg.voxelize_frames(t, 16, cam=hc)
    torch.cuda.synchronize()
    assert c1.grid is None and same(c1.depth[:int(o[-1])], d[:int(o[-1])]) and same(c1.headers, h)
    for k in ("tsdf", "max_l", "mid_p", "status"):
        assert same(getattr(batch, k), getattr(want, k)), k
    wl, wnor = pkg.voxelize_labels(d, o, h, gt, res=16, cam=hc)
    bl, _, nor = pkg.voxelize_frames(t, 16, gt=gt, cam=hc)
    torch.cuda.synchronize()
    assert same(bl.tsdf, wl.tsdf) and same(nor, wnor)
    w2 = pkg.voxelize_lowp(d, o, h, res=16, dtype=torch.bfloat16, cam=hc)
    b2, _, nor2 = pkg.voxelize_frames(t, 16, dtype=torch.bfloat16, gt=gt, cam=hc)
    torch.cuda.synchronize()
    assert same(b2.tsdf, w2.tsdf) and same(b2.max_l, w2.max_l) and same(nor2, pkg.normalize_joints(gt, w2.max_l, w2.mid_p))


def test_augmented_step_on_a_located_pack(pkg):
    H, W, cam, _ = lr.SETS["64x48"]
    hc = hip_cam(pkg, cam)
    t = up(lr.frames_of("64x48")[:8])
    crops = pkg.locate_hands(t, cam=hc)
    step = pkg.AugmentedStep(crops.depth, crops.offsets, crops.headers, 4, res=32, cam=hc)
    idx = torch.tensor([5, 1, 1, 6], dtype=torch.int64, device=dev())
    for key, c0 in ((77, 5), (78, 9)):
        out = step.step(idx, key=key, counter0=c0)
        torch.cuda.synchronize()
        xf = step.xforms.clone()
        assert not same(xf, torch.from_numpy(pkg.augment.identity_affines(4)).to(dev()))
        # the batch's frames located in batch order are the same crops (a frame's bits do not depend on its position) ...
        b4 = pkg.locate_hands(t, cam=hc, index=idx)
        want = pkg.voxelize_aug(b4.depth, b4.offsets, b4.headers, xf, res=32, cam=hc)
        torch.cuda.synchronize()
        assert not bool(want.status.any()) and bool(want.tsdf.any())
        for k in ("tsdf", "max_l", "mid_p", "status"):
            assert same(getattr(out, k), getattr(want, k)), (key, k)
