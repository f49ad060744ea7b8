"""GPU tier of the farthest-point sampled clouds (include/tsdf_fps.h): libtsdf_fps.so against the numpy restatement
(tests/fps_ref.py), BIT FOR BIT — ``pixel`` equal, ``points`` and ``radius2`` equal as int32 bit patterns, ``count`` and
``status`` equal — on the frame zoo, sixteen crops at M = 1024, under maps, through both forms, indexed, batched, on a
side stream, captured into a graph, on clouds, and as the last launch of the augmented step.  Each reference is computed
once per module."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fps_ref as fr  # noqa: E402
import frame_zoo as fz  # noqa: E402
import map_geom_ref as mg  # noqa: E402
import occupancy_ref as orf  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BIG = 200000     # a capacity above every count here


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def on(dev, pack):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in pack)


def host(b):
    """An FpsBatch as a tests/fps_ref.py Fps of numpy arrays."""
    return fr.Fps(*[None if t is None else t.cpu().numpy() for t in b])


def equal(a, b):
    """Two FpsBatch, bit for bit, on the device."""
    return all(torch.equal(x.view(torch.int32) if x.dtype is torch.float32 else x, y.view(torch.int32) if y.dtype is torch.float32 else y)
               for x, y in zip(a, b))


# ---- the inputs and their references, once ----
@pytest.fixture(scope="module")
def crops(dev):
    pack = fr.crops(16)
    return pack, on(dev, pack), fr.batch(*pack, 1024, capacity=BIG)


@pytest.fixture(scope="module")
def zoo(dev):
    pack = fr.zoo_pack()[0]
    return pack, on(dev, pack), fr.batch(*pack, 200, capacity=BIG)


@pytest.fixture(scope="module")
def exact(dev):
    pack = fr.exact_pack()
    return pack, on(dev, pack), fr.batch(*pack, 200)


def small_cases(crops, zoo, exact):
    """(name, device pack, reference, M of the reference) of every small case: what runs again under form=1."""
    return [("zoo", zoo[1], zoo[2], 200), ("exact", exact[1], exact[2], 200), ("crops", crops[1], crops[2], 1024)]


# ---- the frame zoo: count below, equal to and above M ----
@pytest.mark.parametrize("M", fr.ZOO_M)
def test_frame_zoo(pkg, zoo, exact, M):
    for name, (_, t, ref) in (("zoo", zoo), ("exact", exact)):
        got = pkg.farthest_points(*t, points=M, capacity=int(ref.count.max()) or 1)
        assert fr.same(host(got), ref, M) is None, (name, fr.same(host(got), ref, M))
    ref = exact[2]
    assert ref.count.tolist() == [7, 63, 64, 0] and ref.status.tolist() == [0, 0, 0, 1]
    counts = np.concatenate([zoo[2].count, ref.count])
    assert (counts < M).any() and (counts == M).any() == (M in (1, 2, 7, 64)) and (counts > M).any()
    assert (counts > fr.RESIDENT).sum() >= 3


def test_sixteen_crops_at_1024(pkg, crops):
    _, t, ref = crops
    over = ref.count > fr.RESIDENT
    assert over.sum() == 2 and not ref.status.any()                      # two of them stream, reached naturally
    got = host(pkg.farthest_points(*t, points=1024, capacity=int(ref.count.max())))
    assert fr.same(got, ref) is None, fr.same(got, ref)
    assert (got.radius2[:, 1:] <= got.radius2[:, :-1]).all() and np.isposinf(got.radius2[:, 0]).all()
    # the hierarchy costs one call: the first 512 and 128 rows are those calls' results
    for k in (512, 128):
        assert fr.same(host(pkg.farthest_points(*t, points=k, capacity=int(ref.count.max()))), ref, k) is None, k


def test_over_capacity_without_a_workspace_is_status_3_with_the_true_count(pkg, crops):
    pack, t, ref = crops
    want = fr.batch(*pack, 64)                                           # no workspace: the reference's rule
    assert sorted(want.status.tolist()) == [0] * 14 + [3, 3] and np.array_equal(want.count, ref.count)
    got = host(pkg.farthest_points(*t, points=64))
    assert fr.same(got, want) is None, fr.same(got, want)
    over = want.status == 3
    assert (got.pixel[over] == -1).all() and not got.points[over].any() and not got.radius2[over].any()
    # a workspace that is too small for one of the two
    cap = int(np.sort(ref.count)[-2])
    want = fr.batch(*pack, 64, capacity=cap)
    assert sorted(want.status.tolist()) == [0] * 15 + [3]
    got = host(pkg.farthest_points(*t, points=64, capacity=cap))
    assert fr.same(got, want) is None, fr.same(got, want)


# ---- maps ----
def test_identity_obb_and_augmentation_maps(pkg, dev, crops):
    pack, t, ref = crops
    n = 16
    ident = np.tile(mg.pack(np.eye(3), np.zeros(3)), (n, 1))
    plain = pkg.farthest_points(*t, points=128, capacity=BIG)
    mapped = pkg.farthest_points(*t, points=128, capacity=BIG, xforms=torch.from_numpy(ident).to(dev))
    # identity rows: the unmapped result — the same samples at the same radii, and the same points; only a zero keeps no
    # sign: the row of the optical axis has p_y = -0, and (0 * p_x + 1 * -0) + (0 * p_z + 0) is +0 (include/tsdf_fps.h)
    assert fr.same(host(plain), ref, 128) is None
    assert torch.equal(plain.pixel, mapped.pixel) and torch.equal(plain.radius2.view(torch.int32), mapped.radius2.view(torch.int32))
    assert torch.equal(plain.count, mapped.count) and torch.equal(plain.status, mapped.status)
    assert torch.equal(plain.points, mapped.points)                          # as values: -0 == +0
    differ = plain.points.view(torch.int32) != mapped.points.view(torch.int32)
    assert bool((plain.points[differ] == 0).all())
    want = fr.batch(*pack, 128, xforms=ident, capacity=BIG)
    assert fr.same(host(mapped), want) is None                               # and the restatement's bits, zeros included
    obb = pkg.obb_xforms(*t)
    assert not obb.status.any()
    for name, xf in (("obb", obb.xforms.cpu().numpy()), ("aug", fz.aug_maps(orf.placed(pack)[1]))):
        want = fr.batch(*pack, 128, xforms=xf, capacity=BIG)
        got = host(pkg.farthest_points(*t, points=128, capacity=BIG, xforms=torch.from_numpy(xf).to(dev)))
        assert fr.same(got, want) is None, (name, fr.same(got, want))
        if name == "aug":   # a stretch changes the selection (every fifth map is the identity); a rotation need not
            changed = (want.pixel != ref.pixel[:, :128]).any(1)
            assert changed.sum() >= 8 and not changed[::5].any()


# ---- capacity and forms ----
@pytest.fixture(scope="module")
def dense(dev):
    """A 96 x 96 crop and one full 320 x 240 frame, every pixel valid: 9216 candidates (below the resident cap, streamed by
    the hint) and 76800 (above it, streamed naturally)."""
    rng = np.random.default_rng(5)
    imgs = []
    for bh, bw in ((96, 96), (240, 320)):
        ys, xs = np.mgrid[0:bh, 0:bw]
        imgs.append((420 + 60 * np.sin(xs / 17.0) * np.cos(ys / 23.0) + rng.uniform(-2, 2, (bh, bw))).astype(np.float32))
    pack = fz.pack(imgs, [(101, 77), (0, 0)])
    return pack, on(dev, pack), fr.batch(*pack, 128, capacity=76800)


def test_dense_frames_through_the_streaming_form(pkg, dense):
    _, t, ref = dense
    assert ref.count.tolist() == [9216, 76800] and not ref.status.any()
    assert fr.holds(9216, 76800, 1) == 2 and fr.holds(76800, 76800, 0) == 2 and fr.holds(9216, 76800, 0) == 1
    streamed = pkg.farthest_points(*t, points=128, capacity=76800, form=1)
    assert fr.same(host(streamed), ref) is None, fr.same(host(streamed), ref)
    chosen = pkg.farthest_points(*t, points=128, capacity=76800)         # the small one resident, the large one streaming
    assert equal(streamed, chosen)
    bare = host(pkg.farthest_points(*t, points=128))
    assert bare.status.tolist() == [0, 3] and bare.count.tolist() == [9216, 76800]
    assert np.array_equal(bare.pixel[0], ref.pixel[0]) and (bare.pixel[1] == -1).all()
    tight = host(pkg.farthest_points(*t, points=128, capacity=76799))
    assert tight.status.tolist() == [0, 3] and tight.count.tolist() == [9216, 76800]


def test_every_small_case_again_through_the_streaming_form(pkg, crops, zoo, exact):
    for name, t, ref, M in small_cases(crops, zoo, exact):
        cap = int(ref.count.max())
        a = pkg.farthest_points(*t, points=M, capacity=cap, form=0)
        b = pkg.farthest_points(*t, points=M, capacity=cap, form=1)
        assert equal(a, b), name
        assert fr.same(host(b), ref, M) is None, name


# ---- index ----
def test_index_with_repeats_and_entries_out_of_range(pkg, dev, crops):
    pack, t, ref = crops
    index = [3, 3, -1, 16, 1, 2 ** 40, 15, 3, -2 ** 40, 0]
    want = fr.batch(*pack, 64, index=index, capacity=BIG)
    assert want.status.tolist() == [0, 0, 2, 2, 0, 2, 0, 0, 2, 0]
    got = host(pkg.farthest_points(*t, points=64, index=torch.tensor(index, device=dev), capacity=BIG))
    assert fr.same(got, want) is None, fr.same(got, want)
    assert np.array_equal(got.pixel[0], got.pixel[1]) and np.array_equal(got.pixel[0], ref.pixel[3, :64])
    # one map per batch position, not per source frame
    xf = fz.aug_maps(np.zeros((10, 3)) + [0.0, 0.0, -400.0])
    want = fr.batch(*pack, 64, index=index, xforms=xf, capacity=BIG)
    got = host(pkg.farthest_points(*t, points=64, index=torch.tensor(index, device=dev), capacity=BIG,
                                   xforms=torch.from_numpy(xf).to(dev)))
    assert fr.same(got, want) is None, fr.same(got, want)
    assert not np.array_equal(got.pixel[1], got.pixel[7])                # the same frame under two maps


# ---- alone, in any batch, twice, on a side stream ----
def test_a_frame_s_bits_do_not_depend_on_its_company(pkg, dev, crops):
    pack, t, ref = crops
    whole = pkg.farthest_points(*t, points=200, capacity=BIG)
    assert fr.same(host(whole), ref, 200) is None
    again = pkg.farthest_points(*t, points=200, capacity=BIG)
    assert equal(whole, again)
    for g in (0, 7, 15):
        alone = pkg.farthest_points(*t, points=200, capacity=BIG, index=torch.tensor([g], device=dev))
        assert all(torch.equal(a[0], w[g]) for a, w in zip(alone, whole)), g
    perm = torch.tensor([15, 2, 9, 0, 11], device=dev)
    part = pkg.farthest_points(*t, points=200, capacity=BIG, index=perm)
    assert all(torch.equal(p, w[perm]) for p, w in zip(part, whole))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        there = pkg.farthest_points(*t, points=200, capacity=BIG)
    side.synchronize()
    assert equal(whole, there)


def test_every_output_byte_is_written(pkg, dev, crops, exact):
    for (_, t, ref), n in ((crops, 16), (exact, 4)):
        for capacity in (None, BIG):
            out = pkg.FpsBatch(torch.full((n, 70, 3), -7.5, device=dev), torch.full((n, 70), -77, dtype=torch.int32, device=dev),
                               torch.full((n, 70), -7.5, device=dev), torch.full((n,), -77, dtype=torch.int32, device=dev),
                               torch.full((n,), -77, dtype=torch.int32, device=dev))
            got = pkg.farthest_points(*t, points=70, capacity=capacity, out=out)
            assert got is out
            h = host(out)
            assert not (h.points == -7.5).any() and not (h.radius2 == -7.5).any() and not (h.pixel == -77).any()
            assert not (h.count == -77).any() and not (h.status == -77).any()
            if capacity:
                assert fr.same(h, ref, 70) is None
    # radius2 is optional: without it the other four are what they were
    _, t, ref = exact
    kept = pkg.farthest_points(*t, points=70)
    bare = pkg.farthest_points(*t, points=70, out=kept._replace(radius2=None, points=torch.empty_like(kept.points),
                                                                  pixel=torch.empty_like(kept.pixel)))
    assert bare.radius2 is None and torch.equal(bare.pixel, kept.pixel) and torch.equal(bare.points, kept.points)


# ---- clouds ----
def test_farthest_of_lattices_and_duplicates_where_ties_decide(pkg, dev):
    clouds = fr.tie_clouds()
    want = fr.cloud_batch(clouds, 70)
    for c in (clouds, clouds.astype(np.float64)):
        for kw in (dict(), dict(capacity=64, form=1)):
            got = host(pkg.farthest_of(torch.from_numpy(c).to(dev), points=70, **kw))
            assert fr.same(got, want) is None, (c.dtype, kw, fr.same(got, want))
    assert want.pixel[2].tolist() == [0] * 70 and want.pixel[3].tolist() == [0, 1] + [0] * 68


def test_farthest_of_hard_values(pkg, dev):
    clouds = fr.hard_clouds()
    want = fr.cloud_batch(clouds, 16)
    assert want.count.tolist() == [37, 20, 0, 1] and want.status.tolist() == [0, 0, 1, 0]
    with np.errstate(over="ignore"):
        narrow = clouds.astype(np.float32)                               # 1e39 becomes an infinity: dropped either way
    for c in (clouds, narrow):
        for kw in (dict(), dict(capacity=40, form=1), dict(capacity=30, form=1)):
            ref = fr.cloud_batch(c, 16, **{k: v for k, v in kw.items()})
            got = host(pkg.farthest_of(torch.from_numpy(c).to(dev), points=16, **kw))
            assert fr.same(got, ref) is None, (c.dtype, kw, fr.same(got, ref))
            assert np.array_equal(ref.pixel, want.pixel)                   # (30 < 37: resident all the same)
    assert np.isposinf(want.radius2[0, :14]).all()


def test_farthest_of_point_clouds_output(pkg, crops):
    _, t, _ = crops
    pc = pkg.point_clouds(*t, points=6000, seed=3)
    assert pc.points.dtype is torch.float64 and not pc.status.any()
    want = fr.cloud_batch(pc.points.cpu().numpy(), 128)
    got = host(pkg.farthest_of(pc.points, points=128))
    assert fr.same(got, want) is None, fr.same(got, want)
    assert (want.count == 6000).all()
    wide = host(pkg.farthest_of(pc.points.float(), points=128, capacity=6000, form=1))
    assert fr.same(wide, want) is None
    # a draw with replacement repeats points: the sample never does
    assert all(len(np.unique(want.points[i], axis=0)) == 128 for i in range(16))


# ---- graphs ----
def test_graph_capture_and_three_replays(pkg, dev, crops):
    pack, t, ref = crops
    cap = int(ref.count.max())
    work = torch.empty((16, cap, 4), device=dev)
    out = pkg.farthest_points(*t, points=64, work=work)                  # eagerly once
    first = pkg.FpsBatch(*[x.clone() for x in out])
    assert fr.same(host(first), ref, 64) is None
    index = torch.arange(16, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        pkg.farthest_points(*t, points=64, work=work, out=out, index=index)
    for turn in range(3):
        for x in out:
            x.fill_(-5)
        index.copy_(torch.arange(16, device=dev).roll(turn))              # the replay reads the index anew
        g.replay()
        torch.cuda.synchronize(dev)
        assert all(torch.equal(x, f.roll(turn, 0)) for x, f in zip(out, first)), turn


# ---- the augmented step ----
@pytest.mark.parametrize("graph", [False, True])
def test_augmented_step_with_fps(pkg, dev, crops, graph):
    pack, t, _ = crops
    rng = np.random.default_rng(3)
    gt = torch.from_numpy(rng.uniform(-80, 80, (16, 21, 3)).astype(np.float32) + np.float32([0, 0, -420])).to(dev)
    n = 6
    plain = pkg.AugmentedStep(*t, n, gt=gt, graph=graph)
    with_fps = pkg.AugmentedStep(*t, n, gt=gt, graph=graph, fps=(64,), occupancy=(16,))
    assert plain.cloud is None and with_fps.cloud.shape == (n, 64, 3)
    for key, index in ((11, [1, 2, 3, 4, 5, 6]), (12, [15, 1, 1, 9, 0, 7])):
        a, a_nor, a_aug = plain.step(index, key)
        b, b_nor, b_aug = with_fps.step(index, key)
        torch.cuda.synchronize(dev)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(a_nor, b_nor) and torch.equal(a_aug, b_aug)
        assert torch.equal(plain.xforms, with_fps.xforms)
        want = pkg.farthest_points(*t, points=64, xforms=with_fps.xforms, index=with_fps.index)
        assert torch.equal(with_fps.cloud.view(torch.int32), want.points.view(torch.int32))
        assert torch.equal(with_fps.cloud_pixel, want.pixel) and torch.equal(with_fps.cloud_status, want.status)
        assert torch.equal(with_fps.cloud_count, want.count)
        ref = fr.batch(*pack, 64, xforms=with_fps.xforms.cpu().numpy(), index=index)
        assert fr.same(host(want), ref) is None
        assert (ref.status == 3).sum() == (1 if 0 in index else 0)        # frame 0 is above the resident cap
