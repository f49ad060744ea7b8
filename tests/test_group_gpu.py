"""GPU tier of the kNN grouping and the surface normals (include/tsdf_group.h): libtsdf_group.so against the numpy
restatement (tests/group_ref.py), BIT FOR BIT — ``index`` and ``status`` equal, ``dist2``, ``offsets``, ``normals`` and
``curvature`` equal as int32 bit patterns — at the smallest shapes at which the kernels can go wrong: wave tails, both
list sizes, fewer candidates than K, the plan's queries per workgroup, the cloud cap, ties, infinite distances, dropped
rows, explicit queries, the two HandPointNet levels on sampled clouds, caller's buffers, batches, a graph, and as the last
launches of the augmented step."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fps_ref as fr  # noqa: E402
import group_ref as gr  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def to(dev, a):
    return None if a is None else a if isinstance(a, (int, torch.Tensor)) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def host(b):
    return type(b)(*[None if t is None else t.cpu().numpy() for t in b])


def knn(pkg, dev, clouds, K, queries=None, status=None, **kw):
    """The library's answer and the restatement's to one call: (Knn of numpy arrays, Knn)."""
    st = None if status is None else np.asarray(status, np.int32)
    got = pkg.knn_groups(to(dev, clouds), K, queries=to(dev, queries), status=to(dev, st), offsets=True, **kw)
    return host(got), gr.knn(clouds, K, queries, st)


def normals(pkg, dev, clouds, K, queries=None, status=None, view=None, **kw):
    st = None if status is None else np.asarray(status, np.int32)
    got = pkg.point_normals(to(dev, clouds), K, queries=to(dev, queries), status=to(dev, st), view=to(dev, view), **kw)
    return host(got), gr.normals(clouds, K, queries, st, view)


def equal(a, b):
    """Two batches bit for bit, on the device."""
    return all((x is None and y is None) or torch.equal(x.view(torch.int32) if x.dtype is torch.float32 else x,
                                                        y.view(torch.int32) if y.dtype is torch.float32 else y)
               for x, y in zip(a, b))


# ---- kNN ----
@pytest.mark.parametrize("P", (1, 2, 63, 64, 65, 127, 129))
def test_wave_tails_and_both_list_sizes(pkg, dev, P):
    clouds = gr.random_clouds(2, P, seed=P)
    for K in (1, 3, 64, 65, 128):
        got, want = knn(pkg, dev, clouds, K)
        assert gr.same_knn(got, want) is None, (K, gr.same_knn(got, want))
        assert (got.index[:, :, 0] == np.arange(P)).all() and not got.dist2[:, :, 0].any()     # a query finds itself
        assert (np.diff(got.dist2[:, :, :min(K, P)], axis=2) >= 0).all() and not got.status.any()


def test_fewer_candidates_than_k_repeat_slot_0(pkg, dev):
    clouds = gr.ragged_cloud()
    got, want = knn(pkg, dev, clouds, 8)
    assert gr.same_knn(got, want) is None, gr.same_knn(got, want)
    assert got.index[0, 0].tolist()[3:] == [0] * 5 and sorted(got.index[0, 0, :3].tolist()) == [0, 2, 4]
    assert (got.index[0, [1, 3]] == -1).all() and not got.offsets[0, [1, 3]].any()              # the NaN rows as queries
    assert got.status.tolist() == [0]


def test_queries_around_a_workgroup_and_every_row_a_query(pkg, dev):
    per = pkg.group_plan(40, 40, 4)[1]
    assert per == gr.QUERIES_PER_GROUP
    clouds = gr.random_clouds(3, per + 8, seed=1)
    for C in (per - 1, per, per + 1, None):
        got, want = knn(pkg, dev, clouds, 4, queries=C)
        assert gr.same_knn(got, want) is None, (C, gr.same_knn(got, want))
    assert got.index.shape == (3, per + 8, 4)


def test_the_cap(pkg, dev):
    P = gr.MAX_CLOUD
    assert pkg.group_plan(P, 3, 128)[0] == gr.lds_bytes(P) == 147472
    clouds = gr.random_clouds(2, P, seed=2)
    clouds[1, 1::7] = np.nan                                  # dropped rows at the cap: ranks differ from compact indices
    clouds[1, P - 1] = clouds[1, 0]                           # the last lane slot of the last step ties with row 0
    for K in (5, 128):
        got, want = knn(pkg, dev, clouds, K, queries=3)
        assert gr.same_knn(got, want) is None, (K, gr.same_knn(got, want))
    assert got.index[1, 0, :2].tolist() == [0, P - 1] and (got.index[1, 1] == -1).all() and got.index.max() > 12000


def test_ties_go_to_the_lowest_rank(pkg, dev):
    clouds = gr.tie_clouds()
    got, want = knn(pkg, dev, clouds, 9)
    assert gr.same_knn(got, want) is None, gr.same_knn(got, want)
    assert got.index[0, 32, :2].tolist() == [0, 32] and got.index[0, 0, :2].tolist() == [0, 32]   # duplicates: the lower row first
    assert gr.same_knn(got, gr.knn(clouds, 9, mistake="ties_high")) == "index"


def test_infinite_distances_order_by_rank_alone(pkg, dev):
    clouds = gr.huge_cloud(70)
    got, want = knn(pkg, dev, clouds, 10)
    assert gr.same_knn(got, want) is None, gr.same_knn(got, want)
    assert np.isposinf(got.dist2[0, :, 1:]).all() and (got.index[0, 20] == [20] + list(range(9))).all()


def test_dropped_rows_nan_queries_no_candidate_and_status_pass_through(pkg, dev):
    clouds = gr.hard_clouds()
    got, want = knn(pkg, dev, clouds, 6)
    assert gr.same_knn(got, want) is None, gr.same_knn(got, want)
    assert got.status.tolist() == [0, 0, 1, 0] and (got.index[2] == -1).all() and (got.index[3, 23] == 23).all()
    assert (got.index[0, [5, 9, 17]] == -1).all() and not np.isin(got.index[0], [5, 9, 17]).any()
    status = [0, 7, 0, 2]
    got, want = knn(pkg, dev, clouds, 6, status=status)
    assert gr.same_knn(got, want) is None, gr.same_knn(got, want)
    assert got.status.tolist() == [0, 7, 1, 2] and (got.index[[1, 3]] == -1).all() and not got.dist2[[1, 3]].any()


def test_explicit_queries_not_in_the_cloud(pkg, dev):
    clouds = gr.random_clouds(3, 100, seed=4)
    queries = gr.random_clouds(3, 37, seed=5, scale=150.0)
    queries[1, 4, 0] = np.inf
    got, want = knn(pkg, dev, clouds, 7, queries=queries)
    assert gr.same_knn(got, want) is None, gr.same_knn(got, want)
    assert (got.dist2[:, :, 0] > 0).sum() == 3 * 37 - 1 and (got.index[1, 4] == -1).all() and not got.status.any()


@pytest.fixture(scope="module")
def sampled(pkg, dev):
    """fps_ref.crops(4) sampled at M = 256 by the library (which tests/test_fps_gpu.py pins to its restatement)."""
    pack = fr.crops(4)
    fps = pkg.farthest_points(*[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in pack], points=256, capacity=200000)
    assert not fps.status.any()
    return fps


def test_the_two_handpointnet_levels_on_sampled_clouds(pkg, dev, sampled):
    cloud = sampled.points.cpu().numpy()
    g1 = pkg.knn_groups(sampled.points, 32, queries=128, status=sampled.status, offsets=True)
    assert gr.same_knn(host(g1), gr.knn(cloud, 32, 128)) is None
    prefix = sampled.points[:, :128]                          # read in place: the next level's cloud is a prefix
    assert not prefix.is_contiguous()
    g2 = pkg.knn_groups(prefix, 32, queries=32, offsets=True)
    assert gr.same_knn(host(g2), gr.knn(cloud[:, :128], 32, 32)) is None
    assert equal(g2, pkg.knn_groups(prefix.contiguous(), 32, queries=32, offsets=True))
    again = pkg.farthest_of(sampled.points, points=128)       # the centres ARE the first rows
    assert torch.equal(again.points, prefix)
    # the sampler's status chains: a position it gave a status is not read
    status = torch.tensor([0, 3, 0, 0], dtype=torch.int32, device=dev)
    g3 = pkg.knn_groups(sampled.points, 32, queries=128, status=status, offsets=True)
    assert gr.same_knn(host(g3), gr.knn(cloud, 32, 128, status_in=[0, 3, 0, 0])) is None and g3.status.tolist() == [0, 3, 0, 0]


def test_offsets_are_the_differences_recomputed(pkg, dev, sampled):
    g = pkg.knn_groups(sampled.points, 16, queries=64, offsets=True)
    picked = torch.gather(sampled.points[:, None].expand(-1, 64, -1, -1), 2, g.index.long()[..., None].expand(-1, -1, -1, 3))
    assert torch.equal(g.offsets, picked - sampled.points[:, :64, None])
    assert torch.equal(g.dist2, (g.offsets[..., 0] * g.offsets[..., 0] + g.offsets[..., 1] * g.offsets[..., 1])
                       + g.offsets[..., 2] * g.offsets[..., 2])


def test_out_buffers_are_overwritten_whole_and_optional_outputs_stay_away(pkg, dev):
    clouds = gr.hard_clouds()
    t = to(dev, clouds)
    want = pkg.knn_groups(t, 6, offsets=True, status=to(dev, np.array([0, 7, 0, 0], np.int32)))
    out = pkg.KnnBatch(torch.full((4, 40, 6), 0x5a5a5a5a, dtype=torch.int32, device=dev),
                       torch.full((4, 40, 6), float("nan"), device=dev), torch.full((4, 40, 6, 3), float("nan"), device=dev),
                       torch.full((4,), 0x5a5a5a5a, dtype=torch.int32, device=dev))
    got = pkg.knn_groups(t, 6, status=to(dev, np.array([0, 7, 0, 0], np.int32)), out=out)
    assert got is out and equal(out, want) and not torch.isnan(out.dist2).any() and not torch.isnan(out.offsets).any()
    bare = pkg.knn_groups(t, 6, dist2=False)
    assert bare.dist2 is None and bare.offsets is None
    nout = pkg.NormalBatch(torch.full((4, 40, 3), float("nan"), device=dev), torch.full((4, 40), float("nan"), device=dev),
                           torch.full((4,), 0x5a5a5a5a, dtype=torch.int32, device=dev))
    assert pkg.point_normals(t, 6, out=nout) is nout and equal(nout, pkg.point_normals(t, 6))
    assert not torch.isnan(nout.normals).any() and not torch.isnan(nout.curvature).any()
    assert pkg.point_normals(t, 6, curvature=False).curvature is None


def test_a_position_alone_in_a_batch_and_in_a_second_call(pkg, dev):
    clouds = to(dev, gr.random_clouds(5, 150, seed=6))
    whole = pkg.knn_groups(clouds, 20, queries=70, offsets=True)
    wn = pkg.point_normals(clouds, 20, queries=70)
    assert equal(whole, pkg.knn_groups(clouds, 20, queries=70, offsets=True)) and equal(wn, pkg.point_normals(clouds, 20, queries=70))
    for i in (0, 3):
        assert equal([t[i:i + 1] for t in whole], pkg.knn_groups(clouds[i:i + 1], 20, queries=70, offsets=True))
        assert equal([t[i:i + 1] for t in wn], pkg.point_normals(clouds[i:i + 1], 20, queries=70))


def test_a_graph_replay_equals_the_eager_call(pkg, dev):
    clouds = to(dev, gr.patches())
    eager, neager = pkg.knn_groups(clouds, 70, queries=50, offsets=True), pkg.point_normals(clouds, 12)
    out = pkg.KnnBatch(*[torch.zeros_like(t) for t in eager])
    nout = pkg.NormalBatch(*[torch.zeros_like(t) for t in neager])
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
        pkg.knn_groups(clouds, 70, queries=50, out=out)
        pkg.point_normals(clouds, 12, out=nout)
    for t in (*out, *nout):
        t.zero_()
    g.replay()
    torch.cuda.synchronize(dev)
    assert equal(out, eager) and equal(nout, neager)


# ---- normals ----
def test_normals_of_smooth_patches_with_and_without_a_viewpoint(pkg, dev):
    clouds = gr.patches()
    got, want = normals(pkg, dev, clouds, 30)
    assert gr.same_normals(got, want) is None, gr.same_normals(got, want)
    assert (got.normals[..., 2] > 0.7).all()                                  # towards the camera at the origin: +z
    assert np.abs(np.linalg.norm(got.normals.astype(np.float64), axis=2) - 1).max() < 1e-6
    assert got.curvature[0].max() < 1e-4 and got.curvature.min() >= 0         # the plane is flat
    view = np.array([[0.0, 0.0, -1000.0], [500.0, 0.0, -400.0], [0.0, 0.0, 0.0], [1e6, -1e6, -1e9]])
    got, want = normals(pkg, dev, clouds, 30, view=view)
    assert gr.same_normals(got, want) is None, gr.same_normals(got, want)
    assert (got.normals[0, :, 2] < -0.7).all() and (got.normals[2, :, 2] > 0.7).all()             # seen from behind: flipped
    assert gr.same_normals(got, gr.normals(clouds, 30, view=view, mistake="no_flip")) == "normals"
    # xforms=: the viewpoint is the translation column of each map's forward rows
    xf = np.random.default_rng(8).normal(0, 1, (4, 24))
    xf[:, [3, 7, 11]] = view
    by_maps = pkg.point_normals(to(dev, clouds), 30, xforms=to(dev, xf))
    assert gr.same_normals(host(by_maps), want) is None


@pytest.mark.parametrize("K", (3, 64, 65, 128))
def test_normals_at_both_list_sizes_and_wave_tails(pkg, dev, K):
    for P in (2, 65, 129, 200):
        clouds = gr.patches(2, P, seed=P)
        got, want = normals(pkg, dev, clouds, K, queries=min(5, P))
        assert gr.same_normals(got, want) is None, (P, K, gr.same_normals(got, want))
        assert (P >= 3) == bool(got.normals.any())                            # m' < 3: a zero normal and zero curvature


def test_normals_of_the_hard_clouds_and_the_sampled_clouds(pkg, dev, sampled):
    for clouds, K in ((gr.cubic_clouds(), 7), (gr.hard_clouds(), 6), (gr.tie_clouds(), 9), (gr.ragged_cloud(), 8)):
        if K == 7:   # isotropic neighbourhoods: the order of the tree sum decides the direction
            assert gr.same_normals(gr.normals(clouds, K, mistake="sequential_sum"), gr.normals(clouds, K)) == "normals"
        got, want = normals(pkg, dev, clouds, K, status=[0, 5, 0, 0][:len(clouds)])
        assert gr.same_normals(got, want) is None, (K, gr.same_normals(got, want))
        assert np.isfinite(got.normals).all() and np.isfinite(got.curvature).all()
    assert got.status.tolist() == [0] and not got.normals[0, [1, 3]].any()
    cloud = sampled.points.cpu().numpy()
    got = host(pkg.point_normals(sampled.points, 10, status=sampled.status))
    want = gr.normals(cloud, 10)
    assert gr.same_normals(got, want) is None, gr.same_normals(got, want)


# ---- the augmented step ----
def test_augmented_step_groups_and_normals_equal_the_explicit_chain(pkg, dev):
    pack = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in fr.crops(4)]
    step = pkg.AugmentedStep(*pack, 4, res=8, fps=(128,), groups=((64, 16), (16, 16)), normals=10)
    assert step.graph is not None
    step.step([2, 0, 3, 1], key=11, counter0=5)
    torch.cuda.synchronize(dev)
    fps = pkg.farthest_points(*pack, 128, xforms=step.xforms, index=step.index)
    assert torch.equal(fps.points, step.cloud) and torch.equal(fps.status, step.cloud_status) and fps.status.tolist().count(0) >= 3
    nrm = pkg.point_normals(fps.points, 10, xforms=step.xforms, status=fps.status)
    g1 = pkg.knn_groups(fps.points, 16, queries=64, status=fps.status, offsets=True)
    g2 = pkg.knn_groups(fps.points[:, :64], 16, queries=16, status=fps.status, offsets=True)
    assert equal(step.normals, nrm) and equal(step.groups[0], g1) and equal(step.groups[1], g2)
    assert gr.same_knn(host(step.groups[1]), gr.knn(step.cloud.cpu().numpy()[:, :64], 16, 16,
                                                          status_in=step.cloud_status.cpu().numpy())) is None
    plain = pkg.AugmentedStep(*pack, 4, res=8, fps=(128,))
    plain.step([2, 0, 3, 1], key=11, counter0=5)
    assert torch.equal(plain.cloud, step.cloud) and torch.equal(plain.out.tsdf, step.out.tsdf) and plain.groups is None
