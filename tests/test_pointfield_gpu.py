"""GPU tier of the point-wise offset fields (include/tsdf_pointfield.h): libtsdf_pointfield.so against the numpy
restatement (tests/pointfield_ref.py), BIT FOR BIT — ``valid`` and ``status`` equal, the field, the joints and the weights
equal as int32 / int16 bit patterns — at the smallest shapes at which the kernels can go wrong: wave tails, K below, at
and above the candidates, the plan's joints per workgroup, both layouts, the three element types, the cloud cap (the
kernels' other form), ties, a point on the joint and one at exactly the radius, infinite distances, dropped rows, NaN
joints, no candidate, a status passed through, NaN / negative / large / tied heats, zero vectors, sampled clouds,
caller's buffers, batches, a graph, and as the last launch of the augmented step."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fps_ref as fr  # noqa: E402
import pointfield_ref as pr  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def to(dev, a):
    return None if a is None else a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def raw(t):
    """A tensor's values as a numpy array; bfloat16 as its uint16 patterns."""
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype is torch.bfloat16 else t.cpu().numpy()


def host(b):
    return type(b)(*[raw(t) for t in b])


def field_to(dev, field, layout="cp", dtype="float32"):
    """A restated float32 "cp" field as the tensor the library reads in ``layout`` and ``dtype``."""
    a = pr.to_layout(pr.narrow(field, dtype), layout)
    t = torch.from_numpy(a.view(np.int16) if dtype == "bfloat16" else a).to(dev)
    return t.view(torch.bfloat16) if dtype == "bfloat16" else t


def encode(pkg, dev, clouds, joints, K, radius, layout="cp", dtype="float32", status=None):
    """None if the library's field is the restatement's bit for bit, else what differs; and both."""
    st = None if status is None else np.asarray(status, np.int32)
    got = host(pkg.point_fields(to(dev, clouds), to(dev, joints), K, radius=radius, layout=layout, dtype=DTYPES[dtype],
                                status=to(dev, st)))
    want = pr.encode(clouds, joints, K, radius, st)
    return pr.same_field(got, want, dtype, layout), got, want


def decode(pkg, dev, clouds, field, M, radius, layout="cp", dtype="float32", status=None):
    """``field`` is float32 "cp"; the restatement decodes what the library reads: the narrowed field widened again."""
    st = None if status is None else np.asarray(status, np.int32)
    got = host(pkg.field_joints(to(dev, clouds), field_to(dev, field, layout, dtype), radius=radius, points=M, layout=layout,
                                status=to(dev, st)))
    want = pr.decode(clouds, pr.widen(pr.narrow(field, dtype), dtype), M, radius, st)
    return pr.same_joints(got, want), got, want


def equal(a, b):
    """Two batches bit for bit, on the device."""
    return all(torch.equal(x.view(torch.int32) if x.dtype is torch.float32 else x.view(torch.int16) if x.element_size() == 2 else x,
                           y.view(torch.int32) if y.dtype is torch.float32 else y.view(torch.int16) if y.element_size() == 2 else y)
               for x, y in zip(a, b))


# ---- encode ----
@pytest.mark.parametrize("layout", ("cp", "pc"))
@pytest.mark.parametrize("P", (1, 2, 63, 64, 65, 127, 129))
def test_wave_tails_every_k_and_the_joints_of_a_workgroup(pkg, dev, P, layout):
    per = pkg.pointfield_plan(P, 21, 64)[1]
    assert per == pr.JOINTS_PER_GROUP
    clouds = pr.random_clouds(2, P, seed=P, scale=20.0)
    for J in (1, per - 1, per + 1, 21):
        joints = pr.joints_near(clouds, J, seed=P + J, spread=8.0)
        for K in (1, 3, 64, 65, P, P + 1):
            bad, got, want = encode(pkg, dev, clouds, joints, K, 25.0, layout)
            assert bad is None, (J, K, bad)
            assert got.valid.all() and not got.status.any()
        heat = (got.field[:, :J] if layout == "cp" else got.field[:, :, :J])
        assert heat.max() == 1.0 and (heat >= 0).all()       # the first joint lies on a row


@pytest.mark.parametrize("layout", ("cp", "pc"))
@pytest.mark.parametrize("dtype", ("float32", "float16", "bfloat16"))
def test_the_three_element_types_both_ways(pkg, dev, dtype, layout):
    clouds, joints, K, radius, M = pr.groups()["dense"]
    bad, got, want = encode(pkg, dev, clouds, joints, K, radius, layout, dtype)
    assert bad is None, bad
    assert got.field.dtype == {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}[dtype]
    for field in (want.field, pr.prediction("dense", want.field)):
        bad, got, _ = decode(pkg, dev, clouds, field, M, radius, layout, dtype)
        assert bad is None, bad


def test_the_cap_with_dropped_rows(pkg, dev):
    P = pr.MAX_CLOUD
    assert pkg.pointfield_plan(P, 3, 64)[0] == pr.lds_bytes(P) == 147472
    clouds = pr.random_clouds(1, P, seed=2, scale=30.0)
    clouds[0, 1::7] = np.nan                                  # dropped rows at the cap
    clouds[0, P - 1] = clouds[0, 0]                           # the last lane slot of the last step ties with row 0
    joints = np.stack([np.stack([clouds[0, 0], clouds[0, 5000] + np.float32(0.5), clouds[0, 12000]])])
    for K in (2, 64, P):
        bad, got, want = encode(pkg, dev, clouds, joints, K, 9.0)
        assert bad is None, (K, bad)
    assert got.field[0, 0, 0] == 1.0 and got.field[0, 0, P - 1] == 1.0 and not got.field[0, :, 1::7].any()
    bad, got, want = encode(pkg, dev, clouds, joints, 1, 9.0, "pc")
    assert bad is None and got.field[0, 0, 0] == 1.0 and got.field[0, P - 1, 0] == 0.0   # K = 1: the tie goes to row 0
    field = pr.prediction("cap", pr.encode(clouds, joints, 64, 9.0).field)
    for M in (1, 25, 128):
        bad, got, _ = decode(pkg, dev, clouds, field, M, 9.0)
        assert bad is None, (M, bad)


@pytest.mark.parametrize("name", sorted(pr.groups()))
def test_the_input_groups_both_ways(pkg, dev, name):
    """Tie lattices, a dense and a sparse cloud, a joint on a point, a point at exactly d == radius, 1e30 coordinates, NaN
    rows, NaN joints, m == 0, m == 1, and sums that cancel: the groups the CPU tier shows every mistake on."""
    clouds, joints, K, radius, M = pr.groups()[name]
    bad, got, want = encode(pkg, dev, clouds, joints, K, radius)
    assert bad is None, bad
    for m in pr.ENCODE_MISTAKES:                              # what the CPU tier sees, the GPU does not do
        wrong = pr.encode(clouds, joints, K, radius, mistake=m)
        assert np.array_equal(pr.bits(wrong.field), pr.bits(want.field)) or pr.same_field(got, wrong) == "field", m
    for field in (want.field, pr.prediction(name, want.field)):
        for votes in sorted({1, M, 25, 64, 65, 128, clouds.shape[1] + 1} & set(range(1, 129)) | {M}):
            bad, back, ref = decode(pkg, dev, clouds, field, votes, radius)
            assert bad is None, (votes, bad)
    if name == "edges":
        J = joints.shape[1]
        assert got.status.tolist() == [0, 0, 0, 1, 0] and got.valid.tolist() == [[1] * 3, [1] * 3, [1, 0, 0], [0] * 3, [1] * 3]
        assert got.field[0, 0, 1] == 1.0 and not got.field[0, J:J + 3, 1].any()                   # on the joint
        assert pr.bits(got.field[0, 0, :1])[0] == 0 and got.field[0, J:J + 3, 0].tolist() == [-1.0, 0.0, 0.0]   # d == radius
        assert not got.field[3].any() and not got.field[2, 1:3].any() and not got.field[2, :, [0, 3, 6]].any()


def test_status_passes_through_and_the_position_is_not_read(pkg, dev):
    clouds, joints, K, radius, M = pr.groups()["edges"]
    status = [0, 7, 0, 2, 0]
    bad, got, want = encode(pkg, dev, clouds, joints, K, radius, status=status)
    assert bad is None and got.status.tolist() == [0, 7, 0, 2, 0] and not got.field[[1, 3]].any() and not got.valid[[1, 3]].any()
    bad, back, _ = decode(pkg, dev, clouds, pr.prediction("edges", want.field), M, radius, status=status)
    assert bad is None and back.status.tolist() == [0, 7, 0, 2, 0] and not back.joints[[1, 3]].any() and not back.weight[[1, 3]].any()


def test_the_members_are_knn_groups_neighbours_inside_the_ball(pkg, dev):
    clouds, joints, K, radius, _ = pr.groups()["dense"]
    c, j = to(dev, clouds), to(dev, joints)
    f = pkg.point_fields(c, j, K, radius=radius)
    g = pkg.knn_groups(c, K, queries=j)
    J, P = joints.shape[1], clouds.shape[1]
    inside = torch.sqrt(g.dist2.double()) <= radius
    want = torch.zeros((len(clouds), J, P), dtype=torch.bool, device=dev)
    want.scatter_(2, g.index.long(), inside)
    vec = f.field[:, J:].reshape(len(clouds), J, 3, P)
    got = (f.field[:, :J] != 0) | (vec != 0).any(2)           # a member at d == radius has heat 0 but a unit vector
    assert torch.equal(got, want) and int(want.sum()) > 2 * J
    heat = 1.0 - torch.sqrt(g.dist2.double()) / radius        # and the heat is that of the very dist2 knn_groups measured
    assert torch.equal(torch.gather(f.field[:, :J], 2, g.index.long())[inside], heat.float()[inside])


# ---- on sampled clouds ----
@pytest.fixture(scope="module")
def sampled(pkg, dev):
    """fps_ref.crops(4) sampled at M = 1024 under their principal-axis maps by the library (tests/test_fps_gpu.py pins it)."""
    pack = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in fr.crops(4)]
    obb = pkg.obb_xforms(*pack)
    fps = pkg.farthest_points(*pack, points=1024, capacity=200000, xforms=obb.xforms)
    assert not fps.status.any()
    return fps


def test_sampled_clouds_encode_then_decode(pkg, dev, sampled):
    cloud = sampled.points.cpu().numpy()
    joints = pr.joints_near(cloud, 21, seed=3, spread=6.0)
    radius = 30.0
    f = pkg.point_fields(sampled.points, to(dev, joints), 64, radius=radius, status=sampled.status)
    want = pr.encode(cloud, joints, 64, radius)
    assert pr.same_field(host(f), want) is None
    back = pkg.field_joints(sampled.points, f.field, radius=radius, status=sampled.status)
    assert pr.same_joints(host(back), pr.decode(cloud, want.field, 25, radius)) is None
    err = (back.joints - to(dev, joints)).abs().max().item()
    print(f"round trip on sampled clouds: max |decode(encode(j)) - j| = {err:.3g} mm, min weight {back.weight.min().item():.3g}")
    assert back.weight.min().item() > 0 and err <= radius * 2.0 ** -20 + 2.0 ** -23 * np.abs(joints).max()
    # the sampler's status chains: a position it gave a status is not read
    status = torch.tensor([0, 3, 0, 0], dtype=torch.int32, device=dev)
    f3 = pkg.point_fields(sampled.points, to(dev, joints), 64, radius=radius, status=status)
    assert f3.status.tolist() == [0, 3, 0, 0] and not f3.field[1].any() and torch.equal(f3.field[0], f.field[0])
    prefix = sampled.points[:, :256]                          # read in place, as knn_groups reads a prefix
    assert not prefix.is_contiguous()
    assert equal(pkg.point_fields(prefix, to(dev, joints), 16, radius=radius),
                 pkg.point_fields(prefix.contiguous(), to(dev, joints), 16, radius=radius))


def test_out_buffers_are_overwritten_whole(pkg, dev):
    clouds, joints, K, radius, M = pr.groups()["edges"]
    c, j, st = to(dev, clouds), to(dev, joints), to(dev, np.array([0, 7, 0, 0, 0], np.int32))
    for layout in ("cp", "pc"):
        want = pkg.point_fields(c, j, K, radius=radius, layout=layout, status=st)
        out = pkg.PointFieldBatch(torch.full_like(want.field, float("nan")), torch.full_like(want.valid, 0x5a5a5a5a),
                                  torch.full_like(want.status, 0x5a5a5a5a))
        assert pkg.point_fields(c, j, K, radius=radius, layout=layout, status=st, out=out) is out and equal(out, want)
        assert not torch.isnan(out.field).any()
        back = pkg.field_joints(c, want.field, radius=radius, points=M, layout=layout, status=st)
        jout = pkg.FieldJoints(torch.full_like(back.joints, float("nan")), torch.full_like(back.weight, float("nan")),
                               torch.full_like(back.status, 0x5a5a5a5a))
        assert pkg.field_joints(c, want.field, radius=radius, points=M, layout=layout, status=st, out=jout) is jout
        assert equal(jout, back) and not torch.isnan(jout.joints).any() and not torch.isnan(jout.weight).any()
    flat = pkg.point_fields(c, j.reshape(len(clouds), -1), K, radius=radius, status=st)   # joints as [n, 3J]
    assert equal(flat, pkg.point_fields(c, j, K, radius=radius, status=st))


def test_a_position_alone_in_a_batch_and_in_a_second_call(pkg, dev):
    clouds = pr.random_clouds(5, 150, seed=6, scale=20.0)
    c, j = to(dev, clouds), to(dev, pr.joints_near(clouds, 6, seed=7))
    whole = pkg.point_fields(c, j, 20, radius=25.0)
    pred = to(dev, pr.perturbed(whole.field.cpu().numpy(), seed=8))
    back = pkg.field_joints(c, pred, radius=25.0, points=30)
    assert equal(whole, pkg.point_fields(c, j, 20, radius=25.0)) and equal(back, pkg.field_joints(c, pred, radius=25.0, points=30))
    for i in (0, 3):
        assert equal([t[i:i + 1] for t in whole], pkg.point_fields(c[i:i + 1], j[i:i + 1], 20, radius=25.0))
        assert equal([t[i:i + 1] for t in back], pkg.field_joints(c[i:i + 1], pred[i:i + 1], radius=25.0, points=30))


def test_a_graph_replay_equals_the_eager_call(pkg, dev):
    clouds, joints, K, radius, M = pr.groups()["sparse"]
    c, j = to(dev, clouds), to(dev, joints)
    eager = pkg.point_fields(c, j, K, radius=radius)
    back = pkg.field_joints(c, eager.field, radius=radius, points=M)
    out = pkg.PointFieldBatch(*[torch.zeros_like(t) for t in eager])
    jout = pkg.FieldJoints(*[torch.zeros_like(t) for t in back])
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
        pkg.point_fields(c, j, K, radius=radius, out=out)
        pkg.field_joints(c, out.field, radius=radius, points=M, out=jout)
    for t in (*out, *jout):
        t.zero_()
    g.replay()
    torch.cuda.synchronize(dev)
    assert equal(out, eager) and equal(jout, back)


# ---- the augmented step ----
def test_augmented_step_fields_equal_the_explicit_chain(pkg, dev):
    pack = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in fr.crops(4)]
    gt = pkg.point_clouds(*pack, points=5, seed=1).points.float().reshape(4, 15).contiguous()   # five surface points a frame
    radius = 40.0
    step = pkg.AugmentedStep(*pack, 4, gt=gt, res=8, fps=(128,), fields=(16, radius))
    assert step.graph is not None and step.field.shape == (4, 20, 128) and step.field_valid.shape == (4, 5)
    out, gt_nor, gt_aug = step.step([2, 0, 3, 1], key=11, counter0=5)
    torch.cuda.synchronize(dev)
    fps = pkg.farthest_points(*pack, 128, xforms=step.xforms, index=step.index)
    assert torch.equal(fps.points, step.cloud) and torch.equal(fps.status, step.cloud_status) and fps.status.tolist().count(0) >= 3
    f = pkg.point_fields(fps.points, gt_aug, 16, radius=radius, status=fps.status)
    assert equal((step.field, step.field_valid), (f.field, f.valid)) and int((step.field[:, :5] > 0).sum()) > 20
    assert pr.same_field(host(f), pr.encode(step.cloud.cpu().numpy(), gt_aug.cpu().numpy().reshape(4, 5, 3), 16, radius,
                                            step.cloud_status.cpu().numpy())) is None
    plain = pkg.AugmentedStep(*pack, 4, gt=gt, res=8, fps=(128,))
    pout, pnor, paug = plain.step([2, 0, 3, 1], key=11, counter0=5)
    assert plain.field is None and torch.equal(plain.cloud, step.cloud) and torch.equal(pout.tsdf, out.tsdf)
    assert torch.equal(pnor.view(torch.int32), gt_nor.view(torch.int32)) and torch.equal(paug.view(torch.int32), gt_aug.view(torch.int32))
    assert all(torch.equal(a, b) for a, b in zip(pout[1:], out[1:])) and torch.equal(plain.xforms, step.xforms)
    half = pkg.AugmentedStep(*pack, 4, gt=gt, res=8, fps=(128,), fields=(16, radius, torch.bfloat16), graph=False)
    half.step([2, 0, 3, 1], key=11, counter0=5)
    assert torch.equal(half.field.view(torch.int16), step.field.bfloat16().view(torch.int16))
