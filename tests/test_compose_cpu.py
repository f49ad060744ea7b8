"""CPU tier of the composed entries of ``voxelize`` and of the default hooks of ``export``: which primitives each one
launches, in which order, with which arguments, and what it returns from whose outputs; then the pass table
(``_grid_pass``) cell by cell and the status combiner.  Every primitive is replaced by a recorder that returns CPU tensors
of the right shapes (n = 3, R = 8), so nothing here touches a GPU or a library; the GPU tiers pin the same entries bit for
bit to their explicit chains."""
import importlib
import inspect

import pytest

torch = pytest.importorskip("torch")

PKG = "handposeestimation-with-3d-cnns_amd"
N, R, P = 3, 8, 5
BF16 = torch.bfloat16
PRIMITIVES = ("aabb", "map_grids", "cloud_grids", "point_clouds", "locate_hands", "voxelize", "voxelize_labels",
              "voxelize_grid", "voxelize_grid_lowp", "voxelize_aug_grid", "voxelize_map_grid_lowp", "_map_grid_lowp",
              "voxelize_grid_accurate", "narrow_volumes", "aug_xforms", "transform_joints", "normalize_joints")


def _st(*v):
    return torch.tensor(v, dtype=torch.int32)


def _f(*shape):
    return torch.rand(shape, dtype=torch.float32)


def _vol(dtype=torch.float32):
    return torch.rand((N, 3, R, R, R), dtype=torch.float32).to(dtype)


class Rec:
    """The recorders: ``log`` holds (name, arguments by parameter name, what was returned) of every primitive call."""

    def __init__(self, V, monkeypatch):
        self.V, self.log = V, []
        for name in PRIMITIVES:
            monkeypatch.setattr(V, name, self._stub(name, getattr(V, name)))

    def _stub(self, name, real):
        sig = inspect.signature(real)

        def fn(*a, **kw):
            b = sig.bind(*a, **kw)
            b.apply_defaults()
            ret = getattr(self, "_" + name.lstrip("_"))(b.arguments)
            self.log.append((name, dict(b.arguments), ret))
            return ret
        fn.__name__ = name
        return fn

    def names(self):
        return [e[0] for e in self.log]

    # ---- placements: every stage has a status of its own, so that the rule a caller applies shows ----
    def _aabb(self, a):
        return self.V.AabbBatch(_f(N, 6), _f(N, 8), _f(N, 3), _st(0, 11, 0))

    def _map_grids(self, a):
        return self.V.MapGridBatch(_f(N, 8), _f(N), _f(N, 3), _st(0, 12, 0))

    def _cloud_grids(self, a):
        return self.V.CloudGridBatch(_f(N, 8), _f(N), _f(N, 3), _f(N, 6), _st(0, 21, 22))

    def _point_clouds(self, a):
        return self.V.PointCloudBatch(torch.rand((N, P, 3), dtype=torch.float64), _st(4, 5, 6), _st(0, 31, 0))

    def _locate_hands(self, a):
        g = (_f(N, 8), _f(N), _f(N, 3)) if a["grid"] else (None, None, None)
        return self.V.HandCrops(_f(40), torch.tensor([0, 10, 20, 30]), torch.zeros((N, 6), dtype=torch.int32),
                                torch.rand((N, 3), dtype=torch.float64), _st(10, 10, 10), _st(0, 0, 41), *g)

    # ---- voxel passes ----
    def _voxelize(self, a):
        return self.V.TsdfBatch(_vol(), _f(N), _f(N, 3), _st(0, 51, 0))

    def _voxelize_labels(self, a):
        return self._voxelize(a), torch.rand_like(a["gt"])

    def _voxelize_grid(self, a):
        return _vol(), _st(61, 62, 63)

    _voxelize_aug_grid = _voxelize_grid_accurate = _voxelize_grid

    def _voxelize_grid_lowp(self, a):
        return _vol(a["dtype"]), _st(61, 62, 63)

    _voxelize_map_grid_lowp = _voxelize_grid_lowp

    def _map_grid_lowp(self, a):
        return _vol(a["dtype"]), (_st(61, 62, 63) if a["want_status"] else None)

    def _narrow_volumes(self, a):
        return a["tsdf32"].to(a["dtype"])

    # ---- maps and labels ----
    def _aug_xforms(self, a):
        return torch.rand((N, 24), dtype=torch.float64)

    def _transform_joints(self, a):
        return torch.rand_like(a["gt"])

    def _normalize_joints(self, a):
        return torch.rand_like(a["gt"])


@pytest.fixture()
def V():
    return importlib.import_module(PKG + ".voxelize")


@pytest.fixture()
def rec(V, monkeypatch):
    return Rec(V, monkeypatch)


@pytest.fixture()
def pack():
    return _f(30), torch.tensor([0, 10, 20, 30]), torch.zeros((N, 6), dtype=torch.int32)


@pytest.fixture()
def cam(pkg):
    return pkg._lib.TsdfCam()          # (never read here: it travels by identity)


def _first(*stages):
    """"The first non-zero status of the stages", written out."""
    out = stages[-1]
    for s in reversed(stages[:-1]):
        out = torch.where(s != 0, s, out)
    return out


def _same_pack(args, pack):
    return all(args[k] is t for k, t in zip(("depth", "offsets", "headers"), pack))


def _aabb_rows(ab):
    return torch.cat([ab.ori, ab.grid[:, 4:6], torch.zeros_like(ab.ori)], dim=1)


def _is_aabb_placement(batch, ab):
    return torch.equal(batch.max_l, ab.grid[:, 3]) and batch.max_l.is_contiguous() and \
        torch.equal(batch.mid_p, ab.grid[:, :3]) and batch.mid_p.is_contiguous() and batch.status is ab.status


# ---- the AABB placement followed by one pass ----
def test_voxelize_lowp(V, rec, pack, cam):
    out = V.voxelize_lowp(*pack, res=R, layout="cxyz", dtype=BF16, cam=cam)
    assert rec.names() == ["aabb", "voxelize_grid_lowp"]
    (_, pa, ab), (_, va, (tsdf, _)) = rec.log
    assert _same_pack(pa, pack) and pa["res"] == R and pa["cam"] is cam
    assert _same_pack(va, pack) and (va["res"], va["layout"], va["dtype"]) == (R, "cxyz", BF16) and va["cam"] is cam
    assert va["index"] is None and va["out"] is None
    assert torch.equal(va["grid"], _aabb_rows(ab)) and va["grid"].is_contiguous()
    assert isinstance(out, V.TsdfBatch) and out.tsdf is tsdf and _is_aabb_placement(out, ab)
    with pytest.raises(ValueError, match="float16 or torch.bfloat16"):
        V.voxelize_lowp(*pack, dtype=torch.float32)
    assert len(rec.log) == 2                                           # refused before the first launch


def test_voxelize_accurate(V, rec, pack, cam):
    out = V.voxelize_accurate(*pack, res=R, layout="cxyz", cam=cam)
    assert rec.names() == ["aabb", "voxelize_grid_accurate"]
    (_, pa, ab), (_, va, (tsdf, _)) = rec.log
    assert _same_pack(pa, pack) and pa["res"] == R and pa["cam"] is cam
    assert _same_pack(va, pack) and (va["res"], va["layout"]) == (R, "cxyz") and va["cam"] is cam
    assert va["index"] is None and va["out"] is None and va["nearest"] is False
    assert torch.equal(va["grid"], _aabb_rows(ab))
    assert isinstance(out, V.TsdfBatch) and out.tsdf is tsdf and _is_aabb_placement(out, ab)


# ---- the placement under a map followed by the status-less low-precision pass ----
@pytest.mark.parametrize("with_gt", [False, True])
def test_voxelize_aug_lowp(V, rec, pack, cam, with_gt, monkeypatch):
    monkeypatch.setattr(V, "_dev_check", lambda *a, **kw: None)        # (gt "on the GPU": the check is not under test)
    xf, index = torch.rand((N, 24), dtype=torch.float64), torch.tensor([2, 0, 1])
    gt = _f(N, 63) if with_gt else None
    out = V.voxelize_aug_lowp(*pack, xf, res=R, layout="cxyz", dtype=BF16, cam=cam, gt=gt, clamp=False, index=index)
    assert rec.names() == ["map_grids", "_map_grid_lowp"] + (["transform_joints", "normalize_joints"] if with_gt else [])
    (_, pa, mg), (_, va, (tsdf, _)) = rec.log[:2]
    assert _same_pack(pa, pack) and pa["xforms"] is xf and pa["res"] == R and pa["cam"] is cam and pa["index"] is index
    assert _same_pack(va, pack) and va["xforms"] is xf and va["grid"] is mg.grid and va["cam"] is cam
    assert (va["res"], va["layout"], va["dtype"]) == (R, "cxyz", BF16) and va["index"] is index
    assert va["out"] is None and va["want_status"] is False
    batch = out[0] if with_gt else out
    assert isinstance(batch, V.TsdfBatch) and batch.tsdf is tsdf
    assert batch.max_l is mg.max_l and batch.mid_p is mg.mid_p and batch.status is mg.status
    if with_gt:
        (_, ta, gt_aug), (_, na, gt_nor) = rec.log[2:]
        assert torch.equal(ta["gt"], gt.index_select(0, index)) and ta["xforms"] is xf
        assert na["gt"] is gt_aug and na["max_l"] is mg.max_l and na["mid_p"] is mg.mid_p and na["clamp"] is False
        assert out[1] is gt_nor and out[2] is gt_aug


# ---- the cloud placement ----
def _check_process(V, rec, log, pack, cam, dtype, seed, xforms=None):
    """The three stages of a cloud-placed half in ``log``; returns (cloud, grid, volume, combined status)."""
    (n0, pa, pc), (n1, ca, cg), (n2, va, (tsdf, st)) = log
    lowp = dtype is not None
    want = ("voxelize_grid", "voxelize_grid_lowp") if xforms is None else ("voxelize_aug_grid", "voxelize_map_grid_lowp")
    assert [n0, n1, n2] == ["point_clouds", "cloud_grids", want[lowp]]
    assert _same_pack(pa, pack) and (pa["points"], pa["seed"], pa["frame_base"]) == (P, seed, 9) and pa["cam"] is cam
    assert pa["xforms"] is xforms and pa["out"] is None
    assert ca["points"] is pc.points and ca["res"] == R and ca["cam"] is cam
    assert _same_pack(va, pack) and va["grid"] is cg.grid and (va["res"], va["layout"]) == (R, "cxyz") and va["cam"] is cam
    if lowp:
        assert va["dtype"] is dtype and va["index"] is None and va["out"] is None
    if xforms is not None:
        assert va["xforms"] is xforms
    return pc, cg, tsdf, _first(pc.status, cg.status, st)


@pytest.mark.parametrize("dtype", [None, BF16])
def test_process_batch(V, rec, pack, cam, dtype):
    out = V.process_batch(*pack, points=P, seed=7, frame_base=9, res=R, layout="cxyz", cam=cam, dtype=dtype)
    pc, cg, tsdf, status = _check_process(V, rec, rec.log, pack, cam, dtype, 7)
    assert isinstance(out, V.ProcessBatch) and out.points is pc.points and out.tsdf is tsdf and out.count is pc.count
    assert out.max_l is cg.max_l and out.mid_p is cg.mid_p
    assert out.status.tolist() == status.tolist() == [61, 31, 22] and out.status.dtype is torch.int32
    with pytest.raises(ValueError, match="float16 or torch.bfloat16"):
        V.process_batch(*pack, dtype=torch.float64)
    assert len(rec.log) == 3


@pytest.mark.parametrize("dtype,with_gt,own_maps", [(None, True, False), (BF16, False, False), (None, False, True)])
def test_process_batch_aug(V, rec, pack, cam, dtype, with_gt, own_maps):
    gt = _f(N, 21, 3) if with_gt else None
    mine = torch.rand((N, 24), dtype=torch.float64) if own_maps else None
    out = V.process_batch_aug(*pack, xforms=mine, gt=gt, points=P, seed=7, aug_seed=8, key=13, frame_base=9, res=R,
                              layout="cxyz", cam=cam, dtype=dtype)
    pc, cg, tsdf, status = _check_process(V, rec, rec.log[:3], pack, cam, dtype, 7)
    rest = rec.log[3:]
    if own_maps:
        xf = mine
    else:
        name, xa, xf = rest.pop(0)
        assert name == "aug_xforms" and xa["centres"] is cg.mid_p and (xa["key"], xa["counter0"]) == (13, 9)
        assert xa["n"] is None and xa["index"] is None
    pa, ca, tsdf_a, status_a = _check_process(V, rec, rest[:3], pack, cam, dtype, 8, xforms=xf)
    assert [e[0] for e in rest[3:]] == (["transform_joints"] if with_gt else [])
    gt_aug = None
    if with_gt:
        _, ta, gt_aug = rest[3]
        assert ta["gt"] is gt and ta["xforms"] is xf
    assert isinstance(out, V.ProcessAugBatch)
    want = (pc.points, tsdf, cg.max_l, cg.mid_p, pa.points, tsdf_a, ca.max_l, ca.mid_p, gt_aug, None, None, pc.count, xf)
    assert all(w is None or o is w for o, w in zip(out, want)) and out.gt_aug is gt_aug
    assert out.status.tolist() == status.tolist() and out.status_aug.tolist() == status_a.tolist() == [61, 31, 22]
    with pytest.raises(ValueError, match="float16 or torch.bfloat16"):
        V.process_batch_aug(*pack, dtype="bf16")
    assert len(rec.log) == 3 + (not own_maps) + 3 + with_gt


# ---- raw frames: locate, place, pass ----
FRAMES_ROWS = [
    # placement, dtype, tsdf, the primitives after locate_hands (without gt)
    ("aabb", None, "projective", ["voxelize"]),
    ("aabb", BF16, "projective", ["aabb", "voxelize_grid_lowp"]),
    ("aabb", None, "accurate", ["aabb", "voxelize_grid_accurate"]),
    ("aabb", BF16, "accurate", ["aabb", "voxelize_grid_accurate", "narrow_volumes"]),
    ("cube", None, "projective", ["voxelize_grid"]),
    ("cube", BF16, "projective", ["voxelize_grid_lowp"]),
    ("cube", None, "accurate", ["voxelize_grid_accurate"]),
    ("cube", BF16, "accurate", ["voxelize_grid_accurate", "narrow_volumes"]),
]


@pytest.mark.parametrize("with_gt", [False, True], ids=["", "gt"])
@pytest.mark.parametrize("placement,dtype,tsdf,chain", FRAMES_ROWS,
                         ids=["-".join(map(str, r[:3])).replace("torch.", "") for r in FRAMES_ROWS])
def test_voxelize_frames(V, rec, cam, placement, dtype, tsdf, chain, with_gt):
    frames, index = _f(4, 6, 7), torch.tensor([3, 0, 1])
    gt = _f(N, 63) if with_gt else None
    out = V.voxelize_frames(frames, R, placement=placement, dtype=dtype, gt=gt, layout="cxyz", tsdf=tsdf, cam=cam,
                            index=index, cube=200.0)
    fused = chain == ["voxelize"]
    if fused and with_gt:
        chain = ["voxelize_labels"]
    assert rec.names() == ["locate_hands"] + chain + (["normalize_joints"] if with_gt and not fused else [])
    _, la, crops = rec.log[0]
    assert la["frames"] is frames and la["res"] == R and la["grid"] is (placement == "cube") and la["cam"] is cam
    assert la["index"] is index and la["cube"] == 200.0
    assert len(out) == 2 + with_gt and out[1] is crops
    batch = out[0]
    assert isinstance(batch, V.TsdfBatch)
    pk = (crops.depth, crops.offsets, crops.headers)
    log = rec.log[1:]
    if fused:
        _, va, ret = log[0]
        assert _same_pack(va, pk) and (va["res"], va["layout"]) == (R, "cxyz") and va["cam"] is cam and va["out"] is None
        assert batch is (ret[0] if with_gt else ret)
        if with_gt:
            assert va["gt"] is gt and out[2] is ret[1]
        return
    if placement == "aabb":
        _, pa, ab = log.pop(0)
        assert _same_pack(pa, pk) and pa["res"] == R and pa["cam"] is cam
    _, va, (vol, st) = log.pop(0)
    assert _same_pack(va, pk) and (va["res"], va["layout"]) == (R, "cxyz") and va["cam"] is cam
    assert va.get("index") is None and va.get("out") is None          # (the index is the locator's: the crops are the batch)
    if tsdf == "projective" and dtype is not None:
        assert va["dtype"] is dtype
    if placement == "aabb":
        assert torch.equal(va["grid"], _aabb_rows(ab)) and _is_aabb_placement(batch, ab)
    else:
        assert va["grid"] is crops.grid
        assert batch.max_l is crops.max_l and batch.mid_p is crops.mid_p and batch.status is st
    if tsdf == "accurate" and dtype is not None:
        _, na, narrow = log.pop(0)
        assert na["tsdf32"] is vol and na["dtype"] is dtype and na["out"] is None
        vol = narrow
    assert batch.tsdf is vol and batch.tsdf.dtype is (dtype or torch.float32)
    if with_gt:
        _, ja, gt_nor = log.pop(0)
        assert ja["gt"] is gt and ja["max_l"] is batch.max_l and ja["mid_p"] is batch.mid_p and ja["clamp"] is True
        assert out[2] is gt_nor
    assert not log


def test_voxelize_frames_refusals_come_before_the_locator(V, rec):
    frames = _f(2, 6, 7)
    for kw, exc, text in ((dict(placement="obb"), ValueError, "placement"), (dict(layout="xyz"), ValueError, "layout"),
                          (dict(dtype=torch.float32), ValueError, "float16 or torch.bfloat16"),
                          (dict(tsdf="exact"), ValueError, "tsdf"), (dict(grid=False), TypeError, "grid and res")):
        with pytest.raises(exc, match=text):
            V.voxelize_frames(frames, R, **kw)
    assert not rec.log


# ---- the dispatcher itself ----
GRID_PASS_CELLS = [
    # xforms?, dtype, tsdf, the entries in order
    (False, None, "projective", ["voxelize_grid"]),
    (False, BF16, "projective", ["voxelize_grid_lowp"]),
    (True, None, "projective", ["voxelize_aug_grid"]),
    (True, torch.float16, "projective", ["voxelize_map_grid_lowp"]),
    (False, None, "accurate", ["voxelize_grid_accurate"]),
    (False, BF16, "accurate", ["voxelize_grid_accurate", "narrow_volumes"]),
]


@pytest.mark.parametrize("mapped,dtype,tsdf,chain", GRID_PASS_CELLS,
                         ids=["-".join(map(str, c[:3])).replace("torch.", "") for c in GRID_PASS_CELLS])
def test_grid_pass_table(V, rec, pack, cam, mapped, dtype, tsdf, chain):
    grid, xf = _f(N, 8), (torch.rand((N, 24), dtype=torch.float64) if mapped else None)
    takes_both = chain != ["voxelize_grid"] and chain != ["voxelize_aug_grid"]
    index, out = (torch.tensor([1, 1, 0]), _vol(dtype or torch.float32)) if takes_both else (None, None)
    vol, st = V._grid_pass(*pack, grid, res=R, layout="cxyz", cam=cam, xforms=xf, dtype=dtype, tsdf=tsdf, index=index, out=out)
    assert rec.names() == chain
    _, va, (v0, s0) = rec.log[0]
    assert _same_pack(va, pack) and va["grid"] is grid and (va["res"], va["layout"]) == (R, "cxyz") and va["cam"] is cam
    assert va.get("xforms") is xf and va.get("index") is index and st is s0
    if tsdf == "projective":
        assert va.get("dtype") is dtype and va.get("out") is out and vol is v0
    elif dtype is None:
        assert va["out"] is out and vol is v0
    else:   # the accurate pass allocates its float32 volume; the caller's buffer is the narrow one
        _, na, narrow = rec.log[1]
        assert va["out"] is None and na["tsdf32"] is v0 and na["dtype"] is dtype and na["out"] is out and vol is narrow


def test_grid_pass_refusals_launch_nothing(V, rec, pack, cam):
    grid, xf = _f(N, 8), torch.rand((N, 24), dtype=torch.float64)
    kw = dict(res=R, layout="czyx", cam=cam)
    for dtype in (None, BF16):
        with pytest.raises(ValueError, match="accurate pass under a per-frame map"):
            V._grid_pass(*pack, grid, xforms=xf, dtype=dtype, tsdf="accurate", **kw)
    for mapped, name in ((None, "voxelize_grid"), (xf, "voxelize_aug_grid")):
        for extra in (dict(index=torch.tensor([0])), dict(out=_vol())):
            with pytest.raises(ValueError, match=name + " takes neither index nor out"):
                V._grid_pass(*pack, grid, xforms=mapped, **extra, **kw)
    with pytest.raises(ValueError, match="float16 or torch.bfloat16"):
        V._grid_pass(*pack, grid, dtype=torch.float32, **kw)
    with pytest.raises(ValueError, match="tsdf must be"):
        V._grid_pass(*pack, grid, tsdf="exact", **kw)
    assert not rec.log


def test_first_status_is_the_written_out_where(V):
    a, b, c = _st(0, 1, 0, 2, 0, 0), _st(0, 3, 4, 0, 0, 1), _st(5, 6, 0, 7, 0, 2)
    got = V._first_status(a, b, c)
    assert got.dtype is torch.int32
    assert torch.equal(got, torch.where(a != 0, a, torch.where(b != 0, b, c))) and got.tolist() == [5, 1, 4, 2, 0, 1]
    assert torch.equal(V._first_status(b, c), torch.where(b != 0, b, c))
    assert V._first_status(c) is c


# ---- export.py: the six default hooks, uploads and the device wait replaced ----
def test_export_default_hooks(V, rec, pkg, synth, tmp_path, monkeypatch):
    import numpy as np

    export = importlib.import_module(PKG + ".export")
    synth.synth_msra_tree(str(tmp_path), n_sub=1, n_ges=1, n_frames=N, seed=8)
    pk = pkg.packing.pack_bin_files(pkg.packing.gesture_bin_paths(str(tmp_path / "P0" / "1"), N))
    to_torch = pkg.packing.PackedFrames.to_torch
    monkeypatch.setattr(pkg.packing.PackedFrames, "to_torch", lambda self, device, **kw: to_torch(self, "cpu"))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)

    def fused(depth, offsets, headers, xforms, gt=None, **kw):         # (voxelize_aug is fused: a primitive here)
        rec.log.append(("voxelize_aug", dict(kw, xforms=xforms, gt=gt), None))
        return rec._voxelize({}), torch.rand_like(gt), torch.rand_like(gt)
    monkeypatch.setattr(V, "voxelize_aug", fused)
    xf, gt, cloud = np.random.rand(N, 24), np.random.rand(N, 21, 3).astype(np.float32), np.random.rand(N, P, 3)
    for name, args, chain in (("_default_voxelize", (), ["voxelize"]),
                              ("_default_voxelize_accurate", (), ["aabb", "voxelize_grid_accurate"]),
                              ("_default_voxelize_aug", (xf, gt), ["voxelize_aug"]),
                              ("_default_voxelize_cloud", (cloud,), ["cloud_grids", "voxelize_grid"]),
                              ("_default_voxelize_cloud_accurate", (cloud,), ["cloud_grids", "voxelize_grid_accurate"]),
                              ("_default_voxelize_aug_cloud", (xf, cloud, gt),
                               ["cloud_grids", "voxelize_aug_grid", "transform_joints"])):
        del rec.log[:]
        out = getattr(export, name)(pk, *args, R, "cxyz", "cpu")
        assert rec.names() == chain, name
        assert len(out) == 4 + (len(args) >= 2) and all(isinstance(a, np.ndarray) for a in out)
        assert out[0].shape == (N, 3, R, R, R) and out[3].dtype == np.int32
        for _, a, _ in rec.log:
            assert a.get("res", R) == R and a.get("layout", "cxyz") == "cxyz" and a.get("cam") is None
            if a.get("xforms") is not None:
                assert np.array_equal(a["xforms"].numpy(), xf)
        if "cloud" in name:
            (_, ca, cg), (_, va, (vol, st)) = rec.log[:2]
            assert np.array_equal(ca["points"].numpy(), cloud) and va["grid"] is cg.grid
            assert np.array_equal(out[1], cg.max_l.numpy()) and np.array_equal(out[2], cg.mid_p.numpy())
            assert out[3].tolist() == _first(cg.status, st).tolist() == [61, 21, 22]
        if len(args) >= 2:                                             # the augmented hooks: the joints under the maps
            want = rec.log[-1][2] if "cloud" in name else None
            assert out[4].shape == (N, 63) and (want is None or np.array_equal(out[4], want.numpy()))
