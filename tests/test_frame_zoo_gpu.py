"""GPU tier of the frame zoo (tests/frame_zoo.py): every kernel form and every entry of the core voxelizer
(csrc/tsdf_hip.hip) over the frames that break row streaming and pixel staging — short, tall and wide boxes, rectangles of
valid pixels on both sides of the LDS pool's size, valid pixels in one edge row or column only, degenerate and NaN-laden
frames — against the oracle.

One master batch (the zoo, then fresh draws) is voxelized by the oracle once per (R, layout, augmented); every launch is a
gather of master frames, so its reference is a gather of that result, compared on the device.  Bounds are the project's:
status, max_l and mid_p bit for bit, volumes within TOL (tests/test_parity_gpu.py), bit for bit between two paths of the
library wherever an existing test asserts that already (captured replay == eager launch, indexed == gathered, the label
entries == the plain entry).  No frame and no voxel is left out.  Batch sizes follow the CU count (kernel_path / n_for of
tests/test_pca_paths_gpu.py); the form a launch takes is asserted with tsdf_describe_launch."""
import functools
import importlib

import numpy as np
import pytest
import torch

import frame_zoo as fz
import oracle
import plan_ref
from pca_ref import same_bits
from test_parity_gpu import TOL
from test_pca_paths_gpu import PKG, _basis, _described, _expect, groups_for, kernel_path, n_for

pytestmark = pytest.mark.gpu
DEV = "cuda"
Z = len(fz.zoo())
LAY = {"czyx": 0, "cxyz": 1}


@functools.lru_cache(maxsize=None)
def _cus():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus >= Z, "an MI355X has 256 CUs: a one-group static launch holds the whole zoo"
    return cus


def _queue_n(R):
    cus = _cus()
    return n_for("queue", R, cus, groups_for(R) * cus + 5)


def _master_n(R):
    """Frames of the master batch at R: the largest launch there (the queue path's)."""
    return _queue_n(R)


def _t(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(DEV)     # (the references are read-only)


# ---- references: once per (R, layout, aug), read-only, on the host and on the device --------------------------------

@functools.lru_cache(maxsize=None)
def _maps():
    """The maps of the augmented runs, one per master frame (about its own plain grid centre)."""
    plain = oracle.voxelize(*fz.master(_master_n(32)), R=32, n_threads=8, want_tsdf=False)
    xf = fz.aug_maps(plain["mid_p"])
    xf.setflags(write=False)
    return xf


@functools.lru_cache(maxsize=None)
def _ref(R, layout, aug):
    n = _master_n(R)
    parts = fz.take(fz.master(_master_n(32)), np.arange(n))
    if aug:
        ref = oracle.voxelize_aug(*parts, _maps()[:n], R=R, layout=LAY[layout], n_threads=8)
    else:
        ref = oracle.voxelize(*parts, R=R, layout=LAY[layout], n_threads=8, extras=True)
    ref = {k: v for k, v in ref.items() if isinstance(v, np.ndarray)}
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _ref_dev(R, layout, aug):
    return {k: _t(v) for k, v in _ref(R, layout, aug).items()}


@pytest.fixture(scope="module", autouse=True)
def _release_references():
    yield
    for f in (_ref_dev, _ref, _pixmaps, _batch):
        f.cache_clear()


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _same_batch(a, b, what):
    """Two launches of the library bit for bit: status, placement and every voxel."""
    for k in ("status", "max_l", "mid_p", "tsdf"):
        assert _bits_equal(getattr(a, k), getattr(b, k)), f"{what}: {k} differs"


def _check(out, R, layout, aug, sel, what, rows=None):
    """A launch over the master frames ``sel`` against the oracle: every frame, every voxel.  ``rows``: the positions of the
    launch that ``sel`` describes (default: all of them, in order)."""
    ref = _ref_dev(R, layout, aug)
    s = _t(np.asarray(sel, np.int64))
    pick = (lambda x: x) if rows is None else (lambda x, r=_t(np.asarray(rows, np.int64)): x[r])
    assert torch.equal(pick(out.status), ref["status"][s]), f"{what}: status"
    for k in ("max_l", "mid_p"):
        assert _bits_equal(pick(getattr(out, k)), ref[k][s]), f"{what}: {k} differs from the oracle"
    err = float((pick(out.tsdf) - ref["tsdf"][s]).abs().max())
    print(f"{what}: {len(sel)} frames, max |hip - oracle| = {err:.3g}")
    assert err <= TOL, f"{what}: max |hip - oracle| = {err}"     # (a NaN fails this too)


# ---- batches ------------------------------------------------------------------------------------------------------------

def _sel_for(size, R):
    """The master frames of a launch of this size class ("split16", "splitmax", "static", "queue") at R, in launch order,
    and the path it takes."""
    cus = _cus()
    if size == "queue":
        return fz.whole_batch(_queue_n(R), 11), "queue"
    if size == "static":
        n = n_for("static", R, cus, 300 if groups_for(R) == 2 else 240)
        assert n >= Z
        return fz.whole_batch(n, 12), "static"
    n = n_for("split", R, cus, 16 if size == "split16" else 128)
    return fz.geometry_batch(n, 13 if size == "split16" else 14), "split"


@functools.lru_cache(maxsize=None)
def _batch(size, R):
    sel, path = _sel_for(size, R)
    parts = fz.take(fz.master(_master_n(32)), sel)
    return sel, path, tuple(_t(a) for a in parts), _t(_maps()[sel])


def _assert_form(pkg, n, R, layout, aug, path):
    """The kernel the launch takes, as the library describes it."""
    cus = _cus()
    assert kernel_path(n, R, cus) == path
    got = _described(pkg, n, R, LAY[layout], aug)
    rt = R if R in (32, 64) else 0
    a = "true" if aug else "false"
    if path == "split":
        assert got.startswith("tsdf_split_kernel<%d, %d, %s, " % (rt, LAY[layout], a)), got
    else:
        assert got == "tsdf_fused_kernel<%d, %d, %s, false, %d>" % (rt, LAY[layout], a, groups_for(R)), got
    assert got.startswith(plan_ref.describe(n, R, LAY[layout], aug, cus)), got
    return got


def _id(case):
    return "-".join(str(c) for c in case)


# ---- plain --------------------------------------------------------------------------------------------------------------

PLAIN = [(32, "cxyz", "queue"), (32, "czyx", "static"), (32, "cxyz", "static"),
         (48, "czyx", "queue"), (48, "czyx", "static"), (64, "czyx", "queue"), (64, "czyx", "static"),
         (40, "czyx", "static"),                      # generic (no tables of its own size) with two groups
         (32, "czyx", "split16"), (32, "czyx", "splitmax"), (48, "czyx", "split16"),
         (64, "czyx", "split16"), (64, "czyx", "splitmax")]


@pytest.mark.parametrize("case", PLAIN, ids=_id)
def test_plain(pkg, case):
    R, layout, size = case
    sel, path, (d, o, h), _ = _batch(size, R)
    _assert_form(pkg, len(sel), R, layout, False, path)
    out = pkg.voxelize(d, o, h, res=R, layout=layout)
    torch.cuda.synchronize()
    _check(out, R, layout, False, sel, _id(case))


# ---- augmented ----------------------------------------------------------------------------------------------------------

AUG = [(R, layout, size) for R, layout in ((32, "czyx"), (32, "cxyz"), (48, "czyx"), (64, "czyx"))
       for size in ("split16", "static", "queue")] + [(40, "czyx", "queue")]


@pytest.mark.parametrize("case", AUG, ids=_id)
def test_augmented(pkg, case):
    R, layout, size = case
    sel, path, (d, o, h), xf = _batch(size, R)
    _assert_form(pkg, len(sel), R, layout, True, path)
    out = pkg.voxelize_aug(d, o, h, xf, res=R, layout=layout)
    plain = pkg.voxelize(d, o, h, res=R, layout=layout)
    torch.cuda.synchronize()
    _check(out, R, layout, True, sel, _id(case))
    # identity-map frames: the plain launch's placement bit for bit, its volume within TOL
    ident = _t(np.nonzero(sel % 5 == 0)[0])
    assert len(ident) >= len(sel) // 8
    assert _bits_equal(out.max_l[ident], plain.max_l[ident]) and _bits_equal(out.mid_p[ident], plain.mid_p[ident])
    assert torch.equal(out.status[ident], plain.status[ident])
    err = float((out.tsdf[ident] - plain.tsdf[ident]).abs().max())
    print(f"{_id(case)}: identity maps vs plain: {err:.3g}")
    assert err <= TOL


# ---- captured -----------------------------------------------------------------------------------------------------------

# (a) fused with no queue word; (b) the split kernel's redundant form: span capture, and capture refused at 321 columns,
# at 257 rows and on the dense frame
CAPTURED = [(32, False, "queue"), (64, True, "queue")] + \
           [(R, aug, size) for R in (32, 48, 64) for aug in (False, True) for size in ("split16", "splitmax")]


def _poison(out):
    out.tsdf.fill_(7.0)
    out.max_l.fill_(-1.0)
    out.mid_p.fill_(-1.0)
    out.status.fill_(99)


@pytest.mark.parametrize("case", CAPTURED, ids=_id)
def test_captured(pkg, case):
    R, aug, size = case
    layout = "czyx"
    sel, path, (d, o, h), xf = _batch(size, R)
    _assert_form(pkg, len(sel), R, layout, aug, path)
    if size != "queue":   # what the redundant form has to refuse is in the batch
        shapes = {fz.zoo()[i].img.shape for i in sel}
        assert any(s[1] > 320 for s in shapes) and any(s[0] > 256 for s in shapes)
        assert size == "split16" or (240, 320) in shapes

    def launch(out=None):
        if aug:
            return pkg.voxelize_aug(d, o, h, xf, res=R, layout=layout, out=out)
        return pkg.voxelize(d, o, h, res=R, layout=layout, out=out)

    eager = launch()
    out = launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    cs = torch.cuda.Stream(DEV)
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):
        with torch.cuda.graph(g, stream=cs):
            launch(out)
    for rep in range(2):
        _poison(out)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _same_batch(out, eager, f"{_id(case)} replay {rep}")
    _check(out, R, layout, aug, sel, _id(case))


# ---- labels, PCA, indexed -----------------------------------------------------------------------------------------------

def _gt(n_master, J=21):
    """Joints around every master frame's plain grid (some outside the cube: the clamp bites): float32[n, 3J]."""
    ref = _ref(32, "czyx", False)
    rng = np.random.default_rng(77)
    gt = ref["mid_p"][:n_master, None, :] + rng.normal(0, 1, (n_master, J, 3)) * ref["max_l"][:n_master, None, None] * 0.45
    return np.ascontiguousarray(gt.astype(np.float32).reshape(n_master, 3 * J))


@pytest.mark.parametrize("case", [(32, "cxyz", "queue"), (32, "czyx", "splitmax"), (64, "czyx", "split16")], ids=_id)
def test_labels_and_pca(pkg, case):
    R, layout, size = case
    J, k = 21, 50
    sel, path, (d, o, h), _ = _batch(size, R)
    _assert_form(pkg, len(sel), R, layout, False, path)
    pca = _basis(importlib.import_module(PKG + ".pca"), J)
    gt = _gt(_master_n(32), J)[sel]
    g = _t(gt)
    plain = pkg.voxelize(d, o, h, res=R, layout=layout)
    for clamp in (True, False):
        out, nor = pkg.voxelize_labels(d, o, h, g, res=R, layout=layout, clamp=clamp)
        outp, norp, gt_pca = pkg.voxelize_labels(d, o, h, g, res=R, layout=layout, clamp=clamp, pca=pca, k=k)
        torch.cuda.synchronize()
        _same_batch(out, plain, f"{_id(case)} labels")
        _same_batch(outp, plain, f"{_id(case)} labels + pca")
        ref = _ref(R, layout, False)
        want = oracle.normalize_joints(gt, ref["max_l"][sel], ref["mid_p"][sel], clamp=clamp)
        assert same_bits(nor, want) and same_bits(norp, want)
        assert same_bits(gt_pca, _expect(gt, outp, pca, k))
    _check(plain, R, layout, False, sel, _id(case))
    st = plain.status.cpu().numpy()
    assert (st != 0).any() or size == "split16"      # (the larger batches hold the degenerate short frames)
    assert same_bits(nor[_t(np.nonzero(st != 0)[0])], np.full(((st != 0).sum(), 3 * J), 0.5, np.float32))


@pytest.fixture(scope="module")
def pack():
    """The zoo as a resident pack with its labels."""
    d, o, h = (_t(a) for a in fz.master(Z))
    return d, o, h, _t(_gt(_master_n(32))[:Z])


def test_indexed_resident_pack(pkg, pack):
    """A permuted index over the whole zoo with repeats and two bad entries, on the device and pinned: bit-equal to
    voxelizing the gathered frames, and within the oracle's bounds."""
    d, o, h, g = pack
    rng = np.random.default_rng(21)
    idx = np.concatenate([rng.permutation(Z), rng.integers(0, Z, 38), [-1, Z]]).astype(np.int64)
    idx = idx[rng.permutation(len(idx))]
    n = len(idx)
    _assert_form(pkg, n, 32, "czyx", False, kernel_path(n, 32, _cus()))
    good = np.nonzero((idx >= 0) & (idx < Z))[0]
    assert len(good) == n - 2 and len(set(idx[good].tolist())) == Z
    gd, go, gh = (_t(a) for a in fz.take(fz.master(Z), idx[good]))
    want, want_nor = pkg.voxelize_labels(gd, go, gh, g[_t(idx[good])])
    tgood, tbad = _t(good), _t(np.setdiff1d(np.arange(n), good))
    for index in (_t(idx), torch.from_numpy(idx).pin_memory()):
        got, nor, gt_b = pkg.voxelize_indexed(d, o, h, index, g, gt_copy=True)
        torch.cuda.synchronize()
        for k in ("status", "max_l", "mid_p", "tsdf"):
            assert _bits_equal(getattr(got, k)[tgood], getattr(want, k)), k
        assert _bits_equal(nor[tgood], want_nor) and _bits_equal(gt_b[tgood], g[_t(idx[good])])
        assert got.status[tbad].tolist() == [2, 2] and not bool(got.tsdf[tbad].any())
        _check(got, 32, "czyx", False, idx[good], "indexed", rows=good)
        plain = pkg.voxelize_indexed(d, o, h, index)
        assert _bits_equal(plain.tsdf, got.tsdf) and _bits_equal(plain.mid_p, got.mid_p)
        # the PCA-carrying indexed entry: every other output unchanged, the projection by the restatement
        pca = _basis(importlib.import_module(PKG + ".pca"), 21)
        gotp, norp, gt_p, gt_pca = pkg.voxelize_indexed(d, o, h, index, g, gt_copy=True, pca=pca, k=50)
        torch.cuda.synchronize()
        _same_batch(gotp, got, "indexed + pca")
        assert _bits_equal(norp[tgood], nor[tgood])
        labels = gt_p.cpu().numpy()
        labels[np.setdiff1d(np.arange(n), good)] = 0          # (a bad index copies no labels; its frame is not OK)
        assert same_bits(gt_pca, _expect(labels, gotp, pca, 50))


@pytest.mark.parametrize("R", [32, 64])
def test_indexed_by_value(pkg, pack, R):
    """An index of short and wide frames in ordinary host memory (it travels inside the kernel arguments)."""
    d, o, h, g = pack
    rng = np.random.default_rng(22)
    idx = np.asarray(fz.subset("short", "wide"), np.int64)
    idx = np.concatenate([idx, idx[:2]])[: pkg._lib.INLINE_INDEX_MAX]
    idx = idx[rng.permutation(len(idx))]
    assert len(idx) == 32 and set(fz.subset("wide")) <= set(idx.tolist())
    _assert_form(pkg, len(idx), R, "czyx", False, "split")
    gd, go, gh = (_t(a) for a in fz.take(fz.master(Z), idx))
    want, want_nor = pkg.voxelize_labels(gd, go, gh, g[_t(idx)], res=R)
    host = torch.from_numpy(idx.copy())
    assert not host.is_pinned()
    got, nor = pkg.voxelize_indexed(d, o, h, host, g, res=R)
    host.fill_(0)                                   # (the call has read it already)
    torch.cuda.synchronize()
    _same_batch(got, want, "by value")
    assert _bits_equal(nor, want_nor)
    _check(got, R, "czyx", False, idx, "by value R=%d" % R)


# ---- aabb only ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [32, 64])
def test_aabb_only(pkg, R):
    """Phase 1 and the glue alone (no volume, so no pool lock) over the queue-sized batch, bit for bit."""
    sel, path, (d, o, h), _ = _batch("queue", R)
    r = pkg.aabb(d, o, h, res=R)
    torch.cuda.synchronize()
    ref = _ref_dev(R, "czyx", False)
    s = _t(sel)
    assert torch.equal(r.status, ref["status"][s])
    for k in ("aabb", "grid", "ori"):
        assert _bits_equal(getattr(r, k), ref[k][s]), k


# ---- pixel maps ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pixmaps(R):
    """The oracle's pixel map of every zoo frame on its own grid: int32[Z, R, R, R] indexed [z, y, x]; -1 throughout for a
    frame that is not OK."""
    ref = _ref(R, "czyx", False)
    depth, off, hdr = fz.master(Z)
    pm = np.full((Z, R, R, R), -1, np.int32)
    for i in range(Z):
        if ref["status"][i] == 0:
            pm[i] = oracle.voxels(depth[off[i]:off[i + 1]], hdr[i], ref["ori"][i], ref["grid"][i, 4], ref["grid"][i, 5],
                                  R=R, want_pixmap=True)[1]
    pm.setflags(write=False)
    return pm


@pytest.mark.parametrize("layout", ["czyx", "cxyz"])
@pytest.mark.parametrize("R", [32, 48])
def test_pixel_maps(pkg, R, layout):
    """The diagnostic build (the whole bounding box is what it stages) over the zoo: the pixel every voxel gathers, equal to
    the oracle's."""
    sel = fz.whole_batch(Z, 15)
    d, o, h = (_t(a) for a in fz.take(fz.master(Z), sel))
    t, pm, st = pkg.voxel_pixels(d, o, h, res=R, layout=layout)
    torch.cuda.synchronize()
    want = _t(_pixmaps(R))[_t(sel)]
    bad = (pm != want).reshape(Z, -1).any(dim=1).nonzero().flatten().tolist()
    assert not bad, "pixel maps differ in frames %s" % [fz.zoo()[sel[i]].name for i in bad[:10]]
    ref = _ref_dev(R, layout, False)
    s = _t(sel)
    assert torch.equal(st, ref["status"][s])
    err = float((t - ref["tsdf"][s]).abs().max())
    print(f"pixel maps R={R} {layout}: volumes max |hip - oracle| = {err:.3g}")
    assert err <= TOL
