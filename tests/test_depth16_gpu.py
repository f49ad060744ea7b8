"""GPU tier of the packs with 16-bit depth: the widen kernel of libtsdf_depth16.so (include/tsdf_depth16.h) on every
alignment, tail and input value, its stream order, and the loaders over 16-bit packs against the same loaders over the
float32 packs of the same frames.  The feature is lossless: numpy is the reference — ``q.astype(float32) *
float32(2.0 ** -k)`` — and every comparison is exact, bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = np.int32(0x7FC0BEEF)   # a NaN with a payload, as bits
N_PX = [0, 1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 4095, 4096, 4097, 1000003]
SRC_OFF = [0, 1, 3, 4, 7]
DST_OFF = [0, 1, 2, 3]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the kernel --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def source():
    """1,000,003 + 8 random uint16, on the host and on the GPU."""
    q = np.random.default_rng(16).integers(0, 65536, max(N_PX) + 8, dtype=np.uint16)
    q[:4] = [0, 65535, 1, 32768]
    return q, torch.from_numpy(q).to(dev())


@pytest.mark.parametrize("n_px", N_PX)
def test_widen_every_alignment_and_tail(pkg, source, n_px):
    """Source element offsets {0,1,3,4,7} x destination element offsets {0,1,2,3} (slices of larger tensors, whose own
    bases are 16-byte aligned) x shifts {0,3,7}: the values against numpy, and the sentinel everywhere outside
    [offset, offset + n_px) of the destination."""
    q, d_q = source
    assert d_q.data_ptr() % 16 == 0
    dst = torch.empty(n_px + 8, dtype=torch.float32, device=dev())
    assert dst.data_ptr() % 16 == 0
    want = np.empty(n_px + 8, f32)
    for shift in (0, 3, 7):
        scale = f32(2.0 ** -shift)
        for so in SRC_OFF:
            ref = q[so:so + n_px].astype(f32) * scale
            for do in DST_OFF:
                dst.view(torch.int32).fill_(int(SENTINEL))
                out = pkg.widen_depth16(d_q[so:so + n_px], shift, out=dst[do:do + n_px])
                assert n_px == 0 or (out.data_ptr() == dst.data_ptr() + 4 * do and out.data_ptr() % 16 == (4 * do) % 16)
                want.view(np.int32)[:] = SENTINEL
                want[do:do + n_px] = ref
                got = dst.cpu().numpy()
                assert np.array_equal(got.view(np.int32), want.view(np.int32)), (n_px, shift, so, do)
    # allocated by the wrapper, and shaped like the source
    out = pkg.widen_depth16(d_q[1:1 + n_px], 3)
    assert out.dtype == torch.float32 and out.shape == (n_px,)
    assert np.array_equal(out.cpu().numpy().view(np.int32), (q[1:1 + n_px].astype(f32) * f32(0.125)).view(np.int32))


@pytest.mark.parametrize("shift", range(8))
def test_widen_every_input_value(pkg, shift):
    q = np.arange(65536, dtype=np.uint16)
    out = pkg.widen_depth16(torch.from_numpy(q).to(dev()), shift).cpu().numpy()
    want = q.astype(f32) * f32(2.0 ** -shift)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(out.astype(np.float64) * 2.0 ** shift, q.astype(np.float64))    # and that IS q * 2^-k, exactly


def test_widen_wrapper_checks(pkg):
    d = dev()
    u16 = torch.zeros(64, dtype=torch.uint16, device=d)
    with pytest.raises(TypeError):
        pkg.widen_depth16(torch.zeros(64, dtype=torch.int16, device=d), 0)
    with pytest.raises(ValueError):
        pkg.widen_depth16(u16[::2], 0)                                  # not contiguous
    with pytest.raises(ValueError):
        pkg.widen_depth16(u16, 8)
    with pytest.raises(ValueError):
        pkg.widen_depth16(u16, 0, out=torch.zeros(63, dtype=torch.float32, device=d))
    with pytest.raises(TypeError):
        pkg.widen_depth16(u16, 0, out=torch.zeros(64, dtype=torch.float64, device=d))
    with pytest.raises(ValueError):
        pkg.widen_depth16(u16, 0, out=torch.zeros(64, dtype=torch.float32))   # a host destination
    assert pkg.widen_depth16(u16[:0], 5).shape == (0,)


def test_widen_in_stream_order_after_a_pinned_copy(pkg):
    """The _Staging sequence at 4096 pixels: on a side stream an asynchronous copy out of pinned memory, the widen, an
    event; a consumer stream that waits on the event reads the right values."""
    d = dev()
    n = 4096
    q = np.random.default_rng(2).integers(0, 65536, n, dtype=np.uint16)
    h = torch.empty(n, dtype=torch.uint16).pin_memory()
    h.numpy()[:] = q
    d_q = torch.zeros(n, dtype=torch.uint16, device=d)
    d_f = torch.full((n,), -1.0, dtype=torch.float32, device=d)
    side, consumer, copied = torch.cuda.Stream(device=d), torch.cuda.Stream(device=d), torch.cuda.Event()
    torch.cuda.synchronize(d)
    with torch.cuda.stream(side):
        d_q.copy_(h, non_blocking=True)
        pkg.widen_depth16(d_q, 4, out=d_f)
        copied.record(side)
    with torch.cuda.stream(consumer):
        consumer.wait_event(copied)
        seen = d_f.clone()
    consumer.synchronize()
    assert np.array_equal(seen.cpu().numpy().view(np.uint32), (q.astype(f32) * f32(2.0 ** -4)).view(np.uint32))


# ---- the loaders ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def packs(pkg, synth):
    """48 MSRA-like crops quantised to eighths of a millimetre, with labels: as float32 packs and as their 16-bit twins,
    split 24 + 24 and as one pack of 48."""
    depth, off, hdr = synth.synth_batch(48, "crop", seed0=4800)
    depth = (np.round(depth * 8) / 8).astype(f32)
    gt = np.random.default_rng(7).normal(0, 50, (48, 63)).astype(f32)
    gt[:, 2::3] -= 450.0
    whole = pkg.packing.PackedFrames(depth, off, hdr, gt)
    assert pkg.packing.depth16_shift(depth) == 3
    out = {}
    for name, cuts in (("two", [(0, 24), (24, 48)]), ("one", [(0, 48)])):
        p32 = [whole.slice(a, b) for a, b in cuts]
        for p in p32:
            p.depth = np.ascontiguousarray(p.depth)
        p16 = [p.to_depth16() for p in p32]
        assert all(p.depth_shift == 3 and p.depth.dtype == np.uint16 for p in p16)
        out[name] = (p32, p16)
    return out


def fresh(pkg, ps):
    """Packs of their own for one loader (pinning replaces a pack's depth array)."""
    P = pkg.packing.PackedFrames
    return pkg.MSRADepthDataset.from_packs([P(p.depth.copy(), p.offsets, p.headers, p.gt, depth_shift=p.depth_shift)
                                            for p in ps])


def same_batch(a, b):
    assert type(a) is type(b) and len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))     # every field, bit for bit


@pytest.mark.parametrize("split", ["two", "one"])
@pytest.mark.parametrize("shuffle", [False, True])
def test_voxel_loader_over_16_bit_packs_equals_float32(pkg, packs, split, shuffle):
    p32, p16 = packs[split]
    kw = dict(batch_size=16, device=dev(), shuffle=shuffle, seed=5, max_pixels=16 * 160 * 160)
    a, b = pkg.VoxelLoader(fresh(pkg, p32), **kw), pkg.VoxelLoader(fresh(pkg, p16), **kw)
    assert b.ds.depth_shift == 3 and a.ds.depth_shift is None
    for epoch in range(2):                                     # the second epoch reuses the staging sets
        n = 0
        for x, y in zip(a, b):
            same_batch(x, y)
            assert bool((y.status == 0).all()) and bool(y.tsdf.any())
            n += y.tsdf.shape[0]
        assert n == 48
    s = b._sets[0]
    assert s.h_depth.dtype == torch.uint16 and s.h_depth.is_pinned() and s.d_depth16.dtype == torch.uint16
    assert s.d_depth.dtype == torch.float32 and s.d_depth16.numel() == s.d_depth.numel() == b.max_px
    assert a._sets[0].d_depth16 is None and a._sets[0].h_depth.dtype == torch.float32
    assert all(pk._pinned.dtype == torch.uint16 for pk in b.ds.packs)          # pinned at half the bytes


def test_voxel_loader_without_pinned_packs(pkg, packs):
    p32, p16 = packs["two"]
    kw = dict(batch_size=16, device=dev(), max_pixels=16 * 160 * 160, pin_packs=False)
    for x, y in zip(pkg.VoxelLoader(fresh(pkg, p32), **kw), pkg.VoxelLoader(fresh(pkg, p16), **kw)):
        same_batch(x, y)


@pytest.mark.parametrize("prefetch", [1, 4])
def test_resident_loader_over_16_bit_packs_equals_float32(pkg, packs, prefetch):
    p32, p16 = packs["two"]
    kw = dict(batch_size=16, device=dev(), shuffle=True, seed=9, prefetch=prefetch)
    a, b = pkg.ResidentLoader(fresh(pkg, p32), **kw), pkg.ResidentLoader(fresh(pkg, p16), **kw)
    assert a.resident_bytes() == b.resident_bytes() == 4 * sum(int(p.depth.size) for p in p32)
    for epoch in range(2):
        n = 0
        for x, y in zip(a, b):
            same_batch(x, y)
            n += y.tsdf.shape[0]
        assert n == 48
    assert b._dev[0].dtype == torch.float32 and same_bits(a._dev[0], b._dev[0])   # what is resident is float32


def test_msra_dataset_under_a_dataloader_equals_float32(pkg, packs):
    p32, p16 = packs["two"]
    d = dev()
    dls = []
    for ps in (p32, p16):
        ds = pkg.MSRA_Dataset.from_raw(fresh(pkg, ps), device=d)
        assert ds.resident
        dls.append(torch.utils.data.DataLoader(ds, batch_size=16, shuffle=True, generator=torch.Generator().manual_seed(3)))
    n = 0
    for x, y in zip(*dls):
        assert len(x) == len(y) == 4
        for u, v in zip(x, y):
            assert same_bits(u, v)
        n += y[0].shape[0]
    assert n == 48
    # the host-fed paths (resident=False) decode through PackedFrames.to_torch
    h32, h16 = (pkg.MSRA_Dataset.from_raw(fresh(pkg, ps), device=d, resident=False) for ps in (p32, p16))
    for u, v in zip(h32.__getitems__([40, 3, 17, 25]), h16.__getitems__([40, 3, 17, 25])):
        assert all(same_bits(s, t) for s, t in zip(u, v))
    assert all(same_bits(s, t) for s, t in zip(h32[30], h16[30]))


def test_to_torch_uploads_16_bits_and_widens(pkg, packs):
    p32, p16 = packs["one"]
    d = dev()
    a, b = p32[0].to_torch(d), p16[0].to_torch(d, pin=True, non_blocking=True)
    assert b[0].dtype == torch.float32 and b[0].is_cuda and same_bits(a[0], b[0])
    x, y = pkg.voxelize(*a), pkg.voxelize(*b)
    same_batch(x, y)
    assert bool((y.status == 0).all())
    out = pkg.dataset.voxelize_batch(p16[0], p16[0].gt, d)
    assert same_bits(out[0], x.tsdf) and same_bits(out[2], x.max_l)
