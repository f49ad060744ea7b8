"""CPU tier of the device-drawn augmentation (include/tsdf_augment.h): the numpy restatement of the draws
(augment.device_draws_np, augment.device_key) is pinned to recorded values and to the reference's distributions, and
libtsdf_augment.so is checked as far as it goes without a GPU — exports, version, argument checks before device work."""
import ctypes
import itertools

import numpy as np
import pytest
from abi_util import declared_functions, exported

M = 1 << 64


def test_mix_is_splitmix64(pkg):
    """The first outputs of splitmix64 seeded with 0 (the published test vector of the generator): mix(0),
    mix(golden), ... — the state advances by the golden-ratio constant, which mix adds itself."""
    aug = pkg.augment
    golden = 0x9E3779B97F4A7C15
    assert [aug._mix((k * golden) % M) for k in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    z = np.array([0, golden, (2 * golden) % M, M - 1], np.uint64)
    with np.errstate(over="ignore"):
        assert [int(v) for v in aug._mix_np(z)] == [aug._mix(int(v)) for v in z]


# (key, counters) -> (stretch as float.hex, rot_xy, rot_z), recorded from device_draws_np when it was written; the rows
# cover key = 2^64 - 1 and counters whose sum with the key, or with counter0, wraps past 2^64
RECORDED = [
    (0, [0, 1, 2],
     ["0x1.35db0da76aea9p+0", "0x1.f26d72636c5fap-1", "0x1.fcadd483c511dp-1"], [-21, 1, 22], [0, 14, 4]),
    (M - 1, [0, 1, M - 1],
     ["0x1.f198bc6cd4641p-1", "0x1.35db0da76aea9p+0", "0x1.2d2e1d8a81e62p+0"], [-6, -21, 11], [-11, 0, -1]),
    (12345, [M - 2, M - 1, M, M + 1],
     ["0x1.210c9ae06ca6fp+0", "0x1.82e1e02b4cea2p-1", "0x1.5c164ae0d914ep-1", "0x1.6d025867aede2p+0"],
     [-28, 0, 20, -12], [1, -4, 2, 21]),
    (902413603941569471, [5], ["0x1.943ae2a32dca1p-1"], [3], [20]),
]


@pytest.mark.parametrize("key,counters,stretch,rot_xy,rot_z", RECORDED)
def test_device_draws_are_bit_stable(pkg, key, counters, stretch, rot_xy, rot_z):
    s, rx, rz = pkg.augment.device_draws_np(key, counters)
    assert s.dtype == np.float64 and rx.dtype == np.int64 and rz.dtype == np.int64
    assert [float(v).hex() for v in s] == stretch
    assert rx.tolist() == rot_xy and rz.tolist() == rot_z


def test_device_draws_depend_on_key_plus_counter_mod_2_64(pkg):
    aug = pkg.augment
    a = aug.device_draws_np(M - 1, [1, 2, 3])                 # key + c wraps to 0, 1, 2
    b = aug.device_draws_np(0, [0, 1, 2])
    c = aug.device_draws_np(0, [M, M + 1, M + 2])             # counter0 + i wraps
    d = aug.device_draws_np(7, np.array([M - 7, M - 6, M - 5], dtype=object))
    for x in (a, c, d):
        for u, v in zip(x, b):
            assert np.array_equal(u, v)
    # scalar formulas of the contract on Python integers, for a few counters
    for key, cnt in ((0, 0), (M - 1, 12345), (3, M - 2)):
        h = aug._mix((key + cnt) % M)
        lo = 2.0 / 3.0
        want_s = lo + float(aug._mix(h) >> 11) * 2.0 ** -53 * (1.5 - lo)
        want_r = [-30 + (((aug._mix((h + k) % M) >> 32) * 60) >> 32) for k in (1, 2)]
        s, rx, rz = aug.device_draws_np(key, [cnt])
        assert float(s[0]) == want_s and [int(rx[0]), int(rz[0])] == want_r


def test_device_draws_have_the_reference_distributions(pkg):
    """60,000 consecutive counters under key 0 (key 0 passed when first run; nothing was re-picked): U(2/3, 3/2) and
    integers in [-30, 30) (pre/process.py:209-216).  Means within 5 standard errors: sd of the uniform is (5/6)/sqrt(12),
    of the 60 integers sqrt((60^2 - 1)/12)."""
    n = 60000
    s, rx, rz = pkg.augment.device_draws_np(0, np.arange(n))
    assert s.min() >= 2.0 / 3.0 and s.max() < 1.5
    se_s = (1.5 - 2.0 / 3.0) / np.sqrt(12.0 * n)
    se_r = np.sqrt((60.0 ** 2 - 1) / 12.0 / n)
    assert abs(s.mean() - 13.0 / 12.0) <= 5 * se_s
    for r in (rx, rz):
        assert sorted(set(r.tolist())) == list(range(-30, 30))
        assert abs(r.mean() + 0.5) <= 5 * se_r
    assert not np.array_equal(rx, rz)


def test_device_key_is_injective_over_small_arguments(pkg):
    aug = pkg.augment
    keys = {aug.device_key(s, e, r) for s, e, r in itertools.product(range(3), repeat=3)}
    assert len(keys) == 27 and all(0 <= k < M for k in keys)
    assert aug.device_key(9, 1, 0) == aug._mix((aug._mix((aug._mix(9) + 1) % M) + 0) % M) == 902413603941569471


def test_augment_library_exports_exactly_its_header(pkg):
    want = declared_functions("tsdf_augment.h")
    assert want == ["tsdf_aug_draw_hip", "tsdf_augment_version"]
    funcs, named = exported(pkg._lib.AUGMENT_LIB_PATH)
    assert funcs == want                                                               # the functions it defines
    assert named == want
    A = pkg._lib.load_augment()
    assert A.tsdf_augment_version() == 1 == pkg._lib.AUGMENT_VERSION
    assert pkg._lib.load_augment() is A
    assert pkg._lib.load() is not A and pkg._lib.load().tsdf_version() == 7          # the product is untouched


def test_argument_validation_happens_before_device_work(pkg):
    A = pkg._lib.load_augment()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(20)
    draw = A.tsdf_aug_draw_hip
    # centres, n_src, index, n, key, counter0, stream, xforms, stretch, rot
    assert draw(one, 4, null, -1, 0, 0, null, one, null, null) == -1           # n < 0
    assert draw(null, 4, null, 1, 0, 0, null, one, null, null) == -1           # no centres
    assert draw(one, 4, null, 1, 0, 0, null, null, null, null) == -1           # no xforms
    assert draw(one, 0, null, 1, 0, 0, null, one, null, null) == -1            # n_src < 1
    assert draw(one, -3, one, 1, 0, 0, null, one, one, one) == -1
    assert draw(one, 4, null, 1, 0, 0, null, odd, null, null) == -1            # xforms not 8-byte aligned
    assert draw(one, 4, one, 1, M - 1, M - 1, null, odd, one, one) == -1
    # n == 0 is a no-op, whatever else is passed
    assert draw(null, 0, null, 0, 0, 0, null, null, null, null) == 0
    assert draw(one, 4, one, 0, 1, 2, null, odd, one, one) == 0


def test_resident_loader_refuses_an_unknown_augment_mode(pkg, synth):
    pk = pkg.packing.pack_frames([synth.synth_frame(1, "crop")])
    ds = pkg.MSRADepthDataset.from_packs([pk])
    for bad in ("bogus", "Device", ""):
        with pytest.raises(ValueError):
            pkg.ResidentLoader(ds, batch_size=1, device="cpu", augment=bad)
    for ok in (False, True, "device"):
        ld = pkg.ResidentLoader(ds, batch_size=1, device="cpu", augment=ok)   # (nothing touches a device before iteration)
        assert ld.augment is bool(ok) and ld.device_draws is (ok == "device")
