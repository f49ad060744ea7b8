"""CPU tier of the draws from device-resident counters (include/tsdf_augstep.h): libtsdf_augstep.so as far as it goes
without a GPU — exports, version, argument checks before device work —, the two frozen libraries beside it, the new
``aug`` / ``graph`` values of the consumers, and the numpy side of the per-frame contract."""
import ctypes

import numpy as np
import pytest
from abi_util import declared_functions, exported

M = 1 << 64


def test_augstep_library_exports_exactly_its_header(pkg):
    want = ["tsdf_aug_draw_at_hip", "tsdf_augstep_version"]
    assert declared_functions("tsdf_augstep.h") == want
    funcs, named = exported(pkg._lib.AUGSTEP_LIB_PATH)
    assert funcs == want and named == want
    S = pkg._lib.load_augstep()
    assert S.tsdf_augstep_version() == 1 == pkg._lib.AUGSTEP_VERSION
    assert pkg._lib.load_augstep() is S
    # the two libraries beside it are what they were
    assert pkg._lib.load().tsdf_version() == 7
    A = pkg._lib.load_augment()
    assert A is not S and A.tsdf_augment_version() == 1
    funcs, named = exported(pkg._lib.AUGMENT_LIB_PATH)
    assert funcs == named == ["tsdf_aug_draw_hip", "tsdf_augment_version"] == declared_functions("tsdf_augment.h")


def test_argument_validation_happens_before_device_work(pkg):
    S = pkg._lib.load_augstep()
    null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(20)
    draw = S.tsdf_aug_draw_at_hip
    # centres, n_src, index, n, state, counters, stream, xforms, stretch, rot
    assert draw(one, 4, null, -1, one, null, null, one, null, null) == -1      # n < 0
    assert draw(null, 4, null, 1, one, null, null, one, null, null) == -1      # no centres
    assert draw(one, 4, null, 1, null, null, null, one, null, null) == -1      # no state
    assert draw(one, 4, null, 1, one, null, null, null, null, null) == -1      # no xforms
    assert draw(one, 0, null, 1, one, null, null, one, null, null) == -1       # n_src < 1
    assert draw(one, -3, one, 1, one, one, null, one, one, one) == -1
    assert draw(one, 4, null, 1, one, null, null, odd, null, null) == -1       # xforms not 8-byte aligned
    assert draw(one, 4, null, 1, odd, null, null, one, null, null) == -1       # state not 8-byte aligned
    assert draw(one, 4, one, 1, odd, one, null, odd, one, one) == -1
    # n == 0 is a no-op, whatever else is passed
    assert draw(null, 0, null, 0, null, null, null, null, null, null) == 0
    assert draw(one, 4, one, 0, odd, one, null, odd, one, one) == 0


def test_consumers_refuse_unknown_modes_before_any_device(pkg, synth):
    pk = pkg.packing.pack_frames([synth.synth_frame(1, "crop")])
    raw = pkg.MSRADepthDataset.from_packs([pk])
    for bad in ("bogus", "Device", "", "host"):
        with pytest.raises(ValueError):
            pkg.MSRA_Dataset.from_raw(raw, device="cpu", aug=bad)
    for ok in (False, True, "device"):
        ds = pkg.MSRA_Dataset.from_raw(raw, device="cpu", aug=ok)   # (nothing touches a device before the first item)
        assert ds.AUG is bool(ok) and ds.aug_device is (ok == "device") and len(ds) == (2 if ok else 1)
    assert pkg.MSRA_Dataset.from_raw(raw, device="cpu", aug="device", aug_seed=9)._aug_key == pkg.augment.device_key(9, 0, 0)
    kw = dict(batch_size=1, device="cpu")
    for bad in ("yes", 1, None, "device"):
        with pytest.raises(ValueError):
            pkg.ResidentLoader(raw, augment="device", graph=bad, **kw)
    for aug in (False, True):          # a graph replays the device-drawn step, nothing else
        with pytest.raises(ValueError):
            pkg.ResidentLoader(raw, augment=aug, graph=True, **kw)
    with pytest.raises(ValueError):
        pkg.ResidentLoader(raw, augment="device", graph=True, prefetch=2, **kw)
    assert pkg.ResidentLoader(raw, augment="device", **kw).graph is False          # the default
    assert pkg.ResidentLoader(raw, augment="device", graph=True, **kw).graph is True
    for aug in (False, True, "device"):
        assert pkg.ResidentLoader(raw, augment=aug, graph=False, **kw).device_draws is (aug == "device")


def test_a_frame_draws_the_same_in_every_batch(pkg):
    """The numpy side of MSRA_Dataset(aug="device"): frame g's draw is device_draws_np(key, [g]) wherever g stands."""
    aug = pkg.augment
    key = aug.device_key(3, 0, 0)
    n = 500
    whole = aug.device_draws_np(key, np.arange(n))
    rng = np.random.default_rng(1)
    for batch in (rng.permutation(n)[:16], np.array([7, 7, 499, 0, 7]), np.array([499])):
        got = aug.device_draws_np(key, batch)
        for u, v in zip(got, whole):
            assert np.array_equal(u, v[batch])
    # counter0 + counters mod 2^64, negative int64 counters included (what tsdf_aug_draw_at_hip computes)
    c0 = M - 3
    cnt = np.array([-5, 0, 2, 3, 4], np.int64)
    a = aug.device_draws_np(key, [(c0 + int(c)) % M for c in cnt])
    b = aug.device_draws_np(key, [M - 8, M - 3, M - 1, 0, 1])
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
