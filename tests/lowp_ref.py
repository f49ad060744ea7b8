"""The tests' own restatement of the narrowing of include/tsdf_lowp.h, and the float32 values it is tested on.

Round-to-nearest-even from float32: for float16 it is numpy's ``astype(np.float16)`` (IEEE conversion, subnormals
produced), for bfloat16 the integer formula on the float32 bits — add 0x7fff plus the bit that will become the last one
kept, then drop the low half.  Both are checked against torch's CPU casts in tests/test_lowp_cpu.py; the GPU tier then
compares the library's output with the same casts done on the device."""
import numpy as np

KINDS = ("f16", "bf16")


def narrow_bits(x, kind):
    """float32 array -> the uint16 bit patterns of its round-to-nearest-even narrowing (finite values and infinities)."""
    x = np.ascontiguousarray(x, np.float32)
    if kind == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen(bits, kind):
    """uint16 patterns -> their float32 values (exact)."""
    bits = np.ascontiguousarray(bits, np.uint16)
    if kind == "f16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def finite_patterns(kind):
    """Every finite 2-byte pattern of the type, both signs (float16: 2 x 31744, bfloat16: 2 x 32640)."""
    top = 0x7c00 if kind == "f16" else 0x7f80
    mag = np.arange(top, dtype=np.uint16)
    return np.concatenate([mag, mag | 0x8000]).astype(np.uint16)


def neighbourhoods(kind):
    """Five float32 values around every finite pattern v of the type: v itself, one float32 ulp beyond it (away from
    zero), the midpoint between v and the next pattern of larger magnitude (a tie: it must go to the even pattern; beyond
    the largest finite value the "next pattern" is the power of two that follows, and the tie goes to infinity), and one
    float32 ulp either side of that midpoint.  float16 subnormals, +-0 and +-1 are among the patterns.
    Returns float32[5 * patterns], all finite."""
    p = finite_patterns(kind)
    v = widen(p, kind)
    if kind == "bf16":
        mid = ((p.astype(np.uint32) << 16) | 0x8000).view(np.float32)     # one more bit than the type keeps
    else:
        mag = p & 0x7fff
        nxt = np.where(mag == 0x7bff, np.float32(65536.0), widen(np.minimum(mag + 1, 0x7bff).astype(np.uint16), kind))
        nxt = np.copysign(nxt, v).astype(np.float32)
        mid = ((v.astype(np.float64) + nxt.astype(np.float64)) / 2).astype(np.float32)   # exact in float32
        assert np.array_equal(mid.astype(np.float64), (v.astype(np.float64) + nxt.astype(np.float64)) / 2)
    away = np.copysign(np.float32(np.inf), v).astype(np.float32)
    out = np.concatenate([v, np.nextafter(v, away), np.nextafter(mid, -away), mid, np.nextafter(mid, away)])
    assert out.dtype == np.float32 and np.isfinite(out).all()
    return out
