"""Numpy restatement of tsdf_point_clouds_hip (include/tsdf.h, "Point clouds") for the tests: valid pixels d != 0 in
row-major order, float64 back-projection one operation at a time, the splitmix64 draw with Python integers, and the
forward map grouped (A_i0 x + A_i1 y) + (A_i2 z + b_i).  numpy's elementwise float64 operations round once each."""
import numpy as np

M64 = (1 << 64) - 1
FOCAL = 241.42


def mix(z: int) -> int:
    """splitmix64, every operation mod 2^64."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix_np(z: np.ndarray) -> np.ndarray:
    """splitmix64 on uint64 arrays (numpy's uint64 arithmetic wraps mod 2^64)."""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draws_slow(seed: int, g: int, m: int, P: int) -> np.ndarray:
    """k(j) = ((u >> 32) * m) >> 32, u = mix(mix(seed + g) + j), for j = 0..P-1, with Python integers (int64)."""
    h = mix((seed + g) & M64)
    return np.array([(((mix((h + j) & M64) >> 32) * m) >> 32) for j in range(P)], np.int64)


def draws(seed: int, g: int, m: int, P: int) -> np.ndarray:
    """draws_slow vectorised (m < 2^32, so the product fits 64 bits)."""
    assert 0 < m < 1 << 32
    h = np.uint64(mix((seed + g) & M64))
    with np.errstate(over="ignore"):
        u = mix_np(h + np.arange(P, dtype=np.uint64)) >> np.uint64(32)
        return ((u * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def indices(m: int, P: int, seed: int, g: int) -> np.ndarray:
    """The valid-pixel rank of every slot (set_length's rule): j for j < m when m < P, else the draw."""
    idx = draws(seed, g, m, P)
    if m < P:
        idx[:m] = np.arange(m)
    return idx


def frame_points(header, depth, focal: float = FOCAL) -> np.ndarray:
    """Every valid pixel of one crop, back-projected: float64[m, 3] in row-major order."""
    W, H, left, top, right, bottom = (int(v) for v in header)
    bw, bh = right - left, bottom - top
    d = np.asarray(depth, np.float32).reshape(bh, bw)
    r, c = np.nonzero(d != 0)          # NaN != 0: valid
    dv = d[r, c].astype(np.float64)
    x = (((c.astype(np.float64) + float(left)) - W / 2) * dv) / focal
    y = (-(((r.astype(np.float64) + float(top)) - H / 2) * dv)) / focal
    z = (-d[r, c]).astype(np.float64)
    return np.stack([x, y, z], axis=1)


def map_points(pts: np.ndarray, xform) -> np.ndarray:
    f = np.asarray(xform, np.float64).reshape(24)[:12].reshape(3, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([(f[k, 0] * x + f[k, 1] * y) + (f[k, 2] * z + f[k, 3]) for k in range(3)], axis=1)


def header_ok(header, off0: int, off1: int, depth_len: int) -> bool:
    """The voxelizer's header rule."""
    _, _, left, top, right, bottom = (int(v) for v in header)
    bw, bh = right - left, bottom - top
    return 0 < bw <= 0x7fffffff and 0 < bh <= 0x7fffffff and bw * bh == off1 - off0 and off0 >= 0 and off1 <= depth_len


def point_clouds(depth, offsets, headers, P: int, seed: int = 0, frame_base: int = 0, xforms=None, focal: float = FOCAL):
    """(points float64[n,P,3], count int32[n], status int32[n]) as the kernel computes them."""
    depth = np.asarray(depth, np.float32)
    offsets = np.asarray(offsets, np.int64)
    headers = np.asarray(headers, np.int32).reshape(-1, 6)
    n = headers.shape[0]
    out = np.zeros((n, P, 3), np.float64)
    count = np.zeros(n, np.int32)
    status = np.zeros(n, np.int32)
    for i in range(n):
        o0, o1 = int(offsets[i]), int(offsets[i + 1])
        if not header_ok(headers[i], o0, o1, depth.size):
            status[i] = 2
            continue
        pts = frame_points(headers[i], depth[o0:o1], focal)
        m = pts.shape[0]
        count[i] = min(m, 0x7fffffff)
        if m == 0:
            status[i] = 1
            continue
        if xforms is not None:
            pts = map_points(pts, xforms[i])
        out[i] = pts[indices(m, P, seed, (frame_base + i) & M64)]
    return out, count, status


def same_bits(a, b) -> bool:
    """Equal bit for bit, except that NaN is compared by position only."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))
