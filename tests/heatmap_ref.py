"""The numpy restatement of include/tsdf_heatmap.h, float64 operation for operation: what the heatmap tests compare the
GPU with.  Nothing here touches a GPU or the library."""
import numpy as np

TINY = 2.0 ** -126          # below it a voxel is written as +0 (the flush rule)
LAYOUTS = ("czyx", "cxyz")


def tables(u, R, sigma):
    """g[..., a, i] = exp(-((i - c_a)^2 * k)) for labels ``u[..., 3]`` (columns x, y, z), float64, every operation on its
    own; ``sigma`` is taken as the float32 the entry receives."""
    u = np.asarray(u, np.float32).astype(np.float64)
    s = np.float64(np.float32(sigma))
    k = 1.0 / (2.0 * (s * s))
    c = u * np.float64(R) - 0.5
    t = np.arange(R, dtype=np.float64) - c[..., None]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.exp(-((t * t) * k))


def encode(u, status, R, sigma, layout="czyx"):
    """``(heat float32[n,J,R,R,R], valid int32[n,J])`` of labels ``u`` float32[n,J,3] and ``status`` int32[n] or None."""
    assert layout in LAYOUTS
    u = np.asarray(u, np.float32)
    n, J = u.shape[:2]
    valid = np.isfinite(u).all(axis=2)
    if status is not None:
        valid &= (np.asarray(status) == 0)[:, None]
    g = tables(np.where(valid[..., None], u, np.float32(0)), R, sigma)
    gx, gy, gz = g[:, :, 0], g[:, :, 1], g[:, :, 2]
    heat = np.empty((n, J, R, R, R), np.float32)
    for i in range(n):   # frame by frame: one float64 volume set at a time
        with np.errstate(under="ignore"):
            zy = gz[i][:, :, None] * gy[i][:, None, :]                 # [J, z, y]
            if layout == "czyx":
                p = zy[:, :, :, None] * gx[i][:, None, None, :]        # [J, z, y, x]
            else:
                p = zy.transpose(0, 2, 1)[:, None, :, :] * gx[i][:, :, None, None]   # [J, x, y, z]
        p = np.where(p < TINY, 0.0, p)
        p[~valid[i]] = 0.0
        heat[i] = p.astype(np.float32)
    return heat, valid.astype(np.int32)


def _axes(layout, idx, R):
    """(x, y, z) of a linear index in memory order."""
    slow, mid, fast = idx // (R * R), (idx // R) % R, idx % R
    return (fast, mid, slow) if layout == "czyx" else (slow, mid, fast)


def peaks(heat):
    """``(peak float32[n,J], arg int32[n,J])``: per volume the maximum under ``>`` (a NaN is never it) and the lowest linear
    index that holds it (+0 == -0); NaN and -1 where every value is a NaN.  float32 holds a 2-byte value exactly."""
    heat = np.asarray(heat, np.float32)
    n, J = heat.shape[:2]
    flat = heat.reshape(n * J, -1)
    nans = np.isnan(flat)
    arg = np.where(nans, -np.inf, flat).argmax(axis=1).astype(np.int32)     # the first of equal values
    peak = flat[np.arange(n * J), arg].copy()
    for r in np.flatnonzero(np.isnan(peak) | np.isneginf(peak)):             # index 0 may be a NaN standing in for -inf
        ok = np.flatnonzero(~nans[r])
        arg[r], peak[r] = (ok[0], flat[r, ok[0]]) if len(ok) else (-1, np.nan)
    return peak.reshape(n, J), arg.reshape(n, J)


def decode(heat, R, layout="czyx", radius=0, found=None):
    """``(u float32[n,J,3], peak float32[n,J], arg int32[n,J])`` of ``heat`` [n,J,R,R,R] in float32 (which holds a 2-byte
    value exactly); ``found``: ``peaks(heat)`` if the caller has it (it depends on neither the layout nor the radius)."""
    assert layout in LAYOUTS and 0 <= radius <= 3
    heat = np.asarray(heat, np.float32)
    n, J = heat.shape[:2]
    peak, arg = found if found is not None else peaks(heat)
    u = np.empty((n, J, 3), np.float32)
    for i in range(n):
        for j in range(J):
            a = int(arg[i, j])
            if a < 0:
                u[i, j] = 0.5
                continue
            s, mi, f = a // (R * R), (a // R) % R, a % R
            c = np.array([s, mi, f], np.float64)
            if radius:
                lo = [max(k - radius, 0) for k in (s, mi, f)]
                hi = [min(k + radius, R - 1) + 1 for k in (s, mi, f)]
                w = heat[i, j, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].astype(np.float64)
                w = np.where(w > 0, w, 0.0)            # max(h, 0); a NaN counts as 0
                sw = w.sum()
                if np.isfinite(sw) and sw > 0:
                    grids = np.meshgrid(*[np.arange(lo[k], hi[k], dtype=np.float64) for k in range(3)], indexing="ij")
                    c = np.array([(w * g).sum() / sw for g in grids])
            un = ((c + 0.5) / np.float64(R)).astype(np.float32)    # slow, mid, fast
            u[i, j] = un[::-1] if layout == "czyx" else un
    return u, peak, arg


def plan(nj, R, cus):
    """``(slab, nslab, workgroups)`` of the encode launch: one slab of R slices per (frame, joint) when there are 2 * CUs of
    them or more; otherwise floor(2 * CUs / nj) slabs at most (R at most), of equal size but a shorter last one."""
    want = max(1, min(R, (2 * cus) // nj))
    slab = -(-R // want)
    nslab = -(-R // slab)
    return slab, nslab, nj * nslab


def plan_class(nj, R, cus):
    """"one", "equal" or "ragged": the three shapes a plan takes."""
    slab, nslab, _ = plan(nj, R, cus)
    return "one" if nslab == 1 else "equal" if R % slab == 0 else "ragged"
