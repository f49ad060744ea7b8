"""The numpy restatement of include/tsdf_group.h: what the kNN-grouping and surface-normal tests compare the GPU with, bit
for bit.  The distances are float32 throughout, the normals float64; numpy rounds every binary operation of arrays of one
type on its own in that type and never fuses a product into a sum, so each expression below is one operation of the
contract.  Nothing here touches a GPU or the library."""
from typing import NamedTuple

import numpy as np

from fps_ref import bits, cloud_batch, crops, lattice  # noqa: F401  (the input builders are fps_ref's, not copies)

OK, DEGENERATE = 0, 1
MAX_CLOUD, MAX_K, SWEEPS = 12288, 128, 8      # TSDF_GROUP_MAX_CLOUD, TSDF_GROUP_MAX_K, TSDF_GROUP_SWEEPS
QUERIES_PER_GROUP = 32                        # kGrpQueries of csrc/group_host.inc; the tests check it against the plan
KNN_MISTAKES = ("ties_high", "exclude_self", "float64", "pad_minus_one")
NORMAL_MISTAKES = ("sequential_sum", "no_flip")
MISTAKES = KNN_MISTAKES + NORMAL_MISTAKES
LANE = np.arange(64)


class Knn(NamedTuple):
    index: np.ndarray     # int32[n,C,K]
    dist2: np.ndarray     # float32[n,C,K]
    offsets: np.ndarray   # float32[n,C,K,3]
    status: np.ndarray    # int32[n]


class Normals(NamedTuple):
    normals: np.ndarray     # float32[n,C,3]
    curvature: np.ndarray   # float32[n,C]
    status: np.ndarray      # int32[n]


def lds_bytes(P):
    """group_host.inc::grp_plan's LDS bytes, restated."""
    return 12 * ((P + 63) // 64 * 64) + 16


def candidates(cloud):
    """``(points float32[m,3], rank int64[m])`` of a cloud float32[P,3]: the rows whose three coordinates are finite."""
    p = np.asarray(cloud)
    assert p.dtype == np.float32
    keep = np.isfinite(p).all(1)
    return p[keep], np.flatnonzero(keep)


def select(p, rank, q, K, mistake=None):
    """The rule for one query: ``(sel int64[m'], dist float32[m'], offsets float32[m',3])``, ``sel`` indexing ``p``, in
    ascending key order, m' = min(K, m)."""
    wide = mistake == "float64"
    a, b = (p.astype(np.float64), q.astype(np.float64)) if wide else (p, q)
    with np.errstate(all="ignore"):
        dx, dy, dz = a[:, 0] - b[0], a[:, 1] - b[1], a[:, 2] - b[2]
        d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == a.dtype
    if wide:
        order = np.lexsort((rank, d))
    else:
        order = np.lexsort((-rank if mistake == "ties_high" else rank, d.view(np.uint32)))   # key = dist bits << 32 | rank
    if mistake == "exclude_self" and len(order) > 1 and d[order[0]] == 0:
        order = order[1:]
    sel = order[:K]
    with np.errstate(all="ignore"):
        return sel, d[sel].astype(np.float32), np.stack([dx[sel], dy[sel], dz[sel]], 1).astype(np.float32)


def _queries(cloud, queries, i):
    if queries is None:
        return cloud
    if isinstance(queries, (int, np.integer)):
        assert queries <= len(cloud)
        return cloud[:queries]
    return np.asarray(queries[i], np.float32)


def knn(clouds, K, queries=None, status_in=None, mistake=None):
    """A whole call of tsdf_knn_hip on clouds float32[n,P,3]; ``queries`` None (every row), an int C (rows 0..C-1) or
    float32[n,C,3]."""
    assert mistake is None or mistake in MISTAKES
    clouds = np.asarray(clouds, np.float32)
    n = len(clouds)
    C = len(_queries(clouds[0], queries, 0)) if n else 0
    out = Knn(np.full((n, C, K), -1, np.int32), np.zeros((n, C, K), np.float32), np.zeros((n, C, K, 3), np.float32),
              np.zeros(n, np.int32))
    for i in range(n):
        if status_in is not None and status_in[i] != 0:
            out.status[i] = status_in[i]                      # not read: copied through, "no result" rows
            continue
        p, rank = candidates(clouds[i])
        if len(p) == 0:
            out.status[i] = DEGENERATE
            continue
        for c, q in enumerate(_queries(clouds[i], queries, i)):
            if not np.isfinite(q).all():
                continue                                      # a "no result" row; the status stays 0
            sel, d, off = select(p, rank, q, K, mistake)
            m = len(sel)
            out.index[i, c, :m], out.dist2[i, c, :m], out.offsets[i, c, :m] = rank[sel], d, off
            if mistake != "pad_minus_one":                    # slots m..K-1 repeat slot 0
                out.index[i, c, m:], out.dist2[i, c, m:], out.offsets[i, c, m:] = rank[sel[0]], d[0], off[0]
    return out


def tree(a, mistake=None):
    """The tree sum of the slots' values ``a`` float64[..., m'] (m' <= 128): slot j in lane j % 64, a lane adds its slot j
    and its slot j + 64, a missing slot is +0.0, then v = v + v[lane ^ s] for s = 1 .. 32."""
    if mistake == "sequential_sum":
        return np.cumsum(a, -1)[..., -1]
    slots = np.zeros(a.shape[:-1] + (128,))
    slots[..., :a.shape[-1]] = a
    v = slots[..., :64] + slots[..., 64:]
    for s in (1, 2, 4, 8, 16, 32):
        v = v + v[..., LANE ^ s]
    assert (v == v[..., :1]).all()                            # addition commutes: the same bits in every lane
    return v[..., 0]


def covariance(nb, mistake=None):
    """Neighbours ``nb`` float32[m',3] in slot order -> the six covariance sums (xx, xy, xz, yy, yz, zz), float64."""
    m = np.float64(len(nb))
    p = nb.astype(np.float64)
    mean = tree(p.T, mistake) / m
    e = p - mean
    return np.array([tree(e[:, a] * e[:, b], mistake) / m for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])


def _rot(A, V, p, q, r):
    """tsdf_obb.hip's jacobi_rot, restated for arrays of matrices: one rotation of the pair (p, q), r the third index;
    skipped where the off-diagonal element is exactly 0."""
    apq = A[p][q]
    live = apq != 0.0
    if not live.any():
        return
    with np.errstate(all="ignore"):
        theta = (A[q][q] - A[p][p]) / (2.0 * np.where(live, apq, 1.0))
        th2 = theta * theta
        t = 1.0 / (np.abs(theta) + np.sqrt(th2 + 1.0))
        t = np.where(theta < 0.0, -t, t)
        t2 = t * t
        c = 1.0 / np.sqrt(t2 + 1.0)
        s = t * c
        tp = t * apq
        new = {(p, p): A[p][p] - tp, (q, q): A[q][q] + tp, (p, q): np.zeros_like(apq)}
        rp, rq = A[r][p], A[r][q]
        crp, srq, srp, crq = c * rp, s * rq, s * rp, c * rq
        new[r, p], new[r, q] = crp - srq, srp + crq
        for (i, j), v in new.items():
            A[i][j] = A[j][i] = np.where(live, v, A[i][j])
        for row in range(3):
            a, b = V[row][p], V[row][q]
            ca, sb, sa, cb = c * a, s * b, s * a, c * b
            V[row][p], V[row][q] = np.where(live, ca - sb, a), np.where(live, sa + cb, b)


def jacobi(cov, sweeps=SWEEPS):
    """``cov`` float64[N,6] (xx, xy, xz, yy, yz, zz) -> (diagonal float64[N,3], V float64[N,3,3]) after ``sweeps`` cyclic
    sweeps in pair order (0,1), (0,2), (1,2)."""
    cov = np.asarray(cov, np.float64)
    xx, xy, xz, yy, yz, zz = (cov[:, k].copy() for k in range(6))
    A = [[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]
    one, zero = np.ones_like(xx), np.zeros_like(xx)
    V = [[one, zero, zero], [zero, one, zero], [zero, zero, one]]
    V = [[v.copy() for v in row] for row in V]
    for _ in range(sweeps):
        _rot(A, V, 0, 1, 2)
        _rot(A, V, 0, 2, 1)
        _rot(A, V, 1, 2, 0)
    return np.stack([A[0][0], A[1][1], A[2][2]], 1), np.stack([np.stack(row, 1) for row in V], 1)


def finish(diag, V, q, view, count, mistake=None):
    """The normal and the curvature of N queries from the Jacobi's result: float32[N,3], float32[N]."""
    col1 = diag[:, 1] < diag[:, 0]
    col2 = diag[:, 2] < np.where(col1, diag[:, 1], diag[:, 0])
    col = np.where(col2, 2, np.where(col1, 1, 0))             # the smallest, ties to the lowest column
    nrm = V[np.arange(len(V)), :, col]
    w = view - q.astype(np.float64)
    d = (nrm[:, 0] * w[:, 0] + nrm[:, 1] * w[:, 1]) + nrm[:, 2] * w[:, 2]
    if mistake != "no_flip":
        nrm = np.where((d < 0.0)[:, None], -nrm, nrm)
    lam = np.sort(diag, 1)
    total = (lam[:, 0] + lam[:, 1]) + lam[:, 2]
    with np.errstate(all="ignore"):
        curv = np.where(total == 0.0, 0.0, lam[:, 0] / np.where(total == 0.0, 1.0, total))
    few = np.asarray(count) < 3
    nrm = np.where(few[:, None], 0.0, nrm)
    curv = np.where(few, 0.0, curv)
    return nrm.astype(np.float32), curv.astype(np.float32)


def normals(clouds, K, queries=None, status_in=None, view=None, mistake=None, sweeps=SWEEPS):
    """A whole call of tsdf_normals_hip; ``view`` float64[n,3] or None (the origin)."""
    assert mistake is None or mistake in MISTAKES
    clouds = np.asarray(clouds, np.float32)
    n = len(clouds)
    C = len(_queries(clouds[0], queries, 0)) if n else 0
    out = Normals(np.zeros((n, C, 3), np.float32), np.zeros((n, C), np.float32), np.zeros(n, np.int32))
    for i in range(n):
        if status_in is not None and status_in[i] != 0:
            out.status[i] = status_in[i]
            continue
        p, rank = candidates(clouds[i])
        if len(p) == 0:
            out.status[i] = DEGENERATE
            continue
        qs = _queries(clouds[i], queries, i)
        live = [c for c, q in enumerate(qs) if np.isfinite(q).all()]
        if not live:
            continue
        kmist = mistake if mistake in KNN_MISTAKES else None
        cov = [covariance(p[select(p, rank, qs[c], K, kmist)[0]], mistake) for c in live]
        diag, V = jacobi(np.array(cov), sweeps)
        v = np.zeros(3) if view is None else np.asarray(view[i], np.float64)
        out.normals[i, live], out.curvature[i, live] = finish(diag, V, qs[live], v, np.full(len(live), min(K, len(p))), mistake)
    return out


def same_knn(got, want):
    """None if every field of ``got`` given is ``want``'s bit for bit, else the name of the first that differs."""
    if not np.array_equal(np.asarray(got.status), want.status):
        return "status"
    if not np.array_equal(np.asarray(got.index), want.index):
        return "index"
    if got.dist2 is not None and not np.array_equal(bits(got.dist2), bits(want.dist2)):
        return "dist2"
    if got.offsets is not None and not np.array_equal(bits(got.offsets), bits(want.offsets)):
        return "offsets"
    return None


def same_normals(got, want):
    if not np.array_equal(np.asarray(got.status), want.status):
        return "status"
    if not np.array_equal(bits(got.normals), bits(want.normals)):
        return "normals"
    if got.curvature is not None and not np.array_equal(bits(got.curvature), bits(want.curvature)):
        return "curvature"
    return None


# ---- the inputs both tiers use -----------------------------------------------------------------------------------

def random_clouds(n, P, seed=0, scale=100.0):
    return np.random.default_rng(seed).normal(0, scale, (n, P, 3)).astype(np.float32)


def tie_clouds():
    """float32[2, 40, 3]: the 4 x 4 x 2 lattice plus its first eight rows again (most distances tie, and every tie among
    duplicates must go to the lower row), and the same with the rows reversed."""
    lat = lattice()
    a = np.concatenate([lat, lat[:8]])
    return np.stack([a, a[::-1]]).astype(np.float32)


def cubic_clouds():
    """float32[2, 125, 3]: a 5 x 5 x 5 lattice of an inexact step, and its rows reversed and scaled.  An inner point and
    its six nearest neighbours have an isotropic covariance: the eigenvalues tie, and which direction comes out is
    decided by the last bit of the covariance sums — the inputs that see the ORDER of the tree sum."""
    lat = lattice(5, 5, 5, 0.7)
    return np.stack([lat, lat[::-1] * np.float32(1.7)]).astype(np.float32)


def huge_cloud(P=70):
    """float32[1, P, 3] with coordinates of 1e30: every distance between different points is +inf, the order by rank."""
    rng = np.random.default_rng(5)
    return (rng.choice([-1.0, 1.0], (1, P, 3)) * rng.uniform(1e30, 3e30, (1, P, 3))).astype(np.float32)


def hard_clouds():
    """float32[4, 40, 3]: fps_ref.hard_clouds' positions rounded to float32 — 1e30-sized rows next to ordinary ones, rows
    with a NaN or an infinity, a cloud with no candidate and one with a single candidate."""
    from fps_ref import hard_clouds as wide
    with np.errstate(all="ignore"):
        return wide().astype(np.float32)


def ragged_cloud():
    """float32[1, 5, 3] with two NaN rows: m = 3, below K = 8."""
    c = random_clouds(1, 5, seed=3)
    c[0, 1] = np.nan
    c[0, 3, 2] = np.nan
    return c


def patches(n=4, P=200, seed=9):
    """Smooth surface patches float32[n, P, 3] in front of a camera at the origin (z about -400): a plane, a tilted
    plane, a paraboloid and a sphere cap, each with a little noise off the surface, so that the two smallest eigenvalues
    of a neighbourhood's covariance are well apart."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        u, v = rng.uniform(-60, 60, P), rng.uniform(-60, 60, P)
        w = (0 * u, 0.4 * u - 0.2 * v, (u * u + 0.5 * v * v) / 300.0, np.sqrt(150.0 ** 2 - u * u - v * v) - 150.0)[k % 4]
        w = w + rng.normal(0, 0.05, P)
        out.append(np.stack([u + 10 * k, v - 5 * k, w - 400.0], 1))
    return np.array(out, np.float32)
