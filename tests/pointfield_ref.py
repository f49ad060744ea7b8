"""The numpy restatement of include/tsdf_pointfield.h: what the offset-field tests compare the GPU with, bit for bit.
Distances are float32, heat, vectors and the vote float64; numpy rounds every binary operation of arrays of one type on
its own in that type and never fuses a product into a sum, so each expression below is one operation of the contract.
Nothing here touches a GPU or the library.  Fields are float32[n, 4J, P] (layout "cp") throughout; ``to_layout``
and ``narrow`` / ``widen`` are the other layout and the 2-byte element types."""
from typing import NamedTuple

import numpy as np

from group_ref import candidates, huge_cloud, random_clouds, tie_clouds  # noqa: F401  (the input builders are group_ref's, not copies)

OK, DEGENERATE = 0, 1
MAX_CLOUD, MAX_K, MAX_VOTES, MAX_JOINTS = 12288, 12288, 128, 65536   # the TSDF_POINTFIELD_MAX_* of the header
JOINTS_PER_GROUP = 4                          # kPfJoints of csrc/pointfield_host.inc; the tests check it against the plan
ENCODE_MISTAKES = ("ties_high", "ball_only", "knn_only", "float32_heat", "vector_from_joint")
DECODE_MISTAKES = ("ties_high", "sequential_sum", "nan_wins", "no_clamp")
MISTAKES = ENCODE_MISTAKES + DECODE_MISTAKES[1:]
LANE = np.arange(64)


class Field(NamedTuple):
    field: np.ndarray    # float32[n,4J,P]
    valid: np.ndarray    # int32[n,J]
    status: np.ndarray   # int32[n]


class Joints(NamedTuple):
    joints: np.ndarray   # float32[n,J,3]
    weight: np.ndarray   # float32[n,J]
    status: np.ndarray   # int32[n]


def bits(a):
    """The bit patterns of a float32 / float16 array (a uint16 array of bfloat16 patterns is returned as it is)."""
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint16 else a.view({4: np.int32, 2: np.int16}[a.dtype.itemsize])


def lds_bytes(P):
    """pointfield_host.inc::pf_plan's LDS bytes, restated."""
    return 12 * ((P + 63) // 64 * 64) + 16


def narrow(field, dtype):
    """float32 -> ``dtype`` ("float32", "float16", "bfloat16") by round-to-nearest-even; bfloat16 as uint16 patterns."""
    field = np.asarray(field, np.float32)
    if dtype == "float32":
        return field
    if dtype == "float16":
        with np.errstate(all="ignore"):
            return field.astype(np.float16)
    assert dtype == "bfloat16"
    u = field.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(field)
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def widen(a, dtype):
    """The exact float32 of a field of ``dtype`` (bfloat16: uint16 patterns)."""
    if dtype == "bfloat16":
        return (np.asarray(a, np.uint16).astype(np.uint32) << 16).view(np.float32)
    return np.asarray(a).astype(np.float32)


def to_layout(field, layout):
    return field if layout == "cp" else np.ascontiguousarray(np.swapaxes(field, 1, 2))


def distances(p, q):
    """``(dx, dy, dz, dist2)`` float32[m] of joint ``q`` float32[3] from candidates ``p`` float32[m,3]."""
    with np.errstate(all="ignore"):
        dx, dy, dz = q[0] - p[:, 0], q[1] - p[:, 1], q[2] - p[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return dx, dy, dz, d2


def members(p, rank, q, K, radius, mistake=None):
    """The rule for one joint: ``(member bool[m], heat float32[m], vec float32[m,3])`` over the candidates."""
    dx, dy, dz, d2 = distances(p, q)
    m = len(p)
    order = np.lexsort((-rank if mistake == "ties_high" else rank, d2.view(np.uint32)))   # key = dist2 bits << 32 | rank
    near = np.zeros(m, bool)
    near[order[:m if mistake == "ball_only" else min(K, m)]] = True
    with np.errstate(all="ignore"):
        d = np.sqrt(d2.astype(np.float64))
        inside = np.isfinite(d) if mistake == "knn_only" else d <= np.float64(radius)
        if mistake == "float32_heat":
            heat = np.float32(1) - np.sqrt(d2) / np.float32(radius)
        else:
            heat = (1.0 - d / np.float64(radius)).astype(np.float32)
        off = np.stack([dx, dy, dz], 1).astype(np.float64)
        if mistake == "vector_from_joint":
            off = -off
        vec = np.where((d2 == 0)[:, None], 0.0, off / np.where(d2 == 0, 1.0, d)[:, None]).astype(np.float32)
    return near & inside, heat, vec


def encode(clouds, joints, K, radius, status_in=None, mistake=None):
    """A whole call of tsdf_pointfield_encode_hip on clouds float32[n,P,3] and joints float32[n,J,3]: float32, "cp"."""
    assert mistake is None or mistake in ENCODE_MISTAKES
    clouds, joints = np.asarray(clouds, np.float32), np.asarray(joints, np.float32)
    n, P, J = len(clouds), clouds.shape[1], joints.shape[1]
    out = Field(np.zeros((n, 4 * J, P), np.float32), np.zeros((n, J), np.int32), np.zeros(n, np.int32))
    for i in range(n):
        if status_in is not None and status_in[i] != 0:
            out.status[i] = status_in[i]                      # not read: copied through, zeros
            continue
        p, rank = candidates(clouds[i])
        if len(p) == 0:
            out.status[i] = DEGENERATE
            continue
        for j, q in enumerate(joints[i]):
            if not np.isfinite(q).all():
                continue
            out.valid[i, j] = 1
            mem, heat, vec = members(p, rank, q, K, radius, mistake)
            out.field[i, j, rank[mem]] = heat[mem]
            for a in range(3):
                out.field[i, J + 3 * j + a, rank[mem]] = vec[mem, a]
    return out


def heat_keys(h, mistake=None):
    """uint32 keys of float32 heats whose ascending order is the selection's: the greatest heat first, -0 below +0, a NaN
    behind every number."""
    u = np.ascontiguousarray(h, np.float32).view(np.uint32)
    image = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(h), np.uint32(0 if mistake == "nan_wins" else 0xFFFFFFFE), ~image).astype(np.uint32)


def tree(values, lanes, mistake=None):
    """The tree sum of ``values`` float64[k] whose compact indices ascend and lie in ``lanes`` (c % 64)."""
    if mistake == "sequential_sum":
        acc = np.float64(0.0)
        for v in values:
            acc = acc + v
        return acc
    v = np.zeros(64)
    for x, lane in zip(values, lanes):
        v[lane] = v[lane] + x
    for s in (1, 2, 4, 8, 16, 32):
        v = v + v[LANE ^ s]
    assert (v == v[0]).all() or np.isnan(v).any()
    return v[0]


def vote(p, h, v, M, radius, mistake=None):
    """One joint: candidates ``p`` float32[m,3], their heats float32[m] and vectors float32[m,3] -> (joint float32[3], weight)."""
    m = len(p)
    c = np.arange(m)
    order = np.lexsort((-c if mistake == "ties_high" else c, heat_keys(h, mistake)))
    sel = np.sort(order[:min(M, m)])
    with np.errstate(all="ignore"):
        hd = h[sel].astype(np.float64)
        w = hd if mistake == "no_clamp" else np.where(hd < 0.0, 0.0, np.where(hd > 1.0, 1.0, hd))
        w = np.where(np.isnan(hd), 0.0, w)
        vd = v[sel].astype(np.float64)
        nv = np.sqrt((vd[:, 0] * vd[:, 0] + vd[:, 1] * vd[:, 1]) + vd[:, 2] * vd[:, 2])
        ok = (nv > 0.0) & (nv < np.inf)
        u = np.where(ok[:, None], vd / np.where(ok, nv, 1.0)[:, None], 0.0)
        reach = np.float64(radius) * (1.0 - w)
        e = p[sel].astype(np.float64) + reach[:, None] * u
        W = tree(w, sel % 64, mistake)
        S = [tree(w * e[:, a], sel % 64, mistake) for a in range(3)]
        if not W != 0.0:
            return np.zeros(3, np.float32), np.float32(0)
        return np.array([s / W for s in S]).astype(np.float32), np.float32(W)


def decode(clouds, field, M, radius, status_in=None, mistake=None):
    """A whole call of tsdf_pointfield_decode_hip on clouds float32[n,P,3] and a field float32[n,4J,P] ("cp", widened)."""
    assert mistake is None or mistake in DECODE_MISTAKES
    clouds, field = np.asarray(clouds, np.float32), np.asarray(field, np.float32)
    n, J = len(clouds), field.shape[1] // 4
    out = Joints(np.zeros((n, J, 3), np.float32), np.zeros((n, J), np.float32), np.zeros(n, np.int32))
    for i in range(n):
        if status_in is not None and status_in[i] != 0:
            out.status[i] = status_in[i]
            continue
        p, rank = candidates(clouds[i])
        if len(p) == 0:
            out.status[i] = DEGENERATE
            continue
        for j in range(J):
            out.joints[i, j], out.weight[i, j] = vote(p, field[i][j][rank], field[i][J + 3 * j:J + 3 * j + 3][:, rank].T, M, radius,
                                                      mistake)
    return out


def same_field(got, want, dtype="float32", layout="cp"):
    """None if every output of an encode is ``want``'s bit for bit (``want`` float32 "cp", narrowed and laid out here)."""
    if not np.array_equal(np.asarray(got.status), want.status):
        return "status"
    if not np.array_equal(np.asarray(got.valid), want.valid):
        return "valid"
    if not np.array_equal(bits(got.field), bits(to_layout(narrow(want.field, dtype), layout))):
        return "field"
    return None


def same_joints(got, want):
    if not np.array_equal(np.asarray(got.status), want.status):
        return "status"
    if not np.array_equal(bits(got.joints), bits(want.joints)):
        return "joints"
    if not np.array_equal(bits(got.weight), bits(want.weight)):
        return "weight"
    return None


# ---- the inputs both tiers use -----------------------------------------------------------------------------------

def joints_near(clouds, J, seed=0, spread=10.0):
    """float32[n,J,3]: joints near randomly chosen finite rows of each cloud (the first one exactly ON its row)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(clouds), J, 3), np.float32)
    for i, c in enumerate(clouds):
        rows = np.flatnonzero(np.isfinite(c).all(1) & (np.abs(c) < 1e20).all(1))
        if len(rows) == 0:
            out[i] = rng.normal(0, spread, (J, 3))
            continue
        pick = rng.choice(rows, J)
        out[i] = c[pick] + rng.normal(0, spread, (J, 3)).astype(np.float32)
        out[i, 0] = c[pick[0]]
    return out


def lattice_group():
    """The tie lattice with duplicate rows and its reverse; joints on lattice points, on cell centres and off the lattice:
    most distances tie, K cuts through the tie classes."""
    clouds = tie_clouds()
    lat = clouds[0]
    joints = np.stack([np.stack([lat[5], (lat[0] + lat[21]) / 2, lat[3] + np.float32(0.25), lat[39]])] * 2).astype(np.float32)
    return clouds, joints


def dense_group(n=2, P=300, J=5, seed=21):
    """Clouds dense enough that far more than K points lie in the ball of every joint."""
    clouds = random_clouds(n, P, seed=seed, scale=8.0)
    return clouds, joints_near(clouds, J, seed=seed + 1, spread=2.0)


def sparse_group(n=2, P=129, J=5, seed=31):
    """Clouds so sparse that the K-th nearest point of a joint lies outside the ball."""
    clouds = random_clouds(n, P, seed=seed, scale=100.0)
    return clouds, joints_near(clouds, J, seed=seed + 1, spread=5.0)


def edge_group():
    """float32[5, 8, 3] and joints [5, 3, 3], radius 4: a point at exactly d == radius and one on the joint; 1e30 rows (an
    infinite dist2); NaN rows and a NaN joint; a cloud without a candidate; a single candidate."""
    c = np.zeros((5, 8, 3), np.float32)
    j = np.zeros((5, 3, 3), np.float32)
    c[0] = [[4, 0, 0], [0, 0, 0], [0, 4, 0], [1, 1, 1], [3, 0, 0], [0, 0, 5], [2, 2, 2], [-4, 0, 0]]
    j[0] = [[0, 0, 0], [1, 1, 1], [10, 10, 10]]
    c[1] = c[0]
    c[1, 2], c[1, 5] = 1e30, [-2e30, 1e30, 3e30]
    j[1] = [[0, 0, 0], [1e30, 1e30, 1e30], [3, 0, 0]]
    c[2] = c[0]
    c[2, 0, 1], c[2, 3], c[2, 6, 2] = np.nan, np.nan, np.inf
    j[2] = [[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]]
    c[3] = np.nan
    j[3] = [[0, 0, 0], [1, 1, 1], [2, 2, 2]]
    c[4] = np.nan
    c[4, 6] = [1, 2, 3]
    j[4] = [[1, 2, 3], [1, 2, 5], [1, 2, 8]]
    return c, j


def perturbed(field, seed=0, quantum=0.125):
    """A "prediction" float32[n,4J,P] from an encoder's field: heats replaced by random values quantised to ``quantum``
    (many ties; None: not quantised) with NaN, negative, > 1 and infinite entries; vectors noised, some zeroed, some NaN."""
    rng = np.random.default_rng(seed)
    f = np.array(field, np.float32)
    n, C, P = f.shape
    J = C // 4
    heat = rng.uniform(-0.3, 1.3, (n, J, P))
    heat = (heat if quantum is None else np.round(heat / quantum) * quantum).astype(np.float32)
    kind = rng.integers(0, 40, (n, J, P))
    heat[kind == 0] = np.nan
    heat[kind == 1] = np.inf
    heat[kind == 2] = -np.inf
    heat[kind == 3] = -0.0
    f[:, :J] = heat
    vec = f[:, J:] + rng.normal(0, 0.3, (n, 3 * J, P)).astype(np.float32)
    vkind = np.repeat(rng.integers(0, 30, (n, J, P)), 3, axis=1)
    vec[vkind == 0] = 0.0
    vec[vkind == 1] = np.nan
    vec[vkind == 2] = np.inf
    f[:, J:] = vec
    return f


def huge_group():
    """A cloud of 1e30-sized rows: every dist2 is +inf but for a joint exactly on a row."""
    clouds = huge_cloud(70)
    joints = joints_near(clouds, 3, seed=41)
    joints[0, 0], joints[0, 1] = clouds[0, 3], clouds[0, 69]
    return clouds, joints


def _cancel_perm(half):
    return np.random.default_rng(7).permutation(half)


def cancel_group(n=2, P=192, J=2, seed=51):
    """Clouds of pairs p, -p of 1e5-sized rows (the negatives shuffled): a vote over many of them cancels down to the
    rounding errors of its sums, so the ORDER of the tree sum decides the result's bits."""
    rng = np.random.default_rng(seed)
    half = rng.normal(0, 1e5, (n, P // 2, 3)).astype(np.float32)
    clouds = np.concatenate([half, -half[:, _cancel_perm(P // 2)]], 1)
    return clouds, joints_near(clouds, J, seed=seed + 1, spread=1e4)


def groups():
    """name -> (clouds, joints, K, radius, M): the input groups of both tiers."""
    return {"lattice": lattice_group() + (3, 12.0, 5), "dense": dense_group() + (16, 15.0, 25),
            "sparse": sparse_group() + (64, 60.0, 64), "edges": edge_group() + (5, 4.0, 3),
            "huge": huge_group() + (10, 1e30, 5), "cancel": cancel_group() + (8, 1e5, 128)}


def prediction(name, field, seed=1):
    """The "predicted" field the decoder is tried on next to the encoder's own: :func:`perturbed`, but for the group
    "cancel", where the rows of p and -p get the same random heat and zero vectors, so that the vote is 0 but for
    the rounding errors of its sums."""
    if name != "cancel":
        return perturbed(field, seed)
    f = np.zeros_like(field)
    n, C, P = f.shape
    heat = np.random.default_rng(seed).uniform(0.01, 1.0, (n, C // 4, P // 2)).astype(np.float32)
    f[:, :C // 4] = np.concatenate([heat, heat[:, :, _cancel_perm(P // 2)]], 2)
    return f
