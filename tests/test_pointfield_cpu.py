"""CPU tier of the point-wise offset fields (include/tsdf_pointfield.h): the properties of the numpy restatement the GPU
tier compares with (tests/pointfield_ref.py) on that tier's own inputs — the member set against group_ref's kNN and the
ball, the heat's range and order, unit vectors, the pure ball rule, the round trip through the decoder, both layouts'
channel order, and that each deliberate mistake is seen —, and libtsdf_pointfield.so as far as it goes without a GPU: the
loader's row against header and binary, every argument refusal before device work, the plan, the build rule and the
resource report, the host-only code under the CPU sanitizers as a child process, the public names and refusals with
launches stubbed, and AugmentedStep(fields=) through stubbed primitives."""
import ctypes
import importlib
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_ref as gr  # noqa: E402
import pointfield_ref as pr  # noqa: E402
from abi_util import declared_functions, exported  # noqa: E402

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "handposeestimation-with-3d-cnns_amd"
CSRC = os.path.join(ROOT, PKG, "csrc")
INVALID, NO_DEVICE = -1, -2
WANT = ["tsdf_pointfield_decode_hip", "tsdf_pointfield_encode_hip", "tsdf_pointfield_plan", "tsdf_pointfield_version"]


# ---- the reference, on the inputs of the GPU tier ----
@pytest.fixture(scope="module")
def groups():
    return pr.groups()


@pytest.fixture(scope="module")
def refs(groups):
    """name -> (the encoder's field, the decoder's answer to it, the "predicted" field, the decoder's answer to that)."""
    out = {}
    for name, (c, j, K, radius, M) in groups.items():
        enc = pr.encode(c, j, K, radius)
        pred = pr.prediction(name, enc.field)
        out[name] = (enc, pr.decode(c, enc.field, M, radius), pred, pr.decode(c, pred, M, radius))
    return out


def test_members_are_the_knn_neighbours_inside_the_ball_with_ordered_heat_and_unit_vectors(groups, refs):
    for name, (clouds, joints, K, radius, _) in groups.items():
        field = refs[name][0].field
        J, P = joints.shape[1], clouds.shape[1]
        knn = gr.knn(clouds, min(K, gr.MAX_K), queries=joints)          # the seventeenth library's rule, restated there
        for i in range(len(clouds)):
            m = len(gr.candidates(clouds[i])[0])
            for j in range(J):
                heat, vec = field[i, j], field[i, J + 3 * j:J + 3 * j + 3]
                got = np.flatnonzero((heat != 0) | (vec != 0).any(0))
                if knn.index[i, j, 0] < 0:                                # a "no result" row there: a zero field here
                    assert got.size == 0 and not refs[name][0].valid[i, j], (name, i, j)
                    continue
                idx, d2 = knn.index[i, j, :min(K, m)], knn.dist2[i, j, :min(K, m)]
                with np.errstate(all="ignore"):
                    inside = np.sqrt(d2.astype(np.float64)) <= radius
                assert np.array_equal(got, np.sort(idx[inside])), (name, i, j)
                along = heat[idx]                                          # nearest first
                assert (along >= 0).all() and (along <= 1).all() and (np.diff(along) <= 0).all(), (name, i, j)
                norm = np.linalg.norm(vec[:, got].astype(np.float64), axis=0)
                assert ((np.abs(norm - 1) <= 2.0 ** -23) | (norm == 0)).all(), (name, i, j)
                assert ((norm == 0) == (heat[got] == 1)).all()            # a zero vector only ON the joint
        assert not np.isnan(field).any() and not (pr.bits(field) == np.int32(-2 ** 31)).any(), name   # every other cell is +0


def test_k_at_or_above_m_is_the_pure_ball_rule(groups):
    for name, (clouds, joints, K, radius, _) in groups.items():
        ball = pr.encode(clouds, joints, K, radius, mistake="ball_only")
        for big in (clouds.shape[1], clouds.shape[1] + 1, pr.MAX_K):
            assert pr.same_field(pr.encode(clouds, joints, big, radius), ball) is None, (name, big)


def test_round_trip_returns_each_joint_that_has_a_voting_member(groups, refs):
    """decode(encode(cloud, joints)): every vote of positive weight points at the joint, so the result is the joint up to
    the three roundings of heat, vector and output, each at most 2^-24 relative: within radius * 2^-20 plus one float32 ulp
    of the coordinate.  The worst ratio to that bound, measured here, is printed."""
    worst, worst_r = 0.0, 0.0
    for name, (clouds, joints, K, radius, M) in groups.items():
        enc, back = refs[name][0], refs[name][1]
        J = joints.shape[1]
        voting = (enc.field[:, :J] > 0).any(2)
        assert np.array_equal(voting, back.weight > 0), name
        assert not back.joints[~voting].any() and (enc.valid[voting] == 1).all()
        err = np.abs(back.joints.astype(np.float64) - joints.astype(np.float64))[voting]
        bound = radius * 2.0 ** -20 + np.spacing(np.abs(joints))[voting].astype(np.float64)
        if err.size:
            worst = max(worst, float((err / bound).max()))
            worst_r = max(worst_r, float(err.max() / (radius * 2.0 ** -24)))
            assert (err <= bound).all(), (name, float((err / bound).max()))
    print(f"round trip: worst |decode(encode(j)) - j| is {worst:.3f} of (radius * 2^-20 + ulp), {worst_r:.3f} of radius * 2^-24")
    assert worst > 0


SEEN = {   # (group, side, mistake) -> positions an output of which the mistake changes: the table of DESIGN.md
    ('lattice', 'encode', 'ties_high'): 2, ('lattice', 'encode', 'ball_only'): 2,
    ('lattice', 'encode', 'float32_heat'): 2, ('lattice', 'encode', 'vector_from_joint'): 2,
    ('lattice', 'decode', 'ties_high'): 2, ('lattice', 'decode', 'nan_wins'): 2, ('lattice', 'decode', 'no_clamp'): 2,
    ('dense', 'encode', 'ball_only'): 2, ('dense', 'encode', 'knn_only'): 1, ('dense', 'encode', 'float32_heat'): 2,
    ('dense', 'encode', 'vector_from_joint'): 2, ('dense', 'decode', 'ties_high'): 2,
    ('dense', 'decode', 'nan_wins'): 2, ('dense', 'decode', 'no_clamp'): 2, ('sparse', 'encode', 'knn_only'): 2,
    ('sparse', 'encode', 'float32_heat'): 2, ('sparse', 'encode', 'vector_from_joint'): 2,
    ('sparse', 'decode', 'ties_high'): 2, ('sparse', 'decode', 'nan_wins'): 2, ('sparse', 'decode', 'no_clamp'): 2,
    ('edges', 'encode', 'ties_high'): 2, ('edges', 'encode', 'ball_only'): 2, ('edges', 'encode', 'knn_only'): 3,
    ('edges', 'encode', 'float32_heat'): 2, ('edges', 'encode', 'vector_from_joint'): 4,
    ('edges', 'decode', 'no_clamp'): 4, ('huge', 'decode', 'ties_high'): 1, ('huge', 'decode', 'nan_wins'): 1,
    ('huge', 'decode', 'no_clamp'): 1, ('cancel', 'encode', 'ball_only'): 2, ('cancel', 'encode', 'knn_only'): 1,
    ('cancel', 'encode', 'float32_heat'): 2, ('cancel', 'encode', 'vector_from_joint'): 2,
    ('cancel', 'decode', 'sequential_sum'): 2,
}


def test_each_mistake_changes_an_output(groups, refs):
    seen = {}
    for name, (clouds, joints, K, radius, M) in groups.items():
        enc, back, pred, back_pred = refs[name]
        n = len(clouds)
        for mistake in pr.ENCODE_MISTAKES:
            bad = pr.encode(clouds, joints, K, radius, mistake=mistake)
            seen[name, "encode", mistake] = sum(
                pr.same_field(pr.Field(*[f[i:i + 1] for f in bad]), pr.Field(*[f[i:i + 1] for f in enc])) is not None for i in range(n))
        for mistake in pr.DECODE_MISTAKES:
            rows = 0
            for field, good in ((enc.field, back), (pred, back_pred)):
                bad = pr.decode(clouds, field, M, radius, mistake=mistake)
                rows = max(rows, sum(pr.same_joints(pr.Joints(*[f[i:i + 1] for f in bad]), pr.Joints(*[f[i:i + 1] for f in good]))
                                     is not None for i in range(n)))
            seen[name, "decode", mistake] = rows
    for (name, side, mistake), rows in seen.items():
        print(f"{name:8s} {side} {mistake:18s} changes {rows} of {len(groups[name][0])} positions")
    for side, mistakes in (("encode", pr.ENCODE_MISTAKES), ("decode", pr.DECODE_MISTAKES)):
        for mistake in mistakes:
            assert any(seen[name, side, mistake] for name in groups), (side, mistake)
    # random clouds do NOT show these two: the lattice, the duplicates and the dense cloud do
    assert not seen["sparse", "encode", "ties_high"] and not seen["sparse", "encode", "ball_only"]
    assert seen["lattice", "encode", "ties_high"] and seen["dense", "encode", "ball_only"] and seen["cancel", "decode", "sequential_sum"]
    assert {k: v for k, v in seen.items() if v} == SEEN


def test_both_layouts_channel_order_and_the_narrowed_types(groups, refs):
    clouds, joints, K, radius, _ = groups["dense"]
    field = refs["dense"][0].field
    n, J, P = len(clouds), joints.shape[1], clouds.shape[1]
    pc = pr.to_layout(field, "pc")
    assert field.shape == (n, 4 * J, P) and pc.shape == (n, P, 4 * J) and pc.flags["C_CONTIGUOUS"]
    for j in range(J):
        assert np.array_equal(pc[:, :, j], field[:, j])                                  # channel j: joint j's heat
        for a in range(3):
            assert np.array_equal(pc[:, :, J + 3 * j + a], field[:, J + 3 * j + a])     # J + 3j + a: component a
    i, j = 0, 1
    row = int(np.argmax(field[i, j]))
    p, q = clouds[i, row].astype(np.float64), joints[i, j].astype(np.float64)
    assert np.allclose(field[i, J + 3 * j:J + 3 * j + 3, row], (q - p) / np.linalg.norm(q - p), atol=1e-6)   # TOWARDS the joint
    assert np.isclose(field[i, j, row], 1 - np.linalg.norm(q - p) / radius, atol=1e-6)
    # the 2-byte types: round-to-nearest-even, widened exactly
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 6e-8, 0.0], np.float32)
    assert pr.narrow(x, "bfloat16").tolist() == [0x3F80, 0x3F80, 0x3F82, 0x3F80, 0x3F80, 0x3381, 0]
    assert pr.narrow(x, "float16").view(np.uint16).tolist() == [0x3C00, 0x3C04, 0x3C0C, 0x3C00, 0x3C02, 1, 0]
    for dtype in ("float16", "bfloat16"):
        back = pr.widen(pr.narrow(field, dtype), dtype)
        assert back.dtype == np.float32 and np.abs(back - field).max() <= 2.0 ** -8 and np.array_equal(pr.narrow(back, dtype), pr.narrow(field, dtype))
    assert torch.equal(torch.from_numpy(field).bfloat16().view(torch.int16), torch.from_numpy(pr.narrow(field, "bfloat16").view(np.int16)))
    assert torch.equal(torch.from_numpy(field).half(), torch.from_numpy(pr.narrow(field, "float16")))


def test_heat_keys_order_numbers_then_nan():
    h = np.array([np.inf, 2.0, 1.0, 0.5, 0.0, -0.0, -1.0, -np.inf, np.nan], np.float32)
    keys = pr.heat_keys(h)
    assert (np.diff(keys.astype(np.int64)) > 0).all() and keys[-1] == 0xFFFFFFFE and keys[0] == 0x007FFFFF
    assert pr.heat_keys(h, "nan_wins")[-1] == 0


# ---- library pins ----
def test_row_binds_exactly_its_header_with_types(pkg):
    lib = pkg._lib
    ext = lib._POINTFIELD
    assert isinstance(ext, lib._Ext) and "pointfield" not in lib._EXTS and len(lib._EXTS) == 11
    assert declared_functions("tsdf_pointfield.h") == WANT == sorted([ext.version_symbol, *ext.entries])
    funcs, named = exported(lib.POINTFIELD_LIB_PATH)
    assert funcs == WANT and named == WANT
    assert ext.path == lib.POINTFIELD_LIB_PATH and ext.version == lib.POINTFIELD_VERSION == 1
    L = lib.load_pointfield()
    assert L.tsdf_pointfield_version() == 1
    vp, i, i64, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    ip = ctypes.POINTER(ctypes.c_int)
    assert list(L.tsdf_pointfield_plan.argtypes) == [i, i, i, ip, ip, ip]
    assert list(L.tsdf_pointfield_encode_hip.argtypes) == [vp, i64, vp, vp, i, i, i, i, dbl, i, i, vp, vp, vp, vp]
    assert list(L.tsdf_pointfield_decode_hip.argtypes) == [vp, i64, vp, vp, i, i, i, i, dbl, i, i, vp, vp, vp, vp]
    for name in (ext.version_symbol, *ext.entries):
        assert getattr(L, name).restype is ctypes.c_int
    assert lib.load_pointfield() is L and L is not lib.load() and L is not lib.load_group()
    text = open(os.path.join(ROOT, "include", "tsdf_pointfield.h")).read()
    for word in ("#define TSDF_POINTFIELD_VERSION 1", "#define TSDF_POINTFIELD_MAX_CLOUD 12288", "#define TSDF_POINTFIELD_MAX_K 12288",
                 "#define TSDF_POINTFIELD_MAX_VOTES 128", "#define TSDF_POINTFIELD_MAX_JOINTS 65536", "ties to the LOWEST rank",
                 "TREE SUM", "never a member", "rounded ONCE"):
        assert word in text, word
    assert (lib.POINTFIELD_MAX_CLOUD, lib.POINTFIELD_MAX_K, lib.POINTFIELD_MAX_VOTES, lib.POINTFIELD_MAX_JOINTS) == \
        (pr.MAX_CLOUD, pr.MAX_K, pr.MAX_VOTES, pr.MAX_JOINTS) and lib.POINTFIELD_MAX_CLOUD == lib.GROUP_MAX_CLOUD
    assert lib.POINTFIELD_LAYOUTS == {"cp": 0, "pc": 1}
    assert (lib.TSDF_HEATMAP_F32, lib.TSDF_LOWP_F16, lib.TSDF_LOWP_BF16) == (0, 1, 2)     # joint_heatmaps' dtype codes
    for code, word in enumerate(("F32", "F16", "BF16")):
        assert f"#define TSDF_POINTFIELD_{word} {code}" in text
    assert lib.load().tsdf_version() == 7 and lib.load_group().tsdf_group_version() == 1


def test_wrong_version_and_missing_library_raise_import_error(pkg, monkeypatch):
    lib = pkg._lib
    row = lib._POINTFIELD
    monkeypatch.delitem(lib._ext_libs, "pointfield", raising=False)
    monkeypatch.setattr(lib, "_POINTFIELD", row._replace(version=row.version + 1))
    with pytest.raises(ImportError, match="version 1.*csrc pointfield"):
        lib.load_pointfield()
    monkeypatch.setattr(lib, "_POINTFIELD", row._replace(path=os.path.join(ROOT, "build", "no_such_libtsdf_pointfield.so")))
    with pytest.raises(ImportError, match="csrc pointfield"):
        lib.load_pointfield()


# ---- build pins ----
def test_makefile_builds_it_outside_the_pinned_table():
    src = open(os.path.join(CSRC, "Makefile")).read()
    lines = src.splitlines()
    assert "pointfield_DEPS := prim.inc pointfield_host.inc" in lines and "$(eval $(call EXT_RULES,pointfield))" in lines
    (all_line,) = [ln for ln in lines if ln.startswith("all:")]
    (phony,) = [ln for ln in lines if ln.startswith(".PHONY:")]
    assert "pointfield" in all_line.split()
    assert {"pointfield", "pointfield-resources", "pointfield-asm", "pointfield-host-asan"} <= set(phony.split())
    assert "../libtsdf_pointfield.so" in lines[lines.index("clean:") + 1].split()
    assert "pointfield_host.inc" in src.split("$(filter-out", 1)[1].split(",", 1)[0].split()   # not a part of the product
    (exts,) = [ln for ln in lines if re.match(r"^EXTS := ", ln)]
    assert "pointfield" not in exts.split() and len(exts.split(":=")[1].split()) == 11
    assert "-ffp-contract=off" in src


def test_make_rules_cross_compile_for_gfx950_without_scratch():
    r = subprocess.run(["make", "-C", CSRC, "pointfield", "pointfield-resources"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stdout + r.stderr
    assert "tsdf_pointfield_encode_kernel" in text and "tsdf_pointfield_decode_kernel" in text
    scratch = [ln for ln in text.splitlines() if "ScratchSize" in ln]
    # two kernels, each with its keys in registers and with its keys recomputed
    assert len(scratch) == 4 and all(ln.split("]:")[1].split()[0] == "0" for ln in scratch), scratch
    vgprs = [int(ln.split("VGPRs:")[1].split()[0]) for ln in text.splitlines() if " VGPRs:" in ln]
    lds = [int(ln.split("]:")[1].split()[0]) for ln in text.splitlines() if "LDS Size" in ln]
    assert len(vgprs) == 4 and max(vgprs) <= 128          # 256 lanes a workgroup, four or more workgroups a CU
    assert lds == [0] * 4                                 # all of it dynamic, sized by P
    unit = open(os.path.join(CSRC, "tsdf_pointfield.hip")).read()
    assert sorted(re.findall(r'#include "(\w+\.inc)"', unit)) == ["device.inc", "pointfield_host.inc", "prim.inc"]
    body = unit.split("namespace {", 1)[1]
    assert not re.search(r"atomic(Add|Max|Min|CAS|Exch|And|Or|Xor)", body) and "__device__ int" not in unit   # no globals
    assert "__builtin_fma" not in unit and "fma(" not in body and "printf" not in unit and "hipMalloc" not in unit
    select = body.split("void pf_select(", 1)[1].split("\n}\n", 1)[0]
    assert "__syncthreads" not in select and "__popcll(__ballot(" in select and "sort" not in select   # a selection without a sort
    recorded = open(os.path.join(ROOT, "profiles", "pointfield", "resources.txt")).read()
    assert recorded.count("ScratchSize [bytes/lane]: 0") >= 4 and f"VGPRs: {max(vgprs)}" in recorded


def test_the_library_includes_the_same_text():
    unit = open(os.path.join(CSRC, "tsdf_pointfield.hip")).read()
    inc, main = (open(os.path.join(CSRC, f)).read() for f in ("pointfield_host.inc", "pointfield_host_main.cc"))
    theirs = open(os.path.join(CSRC, "device.inc")).read().splitlines()
    (line,) = [ln for ln in main.splitlines() if re.search(r"\bbool misaligned\(", ln)]
    assert line in theirs and "misaligned(" in inc and not re.search(r"\bbool misaligned\(", inc)   # used, not restated
    order = [unit.index(f'#include "{f}"') for f in ("device.inc", "prim.inc", "pointfield_host.inc")]
    assert order == sorted(order)
    for name in ("pf_encode_defect(", "pf_decode_defect(", "pf_plan(", "pf_padded("):
        assert name in unit and name in inc, name
    for name in ("pf_defect(", "pf_plan(", "pf_padded(", "pf_encode_defect(", "pf_decode_defect("):
        assert name in main, name
    assert "constexpr int kPfJoints = kPfWaves * kPfPerWave;" in inc and "constexpr int kPfPerWave = 1;" in inc


def test_host_code_under_sanitizers_as_a_stand_alone_program():
    subprocess.check_call(["make", "-C", CSRC, "-B", "pointfield-host-asan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "build", "pointfield_host_asan")
    env = dict(os.environ)
    env.update(ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert f"pointfield host code ok (256 lanes, {pr.JOINTS_PER_GROUP} joints a group, cap {pr.MAX_CLOUD}, " in r.stdout, tail
    assert "Sanitizer" not in tail and "runtime error" not in tail and "FAILED" not in tail, tail


# ---- the plan ----
def test_plan(pkg):
    L = pkg._lib.load_pointfield()
    lds, per, grp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for P in (1, 63, 64, 65, 1024, 1025, 12288):
        for J in (1, 3, 4, 5, 21, 65536):
            for K in (1, 64, 128, 12288):
                assert L.tsdf_pointfield_plan(P, J, K, lds, per, grp) == 0
                assert (lds.value, per.value, grp.value) == (pr.lds_bytes(P), pr.JOINTS_PER_GROUP, -(-J // pr.JOINTS_PER_GROUP))
                assert pkg.pointfield_plan(P, J, K) == (lds.value, per.value, grp.value)
    assert pkg.pointfield_plan(1024, 21, 64) == (12 * 1024 + 16, 4, 6) and pkg.pointfield_plan(12288, 3, 128)[0] <= 160 * 1024
    for bad in ((0, 1, 1), (12289, 1, 1), (-1, 1, 1), (64, 0, 1), (64, -1, 1), (64, 65537, 1), (64, 1, 0), (64, 1, 12289), (64, 1, -1)):
        assert L.tsdf_pointfield_plan(*bad, lds, per, grp) == INVALID, bad
        with pytest.raises(ValueError):
            pkg.pointfield_plan(*bad)
    assert L.tsdf_pointfield_plan(64, 1, 1, None, per, grp) == INVALID and L.tsdf_pointfield_plan(64, 1, 1, lds, per, None) == INVALID
    assert L.tsdf_pointfield_plan(64, 1, 1, lds, None, grp) == INVALID


# ---- refusals ----
null, one, odd4, odd2, odd1 = (ctypes.c_void_p(v) for v in (0, 64, 68, 66, 65))


def _entries(pkg):
    """The two entries on dummy pointers (64: aligned for every check), every argument good unless named."""
    L = pkg._lib.load_pointfield()

    def encode(points=one, pitch=100, joints=one, status_in=one, n=3, P=100, J=21, K=8, radius=30.0, layout=0, dtype=0, field=one,
               valid=one, status=one):
        return L.tsdf_pointfield_encode_hip(points, pitch, joints, status_in, n, P, J, K, radius, layout, dtype, null, field, valid, status)

    def decode(points=one, pitch=100, field=one, status_in=one, n=3, P=100, J=21, K=8, radius=30.0, layout=0, dtype=0, joints=one,
               weight=one, status=one):
        return L.tsdf_pointfield_decode_hip(points, pitch, field, status_in, n, P, J, K, radius, layout, dtype, null, joints, weight, status)
    return encode, decode


# in the header's order
SHAPE = [dict(n=-1), dict(P=0), dict(P=-1), dict(P=12289), dict(J=0), dict(J=-1), dict(J=65537), dict(K=0), dict(K=-1),
         dict(pitch=99), dict(pitch=-1), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")),
         dict(layout=2), dict(layout=-1), dict(dtype=3), dict(dtype=-1)]                # refused whatever n is
LATER = [dict(points=null), dict(field=null), dict(joints=null), dict(status=null), dict(points=odd2), dict(joints=odd2),
         dict(field=odd2), dict(field=odd1, dtype=1), dict(field=odd1, dtype=2), dict(n=2 ** 22)]   # ... with n > 0; n == 0 is a no-op
ENCODE = [dict(K=12289), dict(valid=null), dict(valid=odd2)]
DECODE = [dict(K=129), dict(weight=null), dict(weight=odd2)]


def test_every_defect_is_refused_before_device_work(pkg):
    encode, decode = _entries(pkg)
    for fn, more in ((encode, ENCODE), (decode, DECODE)):
        for kw in SHAPE + more[:1]:
            assert fn(**kw) == INVALID, kw
            if "n" not in kw:
                assert fn(n=0, **kw) == INVALID, kw
        for kw in LATER + more[1:]:
            assert fn(**kw) == INVALID, kw
            if "n" not in kw:
                assert fn(n=0, **kw) == 0, kw
        assert fn(n=0) == 0
        # of two defects the earlier rule speaks: a bad K before a bad radius before a NULL pointer
        assert fn(K=0, points=null) == INVALID and fn(n=0, K=0, points=null) == INVALID
        assert fn(n=0, radius=0.0, points=null) == INVALID and fn(n=0, points=null, field=odd1) == 0


# Good arguments reach check_device.  On a machine WITH a device they would launch on the dummy pointers, so this row is
# checked where the device check answers -2.
@pytest.mark.skipif(torch.cuda.is_available(), reason="good arguments with dummy pointers must stop at the device check")
def test_good_arguments_get_as_far_as_the_device(pkg):
    encode, decode = _entries(pkg)
    assert encode() == NO_DEVICE and decode() == NO_DEVICE
    for K in (1, 64, 128):
        assert encode(K=K) == NO_DEVICE and decode(K=K) == NO_DEVICE
    assert encode(K=12288) == NO_DEVICE and encode(status_in=null) == NO_DEVICE and decode(status_in=null) == NO_DEVICE
    for fn in (encode, decode):
        assert fn(layout=1) == NO_DEVICE and fn(dtype=1, field=odd2) == NO_DEVICE and fn(dtype=2, field=odd2) == NO_DEVICE
        assert fn(pitch=2 ** 40) == NO_DEVICE and fn(P=12288, pitch=12288) == NO_DEVICE and fn(radius=1e-300) == NO_DEVICE
        assert fn(n=2 ** 24 - 1, J=4) == NO_DEVICE and fn(n=2 ** 24, J=4) == INVALID and fn(n=2 ** 23, J=5) == INVALID


# ---- Python wrappers ----
@pytest.fixture()
def V():
    return importlib.import_module(PKG + ".voxelize")


def V_dev_check(name, t, dtype):
    """``_dev_check`` without "lives on the GPU": the rest of it is under test."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def test_public_names_and_refusals(pkg, V, monkeypatch):
    log = []
    monkeypatch.setattr(V, "_call", lambda *a, **kw: log.append(a))
    for name in ("point_fields", "field_joints", "PointFieldBatch", "FieldJoints", "pointfield_plan"):
        assert name in pkg.__all__ and hasattr(pkg, name) and name in pkg.__doc__, name
    assert "tsdf_pointfield.h" in pkg.__doc__ and "libtsdf_pointfield.so" in pkg.__doc__ and "fields=" in pkg.__doc__
    sig = inspect.signature(pkg.point_fields).parameters
    assert list(sig) == ["cloud", "joints", "k", "radius", "layout", "dtype", "status", "out"]
    assert sig["k"].default == 64 and sig["radius"].default is inspect.Parameter.empty and sig["layout"].default == "cp"
    assert sig["dtype"].default is torch.float32
    sig = inspect.signature(pkg.field_joints).parameters
    assert list(sig) == ["cloud", "field", "radius", "points", "layout", "status", "out"]
    assert sig["points"].default == 25 and sig["radius"].default is inspect.Parameter.empty
    assert inspect.signature(pkg.AugmentedStep.__init__).parameters["fields"].default is None
    assert pkg.PointFieldBatch._fields == ("field", "valid", "status") and pkg.FieldJoints._fields == ("joints", "weight", "status")
    cloud, joints = torch.rand(3, 50, 3), torch.rand(3, 21, 3)
    with pytest.raises(TypeError):
        pkg.point_fields(cloud, joints)                                  # radius has no default
    with pytest.raises(TypeError):
        pkg.field_joints(cloud, torch.rand(3, 84, 50))
    # there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        pkg.point_fields(cloud, joints, radius=30.0)
    with pytest.raises(ValueError, match="GPU"):
        pkg.field_joints(cloud, torch.rand(3, 84, 50), radius=30.0)
    # everything else, with the device check out of the way: judged before the launch
    monkeypatch.setattr(V, "_dev_check", lambda name, t, dtype, device=None, host_ok=False: V_dev_check(name, t, dtype))
    field = torch.rand(3, 84, 50)
    for bad in (0, -1, 12289, 8.0, True, "8", None):
        with pytest.raises(ValueError, match="k must be"):
            pkg.point_fields(cloud, joints, bad, radius=30.0)
    for bad in (0, -1, 129, 8.0, True, "8", None):
        with pytest.raises(ValueError, match="points must be"):
            pkg.field_joints(cloud, field, radius=30.0, points=bad)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), "30", None, True, torch.tensor(30.0)):
        with pytest.raises(ValueError, match="radius"):
            pkg.point_fields(cloud, joints, radius=bad)
        with pytest.raises(ValueError, match="radius"):
            pkg.field_joints(cloud, field, radius=bad)
    for bad in ("czyx", "PC", 0, None):
        with pytest.raises(ValueError, match="layout"):
            pkg.point_fields(cloud, joints, radius=30.0, layout=bad)
        with pytest.raises(ValueError, match="layout"):
            pkg.field_joints(cloud, field, radius=30.0, layout=bad)
    for bad in (torch.float64, torch.int32, "float32", None, np.float32):
        with pytest.raises(ValueError, match="dtype"):
            pkg.point_fields(cloud, joints, radius=30.0, dtype=bad)
    for bad in (cloud.double(), cloud.half(), cloud.numpy(), None, torch.rand(3, 50, 2), torch.rand(50, 3), torch.rand(3, 0, 3),
                torch.rand(3, 12289, 3), cloud.transpose(0, 1), torch.rand(3, 50, 6)[:, :, :3], torch.rand(3, 100, 3)[:, ::2]):
        with pytest.raises(ValueError):
            pkg.point_fields(bad, joints, radius=30.0)
        with pytest.raises(ValueError):
            pkg.field_joints(bad, field, radius=30.0)
    for bad in (joints.double(), joints.numpy(), None, torch.rand(2, 21, 3), torch.rand(3, 21, 2), torch.rand(3, 64), torch.rand(3, 0, 3),
                torch.rand(3, 171, 3), torch.rand(3, 42, 3)[:, ::2], torch.rand(3, 7, 3, 1), torch.rand(3)):
        with pytest.raises(ValueError):
            pkg.point_fields(cloud, bad, radius=30.0)
    for bad in (field.double(), field.numpy(), None, torch.rand(2, 84, 50), torch.rand(3, 83, 50), torch.rand(3, 84, 49), torch.rand(3, 50, 84),
                torch.rand(3, 0, 50), torch.rand(3, 84, 100)[:, :, ::2], torch.rand(3, 84 * 50)):
        with pytest.raises(ValueError):
            pkg.field_joints(cloud, bad, radius=30.0)
    with pytest.raises(ValueError):
        pkg.field_joints(cloud, field, radius=30.0, layout="pc")         # [3, 84, 50] is no [3, 50, 4J]
    for fn, arg in ((pkg.point_fields, joints), (pkg.field_joints, field)):
        for bad in (torch.zeros(3), torch.zeros(4, dtype=torch.int32), torch.zeros((3, 2), dtype=torch.int32), [0, 0, 0]):
            with pytest.raises(ValueError):
                fn(cloud, arg, radius=30.0, status=bad)
    good = pkg.point_fields(cloud, joints, 6, radius=30.0)
    assert [tuple(t.shape) for t in good] == [(3, 84, 50), (3, 21), (3,)] and len(log) == 1
    back = pkg.field_joints(cloud, good.field, radius=30.0)
    assert [tuple(t.shape) for t in back] == [(3, 21, 3), (3, 21), (3,)] and len(log) == 2
    del log[:]
    for bad in (good._replace(field=torch.zeros((3, 50, 84))), good._replace(field=torch.zeros((3, 84, 50), dtype=torch.float16)),
                good._replace(valid=torch.zeros((3, 21))), good._replace(status=torch.zeros(4, dtype=torch.int32)),
                tuple(good), "out", back):
        with pytest.raises(ValueError):
            pkg.point_fields(cloud, joints, 6, radius=30.0, out=bad)
    for bad in (back._replace(joints=torch.zeros((3, 21, 4))), back._replace(weight=torch.zeros((3, 22))),
                back._replace(status=torch.zeros(3)), tuple(back), good):
        with pytest.raises(ValueError):
            pkg.field_joints(cloud, good.field, radius=30.0, out=bad)
    assert log == []                                                    # refused before anything is launched
    # a good call is one launch of the entry, the stream at position 11
    status = torch.zeros(3, dtype=torch.int32)
    out = pkg.point_fields(cloud, joints.reshape(3, 63), 7, radius=12.5, layout="pc", dtype=torch.bfloat16, status=status)
    (dev, fn, args, stream_at), = log
    assert fn.__name__ == "tsdf_pointfield_encode_hip" and stream_at == 11 and len(args) == 15 and args[11] is None
    assert args[:11] == [cloud.data_ptr(), 50, joints.data_ptr(), status.data_ptr(), 3, 50, 21, 7, 12.5, 1, 2]
    assert args[12:] == [t.data_ptr() for t in out] and isinstance(out, pkg.PointFieldBatch)
    assert [tuple(t.shape) for t in out] == [(3, 50, 84), (3, 21), (3,)]
    assert [t.dtype for t in out] == [torch.bfloat16, torch.int32, torch.int32]
    del log[:]
    got = pkg.field_joints(cloud[:, :30], out.field[:, :30].contiguous(), radius=12.5, points=9, layout="pc")   # a prefix, read in place
    (dev, fn, args, stream_at), = log
    assert fn.__name__ == "tsdf_pointfield_decode_hip" and stream_at == 11 and len(args) == 15
    assert args[:2] == [cloud.data_ptr(), 50] and args[3:11] == [None, 3, 30, 21, 9, 12.5, 1, 2]
    assert args[12:] == [t.data_ptr() for t in got] and [t.dtype for t in got] == [torch.float32, torch.float32, torch.int32]
    del log[:]
    assert pkg.field_joints(cloud, good.field, radius=1)[0].shape == (3, 21, 3) and log[0][2][7] == 25 and log[0][2][8] == 1.0
    # an empty batch launches nothing
    del log[:]
    empty = pkg.point_fields(torch.zeros((0, 5, 3)), torch.zeros((0, 2, 3)), radius=1.0)
    assert log == [] and empty.field.shape == (0, 8, 5) and empty.valid.shape == (0, 2)
    assert pkg.field_joints(torch.zeros((0, 5, 3)), empty.field, radius=1.0).joints.shape == (0, 2, 3) and log == []


# ---- AugmentedStep(fields=) through stubbed primitives ----
N, R8 = 3, 8
STUBBED = ("aug_xforms_at", "map_step_head", "voxelize_indexed", "map_grids", "_map_grid_lowp", "_map_grid_accurate",
           "narrow_volumes", "transform_joints", "normalize_joints", "joint_heatmaps", "aabb", "_occupancy", "_fps_crop",
           "_knn", "_normals", "_point_fields")


class Rec:
    """Recorders in the style of tests/test_group_cpu.py: ``log`` holds (name, arguments by parameter name) of every
    primitive call; every stub returns the ``out`` it was given."""

    def __init__(self, V, monkeypatch):
        self.log = []
        for name in STUBBED:
            monkeypatch.setattr(V, name, self._stub(name, getattr(V, name)))
        monkeypatch.setattr(V, "_dev_check", lambda *a, **kw: None)    # ("on the GPU": the check is not under test)
        monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)

    def _stub(self, name, real):
        sig = inspect.signature(real)

        def fn(*a, **kw):
            b = sig.bind(*a, **kw)
            b.apply_defaults()
            self.log.append((name, dict(b.arguments)))
            out = b.arguments.get("out")
            return (out, None) if name in ("_map_grid_lowp", "_occupancy") else (out, None, None) if name == "_map_grid_accurate" else out
        fn.__name__ = name
        return fn

    def names(self):
        return [e[0] for e in self.log]


CONFIGS = {
    "plain": (dict(), ["aug_xforms_at", "voxelize_indexed"]),
    "head": (dict(fused_head=True), ["map_step_head", "voxelize_indexed"]),
    "heatmap_occupancy": (dict(heatmap=(12, 1.7), occupancy=(16,)), ["aug_xforms_at", "voxelize_indexed", "joint_heatmaps", "_occupancy"]),
}


def _step(V, kw, **more):
    pack = torch.rand(30), torch.tensor([0, 10, 20, 30]), torch.zeros((N, 6), dtype=torch.int32)
    return V.AugmentedStep(*pack, N, gt=torch.rand(N, 21, 3), centres=torch.rand(N, 3), res=R8, layout="cxyz", graph=False, **kw, **more)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_augmented_step_appends_exactly_one_launch_at_the_end(V, monkeypatch, name):
    kw, want = CONFIGS[name]
    rec = Rec(V, monkeypatch)
    s = _step(V, kw)
    assert rec.names() == want and s.field is None and s.field_valid is None
    del rec.log[:]
    s = _step(V, kw, fps=(64,), fields=None)
    assert rec.names() == want + ["_fps_crop"] and s.field is None           # the launches there were
    del rec.log[:]
    s = _step(V, kw, fps=(64,), groups=((32, 16),), normals=10, fields=(16, 40.0))
    assert rec.names() == want + ["_fps_crop", "_normals", "_knn", "_point_fields"]
    f = rec.log[-1][1]
    assert f["cloud"] is s.cloud and f["joints"] is s.gt_aug and f["status"] is s.cloud_status and f["layout"] == "cp"
    assert (f["k"], f["radius"], f["dtype"]) == (16, 40.0, torch.float32)
    assert f["out"].field is s.field and f["out"].valid is s.field_valid and f["out"].status.shape == (N,)
    assert s.field.shape == (N, 84, 64) and s.field.dtype is torch.float32 and s.field_valid.shape == (N, 21)
    assert s.field_valid.dtype is torch.int32
    del rec.log[:]
    s._run()                                                              # what a step without a graph issues
    assert rec.names() == want + ["_fps_crop", "_normals", "_knn", "_point_fields"] and rec.log[-1][1]["out"].field is s.field
    assert "return self.out if self._gt is None else (self.out, self.gt_nor, self.gt_aug)" in inspect.getsource(V.AugmentedStep.step)
    del rec.log[:]
    s = _step(V, kw, fps=(64,), fields=(64, 25, torch.bfloat16))
    assert rec.names() == want + ["_fps_crop", "_point_fields"] and s.field.dtype is torch.bfloat16
    assert rec.log[-1][1]["radius"] == 25.0 and rec.log[-1][1]["k"] == 64


def test_augmented_step_refuses_bad_fields(V, monkeypatch):
    Rec(V, monkeypatch)
    for more in (dict(fields=(16, 40.0)), dict(fps=(64,), fields=(16,)), dict(fps=(64,), fields=16), dict(fps=(64,), fields=(0, 40.0)),
                 dict(fps=(64,), fields=(12289, 40.0)), dict(fps=(64,), fields=(16, 0.0)), dict(fps=(64,), fields=(16, float("nan"))),
                 dict(fps=(64,), fields=(16, 40.0, torch.float64)), dict(fps=(64,), fields=(16, 40.0, torch.float32, 1)),
                 dict(fps=(16384,), fields=(16, 40.0))):
        with pytest.raises(ValueError):
            _step(V, {}, **more)
    pack = torch.rand(30), torch.tensor([0, 10, 20, 30]), torch.zeros((N, 6), dtype=torch.int32)
    with pytest.raises(ValueError, match="gt"):
        V.AugmentedStep(*pack, N, centres=torch.rand(N, 3), res=R8, graph=False, fps=(64,), fields=(16, 40.0))
