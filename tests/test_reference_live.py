"""CPU tier: the oracle against the reference's own loop on frames that are NOT among the volume fixtures.  tests/golden/
pins 22 frames in its *.npz volumes; tests/golden/unseen_ref_<k>.npz hold what the reference's loop (pre/tsdf_for.py::
tsdf_f / tsdf_cal through tools/make_goldens.run_reference: as it runs today and on float64-typed parameters = the numba
typing) computed for 33 more seeded frames of every family — benchmark distributions, near / far hands, corner bboxes,
sparse, dense, negative and mixed-sign depths (tools/make_goldens.unseen_frames) — and the oracle must give the same
bits.  The depths are made again by the seeded generator and checked against the sha256 the fixtures recorded; nothing
here touches a GPU."""
import glob
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mg():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return importlib.import_module("make_goldens")     # its frame list and loop32_emulation; not the reference
    finally:
        sys.path.pop(0)


def _recorded(golden_dir):
    """name -> what the reference computed for that frame (loop32 rebuilt from loop64 and the recorded differences)."""
    out = {}
    for fn in sorted(glob.glob(os.path.join(golden_dir, "unseen_ref_*.npz"))):
        z = np.load(fn)
        for i, name in enumerate(z["names"]):
            g = {k[len(f"f{i}_"):]: z[k] for k in z.files if k.startswith(f"f{i}_")}
            loop32 = g["loop64"].copy()
            loop32.reshape(-1)[g["loop32_diff_index"]] = g["loop32_diff_value"]
            g["loop32"] = loop32
            out[str(name)] = g
    return out


def test_oracle_equals_the_reference_loop_on_unseen_frames(mg, golden_dir):
    import oracle

    n_flip_frames = 0
    frames = mg.unseen_frames()
    rec = _recorded(golden_dir)
    assert len(frames) >= 33
    assert sorted(rec) == sorted(name for name, _, _ in frames)
    for name, h, d in frames:
        g = rec[name]
        assert str(g["depth_sha256"]) == mg.depth_digest(d), f"{name}: the generator no longer makes the recorded frame"
        np.testing.assert_array_equal(h, g["header"], err_msg=name)
        out, pm = oracle.voxels(d, h, g["vox_ori"], g["voxel_len"], g["trunc"], R=32, layout=0, want_pixmap=True)
        np.testing.assert_array_equal(out, g["loop64"], err_msg=name)                 # a4, numba typing: bit for bit
        bad = (np.abs(out - g["loop32"]) > 1e-5).any(axis=0)
        assert bad.sum() == int(g["n_flip"]), name                                     # a4', the loop as it runs
        n_flip_frames += int(g["n_flip"]) > 0
        grid, ori = oracle.glue(g["aabb_min"], g["aabb_max"], 32)                     # a3: the reference's own glue
        np.testing.assert_array_equal(grid[:3], g["mid_p"], err_msg=name)
        assert grid[3] == g["max_l"] and grid[4] == g["voxel_len"] and grid[5] == g["trunc"], name
        np.testing.assert_array_equal(ori, g["vox_ori"], err_msg=name)
        nv, mn, mx = oracle.aabb(d, h)                                                 # a2': CPU witness, 1 ulp
        assert nv == int(g["pc_n"])
        np.testing.assert_allclose(mn, g["pc_min"], rtol=3e-7, atol=0, err_msg=name)
        np.testing.assert_allclose(mx, g["pc_max"], rtol=3e-7, atol=0, err_msg=name)
        # the search emulation of tools/make_goldens.py stays the reference's float32 loop
        np.testing.assert_array_equal(mg.loop32_emulation(d, h, g["vox_ori"], g["voxel_len"], g["trunc"]), g["loop32"])
    print(f"{len(frames)} unseen frames against the reference loop's recorded results; {n_flip_frames} of them with "
          "float32/float64 flips")
