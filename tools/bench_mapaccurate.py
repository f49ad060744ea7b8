#!/usr/bin/env python3
"""What the accurate directional TSDF costs under a per-frame map (one JSON line; ``--out`` also writes it to a file,
default profiles/mapaccurate/bench_mapaccurate.json).

Legs, per shape, on the same frames in the same run (the rows of a mapped leg are its maps' own placement, map_grids):
  plain          voxelize_grid_accurate()        the un-mapped search (libtsdf_accurate.so) on the aabb rows: the yardstick
  map_identity   voxelize_map_grid_accurate()    identity maps on the SAME rows: mapped / plain is the price of the general
                                                 arithmetic
  map_aug        voxelize_map_grid_accurate()    drawn augmentation maps (aug_xforms): the rectangle widens by the rows of A^-1
  map_obb        voxelize_map_grid_accurate()    principal-axis maps (obb_xforms)
  proj_aug       voxelize_aug_grid()             the mapped PROJECTIVE pass under the drawn maps: the price of the encoding
at 16 crops R = 32 (the reference's batch), 1024 crops R = 32 and 256 crops R = 64; and at batch 16 and 1024, R = 32,
  step_projective / step_accurate (and both with dtype=torch.bfloat16)   AugmentedStep.step() replayed from its graph.
``--windows`` (CPU only, no device) prints instead the mean search-window size per voxel the kernel's rectangle gives on
the first frames of a shape under the three map families, from the formulas restated in numpy: where the area goes.

Method: inputs resident on the device, a warm-up, then device events around back-to-back launches — at most --iters of
them, fewer where one launch is long (about --budget seconds per timed window, at least 5) —; the legs of a shape take
turns for --rounds rounds and the median round is reported with min and max.  Every shape runs in a child process of its
own under its own time limit (--limit seconds), one after the other, and the first that fails ends the run: nothing more
is started on the device after it.  ``--lib`` names another build of libtsdf_mapaccurate.so and ``--accurate-lib`` one of
libtsdf_accurate.so (the `plain` leg's): an A/B against the parent commit's, one process per build, taking turns.

    python tools/bench_mapaccurate.py [--iters 100] [--rounds 5] [--limit 420] [--lib x.so] [--accurate-lib y.so] [--out x.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "handposeestimation-with-3d-cnns_amd"
SHAPES = ((16, 32), (1024, 32), (256, 64))
STEP_BATCHES = (16, 1024)
KEY = 0xABCDEF


def _measure(legs, a):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from _timing import timed_us
    iters = {}
    for k, fn in legs.items():                               # warm-up, and how long one launch is
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        one = time.perf_counter() - t0
        iters[k] = int(min(a.iters, max(5, a.budget / max(one, 1e-6))))
    times = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            times[k].append(timed_us(fn, iters[k]))
    return {k: dict(us=round(float(np.median(v)), 2), us_min=round(min(v), 2), us_max=round(max(v), 2), iters=iters[k])
            for k, v in times.items()}


def _inputs(n, R, a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    for name, path in (("mapaccurate", a.lib), ("accurate", a.accurate_lib)):
        if path:
            pkg._lib._EXTS[name] = pkg._lib._EXTS[name]._replace(path=os.path.abspath(path))
    synth = importlib.import_module(PKG + ".synth")
    assert torch.cuda.is_available(), "bench_mapaccurate.py needs a HIP device"
    dev = torch.device("cuda:0")
    depth, off, hdr = synth.synth_batch(n, "crop", seed0=0, threads=8)
    td, to, th = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depth, off, hdr))
    return pkg, torch, dev, depth, (td, to, th)


def one_shape(n, R, a):
    pkg, torch, dev, depth, (td, to, th) = _inputs(n, R, a)
    ab = pkg.aabb(td, to, th, res=R)
    assert not ab.status.any()
    rows = torch.cat([ab.ori, ab.grid[:, 4:6], torch.zeros_like(ab.ori)], dim=1)
    ident = torch.tensor([1., 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] * 2, dtype=torch.float64, device=dev).repeat(n, 1)
    aug = pkg.aug_xforms(ab.grid[:, :3].contiguous(), key=KEY)
    obb = pkg.obb_xforms(td, to, th)
    assert not obb.status.any()
    g_aug = pkg.map_grids(td, to, th, aug, res=R)
    g_obb = pkg.map_grids(td, to, th, obb.xforms, res=R)
    assert not g_aug.status.any() and not g_obb.status.any()
    out = torch.empty((n, 3, R, R, R), dtype=torch.float32, device=dev)
    legs = {"plain": lambda: pkg.voxelize_grid_accurate(td, to, th, rows, res=R, out=out),
            "map_identity": lambda: pkg.voxelize_map_grid_accurate(td, to, th, ident, rows, res=R, out=out),
            "map_aug": lambda: pkg.voxelize_map_grid_accurate(td, to, th, aug, g_aug.grid, res=R, out=out),
            "map_obb": lambda: pkg.voxelize_map_grid_accurate(td, to, th, obb.xforms, g_obb.grid, res=R, out=out),
            "proj_aug": lambda: pkg.voxelize_aug_grid(td, to, th, aug, g_aug.grid, res=R)}
    # the identity leg computes what the plain pass computes (checked once, outside the clock)
    p, _, pn = pkg.voxelize_grid_accurate(td, to, th, rows, res=R, nearest=True)
    m, _, mn = pkg.voxelize_map_grid_accurate(td, to, th, ident, rows, res=R, nearest=True)
    agree = float((pn == mn).double().mean())
    diff = float((p - m).abs().max())
    near = {k: float((pkg.voxelize_map_grid_accurate(td, to, th, x, g, res=R, nearest=True)[2] >= 0).double().mean())
            for k, (x, g) in dict(map_identity=(ident, rows), map_aug=(aug, g_aug.grid), map_obb=(obb.xforms, g_obb.grid)).items()}
    t = _measure(legs, a)
    row = dict(device=torch.cuda.get_device_name(0), n=n, kind="crop", res=R, pixels=int(depth.size),
               identity_agrees_with_plain_on_nearest=round(agree, 6), identity_largest_difference_to_plain=diff,
               near_share={k: round(v, 4) for k, v in near.items()}, **t,
               us_per_frame={k: round(v["us"] / n, 2) for k, v in t.items()},
               mapped_over_plain_identity=round(t["map_identity"]["us"] / t["plain"]["us"], 3),
               mapped_over_plain_aug=round(t["map_aug"]["us"] / t["plain"]["us"], 3),
               mapped_over_plain_obb=round(t["map_obb"]["us"] / t["plain"]["us"], 3),
               accurate_over_projective_aug=round(t["map_aug"]["us"] / t["proj_aug"]["us"], 2))
    print(json.dumps(row))


def one_step(n, a):
    R = 32
    pkg, torch, dev, depth, (td, to, th) = _inputs(n, R, a)
    centres = pkg.aabb(td, to, th, res=R).grid[:, :3].contiguous()
    index = torch.arange(n, dtype=torch.int64, device=dev)
    steps = {f"step_{kind}{'_bf16' if dt is not None else ''}":
             pkg.AugmentedStep(td, to, th, n, centres=centres, res=R, dtype=dt, tsdf=kind)
             for kind in ("projective", "accurate") for dt in (None, torch.bfloat16)}
    counter = [0]

    def leg(s):
        def fn():
            counter[0] += n
            s.step(index, KEY, counter[0])
        return fn
    t = _measure({k: leg(s) for k, s in steps.items()}, a)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), n=n, res=R, **t,
                          accurate_over_projective=round(t["step_accurate"]["us"] / t["step_projective"]["us"], 2),
                          accurate_over_projective_bf16=round(t["step_accurate_bf16"]["us"] / t["step_projective_bf16"]["us"], 2))))


def windows(a):
    """CPU only: the mean rectangle per voxel (pixels) by the kernel's formulas, per map family, on a few frames."""
    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import map_geom_ref as mg
    import mapaccurate_ref as mr
    synth = importlib.import_module(PKG + ".synth")
    augment = importlib.import_module(PKG + ".augment")
    F, cx, cy, eps = mg.DEFAULT_CAM[:4]
    n, R = a.windows, 32
    depth, off, hdr = synth.synth_batch(n, "crop", seed0=0)
    rng = np.random.default_rng(0)
    rows_out = []
    for family in ("identity", "aug", "obb"):
        area, crop = [], []
        for i in range(n):
            d, h = depth[off[i]:off[i + 1]], hdr[i]
            if family == "identity":
                xf = mg.pack(np.eye(3), np.zeros(3))
            elif family == "obb":
                xf = mg.xforms_for(["obb"], d, np.array([0, d.size]), h[None])[0]
            else:                                            # the augmentation's distributions, about the cloud's centre
                xf = augment.random_affines(mg.centre(d, h)[None], rng)[0][0]
            row, _ = mr.placement_row(d, h, xf, R)
            Aw = xf[:12].reshape(3, 4)[:, :3]
            B = np.linalg.inv(Aw)
            hh = np.sqrt((B * B).sum(1))
            Tw = float(row[4]) * (1 + 2.0 ** -20)
            vx, vy, vz = mg.centres(row, R)
            zz, yy, xx = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
            c = np.einsum("ij,j...->i...", B, np.stack([vx[xx] - xf[3], vy[yy] - xf[7], vz[zz] - xf[11]]))
            H = Tw * hh[:, None, None, None]
            left, top, right, bottom = (int(v) for v in h[2:6])
            dlo, dhi = -c[2] - H[2], -c[2] + H[2]
            fin = (dlo >= eps) | (dhi <= -eps)
            with np.errstate(all="ignore"):
                q = lambda lo, hi: (np.minimum.reduce([lo / dlo, lo / dhi, hi / dlo, hi / dhi]),
                                    np.maximum.reduce([lo / dlo, lo / dhi, hi / dlo, hi / dhi]))   # noqa: E731
                (xl, xh), (yl, yh) = q(c[0] - H[0], c[0] + H[0]), q(c[1] - H[1], c[1] + H[1])
                c0, c1 = np.clip(np.floor(cx + F * xl) - 1, left, right), np.clip(np.ceil(cx + F * xh) + 2, left, right)
                r0, r1 = np.clip(np.floor(cy - F * yh) - 1, top, bottom), np.clip(np.ceil(cy - F * yl) + 2, top, bottom)
            w = np.where(fin, (c1 - c0) * (r1 - r0), (right - left) * (bottom - top))
            area.append(float(w.mean()))
            crop.append((right - left) * (bottom - top))
        rows_out.append(dict(family=family, frames=n, res=R, mean_window_px=round(float(np.mean(area)), 1),
                             mean_crop_px=round(float(np.mean(crop)), 1)))
    print(json.dumps(dict(windows=rows_out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--limit", type=int, default=420, help="seconds per child process")
    ap.add_argument("--one", nargs=2, type=int, metavar=("N", "R"))
    ap.add_argument("--step", type=int, metavar="N")
    ap.add_argument("--lib")
    ap.add_argument("--accurate-lib")
    ap.add_argument("--windows", type=int, metavar="FRAMES", help="CPU only: mean search-window sizes, no device")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapaccurate", "bench_mapaccurate.json"))
    a = ap.parse_args()
    if a.one:
        return one_shape(a.one[0], a.one[1], a)
    if a.step:
        return one_step(a.step, a)
    if a.windows:
        return windows(a)
    common = ["--iters", str(a.iters), "--rounds", str(a.rounds), "--budget", str(a.budget)]
    common += [x for flag, path in (("--lib", a.lib), ("--accurate-lib", a.accurate_lib)) if path for x in (flag, path)]
    todo = [["--one", str(n), str(R)] for n, R in SHAPES] + [["--step", str(n)] for n in STEP_BATCHES]
    rows, steps = [], []
    for step in todo:                                        # one child per step, each under its own limit; stop at the first failure
        r = subprocess.run([sys.executable, os.path.abspath(__file__), *step, *common], capture_output=True, text=True,
                           timeout=a.limit)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            raise SystemExit(f"bench_mapaccurate.py {' '.join(step)} ended with status {r.returncode}")
        row = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(row), file=sys.stderr)
        (rows if step[0] == "--one" else steps).append(row)
    device = [row.pop("device") for row in rows + steps][0]
    line = json.dumps(dict(device=device, iters_max=a.iters, rounds=a.rounds, rows=rows, steps=steps))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
