#!/usr/bin/env python3
"""What the accurate directional TSDF costs (one JSON line; ``--out`` also writes it to a file, default
profiles/accurate/bench_accurate.json).

Legs, per shape, on the same frames and the same grid rows in the same run:
  grid_accurate   voxelize_grid_accurate()   tsdf_voxelize_grid_accurate_hip, libtsdf_accurate.so
  accurate        voxelize_accurate()        aabb + the rows + the pass above
  grid            voxelize_grid()            the PROJECTIVE pass (tsdf_voxelize_grid_hip): the ratio is the price of the
                                             accurate encoding
  torch           the contract's search written in torch ops on the same GPU, what a user can do today: per frame the
                  float64 pairwise distances voxels x valid points in chunks, argmin, the three clamped components.  The
                  valid points of each frame are extracted BEFORE the clock starts, and the sign / rejection pass is left
                  out: both favour this leg.  It is timed on the first ``--torch-frames`` frames of the shape and
                  reported per frame.
at 16 crops R = 32 (the reference's batch), 1024 crops R = 32 and 256 crops R = 64, and
  tree_projective / tree_accurate   export.preprocess_tree(tsdf=...) on one synthetic subject (wall clock, files included).

Method: inputs resident on the device, a warm-up, then device events around back-to-back launches — at most --iters of
them, fewer where one launch is long (about --budget seconds per timed window, at least 5) —; the legs of a shape take
turns for --rounds rounds and the median round is reported with min and max.  Every shape and the tree leg run in a child
process of their own under their own time limit (--limit seconds), one after the other, and the first that fails ends the
run: nothing more is started on the device after it.  ``--lib`` names another build of libtsdf_accurate.so (an A/B against
the parent commit's: one process per build, taking turns).

    python tools/bench_accurate.py [--iters 100] [--rounds 5] [--limit 420] [--lib x.so] [--out x.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((16, 32), (1024, 32), (256, 64))
CHUNK_PAIRS = 1 << 24


def torch_accurate(torch, pts, rows, R):
    """The search of the contract in torch ops: per frame (nearest int64[R^3], values float32[R^3, 3])."""
    out = []
    ar = torch.arange(R, dtype=torch.float64, device=rows.device)
    for w, row in zip(pts, rows.double()):
        c = row[:3, None] + ar[None, :] * row[3]
        v = torch.stack(torch.meshgrid(c[2], c[1], c[0], indexing="ij"), dim=-1).reshape(-1, 3).flip(1)   # z, y, x order
        td = row[4]
        step = max(1, CHUNK_PAIRS // max(1, w.shape[0]))
        best, arg = [], []
        for b in range(0, v.shape[0], step):
            s = ((v[b:b + step, None, :] - w[None, :, :]) ** 2).sum(-1)
            m, k = s.min(dim=1)
            best.append(m)
            arg.append(k)
        best, arg = torch.cat(best) / (td * td), torch.cat(arg)
        t = ((v - w[arg]).abs() / td).clamp(max=1.0).float()
        out.append((torch.where(best <= 1.0, arg, torch.full_like(arg, -1)), t))
    return out


def _package(a):
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("handposeestimation-with-3d-cnns_amd")
    if a.lib:
        pkg._lib._EXTS["accurate"] = pkg._lib._EXTS["accurate"]._replace(path=os.path.abspath(a.lib))
    return pkg


def one_shape(n, R, a):
    import numpy as np
    import torch
    pkg = _package(a)
    synth = importlib.import_module("handposeestimation-with-3d-cnns_amd.synth")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from _timing import timed_us

    assert torch.cuda.is_available(), "bench_accurate.py needs a HIP device"
    dev = torch.device("cuda:0")
    depth, off, hdr = synth.synth_batch(n, "crop", seed0=0, threads=8)
    td, to, th = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depth, off, hdr))
    ab = pkg.aabb(td, to, th, res=R)
    assert not ab.status.any()
    grid = torch.cat([ab.ori, ab.grid[:, 4:6], torch.zeros_like(ab.ori)], dim=1)
    out = torch.empty((n, 3, R, R, R), dtype=torch.float32, device=dev)
    nt = min(n, a.torch_frames)
    cam = pkg.default_cam()
    pts = []
    for i in range(nt):
        h = hdr[i]
        d = td[off[i]:off[i + 1]].double()
        k = torch.nonzero(d.abs() >= cam.invalid_eps).flatten()
        bw = int(h[4] - h[2])
        col, row, dd = (h[2] + k % bw).double(), (h[3] + k // bw).double(), d[k]
        pts.append(torch.stack([(col - cam.cx) * dd / cam.focal, -(row - cam.cy) * dd / cam.focal, -dd], dim=1))
    legs = {"grid_accurate": lambda: pkg.voxelize_grid_accurate(td, to, th, grid, res=R, out=out),
            "accurate": lambda: pkg.voxelize_accurate(td, to, th, res=R),
            "grid": lambda: pkg.voxelize_grid(td, to, th, grid, res=R),
            "torch": lambda: torch_accurate(torch, pts, grid[:nt], R)}
    # the torch form names the same pixels (checked once, outside the clock, on the first frame)
    _, _, nn = pkg.voxelize_grid_accurate(td[:off[1]], to[:2], th[:1], grid[:1], res=R, nearest=True)
    p0 = torch.nonzero(td[:off[1]].abs() >= cam.invalid_eps).flatten()
    tn, _ = torch_accurate(torch, pts[:1], grid[:1], R)[0]
    tn = torch.where(tn >= 0, p0[tn.clamp(min=0)], tn)
    agree = float((tn == nn.flatten()).double().mean())
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
    t = {k: dict(us=round(float(np.median(v)), 2), us_min=round(min(v), 2), us_max=round(max(v), 2), iters=iters[k])
         for k, v in times.items()}
    per = {k: t[k]["us"] / (nt if k == "torch" else n) for k in t}
    row = dict(device=torch.cuda.get_device_name(0), n=n, kind="crop", res=R, pixels=int(depth.size), torch_frames=nt,
               torch_agrees_on_nearest=round(agree, 6), **t,
               us_per_frame={k: round(v, 2) for k, v in per.items()},
               accurate_over_projective=round(t["grid_accurate"]["us"] / t["grid"]["us"], 2),
               torch_over_accurate_per_frame=round(per["torch"] / per["grid_accurate"], 2))
    print(json.dumps(row))


def tree(a):
    import numpy as np
    import torch
    pkg = _package(a)
    synth = importlib.import_module("handposeestimation-with-3d-cnns_amd.synth")
    assert torch.cuda.is_available(), "bench_accurate.py needs a HIP device"
    with tempfile.TemporaryDirectory() as tmp:
        db = os.path.join(tmp, "db")
        frames = synth.synth_msra_tree(db, n_sub=1, n_ges=4, n_frames=64, seed=0)
        times = {"projective": [], "accurate": []}
        for r in range(a.rounds + 1):                        # round 0 warms up
            for kind in times:
                t0 = time.perf_counter()
                pkg.export.preprocess_tree(db, os.path.join(tmp, f"{kind}{r}"), point_clouds=False, tsdf=kind,
                                           rng=np.random.default_rng(0))
                if r:
                    times[kind].append(1e3 * (time.perf_counter() - t0))
    t = {"tree_" + k: dict(ms=round(float(np.median(v)), 2), ms_min=round(min(v), 2), ms_max=round(max(v), 2))
         for k, v in times.items()}
    print(json.dumps(dict(frames=frames, gestures=4, res=32, **t,
                          accurate_over_projective=round(t["tree_accurate"]["ms"] / t["tree_projective"]["ms"], 3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--torch-frames", type=int, default=4)
    ap.add_argument("--limit", type=int, default=420, help="seconds per child process")
    ap.add_argument("--one", nargs=2, type=int, metavar=("N", "R"))
    ap.add_argument("--tree", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accurate", "bench_accurate.json"))
    a = ap.parse_args()
    if a.one:
        return one_shape(a.one[0], a.one[1], a)
    if a.tree:
        return tree(a)
    common = ["--iters", str(a.iters), "--rounds", str(a.rounds), "--budget", str(a.budget), "--torch-frames", str(a.torch_frames)]
    common += ["--lib", a.lib] if a.lib else []
    steps = [["--one", str(n), str(R)] for n, R in SHAPES] + [["--tree"]]
    rows, tree_row = [], None
    for step in steps:                                       # one child per step, each under its own limit; stop at the first failure
        r = subprocess.run([sys.executable, os.path.abspath(__file__), *step, *common], capture_output=True, text=True,
                           timeout=a.limit)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            raise SystemExit(f"bench_accurate.py {' '.join(step)} ended with status {r.returncode}")
        row = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(row), file=sys.stderr)
        if step[0] == "--tree":
            tree_row = row
        else:
            rows.append(row)
    device = [row.pop("device") for row in rows][0]
    line = json.dumps(dict(device=device, iters_max=a.iters, rounds=a.rounds, rows=rows, tree=tree_row))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
