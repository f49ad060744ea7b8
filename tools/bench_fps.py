#!/usr/bin/env python3
"""What the farthest-point sampled clouds cost (one JSON line; ``--out`` also writes it to a file, default
profiles/fps/bench_fps.json).

Legs, per shape (n frames of ``synth_frame(kind="crop")``, M samples), in the same run:
  fps            farthest_points() with a workspace: frames up to the resident cap run resident, the others stream
  fps_mapped     the same under obb_xforms()' maps
  fps_streaming  form=1: every frame through the workspace
  of_clouds      farthest_of() on point_clouds(6000) output, float64[n, 6000, 3]
  torch          the torch form a user writes today: M - 1 dependent iterations over the batch's clouds padded to the
                 longest, float32[n, P, 3] — broadcast difference, squared sum, minimum, argmax, gather.  The padded
                 clouds and their mask come for free (made outside the clock).  ``torch_differs`` counts the positions
                 whose selected points are not the library's (it resolves ties as argmax does, and a padded row can win)
at n = 16 and 1024, M = 128 and 1024; then, at batch 16 and 1024, R = 32, bfloat16,
  step / step_fps    AugmentedStep.step() replayed from its graph, without and with fps=(1024,);
and with --wg 256 512 1024 the fps leg of (16, 1024) and (1024, 1024) from build/libtsdf_fps_wgN.so (make fps-variants).
``resident_share`` is the share of crop seeds 0..255 whose candidates fit the resident cap.

Method: inputs resident on the device, a warm-up of every leg, then device events around back-to-back launches — at most
--iters of them, fewer where one launch is long (about --budget seconds per timed window, at least 3) —; the legs of a shape
take turns for --rounds rounds and the median round is reported with min and max.  Every shape runs in a child process of
its own under its own time limit (--limit seconds), one after the other, and the first that fails ends the run: nothing
more is started on the device after it.  Without an MI355X the tool fails; it prints no times.

    python tools/bench_fps.py [--iters 50] [--rounds 5] [--limit 400] [--wg 256 512 1024] [--out x.json]
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
SHAPES = ((16, 128), (16, 1024), (1024, 128), (1024, 1024))
STEP_BATCHES = (16, 1024)
WG_SHAPES = ((16, 1024), (1024, 1024))
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
        iters[k] = int(min(a.iters, max(3, a.budget / max(one, 1e-6))))
    times = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            times[k].append(timed_us(fn, iters[k]))
    return {k: dict(us=round(float(np.median(v)), 2), us_min=round(min(v), 2), us_max=round(max(v), 2), iters=iters[k])
            for k, v in times.items()}


def _setup(wg=0):
    import torch
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    assert torch.cuda.is_available() and torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950"), \
        "bench_fps.py needs an MI355X (gfx950)"
    if wg:   # an experiment's build of the same library: another workgroup size
        pkg._lib._FPS = pkg._lib._FPS._replace(path=os.path.join(ROOT, "build", f"libtsdf_fps_wg{wg}.so"))
    return pkg, torch, torch.device("cuda:0")


def _pack(pkg, torch, dev, n):
    import numpy as np
    synth = importlib.import_module(PKG + ".synth")
    depth, off, hdr = synth.synth_batch(n, "crop", seed0=0, threads=8)
    t = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depth, off, hdr))
    return (depth, off, hdr), t


def one_shape(n, M, a):
    import numpy as np
    pkg, torch, dev = _setup()
    (depth, off, hdr), t = _pack(pkg, torch, dev, n)
    counts = pkg.farthest_points(*t, points=1).count.cpu()
    cap = int(counts.max())
    resident = pkg.FPS_RESIDENT_POINTS
    work = torch.empty((n, cap, 4), device=dev)
    out = pkg.farthest_points(*t, points=M, work=work)
    assert not out.status.any()
    xf = pkg.obb_xforms(*t).xforms
    clouds = pkg.point_clouds(*t, points=6000, seed=1).points
    out_c = pkg.farthest_of(clouds, points=M)
    # the torch form's inputs, for free: the candidates of every frame in rank order (the contract's float64
    # back-projection, rounded once), padded to the longest
    padded = np.zeros((n, cap, 3), np.float32)
    valid = np.zeros((n, cap), bool)
    for i in range(n):
        left, top, right, bottom = (int(v) for v in hdr[i, 2:6])
        d = depth[off[i]:off[i + 1]].reshape(bottom - top, right - left)
        r, c = np.nonzero(np.abs(d) >= 1.0)
        d64 = d[r, c].astype(np.float64)
        q = d64 / 241.42
        p = np.stack([q * ((left + c) - 160.0), -(q * ((top + r) - 120.0)), -d64], 1).astype(np.float32)
        assert len(p) == int(counts[i])
        padded[i, :len(p)], valid[i, :len(p)] = p, True
    padded, mask = torch.from_numpy(padded).to(dev), torch.from_numpy(valid).to(dev)
    rows = torch.arange(n, device=dev)
    minus = torch.where(mask, torch.tensor(float("inf"), device=dev), torch.tensor(-1.0, device=dev))   # padding never wins

    def torch_form():
        dist = minus.clone()
        sel = torch.empty((n, M, 3), device=dev)
        s = padded[:, 0]
        sel[:, 0] = s
        for j in range(1, M):
            d = ((padded - s[:, None, :]) ** 2).sum(-1)
            dist = torch.minimum(dist, d)
            s = padded[rows, dist.argmax(1)]
            sel[:, j] = s
        return sel

    differs = int((torch_form().view(torch.int32) != out.points.view(torch.int32)).any(-1).any(-1).sum())
    legs = {"fps": lambda: pkg.farthest_points(*t, points=M, work=work, out=out),
            "fps_mapped": lambda: pkg.farthest_points(*t, points=M, work=work, out=out, xforms=xf),
            "fps_streaming": lambda: pkg.farthest_points(*t, points=M, work=work, out=out, form=1),
            "of_clouds": lambda: pkg.farthest_of(clouds, points=M, out=out_c),
            "torch": torch_form}
    tm = _measure(legs, a)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), n=n, M=M, pixels=int(t[0].numel()),
                          candidates=int(counts.sum()), longest=cap, streamed_frames=int((counts > resident).sum()),
                          torch_differs=differs, **tm,
                          us_per_iteration={k: round(v["us"] / max(M - 1, 1), 3) for k, v in tm.items()},
                          torch_over_fps=round(tm["torch"]["us"] / tm["fps"]["us"], 2),
                          streaming_over_fps=round(tm["fps_streaming"]["us"] / tm["fps"]["us"], 2),
                          mapped_over_plain=round(tm["fps_mapped"]["us"] / tm["fps"]["us"], 3))))


def one_wg(wg, n, M, a):
    pkg, torch, dev = _setup(wg)
    _, t = _pack(pkg, torch, dev, n)
    cap = int(pkg.farthest_points(*t, points=1).count.max())
    work = torch.empty((n, cap, 4), device=dev)
    out = pkg.farthest_points(*t, points=M, work=work)
    tm = _measure({"fps": lambda: pkg.farthest_points(*t, points=M, work=work, out=out)}, a)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), wg=wg, n=n, M=M, **tm)))


def one_step(n, a):
    import numpy as np
    pkg, torch, dev = _setup()
    R, J = 32, 21
    _, (td, to, th) = _pack(pkg, torch, dev, n)
    ab = pkg.aabb(td, to, th, res=R)
    centres = ab.grid[:, :3].contiguous()
    noise = torch.from_numpy(np.random.default_rng(1).normal(0, 40, (n, J, 3)).astype(np.float32)).to(dev)
    gt = (centres[:, None, :] + noise).reshape(n, 3 * J).contiguous()
    index = torch.arange(n, dtype=torch.int64, device=dev)
    kw = dict(gt=gt, centres=centres, res=R, dtype=torch.bfloat16)
    steps = {"step": pkg.AugmentedStep(td, to, th, n, **kw),
             "step_fps": pkg.AugmentedStep(td, to, th, n, fps=(1024,), **kw)}
    counter = [0]

    def leg(s):
        def fn():
            counter[0] += n
            s.step(index, KEY, counter[0])
        return fn
    t = _measure({k: leg(s) for k, s in steps.items()}, a)
    over = int((steps["step_fps"].cloud_status == 3).sum())
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), n=n, res=R, fps_points=1024, over_capacity=over, **t,
                          fps_adds_us=round(t["step_fps"]["us"] - t["step"]["us"], 2),
                          with_over_without=round(t["step_fps"]["us"] / t["step"]["us"], 3))))


def resident_share():
    """The share of ``synth_frame(kind="crop")`` seeds 0..255 whose candidates fit the resident cap (host arithmetic)."""
    import numpy as np
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    depth, off, _ = synth.synth_batch(256, "crop", seed0=0, threads=8)
    valid = np.add.reduceat(np.abs(depth) >= 1.0, off[:-1])
    cap = pkg.FPS_RESIDENT_POINTS
    return dict(resident_cap=cap, seeds=256, fit=int((valid <= cap).sum()), share=round(float((valid <= cap).mean()), 4),
                median_candidates=int(np.median(valid)), max_candidates=int(valid.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--limit", type=int, default=400, help="seconds per child process")
    ap.add_argument("--one", nargs=2, type=int, metavar=("N", "M"))
    ap.add_argument("--one-wg", nargs=3, type=int, metavar=("WG", "N", "M"))
    ap.add_argument("--step", type=int, metavar="N")
    ap.add_argument("--wg", nargs="*", type=int, default=[], help="also time build/libtsdf_fps_wgN.so for these N")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps", "bench_fps.json"))
    a = ap.parse_args()
    if a.one:
        return one_shape(*a.one, a)
    if a.one_wg:
        return one_wg(*a.one_wg, a)
    if a.step:
        return one_step(a.step, a)
    common = ["--iters", str(a.iters), "--rounds", str(a.rounds), "--budget", str(a.budget)]
    todo = [["--one", str(n), str(M)] for n, M in SHAPES] + [["--step", str(n)] for n in STEP_BATCHES] + \
           [["--one-wg", str(wg), str(n), str(M)] for n, M in WG_SHAPES for wg in a.wg]
    got = {"--one": [], "--step": [], "--one-wg": []}
    for step in todo:                                        # one child per step, each under its own limit; stop at the first failure
        r = subprocess.run([sys.executable, os.path.abspath(__file__), *step, *common], capture_output=True, text=True,
                           timeout=a.limit)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            raise SystemExit(f"bench_fps.py {' '.join(step)} ended with status {r.returncode}")
        row = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(row), file=sys.stderr)
        got[step[0]].append(row)
    device = [row.pop("device") for rows in got.values() for row in rows][0]
    line = json.dumps(dict(device=device, iters_max=a.iters, rounds=a.rounds, resident=resident_share(), rows=got["--one"],
                           steps=got["--step"], workgroups=got["--one-wg"]))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
