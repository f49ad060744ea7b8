#!/usr/bin/env python3
"""What the voxel heatmap training entries cost (one JSON line; ``--out`` also writes it to a file, default
profiles/heatloss/bench_heatloss.json).

Legs, per shape (n frames, J joints, R^3 voxels) and dtype (float32, bfloat16), in the same run:
  loss_fb             heatmap_mse_loss(pred, gt_nor) + .backward()             two launches and a few small torch ops
  loss_fb_torch       what a user writes today: joint_heatmaps(...) + ((pred - heat) ** 2).mean() + .backward()
  loss_fb_torch_free  the same with the targets handed over for free (encoded outside the clock)
  sse                 tsdf_heat_sse_hip alone          against  amax   torch.amax(pred): one read of the same bytes
  sse_grad            tsdf_heat_sse_grad_hip alone     against  neg    torch.neg(pred, out=...): one read plus one write
  soft / soft_grad    tsdf_soft_argmax_hip / tsdf_soft_argmax_grad_hip alone, against the same two floors
  soft_fb             soft_argmax_joints(pred) + an L1 against gt_nor + .backward()
  soft_fb_torch       torch.softmax(beta * pred.view(nJ, -1).float(), 1) times three coordinate vectors, the same L1, and
                      its autograd
and the peak device memory of one forward + backward of the torch form against the fused one
(torch.cuda.max_memory_allocated above what is allocated before it), for the loss and for the soft-argmax,
at (16, 21, 32), (16, 21, 44), (1024, 21, 32) and (64, 21, 64).

Method, that of tools/bench_heatmap.py: inputs resident on the device, a warm-up of every leg, then device events around
back-to-back calls — at most --iters of them, fewer where one call is long (about --budget seconds per timed window, at
least 5) —; the legs of a shape take turns for --rounds rounds and the median round is reported with min and max.  Every
shape runs in a child process of its own under its own time limit (--limit seconds), one after the other, and the first
that fails ends the run: nothing more is started on the device after it.  Without an MI355X the tool fails; it prints no
times.

    python tools/bench_heatloss.py [--iters 100] [--rounds 5] [--limit 300] [--out x.json]
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
SHAPES = ((16, 21, 32), (16, 21, 44), (1024, 21, 32), (64, 21, 64))
SIGMA, BETA = 1.7, 1.0


def _measure(legs, a):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from _timing import timed_us
    iters = {}
    for k, fn in legs.items():                               # warm-up, and how long one call is
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


def _peak(torch, fn):
    """The peak of allocated device memory during one ``fn()`` above what was allocated before it, in bytes."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def one_shape(n, J, R, a):
    import numpy as np
    sys.path.insert(0, ROOT)
    import torch
    pkg = importlib.import_module(PKG)
    V = importlib.import_module(PKG + ".voxelize")
    assert torch.cuda.is_available() and torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950"), \
        "bench_heatloss.py needs an MI355X (gfx950)"
    dev = torch.device("cuda:0")
    L = pkg._lib.load_heatloss()
    rng = np.random.default_rng(0)
    u = torch.from_numpy(rng.uniform(0.1, 0.9, (n, J, 3)).astype(np.float32)).to(dev)
    w = torch.full((n, J), 2.0 / (n * J * R ** 3), device=dev)
    gu = torch.from_numpy(rng.standard_normal((n, J, 3)).astype(np.float32)).to(dev)
    coords = [((torch.arange(R ** 3, device=dev) // d) % R).float() for d in (1, R, R * R)]     # x, y, z under czyx
    row = dict(device=torch.cuda.get_device_name(0), n=n, joints=J, res=R)
    for name, dt, code in (("float32", torch.float32, 0), ("bfloat16", torch.bfloat16, 2)):
        heat = pkg.joint_heatmaps(u, R, SIGMA, dtype=dt)
        pred = (torch.randn((n, J, R, R, R), device=dev) + heat.float()).to(dt).requires_grad_()
        data = pred.detach()
        out = torch.empty_like(data)
        nbytes = data.numel() * data.element_size()
        sse = torch.empty((n, J), dtype=torch.float64, device=dev)
        su = torch.empty((n, J, 3), device=dev)
        stats = torch.empty((n, J, 5), dtype=torch.float64, device=dev)

        def loss_fb():
            pred.grad = None
            pkg.heatmap_mse_loss(pred, u, sigma=SIGMA).backward()

        def loss_fb_torch():
            pred.grad = None
            ((pred - pkg.joint_heatmaps(u, R, SIGMA, dtype=dt)) ** 2).mean().backward()

        def loss_fb_torch_free():
            pred.grad = None
            ((pred - heat) ** 2).mean().backward()

        def soft_fb():
            pred.grad = None
            (pkg.soft_argmax_joints(pred, beta=BETA) - u).abs().sum().backward()

        def soft_torch():
            q = torch.softmax(BETA * pred.view(n * J, -1).float(), 1)
            return ((torch.stack([q @ c for c in coords], dim=1) + 0.5) / R).view(n, J, 3)

        def soft_fb_torch():
            pred.grad = None
            (soft_torch() - u).abs().sum().backward()

        def entry(fn, args, at):
            return lambda: V._call(dev, fn, list(args), at)

        p, o = data.data_ptr(), out.data_ptr()
        legs = {
            "loss_fb": loss_fb, "loss_fb_torch": loss_fb_torch, "loss_fb_torch_free": loss_fb_torch_free,
            "sse": entry(L.tsdf_heat_sse_hip, [p, code, u.data_ptr(), None, n, J, R, SIGMA, 0, None, sse.data_ptr(), None], 9),
            "sse_grad": entry(L.tsdf_heat_sse_grad_hip, [p, code, u.data_ptr(), None, w.data_ptr(), n, J, R, SIGMA, 0, None, o], 10),
            "soft": entry(L.tsdf_soft_argmax_hip, [p, code, n, J, R, BETA, 0, None, su.data_ptr(), stats.data_ptr()], 7),
            "soft_grad": entry(L.tsdf_soft_argmax_grad_hip, [p, code, stats.data_ptr(), gu.data_ptr(), n, J, R, BETA, 0, None, o], 9),
            "soft_fb": soft_fb, "soft_fb_torch": soft_fb_torch,
            "amax": lambda: torch.amax(data), "neg": lambda: torch.neg(data, out=out),
        }
        # the two forms compute one thing
        loss_fb()
        fused_grad = pred.grad.float()
        fused_loss = float(pkg.heatmap_mse_loss(data, u, sigma=SIGMA))
        loss_fb_torch_free()
        agree = dict(loss_rel=abs(fused_loss - float(((data.float() - heat.float()) ** 2).mean())) / fused_loss,
                     grad_largest_difference=float((fused_grad - pred.grad.float()).abs().max()),
                     soft_largest_difference=float((pkg.soft_argmax_joints(data, beta=BETA) - soft_torch().detach()).abs().max()))
        del fused_grad
        pred.grad = None
        peaks = {}
        for k in ("loss_fb", "loss_fb_torch", "loss_fb_torch_free", "soft_fb", "soft_fb_torch"):
            pred.grad = None                                 # every leg starts without a gradient: its peak holds its own
            peaks[k] = _peak(torch, legs[k])
        pred.grad = None
        tm = _measure(legs, a)
        us = {k: v["us"] for k, v in tm.items()}
        tbs = {k: round((2 if k in ("sse_grad", "soft_grad", "neg") else 1) * nbytes / (us[k] * 1e-6) / 1e12, 3)
               for k in ("sse", "sse_grad", "soft", "soft_grad", "amax", "neg")}
        row[name] = dict(bytes=nbytes, agreement=agree, **tm, tb_per_s=tbs, peak_bytes=peaks,
                         torch_over_loss_fb=round(us["loss_fb_torch"] / us["loss_fb"], 2),
                         torch_free_over_loss_fb=round(us["loss_fb_torch_free"] / us["loss_fb"], 2),
                         sse_over_amax=round(us["sse"] / us["amax"], 2), sse_grad_over_neg=round(us["sse_grad"] / us["neg"], 2),
                         torch_over_soft_fb=round(us["soft_fb_torch"] / us["soft_fb"], 2),
                         soft_over_amax=round(us["soft"] / us["amax"], 2), soft_grad_over_neg=round(us["soft_grad"] / us["neg"], 2),
                         torch_peak_over_loss_fb_peak=round(peaks["loss_fb_torch"] / max(peaks["loss_fb"], 1), 2),
                         torch_peak_over_soft_fb_peak=round(peaks["soft_fb_torch"] / max(peaks["soft_fb"], 1), 2))
        del pred, data, out, heat, legs
        torch.cuda.empty_cache()
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--limit", type=int, default=300, help="seconds per child process")
    ap.add_argument("--one", nargs=3, type=int, metavar=("N", "J", "R"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heatloss", "bench_heatloss.json"))
    a = ap.parse_args()
    if a.one:
        return one_shape(*a.one, a)
    common = ["--iters", str(a.iters), "--rounds", str(a.rounds), "--budget", str(a.budget)]
    rows = []
    for n, J, R in SHAPES:                                   # one child per shape, each under its own limit; stop at the first failure
        step = ["--one", str(n), str(J), str(R)]
        r = subprocess.run([sys.executable, os.path.abspath(__file__), *step, *common], capture_output=True, text=True,
                           timeout=a.limit)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            raise SystemExit(f"bench_heatloss.py {' '.join(step)} ended with status {r.returncode}")
        row = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(row), file=sys.stderr)
        rows.append(row)
    device = [row.pop("device") for row in rows][0]
    line = json.dumps(dict(device=device, iters_max=a.iters, rounds=a.rounds, sigma=SIGMA, beta=BETA, rows=rows))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
