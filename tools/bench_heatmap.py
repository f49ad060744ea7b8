#!/usr/bin/env python3
"""What the voxel heatmap labels cost (one JSON line; ``--out`` also writes it to a file, default
profiles/heatmap/bench_heatmap.json).

Legs, per shape (n frames, J joints, R^3 voxels) and dtype (float32, bfloat16), in the same run:
  encode        joint_heatmaps()                  one launch (libtsdf_heatmap.so)
  encode_torch  the torch form a user writes today: the three per-axis tables handed over for free (float64, computed
                outside the clock), a broadcast product, .to(dtype) — the yardstick; it leaves out the flush below 2^-126,
                so its values are the library's only down to there
  encode_torch_flush   the same with the flush (one torch.where over the float64 product): the library's bits
  fill          out.zero_() of the same bytes: the write floor
  decode        heatmap_joints(radius=0)          one launch
  decode_r2     heatmap_joints(radius=2)
  decode_torch  heat.view(n J, -1).max(dim=1) plus the index arithmetic
  amax          torch.amax of the same tensor: the read floor
at (16, 21, 32), (16, 21, 44), (1024, 21, 32) and (64, 21, 64); and at batch 16 and 1024, R = 32, bfloat16, heatmap 32^3,
  step / step_heatmap    AugmentedStep.step() replayed from its graph, without and with heatmap=(32, 1.7, bfloat16).

Method: inputs resident on the device, a warm-up of every leg, then device events around back-to-back launches — at most
--iters of them, fewer where one launch is long (about --budget seconds per timed window, at least 5) —; the legs of a shape
take turns for --rounds rounds and the median round is reported with min and max.  Every shape runs in a child process of
its own under its own time limit (--limit seconds), one after the other, and the first that fails ends the run: nothing
more is started on the device after it.  Without an MI355X the tool fails; it prints no times.

    python tools/bench_heatmap.py [--iters 100] [--rounds 5] [--limit 300] [--out x.json]
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
STEP_BATCHES = (16, 1024)
SIGMA = 1.7
PEAK_TBS = 8.0     # the HBM peak the shares are quoted against
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


def _setup():
    import torch
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    assert torch.cuda.is_available() and torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950"), \
        "bench_heatmap.py needs an MI355X (gfx950)"
    return pkg, torch, torch.device("cuda:0")


def one_shape(n, J, R, a):
    import numpy as np
    pkg, torch, dev = _setup()
    u = torch.from_numpy(np.random.default_rng(0).uniform(0.1, 0.9, (n, J, 3)).astype(np.float32)).to(dev)
    # the torch form's tables, for free: g[a] float64[n, J, R]
    c = u.double() * R - 0.5
    t = torch.arange(R, dtype=torch.float64, device=dev) - c[..., None]
    g = torch.exp(-((t * t) * (1.0 / (2.0 * float(np.float32(SIGMA)) ** 2))))
    gx, gy, gz = g[:, :, 0], g[:, :, 1], g[:, :, 2]
    row = dict(device=torch.cuda.get_device_name(0), n=n, joints=J, res=R)
    for name, dt in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
        out = torch.empty((n, J, R, R, R), dtype=dt, device=dev)
        nbytes = out.numel() * out.element_size()

        def encode_torch():
            return ((gz[:, :, :, None, None] * gy[:, :, None, :, None]) * gx[:, :, None, None, :]).to(dt)

        def encode_torch_flush():
            p = (gz[:, :, :, None, None] * gy[:, :, None, :, None]) * gx[:, :, None, None, :]
            return torch.where(p < 2.0 ** -126, 0.0, p).to(dt)

        heat = pkg.joint_heatmaps(u, R, SIGMA, dtype=dt)
        same = float((encode_torch_flush().float() - heat.float()).abs().max())    # the two forms compute one thing
        flat = heat.view(n * J, -1)

        def decode_torch():
            peak, arg = flat.max(dim=1)
            idx = torch.stack([arg % R, (arg // R) % R, arg // (R * R)], dim=1)
            return ((idx.double() + 0.5) / R).float(), peak

        ref_u = decode_torch()[0].view(n, J, 3)
        agree = bool(torch.equal(pkg.heatmap_joints(heat).u, ref_u))
        legs = {"encode": lambda: pkg.joint_heatmaps(u, R, SIGMA, dtype=dt, out=out), "encode_torch": encode_torch,
                "encode_torch_flush": encode_torch_flush,
                "fill": lambda: out.zero_(), "decode": lambda: pkg.heatmap_joints(heat),
                "decode_r2": lambda: pkg.heatmap_joints(heat, radius=2), "decode_torch": decode_torch,
                "amax": lambda: torch.amax(flat, dim=1)}
        tm = _measure(legs, a)
        tbs = {k: round(nbytes / (tm[k]["us"] * 1e-6) / 1e12, 3) for k in ("encode", "fill", "decode", "amax")}
        row[name] = dict(bytes=nbytes, encode_torch_largest_difference=same, decode_agrees_with_torch=agree, **tm, tb_per_s=tbs,
                         encode_share_of_peak=round(tbs["encode"] / PEAK_TBS, 3),
                         encode_over_fill=round(tm["encode"]["us"] / tm["fill"]["us"], 3),
                         torch_over_encode=round(tm["encode_torch"]["us"] / tm["encode"]["us"], 2),
                         torch_flush_over_encode=round(tm["encode_torch_flush"]["us"] / tm["encode"]["us"], 2),
                         decode_over_amax=round(tm["decode"]["us"] / tm["amax"]["us"], 3),
                         torch_over_decode=round(tm["decode_torch"]["us"] / tm["decode"]["us"], 2))
        del out, heat, flat
    print(json.dumps(row))


def one_step(n, a):
    import numpy as np
    pkg, torch, dev = _setup()
    synth = importlib.import_module(PKG + ".synth")
    R, J = 32, 21
    depth, off, hdr = synth.synth_batch(n, "crop", seed0=0, threads=8)
    td, to, th = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depth, off, hdr))
    ab = pkg.aabb(td, to, th, res=R)
    centres = ab.grid[:, :3].contiguous()
    noise = torch.from_numpy(np.random.default_rng(1).normal(0, 40, (n, J, 3)).astype(np.float32)).to(dev)
    gt = (centres[:, None, :] + noise).reshape(n, 3 * J).contiguous()
    index = torch.arange(n, dtype=torch.int64, device=dev)
    kw = dict(gt=gt, centres=centres, res=R, dtype=torch.bfloat16)
    steps = {"step": pkg.AugmentedStep(td, to, th, n, **kw),
             "step_heatmap": pkg.AugmentedStep(td, to, th, n, heatmap=(32, SIGMA, torch.bfloat16), **kw)}
    counter = [0]

    def leg(s):
        def fn():
            counter[0] += n
            s.step(index, KEY, counter[0])
        return fn
    t = _measure({k: leg(s) for k, s in steps.items()}, a)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), n=n, res=R, heatmap_res=32, **t,
                          heatmap_adds_us=round(t["step_heatmap"]["us"] - t["step"]["us"], 2),
                          with_over_without=round(t["step_heatmap"]["us"] / t["step"]["us"], 3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--limit", type=int, default=300, help="seconds per child process")
    ap.add_argument("--one", nargs=3, type=int, metavar=("N", "J", "R"))
    ap.add_argument("--step", type=int, metavar="N")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heatmap", "bench_heatmap.json"))
    a = ap.parse_args()
    if a.one:
        return one_shape(*a.one, a)
    if a.step:
        return one_step(a.step, a)
    common = ["--iters", str(a.iters), "--rounds", str(a.rounds), "--budget", str(a.budget)]
    todo = [["--one", str(n), str(J), str(R)] for n, J, R in SHAPES] + [["--step", str(n)] for n in STEP_BATCHES]
    rows, steps = [], []
    for step in todo:                                        # one child per step, each under its own limit; stop at the first failure
        r = subprocess.run([sys.executable, os.path.abspath(__file__), *step, *common], capture_output=True, text=True,
                           timeout=a.limit)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            raise SystemExit(f"bench_heatmap.py {' '.join(step)} ended with status {r.returncode}")
        row = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(row), file=sys.stderr)
        (rows if step[0] == "--one" else steps).append(row)
    device = [row.pop("device") for row in rows + steps][0]
    line = json.dumps(dict(device=device, iters_max=a.iters, rounds=a.rounds, sigma=SIGMA, rows=rows, steps=steps))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
