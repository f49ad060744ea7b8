#!/usr/bin/env python3
"""What the occupancy volumes cost (one JSON line; ``--out`` also writes it to a file, default
profiles/occupancy/bench_occupancy.json).

Legs, per shape (n frames of ``synth_frame(kind="crop")``, R^3 voxels) and dtype (float32, bfloat16), in the same run:
  occupancy         occupancy_volumes() on aabb()'s cubes                       one launch (libtsdf_occupancy.so)
  occupancy_mapped  the same under drawn augmentation maps, on map_grids()'s cubes
  fill              out.zero_() of the same bytes: the store floor
  aabb              aabb() over the same pack: one read of the crop, the read side's yardstick
  torch             the torch form a user writes today: back-projection of every pixel in float64, floor, and
                    index_put_ of ones into a zeroed volume; the pixel coordinates, the frame number of every pixel and
                    the grids come for free (computed outside the clock).  It has no skin rule, so it may lose a frame's
                    outermost pixels: ``torch_differs`` counts the voxels in which it is not the library's volume
at 16 x 32^3, 16 x 88^3, 1024 x 32^3 and 256 x 88^3; and at batch 16 and 1024, R = 32, bfloat16,
  step / step_occupancy    AugmentedStep.step() replayed from its graph, without and with occupancy=(88, bfloat16).

Method: inputs resident on the device, a warm-up of every leg, then device events around back-to-back launches — at most
--iters of them, fewer where one launch is long (about --budget seconds per timed window, at least 5) —; the legs of a shape
take turns for --rounds rounds and the median round is reported with min and max.  Every shape runs in a child process of
its own under its own time limit (--limit seconds), one after the other, and the first that fails ends the run: nothing
more is started on the device after it.  Without an MI355X the tool fails; it prints no times.

    python tools/bench_occupancy.py [--iters 100] [--rounds 5] [--limit 300] [--out x.json]
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
SHAPES = ((16, 32), (16, 88), (1024, 32), (256, 88))
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


def _setup():
    import torch
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    assert torch.cuda.is_available() and torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950"), \
        "bench_occupancy.py needs an MI355X (gfx950)"
    return pkg, torch, torch.device("cuda:0")


def _pack(pkg, torch, dev, n):
    import numpy as np
    synth = importlib.import_module(PKG + ".synth")
    depth, off, hdr = synth.synth_batch(n, "crop", seed0=0, threads=8)
    t = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depth, off, hdr))
    return (depth, off, hdr), t


def one_shape(n, R, a):
    import numpy as np
    pkg, torch, dev = _setup()
    (depth, off, hdr), t = _pack(pkg, torch, dev, n)
    ab = pkg.aabb(*t, res=R)
    max_l, mid_p = ab.grid[:, 3].contiguous(), ab.grid[:, :3].contiguous()
    xf = pkg.aug_xforms(mid_p, key=KEY)
    place = pkg.map_grids(*t, xf, res=R)
    # the torch form's inputs, for free: per pixel its frame, column and row; per frame the grid
    sizes = np.diff(off)
    fid = torch.from_numpy(np.repeat(np.arange(n), sizes)).to(dev)
    bw = (hdr[:, 4] - hdr[:, 2]).astype(np.int64)
    local = np.arange(len(depth), dtype=np.int64) - np.repeat(off[:-1], sizes)
    xs = torch.from_numpy((np.repeat(hdr[:, 2], sizes) + local % np.repeat(bw, sizes)).astype(np.float64) - 160.0).to(dev)
    ys = torch.from_numpy((np.repeat(hdr[:, 3], sizes) + local // np.repeat(bw, sizes)).astype(np.float64) - 120.0).to(dev)
    vl = max_l / R
    ori = ((mid_p - (max_l / 2)[:, None]) + (vl / 2)[:, None]).double()[fid]                  # [pixels, 3]
    iv = (1.0 / vl.double())[fid]
    row = dict(device=torch.cuda.get_device_name(0), n=n, res=R, pixels=int(len(depth)))
    for name, dt in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
        out = torch.empty((n, 1, R, R, R), dtype=dt, device=dev)
        nbytes = out.numel() * out.element_size()
        one = torch.ones((), dtype=dt, device=dev)

        def torch_form():
            d = t[0]
            d64 = d.double()
            q = d64 / 241.42
            p = torch.stack([q * xs, -(q * ys), -d64], dim=1)
            k = torch.floor((p - ori) * iv[:, None] + 0.5)
            inside = (d.abs() >= 1.0) & ((k >= 0) & (k < R)).all(dim=1)
            k = k[inside].long()
            lin = ((fid[inside] * R + k[:, 2]) * R + k[:, 1]) * R + k[:, 0]
            vol = torch.zeros((n, 1, R, R, R), dtype=dt, device=dev)
            vol.view(-1).index_put_((lin,), one)
            return vol

        occ, _ = pkg.occupancy_volumes(*t, max_l, mid_p, res=R, dtype=dt)
        differs = int((torch_form() != occ).sum())
        legs = {"occupancy": lambda: pkg.occupancy_volumes(*t, max_l, mid_p, res=R, dtype=dt, out=out),
                "occupancy_mapped": lambda: pkg.occupancy_volumes(*t, place.max_l, place.mid_p, res=R, dtype=dt, xforms=xf, out=out),
                "fill": lambda: out.zero_(), "aabb": lambda: pkg.aabb(*t, res=R), "torch": torch_form}
        tm = _measure(legs, a)
        floor = tm["fill"]["us"] + tm["aabb"]["us"]
        row[name] = dict(bytes=nbytes, occupied=int((occ != 0).sum()), torch_differs=differs, **tm,
                         tb_per_s={k: round(nbytes / (tm[k]["us"] * 1e-6) / 1e12, 3) for k in ("occupancy", "fill")},
                         occupancy_over_fill_plus_aabb=round(tm["occupancy"]["us"] / floor, 3),
                         mapped_over_plain=round(tm["occupancy_mapped"]["us"] / tm["occupancy"]["us"], 3),
                         torch_over_occupancy=round(tm["torch"]["us"] / tm["occupancy"]["us"], 2))
        del out, occ
    print(json.dumps(row))


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
             "step_occupancy": pkg.AugmentedStep(td, to, th, n, occupancy=(88, torch.bfloat16), **kw)}
    counter = [0]

    def leg(s):
        def fn():
            counter[0] += n
            s.step(index, KEY, counter[0])
        return fn
    t = _measure({k: leg(s) for k, s in steps.items()}, a)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), n=n, res=R, occupancy_res=88, **t,
                          occupancy_adds_us=round(t["step_occupancy"]["us"] - t["step"]["us"], 2),
                          with_over_without=round(t["step_occupancy"]["us"] / t["step"]["us"], 3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--limit", type=int, default=300, help="seconds per child process")
    ap.add_argument("--one", nargs=2, type=int, metavar=("N", "R"))
    ap.add_argument("--step", type=int, metavar="N")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occupancy", "bench_occupancy.json"))
    a = ap.parse_args()
    if a.one:
        return one_shape(*a.one, a)
    if a.step:
        return one_step(a.step, a)
    common = ["--iters", str(a.iters), "--rounds", str(a.rounds), "--budget", str(a.budget)]
    todo = [["--one", str(n), str(R)] for n, R in SHAPES] + [["--step", str(n)] for n in STEP_BATCHES]
    rows, steps = [], []
    for step in todo:                                        # one child per step, each under its own limit; stop at the first failure
        r = subprocess.run([sys.executable, os.path.abspath(__file__), *step, *common], capture_output=True, text=True,
                           timeout=a.limit)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            raise SystemExit(f"bench_occupancy.py {' '.join(step)} ended with status {r.returncode}")
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
