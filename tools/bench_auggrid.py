#!/usr/bin/env python3
"""What the augmented voxelization on a caller-supplied grid costs (one JSON line; ``--out`` also writes it to a file).

Kernel legs — the same frames and maps, only the grid placement differs (the fused entry places its own grid on all
mapped valid pixels, the stand-alone entry is handed the grid of a 6000-point resample of the mapped cloud):
  fused      voxelize_aug          (tsdf_voxelize_aug_hip, libtsdf_hip.so: phase 1 + placement + voxel pass in one launch)
  auggrid    voxelize_aug_grid     (tsdf_voxelize_aug_grid_hip, libtsdf_auggrid.so: the voxel pass alone)
at 1024 crops R = 32, 16 crops R = 32 and 1024 crops R = 64.
Pipeline legs at 16 and 1024 crops, R = 32, 6000 points:
  process_batch       point_clouds -> cloud_grids -> voxelize_grid
  process_batch_aug   the same plus aug_xforms -> point_clouds(xforms) -> cloud_grids -> voxelize_aug_grid

Method: inputs resident on the device, --warmup launches, then device events around --iters back-to-back launches (at
least 50); the legs of a shape take turns for --rounds rounds and the median round is reported with min and max, so a
drift of the machine meets both alike.  The wrappers allocate their outputs (torch's caching allocator: no device
allocation in the steady state).  Bytes written per launch: n * 3 * R^3 * 4.

    python tools/bench_auggrid.py [--iters 100] [--warmup 20] [--rounds 5] [--out x.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("handposeestimation-with-3d-cnns_amd")
synth = importlib.import_module("handposeestimation-with-3d-cnns_amd.synth")
from _timing import take_turns  # noqa: E402  (tools/_timing.py, beside this file)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.iters >= 50, "time at least 50 launches"
    assert torch.cuda.is_available(), "bench_auggrid.py needs a HIP device"
    dev = torch.device("cuda:0")
    depth, off, hdr = synth.synth_batch(1024, "crop", seed0=0, threads=8)
    rows = []
    for n, R in ((1024, 32), (16, 32), (1024, 64)):
        td, to, th = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depth[:off[n]], off[:n + 1], hdr[:n]))
        centres = pkg.aabb(td, to, th, res=R).grid[:, :3].contiguous()
        xf = pkg.aug_xforms(centres, key=1)
        grid = pkg.cloud_grids(pkg.point_clouds(td, to, th, points=6000, xforms=xf).points, res=R).grid
        st = pkg.voxelize_aug_grid(td, to, th, xf, grid, res=R)[1]
        assert not st.any()
        legs = {"fused": lambda: pkg.voxelize_aug(td, to, th, xf, res=R),
                "auggrid": lambda: pkg.voxelize_aug_grid(td, to, th, xf, grid, res=R)}
        t = take_turns(legs, a.iters, a.warmup, a.rounds)
        out_bytes = n * 3 * R ** 3 * 4
        row = dict(kind="kernel", n=n, res=R, out_bytes=out_bytes, **{k: v for k, v in t.items()},
                   auggrid_over_fused=round(t["auggrid"]["us"] / t["fused"]["us"], 3),
                   auggrid_write_GBps=round(out_bytes / t["auggrid"]["us"] / 1e3, 1),
                   fused_write_GBps=round(out_bytes / t["fused"]["us"] / 1e3, 1))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        if R == 32:
            legs = {"process_batch": lambda: pkg.process_batch(td, to, th, points=6000, res=R),
                    "process_batch_aug": lambda: pkg.process_batch_aug(td, to, th, points=6000, res=R)}
            t = take_turns(legs, a.iters, a.warmup, a.rounds)
            row = dict(kind="pipeline", n=n, res=R, points=6000, **{k: v for k, v in t.items()},
                       aug_over_plain=round(t["process_batch_aug"]["us"] / t["process_batch"]["us"], 3))
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
        del td, to, th, centres, xf, grid
        torch.cuda.empty_cache()
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=a.rounds, rows=rows))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
