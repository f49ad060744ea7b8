#!/usr/bin/env python3
"""What the principal-axis maps cost (one JSON line; ``--out`` also writes it to a file).

Legs, per shape, on the same frames in the same run:
  aabb           aabb()          (tsdf_aabb_hip: phase 1 alone, ONE read of the crop — the yardstick of a moments pass)
  obb_xforms     obb_xforms()    (tsdf_obb_xforms_hip, libtsdf_obb.so: two reads of the crop, the second from L2, two
                                 float64 divisions per valid pixel, then one lane's Jacobi)
  voxelize_aug   voxelize_aug()  with ready maps (tsdf_voxelize_aug_hip)
  voxelize_obb   voxelize_obb()  obb_xforms + voxelize_aug on one stream
at 1024 full frames, 1024 crops and 16 crops, R = 32.

Method: inputs resident on the device, --warmup launches, then device events around --iters back-to-back launches (at
least 50); the legs of a shape take turns for --rounds rounds and the median round is reported with min and max, so a
drift of the machine meets all alike.  The wrappers allocate their outputs (torch's caching allocator: no device
allocation in the steady state).  Bytes read per launch of a one-read pass: 4 * pixels.

``--lib PATH`` times another build of libtsdf_obb.so (an A/B of two builds) in the obb_xforms and voxelize_obb legs.

    python tools/bench_obb.py [--iters 100] [--warmup 20] [--rounds 5] [--lib x.so] [--out x.json]
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
    ap.add_argument("--lib")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.iters >= 50, "time at least 50 launches"
    assert torch.cuda.is_available(), "bench_obb.py needs a HIP device"
    if a.lib:
        row = pkg._lib._EXTS["obb"]
        pkg._lib._EXTS["obb"] = row._replace(path=os.path.abspath(a.lib))
    dev = torch.device("cuda:0")
    R = 32
    rows = []
    for n, kind in ((1024, "full"), (1024, "crop"), (16, "crop")):
        depth, off, hdr = synth.synth_batch(n, kind, seed0=0, threads=8)
        td, to, th = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depth, off, hdr))
        ob = pkg.obb_xforms(td, to, th)
        assert not ob.status.any()
        xf = ob.xforms
        legs = {"aabb": lambda: pkg.aabb(td, to, th, res=R),
                "obb_xforms": lambda: pkg.obb_xforms(td, to, th),
                "voxelize_aug": lambda: pkg.voxelize_aug(td, to, th, xf, res=R),
                "voxelize_obb": lambda: pkg.voxelize_obb(td, to, th, res=R)}
        t = take_turns(legs, a.iters, a.warmup, a.rounds)
        read_bytes = 4 * int(depth.size)
        row = dict(n=n, kind=kind, res=R, pixels=int(depth.size), valid=int(ob.count.sum().item()), read_bytes=read_bytes, **t,
                   obb_over_aabb=round(t["obb_xforms"]["us"] / t["aabb"]["us"], 3),
                   voxelize_obb_over_aug=round(t["voxelize_obb"]["us"] / t["voxelize_aug"]["us"], 3),
                   aabb_read_GBps=round(read_bytes / t["aabb"]["us"] / 1e3, 1),
                   obb_read_GBps=round(read_bytes / t["obb_xforms"]["us"] / 1e3, 1))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del td, to, th, ob, xf
        torch.cuda.empty_cache()
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=a.rounds, rows=rows))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
