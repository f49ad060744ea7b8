#!/usr/bin/env python3
"""What a float16 / bfloat16 volume costs (one JSON line; ``--out`` also writes it to a file, default
profiles/lowp/bench_lowp.json).

Legs, per shape, on the same frames and the same grid rows in the same run:
  grid_f32        voxelize_grid()                 the product's float32 kernel (tsdf_voxelize_grid_hip)
  grid_f32_cast   voxelize_grid() + .to(dtype)    what a user does today: THE YARDSTICK
  grid_lowp       voxelize_grid_lowp()            tsdf_voxelize_grid_lowp_hip, libtsdf_lowp.so
  narrow          narrow_volumes() alone          tsdf_lowp_narrow_hip on a float32 volume that is already there
  cast            .to(dtype) alone                torch's cast of the same volume
at 1024 crops R = 32, 16 crops R = 32 and 256 crops R = 64, bfloat16 (``--dtype float16`` for the other type).

Method: inputs resident on the device, --warmup launches, then device events around --iters back-to-back launches (at
least 50); the legs of a shape take turns for --rounds rounds and the median round is reported with min and max, so a
drift of the machine meets all alike.  The float32 legs allocate their outputs (torch's caching allocator: no device
allocation in the steady state), the low-precision legs write into one buffer.  Bytes written per launch: 12 R^3 n for a
float32 volume, 6 R^3 n for a low-precision one.

``--lib PATH`` times another build of libtsdf_lowp.so (an A/B of a build knob such as -DTSDF_LOWP_STORE_ASM) in the
grid_lowp and narrow legs.

    python tools/bench_lowp.py [--iters 100] [--warmup 20] [--rounds 5] [--dtype bfloat16] [--lib x.so] [--out x.json]
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
    ap.add_argument("--dtype", choices=("bfloat16", "float16"), default="bfloat16")
    ap.add_argument("--lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowp", "bench_lowp.json"))
    a = ap.parse_args()
    assert a.iters >= 50, "time at least 50 launches"
    assert torch.cuda.is_available(), "bench_lowp.py needs a HIP device"
    if a.lib:
        row = pkg._lib._EXTS["lowp"]
        pkg._lib._EXTS["lowp"] = row._replace(path=os.path.abspath(a.lib))
    dev = torch.device("cuda:0")
    dt = getattr(torch, a.dtype)
    rows = []
    for n, R in ((1024, 32), (16, 32), (256, 64)):
        depth, off, hdr = synth.synth_batch(n, "crop", seed0=0, threads=8)
        td, to, th = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depth, off, hdr))
        ab = pkg.aabb(td, to, th, res=R)
        assert not ab.status.any()
        grid = torch.cat([ab.ori, ab.grid[:, 4:6], torch.zeros_like(ab.ori)], dim=1)
        vol32, _ = pkg.voxelize_grid(td, to, th, grid, res=R)
        low = torch.empty(vol32.shape, dtype=dt, device=dev)
        legs = {"grid_f32": lambda: pkg.voxelize_grid(td, to, th, grid, res=R),
                "grid_f32_cast": lambda: pkg.voxelize_grid(td, to, th, grid, res=R)[0].to(dt),
                "grid_lowp": lambda: pkg.voxelize_grid_lowp(td, to, th, grid, res=R, dtype=dt, out=low),
                "narrow": lambda: pkg.narrow_volumes(vol32, dtype=dt, out=low),
                "cast": lambda: vol32.to(dt)}
        t = take_turns(legs, a.iters, a.warmup, a.rounds)
        differ = int((pkg.voxelize_grid_lowp(td, to, th, grid, res=R, dtype=dt)[0].view(torch.int16)
                      != vol32.to(dt).view(torch.int16)).sum())
        low_bytes = 2 * vol32.numel()
        row = dict(n=n, kind="crop", res=R, dtype=a.dtype, pixels=int(depth.size), volume_bytes_f32=2 * low_bytes,
                   volume_bytes_lowp=low_bytes, voxels_differing_from_cast=differ, **t,
                   lowp_over_f32_cast=round(t["grid_lowp"]["us"] / t["grid_f32_cast"]["us"], 3),
                   lowp_over_f32=round(t["grid_lowp"]["us"] / t["grid_f32"]["us"], 3),
                   narrow_over_cast=round(t["narrow"]["us"] / t["cast"]["us"], 3),
                   lowp_write_GBps=round(low_bytes / t["grid_lowp"]["us"] / 1e3, 1),
                   f32_write_GBps=round(2 * low_bytes / t["grid_f32"]["us"] / 1e3, 1))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del td, to, th, ab, grid, vol32, low, legs
        torch.cuda.empty_cache()
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=a.rounds, lib=a.lib, rows=rows))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
