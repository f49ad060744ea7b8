#!/usr/bin/env python3
"""What drawing the augmentation on the GPU is worth at the reference's batch size (one JSON line; ``--out`` also
writes it to a file).

  loaders  ResidentLoader(batch_size=16, res=32, shuffle=True) over one synthetic pack-backed subject with
           augment=True (maps drawn by numpy on the host), augment="device" (tsdf_aug_draw_hip) and augment=False, each
           at prefetch=1 and prefetch=64: crops/s over a whole epoch (host clock around the epoch, ended by a device
           synchronise), median of --epochs epochs after one warm-up epoch, with min and max.  The six loaders take
           turns epoch by epoch, so a drift of the machine meets all of them alike.
  kernel   the bare aug_xforms launch at n = 16 and 1024 into a preallocated buffer: GPU time per launch (events around
           a run of launches, median of --reps runs after a warm-up) and the host time of one call (enqueue only).
  voxelizer  where an augmented step's time goes besides the draw: voxelize_indexed at n = 16 and 1024 frames of the same
           subject into preallocated outputs, without maps and with resident maps, timed the same way.

    python tools/bench_aug_draw.py [--frames 2048] [--epochs 5] [--iters 200] [--reps 5] [--out bench_aug_draw.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("handposeestimation-with-3d-cnns_amd")
synth = importlib.import_module("handposeestimation-with-3d-cnns_amd.synth")


def make_subject(frames: int):
    """One synthetic MSRA subject (8 gestures), packed."""
    tmp = tempfile.mkdtemp(prefix="bench_aug_")
    try:
        db = os.path.join(tmp, "db")
        total = synth.synth_msra_tree(db, n_sub=1, n_ges=8, n_frames=max(1, frames // 8), seed=3)
        pk = pkg.packing.pack_subject(os.path.join(db, "P0"))
        assert len(pk) == total      # (held in memory: the tree can go)
        return pkg.MSRADepthDataset.from_packs([pk]), total
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def epoch_seconds(loader) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in loader:
        pass
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def loader_rows(ds, frames: int, epochs: int):
    dev = torch.device("cuda:0")
    loaders = {}
    for prefetch in (1, 64):
        for mode in (True, "device", False):
            loaders[(repr(mode), prefetch)] = pkg.ResidentLoader(ds, batch_size=16, device=dev, res=32, shuffle=True,
                                                                 augment=mode, prefetch=prefetch)
    times = {k: [] for k in loaders}
    for e in range(epochs + 1):              # epoch 0 warms up: upload, code objects, ring buffers
        for k, ld in loaders.items():
            t = epoch_seconds(ld)
            if e:
                times[k].append(t)
    rows = []
    for (mode, prefetch), ts in times.items():
        rate = sorted(frames / t for t in ts)
        rows.append(dict(augment=mode, prefetch=prefetch, batch_size=16, res=32, frames=frames, epochs=len(ts),
                         crops_per_s=round(float(np.median(rate))), crops_per_s_min=round(rate[0]),
                         crops_per_s_max=round(rate[-1]),
                         us_per_batch=round(1e6 * float(np.median(ts)) / (-(-frames // 16)), 1)))
        print(json.dumps(rows[-1]), file=sys.stderr)
    return rows


def kernel_rows(iters: int, reps: int):
    dev = torch.device("cuda:0")
    n_src = 8192
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    centres = (torch.rand((n_src, 3), device=dev, generator=g) * 2000 - 1000).contiguous()
    rows = []
    for n in (16, 1024):
        index = torch.randint(0, n_src, (n,), device=dev, generator=g)
        out = torch.empty((n, 24), dtype=torch.float64, device=dev)

        def call(k):
            pkg.aug_xforms(centres, index=index, key=7, counter0=k * n, out=out)

        for k in range(20):
            call(k)
        torch.cuda.synchronize()
        gpu, host = [], []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            for k in range(iters):
                call(k)
            t1 = time.perf_counter()
            b.record()
            b.synchronize()
            gpu.append(1e3 * a.elapsed_time(b) / iters)
            host.append(1e6 * (t1 - t0) / iters)
        rows.append(dict(n=n, iters=iters, reps=reps, us_per_launch=round(float(np.median(gpu)), 2),
                         us_per_launch_min=round(min(gpu), 2), us_per_launch_max=round(max(gpu), 2),
                         host_us_per_call=round(float(np.median(host)), 2),
                         note="back-to-back launches between two events: the larger of GPU time and enqueue time per launch"))
        print(json.dumps(rows[-1]), file=sys.stderr)
    return rows


def voxelizer_rows(ds, iters: int, reps: int):
    dev = torch.device("cuda:0")
    rp = pkg.dataset.ResidentPacks(ds, dev)
    mid = pkg.aabb(rp.depth, rp.offsets, rp.headers, res=32).grid[:, :3].contiguous()
    n_src = rp.headers.shape[0]
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    rows = []
    for n in (16, 1024):
        index = torch.randint(0, n_src, (n,), device=dev, generator=g)
        xf = pkg.aug_xforms(mid, index=index, key=7)
        out = pkg.empty_batch(n, 32, dev)
        gn = torch.empty((n, 63), dtype=torch.float32, device=dev)
        gg = torch.empty((n, 63), dtype=torch.float32, device=dev)
        for name, maps in (("plain", None), ("augmented", xf)):
            def call():
                pkg.voxelize_indexed(rp.depth, rp.offsets, rp.headers, index, rp.gt, res=32, out=out, out_gt_nor=gn,
                                     out_gt=gg, xforms=maps)

            for _ in range(20):
                call()
            torch.cuda.synchronize()
            gpu = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters):
                    call()
                b.record()
                b.synchronize()
                gpu.append(1e3 * a.elapsed_time(b) / iters)
            rows.append(dict(entry="voxelize_indexed", maps=name, n=n, res=32, us_per_launch=round(float(np.median(gpu)), 2),
                             us_per_launch_min=round(min(gpu), 2), us_per_launch_max=round(max(gpu), 2)))
            print(json.dumps(rows[-1]), file=sys.stderr)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_aug_draw.py needs a HIP device"
    ds, frames = make_subject(a.frames)
    res = dict(device=torch.cuda.get_device_name(0), loaders=loader_rows(ds, frames, a.epochs),
               kernel=kernel_rows(a.iters, a.reps), voxelizer=voxelizer_rows(ds, a.iters, a.reps))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
