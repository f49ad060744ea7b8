#!/usr/bin/env python3
"""Cost of the grid placement from a cloud (one JSON line; ``--out`` also writes it to a file).

  kernel   tsdf_cloud_grid_hip at n = 16, 500, 1024, P = 6000 (the C entry with preallocated outputs): GPU time per
           launch (events around a run of launches, median of --reps runs after a warm-up, with min and max), the
           n*P*24 bytes it reads as GB/s and as a share of the 8 TB/s HBM peak — "resident": one cloud set re-read by
           every launch; "rotating": launches walk over enough cloud sets (>= 512 MB in all, twice the Infinity Cache)
           that none finds its input in a cache.  Beside it, on the same tensors, what a caller has without the kernel:
           the torch composite (amax / amin over x and y, z through torch.where(z != 0, z, -+inf), float32 glue)
  process  process_batch at n = 500 and its three stages on their own
  export   preprocess_tree wall time on one synthetic subject (host clock, after one untimed warm-up run) with
           placement="pixels" against "cloud", point_clouds="device"

    python tools/bench_cloud_grid.py [--iters 50] [--reps 5] [--out bench_cloud_grid.json]
"""
from __future__ import annotations

import argparse
import importlib
import itertools
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
export = importlib.import_module("handposeestimation-with-3d-cnns_amd.export")

HBM_PEAK = 8.0e12        # bytes/s (MI355X)
ROTATE_BYTES = 512 << 20  # cloud sets of the rotating measurement hold at least this much


def gpu_time(fn, iters, reps, warm=10):
    """(median, min, max) GPU time per call in us over ``reps`` runs of ``iters`` calls, each between two events."""
    count = itertools.count()     # runs on across the repetitions: a rotating input never restarts at its first set
    for _ in range(warm):
        fn(next(count))
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn(next(count))
        b.record()
        b.synchronize()
        ts.append(1e3 * a.elapsed_time(b) / iters)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def make_clouds(n, P, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    pts = torch.randn((n, P, 3), dtype=torch.float64, device=dev, generator=g) * 90
    pts[:, :, 2] -= 420
    pts[:, :, 2] *= (torch.rand((n, P), device=dev, generator=g) >= 0.05)    # zeros in z, as a sparse crop leaves them
    return pts


def composite(pts, R=32):
    """The same placement from torch operators (no kernel of this library): the baseline."""
    inf = float("inf")
    x, y, z = pts[:, :, 0], pts[:, :, 1], pts[:, :, 2]
    nz = z != 0
    mx = torch.stack([x.amax(1), y.amax(1), torch.where(nz, z, -inf).amax(1)], 1).to(torch.float32)
    mn = torch.stack([x.amin(1), y.amin(1), torch.where(nz, z, inf).amin(1)], 1).to(torch.float32)
    mid = (mx + mn) / 2
    max_l = (mx - mn).amax(1)
    vl = max_l / R
    grid = torch.zeros((pts.shape[0], 8), dtype=torch.float32, device=pts.device)
    grid[:, :3] = mid - (max_l / 2)[:, None] + (vl / 2)[:, None]
    grid[:, 3] = vl
    grid[:, 4] = vl * 3
    return grid, max_l, mid


def kernel_rows(iters, reps, P=6000):
    dev = torch.device("cuda:0")
    L = pkg._lib.load()
    rows = []
    for n in (16, 500, 1024):
        nbytes = n * P * 24
        sets = max(2, -(-ROTATE_BYTES // nbytes))
        clouds = [make_clouds(n, P, dev, s) for s in range(sets)]
        grid = torch.empty((n, 8), dtype=torch.float32, device=dev)
        ml = torch.empty(n, dtype=torch.float32, device=dev)
        mp = torch.empty((n, 3), dtype=torch.float32, device=dev)
        ab = torch.empty((n, 6), dtype=torch.float32, device=dev)
        st = torch.empty(n, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        ptrs = [c.data_ptr() for c in clouds]
        tail = (None, stream, grid.data_ptr(), ml.data_ptr(), mp.data_ptr(), ab.data_ptr(), st.data_ptr())

        def kernel(k, rot):
            rc = L.tsdf_cloud_grid_hip(ptrs[k % sets if rot else 0], n, P, 32, *tail)
            assert rc == 0

        ref = composite(clouds[0])
        kernel(0, False)
        torch.cuda.synchronize()
        assert torch.equal(grid[:, :5], ref[0][:, :5]) and torch.equal(ml, ref[1]), "kernel and composite disagree"
        for rot in (False, True):
            k_med, k_lo, k_hi = gpu_time(lambda k: kernel(k, rot), iters, reps)
            c_med, c_lo, c_hi = gpu_time(lambda k: composite(clouds[k % sets if rot else 0]), iters, reps)
            rows.append(dict(n=n, P=P, input="rotating" if rot else "resident", sets=sets if rot else 1,
                             bytes=nbytes, us=round(k_med, 2), us_min=round(k_lo, 2), us_max=round(k_hi, 2),
                             GBps=round(nbytes / k_med / 1e3, 1), share_of_peak=round(nbytes / (k_med * 1e-6) / HBM_PEAK, 3),
                             torch_us=round(c_med, 2), torch_us_min=round(c_lo, 2), torch_us_max=round(c_hi, 2),
                             speedup=round(c_med / k_med, 2),
                             beats_by_more_than_spreads=bool(c_med - k_med > (k_hi - k_lo) + (c_hi - c_lo))))
            print(json.dumps(rows[-1]), file=sys.stderr)
        del clouds
        torch.cuda.empty_cache()
    return rows


def process_rows(iters, reps, n=500, P=6000):
    dev = torch.device("cuda:0")
    depth, off, hdr = synth.synth_batch(n, "crop", seed0=1, threads=8)
    d, o, h = (torch.from_numpy(x).to(dev) for x in (depth, off, hdr))
    pc = pkg.point_clouds(d, o, h, points=P, seed=1)
    cgr = pkg.cloud_grids(pc.points)
    stages = {
        "point_clouds": lambda k: pkg.point_clouds(d, o, h, points=P, seed=1, out=pc),
        "cloud_grids": lambda k: pkg.cloud_grids(pc.points),
        "voxelize_grid": lambda k: pkg.voxelize_grid(d, o, h, cgr.grid),
        "process_batch": lambda k: pkg.process_batch(d, o, h, points=P, seed=1),
        "voxelize (pixel placement, one launch)": lambda k: pkg.voxelize(d, o, h),
    }
    rows = []
    for name, fn in stages.items():
        med, lo, hi = gpu_time(fn, iters, reps)
        rows.append(dict(stage=name, n=n, P=P, us=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2)))
        print(json.dumps(rows[-1]), file=sys.stderr)
    return rows


def export_rows(frames_per_gesture=500, gestures=1, reps=2):
    tmp = tempfile.mkdtemp(prefix="bench_cg_")
    try:
        db = os.path.join(tmp, "db")
        synth.synth_msra_tree(db, n_sub=1, n_ges=gestures, n_frames=frames_per_gesture, seed=3)
        rows = []
        for placement in ("pixels", "cloud"):
            ts = []
            for r in range(reps + 1):
                out = os.path.join(tmp, "out_%s_%d" % (placement, r))
                t0 = time.perf_counter()
                export.preprocess_tree(db, out, point_clouds="device", placement=placement, rng=np.random.default_rng(0))
                ts.append(time.perf_counter() - t0)
                shutil.rmtree(out)
            ts = ts[1:]   # the first run warms caches and code objects
            frames = frames_per_gesture * gestures
            rows.append(dict(placement=placement, point_clouds="device", frames=frames, s=round(float(np.median(ts)), 3),
                             s_min=round(min(ts), 3), s_max=round(max(ts), 3),
                             ms_per_frame=round(1e3 * float(np.median(ts)) / frames, 3)))
            print(json.dumps(rows[-1]), file=sys.stderr)
        return rows
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=500, help="frames of the export subject's gesture")
    ap.add_argument("--skip-export", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cloud_grid.py needs a HIP device"
    res = dict(device=torch.cuda.get_device_name(0), iters=a.iters, reps=a.reps, kernel=kernel_rows(a.iters, a.reps),
               process=process_rows(a.iters, a.reps))
    if not a.skip_export:
        res["export"] = export_rows(a.frames)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
