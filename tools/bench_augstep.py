#!/usr/bin/env python3
"""What the draws from device-resident counters are worth at the reference's batch size (one JSON line; ``--out`` also
writes it to a file).  Batch 16, R = 32, shuffled, one synthetic pack-backed subject.

  loader-eager   ResidentLoader(augment="device", prefetch=1): two C calls per batch (the baseline; this leg uses nothing
                 newer than augment="device", so the same file measures a checkout without graph=)
  loader-graph   ResidentLoader(augment="device", prefetch=1, graph=True): one small copy and one graph replay per batch
  dataset-host   DataLoader(MSRA_Dataset(aug=True), batch_size=16, shuffle=True): maps gathered from a page-locked table
  dataset-device DataLoader(MSRA_Dataset(aug="device"), ...): maps drawn per batch by tsdf_aug_draw_at_hip

Method (that of tools/bench_aug_draw.py): crops/s over a whole epoch — host clock around the epoch, ended by a device
synchronise —, median of --epochs epochs after one warm-up epoch, with min and max; the legs take turns epoch by epoch, so
a drift of the machine meets all of them alike.

    python tools/bench_augstep.py [--frames 8192] [--epochs 5] [--legs loader-eager,loader-graph,...] [--out x.json]
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

LEGS = ("loader-eager", "loader-graph", "dataset-host", "dataset-device")
BS = 16


def make_subject(frames: int):
    """One synthetic MSRA subject (8 gestures), packed."""
    tmp = tempfile.mkdtemp(prefix="bench_augstep_")
    try:
        db = os.path.join(tmp, "db")
        total = synth.synth_msra_tree(db, n_sub=1, n_ges=8, n_frames=max(1, frames // 8), seed=3)
        pk = pkg.packing.pack_subject(os.path.join(db, "P0"))
        assert len(pk) == total      # (held in memory: the tree can go)
        return pkg.MSRADepthDataset.from_packs([pk]), total
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def make_leg(name: str, raw, dev):
    """(iterable over one epoch, crops per epoch)."""
    if name.startswith("loader"):
        kw = dict(graph=True) if name == "loader-graph" else {}
        return pkg.ResidentLoader(raw, batch_size=BS, device=dev, res=32, shuffle=True, augment="device", prefetch=1,
                                  **kw), len(raw)
    ds = pkg.MSRA_Dataset.from_raw(raw, device=dev, aug=True if name == "dataset-host" else "device")
    return torch.utils.data.DataLoader(ds, batch_size=BS, shuffle=True), len(ds)


def epoch_seconds(it) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in it:
        pass
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--out")
    a = ap.parse_args()
    names = [s for s in a.legs.split(",") if s]
    assert names and all(s in LEGS for s in names), f"--legs takes a comma-separated subset of {LEGS}"
    assert torch.cuda.is_available(), "bench_augstep.py needs a HIP device"
    dev = torch.device("cuda:0")
    raw, _ = make_subject(a.frames)
    legs = {s: make_leg(s, raw, dev) for s in names}
    times = {s: [] for s in names}
    for e in range(a.epochs + 1):            # epoch 0 warms up: upload, code objects, rings, the graph's capture
        for s, (it, _) in legs.items():
            t = epoch_seconds(it)
            if e:
                times[s].append(t)
    rows = []
    for s, ts in times.items():
        crops = legs[s][1]
        rate = sorted(crops / t for t in ts)
        rows.append(dict(leg=s, batch_size=BS, res=32, crops_per_epoch=crops, epochs=len(ts),
                         crops_per_s=round(float(np.median(rate))), crops_per_s_min=round(rate[0]),
                         crops_per_s_max=round(rate[-1]),
                         us_per_batch=round(1e6 * float(np.median(ts)) / (-(-crops // BS)), 1)))
        print(json.dumps(rows[-1]), file=sys.stderr)
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), legs=rows))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
