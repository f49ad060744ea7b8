#!/usr/bin/env python3
"""What locating the hand in raw frames costs (one JSON line; ``--out`` also writes it to a file).

Legs, per shape, on the same frames in the same run (seeded blob scenes of tests/locate_ref.py: a hand in front of a body
plane, a fifth of the frame empty; 64 distinct scenes tiled to n):
  aabb            aabb() over the whole frames as one pack: ONE read of every frame — the floor a scan can reach
  locate          locate_hands(), float32 frames, refine = 2 (tsdf_locate_hip: three launches)
  locate_r0       the same with refine = 0
  locate_u16      the same frames as uint16 eighths of a millimetre (shift = 3), refine = 2
  torch           the same contract in torch ops, as a user writes it today: validity, nearest depth, seed sums, rectangle,
                  two refinements, and the masked FULL frame — WITHOUT the repack into crops (variable sizes: that needs
                  the host), so it does less than locate_hands
and for the 320x240 shapes with n >= 16:
  voxelize        voxelize() of the READY located pack, R = 32
  frames_aabb     voxelize_frames(placement="aabb"): locate_hands + voxelize
  frames_cube     voxelize_frames(placement="cube"): locate_hands + voxelize_grid
Shapes: 1, 16 and 1024 frames of 320x240 (the MSRA camera) and 1 and 256 frames of 640x480 (focal 588.04).

Method: inputs resident on the device, --warmup calls, then device events around --iters back-to-back calls (the torch leg:
a tenth of that); the legs of a shape take turns for --rounds rounds and the median round is reported with min and max.  The
wrappers allocate their outputs (torch's caching allocator: no device allocation in the steady state).

``need_bytes``: what the algorithm has to move, computed from the shapes — every frame read once (elements x 4 or 2) plus
the crops written (4 x offsets[n]); ``hbm_share`` is need_bytes over the kernel time as a share of PEAK (8 TB/s).  A leg at
n = 1 or 16 is launch latency (three dependent launches), not bandwidth: its share says nothing.

    python tools/bench_locate.py [--iters 100] [--warmup 10] [--rounds 5] [--out profiles/locate/bench_locate.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("handposeestimation-with-3d-cnns_amd")
import locate_ref as lr  # noqa: E402  (tests/locate_ref.py: the scenes)
from _timing import timed_us  # noqa: E402  (tools/_timing.py, beside this file)

PEAK = 8.0e12   # bytes/s, the HBM peak the share is taken of
P = lr.PARAMS


def torch_locate(frames, cam, cube=250.0, near=100.0, far=1500.0, band=150.0, refine=2):
    """The contract in torch ops, batched, float64 sums; returns (com, rectangles, the masked full frames)."""
    F, cx, cy, eps = cam[:4]
    n, H, W = frames.shape
    d = frames
    valid = torch.isfinite(d) & (d.abs() >= eps) & (d >= near) & (d <= far)
    dmin = torch.where(valid, d, torch.full_like(d, float("inf"))).amin(dim=(1, 2), keepdim=True)
    d64 = d.double()
    xs = (torch.arange(W, device=d.device, dtype=torch.float64) - cx)[None, None, :]
    ys = (torch.arange(H, device=d.device, dtype=torch.float64) - cy)[None, :, None]
    col = torch.arange(W, device=d.device)[None, None, :]
    row = torch.arange(H, device=d.device)[None, :, None]
    h = cube / 2.0

    def centre(S):
        w = torch.where(S, d64, torch.zeros_like(d64))
        N = S.sum(dim=(1, 2)).double().clamp(min=1.0)
        return (w * xs).sum(dim=(1, 2)) / F / N, -((w * ys).sum(dim=(1, 2)) / F / N), w.sum(dim=(1, 2)) / N

    def rect(c_x, c_y, cd):
        left = (((c_x - h) * F) / cd + cx).floor().clamp(0, W - 1)
        right = ((((c_x + h) * F) / cd + cx).floor() + 1).clamp(max=W).maximum(left + 1)
        top = (((-(c_y + h)) * F) / cd + cy).floor().clamp(0, H - 1)
        bottom = ((((-(c_y - h)) * F) / cd + cy).floor() + 1).clamp(max=H).maximum(top + 1)
        return left, top, right, bottom

    def inside(r, cd):
        left, top, right, bottom = (v[:, None, None] for v in r)
        return valid & (col >= left) & (col < right) & (row >= top) & (row < bottom) & ((d64 - cd[:, None, None]).abs() <= h)

    c_x, c_y, cd = centre(valid & (d64 <= dmin.double() + band))
    r = rect(c_x, c_y, cd)
    for _ in range(refine):
        c_x, c_y, cd = centre(inside(r, cd))
        r = rect(c_x, c_y, cd)
    return torch.stack([c_x, c_y, -cd], 1), torch.stack(r, 1), torch.where(inside(r, cd), d, torch.zeros_like(d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.iters >= 50, "time at least 50 launches"
    assert torch.cuda.is_available(), "bench_locate.py needs a HIP device"
    dev = torch.device("cuda:0")
    R = 32
    rows = []
    base = {}
    for H, W, cam in ((240, 320, lr.DEFAULT_CAM), (480, 640, lr.CAM_VGA)):
        k = 64 if H == 240 else 16
        base[(H, W)] = np.stack([lr.scene(H, W, cam, 9000 + s, corner=(s % 4 == 3))["frame"] for s in range(k)])
    for n, H, W, cam in ((1, 240, 320, lr.DEFAULT_CAM), (16, 240, 320, lr.DEFAULT_CAM), (1024, 240, 320, lr.DEFAULT_CAM),
                         (1, 480, 640, lr.CAM_VGA), (256, 480, 640, lr.CAM_VGA)):
        b = base[(H, W)]
        f32 = np.concatenate([b] * (n // len(b) + 1))[:n]
        hc = pkg.TsdfCam(*cam)
        tf = torch.from_numpy(f32).to(dev)
        tu = torch.from_numpy((f32.astype(np.float64) * 8).astype(np.uint16)).to(dev)
        # the whole frames as one pack, for aabb()
        fo = (torch.arange(n + 1, dtype=torch.int64, device=dev) * (H * W))
        fh = torch.tensor([[W, H, 0, 0, W, H]] * n, dtype=torch.int32, device=dev)
        flat = tf.reshape(-1)
        crops = pkg.locate_hands(tf, cam=hc, **P)
        torch.cuda.synchronize()
        assert not bool(crops.status.any())
        com_t, rect_t, _ = torch_locate(tf, cam)
        torch.cuda.synchronize()
        assert torch.equal(rect_t.int(), crops.headers[:, 2:6]), "the torch leg does not compute the same rectangles"
        assert float((com_t - crops.com).abs().max()) < 1e-6
        crop_px = int(crops.offsets[-1].item())
        legs = {"aabb": (lambda: pkg.aabb(flat, fo, fh, res=R, cam=hc), a.iters),
                "locate": (lambda: pkg.locate_hands(tf, cam=hc, **P), a.iters),
                "locate_r0": (lambda: pkg.locate_hands(tf, cam=hc, **dict(P, refine=0)), a.iters),
                "locate_u16": (lambda: pkg.locate_hands(tu, cam=hc, shift=3, **P), a.iters),
                "torch": (lambda: torch_locate(tf, cam), max(5, a.iters // 10))}
        if H == 240 and n >= 16:
            d, o, h = crops.depth, crops.offsets, crops.headers
            legs["voxelize"] = (lambda: pkg.voxelize(d, o, h, res=R, cam=hc), a.iters)
            legs["frames_aabb"] = (lambda: pkg.voxelize_frames(tf, R, placement="aabb", cam=hc, **P), a.iters)
            legs["frames_cube"] = (lambda: pkg.voxelize_frames(tf, R, placement="cube", cam=hc, **P), a.iters)
        for fn, _ in legs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, (fn, iters) in legs.items():
                times[k].append(timed_us(fn, iters))
        t = {k: dict(us=round(float(np.median(v)), 2), us_min=round(min(v), 2), us_max=round(max(v), 2))
             for k, v in times.items()}
        need = {"locate": 4 * n * H * W + 4 * crop_px, "locate_r0": 4 * n * H * W + 4 * crop_px,
                "locate_u16": 2 * n * H * W + 4 * crop_px, "aabb": 4 * n * H * W}
        row = dict(n=n, H=H, W=W, res=R, crop_pixels=crop_px, **t,
                   need_bytes=need,
                   hbm_share={k: round(v / (t[k]["us"] * 1e-6) / PEAK, 4) for k, v in need.items()},
                   locate_over_aabb=round(t["locate"]["us"] / t["aabb"]["us"], 3),
                   torch_over_locate=round(t["torch"]["us"] / t["locate"]["us"], 2))
        if "voxelize" in t:
            row["frames_aabb_over_voxelize"] = round(t["frames_aabb"]["us"] / t["voxelize"]["us"], 3)
            row["frames_cube_over_voxelize"] = round(t["frames_cube"]["us"] / t["voxelize"]["us"], 3)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del tf, tu, flat, fo, fh, crops, com_t, rect_t, legs
        torch.cuda.empty_cache()
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=a.rounds, peak_bytes_per_s=PEAK,
                           rows=rows))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
