#!/usr/bin/env python3
"""What the depth-image patches cost (one JSON line; ``--out`` also writes it to a file, default
profiles/patch/bench_patch.json).

Shapes: 16 and 1024 frames of 320 x 240 to 128^2, 256 frames of 640 x 480 to 176^2 (frame_patches on the seeded blob scenes
of tests/locate_ref.py, centred by locate_hands), and 1024 MSRA-like crops to 96^2 (crop_patches on synth_batch's pack,
centred by aabb()).  Legs, per shape and element type (float32, bfloat16), in the same run:
  nearest / bilinear            the patch under the identity (affine=None)
  nearest_map / bilinear_map    the same under patch_affines maps (rotation +-pi, scale 0.8..1.2, shift +-0.1)
  fill              out.zero_() of the patch's bytes: the store floor
  aabb              aabb() over the pack, or over the frames as one pack: ONE read of the source
  torch             (frames only) the torch form a user writes today: affine_grid + grid_sample (bilinear,
                    align_corners=False) on [n, 1, H, W] with the cube rectangles handed over for free, then the
                    normalisation and torch.where for the cube's depth test; ``torch_differs`` counts the pixels in which it
                    is not the library's bilinear patch by more than 1e-3 (it blends hand and background at the silhouette)
and once per frame shape
  locate / patch_frames         locate_hands(grid=False) alone, and patch_frames (locate + patch)
  uvd                           joints_to_uvd at J = 21

Method: inputs resident on the device, a warm-up of every leg, then device events around back-to-back launches — at most
--iters of them, fewer where one launch is long (about --budget seconds per timed window, at least 5) —; the legs of a shape
take turns for --rounds rounds and the median round is reported with min and max.  Every shape runs in a child process of
its own under its own time limit (--limit seconds), one after the other, and the first that fails ends the run: nothing
more is started on the device after it.  Without an MI355X the tool fails; it prints no times.

    python tools/bench_patch.py [--iters 100] [--rounds 5] [--limit 300] [--out x.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "handposeestimation-with-3d-cnns_amd"
SHAPES = (("frames", 16, 240, 320, 128), ("frames", 1024, 240, 320, 128), ("frames", 256, 480, 640, 176), ("crops", 1024, 0, 0, 96))
CUBE = 250.0


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
        "bench_patch.py needs an MI355X (gfx950)"
    return pkg, torch, torch.device("cuda:0")


def _maps(pkg, torch, dev, n):
    g = torch.Generator(device="cpu").manual_seed(7)
    angle = (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1) * math.pi
    scale = 0.8 + 0.4 * torch.rand(n, generator=g, dtype=torch.float64)
    shift = (torch.rand((n, 2), generator=g, dtype=torch.float64) * 2 - 1) * 0.1
    return pkg.patch_affines(angle.to(dev), scale.to(dev), shift.to(dev))


def one_shape(kind, n, H, W, S, a):
    import numpy as np
    pkg, torch, dev = _setup()
    row = dict(device=torch.cuda.get_device_name(0), kind=kind, n=n, H=H, W=W, size=S)
    if kind == "frames":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import locate_ref as lr
        cam_t = lr.DEFAULT_CAM if H == 240 else lr.CAM_VGA
        cam = pkg.TsdfCam(*cam_t)
        k = min(n, 16)
        base = np.stack([lr.scene(H, W, cam_t, 9000 + s, corner=(s % 4 == 3))["frame"] for s in range(k)])
        frames = torch.from_numpy(base[np.arange(n) % k].astype(np.float32)).to(dev)
        crops = pkg.locate_hands(frames, cube=CUBE, cam=cam, grid=False)
        com, status = crops.com, crops.status
        fo = torch.arange(n + 1, dtype=torch.int64, device=dev) * (H * W)
        fh = torch.tensor([[W, H, 0, 0, W, H]] * n, dtype=torch.int32, device=dev)
        flat = frames.reshape(-1)
        read = lambda: pkg.aabb(flat, fo, fh, cam=cam)                                           # noqa: E731
        call = lambda **kw: pkg.frame_patches(frames, com, size=S, cube=CUBE, cam=cam, status=status, **kw)   # noqa: E731
        row["source_bytes"] = int(frames.numel() * 4)
    else:
        synth = importlib.import_module(PKG + ".synth")
        cam = None
        pack = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in synth.synth_batch(n, "crop", seed0=0, threads=8))
        ab = pkg.aabb(*pack)
        com, status = ab.grid[:, :3].contiguous().double(), None                                  # the cloud's middle, widened
        read = lambda: pkg.aabb(*pack)                                                            # noqa: E731
        call = lambda **kw: pkg.crop_patches(*pack, com, size=S, cube=CUBE, **kw)                 # noqa: E731
        row["source_bytes"] = int(pack[0].numel() * 4)
    aff = _maps(pkg, torch, dev, n)
    for name, dt in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
        out = pkg.PatchBatch(torch.empty((n, 1, S, S), dtype=dt, device=dev), torch.empty((n,), dtype=torch.int32, device=dev))
        nbytes = out.patch.numel() * out.patch.element_size()
        legs = {"nearest": lambda: call(dtype=dt, out=out), "bilinear": lambda: call(dtype=dt, interp="bilinear", out=out),
                "nearest_map": lambda: call(dtype=dt, affine=aff, out=out),
                "bilinear_map": lambda: call(dtype=dt, interp="bilinear", affine=aff, out=out),
                "fill": lambda: out.patch.zero_(), "aabb": read}
        extra = {}
        if kind == "frames":
            # the torch form's inputs, for free: the cube rectangles as affine_grid's theta (align_corners=False: a pixel's
            # centre at column x is (2x + 1) / W - 1), the centre's depth and the half cube
            c = com.cpu().numpy()
            F, cx, cy = cam.focal, cam.cx, cam.cy
            cd = -c[:, 2]
            h = CUBE / 2
            u0, u1 = (c[:, 0] - h) * F / cd + cx, (c[:, 0] + h) * F / cd + cx
            v0, v1 = -(c[:, 1] + h) * F / cd + cy, -(c[:, 1] - h) * F / cd + cy
            theta = np.zeros((n, 2, 3), np.float32)
            theta[:, 0, 0], theta[:, 0, 2] = (u1 - u0) / W, (u0 + u1 + 1) / W - 1
            theta[:, 1, 1], theta[:, 1, 2] = (v1 - v0) / H, (v0 + v1 + 1) / H - 1
            theta, cd_t = torch.from_numpy(theta).to(dev), torch.from_numpy(cd.astype(np.float32)).to(dev)[:, None, None, None]
            src = frames[:, None]

            def torch_form():
                grid = torch.nn.functional.affine_grid(theta, (n, 1, S, S), align_corners=False)
                d = torch.nn.functional.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
                z = (d - cd_t) / h
                return torch.where((d >= 1.0) & (z.abs() <= 1.0), z, 1.0).to(dt)
            ours = call(dtype=dt, interp="bilinear").patch
            ok = (status == 0)
            differs = int((((torch_form().float() - ours.float()).abs() > 1e-3).flatten(1).sum(dim=1) * ok).sum())
            legs["torch"] = torch_form
            extra = dict(torch_differs=differs, hand_pixels=int(((ours.float() != 1.0).flatten(1).sum(dim=1) * ok).sum()))
        tm = _measure(legs, a)
        floor = tm["fill"]["us"] + tm["aabb"]["us"]
        row[name] = dict(bytes=nbytes, **extra, **tm,
                         tb_per_s={k: round(nbytes / (tm[k]["us"] * 1e-6) / 1e12, 3) for k in ("nearest", "bilinear", "fill")},
                         over_fill_plus_aabb={k: round(tm[k]["us"] / floor, 3) for k in ("nearest", "bilinear", "nearest_map", "bilinear_map")},
                         **({"torch_over_bilinear": round(tm["torch"]["us"] / tm["bilinear"]["us"], 2)} if "torch" in tm else {}))
        del out
    if kind == "frames":
        gt = (com.float()[:, None, :] + 40 * torch.randn((n, 21, 3), device=dev)).contiguous()
        tm = _measure({"locate": lambda: pkg.locate_hands(frames, cube=CUBE, cam=cam, grid=False),
                       "patch_frames": lambda: pkg.patch_frames(frames, S, cube=CUBE, cam=cam),
                       "uvd": lambda: pkg.joints_to_uvd(gt, com, cube=CUBE, cam=cam, status=status)}, a)
        row["chain"] = dict(**tm, patch_frames_over_locate=round(tm["patch_frames"]["us"] / tm["locate"]["us"], 3))
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--limit", type=int, default=300, help="seconds per child process")
    ap.add_argument("--one", nargs=5, metavar=("KIND", "N", "H", "W", "S"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch", "bench_patch.json"))
    a = ap.parse_args()
    if a.one:
        return one_shape(a.one[0], *[int(v) for v in a.one[1:]], a)
    common = ["--iters", str(a.iters), "--rounds", str(a.rounds), "--budget", str(a.budget)]
    rows = []
    for shape in SHAPES:                                     # one child per shape, each under its own limit; stop at the first failure
        step = ["--one", *[str(v) for v in shape]]
        r = subprocess.run([sys.executable, os.path.abspath(__file__), *step, *common], capture_output=True, text=True,
                           timeout=a.limit)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            raise SystemExit(f"bench_patch.py {' '.join(step)} ended with status {r.returncode}")
        row = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(row), file=sys.stderr)
        rows.append(row)
    device = [row.pop("device") for row in rows][0]
    line = json.dumps(dict(device=device, iters_max=a.iters, rounds=a.rounds, rows=rows))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
