#!/usr/bin/env python3
"""What the point-wise offset fields cost (one JSON line; ``--out`` also writes it to a file, default
profiles/pointfield/bench_pointfield.json).

Legs, per batch (n frames of ``synth_frame(kind="crop")`` sampled to P = 1024 points by farthest_points; J = 21 joints near
the cloud, K = 64, radius 30 mm, M = 25, layout "cp"), in the same run:
  encode_f32 / encode_bf16   point_fields(cloud, joints, 64, radius=30) into a preallocated field
  zero_f32 / zero_bf16       ``field.zero_()`` of the same bytes: the store floor of the encoder
  torch_encode               the torch form a user writes today: ``cdist`` + ``topk(largest=False)`` + ``where`` + a division
  decode_f32 / decode_bf16   field_joints(cloud, field, radius=30, points=25) of the encoder's field
  torch_decode               ``topk`` on the heat channels + ``gather`` + a weighted mean
``encode_differs`` / ``decode_differs`` count the positions whose torch member set is not the library's / whose torch joints
are more than 1e-3 mm off the library's; then, at the same batches, R = 32, bfloat16 volumes,
  step_fps / step_fields   AugmentedStep.step() replayed from its graph with fps=(1024,), without and with fields=(64, 30).

Method (that of tools/bench_group.py): inputs resident on the device, a warm-up of every leg, then device events around
back-to-back launches — at most --iters of them, fewer where one launch is long (about --budget seconds per timed window) —;
the legs of a batch take turns for --rounds rounds and the median round is reported with min and max.  Every batch runs in a
child process of its own under its own time limit (--limit seconds), one after the other, and the first that fails ends the
run: nothing more is started on the device after it.  Without an MI355X the tool fails; it prints no times.

    python tools/bench_pointfield.py [--iters 50] [--rounds 5] [--limit 500] [--out x.json]
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
BATCHES = (16, 1024)
P, J, K, M, RADIUS = 1024, 21, 64, 25, 30.0
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
        iters[k] = int(min(a.iters, max(1 if one > 1.0 else 3, a.budget / max(one, 1e-6))))
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
        "bench_pointfield.py needs an MI355X (gfx950)"
    return pkg, torch, torch.device("cuda:0")


def _pack(pkg, torch, dev, n):
    import numpy as np
    synth = importlib.import_module(PKG + ".synth")
    depth, off, hdr = synth.synth_batch(n, "crop", seed0=0, threads=8)
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depth, off, hdr))


def one_batch(n, a):
    pkg, torch, dev = _setup()
    t = _pack(pkg, torch, dev, n)
    cap = int(pkg.farthest_points(*t, points=1).count.max())
    fps = pkg.farthest_points(*t, points=P, capacity=cap)
    assert not fps.status.any()
    cloud = fps.points
    g = torch.Generator(device="cpu").manual_seed(1)
    pick = torch.randint(0, P, (n, J), generator=g).to(dev)
    joints = (torch.gather(cloud, 1, pick[..., None].expand(-1, -1, 3)) + torch.randn((n, J, 3), generator=g).to(dev) * 6.0).contiguous()
    f32 = pkg.point_fields(cloud, joints, K, radius=RADIUS)
    bf16 = pkg.point_fields(cloud, joints, K, radius=RADIUS, dtype=torch.bfloat16)
    j32 = pkg.field_joints(cloud, f32.field, radius=RADIUS, points=M)
    j16 = pkg.field_joints(cloud, bf16.field, radius=RADIUS, points=M)

    def torch_encode():
        d = torch.cdist(joints, cloud)                                           # [n, J, P]
        kth = d.topk(K, dim=2, largest=False).values[..., -1:]
        member = (d <= kth) & (d <= RADIUS)
        heat = torch.where(member, 1 - d / RADIUS, 0.0)
        vec = torch.where(member[..., None] & (d > 0)[..., None], (joints[:, :, None] - cloud[:, None]) / d.clamp_min(1e-30)[..., None], 0.0)
        return torch.cat([heat, vec.permute(0, 1, 3, 2).reshape(n, 3 * J, P)], 1), member

    def torch_decode(field=f32.field):
        heat, idx = field[:, :J].topk(M, dim=2)                                  # [n, J, M]
        w = heat.clamp(0, 1)
        vec = torch.gather(field[:, J:].reshape(n, J, 3, P), 3, idx[:, :, None].expand(-1, -1, 3, -1))   # [n, J, 3, M]
        u = vec / vec.norm(dim=2, keepdim=True).clamp_min(1e-30)
        p = torch.gather(cloud[:, None].expand(-1, J, -1, -1), 2, idx[..., None].expand(-1, -1, -1, 3))  # [n, J, M, 3]
        e = p + (RADIUS * (1 - w))[..., None] * u.permute(0, 1, 3, 2)
        return (w[..., None] * e).sum(2) / w.sum(2, keepdim=True).clamp_min(1e-30)

    member = (f32.field[:, :J] != 0) | (f32.field[:, J:].reshape(n, J, 3, P) != 0).any(2)
    encode_differs = int((torch_encode()[1] != member).any(2).any(1).sum())
    decode_differs = int(((torch_decode() - j32.joints).abs() > 1e-3).any(2).any(1).sum())
    legs = {"encode_f32": lambda: pkg.point_fields(cloud, joints, K, radius=RADIUS, out=f32),
            "encode_bf16": lambda: pkg.point_fields(cloud, joints, K, radius=RADIUS, dtype=torch.bfloat16, out=bf16),
            "zero_f32": lambda: f32.field.zero_(), "zero_bf16": lambda: bf16.field.zero_(),
            "torch_encode": torch_encode}
    tm = _measure(legs, a)
    pkg.point_fields(cloud, joints, K, radius=RADIUS, out=f32)                   # the zero legs emptied them
    pkg.point_fields(cloud, joints, K, radius=RADIUS, dtype=torch.bfloat16, out=bf16)
    legs = {"decode_f32": lambda: pkg.field_joints(cloud, f32.field, radius=RADIUS, points=M, out=j32),
            "decode_bf16": lambda: pkg.field_joints(cloud, bf16.field, radius=RADIUS, points=M, out=j16),
            "torch_decode": torch_decode}
    tm.update(_measure(legs, a))
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), n=n, points=P, joints=J, k=K, votes=M, radius=RADIUS,
                          encode_differs=encode_differs, decode_differs=decode_differs, **tm,
                          field_gb_per_s={k: round(n * 4 * J * P * b / tm[k]["us"] / 1e3, 1) for k, b in
                                          (("encode_f32", 4), ("encode_bf16", 2), ("zero_f32", 4), ("zero_bf16", 2))},
                          encode_over_zero=round(tm["encode_f32"]["us"] / tm["zero_f32"]["us"], 2),
                          encode_bf16_over_zero=round(tm["encode_bf16"]["us"] / tm["zero_bf16"]["us"], 2),
                          torch_over_encode=round(tm["torch_encode"]["us"] / tm["encode_f32"]["us"], 2),
                          torch_over_decode=round(tm["torch_decode"]["us"] / tm["decode_f32"]["us"], 2))))


def one_step(n, a):
    import numpy as np
    pkg, torch, dev = _setup()
    R = 32
    td, to, th = _pack(pkg, torch, dev, n)
    ab = pkg.aabb(td, to, th, res=R)
    centres = ab.grid[:, :3].contiguous()
    noise = torch.from_numpy(np.random.default_rng(1).normal(0, 40, (n, J, 3)).astype(np.float32)).to(dev)
    gt = (centres[:, None, :] + noise).reshape(n, 3 * J).contiguous()
    index = torch.arange(n, dtype=torch.int64, device=dev)
    kw = dict(gt=gt, centres=centres, res=R, dtype=torch.bfloat16, fps=(P,))
    steps = {"step_fps": pkg.AugmentedStep(td, to, th, n, **kw),
             "step_fields": pkg.AugmentedStep(td, to, th, n, fields=(K, RADIUS), **kw)}
    counter = [0]

    def leg(s):
        def fn():
            counter[0] += n
            s.step(index, KEY, counter[0])
        return fn
    t = _measure({k: leg(s) for k, s in steps.items()}, a)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), n=n, res=R, fps_points=P, fields=(K, RADIUS), **t,
                          fields_add_us=round(t["step_fields"]["us"] - t["step_fps"]["us"], 2),
                          with_over_without=round(t["step_fields"]["us"] / t["step_fps"]["us"], 3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--limit", type=int, default=500, help="seconds per child process")
    ap.add_argument("--one", type=int, metavar="N")
    ap.add_argument("--step", type=int, metavar="N")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointfield", "bench_pointfield.json"))
    a = ap.parse_args()
    if a.one:
        return one_batch(a.one, a)
    if a.step:
        return one_step(a.step, a)
    common = ["--iters", str(a.iters), "--rounds", str(a.rounds), "--budget", str(a.budget)]
    todo = [["--one", str(n)] for n in BATCHES] + [["--step", str(n)] for n in BATCHES]
    got = {"--one": [], "--step": []}
    for step in todo:                                        # one child per step, each under its own limit; stop at the first failure
        r = subprocess.run([sys.executable, os.path.abspath(__file__), *step, *common], capture_output=True, text=True,
                           timeout=a.limit)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            raise SystemExit(f"bench_pointfield.py {' '.join(step)} ended with status {r.returncode}")
        row = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(row), file=sys.stderr)
        got[step[0]].append(row)
    device = [row.pop("device") for rows in got.values() for row in rows][0]
    line = json.dumps(dict(device=device, iters_max=a.iters, rounds=a.rounds, rows=got["--one"], steps=got["--step"]))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
