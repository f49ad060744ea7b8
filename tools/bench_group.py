#!/usr/bin/env python3
"""What the kNN grouping and the surface normals cost (one JSON line; ``--out`` also writes it to a file, default
profiles/group/bench_group.json).

Legs, per batch (n frames of ``synth_frame(kind="crop")`` sampled to 1024 points by farthest_points), in the same run:
  knn_1024_512x64   knn_groups(cloud, 64, queries=512): HandPointNet's first set-abstraction level
  knn_512_128x64    knn_groups(cloud[:, :512], 64, queries=128): its second, the cloud a prefix read in place
  knn_offsets       the first level with ``offsets=True``
  normals_30        point_normals(cloud, 30): a normal and a curvature per point
  torch_knn         the torch form a user writes today for the first level with offsets: ``cdist`` + ``topk(largest=False)``
                    + ``gather`` and a subtraction
  torch_normals     ``cdist`` + ``topk`` + ``gather``, the covariance by ``einsum`` and ``torch.linalg.eigh``
``knn_differs`` / ``normals_differ`` count the positions whose torch neighbours are not the library's / whose torch normal is
more than 1e-3 off the library's (up to sign); then, at the same batches, R = 32, bfloat16,
  step_fps / step_groups   AugmentedStep.step() replayed from its graph with fps=(1024,), without and with
                    groups=((512, 64), (128, 64)), normals=30.

Method (that of tools/bench_fps.py): inputs resident on the device, a warm-up of every leg, then device events around
back-to-back launches — at most --iters of them, fewer where one launch is long (about --budget seconds per timed window) —;
the legs of a batch take turns for --rounds rounds (a leg of more than ten seconds a call: one) and the median round is reported with min
and max.  Every batch runs in
a child process of its own under its own time limit (--limit seconds), one after the other, and the first that fails ends
the run: nothing more is started on the device after it.  Without an MI355X the tool fails; it prints no times.

    python tools/bench_group.py [--iters 50] [--rounds 5] [--limit 500] [--out x.json]
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
M, LEVELS, NORMALS_K = 1024, ((512, 64), (128, 64)), 30
KEY = 0xABCDEF


def _measure(legs, a):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from _timing import timed_us
    iters, rounds = {}, {}
    for k, fn in legs.items():                               # warm-up, and how long one launch is
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        one = time.perf_counter() - t0
        iters[k] = int(min(a.iters, max(1 if one > 1.0 else 3, a.budget / max(one, 1e-6))))
        rounds[k] = 1 if one > 10.0 else a.rounds           # a leg of more than ten seconds a call is timed once
    times = {k: [] for k in legs}
    for r in range(a.rounds):
        for k, fn in legs.items():
            if r < rounds[k]:
                times[k].append(timed_us(fn, iters[k]))
    return {k: dict(us=round(float(np.median(v)), 2), us_min=round(min(v), 2), us_max=round(max(v), 2), iters=iters[k], rounds=rounds[k])
            for k, v in times.items()}


def _setup():
    import torch
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    assert torch.cuda.is_available() and torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950"), \
        "bench_group.py needs an MI355X (gfx950)"
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
    fps = pkg.farthest_points(*t, points=M, capacity=cap)
    assert not fps.status.any()
    cloud = fps.points
    (C1, K1), (C2, K2) = LEVELS
    g1 = pkg.knn_groups(cloud, K1, queries=C1)
    g1o = pkg.knn_groups(cloud, K1, queries=C1, offsets=True)
    g2 = pkg.knn_groups(cloud[:, :C1], K2, queries=C2)
    nrm = pkg.point_normals(cloud, NORMALS_K)

    def torch_knn():
        q = cloud[:, :C1]
        idx = torch.cdist(q, cloud).topk(K1, dim=2, largest=False).indices
        nb = torch.gather(cloud[:, None].expand(-1, C1, -1, -1), 2, idx[..., None].expand(-1, -1, -1, 3))
        return idx, nb - q[:, :, None]

    def torch_normals():
        idx = torch.cdist(cloud, cloud).topk(NORMALS_K, dim=2, largest=False).indices
        nb = torch.gather(cloud[:, None].expand(-1, M, -1, -1), 2, idx[..., None].expand(-1, -1, -1, 3)).double()
        e = nb - nb.mean(2, keepdim=True)
        cov = torch.einsum("nqka,nqkb->nqab", e, e) / NORMALS_K
        w, v = torch.linalg.eigh(cov)
        normal = v[..., 0]
        flip = (normal * -cloud.double()).sum(-1) < 0
        return torch.where(flip[..., None], -normal, normal), w[..., 0] / w.sum(-1)

    tidx = torch_knn()[0]
    knn_differs = int((tidx.sort(2).values != g1.index.long().sort(2).values).any(2).any(1).sum())
    tn = torch_normals()[0]
    off = 1 - (tn * nrm.normals.double()).sum(-1).abs()
    normals_differ = int((off > 1e-3).any(1).sum())
    legs = {"knn_1024_512x64": lambda: pkg.knn_groups(cloud, K1, queries=C1, out=g1),
            "knn_512_128x64": lambda: pkg.knn_groups(cloud[:, :C1], K2, queries=C2, out=g2),
            "knn_offsets": lambda: pkg.knn_groups(cloud, K1, queries=C1, out=g1o),
            "normals_30": lambda: pkg.point_normals(cloud, NORMALS_K, out=nrm),
            "torch_knn": torch_knn, "torch_normals": torch_normals}
    tm = _measure(legs, a)
    # the distance arithmetic alone: 8 float32 operations a pair
    pairs = n * C1 * M
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), n=n, points=M, levels=LEVELS, normals_k=NORMALS_K,
                          knn_differs=knn_differs, normals_differ=normals_differ, worst_normal_off=float(off.max()), **tm,
                          ns_per_query={k: round(1e3 * tm[k]["us"] / (n * c), 3) for k, c in
                                        (("knn_1024_512x64", C1), ("knn_512_128x64", C2), ("knn_offsets", C1), ("normals_30", M))},
                          gpairs_per_s=round(pairs / tm["knn_1024_512x64"]["us"] / 1e3, 2),
                          torch_over_knn=round(tm["torch_knn"]["us"] / tm["knn_offsets"]["us"], 2),
                          torch_over_normals=round(tm["torch_normals"]["us"] / tm["normals_30"]["us"], 2))))


def one_step(n, a):
    import numpy as np
    pkg, torch, dev = _setup()
    R, J = 32, 21
    td, to, th = _pack(pkg, torch, dev, n)
    ab = pkg.aabb(td, to, th, res=R)
    centres = ab.grid[:, :3].contiguous()
    noise = torch.from_numpy(np.random.default_rng(1).normal(0, 40, (n, J, 3)).astype(np.float32)).to(dev)
    gt = (centres[:, None, :] + noise).reshape(n, 3 * J).contiguous()
    index = torch.arange(n, dtype=torch.int64, device=dev)
    kw = dict(gt=gt, centres=centres, res=R, dtype=torch.bfloat16, fps=(M,))
    steps = {"step_fps": pkg.AugmentedStep(td, to, th, n, **kw),
             "step_groups": pkg.AugmentedStep(td, to, th, n, groups=LEVELS, normals=NORMALS_K, **kw)}
    counter = [0]

    def leg(s):
        def fn():
            counter[0] += n
            s.step(index, KEY, counter[0])
        return fn
    t = _measure({k: leg(s) for k, s in steps.items()}, a)
    over = int((steps["step_groups"].cloud_status == 3).sum())
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), n=n, res=R, fps_points=M, levels=LEVELS, normals_k=NORMALS_K,
                          over_capacity=over, **t, groups_add_us=round(t["step_groups"]["us"] - t["step_fps"]["us"], 2),
                          with_over_without=round(t["step_groups"]["us"] / t["step_fps"]["us"], 3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--limit", type=int, default=500, help="seconds per child process")
    ap.add_argument("--one", type=int, metavar="N")
    ap.add_argument("--step", type=int, metavar="N")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group", "bench_group.json"))
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
            raise SystemExit(f"bench_group.py {' '.join(step)} ended with status {r.returncode}")
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
