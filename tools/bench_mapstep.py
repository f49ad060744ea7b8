#!/usr/bin/env python3
"""What the augmented training step costs with its head fused into one launch, and in a base (OBB) frame (one JSON line;
``--out`` also writes it to a file, default profiles/mapstep/bench_mapstep.json).

Legs, per batch size, on the same resident pack, every step a host-side upload of the batch's frame numbers and
``{key, counter0}`` and one graph replay:
  step_lowp          AugmentedStep(dtype, graph=True)                    as it was before libtsdf_mapstep.so: THE YARDSTICK
                                                                         (this leg runs unchanged on the parent commit)
  step_lowp_fused    AugmentedStep(dtype, graph=True, fused_head=True)   map_step_head + the voxel pass
  base_lowp_head     AugmentedStep(dtype, graph=True, base=obb)          the same two launches under the composed maps
  base_lowp_chain    the explicit chain under the composed maps, captured into a graph over static buffers like the step:
                     aug_xforms_at, compose_xforms, map_grids, voxelize_map_grid_lowp, the joints' gather (clamp,
                     index_select), transform_joints, normalize_joints
  step_f32           AugmentedStep(graph=True)                           the fused float32 kernel after the draw
  base_f32           AugmentedStep(graph=True, base=obb)                 ... after map_step_head(place=False)
and the launches alone, eagerly into preallocated outputs:
  head               map_step_head(base=obb, gt=...)                     draw, compose, placement, labels
  place              map_grids()                                         the placement alone, next to `head`
  draw               aug_xforms_at()
  compose            compose_xforms()
at 16 and at 1024 crops, R = 32, bfloat16 (``--dtype float16`` for the other type).  Legs whose names the package does
not have yet are left out, so the tool measures the yardstick on an older tree.

Method: device events around --iters back-to-back steps (at least 50); the legs of a shape take turns for --rounds
rounds and the median round is reported with min and max, so a drift of the machine meets all alike.  No threshold is
applied: the ratios to the yardstick are printed next to the spread of the yardstick's own rounds.  ``--lib`` names
another build of libtsdf_mapstep.so and ``--maplowp-lib`` one of libtsdf_maplowp.so, whose placement the chained legs and
`place` launch (an A/B against the parent commit's: one process per build, taking turns).

    python tools/bench_mapstep.py [--iters 100] [--warmup 20] [--rounds 5] [--dtype bfloat16] [--lib x.so]
                                  [--maplowp-lib y.so] [--out x.json]
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


class ChainStep:
    """The composed step as the chain of the entries that existed before map_step_head, in AugmentedStep's form: static
    buffers, one upload, one graph replay."""

    def __init__(self, td, to, th, gt, base, centres, n, R, dt):
        dev = td.device
        self._in = torch.zeros(n + 2, dtype=torch.int64, device=dev)
        self.index, self.state = self._in[:n], self._in[n:]
        self._h = torch.zeros(n + 2, dtype=torch.int64).pin_memory()
        self.U = torch.empty((n, 24), dtype=torch.float64, device=dev)
        self.T = torch.empty((n, 24), dtype=torch.float64, device=dev)

        def run():
            pkg.aug_xforms_at(centres, self.state, index=self.index, out=self.U)
            pkg.compose_xforms(self.U, base, self.index, out=self.T)
            self.res = pkg.voxelize_aug_lowp(td, to, th, self.T, res=R, dtype=dt, gt=gt, index=self.index)

        run()
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=torch.cuda.Stream(dev)):
            run()

    def step(self, index, key, counter0):
        hn = self._h.numpy()
        hn[:-2] = index.numpy()
        hn[-2], hn[-1] = key, counter0
        self._in.copy_(self._h, non_blocking=True)
        self.graph.replay()
        return self.res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtype", choices=("bfloat16", "float16"), default="bfloat16")
    ap.add_argument("--lib")
    ap.add_argument("--maplowp-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapstep", "bench_mapstep.json"))
    a = ap.parse_args()
    assert a.iters >= 50, "time at least 50 steps"
    assert torch.cuda.is_available(), "bench_mapstep.py needs a HIP device"
    for name, path in (("mapstep", a.lib), ("maplowp", a.maplowp_lib)):
        if path:
            row = pkg._lib._EXTS[name]
            pkg._lib._EXTS[name] = row._replace(path=os.path.abspath(path))
    dev = torch.device("cuda:0")
    dt = getattr(torch, a.dtype)
    have = hasattr(pkg, "map_step_head")
    R = 32
    rows = []
    for n in (16, 1024):
        depth, off, hdr = synth.synth_batch(n, "crop", seed0=0, threads=8)
        td, to, th = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depth, off, hdr))
        ab = pkg.aabb(td, to, th, res=R)
        assert not ab.status.any()
        c_cam = ab.grid[:, :3].contiguous()
        gt = (c_cam[:, None, :] + 40 * torch.randn((n, 21, 3), device=dev, generator=torch.Generator(dev).manual_seed(1)))
        gt = gt.reshape(n, 63).contiguous()
        index = torch.from_numpy(np.random.default_rng(n).permutation(n).astype(np.int64))
        count = [0]

        def stepper(obj):
            def go():
                count[0] += n
                return obj.step(index, 0x5EED, count[0])
            return go

        kw = dict(gt=gt, res=R, graph=True)
        legs = {"step_lowp": stepper(pkg.AugmentedStep(td, to, th, n, centres=c_cam, dtype=dt, **kw))}
        if have:
            base = pkg.obb_xforms(td, to, th)
            assert not base.status.any()
            base = base.xforms
            with_base = pkg.AugmentedStep(td, to, th, n, dtype=dt, base=base, **kw)
            c_obb = with_base.centres
            state = pkg.aug_state(0x5EED, 0, device=dev)
            ti = index.to(dev)
            U = pkg.aug_xforms_at(c_obb, state, index=ti)
            T = pkg.compose_xforms(U, base, ti)
            mg = pkg.map_grids(td, to, th, T, res=R, index=ti)
            hb = pkg.map_step_head(td, to, th, c_obb, state, base=base, index=ti, gt=gt, res=R)
            assert torch.equal(hb.xforms, T) and torch.equal(hb.grid, mg.grid) and not mg.status.any()
            legs.update({
                "step_lowp_fused": stepper(pkg.AugmentedStep(td, to, th, n, centres=c_cam, dtype=dt, fused_head=True, **kw)),
                "base_lowp_head": stepper(with_base),
                "base_lowp_chain": stepper(ChainStep(td, to, th, gt, base, c_obb, n, R, dt))})
        legs["step_f32"] = stepper(pkg.AugmentedStep(td, to, th, n, centres=c_cam, **kw))
        if have:
            legs.update({
                "base_f32": stepper(pkg.AugmentedStep(td, to, th, n, base=base, **kw)),
                "head": lambda: pkg.map_step_head(td, to, th, c_obb, state, base=base, index=ti, gt=gt, res=R, out=hb),
                "place": lambda: pkg.map_grids(td, to, th, T, res=R, index=ti, out=mg),
                "draw": lambda: pkg.aug_xforms_at(c_obb, state, index=ti, out=U),
                "compose": lambda: pkg.compose_xforms(U, base, ti, out=T)})
        t = take_turns(legs, a.iters, a.warmup, a.rounds)
        y = t["step_lowp"]
        row = dict(n=n, kind="crop", res=R, dtype=a.dtype, pixels=int(depth.size), **t,
                   yardstick_spread=round(y["us_max"] / y["us_min"], 3))
        if have:
            row.update(fused_over_yardstick=round(t["step_lowp_fused"]["us"] / y["us"], 3),
                       base_head_over_yardstick=round(t["base_lowp_head"]["us"] / y["us"], 3),
                       base_head_over_base_chain=round(t["base_lowp_head"]["us"] / t["base_lowp_chain"]["us"], 3),
                       base_f32_over_step_f32=round(t["base_f32"]["us"] / t["step_f32"]["us"], 3),
                       head_over_place=round(t["head"]["us"] / t["place"]["us"], 3))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del legs
        torch.cuda.empty_cache()
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, rounds=a.rounds, rows=rows))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
