"""Times the reprojection filter's marking (reproj.Target.mark) with the radius-bounded nearest-neighbour query beside the earlier
unbounded one, for a SOURCE that is not the target: most back-projected points then have no target vertex within the threshold.

    python scripts/bench_nn_within.py [--target 2000000] [--queries 500000] [--repeat 7] [--out profiles/reproj/nn_within_bench.json]

The target: a 30 x 20 floor with a bump, uniform by area (the vertices of a prediction).  The queries: one view's worth of
back-projected points of ANOTHER surface -- the same floor for `--near` of them (within the threshold of a vertex), and a wall and
scattered points above it for the rest.  Both paths in one call, warm, device events, alternating, medians and min / max over
--repeat; the flags must be equal.  Prints one JSON line (`within`) and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import lib as L  # noqa: E402
from neuralrecon_w_amd import reproj  # noqa: E402


def floor(n, gen):
    u, v = torch.rand(n, generator=gen, dtype=torch.float64), torch.rand(n, generator=gen, dtype=torch.float64)
    return torch.stack([30 * u, 20 * v, 4.0 * torch.exp(-((30 * u - 18) ** 2 + (20 * v - 11) ** 2) / (2 * 3.0 ** 2))], -1)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", type=int, default=2_000_000)
    ap.add_argument("--queries", type=int, default=500_000)
    ap.add_argument("--near", type=float, default=0.3, help="share of the queries that lie on the target's own surface")
    ap.add_argument("--voxel_size", type=float, default=0.01)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join("profiles", "reproj", "nn_within_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise L.NeuconwHipError("bench_nn_within needs a GPU: nothing here is measured on the CPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator().manual_seed(args.seed)
    xyz = floor(args.target, gen).numpy()
    n_near = int(args.near * args.queries)
    n_wall = (args.queries - n_near) // 2
    n_air = args.queries - n_near - n_wall
    u, v = torch.rand(n_wall, generator=gen, dtype=torch.float64), torch.rand(n_wall, generator=gen, dtype=torch.float64)
    wall = torch.stack([30 * u, torch.zeros_like(u), 0.5 + 14.5 * v], -1)
    air = torch.rand(n_air, 3, generator=gen, dtype=torch.float64) * torch.tensor([30.0, 20.0, 10.0]) + torch.tensor([0.0, 0.0, 5.0])
    q = torch.cat([floor(n_near, gen), wall, air])
    thr = 2 * np.sqrt(2) * args.voxel_size
    targets = {b: reproj.Target(xyz, None, thr, dev, bounded=b) for b in (True, False)}
    centre = torch.from_numpy(targets[True].centre)

    def measure(points):
        q32 = (points - centre).float().to(dev).contiguous()
        for t in targets.values():
            t.flags.zero_()
            t.mark(q32)                                              # warm: the coarse level is built here
        torch.cuda.synchronize()
        tb, tu = [], []
        for _ in range(args.repeat):
            tu.append(timed(lambda: targets[False].mark(q32)))
            tb.append(timed(lambda: targets[True].mark(q32)))
        st, st0 = {}, {}
        targets[True].grid.query_within(q32, thr * (1 + 4 * float(np.finfo(np.float32).eps)), st)
        targets[False].grid.query(q32, st0)
        return {"queries": int(q32.shape[0]), "bounded_ms": float(np.median(tb)), "bounded_min_max_ms": [min(tb), max(tb)],
                "unbounded_ms": float(np.median(tu)), "unbounded_min_max_ms": [min(tu), max(tu)],
                "bounded_outside_unbounded_spread": bool(max(tb) < min(tu)), "beyond_share": st["beyond"] / float(q32.shape[0]),
                "escaped_unbounded": st0["escaped"], "flags_equal": bool(torch.equal(targets[True].flags, targets[False].flags)),
                "marked": int(targets[True].flags.sum())}

    g = targets[True].grid
    within = measure(q)
    within.update(target_vertices=args.target, threshold=thr, repeat=args.repeat, dims=list(g.dims), cells=g.ncells, refined=bool(g.refined),
                  coarse_block=g.coarse_block, coarse_entries=int(g.coarse.numel()))
    # the filter's usual input, source = target: every query lies on the target's own surface
    res = {"what": "reproj.Target.mark, a source that is not the target: bounded beside unbounded", "device": torch.cuda.get_device_name(dev),
           "within": within, "same_surface": measure(floor(args.queries, gen))}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
