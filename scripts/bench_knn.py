"""Times the exact k-NN grid walk (evalmesh.NNGrid.query_k, csrc/ncw_knn.hip) and the per-point PCA on synthetic clouds.

    python scripts/bench_knn.py [--points 2000000] [--repeat 7] [--scipy_points 2000000] [--out profiles/knn/knn_bench.json]

Two clouds: a curved sheet (a 30 x 20 floor with a bump, uniform by area) and the same sheet with 1 % of its points replaced
by points uniform in the box around it, which sends their queries -- and those of their neighbours -- through the coarse
walk.  Each cloud queries ITSELF with its own index excluded (what cloudops.estimate_normals does), at k = 1 / 8 / 16 / 32,
beside NNGrid.query (k = 1, no exclusion: every answer is the point itself at d = 0, the cheapest walk there is) in the same
call; the workgroup sizes 64 / 128 / 256 at every k; ncw_knn_pca at k = 16; if scipy imports, cKDTree.query(k + 1,
workers=16) on the host.  One call, warm, device events, the variants alternating inside every repeat, medians and min /
max over --repeat.  `evals` / `inserts`: distance evaluations and list insertions per query, counted by the kernel.  Prints
one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import cloudops, evalmesh  # noqa: E402
from neuralrecon_w_amd import lib as L  # noqa: E402

KS = (1, 8, 16, 32)
WGS = (64, 128, 256)


def sheet(n, gen):
    u, v = torch.rand(n, generator=gen, dtype=torch.float64), torch.rand(n, generator=gen, dtype=torch.float64)
    return torch.stack([30 * u, 20 * v, 4.0 * torch.exp(-((30 * u - 18) ** 2 + (20 * v - 11) ** 2) / (2 * 3.0 ** 2))], -1)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stat(ts):
    return {"ms": float(np.median(ts)), "min_max_ms": [float(min(ts)), float(max(ts))]}


def measure(points, dev, repeat, scipy_points):
    p32, _, cmax, _ = evalmesh.recentre(points.to(dev), points.to(dev))
    grid = evalmesh.NNGrid(p32, cmax)
    n = int(p32.shape[0])
    own = torch.arange(n, dtype=torch.int32, device=dev)
    variants = {("query", 1, 0): lambda: grid.query(p32)}
    for k in KS:
        for wg in WGS:
            variants[("query_k", k, wg)] = (lambda k=k, wg=wg: grid.query_k(p32, k, exclude=own, wg=wg))
    for fn in variants.values():
        fn()                                                         # warm: the coarse level is built here
    torch.cuda.synchronize()
    times = {key: [] for key in variants}
    for _ in range(repeat):
        for key, fn in variants.items():                             # alternating: every variant once per repeat
            times[key].append(timed(fn))
    res = {"points": n, "dims": list(grid.dims), "cells": grid.ncells, "refined": bool(grid.refined),
           "coarse_block": grid.coarse_block, "nn_query_k1": stat(times[("query", 1, 0)]), "query_k": {}}
    for k in KS:
        st = {}
        _, idx, cnt = grid.query_k(p32, k, exclude=own, stats=st)
        row = {"wg%d" % wg: stat(times[("query_k", k, wg)]) for wg in WGS}
        row.update(evals_per_query=st["evals"] / float(n), inserts_per_query=st["inserts"] / float(n),
                   full_rows=float((cnt == k).float().mean()))
        res["query_k"]["k%d" % k] = row
    _, idx, cnt = grid.query_k(p32, 16, exclude=own)
    cloudops.pca(p32, p32, idx, cnt)
    torch.cuda.synchronize()
    res["pca_k16"] = stat([timed(lambda: cloudops.pca(p32, p32, idx, cnt)) for _ in range(repeat)])
    res["pca_valid"] = float(cloudops.pca(p32, p32, idx, cnt)[3].float().mean())
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        res["ckdtree"] = None
    else:
        m = min(n, int(scipy_points))
        host = p32[:m].double().cpu().numpy()
        t0 = time.perf_counter()
        tree = cKDTree(host)
        res["ckdtree"] = {"points": m, "build_s": time.perf_counter() - t0}
        for k in KS:
            t0 = time.perf_counter()
            tree.query(host, k=k + 1, workers=16)                    # k + 1: the point itself comes first
            res["ckdtree"]["k%d_s" % k] = time.perf_counter() - t0
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--outliers", type=float, default=0.01, help="share of the second cloud that is uniform in the box")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--scipy_points", type=int, default=2_000_000, help="points of the host cKDTree run (a prefix of the cloud)")
    ap.add_argument("--out", default=os.path.join("profiles", "knn", "knn_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise L.NeuconwHipError("bench_knn needs a GPU: nothing here is measured on the CPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator().manual_seed(args.seed)
    clean = sheet(args.points, gen)
    n_out = int(args.outliers * args.points)
    stray = torch.rand(n_out, 3, generator=gen, dtype=torch.float64) * torch.tensor([30.0, 20.0, 10.0]) - torch.tensor([0.0, 0.0, 3.0])
    dirty = torch.cat([clean[: args.points - n_out], stray])
    res = {"what": "NNGrid.query_k self-query (own index excluded) beside NNGrid.query; ncw_knn_pca; cKDTree on the host",
           "device": torch.cuda.get_device_name(dev), "repeat": args.repeat,
           "sheet": measure(clean, dev, args.repeat, args.scipy_points),
           "sheet_with_outliers": measure(dirty, dev, args.repeat, args.scipy_points)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
