"""Timing of the mesh evaluation's GPU path (neuralrecon_w_amd.evalmesh): exact 1-NN in both directions between seeded
synthetic clouds and the metrics over 99 thresholds.  Prints ONE JSON line.

    python scripts/bench_eval_mesh.py [--n_query 1000000] [--n_ref 2000000] [--outliers 64] [--reps 5] [--no_cpu]

Clouds: points on an analytic surface (a wavy sphere of radius ~20 m, 1e-3 m Gaussian noise, centred 500 m from the origin),
plus a few far outliers among the queries (the brute-force escape path).  Times are HIP events around synchronised work
(median of --reps runs after one warm-up): grid build (cell keys, sort, cell table), query per direction (query keys, sort,
shell search, escape pass), metrics.  When scipy imports, `cKDTree.query(workers=16)` on the same float64 clouds is timed
beside it as a CPU comparison.  Kernel names for `rocprofv3 --kernel-trace --stats`: nn_cell_keys_kernel,
nn_cell_ranges_kernel, nn_query_kernel, nn_brute_kernel, nn_brute_finish_kernel.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import evalmesh  # noqa: E402


def surface(n, seed, outliers=0):
    rng = np.random.RandomState(seed)
    d = rng.randn(n, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    theta, phi = np.arccos(np.clip(d[:, 2], -1, 1)), np.arctan2(d[:, 1], d[:, 0])
    r = 20.0 * (1.0 + 0.1 * np.sin(5 * theta) * np.cos(4 * phi))
    p = d * r[:, None] + rng.randn(n, 3) * 1e-3 + np.array([500.0, -300.0, 40.0])
    if outliers:
        p[rng.choice(n, outliers, replace=False)] += rng.randn(outliers, 3) * 200.0
    return p


def timed(fn, reps):
    out, ts = None, []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if i:
            ts.append(e0.elapsed_time(e1))
    return out, float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_query", type=int, default=1_000_000)
    ap.add_argument("--n_ref", type=int, default=2_000_000)
    ap.add_argument("--outliers", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no_cpu", action="store_true", help="skip the scipy cKDTree comparison")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    P = surface(args.n_ref, 1)
    Q = surface(args.n_query, 2, args.outliers)
    Pg, Qg = torch.from_numpy(P).to(dev), torch.from_numpy(Q).to(dev)
    r32, q32, cmax, _ = evalmesh.recentre(Pg, Qg)
    res = {"bench": "eval_mesh_nn", "n_ref": args.n_ref, "n_query": args.n_query, "outliers": args.outliers}

    grid_pq, res["grid_build_ms"] = timed(lambda: evalmesh.NNGrid(r32, cmax), args.reps)
    st = {}
    (d_qp, _), res["query_ms_q_to_p"] = timed(lambda: grid_pq.query(q32), args.reps)
    grid_pq.query(q32, st)
    res.update(grid_dims=grid_pq.dims, grid_refined=grid_pq.refined, escaped_q_to_p=st["escaped"])
    grid_qp, res["grid_build_ms_reverse"] = timed(lambda: evalmesh.NNGrid(q32, cmax), args.reps)
    st = {}
    (d_pq, _), res["query_ms_p_to_q"] = timed(lambda: grid_qp.query(r32), args.reps)
    grid_qp.query(r32, st)
    res.update(grid_dims_reverse=grid_qp.dims, escaped_p_to_q=st["escaped"])
    thresholds = [float(t) for t in np.arange(0.01, 1, 0.01)]
    m, res["metrics_ms_99_thresholds"] = timed(lambda: evalmesh.metrics(d_qp, d_pq, thresholds), args.reps)
    res["fscore_at_0.01"] = m[0]["fscore"]
    if not args.no_cpu:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            cKDTree = None
        if cKDTree is not None:
            t0 = time.perf_counter()
            tree = cKDTree(P)
            t1 = time.perf_counter()
            dk, _ = tree.query(Q, k=1, workers=16)
            t2 = time.perf_counter()
            res["cpu_comparison_scipy_ckdtree"] = {"build_ms": 1e3 * (t1 - t0), "query_ms_q_to_p_workers16": 1e3 * (t2 - t1)}
            res["max_abs_diff_vs_ckdtree"] = float(np.max(np.abs(d_qp.double().cpu().numpy() - dk)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
