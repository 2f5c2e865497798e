"""Timing of the mesh evaluation's GPU path (neuralrecon_w_amd.evalmesh): exact 1-NN in both directions between seeded
synthetic clouds and the metrics over 99 thresholds.  Prints ONE JSON line.

    python scripts/bench_eval_mesh.py [--n_query 1000000] [--n_ref 2000000] [--outliers 64] [--reps 5] [--no_cpu]

Clouds: points on an analytic surface (a wavy sphere of radius ~20 m, 1e-3 m Gaussian noise, centred 500 m from the origin),
plus a few far outliers among the queries (the brute-force escape path).  Times are HIP events around synchronised work
(median of --reps runs after one warm-up): grid build (cell keys, sort, cell table), query per direction (query keys, sort,
shell search, escape pass), metrics.  When scipy imports, `cKDTree.query(workers=16)` on the same float64 clouds is timed
beside it as a CPU comparison.  Kernel names for `rocprofv3 --kernel-trace --stats`: nn_cell_keys_kernel,
nn_cell_ranges_kernel, nn_query_kernel, nn_brute_kernel, nn_brute_finish_kernel.

Surface sampling row (`surface_sampling` in the JSON line; --surf_samples 0 skips it): --surf_samples points (10 M) drawn by
area from a lat-long mesh of the same wavy sphere with --surf_faces triangles (2 M), float64.  The fused launch
(ncw_surf_sample, stratified and iid) is timed against the same distribution composed from torch ops on the same area
table: torch.rand x 3, torch.searchsorted, one gather of the faces, three gathers of the corners, the point formula.  Next
to each time: the bytes it moves.  For the fused kernel that is what the algorithm needs (area table, faces and vertices
read once, 24 bytes written per sample); for the composition it is the operand and result sizes of every torch op summed
(`composed_bytes`).  Kernel names: surf_weights_kernel, surf_sample_kernel.

Point-to-mesh row (`point_to_mesh` in the JSON line; --ptm_queries 0 skips it): the exact recall side (evalmesh.TriGrid,
csrc/ncw_ptm.hip) -- --ptm_queries points (1 M) near the surface against the lat-long mesh with --ptm_faces triangles (2 M),
float64: grid build (pack, count, prefix sum, emit, sort, cell table) and query (query keys, sort, large list + shell
search, escape pass) timed separately, with the grid's `pairs`, `large` and `escaped`.  Beside it, in the same call, the
path it replaces, composed from the functions that exist: `sample_surface` of --ptm_samples points (10 M) from the same
mesh, then `recentre` + `NNGrid` over the samples, then `query` of the same points (`sampled_recall`).  `mean_dist_*`: the
mean distance each path reports (the sampled one is the larger: its bias).  `query_ms_off_poles`: the exact query over the
queries more than 26 degrees from the poles only -- the lat-long mesh leaves a hole at each pole and crowds needle triangles
around it, so the few queries there walk several shells of full cells and set the launch's tail.  Kernel names: ptm_pack_kernel, ptm_count_kernel,
ptm_emit_kernel, ptm_ranges_kernel, ptm_cell_keys_kernel, ptm_query_kernel, ptm_brute_kernel, ptm_brute_finish_kernel.
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


def sphere_mesh(n_faces, dev):
    """Lat-long mesh of the wavy sphere: (float64 [V,3], int32 [F,3]) on the device, F = 2 q^2 close to n_faces."""
    q = max(2, int(round((n_faces / 2.0) ** 0.5)))
    th = torch.linspace(0.05, np.pi - 0.05, q + 1, dtype=torch.float64, device=dev)
    ph = torch.linspace(0.0, 2 * np.pi, q + 1, dtype=torch.float64, device=dev)
    T, P = torch.meshgrid(th, ph, indexing="ij")
    r = 20.0 * (1.0 + 0.1 * torch.sin(5 * T) * torch.cos(4 * P))
    v = torch.stack([r * torch.sin(T) * torch.cos(P), r * torch.sin(T) * torch.sin(P), r * torch.cos(T)], -1).reshape(-1, 3)
    v = v + torch.tensor([500.0, -300.0, 40.0], dtype=torch.float64, device=dev)
    i, j = torch.meshgrid(torch.arange(q, device=dev), torch.arange(q, device=dev), indexing="ij")
    a = (i * (q + 1) + j).reshape(-1)
    f = torch.cat([torch.stack([a, a + q + 1, a + 1], -1), torch.stack([a + 1, a + q + 1, a + q + 2], -1)])
    return v.contiguous(), f.int().contiguous()


def composed_sample(verts, faces64, cdf, n):
    """The fused kernel's distribution (iid) from torch ops; returns (points, bytes moved by the ops)."""
    dev, b = verts.device, 0
    u = torch.rand(n, dtype=torch.float64, device=dev)
    r1 = torch.rand(n, dtype=torch.float64, device=dev)
    r2 = torch.rand(n, dtype=torch.float64, device=dev)
    b += 3 * 8 * n
    x = u * cdf[-1]
    b += 16 * n
    k = torch.searchsorted(cdf, x, right=True).clamp_(max=cdf.shape[0] - 1)
    b += 16 * n + 8 * cdf.shape[0] + 16 * n
    f = faces64[k]
    b += 8 * n + 24 * n + 24 * faces64.shape[0]
    A, B, Cc = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    b += 3 * (8 * n + 8 * n + 24 * n) + 24 * verts.shape[0]  # column copy, index read, rows written; the table once
    s = torch.sqrt(r1)
    wa, wb, wc = 1.0 - s, s * (1.0 - r2), s * r2
    b += 16 * n + 16 * n + (16 * n + 24 * n) + 24 * n
    p = wa[:, None] * A + wb[:, None] * B + wc[:, None] * Cc
    b += 3 * (8 * n + 48 * n) + 2 * 72 * n
    return p, b


def bench_surface(args, dev, res):
    lib = evalmesh.L.get_lib()
    v, f = sphere_mesh(args.surf_faces, dev)
    n, nf = args.surf_samples, int(f.shape[0])
    out = {"n_samples": n, "n_faces": nf, "n_verts": int(v.shape[0])}
    cdf, out["weights_and_cdf_ms"] = timed(lambda: evalmesh.surface_cdf(evalmesh.surface_weights(v, f)), args.reps)
    pts = torch.empty(n, 3, dtype=torch.float64, device=dev)

    def fused(mode):
        evalmesh.L.check(lib.ncw_surf_sample(evalmesh.L.ptr(v), evalmesh.L.ptr(f), evalmesh.L.ptr(cdf), nf, 1, 0, n, n, mode,
                                             evalmesh.L.ptr(pts), None, None, evalmesh.L.stream_ptr(dev)), "ncw_surf_sample")
        return pts

    fused_bytes = 24 * n + 8 * nf + 12 * nf + 24 * int(v.shape[0])
    for mode, name in ((1, "stratified"), (0, "iid")):
        _, ms = timed(lambda: fused(mode), args.reps)
        out["fused_%s_ms" % name] = ms
        out["fused_%s_GBps" % name] = fused_bytes / ms * 1e-6
    out["fused_GB_moved"] = fused_bytes * 1e-9
    f64 = f.long()
    (p, cb), out["composed_torch_ms"] = timed(lambda: composed_sample(v, f64, cdf, n), args.reps)
    out["composed_GB_moved"] = cb * 1e-9
    out["composed_over_fused_iid"] = out["composed_torch_ms"] / out["fused_iid_ms"]
    # both draw from the same surface: the means agree to sampling noise (radius 20 m, n samples)
    out["mean_diff_m"] = float((p.mean(0) - fused(0).mean(0)).abs().max())
    res["surface_sampling"] = out


def bench_ptm(args, dev, res):
    v, f = sphere_mesh(args.ptm_faces, dev)
    q = torch.from_numpy(surface(args.ptm_queries, 3)).to(dev)
    out = {"n_queries": int(q.shape[0]), "n_faces": int(f.shape[0]), "n_verts": int(v.shape[0])}
    centre, cmax = evalmesh.ptm_centre(v, q)
    grid, out["build_ms"] = timed(lambda: evalmesh.TriGrid(v, f, centre, cmax), args.reps)
    (d_exact, _), out["query_ms"] = timed(lambda: grid.query(q), args.reps)
    st = {}
    grid.query(q, stats=st)
    out.update(grid_dims=st["dims"], cell_m=grid.h, pairs=st["pairs"], large=st["large"], escaped=st["escaped"],
               total_ms=out["build_ms"] + out["query_ms"], mean_dist_exact_m=float(d_exact.mean()))
    dirs = q - torch.tensor([500.0, -300.0, 40.0], dtype=torch.float64, device=dev)
    q_off = q[(dirs[:, 2].abs() < 0.9 * dirs.norm(dim=1))].contiguous()
    _, out["query_ms_off_poles"] = timed(lambda: grid.query(q_off), args.reps)
    out["n_queries_off_poles"] = int(q_off.shape[0])
    # the sampled recall this replaces: sample_surface -> NNGrid -> query
    samp = {"n_samples": args.ptm_samples}
    pts, samp["sample_ms"] = timed(lambda: evalmesh.sample_surface(v, f, args.ptm_samples, seed=0), args.reps)

    def build():
        r32, q32, c, _ = evalmesh.recentre(pts, q)
        return evalmesh.NNGrid(r32, c), q32

    (nn, q32), samp["grid_build_ms"] = timed(build, args.reps)
    (d_samp, _), samp["query_ms"] = timed(lambda: nn.query(q32), args.reps)
    st = {}
    nn.query(q32, st)
    samp.update(grid_dims=nn.dims, escaped=st["escaped"], total_ms=samp["sample_ms"] + samp["grid_build_ms"] + samp["query_ms"],
                mean_dist_sampled_m=float(d_samp.double().mean()))
    out["sampled_recall"] = samp
    out["exact_over_sampled_total"] = out["total_ms"] / samp["total_ms"]
    out["max_exact_minus_sampled_m"] = float((d_exact - d_samp.double()).max())
    res["point_to_mesh"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_query", type=int, default=1_000_000)
    ap.add_argument("--n_ref", type=int, default=2_000_000)
    ap.add_argument("--outliers", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no_cpu", action="store_true", help="skip the scipy cKDTree comparison")
    ap.add_argument("--surf_samples", type=int, default=10_000_000, help="surface sampling row: samples (0 = skip the row)")
    ap.add_argument("--surf_faces", type=int, default=2_000_000, help="surface sampling row: triangles of the mesh")
    ap.add_argument("--ptm_queries", type=int, default=1_000_000, help="point-to-mesh row: queries (0 = skip the row)")
    ap.add_argument("--ptm_faces", type=int, default=2_000_000, help="point-to-mesh row: triangles of the mesh")
    ap.add_argument("--ptm_samples", type=int, default=10_000_000, help="point-to-mesh row: samples of the sampled path beside it")
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
    if args.surf_samples > 0:
        bench_surface(args, dev, res)
    if args.ptm_queries > 0:
        bench_ptm(args, dev, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
