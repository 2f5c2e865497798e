"""Times the sfm2gt estimation (neuralrecon_w_amd.align, csrc/ncw_align.hip): 1 M source points against a 20 M-point synthetic
surface cloud.

    python scripts/bench_align.py [--target 20000000] [--source 1000000] [--repeat 7] [--out profiles/align/align_bench.json]

All in one call, warm, device events, medians over --repeat:
  * the target build once (AlignTarget: upload, recentring, the NNGrid) and the spacing measurement behind the default gate_min;
  * ONE iteration split into its stages -- transform (ncw_align_transform), compaction + cell keys + sort (torch.nonzero /
    index_select, ncw_nn_cell_keys, torch.sort), query (ncw_nn_query and the escape launch), sums (ncw_align_sums, both launches),
    host solve with its read-back of 22 numbers -- at the first gate and at a late one;
  * the sums launch beside the same 20 sums composed in torch (index_select, a mask, einsum / sum in float64), alternating, with
    the distance between the two results and whether two runs of each agree bit for bit;
  * a whole icp_similarity call from a perturbed start, its iterations and the error of the matrix it returns;
  * the radius-bounded query (NNGrid.query_within: ncw_nn_query_within at align.gate_bound(gate), one launch, no brute-force pass)
    beside the query stage at both gates, alternating in the same loop (`query_within`, with the min / max of both), and a third
    whole call with bounded=True beside the plain and the skip_far ones; --icp_repeat further skip_far / bounded pairs,
    alternating, give the spread of the whole call (`icp_call.bounded`).
The cloud: three rectangles meeting at a corner and a Gaussian bump, 30 x 20 x 15 units, uniform by area, offset far from the
origin.  The source: target points carried back by a known similarity, a fifth of them replaced by uniform outliers.
Prints one JSON line and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import align  # noqa: E402
from neuralrecon_w_amd import lib as L  # noqa: E402


def surface(n, gen, dev):
    """n float64 points: floor 30 x 20 with a bump, wall 30 x 15, wall 20 x 10, by area; offset (1000, -500, 200)."""
    areas = torch.tensor([600.0, 450.0, 200.0])
    which = torch.searchsorted(torch.cumsum(areas / areas.sum(), 0)[:2].contiguous(), torch.rand(n, generator=gen)).to(dev)
    u = torch.rand(n, generator=gen, dtype=torch.float64).to(dev)
    v = torch.rand(n, generator=gen, dtype=torch.float64).to(dev)
    z0 = torch.zeros_like(u)
    floor = torch.stack([30 * u, 20 * v, 4.0 * torch.exp(-((30 * u - 18) ** 2 + (20 * v - 11) ** 2) / (2 * 3.0 ** 2))], -1)
    wall_a = torch.stack([30 * u, z0, 15 * v], -1)
    wall_b = torch.stack([z0, 20 * u, 10 * v], -1)
    x = torch.where((which == 0)[:, None], floor, torch.where((which == 1)[:, None], wall_a, wall_b))
    return x + torch.tensor([1000.0, -500.0, 200.0], dtype=torch.float64, device=dev)


def similarity(scale, axis, degrees, t):
    k = np.asarray(axis, dtype=np.float64)
    k /= np.linalg.norm(k)
    a = np.radians(degrees)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = scale * (np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K))
    T[:3, 3] = t
    return T


def apply(T, x):
    T = torch.from_numpy(T).to(x.device)
    return x @ T[:3, :3].T + T[:3, 3]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def torch_sums(P, cp, Q, cq, idx, dist, gate, T):
    """The 20 sums and the count composed from torch ops (float64; the order of the sums is torch's)."""
    m = (idx >= 0) & (dist <= gate)
    j = idx.clamp(min=0)
    U = Q.index_select(0, j)
    w = m.to(torch.float64)[:, None]
    p, q = (P - cp) * w, (U - cq) * w
    A = T[:3, :3]
    d = (P @ A.T + T[:3, 3] - U) * w
    dd = dist.double() * w[:, 0]
    return torch.cat([p.sum(0), q.sum(0), torch.einsum("na,nb->ab", p, q).reshape(-1), (p * p).sum().reshape(1), (q * q).sum().reshape(1),
                      (d * d).sum().reshape(1), dd.sum().reshape(1), (dd * dd).sum().reshape(1)]), m.sum()


def iteration_stages(src, cp, target, T, gate, repeat):
    """Median ms of every stage of one iteration (NNGrid.query taken apart into its launches), and the pairs."""
    lib, g = L.get_lib(), target.grid
    dev = src.device
    s = L.stream_ptr(dev)
    rows = []
    for it in range(repeat + 1):
        r = {}
        r["transform"], (q32, inside) = timed(lambda: align.transform_points(src, T, target, gate))

        def compact():
            sel = torch.nonzero(inside, as_tuple=False).reshape(-1)
            q = q32.index_select(0, sel).contiguous()
            keys = torch.empty(q.shape[0], dtype=torch.int32, device=dev)
            L.check(lib.ncw_nn_cell_keys(L.ptr(q), q.shape[0], C.byref(g.cgrid), L.ptr(keys), s), "keys")
            return sel, q, torch.sort(keys, stable=True)[1].contiguous()

        r["compact_keys_sort"], (sel, q, order) = timed(compact)
        n = int(q.shape[0])

        def query():
            d = torch.empty(n, dtype=torch.float32, device=dev)
            i = torch.empty(n, dtype=torch.int64, device=dev)
            esc = torch.empty(n, dtype=torch.int32, device=dev)
            n_esc = torch.zeros(1, dtype=torch.int32, device=dev)
            L.check(lib.ncw_nn_query(L.ptr(g.pts), L.ptr(g.range), L.ptr(q), L.ptr(order), n, C.byref(g.cgrid), g.max_shell, float(g.margin),
                                     L.ptr(d), L.ptr(i), L.ptr(esc), L.ptr(n_esc), s), "query")
            ne = int(n_esc.item())
            if ne:
                scratch = torch.empty(ne, dtype=torch.int64, device=dev)
                L.check(lib.ncw_nn_brute(L.ptr(g.pts), g.m, L.ptr(q), L.ptr(esc), ne, L.ptr(scratch), L.ptr(d), L.ptr(i), s), "brute")
            idx = torch.full((src.shape[0],), -1, dtype=torch.int64, device=dev)
            dist = torch.full((src.shape[0],), float("inf"), dtype=torch.float32, device=dev)
            idx[sel], dist[sel] = i, d
            return idx, dist, ne

        r["query"], (idx, dist, ne) = timed(query)

        def query_within():
            d = torch.empty(n, dtype=torch.float32, device=dev)
            i = torch.empty(n, dtype=torch.int64, device=dev)
            L.check(lib.ncw_nn_query_within(L.ptr(g.pts), L.ptr(g.range), L.ptr(g.coarse), g.coarse_block, L.ptr(q), L.ptr(order), n,
                                            C.byref(g.cgrid), float(g.margin), align.gate_bound(gate), L.ptr(d), L.ptr(i), s), "within")
            idx = torch.full((src.shape[0],), -1, dtype=torch.int64, device=dev)
            dist = torch.full((src.shape[0],), float("inf"), dtype=torch.float32, device=dev)
            idx[sel], dist[sel] = i, d
            return idx, dist

        if g.coarse is None:
            g.build_coarse()
        r["query_within"], (idx_w, dist_w) = timed(query_within)
        r["sums"], (sums, counts) = timed(lambda: align.correspondence_sums(src, cp, target, idx, dist, gate, T))

        def solve():
            sh, ch = sums.cpu().numpy(), counts.cpu().numpy()
            return align.similarity_from_sums(int(ch[0]), sh, cp, target.centre), int(ch[0])

        r["solve_with_readback"], (_, pairs) = timed(solve)
        r["total"] = sum(v for k, v in r.items() if k != "query_within")
        if it:
            rows.append(r)
    out = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    m, mw = (idx >= 0) & (dist <= gate), (idx_w >= 0) & (dist_w <= gate)
    out.update(inside=n, pairs=pairs, escaped=ne, gate=float(gate), query_min_max=[min(r["query"] for r in rows), max(r["query"] for r in rows)],
               query_within_min_max=[min(r["query_within"] for r in rows), max(r["query_within"] for r in rows)],
               within_bound=align.gate_bound(gate), within_beyond=int((idx_w[sel] < 0).sum()),
               within_same_pairs=bool(torch.equal(m, mw) and torch.equal(idx[m], idx_w[m]) and torch.equal(dist[m], dist_w[m])),
               coarse_block=g.coarse_block, coarse_entries=int(g.coarse.numel()))
    out["query_within_outside_query_spread"] = bool(out["query_within_min_max"][1] < out["query_min_max"][0])
    return out, idx, dist


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", type=int, default=20_000_000)
    ap.add_argument("--source", type=int, default=1_000_000)
    ap.add_argument("--outliers", type=float, default=0.2)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max_shell", type=int, default=None, help="NNGrid shells before the brute-force path (default: evalmesh.MAX_SHELL)")
    ap.add_argument("--no_icp", action="store_true", help="skip the whole icp_similarity calls")
    ap.add_argument("--no_plain_icp", action="store_true", help="skip the plain whole call (brute-force pass in every iteration): skip_far and bounded only")
    ap.add_argument("--icp_repeat", type=int, default=3, help="further skip_far / bounded whole calls, alternating: the spread")
    ap.add_argument("--out", default=os.path.join("profiles", "align", "align_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise L.NeuconwHipError("bench_align needs a GPU: nothing here is measured on the CPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator().manual_seed(args.seed)
    gt = surface(args.target, gen, dev)
    truth = similarity(3.7, [0.3, -0.5, 0.8], 40.0, [0.0, 0.0, 0.0])
    truth[:3, 3] = gt.mean(0).cpu().numpy() - truth[:3, :3] @ np.array([0.7, -0.2, 0.4])
    inv = np.linalg.inv(truth)
    pick = torch.randint(0, args.target, (args.source,), generator=gen).to(dev)
    src_gt = gt[pick]
    n_out = int(args.outliers * args.source)
    lo, hi = gt.amin(0) - 2.0, gt.amax(0) + 2.0
    src_gt[:n_out] = lo + (hi - lo) * torch.rand(n_out, 3, generator=gen, dtype=torch.float64).to(dev)
    src = apply(inv, src_gt).contiguous()
    centre = gt.mean(0).cpu().numpy()
    pert = similarity(1.02, [0.6, 0.7, -0.2], 3.0, [0.3, -0.3, 0.2])
    pert[:3, 3] += centre - pert[:3, :3] @ centre
    init = pert @ truth
    res = {"what": "sfm2gt estimation: gated similarity ICP, per stage", "target_points": args.target, "source_points": args.source,
           "outlier_share": args.outliers, "repeat": args.repeat, "device": torch.cuda.get_device_name(dev)}

    kw = {} if args.max_shell is None else {"max_shell": args.max_shell}
    t_build, target = timed(lambda: align.AlignTarget(gt, dev, **kw))
    t_build2, target = timed(lambda: align.AlignTarget(gt, dev, **kw))              # warm
    res["max_shell"] = target.grid.max_shell
    res["target_build_ms"] = {"first": t_build, "warm": t_build2, "cells": target.grid.ncells, "dims": list(target.grid.dims),
                              "refined": bool(target.grid.refined)}
    t_sp, spacing = timed(target.spacing)
    res["spacing_ms"], res["spacing"] = t_sp, spacing
    gate0, gate_min = align.DEFAULT_GATE0 * target.longest_edge, align.DEFAULT_GATE_MIN * spacing
    res["gate0"], res["gate_min"] = gate0, gate_min
    cp = src.cpu().numpy().mean(0)

    res["iteration_first_gate_ms"], idx, dist = iteration_stages(src, cp, target, init, float(np.float32(gate0)), args.repeat)
    res["iteration_late_gate_ms"], idx_l, dist_l = iteration_stages(src, cp, target, truth, float(np.float32(gate_min)), args.repeat)

    # compaction + keys + sort + query of the late gate as `correspondences` runs them, with and without the far skip, alternating
    g_late = float(np.float32(gate_min))
    q32, inside = align.transform_points(src, truth, target, g_late)
    plain = lambda: align.correspondences(q32, inside, target)
    skip = lambda: align.correspondences(q32, inside, target, g_late)
    plain(), skip()
    torch.cuda.synchronize()
    tp, ts = [], []
    for _ in range(args.repeat):
        tp.append(timed(plain)[0])
        ts.append(timed(skip)[0])
    (i1, d1), (i2, d2) = plain(), skip()
    m1, m2 = (i1 >= 0) & (d1 <= g_late), (i2 >= 0) & (d2 <= g_late)
    res["correspondences_late_gate"] = {"ms": float(np.median(tp)), "min_max_ms": [min(tp), max(tp)], "skip_far_ms": float(np.median(ts)),
                                        "skip_far_min_max_ms": [min(ts), max(ts)], "far_reach": align.far_reach(target.grid),
                                        "same_pairs": bool(torch.equal(m1, m2) and torch.equal(i1[m1], i2[m2]) and torch.equal(d1[m1], d2[m2])),
                                        "skipped": int(((i2 < 0) & (i1 >= 0)).sum())}

    # the sums launch beside the torch composition, alternating
    cpd, cqd = torch.from_numpy(cp).to(dev), torch.from_numpy(target.centre).to(dev)
    Td = torch.from_numpy(init).to(dev)
    gate = float(np.float32(gate0))
    fused = lambda: align.correspondence_sums(src, cp, target, idx, dist, gate, init)
    composed = lambda: torch_sums(src, cpd, target.points, cqd, idx, dist, gate, Td)
    fused(), composed()
    torch.cuda.synchronize()
    tf, tc = [], []
    for _ in range(args.repeat):
        tf.append(timed(fused)[0])
        tc.append(timed(composed)[0])
    (s1, c1), (s2, c2) = fused(), fused()
    (t1, n1), (t2, n2) = composed(), composed()
    scale = float(s1.abs().max())
    res["sums_vs_torch"] = {"fused_ms": float(np.median(tf)), "fused_min_max_ms": [min(tf), max(tf)], "torch_ms": float(np.median(tc)),
                            "torch_min_max_ms": [min(tc), max(tc)], "pairs": int(c1[0]), "torch_pairs": int(n1),
                            "fused_two_runs_bit_equal": bool(torch.equal(s1, s2)), "torch_two_runs_bit_equal": bool(torch.equal(t1, t2)),
                            "max_abs_difference_over_largest_sum": float((s1 - t1).abs().max()) / scale,
                            "bytes_read": 24.0 * args.source + 12.0 * args.source + 24.0 * int(c1[0])}
    res["sums_vs_torch"]["fused_GBps"] = res["sums_vs_torch"]["bytes_read"] / (res["sums_vs_torch"]["fused_ms"] * 1e-3) / 1e9

    if args.no_icp:
        return finish(res, args)
    # a whole call, as icp_similarity runs it and with skip_far (the same matrices, bit for bit)
    st, st2, st3 = {}, {}, {}
    t_icp2, T2 = timed(lambda: align.icp_similarity(src, target, init, stats=st2, skip_far=True))
    t_icp3, T3 = timed(lambda: align.icp_similarity(src, target, init, stats=st3, bounded=True))
    same3 = all(np.array_equal(a["matrix"], b["matrix"]) and a["pairs"] == b["pairs"] and a["rms"] == b["rms"]
                for a, b in zip(st2["history"], st3["history"]))
    t_skip, t_bnd = [t_icp2], [t_icp3]
    for _ in range(args.icp_repeat):
        t_skip.append(timed(lambda: align.icp_similarity(src, target, init, skip_far=True))[0])
        t_bnd.append(timed(lambda: align.icp_similarity(src, target, init, bounded=True))[0])
    bounded = {"ms": float(np.median(t_bnd)), "min_max_ms": [min(t_bnd), max(t_bnd)], "skip_far_ms": float(np.median(t_skip)),
               "skip_far_min_max_ms": [min(t_skip), max(t_skip)], "calls_each": len(t_bnd), "iterations": st3["iterations"],
               "same_bits_every_iteration": bool(same3 and np.array_equal(T2, T3) and st2["iterations"] == st3["iterations"]),
               "outside_skip_far_spread": bool(max(t_bnd) < min(t_skip)),
               "beyond_per_iteration": [h["beyond"] for h in st3["history"]],
               "escaped_per_iteration": [h["escaped"] for h in st3["history"]]}
    if args.no_plain_icp:
        res["icp_call"] = {"bounded": bounded, "ms_skip_far": t_icp2, "iterations_skip_far": st2["iterations"],
                           "far_reach": align.far_reach(target.grid), "gate_per_iteration": [h["gate"] for h in st2["history"]],
                           "skipped_far_per_iteration": [h["skipped_far"] for h in st2["history"]],
                           "max_abs_error_over_max_abs_truth": float(np.abs(T3 - truth).max() / np.abs(truth).max())}
        return finish(res, args)
    t_icp, T = timed(lambda: align.icp_similarity(src, target, init, stats=st))
    same = all(np.array_equal(a["matrix"], b["matrix"]) and a["pairs"] == b["pairs"] for a, b in zip(st["history"], st2["history"]))
    res["icp_call"] = {"ms": t_icp, "ms_skip_far": t_icp2, "iterations": st["iterations"], "iterations_skip_far": st2["iterations"],
                       "converged": st["converged"], "ms_per_iteration": t_icp / st["iterations"],
                       "ms_per_iteration_skip_far": t_icp2 / st2["iterations"], "pairs": st["history"][-1]["pairs"],
                       "rms": st["history"][-1]["rms"], "skip_far_same_bits_every_iteration": bool(same and np.array_equal(T, T2)),
                       "far_reach": align.far_reach(target.grid),
                       "max_abs_error_over_max_abs_truth": float(np.abs(T - truth).max() / np.abs(truth).max()),
                       "pairs_per_iteration": [h["pairs"] for h in st["history"]],
                       "gate_per_iteration": [h["gate"] for h in st2["history"]],
                       "skipped_far_per_iteration": [h["skipped_far"] for h in st2["history"]],
                       "escaped_per_iteration": [h["escaped"] for h in st["history"]]}
    bounded["same_bits_every_iteration"] = bool(bounded["same_bits_every_iteration"] and same and np.array_equal(T, T3))
    res["icp_call"]["bounded"] = bounded
    return finish(res, args)


def finish(res, args):
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
