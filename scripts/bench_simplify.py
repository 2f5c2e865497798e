"""Times the mesh simplification (neuralrecon_w_amd.meshops.simplify, csrc/ncw_simplify.hip) on the synthetic marching-cubes
mesh of scripts/bench_meshops.py (about 20 M faces), at cells of 2, 4 and 8 voxels.

    python scripts/bench_simplify.py [--dim 864] [--repeat 5] [--cells 2 4 8] [--out profiles/simplify/simplify_bench.json]

Timed with device events, warm, medians over --repeat, all in one call:
  * every stage of `simplify` (prepare = participation + used flags + box, keys = ncw_mesh_sc_keys + the cluster numbering,
    faces = ncw_mesh_sc_faces, lists = the two stable sorts, place = ncw_mesh_sc_place, dedup = the duplicate faces, compaction =
    submesh + the index map) and the whole call; faces and vertices before and after;
  * beside it the obvious torch composition of the placement -- per-corner quadrics accumulated with index_add_, one batched
    torch.linalg.solve -- from the same cluster map.  Its sums run in whatever order the atomics land: it is NOT bitwise
    reproducible, which is the point of the comparison; the script reports its distance from the kernel's float64 vertices and whether
    two of its own runs agree bit for bit;
  * the bytes the place kernel gathers (24 B per member, 12 + 72 B per incidence) against its measured time;
  * --color_cell 4: mesh.vertex_colors (flagship widths, random weights) on the vertex counts before and after.
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_meshops import synthetic_sdf, timed  # noqa: E402
from neuralrecon_w_amd import mesh, meshops  # noqa: E402


def staged(verts, faces, h, repeat):
    """Median ms per stage and of the whole call (device events recorded inside simplify), the last result and its stats."""
    meshops.simplify(verts, faces, h)                                   # warm-up
    rows = []
    for _ in range(repeat):
        st = {"events": []}
        out = meshops.simplify(verts, faces, h, stats=st)
        torch.cuda.synchronize()
        ev = st["events"]
        row = {ev[i][0]: ev[i - 1][1].elapsed_time(ev[i][1]) for i in range(1, len(ev))}
        row["total"] = ev[0][1].elapsed_time(ev[-1][1])
        rows.append(row)
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}, out, st


def torch_placement(x, f, cluster, centre, h, eps):
    """The placement composed from torch ops: x float64 [V,3], f int64 [F,3] (participating faces), cluster int64 [V] (-1 =
    unused), centre float64 [C,3].  Returns the float64 [C,3] vertices."""
    C = centre.shape[0]
    u = cluster >= 0
    cnt = torch.bincount(cluster[u], minlength=C).to(torch.float64)
    m = torch.zeros(C, 3, dtype=torch.float64, device=x.device).index_add_(0, cluster[u], x[u] - centre[cluster[u]])
    m = m / cnt[:, None]
    fc = cluster[f]
    A = torch.zeros(C, 9, dtype=torch.float64, device=x.device)
    b = torch.zeros(C, 3, dtype=torch.float64, device=x.device)
    P = x[f]                                                             # [F,3,3]
    n0 = torch.linalg.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])        # translation-invariant
    for j in range(3):
        w = torch.ones(f.shape[0], dtype=torch.bool, device=x.device)
        for i in range(j):
            w &= fc[:, j] != fc[:, i]
        k = fc[w, j]
        n = n0[w]
        d = (n * (P[w, 0] - centre[k])).sum(-1)
        A.index_add_(0, k, (n[:, :, None] * n[:, None, :]).reshape(-1, 9))
        b.index_add_(0, k, d[:, None] * n)
    A = A.view(C, 3, 3)
    t = A.diagonal(dim1=1, dim2=2).sum(-1)
    lam = eps * t / 3
    M = A + lam[:, None, None] * torch.eye(3, dtype=torch.float64, device=x.device)
    ok = t != 0
    M[~ok] = torch.eye(3, dtype=torch.float64, device=x.device)
    p = torch.linalg.solve(M, (b + lam[:, None] * m)[:, :, None])[:, :, 0]
    ok &= (p.abs() <= h / 2).all(-1)
    return centre + torch.where(ok[:, None], p, m)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=864)
    ap.add_argument("--pitch", type=int, default=86)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0, 8.0])
    ap.add_argument("--color_cell", type=float, default=4.0, help="time the colour pass before / after at this cell (0 = skip)")
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join("profiles", "simplify", "simplify_bench.json"))
    args = ap.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.color_cell:  # built first: a wrong width fails before the long part
        import neuralrecon_w_amd as nw
        from tests._build import build_system

        emb, _, _, rdr = build_system(W=256, n_a=48, n_vocab=100, nerf_w=256, color_hidden=256, head=128, seed=0, prec=nw.PREC_F32,
                                      device=str(dev))
        a = emb.weight[0].detach()
    verts, faces = mesh.isosurface(synthetic_sdf(args.dim, args.pitch, args.seed, dev))
    torch.cuda.empty_cache()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    res = {"what": "mesh simplification (vertex clustering, quadric placement) on a synthetic marching-cubes mesh", "dim": args.dim,
           "pitch": args.pitch, "seed": args.seed, "vertices": V, "faces": F, "repeat": args.repeat, "eps": args.eps,
           "device": torch.cuda.get_device_name(dev), "cells": {}}
    x = verts.double()
    for h in args.cells:
        ms, (v2, f2, _, ci), st = staged(verts, faces, h, args.repeat)
        row = {"stage_ms": ms, "vertices_after": int(v2.shape[0]), "faces_after": int(f2.shape[0]), "clusters": st["clusters"],
               "clusters_at_mean": st["clusters_at_mean"], "members": st["members"], "list_entries": st["list_entries"]}
        gathered = 28.0 * st["members"] + (4.0 + 12.0 + 72.0) * st["list_entries"] + 56.0 * st["clusters"]
        row["place_bytes_gathered"] = gathered
        row["place_bytes_distinct"] = 24.0 * V + 12.0 * F + 4.0 * st["members"] + 4.0 * st["list_entries"] + 56.0 * st["clusters"]
        row["place_GBps_of_gathered_bytes"] = gathered / (ms["place"] * 1e-3) / 1e9
        # the torch composition of the placement, from the same cluster map (every cluster is in the output or not: compare on
        # the output vertices)
        used = ci >= 0
        cl_all = torch.full((V,), -1, dtype=torch.int64, device=dev)
        # cluster numbers of ALL used vertices: recompute the keys as the contract states them
        keep = meshops.face_select(faces, V) != 0
        fp = faces[keep]
        uv = torch.zeros(V, dtype=torch.bool, device=dev)
        uv[fp.reshape(-1)] = True
        lo = x[uv].amin(0)
        idx = torch.floor((x - lo) / h).clamp_(min=0).long()
        nn = torch.floor((x[uv].amax(0) - lo) / h).long() + 1
        idx = torch.minimum(idx, nn - 1)
        key = (idx[:, 0] * nn[1] + idx[:, 1]) * nn[2] + idx[:, 2]
        ck, inv = torch.unique(key[uv], return_inverse=True)
        cl_all[uv] = inv
        first = torch.full((ck.shape[0],), V, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, torch.nonzero(uv).reshape(-1), "amin")
        centre = lo + (idx[first].double() + 0.5) * h
        t_torch, pv = timed(lambda: torch_placement(x, fp, cl_all, centre, h, args.eps), max(1, min(3, args.repeat)))
        pv2 = torch_placement(x, fp, cl_all, centre, h, args.eps)
        out_cluster = torch.full((ck.shape[0],), -1, dtype=torch.int64, device=dev)
        out_cluster[cl_all[used]] = ci[used]
        sel = out_cluster >= 0
        v64 = meshops.simplify(x, faces, h)[0]                              # float64 in, float64 out: no output rounding
        assert v64.shape[0] == v2.shape[0] and torch.equal(v64.to(v2.dtype), v2)
        diff = (pv[sel] - v64[out_cluster[sel]]).abs()
        row["torch_placement_ms"] = t_torch
        row["torch_two_runs_bit_equal"] = bool(torch.equal(pv, pv2))
        row["torch_vs_kernel_max_abs"] = float(diff.max())
        row["torch_vs_kernel_share_over_1e-9"] = float((diff.max(-1).values > 1e-9).double().mean())
        again = meshops.simplify(verts, faces, h)
        row["kernel_two_runs_bit_equal"] = bool(torch.equal(again[0], v2) and torch.equal(again[1], f2))
        res["cells"]["%g" % h] = row
        if args.color_cell and h == args.color_cell:
            res["color_pass_ms"] = {}
            for name, n in (("before", V), ("after", int(v2.shape[0]))):
                pts = (torch.rand(n, 3, device=dev) - 0.5)
                t, _ = timed(lambda: mesh.vertex_colors(rdr, pts, a), 1)
                res["color_pass_ms"][name] = t
                res["color_pass_ms"][name + "_vertices"] = n
        del pv, pv2, again, v2, f2, ci, v64
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
