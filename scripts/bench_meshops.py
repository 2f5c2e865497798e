"""Times the mesh operations (neuralrecon_w_amd.meshops, csrc/ncw_meshops.hip) on a synthetic mesh of about 20 M faces.

    python scripts/bench_meshops.py [--dim 864] [--repeat 5] [--out profiles/meshops/meshops_bench.json] [--color_pass]

Input: marching cubes (mesh.isosurface) of an analytic SDF on a [dim]^3 lattice -- one sphere per cell of a coarse lattice
(half of them large, half of them floaters of a few voxels) and a slab across the whole volume -- so: one very large
component, hundreds of large ones and hundreds of tiny ones, with the vertex numbering marching cubes gives.
Timed with device events, warm, medians over --repeat, all in one call:
  * labelling, split into hook / flatten / sizes (the three launches of meshops.components);
  * face selection + compaction (meshops.face_select + meshops.submesh, dropping the components under --min_faces);
  * baseline 1: scipy.sparse.csgraph.connected_components on the host, with the copies of the faces to the host and of the
    labels back (wall clock);
  * baseline 2: the same partition composed from torch ops on the device -- min-label propagation over the edges with
    scatter_reduce(amin) and one pointer jump per sweep, iterated to a fixed point.
Both baselines must give the labels of the kernels exactly (checked).  --color_pass also times mesh.vertex_colors (the colour
pass of extract_mesh --vertex_color, flagship widths, random weights) on the vertex counts before and after the clean-up.
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import lib as L  # noqa: E402
from neuralrecon_w_amd import mesh, meshops  # noqa: E402


def synthetic_sdf(dim, pitch, seed, dev):
    """[dim]^3 float32: min(slab, spheres); every sphere lies inside its own cell of side `pitch` voxels."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = (dim + pitch - 1) // pitch
    big = torch.rand(n, n, n, generator=g) < 0.5
    radius = torch.where(big, 0.25 * pitch + 0.2 * pitch * torch.rand(n, n, n, generator=g), 2.0 + 4.0 * torch.rand(n, n, n, generator=g))
    centre = 0.5 * pitch + (torch.rand(n, n, n, 3, generator=g) - 0.5) * 0.05 * pitch
    radius, centre = radius.to(dev), centre.to(dev)
    sdf = torch.empty(dim, dim, dim, device=dev)
    ax = torch.arange(dim, device=dev, dtype=torch.float32)
    cell = (ax / pitch).long()
    loc = ax - cell * pitch
    slab_z = 0.5 * dim + 0.37 * pitch
    for x0 in range(0, dim, 32):
        xs = slice(x0, min(dim, x0 + 32))
        c = centre[cell[xs]][:, cell][:, :, cell]                     # [x, y, z, 3]
        r = radius[cell[xs]][:, cell][:, :, cell]
        d2 = (loc[xs, None, None] - c[..., 0]) ** 2 + (loc[None, :, None] - c[..., 1]) ** 2 + (loc[None, None, :] - c[..., 2]) ** 2
        slab = (ax - slab_z).abs() - 1.5                                # three voxels thick, across every cell
        sdf[xs] = torch.minimum(d2.sqrt() - r, slab[None, None, :])
    return sdf


def timed(fn, repeat):
    """Median device time in ms of fn() over `repeat` runs after one warm-up, and its last result."""
    out = fn()
    ts = []
    for _ in range(repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), out


def torch_labels(f, V, max_sweeps=100000):
    """Min-label propagation composed from torch ops: labels = arange; every sweep takes, per vertex, the minimum label over
    its edges (scatter_reduce amin, both directions) and jumps once (labels = labels[labels]); until nothing changes."""
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    src = torch.cat([e[:, 0], e[:, 1]])
    dst = torch.cat([e[:, 1], e[:, 0]])
    labels = torch.arange(V, device=f.device, dtype=torch.int64)
    for sweep in range(1, max_sweeps + 1):
        new = labels.scatter_reduce(0, dst, labels[src], "amin", include_self=True)
        new = new[new]
        if torch.equal(new, labels):
            return labels, sweep
        labels = new
    raise RuntimeError("no fixed point after %d sweeps" % max_sweeps)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=864)
    ap.add_argument("--pitch", type=int, default=86, help="cell of one sphere, voxels")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--min_faces", type=int, default=2000, help="components under this are the floaters to drop")
    ap.add_argument("--color_pass", action="store_true")
    ap.add_argument("--no_scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "meshops", "meshops_bench.json"))
    args = ap.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.color_pass:  # built first: a wrong width fails before the long part
        import neuralrecon_w_amd as nw
        from tests._build import build_system

        # SDF 8 x 256, colour 4 x 256 (BASELINE configs[1]); extract_mesh.py's default colour precision (fp32)
        emb, _, _, rdr = build_system(W=256, n_a=48, n_vocab=100, nerf_w=256, color_hidden=256, head=128, seed=0, prec=nw.PREC_F32,
                                      device=str(dev))
        a = emb.weight[0].detach()
    verts, faces = mesh.isosurface(synthetic_sdf(args.dim, args.pitch, args.seed, dev))
    torch.cuda.empty_cache()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    f32 = faces.to(torch.int32).contiguous()
    lib, st = L.get_lib(), L.stream_ptr(dev)
    res = {"what": "mesh operations on a synthetic marching-cubes mesh", "dim": args.dim, "pitch": args.pitch, "seed": args.seed,
           "vertices": V, "faces": F, "repeat": args.repeat, "device": torch.cuda.get_device_name(dev)}

    # labelling, launch by launch
    parent = torch.empty(V, dtype=torch.int32, device=dev)
    sizes = torch.empty(V, dtype=torch.int32, device=dev)
    ar = torch.arange(V, dtype=torch.int32, device=dev)

    def hook():
        parent.copy_(ar)
        L.check(lib.ncw_mesh_cc_hook(L.ptr(f32), None, F, V, L.ptr(parent), st), "hook")

    t_init, _ = timed(lambda: parent.copy_(ar), args.repeat)
    t_hook, _ = timed(hook, args.repeat)
    t_flat, _ = timed(lambda: L.check(lib.ncw_mesh_cc_flatten(L.ptr(parent), V, st), "flatten"), args.repeat)  # re-runs are on flat trees

    def flatten_cold():
        hook()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(lib.ncw_mesh_cc_flatten(L.ptr(parent), V, st), "flatten")
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    t_flat_cold = float(np.median([flatten_cold() for _ in range(args.repeat)]))

    def count():
        sizes.zero_()
        L.check(lib.ncw_mesh_cc_sizes(L.ptr(f32), None, F, V, L.ptr(parent), L.ptr(sizes), st), "sizes")

    t_sizes, _ = timed(count, args.repeat)
    t_all, (labels, sz) = timed(lambda: meshops.components(f32, V), args.repeat)
    assert torch.equal(labels, parent) and torch.equal(sz, sizes)
    ncomp = int((sz > 0).sum())
    res["labelling_ms"] = {"hook": t_hook - t_init, "flatten": t_flat_cold, "flatten_already_flat": t_flat, "sizes": t_sizes,
                           "components_call": t_all, "init_copy": t_init}
    res["components"] = ncomp
    res["largest_component_faces"] = int(sz.max())
    # bytes the labelling must move per face, by counting (no counters): hook reads 12 B of corners per face; flatten reads and
    # writes 4 B per vertex; sizes reads 12 B per face and one label.  The walks' dependent 4-B reads and the atomics come on top.
    res["min_bytes_per_face"] = {"hook": 12.0, "flatten": 8.0 * V / F, "sizes": 16.0}
    res["labelling_GBps_of_min_bytes"] = (12.0 + 8.0 * V / F + 16.0) * F / ((t_hook - t_init + t_flat_cold + t_sizes) * 1e-3) / 1e9

    # selection + compaction
    def select_compact():
        ok = meshops.select_components(sz, min_faces=args.min_faces)
        keep = meshops.face_select(f32, V, labels=labels, comp_ok=ok)
        return meshops.submesh(verts, f32, keep)

    t_sel, _ = timed(lambda: meshops.face_select(f32, V, labels=labels, comp_ok=meshops.select_components(sz, min_faces=args.min_faces)),
                     args.repeat)
    t_sc, (v2, f2, _, _) = timed(select_compact, args.repeat)
    res["select_ms"] = t_sel
    res["select_compact_ms"] = t_sc
    res["after"] = {"vertices": int(v2.shape[0]), "faces": int(f2.shape[0]),
                    "components": int(((sz > 0) & (sz >= args.min_faces)).sum())}

    # baseline 2: torch ops
    t_torch, (tl, sweeps) = timed(lambda: torch_labels(faces, V), max(1, min(3, args.repeat)))
    assert torch.equal(tl.to(torch.int32), labels), "the torch composition disagrees with the kernels"
    res["torch_scatter_reduce_ms"] = t_torch
    res["torch_sweeps"] = sweeps
    del tl
    torch.cuda.empty_cache()

    # baseline 1: scipy on the host, copies included
    if not args.no_scipy:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fh = faces.cpu().numpy()
        t1 = time.perf_counter()
        rows = np.concatenate([fh[:, 0], fh[:, 0]])
        cols = np.concatenate([fh[:, 1], fh[:, 2]])
        g = coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(V, V))
        n, comp = connected_components(g, directed=False)
        first = np.full(n, V, dtype=np.int64)
        np.minimum.at(first, comp, np.arange(V))
        t2 = time.perf_counter()
        back = torch.from_numpy(first[comp].astype(np.int32)).to(dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        assert n == int((labels == ar).sum()) and torch.equal(back, labels), "scipy disagrees with the kernels"
        res["scipy_ms"] = {"total": (t3 - t0) * 1e3, "faces_to_host": (t1 - t0) * 1e3, "graph_and_components": (t2 - t1) * 1e3,
                           "labels_to_device": (t3 - t2) * 1e3}

    if args.color_pass:
        res["color_pass_ms"] = {}
        for name, n in (("before", V), ("after", int(v2.shape[0]))):
            pts = (torch.rand(n, 3, device=dev) - 0.5)
            t, _ = timed(lambda: mesh.vertex_colors(rdr, pts, a), 1)
            res["color_pass_ms"][name] = t
            res["color_pass_ms"][name + "_vertices"] = n

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
