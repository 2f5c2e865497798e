"""Times the reprojection visibility filter (neuralrecon_w_amd.reproj) on a seeded synthetic job and prints one JSON line.

The mesh is marching cubes (mesh.isosurface) of an analytic scene-like SDF -- a ground plane, box buildings, a row of columns
and a dome -- on a D^3 lattice over [-1, 1]^3 (about 2.5 million triangles at the default D = 800); the target cloud is the
mesh's own vertices (the pipeline filters the extracted mesh against itself).  N cameras of W x H look at it: most circle
the scene, the last quarter stand inside it between the buildings (they see huge near triangles).  Reported per view
(median over views, HIP events): the small-triangle and large-triangle raster kernels, resolve + back-projection, 1-NN +
marking, and the whole view; plus the whole filter (grid build + every view + the unique rows), the triangles, the
sub-triangles that took the workgroup path and the covered samples per view.

    python scripts/bench_reproj.py [--res 800] [--views 16] [--width 1000] [--height 750]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import mesh, reproj  # noqa: E402


def scene_sdf(D, dev):
    """min over the parts, x-slab by x-slab (the full lattice of coordinates would take 3 D^3 floats)."""
    g = torch.linspace(-1, 1, D, device=dev)
    out = torch.empty(D, D, D, device=dev)
    Y, Z = torch.meshgrid(g, g, indexing="ij")
    rng = np.random.RandomState(0)
    boxes = [(rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), rng.uniform(0.05, 0.15), rng.uniform(0.05, 0.15), rng.uniform(0.1, 0.5))
             for _ in range(10)]
    for i in range(D):
        x = g[i]
        d = Z + 0.6 - 0.3 * (2.0 / (D - 1))  # ground, off the lattice planes
        for bx, by, hx, hy, hz in boxes:
            q = torch.stack([(x - bx).abs().expand_as(Y) - hx, (Y - by).abs() - hy, (Z + 0.6 - hz / 2).abs() - hz / 2])
            d = torch.minimum(d, q.clamp(min=0).norm(dim=0) + q.amax(0).clamp(max=0))
        for k in range(6):  # columns
            cy = -0.5 + 0.2 * k
            d = torch.minimum(d, torch.maximum(torch.sqrt((x - 0.0) ** 2 + (Y - cy) ** 2) - 0.04, (Z + 0.2).abs() - 0.4))
        d = torch.minimum(d, torch.sqrt(x * x + (Y - 0.3) ** 2 + (Z + 0.2) ** 2) - 0.25)  # dome
        out[i] = d
    return out


def look_at(C, T):
    z = np.asarray(T, dtype=np.float64) - C
    z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, 0.0, -1.0]), z)
    x /= np.linalg.norm(x)
    E = np.eye(4)
    E[:3, :3] = np.stack([x, np.cross(z, x), z])
    E[:3, 3] = -E[:3, :3] @ np.asarray(C, dtype=np.float64)
    return E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--height", type=int, default=750)
    ap.add_argument("--voxel_size", type=float, default=0.002)
    ap.add_argument("--small_max", type=int, default=reproj.SMALL_MAX)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    D = args.res
    verts, faces = mesh.isosurface(scene_sdf(D, dev))
    verts = (verts * (2.0 / (D - 1)) - 1.0).double().cpu().numpy()
    faces = faces.cpu().numpy()
    torch.cuda.empty_cache()
    W, H = args.width, args.height
    K = np.array([[0.8 * W, 0, W / 2 + 0.3], [0, 0.8 * W, H / 2 - 0.2], [0, 0, 1]], dtype=np.float32)
    views = []
    n_in = args.views // 4
    for k in range(args.views - n_in):  # around the scene
        a = 2 * math.pi * k / (args.views - n_in)
        views.append(look_at(np.array([1.7 * math.cos(a), 1.7 * math.sin(a), 0.5]), (0.0, 0.0, -0.4)))
    for k in range(n_in):  # inside, between the buildings
        a = 2 * math.pi * (k + 0.5) / max(1, n_in)
        C = np.array([0.35 * math.cos(a), 0.35 * math.sin(a), -0.5])
        views.append(look_at(C, C + np.array([math.cos(a + 1.0), math.sin(a + 1.0), 0.05])))

    def run(timed):
        t0 = time.perf_counter()
        rm = reproj.RasterMesh(verts, faces, dev)
        tgt = reproj.Target(verts, None, 2 * math.sqrt(2) * args.voxel_size, dev)
        zbuf = torch.empty(H * W, dtype=torch.int64, device=dev)
        rec = []
        for E in views:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            s = rm.view_struct(K, E, H, W, small_max=args.small_max)
            rm.rasterize(s, zbuf, timer=lambda st: ev[{"small": 0, "large": 1, "end": 2}[st]].record())
            depth, _ = reproj.resolve(zbuf, H, W, with_face=False)
            pts, _ = reproj.backproject(depth, reproj.backproject_matrix(K, np.linalg.inv(E), tgt.centre))
            ev[3].record()
            tgt.mark(pts)
            ev[4].record()
            rec.append((ev, int(rm.n_large.item()), int(pts.shape[0])))
        xyz, _ = tgt.rows()
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        if not timed:
            return None
        ms = np.array([[e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), e[2].elapsed_time(e[3]), e[3].elapsed_time(e[4]),
                        e[0].elapsed_time(e[4])] for e, _, _ in rec])
        return ms, [r[1] for r in rec], [r[2] for r in rec], total, xyz.shape[0], tgt.m

    run(False)  # warm-up: library load, allocator, kernels
    ms, large, covered, total, kept, m = run(True)
    med = np.median(ms, 0)
    out = {"metric": "reproj_ms_per_view", "value": round(float(med[4]), 4), "unit": "ms", "higher_is_better": False,
           "views": len(views), "width": W, "height": H, "triangles": int(faces.shape[0]), "vertices": int(m),
           "raster_small_ms": round(float(med[0]), 4), "raster_large_ms": round(float(med[1]), 4),
           "backproject_ms": round(float(med[2]), 4), "nn_mark_ms": round(float(med[3]), 4),
           "view_ms_max": round(float(ms[:, 4].max()), 4), "filter_total_ms": round(total, 2),
           "large_tris_per_view_median": int(np.median(large)), "large_tris_per_view_max": int(max(large)),
           "covered_samples_per_view_median": int(np.median(covered)), "kept_vertices": int(kept),
           "small_max": args.small_max}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
