"""Times the reprojection visibility filter (neuralrecon_w_amd.reproj) on a seeded synthetic job and prints one JSON line.

The mesh is marching cubes (mesh.isosurface) of an analytic scene-like SDF -- a ground plane, box buildings, a row of columns
and a dome -- on a D^3 lattice over [-1, 1]^3 (about 2.5 million triangles at the default D = 800); the target cloud is the
mesh's own vertices (the pipeline filters the extracted mesh against itself).  N cameras of W x H look at it: most circle
the scene, the last quarter stand inside it between the buildings (they see huge near triangles).  Reported per view
(median over views, HIP events): the small-triangle and large-triangle raster kernels, resolve + back-projection, 1-NN +
marking, and the whole view; plus the whole filter (grid build + every view + the unique rows), the triangles, the
sub-triangles that took the workgroup path and the covered samples per view.

`cloud_source` in the same line is the point-cloud source of the filter (reproj.VoxelCloud) over the same views: the mesh's
vertices voxelised over [-1, 1]^3 at --voxel_size, ms per view of the fused first-hit launch (ncw_voxel_view_seen) against
the same `seen` voxels composed from torch ray generation + ncw_ray_voxel_trace (count pass, prefix sum, write pass) + the
first crossing per ray + a scatter, the ms of `select` over the vertices, and the bytes each path allocates per view
(median over views and repetitions, warm).  Both grids are cleared before every timed view, outside the timed region: a
view of a filter run marks into a grid that does not hold its bits yet, so the fused launch issues its atomics; the
`*_bits_already_set` figures are the same launches into grids that hold every view's bits (no atomic is issued).

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
from neuralrecon_w_amd import lib as L  # noqa: E402
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


def composed_view(cloud, K, pose, H, W, flags):
    """The first-hit voxels of one view WITHOUT the fused kernel: rays in torch (kaolin_renderer.gen_rays' arithmetic in f32),
    every crossing from ncw_ray_voxel_trace (two passes around a prefix sum), the first per ray, a scatter into flags
    (uint8 per voxel)."""
    dev, lib, st = cloud.dev, L.get_lib(), L.stream_ptr(cloud.dev)
    s = cloud.view_struct(K, pose, H, W)
    j, i = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                          indexing="ij")
    cam = torch.stack([(i - s.cx) / s.fx, (j - s.cy) / s.fy, torch.ones_like(i)], -1).reshape(-1, 3)
    d = cam @ torch.tensor(list(s.pose), device=dev).view(3, 3).T
    d = (d / d.norm(dim=-1, keepdim=True) + 1e-7).contiguous()
    o = torch.tensor(list(s.o_norm), device=dev).expand(d.shape[0], 3).contiguous()
    R = int(d.shape[0])
    counts = torch.empty(R, dtype=torch.int32, device=dev)
    L.check(lib.ncw_ray_voxel_trace(L.ptr(o), L.ptr(d), R, cloud.level, L.ptr(cloud.occ), L.ptr(cloud.brick), None, L.ptr(counts),
                                    None, None, None, st), "ncw_ray_voxel_trace")
    ends = torch.cumsum(counts, 0, dtype=torch.int32)
    offsets = (ends - counts).contiguous()
    n = int(ends[-1])  # the host has to size the nugget arrays
    nug_ray = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    nug_voxel = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    nug_depth = torch.empty(max(n, 1), 2, dtype=torch.float32, device=dev)
    L.check(lib.ncw_ray_voxel_trace(L.ptr(o), L.ptr(d), R, cloud.level, L.ptr(cloud.occ), L.ptr(cloud.brick), L.ptr(offsets), None,
                                    L.ptr(nug_ray), L.ptr(nug_voxel), L.ptr(nug_depth), st), "ncw_ray_voxel_trace")
    first = offsets[counts > 0].long()
    ok = nug_depth[first, 0] > 1e-4
    flags[nug_voxel[first][ok].long()] = 1
    return n


def set_bits(words):
    """Linear indices of the set bits of a bit grid (int32 words), decoded from the non-zero words only."""
    w = words.nonzero().reshape(-1)
    bits = ((words[w].view(-1, 1) >> torch.arange(32, device=words.device, dtype=torch.int32).view(1, 32)) & 1).nonzero()
    return w[bits[:, 0]] * 32 + bits[:, 1]


def cloud_source(verts, views, K, W, H, voxel_size, dev, reps=3):
    """The `cloud_source` object of the JSON line."""
    cloud = reproj.VoxelCloud(verts, {"eval_bbx": [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]}, voxel_size, dev)
    poses = [np.linalg.inv(E) for E in views]
    flags = torch.zeros(cloud.G ** 3, dtype=torch.uint8, device=dev)

    def timed(fn, reset, fresh):
        """ms and bytes allocated (peak above the start) of fn(pose) per view: reps + 1 sweeps over the views, the first one
        dropped.  reset clears the grid fn marks into.  fresh: it is called before every view, outside the timed region, so
        every view marks into a grid that does not hold its bits yet, as each view of a filter run does (the fused launch
        then issues its atomics); otherwise the grid keeps the bits of the earlier sweeps (no atomic is issued: the plain
        load finds every bit set) and holds every view's bits at the end."""
        ms, mem, extra = [], [], []
        reset()
        for rep in range(reps + 1):
            for pose in poses:
                if fresh:
                    reset()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                base = torch.cuda.memory_allocated(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                x = fn(pose)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    ms.append(e0.elapsed_time(e1))
                    mem.append(torch.cuda.max_memory_allocated(dev) - base)
                    extra.append(x)
        return float(np.median(ms)), float(np.max(ms)), int(np.median(mem)), extra

    fused = lambda pose: cloud.trace(K, pose, H, W)  # noqa: E731
    composed = lambda pose: composed_view(cloud, K, pose, H, W, flags)  # noqa: E731
    fused_ms, fused_max, fused_bytes, _ = timed(fused, cloud.clear, True)
    comp_ms, comp_max, comp_bytes, nuggets = timed(composed, flags.zero_, True)
    fused_set_ms, _, _, _ = timed(fused, cloud.clear, False)  # leaves every view's bits in `seen`
    comp_set_ms, _, _, _ = timed(composed, flags.zero_, False)  # ... and in `flags`
    seen = cloud.seen
    lin_fused = set_bits(seen)
    lin_comp = flags.nonzero().reshape(-1)
    both = int(torch.isin(lin_fused, lin_comp).sum())
    # select: the whole call (float64 normalisation on the host, the copy, the kernel) and the kernel alone
    t = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = cloud.select(verts)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    pn = cloud.normalise(verts)
    out = torch.empty(pn.shape[0], dtype=torch.uint8, device=dev)
    tk = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(L.get_lib().ncw_voxel_points_seen(L.ptr(pn), int(pn.shape[0]), cloud.level, L.ptr(seen), L.ptr(out),
                                                  L.stream_ptr(dev)), "ncw_voxel_points_seen")
        e1.record()
        torch.cuda.synchronize()
        tk.append(e0.elapsed_time(e1))
    return {"level": cloud.level, "voxel_size": voxel_size, "points": int(pn.shape[0]),
            "occupied_voxels": int(set_bits(cloud.occ).shape[0]),
            "views": len(poses), "width": W, "height": H, "repetitions": reps,
            "fused_ms_per_view": round(fused_ms, 4), "composed_ms_per_view": round(comp_ms, 4),
            "fused_ms_per_view_max": round(fused_max, 4), "composed_ms_per_view_max": round(comp_max, 4),
            "fused_ms_per_view_bits_already_set": round(fused_set_ms, 4),
            "composed_ms_per_view_bits_already_set": round(comp_set_ms, 4),
            "fused_bytes_per_view": fused_bytes, "composed_bytes_per_view": comp_bytes,
            "crossings_per_view_median": int(np.median(nuggets)),
            "seen_voxels_fused": int(lin_fused.shape[0]), "seen_voxels_composed": int(lin_comp.shape[0]), "seen_voxels_common": both,
            "select_ms": round(float(np.median(t[1:])), 4), "select_kernel_ms": round(float(np.median(tk[1:])), 4),
            "kept_points": int(keep.sum())}


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
    del ms, large, covered
    torch.cuda.empty_cache()
    out["cloud_source"] = cloud_source(verts, views, K, W, H, args.voxel_size, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
