"""Times the stages of cloudmesh.mesh_cloud on a synthetic oriented cloud: grid build, candidate blocks, the IMLS values launch
(csrc/ncw_imls.hip), selection + sort, sparse marching cubes.

    python scripts/bench_cloudmesh.py [--points 2000000] [--repeat 7] [--knn_points 2000000] [--out profiles/cloudmesh/cloudmesh_bench.json]

The cloud is bench_knn.py's curved sheet (a 30 x 20 floor with a bump, uniform by area) with its analytic normals; the voxel is
the mean point spacing sqrt(area / points), support 3 voxels, near 2, min_count 3 (the defaults).  One call, warm, device
events, the variants alternating inside every repeat, medians and min / max over --repeat.  Beside the values launch, the only
other all-within-R gather in the tree -- NNGrid.query_k(k = 32, max_dist = R), which keeps the 32 nearest, not all -- over the
first --knn_points candidate lattice points, and the values launch over the same points.  `staged` / `admitted`: points staged
through LDS and points that passed d2 <= r2, per lattice point.  Prints one JSON line and writes it to --out."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import cloudmesh, evalmesh, mesh  # noqa: E402
from neuralrecon_w_amd import lib as L  # noqa: E402


def sheet(n, gen):
    """bench_knn.py's sheet and its unit normals (-dz/dx, -dz/dy, 1) / |.|."""
    u, v = torch.rand(n, generator=gen, dtype=torch.float64), torch.rand(n, generator=gen, dtype=torch.float64)
    x, y = 30 * u, 20 * v
    z = 4.0 * torch.exp(-((x - 18) ** 2 + (y - 11) ** 2) / (2 * 3.0 ** 2))
    nrm = torch.stack([z * (x - 18) / 9.0, z * (y - 11) / 9.0, torch.ones_like(z)], -1)
    return torch.stack([x, y, z], -1), nrm / nrm.norm(dim=-1, keepdim=True)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stat(ts):
    return {"ms": float(np.median(ts)), "min_max_ms": [float(min(ts)), float(max(ts))]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--knn_points", type=int, default=2_000_000, help="lattice points of the query_k comparison")
    ap.add_argument("--out", default=os.path.join("profiles", "cloudmesh", "cloudmesh_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise L.NeuconwHipError("bench_cloudmesh needs a GPU: nothing here is measured on the CPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    pts, nrm = sheet(args.points, torch.Generator().manual_seed(args.seed))
    pts, nrm = pts.to(dev), nrm.to(dev).float()
    support, near, min_count = 3.0, 2.0, 3
    voxel = math.sqrt(30.0 * 20.0 / args.points)  # the floor's area: the bump adds 1 % to it
    lo, hi = pts.amin(0).tolist(), pts.amax(0).tolist()
    centre = [(a + b) / 2 for a, b in zip(lo, hi)]
    lat_lo, side = cloudmesh.lattice_for([a - c for a, c in zip(lo, centre)], [b - c for b, c in zip(hi, centre)], voxel, support)
    lat_lo = [float(np.float32(v)) for v in lat_lo]
    p32 = (pts - torch.tensor(centre, dtype=torch.float64, device=dev)).float().contiguous()
    cmax = max(float(p32.abs().amax()), max(abs(v) for v in lat_lo), max(abs(l + s * voxel) for l, s in zip(lat_lo, side)))
    radius, G = support * voxel, max(side)
    near2 = float(np.float32(near * voxel) * np.float32(near * voxel))

    grid = evalmesh.NNGrid(p32, cmax)
    ns = cloudmesh.gather_normals(grid, nrm)
    blocks = cloudmesh.candidate_blocks(p32, lat_lo, voxel, side, near)
    nb = int(blocks.shape[0])

    def values(bl=blocks):
        return cloudmesh.imls_values(grid, None, bl, lat_lo, voxel, side, radius, sorted_normals=ns)

    def select(planes):
        value, count, d2min = planes
        sel = torch.nonzero((count >= min_count) & torch.isfinite(value) & (d2min <= near2)).reshape(-1)
        li = cloudmesh._block_points(blocks)[sel]
        keys, order = torch.sort((li[:, 0] * G + li[:, 1]) * G + li[:, 2])
        bricks = torch.stack((keys // (G * G), (keys // G) % G, keys % G), -1).to(torch.int32).contiguous()
        return bricks, value[sel][order].contiguous()

    kq = min(int(args.knn_points) // 64, nb)
    kblocks = blocks[:kq].contiguous()
    kpts = (torch.tensor(lat_lo, dtype=torch.float32, device=dev) + cloudmesh._block_points(kblocks).float() * np.float32(voxel)).contiguous()
    stages = {
        "grid_build": lambda: evalmesh.NNGrid(p32, cmax),
        "candidates": lambda: cloudmesh.candidate_blocks(p32, lat_lo, voxel, side, near),
        "values": values,
        "values_subset": lambda: values(kblocks),
        "query_k32_subset": lambda: grid.query_k(kpts, 32, max_dist=radius),
    }
    planes = values()
    bricks, vals = select(planes)
    stages["select_sort"] = lambda: select(planes)
    stages["marching_cubes"] = lambda: mesh.isosurface_sparse(bricks, 1, vals, 0.0, G=G)
    for fn in stages.values():
        fn()  # warm: the coarse level of query_k is built here
    torch.cuda.synchronize()
    times = {k: [] for k in stages}
    for _ in range(args.repeat):
        for k, fn in stages.items():  # alternating: every stage once per repeat
            times[k].append(timed(fn)[0])
    st = {}
    _, count, _ = cloudmesh.imls_values(grid, None, blocks, lat_lo, voxel, side, radius, stats=st, sorted_normals=ns)
    verts, faces = mesh.isosurface_sparse(bricks, 1, vals, 0.0, G=G)
    n_lat = nb * 64
    res = {"what": "stages of cloudmesh.mesh_cloud on bench_knn.py's sheet; NNGrid.query_k(32, max_dist = R) on a subset beside it",
           "device": torch.cuda.get_device_name(dev), "repeat": args.repeat, "points": args.points, "voxel": voxel, "support": support,
           "near": near, "min_count": min_count, "side": side, "grid_dims": list(grid.dims), "grid_h_over_voxel": grid.h / voxel,
           "blocks": nb, "lattice_points": n_lat, "sparse_points": int(bricks.shape[0]), "vertices": int(verts.shape[0]),
           "faces": int(faces.shape[0]), "staged_per_lattice_point": st["staged"] / float(max(1, nb)),
           "admitted_per_lattice_point": float(count.double().mean()), "subset_lattice_points": kq * 64,
           "stages": {k: stat(v) for k, v in times.items()}}
    res["values_lattice_points_per_s"] = n_lat / (res["stages"]["values"]["ms"] * 1e-3)
    res["values_point_tests_per_s"] = st["staged"] * 64.0 / (res["stages"]["values"]["ms"] * 1e-3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
