"""Times marching cubes on the octree bricks (neuralrecon_w_amd.mesh.isosurface_sparse, csrc/ncw_mc_sparse.hip) on a synthetic
shell, at evaluation levels 10, 11 and 12, and at level 10 against the dense-lattice path (mesh.sparse_volume + mesh.isosurface).

    python scripts/bench_mesh_sparse.py [--levels 10 11 12] [--octree_level 8] [--radius 0.5] [--repeat 7]
                                        [--out profiles/meshsparse/meshsparse_bench.json]

Input: the level-`octree_level` voxels whose centre lies within two voxels of a sphere of `radius` (the lattice spans -1 .. 1), as
the occupied bricks; the analytic SDF (distance to the sphere, in fine voxels) at their sub-voxels.  No network.
Per level, with device events, warm, medians over --repeat:
  * every stage of isosurface_sparse: neighbours = ncw_mcs_neighbors, count = ncw_mcs_count, compact = torch.nonzero +
    ncw_mcs_cube_ids + the sort of the cube ids + the scan of their counts (with the one device->host read of the mesh size),
    emit = ncw_mcs_emit, weld = torch.unique + the vertex scatter + the degenerate-face filter; and the whole call;
  * torch.cuda.max_memory_allocated over one call, beside the bytes resident before it (the values and the bricks);
  * the distinct bytes the count pass must move (4 B read + 1 B written per sub-voxel) over its time.
At --dense_level (10), in the same process: the dense path and the brick path alternating, the order swapped every round, whole
calls; both outputs asserted equal (torch.equal on vertices and faces); both peaks, and the brick peak asserted below the dense one.
The count and emit kernels gather their corners directly from global memory; an LDS-tiled variant has not been written, so
there is no second column.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import mesh  # noqa: E402


def shell_bricks(octree_level, radius, dev):
    """[n,3] int64 occupied voxels (ascending): centre within two voxels of the sphere."""
    G = 1 << octree_level
    ax = torch.arange(G, device=dev, dtype=torch.float32) + 0.5 - G / 2.0
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    d = torch.sqrt(X * X + Y * Y + Z * Z) - radius * G / 2.0
    return torch.nonzero(d.abs() <= 2.0), G


def shell_values(bricks, up, G, radius, chunk=2048):
    """[n * up^3] float32: distance to the sphere in fine voxels at every sub-voxel, brick-major, local z fastest."""
    dev = bricks.device
    k = torch.arange(up, device=dev)
    kern = torch.stack(torch.meshgrid(k, k, k, indexing="ij"), -1).reshape(1, -1, 3)
    out = torch.empty(bricks.shape[0] * up ** 3, device=dev, dtype=torch.float32)
    c = (G * up) / 2.0 - 0.25  # off the lattice points: no value lies exactly on the level
    for i in range(0, bricks.shape[0], chunk):
        p = (bricks[i:i + chunk, None, :] * up + kern).float() - c
        out[i * up ** 3:(i + p.shape[0]) * up ** 3] = (p.norm(dim=-1) - radius * G * up / 2.0).reshape(-1)
    return out


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def staged(bricks32, up, G, values, repeat):
    """Median ms per stage and of the whole (the stages of mesh.isosurface_sparse, called one by one), and the result."""
    names = ("neighbours", "count", "compact", "emit", "weld")
    rows = []
    for it in range(repeat + 1):  # the first pass warms up
        ev = events(6)
        ev[0].record()
        nbr = mesh.brick_neighbors(bricks32, G)
        ev[1].record()
        counts = mesh._mcs_count(values, bricks32, nbr, up, G, 0.0)
        ev[2].record()
        sub, offsets, T = mesh._mcs_compact(counts, bricks32, up, G)
        ev[3].record()
        pos, key = mesh._mcs_emit(values, bricks32, nbr, up, G, 0.0, sub, offsets, T)
        ev[4].record()
        out = mesh._weld(pos, key)
        ev[5].record()
        torch.cuda.synchronize()
        if it:
            row = {n: ev[i].elapsed_time(ev[i + 1]) for i, n in enumerate(names)}
            row["total"] = ev[0].elapsed_time(ev[5])
            rows.append(row)
        stats = {"nonempty_cubes": int(sub.shape[0]), "triangles": int(T)}
        del nbr, counts, sub, offsets, pos, key
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}, out, stats


def peak_of(fn):
    """(result, max_memory_allocated during fn, bytes allocated before it)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, int(torch.cuda.max_memory_allocated()), int(before)


def timed_call(fn):
    e0, e1 = events(2)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, nargs="+", default=[10, 11, 12])
    ap.add_argument("--octree_level", type=int, default=8)
    ap.add_argument("--radius", type=float, default=0.5)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--dense_level", type=int, default=10, help="the level at which the dense-lattice path runs beside (0 = skip)")
    ap.add_argument("--out", default=os.path.join("profiles", "meshsparse", "meshsparse_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_sparse.py measures on the GPU; there is none")
    dev = torch.device("cuda", torch.cuda.current_device())
    bricks, G = shell_bricks(args.octree_level, args.radius, dev)
    b32 = bricks.int().contiguous()
    res = {"what": "marching cubes on octree bricks (mesh.isosurface_sparse) on a synthetic sphere shell", "octree_level":
           args.octree_level, "G": G, "radius": args.radius, "bricks": int(bricks.shape[0]), "repeat": args.repeat,
           "device": torch.cuda.get_device_name(dev), "kernel_variant": "direct gathers", "lds_tiled_variant": None, "levels": {}}
    for level in args.levels:
        up = 1 << (level - args.octree_level)
        values = shell_values(bricks, up, G, args.radius)
        K = int(values.shape[0])
        ms, (v, f), stats = staged(b32, up, G, values, args.repeat)
        (v1, f1), peak, before = peak_of(lambda: mesh.isosurface_sparse(bricks, up, values, 0.0, G=G))
        assert torch.equal(v1, v) and torch.equal(f1, f)  # the whole call is its stages; two runs agree bit for bit
        row = {"up": up, "dim": G * up, "sparse_points": K, "stage_ms": ms, "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
               "peak_bytes": peak, "resident_before_bytes": before, "dense_lattice_points": (G * up) ** 3,
               "count_GBps_of_distinct_bytes": 5.0 * K / (ms["count"] * 1e-3) / 1e9}
        row.update(stats)
        del v1, f1
        if level == args.dense_level:
            sd = {"sparse_vol": (bricks.repeat_interleave(up ** 3, dim=0) * up
                                 + torch.stack(torch.meshgrid(*[torch.arange(up, device=dev)] * 3, indexing="ij"), -1)
                                 .reshape(-1, 3).repeat(bricks.shape[0], 1)).float(),
                  "voxel_size": 1.0, "dim": G * up, "vol_origin": np.zeros(3)}

            def dense():
                vol, mask, _ = mesh.sparse_volume(sd, values)
                return mesh.isosurface(vol, 0.0, mask)

            def brick():
                return mesh.isosurface_sparse(bricks, up, values, 0.0, G=G)

            (vd, fd), peak_dense, before_dense = peak_of(dense)
            assert torch.equal(vd, v) and torch.equal(fd, f), "the brick path and the dense path disagree"
            del vd, fd
            t = {"dense": [], "bricks": []}
            for r in range(args.repeat + 1):
                order = (("dense", dense), ("bricks", brick)) if r % 2 == 0 else (("bricks", brick), ("dense", dense))
                for name, fn in order:
                    dt, out = timed_call(fn)
                    del out
                    if r:  # round 0 warms up
                        t[name].append(dt)
            assert peak < peak_dense, (peak, peak_dense)
            row["dense_path"] = {"outputs_equal": True, "peak_bytes": peak_dense, "resident_before_bytes": before_dense,
                                 "call_ms": t["dense"], "median_ms": float(np.median(t["dense"]))}
            row["bricks_call_ms_alternating"] = t["bricks"]
            row["bricks_median_ms_alternating"] = float(np.median(t["bricks"]))
            del sd
        res["levels"][str(level)] = row
        del values, v, f
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
