"""Mesh an oriented point cloud on the GPU (neuralrecon_w_amd.cloudmesh): implicit-moving-least-squares values on a sparse
lattice around the cloud, then sparse marching cubes on the supported lattice points.

    python scripts/mesh_cloud.py --file_in cloud.ply --file_out mesh.ply --voxel V [--support 3 --near 2 --min_count 3] \
        [--box eval_bbx --scene_config_path config.yaml] [--color] [--min_component_faces N]

  * the cloud needs consistently oriented unit normals (nx / ny / nz): `scripts/surface_cloud.py` writes them, and
    `scripts/clean_cloud.py --toward x,y,z` gives them to a cloud seen from one side.  A cloud without normals is refused;
  * --voxel: the lattice spacing, of the order of the point spacing or a little above.  --support (voxels): the radius of the
    weight (1 - d^2 / R^2)^4.  A lattice point takes part when at least --min_count points lie within the support and the
    nearest is within --near voxels; a cube with a corner that does not take part yields no triangle, so holes of the cloud
    wider than about 2 --near voxels stay open;
  * --box NAME: the lattice covers the box of that name in --scene_config_path (in the cloud's coordinates) instead of the
    cloud's own box; points outside it contribute values but no surface is extracted beyond it;
  * --color: every vertex gets the colour of its nearest cloud point (the cloud must have red / green / blue);
  * --min_component_faces N: components with fewer faces are dropped.
The weight, the rules and the defaults are this project's own; no parity with open3d's Poisson or ball pivoting is claimed.
Two sheets closer than --support voxels with opposite normals mix; nothing propagates the orientation of normals.
Prints the points, the candidate and the sparse lattice points, vertices, faces, components and the share of boundary edges;
writes a binary PLY (double coordinates, int faces, uchar colours).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import cloudmesh, meshops, ply  # noqa: E402

NO_NORMALS = "%s has no normals (nx / ny / nz): scripts/clean_cloud.py --toward x,y,z estimates and orients them"


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--file_in", required=True, help="the oriented cloud (PLY with nx / ny / nz)")
    ap.add_argument("--file_out", required=True, help="the mesh (PLY)")
    ap.add_argument("--voxel", type=float, required=True, help="lattice spacing, in the cloud's units")
    ap.add_argument("--support", type=float, default=3.0, help="radius of the weight, in voxels")
    ap.add_argument("--near", type=float, default=2.0, help="a lattice point needs a cloud point within this many voxels (>= sqrt 3)")
    ap.add_argument("--min_count", type=int, default=3, help="and at least this many within the support")
    ap.add_argument("--box", type=str, default=None, metavar="NAME", help="name of a box in --scene_config_path the lattice covers")
    ap.add_argument("--scene_config_path", type=str, default=None, help="scene config with the box")
    ap.add_argument("--color", default=False, action="store_true", help="colour every vertex by its nearest cloud point")
    ap.add_argument("--min_component_faces", type=int, default=0, help="drop components with fewer faces")
    return ap


def edge_stats(faces):
    """(edges, boundary edges: those of exactly one face, edges of more than two faces) of faces [F,3] (a device tensor)."""
    f = faces.long()
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = torch.sort(e, dim=1)[0]
    n = int(f.max()) + 1 if f.numel() else 1
    _, cnt = torch.unique(e[:, 0] * n + e[:, 1], return_counts=True)
    return int(cnt.shape[0]), int((cnt == 1).sum()), int((cnt > 2).sum())


def main(argv=None):
    args = build_parser().parse_args(argv)
    verts, _, rgb = ply.read_mesh(args.file_in)
    normals = ply.read_normals(args.file_in)
    if normals is None:
        raise SystemExit(NO_NORMALS % args.file_in)
    if args.color and rgb is None:
        raise SystemExit("--color: %s has no red / green / blue" % args.file_in)
    box = None
    if args.box is not None:
        if not args.scene_config_path:
            raise SystemExit("--box needs --scene_config_path")
        import yaml

        with open(args.scene_config_path, "r") as fh:
            box = yaml.safe_load(fh)[args.box]
    dev = torch.device("cuda", torch.cuda.current_device())
    pts = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float64)).to(dev)
    nrm = torch.from_numpy(np.ascontiguousarray(normals, dtype=np.float32)).to(dev)
    col = torch.from_numpy(np.ascontiguousarray(rgb)).to(dev) if args.color else None
    st = {}
    out = cloudmesh.mesh_cloud(pts, nrm, args.voxel, support=args.support, near=args.near, min_count=args.min_count, box=box,
                               colors=col, min_component_faces=args.min_component_faces, stats=st)
    v, f = out[0], out[1]
    n_comp = 0
    edges = boundary = 0
    if f.shape[0]:
        _, sizes = meshops.components(f, int(v.shape[0]))
        n_comp = int((sizes > 0).sum())
        edges, boundary, _ = edge_stats(f)
    ply.write(args.file_out, v.cpu().numpy(), faces=f.cpu().numpy(), rgb=out[2].cpu().numpy() if args.color else None)
    print("points: %d" % st["points"])
    print("lattice: %s, candidate lattice points: %d, sparse points: %d" % (" x ".join(str(s) for s in st["side"]), st["candidates"],
                                                                            st["sparse"]))
    print("vertices: %d, faces: %d, components: %d" % (int(v.shape[0]), int(f.shape[0]), n_comp))
    print("boundary edges: %d of %d (%.3f %%)" % (boundary, edges, 100.0 * boundary / max(1, edges)))
    return st, n_comp, boundary, edges


if __name__ == "__main__":
    main()
