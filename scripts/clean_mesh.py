"""Component clean-up of an existing PLY mesh on the GPU (neuralrecon_w_amd.meshops; not in the reference): drop the detached
pieces ("floaters") of a triangle mesh by the size of their connected component.

    python scripts/clean_mesh.py --file_in results/.../mesh/extracted_mesh_level_10_colored.ply --file_out cleaned.ply \
        [--min_component_faces N] [--largest_components K] [--simplify_cell H]

  * components go by SHARED VERTEX INDEX (the vertices as the file stores them: no welding), a component's size is its number
    of faces; --largest_components keeps the K with the most faces, ties to the one with the smaller first vertex;
  * kept vertices and faces keep their order; coordinates are written in the precision they were read as (double), colours
    when the file has them;
  * prints the components before and after, and the faces kept;
  * --simplify_cell H (off by default; without it the written file is what it always was): after the clean-up, vertex clustering
    on a grid of cell size H, in the file's own units, with a quadric-optimal vertex per cell (meshops.simplify); colours are
    averaged per cell; prints the vertices and faces before and after.  Clustering joins pieces that come within one cell of
    each other, which is why the clean-up goes first.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import meshops, ply  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="drop small connected components of a PLY mesh (GPU)")
    ap.add_argument("--file_in", required=True, help="PLY with faces")
    ap.add_argument("--file_out", required=True, help="PLY to write")
    ap.add_argument("--min_component_faces", type=int, default=0, help="drop components of fewer faces")
    ap.add_argument("--largest_components", type=int, default=None, help="keep the K components with the most faces")
    ap.add_argument("--simplify_cell", type=float, default=None, help="simplify by vertex clustering, cell size in the file's units")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    verts, faces, rgb = ply.read_mesh(args.file_in)
    if faces.shape[0] == 0:
        raise SystemExit("%s has no faces: nothing to label" % args.file_in)
    dev = torch.device("cuda", torch.cuda.current_device())
    stats = {}
    v, f, c, _ = meshops.clean(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev),
                               None if rgb is None else torch.from_numpy(rgb).to(dev), args.min_component_faces,
                               args.largest_components, stats=stats)
    kept_vertices, simp = v.shape[0], {}
    if args.simplify_cell is not None and f.shape[0] > 0:
        v, f, c, _ = meshops.simplify(v, f, args.simplify_cell, c, stats=simp)
    ply.write(args.file_out, v.cpu().numpy(), f.cpu().numpy(), rgb=None if c is None else c.cpu().numpy())
    print("components: %d -> %d" % (stats["components_before"], stats["components_after"]))
    print("faces kept: %d of %d (%d of %d vertices) -> %s" % (stats["faces_after"], stats["faces_before"], kept_vertices,
                                                              verts.shape[0], args.file_out))
    if simp:
        print("simplified (cell %g): %d -> %d vertices, %d -> %d faces, %d of %d cells placed at their mean"
              % (args.simplify_cell, simp["vertices_before"], simp["vertices_after"], simp["faces_before"], simp["faces_after"],
                 simp["clusters_at_mean"], simp["clusters"]))


if __name__ == "__main__":
    main()
