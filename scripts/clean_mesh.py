"""Component clean-up of an existing PLY mesh on the GPU (neuralrecon_w_amd.meshops; not in the reference): drop the detached
pieces ("floaters") of a triangle mesh by the size of their connected component.

    python scripts/clean_mesh.py --file_in results/.../mesh/extracted_mesh_level_10_colored.ply --file_out cleaned.ply \
        [--min_component_faces N] [--largest_components K]

  * components go by SHARED VERTEX INDEX (the vertices as the file stores them: no welding), a component's size is its number
    of faces; --largest_components keeps the K with the most faces, ties to the one with the smaller first vertex;
  * kept vertices and faces keep their order; coordinates are written in the precision they were read as (double), colours
    when the file has them;
  * prints the components before and after, and the faces kept.
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
    ply.write(args.file_out, v.cpu().numpy(), f.cpu().numpy(), rgb=None if c is None else c.cpu().numpy())
    print("components: %d -> %d" % (stats["components_before"], stats["components_after"]))
    print("faces kept: %d of %d (%d of %d vertices) -> %s" % (stats["faces_after"], stats["faces_before"], v.shape[0],
                                                              verts.shape[0], args.file_out))


if __name__ == "__main__":
    main()
