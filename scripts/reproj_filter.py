"""Reprojection visibility filter: the reference's `utils/reproj_filter.py` command line without pyrender,
open3d, trimesh or ray -- keeps the vertices of --target_file that some training view of --data_path sees on the mesh of
--src_file, on one GPU (neuralrecon_w_amd.reproj).

    python scripts/reproj_filter.py --src_file results/.../mesh/extracted_mesh_level_10_colored.ply \
        --target_file results/.../mesh/extracted_mesh_level_10_colored.ply \
        --data_path data/heritage-recon/brandenburg_gate --output_path results/.../mesh

  * a --src_file without faces is a point cloud: it is voxelised over the scene's eval_bbx at --voxel_size and every view is
    traced to the first occupied voxel; a target vertex is kept iff its voxel was some pixel's first hit;
  * writes <output_path>/reprojected.ply (double x / y / z, uchar colours), in GT coordinates;
  * --keep_faces (not in the reference) also writes <output_path>/reprojected_mesh.ply: the target's faces with at least
    --min_corners marked corners (default 1), optionally without the connected components of fewer
    than --min_component_faces faces, vertices in file order; reprojected.ply is unchanged by it;
  * --visualize writes render/depth/<name>.npy and render/reprojects/<name>.ply (the reference writes JPEGs);
  * --n_cpus / --n_gpus are accepted for compatibility and ignored: one process renders every view on one GPU.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import reproj  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="reprojection visibility filter (GPU)")
    ap.add_argument("--src_file", type=str, required=True, help="mesh file path, or a point cloud (no faces)")
    ap.add_argument("--target_file", type=str, default=None, help="point cloud to be filtered (default: --src_file)")
    ap.add_argument("--data_path", type=str, required=True, help="camera poses in colmap format")
    ap.add_argument("--output_path", type=str, required=True, help="output path")
    ap.add_argument("--gt", default=False, action="store_true", help="whether target pc/mesh is in gt coordinates system")
    ap.add_argument("--visualize", default=False, action="store_true",
                    help="store render results: render/depth/<name>.npy and render/reprojects/<name>.ply")
    ap.add_argument("--voxel_size", type=float, default=0.01, help="voxel size in world coordinate system")
    ap.add_argument("--znear", type=float, default=reproj.ZNEAR, help="near plane (pyrender's default)")
    ap.add_argument("--zfar", type=float, default=reproj.ZFAR, help="far plane (pyrender's default)")
    ap.add_argument("--cull", choices=sorted(reproj.CULL), default="back", help="face culling (pyrender: back)")
    ap.add_argument("--keep_faces", default=False, action="store_true",
                    help="also write reprojected_mesh.ply: the target's faces with marked corners (the target needs faces)")
    ap.add_argument("--min_corners", type=int, choices=[1, 2, 3], default=1,
                    help="--keep_faces: marked corners a face needs (1: one-ring rule, 3: nothing the reference would drop)")
    ap.add_argument("--min_component_faces", type=int, default=0,
                    help="--keep_faces: drop connected components (by shared vertex) of fewer kept faces")
    ap.add_argument("--n_cpus", type=int, default=1, help="ignored (accepted for compatibility): one process")
    ap.add_argument("--n_gpus", type=int, default=4, help="ignored (accepted for compatibility): one GPU")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    reproj.reproj_filter(args.src_file, args.target_file or args.src_file, args.data_path, args.output_path, gt=args.gt,
                         voxel_size=args.voxel_size, visualize=args.visualize, znear=args.znear, zfar=args.zfar,
                         cull=args.cull, keep_faces=args.keep_faces, min_corners=args.min_corners,
                         min_component_faces=args.min_component_faces)


if __name__ == "__main__":
    main()
