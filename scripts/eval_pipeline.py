"""Evaluation pipeline of one Heritage-Recon scene: the reference's `scripts/eval_pipeline.sh` in one
process -- the reprojection filter of the extracted mesh (scripts/reproj_filter.py), then the F-score of what it keeps
(scripts/eval_mesh.py) with the scene's thresholds and SfM crop.

    python scripts/eval_pipeline.py --scene_name brandenburg_gate --pred_dir results/phototourism/<run> \
        [--data_root data/heritage-recon]

Reads <pred_dir>/mesh/extracted_mesh_level_10_colored.ply, <data_root>/<scene>/{dense/sparse, *.tsv, config.yaml,
<scene>.ply, neuralsfm/points3D.bin}; writes <pred_dir>/mesh/reprojected.ply and
<pred_dir>/mesh/eval_<scene>_reprojected.ply/.  As in the reference, eval_mesh applies sfm2gt to the filtered cloud that is
already in GT coordinates: the two steps chain correctly only when sfm2gt is the identity.

--sample_surface / --surface_seed / --surface_mode / --error_clouds / --normal_consistency are handed to eval_mesh as scripts/eval_mesh.py does.
The file the pipeline scores, reprojected.ply, is a point cloud: --sample_surface needs faces and is refused on it, and so
is --exact_recall (exact point-to-triangle recall, scripts/eval_mesh.py), before any work: the reprojection filter does not
keep the faces.

--keep_faces (not in the reference) [--min_corners 1|2|3] [--min_component_faces N] makes the filter keep them: it also writes
<pred_dir>/mesh/reprojected_mesh.ply (scripts/reproj_filter.py --keep_faces), the pipeline scores THAT file, with results in
<pred_dir>/mesh/eval_<scene>_reprojected_mesh.ply/, and --sample_surface and --exact_recall work on it.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import reproj  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="reprojection filter + mesh evaluation of a Heritage-Recon scene")
    ap.add_argument("--scene_name", required=True, choices=sorted(reproj.SCENES))
    ap.add_argument("--pred_dir", required=True, help="run directory holding mesh/extracted_mesh_level_10_colored.ply")
    ap.add_argument("--data_root", default="data/heritage-recon", help="Heritage-Recon root")
    ap.add_argument("--sample_surface", type=float, nargs="?", const=10, default=None, metavar="K",
                    help="score the prediction by K * |GT| area-weighted surface samples (needs a file with faces)")
    ap.add_argument("--surface_seed", type=int, default=0, help="seed of the surface samples")
    ap.add_argument("--surface_mode", choices=["iid", "stratified"], default="stratified", help="how the samples are drawn")
    ap.add_argument("--error_clouds", default=False, action="store_true",
                    help="write the error-coloured clouds of every threshold")
    ap.add_argument("--exact_recall", default=False, action="store_true",
                    help="needs --keep_faces; refused without: reprojected.ply has no faces (or score a mesh with "
                         "scripts/eval_mesh.py --exact_recall)")
    ap.add_argument("--normal_consistency", type=int, nargs="?", const=16, default=None, metavar="K",
                    help="also report the normal consistency, normals from K nearest neighbours (scripts/eval_mesh.py)")
    ap.add_argument("--keep_faces", default=False, action="store_true",
                    help="keep the faces through the filter and score reprojected_mesh.ply")
    ap.add_argument("--min_corners", type=int, choices=[1, 2, 3], default=1, help="--keep_faces: marked corners a face needs")
    ap.add_argument("--min_component_faces", type=int, default=0,
                    help="--keep_faces: drop connected components of fewer kept faces")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.exact_recall and not args.keep_faces:
        raise SystemExit("--exact_recall needs a triangle mesh: the pipeline scores mesh/reprojected.ply, a point cloud (the "
                         "reprojection filter does not keep the faces).  Score the mesh itself with scripts/eval_mesh.py "
                         "--exact_recall.")
    print("Evaluating %s ..." % args.pred_dir)
    reproj.eval_pipeline(args.scene_name, args.pred_dir, args.data_root, surface=args.sample_surface,
                         surface_seed=args.surface_seed, surface_mode=args.surface_mode,
                         error_clouds=True if args.error_clouds else None, keep_faces=args.keep_faces,
                         min_corners=args.min_corners, min_component_faces=args.min_component_faces,
                         exact_recall=args.exact_recall,
                         **({} if args.normal_consistency is None else {"normals": args.normal_consistency}))


if __name__ == "__main__":
    main()
