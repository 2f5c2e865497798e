"""Mesh evaluation driver: the reference's `utils/eval_mesh.py` command line (:15-44, :126-147) without
kaolin, trimesh, matplotlib or open3d -- precision / recall / F-score of a predicted mesh or point cloud against the
ground-truth cloud, nearest neighbours on the GPU (neuralrecon_w_amd.evalmesh).

    python scripts/eval_mesh.py --file_pred results/.../extracted_mesh_res_1024_radius_1.0.ply --file_trgt gt.ply \
        --scene_config_path data/heritage-recon/brandenburg_gate/config.yaml --threshold 0.01,1,0.01 --bbx_name eval_bbx \
        [--sfm_path data/.../dense/sparse --track_lenth 10 --reproj_error 1.0 --voxel_size 0.1] --save_name bg

  * --threshold: "start,end,interval" = np.arange(start, end, interval) like the reference, or one value ("0.1");
  * results under <dir of file_pred>/eval_<save_name>/ (the reference's layout: down_gt.ply, down_pred_in_gt.ply, the SfM
    crop's sfm_points.ply / pred_filtered.ply / target_filtered.ply, visualize/<t>/metrics.json, metrics.json);
  * --mesh is accepted and, as in the reference's trimesh branch, changes nothing: the prediction is scored by its vertices;
  * --sample_surface [K] (K = 10 when omitted, the reference's value) scores a predicted MESH by its surface, as the
    reference's open3d branch does with --mesh: K |GT| points drawn uniformly by area on the GPU from the triangles inside
    the box (--surface_seed, --surface_mode iid|stratified);
  * --exact_recall measures the recall side (GT point -> prediction) to the predicted SURFACE: exact point-to-triangle
    distances on the GPU instead of the distance to the nearest vertex or sample; the prediction must have faces; the
    precision side is unchanged; metrics.json gains "recal_mode": "exact";
  * --normal_consistency [K] (K = 16 when omitted) adds the normal consistency of the two scored clouds to metrics.json:
    normals of both estimated from K nearest neighbours on the GPU, |n . n'| averaged over the nearest-neighbour pairs in
    both directions, overall and per threshold; refused with --exact_recall;
  * --error_clouds also writes visualize/<t>/error_pred_precision.ply and error_gt_recal.ply (jet colours of the errors).
"""
import argparse
import os
import sys

import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import evalmesh  # noqa: E402


def get_opts(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--file_pred", required=True, help="ply file path for prediction")
    ap.add_argument("--file_trgt", required=True, help="ply file path for ground truth")
    ap.add_argument("--scene_config_path", required=True, help="scene config path")
    ap.add_argument("--mesh", default=False, action="store_true", help="whether prediction is mesh")
    ap.add_argument("--threshold", type=str, default="0.1",
                    help="threshold for precision and recall: one value, or start,end,interval")
    ap.add_argument("--bbx_name", type=str, default="eval_bbx", help="area to eval")
    ap.add_argument("--sfm_path", type=str, help="if set, eval will use sfm points to crop both gt and prediction")
    ap.add_argument("--track_lenth", type=float, help="track length threshold for sfm points")
    ap.add_argument("--reproj_error", type=float, help="mean reprojection error threshold for sfm points")
    ap.add_argument("--voxel_size", type=float, help="voxel size for sfm points to crop point clouds")
    ap.add_argument("--save_name", type=str, default="eval", help="results go to eval_<save_name>")
    ap.add_argument("--sample_surface", type=float, nargs="?", const=10, default=None, metavar="K",
                    help="score the predicted mesh by K * |GT| area-weighted surface samples (K = 10 when omitted)")
    ap.add_argument("--surface_seed", type=int, default=0, help="seed of the surface samples")
    ap.add_argument("--surface_mode", choices=["iid", "stratified"], default="stratified", help="how the samples are drawn")
    ap.add_argument("--error_clouds", default=False, action="store_true",
                    help="write the error-coloured clouds of every threshold")
    ap.add_argument("--exact_recall", default=False, action="store_true",
                    help="recall from exact point-to-triangle distances to the predicted mesh (needs faces)")
    ap.add_argument("--normal_consistency", type=int, nargs="?", const=16, default=None, metavar="K",
                    help="also report the normal consistency, normals from K nearest neighbours (K = 16 when omitted)")
    return ap.parse_args(argv)


def main(argv=None):
    args = get_opts(argv)
    thresholds = evalmesh.parse_thresholds(args.threshold)
    print("thresholds to eval: %s" % thresholds)
    with open(args.scene_config_path, "r") as f:
        scene_config = yaml.load(f, Loader=yaml.FullLoader)
    sfm = None
    if args.sfm_path:
        print("crop with sfm in %s" % args.sfm_path)
        if args.track_lenth is None or args.reproj_error is None or args.voxel_size is None:
            raise SystemExit("--sfm_path needs --track_lenth, --reproj_error and --voxel_size")
        sfm = {"path": args.sfm_path, "track_length": args.track_lenth, "reproj_error": args.reproj_error,
               "voxel_size": args.voxel_size}
    evalmesh.eval_mesh(args.file_pred, args.file_trgt, scene_config, args.mesh, threshold=thresholds, bbx_name=args.bbx_name,
                       save_name=args.save_name, sfm=sfm, surface=args.sample_surface, surface_seed=args.surface_seed,
                       surface_mode=args.surface_mode, error_clouds=True if args.error_clouds else None,
                       exact_recall=args.exact_recall,
                       **({} if args.normal_consistency is None else {"normals": args.normal_consistency}))


if __name__ == "__main__":
    main()
