"""Estimates a scene's sfm2gt on the GPU: gated similarity ICP of the filtered SfM points onto the ground-truth cloud
(neuralrecon_w_amd/align.py; the reference has no such tool, it ships the matrices).

    python scripts/estimate_sfm2gt.py --data_dir data/my_scene --gt_pcd_path gt/lidar.ply --pairs landmarks.txt --out_dir samples/align
    python scripts/reproj_error.py --data_dir data/my_scene --gt_pcd_path gt/lidar.ply        # afterwards: that remains the check

ICP is local: it REFINES an initial matrix.  --init config (default) starts from sfm2gt of <data_dir>/config.yaml, --init identity
from the identity, --init <file> from a matrix file (16 or 12 numbers as text, .npy, or a yaml / json file with an `sfm2gt` key);
--pairs <file> (rows `x y z X Y Z`: a point in SfM coordinates and the same point in ground-truth coordinates, three or more, not
collinear) is solved in closed form and used instead.  The source is the COLMAP points of <data_dir>/<reconstuct_path> with MORE
THAN --track_length observations and a mean reprojection error BELOW --reproj_error.  --gate0 / --gate_min default to 0.2 x the
longest edge of the cloud's box and 4 x its median point spacing; both are recorded in the report.
The nearest-neighbour queries are radius-bounded by default (nearest target point within the gate, or none: one launch, no
brute-force pass); --no_bounded takes the earlier path -- the same sfm2gt.yaml byte for byte, slower.
Writes report.json (initial and final matrix, the correction's scale / rotation / translation, iterations, pairs and inlier share,
rms, the ground-truth box of the matched points as a suggestion for eval_bbx, the per-iteration history) and sfm2gt.yaml into
--out_dir and prints the matrix.  <data_dir>/config.yaml is left alone unless --write_config is given: then its sfm2gt value is
replaced (the other keys and their order stay), after the previous file was copied to config.yaml.bak; an existing backup is never
overwritten -- the command refuses."""
import argparse
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_dir", type=str, required=True, help="the scene directory: config.yaml, dense/")
    ap.add_argument("--gt_pcd_path", type=str, required=True, help="the ground-truth point cloud (PLY)")
    ap.add_argument("--reconstuct_path", type=str, default="dense/sparse", help="COLMAP model under data_dir (the reference's spelling)")
    ap.add_argument("--init", type=str, default="config", help="config | identity | a matrix file")
    ap.add_argument("--pairs", type=str, default=None, help="text file of `x y z X Y Z` rows (SfM point, ground-truth point): the initial matrix")
    ap.add_argument("--track_length", type=int, default=8, help="keep SfM points with MORE observations than this")
    ap.add_argument("--reproj_error", type=float, default=1.0, help="keep SfM points whose error is BELOW this")
    ap.add_argument("--no_scale", action="store_true", help="rigid: rotation and translation only")
    ap.add_argument("--gate0", type=float, default=None, help="first gate (default 0.2 x the longest edge of the cloud's box)")
    ap.add_argument("--shrink", type=float, default=0.85, help="the gate's factor per iteration")
    ap.add_argument("--gate_min", type=float, default=None, help="smallest gate (default 4 x the cloud's median point spacing)")
    ap.add_argument("--max_iter", type=int, default=60)
    ap.add_argument("--min_pairs", type=int, default=None, help="fail below this many pairs (default 10 %% of the source)")
    ap.add_argument("--no_bounded", action="store_true", help="answer the nearest-neighbour queries without the radius bound (the earlier "
                    "path, brute-force pass included): the same sfm2gt.yaml, slower; kept for the comparison")
    ap.add_argument("--out_dir", type=str, default=os.path.join("samples", "align"))
    ap.add_argument("--write_config", action="store_true", help="replace sfm2gt in <data_dir>/config.yaml (backup: config.yaml.bak)")
    ap.add_argument("--device", type=str, default="cuda:0")
    return ap


def write_config(data_dir, matrix):
    """Replaces the sfm2gt value of <data_dir>/config.yaml, the other keys and their order kept (sceneprep's writer); the previous
    file goes to config.yaml.bak first, and an existing backup is refused (FileExistsError) before anything is written."""
    import numpy as np
    import yaml

    from neuralrecon_w_amd import sceneprep

    path = os.path.join(data_dir, "config.yaml")
    backup = path + ".bak"
    if os.path.exists(backup):
        raise FileExistsError("%s exists: move it away first (it holds the config this command would overwrite a second time)" % backup)
    with open(path, "r") as fh:
        cfg = yaml.safe_load(fh)
    if not isinstance(cfg, dict) or "sfm2gt" not in cfg:
        raise ValueError("%s has no sfm2gt key" % path)
    shutil.copyfile(path, backup)
    cfg["sfm2gt"] = np.asarray(matrix, dtype=np.float64).reshape(4, 4).tolist()  # assignment to an existing key keeps its place
    return sceneprep.write_scene_config(data_dir, cfg, overwrite=True)


def main(argv=None):
    args = build_parser().parse_args(argv)
    import numpy as np
    import yaml

    from neuralrecon_w_amd import align

    pairs = np.loadtxt(args.pairs, dtype=np.float64).reshape(-1, 6) if args.pairs else None
    if args.write_config and os.path.exists(os.path.join(args.data_dir, "config.yaml.bak")):
        raise FileExistsError("%s exists: refusing before the run" % os.path.join(args.data_dir, "config.yaml.bak"))
    T, rep = align.estimate_sfm2gt(args.data_dir, args.gt_pcd_path, args.reconstuct_path, args.init, pairs, args.track_length,
                                   args.reproj_error, args.device, gate0=args.gate0, shrink=args.shrink, gate_min=args.gate_min,
                                   max_iter=args.max_iter, with_scale=not args.no_scale, min_pairs=args.min_pairs,
                                   bounded=not args.no_bounded)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "report.json"), "w") as fh:
        json.dump(rep, fh, indent=1)
    with open(os.path.join(args.out_dir, "sfm2gt.yaml"), "w") as fh:
        yaml.dump({"sfm2gt": T.tolist()}, fh, default_flow_style=False, sort_keys=False)
    np.set_printoptions(precision=10, suppress=True, linewidth=160)
    print(T)
    c = rep["correction"]
    print("%d iterations (%s), %d of %d SfM points paired (%.1f %%), rms %.4g; correction of the initial matrix: scale %.6f, rotation "
          "%.4f deg, translation %.4g -> %s" % (rep["iterations"], "fixed point" if rep["converged"] else "max_iter reached", rep["pairs"],
                                                rep["source_points"], 100 * rep["inlier_share"], rep["rms"], c["scale"], c["rotation_deg"],
                                                c["translation"], args.out_dir))
    if args.write_config:
        print("wrote %s (previous: config.yaml.bak)" % write_config(args.data_dir, T))
    print("now run scripts/reproj_error.py on the scene: the reprojection error in pixels is the check of this matrix")
    return T, rep


if __name__ == "__main__":
    main()
