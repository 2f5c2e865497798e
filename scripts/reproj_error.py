"""Checks a scene's sfm2gt alignment on the GPU: the replacement of the reference's tools/reproj_error.py (same flags and
defaults; see neuralrecon_w_amd/gtreproj.py).

    python scripts/reproj_error.py --data_dir data/heritage-recon/brandenburg_gate --gt_pcd_path gt/bg_sampled_0.01_cropped.ply \\
        --reconstuct_path dense/sparse --track_length 200 --reproj_error 0.4

reads sfm2gt from <data_dir>/config.yaml and the COLMAP model <data_dir>/<reconstuct_path>, drops the images whose mean
reprojection error exceeds --img_reproj_error, and for every track with MORE THAN --track_length observations and an error BELOW
--reproj_error finds the ground-truth point nearest to the camera on the pixel of the track's first observation -- one pass over
the cloud for all tracks -- and reprojects it into the track's other views.  Prints the mean distance to the SfM key-points in
pixels (small when sfm2gt is right) and writes, into --out_dir (default samples/reproject, as the reference), report.json (the
mean, the per-element errors that the reference plots, per-image errors, the counts of kept images / tracks and of tracks
without a ground-truth point), colmap_sfm.ply and gt.ply.
Beyond the reference's flags: --out_dir; --reference_unmatched (the per-image error as the reference computes it: key-points
without a 3-D point are measured against the point of the highest id, which its default --img_reproj_error 300 was tuned to);
--visualize (the per-image red / green PNGs, under <out_dir>/reprojects); --chunk (cloud points per launch); --device.
--batch_size is accepted and ignored."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_dir", type=str, required=True, help="the scene directory: config.yaml, dense/")
    ap.add_argument("--gt_pcd_path", type=str, required=True, help="the ground-truth point cloud (PLY)")
    ap.add_argument("--reconstuct_path", type=str, default="dense/sparse", help="COLMAP model under data_dir (the reference's spelling)")
    ap.add_argument("--track_length", type=int, default=200, help="keep tracks with MORE observations than this")
    ap.add_argument("--reproj_error", type=float, default=0.4, help="keep tracks whose error is BELOW this")
    ap.add_argument("--batch_size", type=int, default=2, help="accepted and ignored: all tracks go through one pass")
    ap.add_argument("--img_reproj_error", type=float, default=300, help="drop images whose mean reprojection error is not below this")
    ap.add_argument("--out_dir", type=str, default=os.path.join("samples", "reproject"))
    ap.add_argument("--reference_unmatched", action="store_true", help="per-image error over ALL key-points, as the reference computes it")
    ap.add_argument("--visualize", action="store_true", help="write the per-image reprojection PNGs")
    ap.add_argument("--chunk", type=int, default=None, help="cloud points per launch (default 2^24)")
    ap.add_argument("--device", type=str, default="cuda:0")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    import numpy as np
    import yaml

    from neuralrecon_w_amd import gtreproj

    with open(os.path.join(args.data_dir, "config.yaml"), "r") as fh:
        cfg = yaml.safe_load(fh)
    rep = gtreproj.gt_reprojection_error(args.data_dir, args.gt_pcd_path, np.array(cfg["sfm2gt"]), args.reconstuct_path, args.track_length,
                                         args.reproj_error, args.img_reproj_error, args.batch_size, args.reference_unmatched, args.chunk,
                                         args.device)
    path = gtreproj.write_outputs(rep, args.out_dir, args.visualize)
    print("%d of %d images, %d tracks (%d more without a ground-truth point), %d elements -> %s"
          % (rep["n_images_kept"], rep["n_images"], rep["n_tracks"], rep["n_tracks_no_gt"], len(rep["errors"]), path))
    return rep


if __name__ == "__main__":
    main()
