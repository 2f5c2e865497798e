"""Clean a point cloud and give it normals on the GPU (neuralrecon_w_amd.cloudops over the exact k-NN grid): statistical
outlier removal, then normals from the PCA of every survivor's neighbourhood.

    python scripts/clean_cloud.py --file_in cloud.ply --file_out clean.ply [--outlier_k 16 --outlier_ratio 2.0] \
        [--normals_k 16] [--toward x,y,z]

  * outliers: m_i = the mean distance of point i to its --outlier_k nearest other points; a point stays when
    m_i <= mean(m) + --outlier_ratio * std(m) (the rule of open3d's remove_statistical_outlier; unpinned against it).
    --outlier_k 0 skips the step;
  * normals: the eigenvector of the smallest eigenvalue of the covariance of the point and its --normals_k nearest other
    points, estimated on the SURVIVORS; --toward x,y,z makes them face that viewpoint, otherwise the component of largest
    magnitude is positive (unoriented normals: nothing propagates orientation).  Points whose neighbourhood is collinear or
    coincident get a zero normal;
  * the output is a binary PLY with double coordinates, float normals and, if the input has them, its colours; faces of
    the input are not kept.  Prints the points before / after and the share of invalid normals.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import cloudops, ply  # noqa: E402


def _xyz(text):
    vals = [float(v) for v in str(text).split(",")]
    if len(vals) != 3:
        raise argparse.ArgumentTypeError("--toward takes x,y,z (got %r)" % text)
    return vals


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--file_in", required=True, help="the cloud to clean (PLY)")
    ap.add_argument("--file_out", required=True, help="the cleaned cloud with normals (PLY)")
    ap.add_argument("--outlier_k", type=int, default=16, help="neighbours of the outlier statistic (0 = keep every point)")
    ap.add_argument("--outlier_ratio", type=float, default=2.0, help="standard deviations above the mean that are kept")
    ap.add_argument("--normals_k", type=int, default=16, help="neighbours of the normal estimate")
    ap.add_argument("--toward", type=_xyz, default=None, metavar="x,y,z", help="viewpoint the normals face")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    verts, _, rgb = ply.read_mesh(args.file_in)
    dev = torch.device("cuda", torch.cuda.current_device())
    pts = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float64)).to(dev)
    n_in = int(pts.shape[0])
    if args.outlier_k > 0:
        keep, _ = cloudops.remove_statistical_outliers(pts, k=args.outlier_k, ratio=args.outlier_ratio)
        pts = pts[keep]
        if rgb is not None:
            rgb = rgb[keep.cpu().numpy()]
    normals, _, valid = cloudops.estimate_normals(pts, k=args.normals_k, toward=args.toward)
    n_out = int(pts.shape[0])
    ply.write(args.file_out, pts.cpu().numpy(), rgb=rgb, normals=normals.cpu().numpy())
    bad = n_out - int(valid.sum())
    print("points: %d -> %d (%d removed)" % (n_in, n_out, n_in - n_out))
    print("invalid normals: %d (%.3f %%)" % (bad, 100.0 * bad / max(1, n_out)))
    return n_in, n_out, bad


if __name__ == "__main__":
    main()
