"""Writes a synthetic phototourism scene with known ground truth (neuralrecon_w_amd/synth.py): images with per-image appearance
and transient occluders, semantic maps, a COLMAP model with noisy tracks, the split, config.yaml with the TRUE sfm2gt, gt.ply,
mesh.ply, train.yaml and truth.json.  The reference has no such tool: its scenes are downloaded.

    python scripts/make_synthetic_scene.py --out data/synth_facade [--mesh file.ply] [--n_views 60] [--size 512x384]
        [--n_points 40000] [--n_gt 2000000] [--pixel_sigma 0.5] [--n_occluders 2] [--ss 2] [--seed 0] [--jpeg] [--overwrite]

--mesh: any triangle PLY in the ground-truth frame (z up; vertex colours become materials); default: the built-in facade.
The same arguments write the same bytes.  Needs a GPU: the images come from the rasterizer and csrc/ncw_synth.hip."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, required=True, help="the scene directory to write")
    ap.add_argument("--mesh", type=str, default=None, help="a triangle PLY in the GT frame (default: the built-in facade)")
    ap.add_argument("--n_views", type=int, default=60)
    ap.add_argument("--size", type=str, default="512x384", help="largest image size, WxH; the views vary below it")
    ap.add_argument("--n_points", type=int, default=40000, help="surface samples that may become SfM points")
    ap.add_argument("--n_gt", type=int, default=2000000, help="points of gt.ply")
    ap.add_argument("--pixel_sigma", type=float, default=0.5, help="standard deviation of the key-point noise per axis, pixels")
    ap.add_argument("--n_occluders", type=int, default=2, help="person-sized boxes per image")
    ap.add_argument("--ss", type=int, default=2, help="sub-samples per pixel and axis (1..4)")
    ap.add_argument("--max_edge", type=float, default=0.5, help="longest triangle edge of the built-in facade, metres")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--jpeg", action="store_true", help="write JPEG images (through PIL) instead of PNG")
    ap.add_argument("--overwrite", action="store_true", help="replace an existing directory")
    ap.add_argument("--device", type=str, default="cuda:0")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    from neuralrecon_w_amd import synth

    try:
        w, h = [int(v) for v in args.size.lower().split("x")]
    except ValueError:
        raise SystemExit("--size: WxH expected, e.g. 512x384 (got %r)" % args.size)
    mesh = synth.load_mesh(args.mesh) if args.mesh else None
    info = synth.generate(args.out, mesh, seed=args.seed, n_views=args.n_views, size=(w, h), n_points=args.n_points, n_gt=args.n_gt,
                          pixel_sigma=args.pixel_sigma, n_occluders=args.n_occluders, ss=args.ss, max_edge=args.max_edge, jpeg=args.jpeg,
                          overwrite=args.overwrite, device=args.device, verbose=True)
    out = args.out
    print("wrote %s: %d images, %d SfM points (%d outliers), %d GT points, sfm2gt scale %.4f"
          % (out, len(info["names"]), info["n_points3d"], len(info["truth"]["outlier_point_ids"]), info["n_gt"], info["truth"]["scale"]))
    print("what applies to it now:")
    for line in ("python scripts/train.py --cfg_path %s/train.yaml --ray_source scene --sfm_path sparse --max_steps 5000" % out,
                 "python scripts/extract_mesh.py --cfg_path %s/train.yaml --ckpt_path <checkpoint> --eval_level 9" % out,
                 "python scripts/eval_mesh.py --file_pred %s/mesh.ply --file_trgt %s/gt.ply --scene_config_path %s/config.yaml --exact_recall"
                 "   # the true mesh: recall 1" % (out, out, out),
                 "python scripts/render_view.py --cfg_path %s/train.yaml --ckpt_path <checkpoint> --sfm_path sparse [--surface]" % out,
                 "python scripts/surface_cloud.py --cfg_path %s/train.yaml --ckpt_path <checkpoint> --sfm_path sparse --max_views 16" % out,
                 "python scripts/eval_depth.py --root_dir %s --gt_mesh %s/mesh.ply --pred_mesh <extracted mesh> | --cfg_path %s/train.yaml "
                 "--ckpt_path <checkpoint>   # depth / normal maps per view against the true mesh" % (out, out, out),
                 "python scripts/estimate_sfm2gt.py --data_dir %s --gt_pcd_path %s/gt.ply   # the answer is in config.yaml and truth.json" % (out, out)):
        print("  " + line)


if __name__ == "__main__":
    main()
