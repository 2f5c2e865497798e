"""Writes <root_dir>/config.yaml from the scene's SfM points: the `bbx_selection` / `generate_config` part of the reference's
tools/pre_process.py (:35-46, 102-108, 135-158; see neuralrecon_w_amd/sceneprep.py).

    python scripts/prepare_scene_config.py --root_dir data/my_scene [--name my_scene] [--sfm_path sparse] [--overwrite]

The box is the 4th .. 96th percentile per axis of the points with more than 2 observations; origin its centre, radius its
longest edge.  sfm2gt is the identity: a scene with ground truth replaces it with scripts/estimate_sfm2gt.py (which also suggests
an eval_bbx; the reference's scenes ship both).
The folder regrouping and COLMAP's image undistorter of pre_process.py are not part of this tool.  No GPU is needed."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_dir", type=str, required=True, help="root directory of the scene")
    ap.add_argument("--name", type=str, default=None, help="the scene's name (default: the directory name)")
    ap.add_argument("--sfm_path", type=str, default="sparse", help="COLMAP model under <root_dir>/dense/")
    ap.add_argument("--overwrite", action="store_true", help="replace an existing config.yaml")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    from neuralrecon_w_amd import sceneprep

    path = sceneprep.write_scene_config(args.root_dir, None, args.name, args.sfm_path, args.overwrite)
    print(open(path).read(), end="")
    print("wrote %s" % path)


if __name__ == "__main__":
    main()
