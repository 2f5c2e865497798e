"""Writes the train / test split of a scene on the GPU: the replacement of the reference's
tools/prepare_data/prepare_data_split.py (same flags and defaults; see neuralrecon_w_amd/sceneprep.py).

    python scripts/prepare_data_split.py --root_dir data/heritage-recon/brandenburg_gate --num_test 10 \\
        --roi_threshold 0 --static_threshold 0

reads <root_dir>/config.yaml (origin, radius), the COLMAP model under <root_dir>/dense/ and the image headers, tests every pixel
of every registered image against the scene sphere in ONE launch, permutes the surviving images, applies the transient filter
to <root_dir>/<semantic_map_path>/*.npz and writes <root_dir>/<dirname>.tsv -- what scripts/prepare_data_cache.py and
scripts/train.py read -- and <root_dir>/split_report.json (per image: ROI share, static share, kept / reason; the reference
re-encodes rejected images into trash_images/ instead).
Beyond the reference's flags: --seed (the reference's permutation is unseeded), --sfm_path (the COLMAP model under dense/),
--overwrite (an existing *.tsv is refused otherwise), --visualize (the ROI mask of every view the ROI rule rejected, as
<root_dir>/split_roi_masks/<stem>_roi.png), --device.  --nima_ckpt_path is accepted and ignored: the reference's NIMA filter is
commented out (prepare_data_split.py:41)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_dir", type=str, required=True, help="the scene directory: config.yaml, dense/, semantic maps")
    ap.add_argument("--num_test", type=int, default=10, help="how many rows at the head of the tsv are marked test")
    ap.add_argument("--min_observation", type=int, default=-1, help="n > 0: also require the image in dense/sparse_filtered_<n>/images.bin (or fx, fy > 2000)")
    ap.add_argument("--roi_threshold", type=float, default=0.5, help="drop an image whose share of pixels that see the scene sphere is below this")
    ap.add_argument("--static_threshold", type=float, default=0.6, help="keep an image only if its share of non-transient pixels exceeds this")
    ap.add_argument("--nima_ckpt_path", type=str, default="weights/nima_epoch-34.pth", help="accepted and ignored (the NIMA filter is dead in the reference)")
    ap.add_argument("--semantic_map_path", type=str, default="semantic_maps", help="directory (under root_dir) of the per-image label maps")
    ap.add_argument("--seed", type=int, default=0, help="seed of the permutation")
    ap.add_argument("--sfm_path", type=str, default="sparse", help="COLMAP model under <root_dir>/dense/")
    ap.add_argument("--overwrite", action="store_true", help="replace an existing *.tsv")
    ap.add_argument("--visualize", action="store_true", help="write the ROI mask of every ROI-rejected view as a PNG")
    ap.add_argument("--device", type=str, default="cuda:0")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    from neuralrecon_w_amd import sceneprep

    if args.nima_ckpt_path != ap.get_default("nima_ckpt_path"):
        print("note: --nima_ckpt_path is ignored: the reference's NIMA filter is commented out and is not restated")
    out = sceneprep.prepare_split(args.root_dir, args.num_test, args.min_observation, args.roi_threshold, args.static_threshold,
                                  args.semantic_map_path, args.seed, args.device, args.sfm_path, args.overwrite,
                                  os.path.join(args.root_dir, "split_roi_masks") if args.visualize else None)
    print("%d images (%d test) -> %s; %d rejected, see %s" % (len(out["names"]), args.num_test, out["tsv"], len(out["reasons"]), out["report"]))


if __name__ == "__main__":
    main()
