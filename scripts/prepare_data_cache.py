"""Writes the training ray cache of a scene on the GPU: the replacement of the reference's
tools/prepare_data/prepare_data_cache.py (same flags; see neuralrecon_w_amd/cachebuild.py).

    python scripts/prepare_data_cache.py --root_dir data/heritage-recon/brandenburg_gate --cache_type npz \\
        --semantic_map_path semantic_maps --split_to_chunks 64

writes <root_dir>/<cache_dir>/splits/split_*/{rays,rgbs}<N>.npz (+ the two meta_info.json), what scripts/train.py reads.
Beyond the reference's flags: --sfm_path (the COLMAP model under dense/; default: the reference's per-scene choice), --seed (the
depth padding and the chunk padding are drawn from seeded generators), --device, --depth_percent.  Only npz is written; the
reference's default `--cache_type h5` is refused with a message (h5py is not a dependency and the reader takes npz)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root_dir", type=str, required=True, help="root directory of dataset")
    ap.add_argument("--dataset_name", type=str, default="phototourism", choices=["phototourism"], help="which dataset to generate cache")
    ap.add_argument("--cache_dir", type=str, default="cache", help="used as output directory of cache")
    ap.add_argument("--cache_type", type=str, default="npz", choices=["h5", "npz"], help="which type of cache to save (only npz is written)")
    ap.add_argument("--img_downscale", type=int, default=1, help="how much to downscale the images for phototourism dataset")
    ap.add_argument("--split_to_chunks", type=int, default=-1, help="split large cache files to small chunks")
    ap.add_argument("--semantic_map_path", type=str, default=None, help="directory (under root_dir) of the per-image label maps")
    ap.add_argument("--sfm_path", type=str, default=None, help="COLMAP model under <root_dir>/dense/ (default: the reference's per-scene choice)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the depth padding and the chunk padding")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--depth_percent", type=float, default=None, help="override the per-scene share of rays with a key-point depth")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    from neuralrecon_w_amd import cachebuild

    print("Preparing cache for scale %d..." % args.img_downscale)
    stats = {}
    t0 = time.time()
    files = cachebuild.build_cache(args.root_dir, args.cache_dir, args.img_downscale, args.semantic_map_path, args.split_to_chunks,
                                   args.sfm_path, args.seed, args.device, cache_type=args.cache_type, depth_percent=args.depth_percent,
                                   stats=stats)
    print("%d images, %d of %d rays kept, %.1f MB device -> host; decode %.1f s, device %.1f s, write %.1f s; %.1f s in all"
          % (stats["n_images"], stats["n_rays"], stats["n_pixels"], stats["d2h_bytes"] / 1e6, stats["t_decode"], stats["t_device"],
             stats["t_write"], time.time() - t0))
    print("Data cache saved to %s ! (%d files)" % (os.path.join(args.root_dir, args.cache_dir), len(files)))


if __name__ == "__main__":
    main()
