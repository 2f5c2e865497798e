"""Render one camera view of a trained scene: the image half of the reference's validation step
(lightning_modules/neuconw_system.py:404-464, 533-546) as a command line -- GT | prediction | depth | normal as one PNG, PSNR
and SSIM printed.

    python scripts/render_view.py --cfg_path config/train_brandenburg_gate.yaml --ckpt_path ckpts/exp/last.ckpt \
        --root_dir data/heritage-recon/brandenburg_gate [--image_id 12 | --image_name 0001.jpg] [--img_downscale 2] \
        [--chunk 4096] [--out results/view.png]

  * the view is the dataset's `test_train` item of that image (neuralrecon_w_amd.views.scene_view: K rescale, pose flip,
    per-image near / far from the SfM points; --split val clamps the downscale to >= 8 like the reference's `val` split); the
    default image is the first training image, the appearance index the image id (--ts overrides it);
  * rays, chunk assembly, the depth colour map and the metrics run on the GPU (csrc/ncw_view.hip); the render is the
    forward-only render at perturb 0.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cfg_path", required=True, help="experiment yaml")
    ap.add_argument("--ckpt_path", required=True, help="checkpoint in the reference's layout (trainer.save_checkpoint / PL)")
    ap.add_argument("--root_dir", default=None, help="overrides DATASET.ROOT_DIR")
    which = ap.add_mutually_exclusive_group()
    which.add_argument("--image_id", type=int, default=None, help="COLMAP image id (default: the first training image)")
    which.add_argument("--image_name", default=None, help="image file name as registered in images.bin")
    ap.add_argument("--img_downscale", type=int, default=None, help="default: DATASET.PHOTOTOURISM.IMG_DOWNSCALE")
    ap.add_argument("--split", default="test_train", choices=["test_train", "val"],
                    help="val clamps the downscale to >= 8 (datasets/phototourism.py:70-71)")
    ap.add_argument("--ts", type=int, default=None, help="appearance index (default: the image id)")
    ap.add_argument("--chunk", type=int, default=None, help="rays per render launch (default: views.DEFAULT_CHUNK)")
    ap.add_argument("--ssim_window", type=int, default=3, choices=[3, 5, 7, 9, 11], help="3 = the reference's metrics.py")
    ap.add_argument("--sfm_path", default=None,
                    help="COLMAP model directory under <root_dir>/dense/ -- the one the ray cache was built from (default: the "
                         "reference's per-scene choice, ../neuralsfm for brandenburg_gate and palacio_de_bellas_artes, else sparse)")
    ap.add_argument("--prec", default=None, choices=["bf16", "f16", "f32"], help="default: the package default")
    ap.add_argument("--out", default=None, help="PNG path (default: results/views/<ckpt dir>_<ckpt name>/<image id>.png)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch

    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import config as C
    from neuralrecon_w_amd import trainer, views

    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    cfg = C.load_config(args.cfg_path, {"DATASET": {"ROOT_DIR": args.root_dir}} if args.root_dir else None)
    prec = {None: None, "bf16": nw.PREC_BF16, "f16": nw.PREC_F16, "f32": nw.PREC_F32}[args.prec]
    emb, neuconw, nerf, rdr, scene = C.build_system(cfg, dev, prec)
    trainer.load_checkpoint(args.ckpt_path, emb, neuconw, nerf)
    for m in (emb, neuconw, nerf):
        m.eval()
    root = cfg["DATASET"]["ROOT_DIR"]
    downscale = args.img_downscale if args.img_downscale is not None else int(cfg["DATASET"]["PHOTOTOURISM"]["IMG_DOWNSCALE"])
    cam, gt, image_id = views.scene_view(root, image_id=args.image_id, image_name=args.image_name, img_downscale=downscale,
                                         sfm_path=args.sfm_path, split=args.split)
    out = views.render_view(rdr, cam, ts=image_id if args.ts is None else args.ts, chunk=args.chunk or views.DEFAULT_CHUNK,
                            gt=gt.to(dev), ssim_window=args.ssim_window,
                            nerf_far_override=bool(cfg["NEUCONW"]["NEAR_FAR_OVERRIDE"]))  # neuconw_system.py:407
    save_name = "_".join(os.path.normpath(args.ckpt_path).split(os.sep)[-2:]).replace(".ckpt", "")
    path = args.out or os.path.join("results", "views", save_name, "%d.png" % image_id)
    w, h = views.write_panel(path, gt, out["color"], out["depth_vis"], out["normal"])
    print("image %d (%d x %d): psnr %.4f  ssim %.4f  mse %.6f -> %s (%d x %d)"
          % (image_id, cam.width, cam.height, float(out["psnr"]), float(out["ssim"]), float(out["mse"]), path, w, h))


if __name__ == "__main__":
    main()
