"""Held-out views of a trained scene, the NeRF-W way: for every `test` row of the scene's split file, fit the appearance code
on the LEFT half of the image with every network weight frozen, render the view with it and score the RIGHT half
(datasets/phototourism.py:520-556, 726-748 hand out exactly these halves; the reference has no consumer for them).

    python scripts/eval_views.py --cfg_path config/train_brandenburg_gate.yaml --ckpt_path ckpts/exp/last.ckpt \
        --root_dir data/heritage-recon/brandenburg_gate [--img_downscale 2] [--n_rays 8192] [--steps 200] [--lr 0.02] \
        [--seed 0] [--init mean|zeros] [--chunk 1024] [--out_dir results/eval_views/<ckpt dir>_<ckpt name>]

  * writes <out_dir>/metrics.json -- per image psnr_right, ssim_right, psnr_full, loss_start, loss_end, skipped_steps, and
    their means -- and one GT | prediction | depth | normal panel per image;
  * the fit runs on frozen geometry (neuralrecon_w_amd.appfit): per iteration only the colour network, the background colour
    head and two small launches (csrc/ncw_appfit.hip);
  * --steps and --lr are this project's defaults, not the reference's: it never runs this fit.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cfg_path", required=True, help="experiment yaml")
    ap.add_argument("--ckpt_path", required=True, help="checkpoint in the reference's layout (trainer.save_checkpoint / PL)")
    ap.add_argument("--root_dir", required=True, help="scene directory (overrides DATASET.ROOT_DIR)")
    ap.add_argument("--img_downscale", type=int, default=None, help="default: DATASET.PHOTOTOURISM.IMG_DOWNSCALE")
    ap.add_argument("--n_rays", type=int, default=8192, help="left-half pixels the fit sees (all if the half holds fewer)")
    ap.add_argument("--steps", type=int, default=200, help="full-batch Adam iterations per image")
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--seed", type=int, default=0, help="seed of the pixel subset")
    ap.add_argument("--init", default="mean", choices=["mean", "zeros"],
                    help="start code: the mean embedding row of the split's train images, or zeros")
    ap.add_argument("--chunk", type=int, default=1024, help="rays per frozen-geometry chunk")
    ap.add_argument("--out_dir", default=None, help="default: results/eval_views/<ckpt dir>_<ckpt name>")
    ap.add_argument("--sfm_path", default=None, help="COLMAP model directory under <root_dir>/dense/ (default: the reference's)")
    ap.add_argument("--prec", default=None, choices=["bf16", "f16", "f32"], help="default: the package default")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch

    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import appfit

    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    prec = {None: None, "bf16": nw.PREC_BF16, "f16": nw.PREC_F16, "f32": nw.PREC_F32}[args.prec]
    save_name = "_".join(os.path.normpath(args.ckpt_path).split(os.sep)[-2:]).replace(".ckpt", "")
    out_dir = args.out_dir or os.path.join("results", "eval_views", save_name)
    res = appfit.eval_views(args.root_dir, args.cfg_path, args.ckpt_path, img_downscale=args.img_downscale, n_rays=args.n_rays,
                            steps=args.steps, lr=args.lr, seed=args.seed, init=args.init, chunk=args.chunk, out_dir=out_dir,
                            sfm_path=args.sfm_path, prec=prec, device=dev)
    for name, m in res["images"].items():
        print("%s: psnr_right %.4f  ssim_right %.4f  psnr_full %.4f  loss %.5f -> %.5f  skipped %d"
              % (name, m["psnr_right"], m["ssim_right"], m["psnr_full"], m["loss_start"], m["loss_end"], m["skipped_steps"]))
    m = res["mean"]
    print("mean over %d image(s): psnr_right %.4f  ssim_right %.4f  psnr_full %.4f -> %s"
          % (len(res["images"]), m["psnr_right"], m["ssim_right"], m["psnr_full"], os.path.join(out_dir, "metrics.json")))


if __name__ == "__main__":
    main()
