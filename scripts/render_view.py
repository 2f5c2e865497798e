"""Render one camera view of a trained scene: the image half of the reference's validation step
(lightning_modules/neuconw_system.py:404-464, 533-546) as a command line -- GT | prediction | depth | normal as one PNG, PSNR
and SSIM printed.

    python scripts/render_view.py --cfg_path config/train_brandenburg_gate.yaml --ckpt_path ckpts/exp/last.ckpt \
        --root_dir data/heritage-recon/brandenburg_gate [--image_id 12 | --image_name 0001.jpg] [--img_downscale 2] \
        [--chunk 4096] [--out results/view.png]
    python scripts/render_view.py ... --surface [--trace_eps 1e-3 --trace_iters 64 --trace_step 1.0]

  * the view is the dataset's `test_train` item of that image (neuralrecon_w_amd.views.scene_view: K rescale, pose flip,
    per-image near / far from the SfM points; --split val clamps the downscale to >= 8 like the reference's `val` split); the
    default image is the first training image, the appearance index the image id (--ts overrides it);
  * rays, chunk assembly, the depth colour map and the metrics run on the GPU (csrc/ncw_view.hip); the render is the
    forward-only render at perturb 0;
  * --surface: the learned SURFACE instead of the volume render (neuralrecon_w_amd.views.trace_view: sphere tracing with the
    value-only SDF kernel, colour and normal evaluated once at the first hit; not in the reference).  The panel becomes
    GT | traced colour | depth | normal; pixels whose ray finds no surface are black.  No background NeRF, no transmittance:
    the PSNR printed is not the reference's validation number (psnr_hit restricts it to the pixels that hit).  The state
    shares, the iteration statistics and the time are printed.  A surface both of whose crossings fall inside one step of the
    walk is jumped (only where |grad sdf| * trace_step > 1): lower --trace_step on such a checkpoint.
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
    ap.add_argument("--surface", action="store_true", help="sphere-trace the surface instead of volume rendering (views.trace_view)")
    ap.add_argument("--trace_eps", type=float, default=1e-3, help="--surface: |sdf| <= eps is a hit (unit-sphere units)")
    ap.add_argument("--trace_iters", type=int, default=64, help="--surface: most SDF evaluations per ray")
    ap.add_argument("--trace_step", type=float, default=1.0, help="--surface: step factor in (0, 1]; < 1 where |grad sdf| > 1")
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
    save_name = "_".join(os.path.normpath(args.ckpt_path).split(os.sep)[-2:]).replace(".ckpt", "")
    if args.surface:
        return surface(args, views, rdr, cam, gt, image_id, dev, bool(cfg["NEUCONW"]["NEAR_FAR_OVERRIDE"]), save_name)
    out = views.render_view(rdr, cam, ts=image_id if args.ts is None else args.ts, chunk=args.chunk or views.DEFAULT_CHUNK,
                            gt=gt.to(dev), ssim_window=args.ssim_window,
                            nerf_far_override=bool(cfg["NEUCONW"]["NEAR_FAR_OVERRIDE"]))  # neuconw_system.py:407
    path = args.out or os.path.join("results", "views", save_name, "%d.png" % image_id)
    w, h = views.write_panel(path, gt, out["color"], out["depth_vis"], out["normal"])
    print("image %d (%d x %d): psnr %.4f  ssim %.4f  mse %.6f -> %s (%d x %d)"
          % (image_id, cam.width, cam.height, float(out["psnr"]), float(out["ssim"]), float(out["mse"]), path, w, h))


def surface(args, views, rdr, cam, gt, image_id, dev, far_override, save_name):
    import time

    import torch

    kw = dict(ts=image_id if args.ts is None else args.ts, chunk=args.chunk or views.TRACE_CHUNK, gt=gt.to(dev),
              ssim_window=args.ssim_window, eps=args.trace_eps, max_iter=args.trace_iters, step=args.trace_step,
              far_override=far_override)
    views.trace_view(rdr, cam, **kw)  # warm-up: weight packing, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = views.trace_view(rdr, cam, **kw)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    path = args.out or os.path.join("results", "views", save_name, "%d_surface.png" % image_id)
    w, h = views.write_panel(path, gt, out["color"], out["depth_vis"], out["normal"])
    s = out["stats"]
    n = float(s["rays"])
    print("image %d (%d x %d) surface: hit %.1f %%  miss %.1f %%  inside %.1f %%  stalled %.1f %%;  iters mean %.1f max %d;  "
          "%d SDF launches over %.2f M points (%.1f per ray);  %.1f ms"
          % (image_id, cam.width, cam.height, 100 * s["hit"] / n, 100 * s["miss"] / n, 100 * s["inside"] / n, 100 * s["stalled"] / n,
             s["iters_mean"], s["iters_max"], s["sdf_launches"], s["sdf_points"] / 1e6, s["sdf_points"] / n, ms))
    print("image %d: psnr %.4f (hit pixels only: %.4f)  ssim %.4f  mse %.6f -> %s (%d x %d)"
          % (image_id, float(out["psnr"]), float(out["psnr_hit"]), float(out["ssim"]), float(out["mse"]), path, w, h))


if __name__ == "__main__":
    main()
