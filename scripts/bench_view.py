"""Times whole-view rendering (neuralrecon_w_amd.views.render_view) on the flagship networks of bench.py: one 1024 x 768 view
at W = 256 with 64 + 64 samples (+ 4 outside) -- 786 432 rays, ~100 M primary ray-samples -- per chunk size.

    python scripts/bench_view.py [--width 1024 --height 768] [--chunks 1024,4096,16384] [--views 3] [--prec f16] [--out DIR]

Per chunk size one JSON line (also written to <out>/view_<W>x<H>.jsonl, default profiles/view/):
  ms_per_view         HIP events around a window of --views whole views (after one warm-up view of the same shape), per view;
  ray_samples_per_s   H W (n_samples + n_importance) / that time  (bench.py --config render's measure);
  glue_ms_per_view    the time between HIP events that bracket every `ncw_view_*` / `ncw_image_*` / `ncw_depth_colormap` call of
                      ONE further view (lib.PROFILE; a separate pass, because the brackets themselves cost host time): ray
                      generation, chunk scatter, depth colour map, PSNR and SSIM -- and its share of ms_per_view.  An UPPER
                      BOUND on the kernels' time: an interval between two events also holds whatever gap the host leaves
                      between the launches (most at small chunks, where the host issues hundreds of chunks per view).
A GPU is required; nothing here is timed on a CPU.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GLUE = ("ncw_view_", "ncw_image_", "ncw_depth_colormap")


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--chunks", default="1024,4096,16384", help="comma-separated rays per render launch")
    ap.add_argument("--views", type=int, default=3, help="views in the timed window")
    ap.add_argument("--prec", default="f16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view"))
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    import numpy as np
    import torch

    import bench
    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import views

    if not torch.cuda.is_available():
        raise SystemExit("bench_view.py needs a GPU: nothing is timed on a CPU")
    dev = torch.device("cuda", 0)
    prec = {"bf16": nw.PREC_BF16, "f16": nw.PREC_F16, "f32": nw.PREC_F32}[args.prec]
    emb, neuconw, nerf, rdr = bench.build_models(dev, prec)
    W, H = args.width, args.height
    # a camera at (0, 0, -2) looking along +z at the unit sphere ("right up back" axes), 40 degrees across the width: the
    # ray distribution of bench.py's synthetic batch, as an image
    fx = 0.5 * W / np.tan(np.deg2rad(20.0))
    K = [[fx, 0, 0.5 * W - 0.3], [0, fx, 0.5 * H + 0.4], [0, 0, 1]]
    c2w = [[-1, 0, 0, 0.0], [0, 1, 0, 0.0], [0, 0, -1, -2.0]]
    cam = views.Camera(K, c2w, W, H, 1.0, 3.0)
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    S = rdr.n_samples + rdr.n_importance
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "view_%dx%d.jsonl" % (W, H))
    lines = []
    for chunk in [int(c) for c in args.chunks.split(",")]:
        views.render_view(rdr, cam, ts=7, chunk=chunk, gt=gt)  # warm-up: the same shapes as the timed window
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.views):
            out = views.render_view(rdr, cam, ts=7, chunk=chunk, gt=gt)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.views
        L.PROFILE = {}
        try:
            views.render_view(rdr, cam, ts=7, chunk=chunk, gt=gt)
            torch.cuda.synchronize()
            glue = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in L.PROFILE.items() if k.startswith(GLUE)}
        finally:
            L.PROFILE = None
        glue_ms = sum(glue.values())
        line = {"metric": "view_render", "width": W, "height": H, "chunk": chunk, "prec": args.prec, "n_samples": rdr.n_samples,
                "n_importance": rdr.n_importance, "n_outside": rdr.n_outside, "views_timed": args.views,
                "ms_per_view": round(ms, 3), "ray_samples_per_s": round(H * W * S / (ms * 1e-3), 1),
                "glue_ms_per_view": round(glue_ms, 3), "glue_share": round(glue_ms / ms, 5),
                "glue_ms_by_entry": {k: round(v, 3) for k, v in sorted(glue.items())},
                "psnr": float(out["psnr"]), "ssim": float(out["ssim"]), "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    with open(path, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
