"""Times surface views by sphere tracing (neuralrecon_w_amd.views.trace_view) against the volume render (views.render_view) on
the flagship networks of bench.py: one 1024 x 768 view at W = 256, the camera and networks of scripts/bench_view.py.

    python scripts/bench_trace.py [--width 1024 --height 768] [--repeats 7] [--prec f16] [--out DIR] [--ab_parent DIR]

One JSON line (also written to <out>/trace_<W>x<H>.json, default profiles/trace/):
  trace_ms / render_ms   medians of --repeats whole views each, HIP events, trace_view and render_view ALTERNATING in this call
                         after a warm-up view of each; ratio = render_ms / trace_ms;
  split_ms               one further trace_view with every C-ABI call bracketed by events (lib.PROFILE): SDF value launches
                         (ncw_sdf_infer), trace kernels (ncw_trace_* + ncw_view_rays + ncw_ray_prologue), shading (ncw_sdf_fwd +
                         ncw_color_fwd + ...).  UPPER BOUNDS: an interval also holds the host gap between two launches;
  active_curve           rays still active in front of every SDF launch (whole view in one call, sync_every 1); sdf_points
                         their sum, against `rays`;
  sync_every_ms / chunk_ms   medians of 3 views per setting; shade_f16_ms: the forward at the hits in fp16 instead of the fp32
                         default of the inference entry points; no_shade_ms: shade=False (depth / state only);
  states                 pixels per state, mean / max evaluations per ray.
--ab_parent DIR: also runs `bench.py --gpus 1 --steps 20 --warmup 5` (timing leg only) of the tree in DIR -- the parent commit,
built -- and of this tree as child processes, alternating and swapping the order every round: `step_ab`.
The weights are at initialisation (a sphere): NOT the iteration counts of a trained facade, and no fine octree.
A GPU is required; nothing here is timed on a CPU.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = {"sdf_value": ("ncw_sdf_infer",), "trace_kernels": ("ncw_trace_", "ncw_view_rays", "ncw_ray_prologue"),
          "shading": ("ncw_sdf_fwd", "ncw_color_", "ncw_aux_ray_bias", "ncw_pack_weights", "ncw_inv_s")}


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--repeats", type=int, default=7, help="views per side of the alternating comparison (medians)")
    ap.add_argument("--prec", default="f16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--sync_every", default="1,4,16")
    ap.add_argument("--chunks", default="16384,65536,131072,786432")
    ap.add_argument("--ab_parent", default=None, help="a built checkout of the parent commit: A/B of the default bench.py step")
    ap.add_argument("--ab_rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace"))
    return ap


def _timed(fn, n):
    import torch

    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms, out


def step_ab(parent, rounds):
    """ms_per_step of `bench.py --gpus 1 --steps 20 --warmup 5` (no CPU baseline, no PMC passes, no parity legs: the timed loop
    is the default run's) for the parent tree and this one, one child process each, order swapped every round."""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-pmc",
           "--no-parity-mode"]
    res = {"parent": [], "new": []}
    for r in range(rounds):
        for side in (("new", "parent") if r % 2 else ("parent", "new")):
            p = subprocess.run(cmd, cwd=parent if side == "parent" else ROOT, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("bench.py failed in %s:\n%s" % (side, p.stderr[-2000:]))
            res[side].append(json.loads(p.stdout.strip().splitlines()[-1])["ms_per_step"])
    return res


def main(argv=None):
    args = build_parser().parse_args(argv)
    import numpy as np
    import torch

    import bench
    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import trace, views

    if not torch.cuda.is_available():
        raise SystemExit("bench_trace.py needs a GPU: nothing is timed on a CPU")
    dev = torch.device("cuda", 0)
    prec = {"bf16": nw.PREC_BF16, "f16": nw.PREC_F16, "f32": nw.PREC_F32}[args.prec]
    emb, neuconw, nerf, rdr = bench.build_models(dev, prec)
    W, H = args.width, args.height
    fx = 0.5 * W / np.tan(np.deg2rad(20.0))  # scripts/bench_view.py's camera
    K = [[fx, 0, 0.5 * W - 0.3], [0, fx, 0.5 * H + 0.4], [0, 0, 1]]
    c2w = [[-1, 0, 0, 0.0], [0, 1, 0, 0.0], [0, 0, -1, -2.0]]
    cam = views.Camera(K, c2w, W, H, 1.0, 3.0)
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)

    def tv(**kw):
        return views.trace_view(rdr, cam, ts=7, gt=gt, **kw)

    def rv():
        return views.render_view(rdr, cam, ts=7, gt=gt)

    tv(), rv()  # warm-up: packing, allocator, the same shapes as the timed views
    torch.cuda.synchronize()
    t_ms, r_ms = [], []
    for _ in range(args.repeats):
        a, out = _timed(tv, 1)
        b, _ = _timed(rv, 1)
        t_ms += a
        r_ms += b
    L.PROFILE = {}
    try:
        tv()
        torch.cuda.synchronize()
        prof = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in L.PROFILE.items()}
        calls = {k: len(v) for k, v in L.PROFILE.items()}
    finally:
        L.PROFILE = None
    split = {g: round(sum(v for k, v in prof.items() if k.startswith(pre)), 3) for g, pre in GROUPS.items()}
    split["other"] = round(sum(prof.values()) - sum(split.values()), 3)
    rays = views.view_rays(cam)
    curve = trace.trace_rays(rdr, rays, sync_every=1)
    sync_ms = {s: round(statistics.median(_timed(lambda s=s: tv(sync_every=int(s)), 3)[0]), 3) for s in args.sync_every.split(",")}
    chunk_ms = {}
    for c in args.chunks.split(","):
        tv(chunk=int(c))
        chunk_ms[c] = round(statistics.median(_timed(lambda c=c: tv(chunk=int(c)), 3)[0]), 3)
    tv(shade_prec=nw.PREC_F16)
    shade16 = round(statistics.median(_timed(lambda: tv(shade_prec=nw.PREC_F16), 3)[0]), 3)
    noshade = round(statistics.median(_timed(lambda: tv(shade=False), 3)[0]), 3)
    s = out["stats"]
    line = {"metric": "view_trace", "width": W, "height": H, "prec": args.prec, "rays": H * W, "eps": 1e-3, "max_iter": 64, "step": 1.0,
            "chunk": views.TRACE_CHUNK, "sync_every": 4, "repeats": args.repeats,
            "trace_ms": round(statistics.median(t_ms), 3), "trace_ms_all": [round(v, 3) for v in t_ms],
            "render_ms": round(statistics.median(r_ms), 3), "render_ms_all": [round(v, 3) for v in r_ms],
            "ratio_render_over_trace": round(statistics.median(r_ms) / statistics.median(t_ms), 2),
            "split_ms": split, "split_calls": {k: calls[k] for k in sorted(calls)},
            "active_curve": curve["active"], "sdf_points": curve["evaluated"], "sdf_points_per_ray": round(curve["evaluated"] / (H * W), 3),
            "sync_every_ms": sync_ms, "chunk_ms": chunk_ms, "shade_f16_ms": shade16, "no_shade_ms": noshade, "states": s,
            "psnr": float(out["psnr"]), "psnr_hit": float(out["psnr_hit"]), "weights": "initialisation (a sphere), no fine octree",
            "device": torch.cuda.get_device_name(0)}
    if args.ab_parent:
        del emb, neuconw, nerf, rdr
        torch.cuda.empty_cache()
        line["step_ab"] = {"metric": "bench.py --gpus 1 --steps 20 --warmup 5, ms_per_step, parent commit and this tree alternating, "
                                     "order swapped every round", "ms_per_step": step_ab(os.path.abspath(args.ab_parent), args.ab_rounds)}
    print(json.dumps(line), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "trace_%dx%d.json" % (W, H)), "w") as fh:
        fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
