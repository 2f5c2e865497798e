"""Times the appearance-code fit on frozen geometry (neuralrecon_w_amd/appfit.py) against what the project offered before it,
on the flagship networks of bench.py: 1024 rays x (64 + 64) + 32 samples, W = 256, fp16 operands.

    python scripts/bench_appfit.py [--rays 1024] [--iters 50] [--repeats 5] [--prec f16] [--out profiles/appfit]
                                   [--parent DIR --rounds 3 --bench_steps 20 --bench_warmup 5]

One JSON line (also written to <out>/appfit_bench.json), every time from HIP events around a window that ends in a
synchronise, after warm runs of the same shapes, medians over --repeats windows measured in ONE call, frozen and composed
windows alternating:
  frozen_ms_per_iter    AppearanceFit.loss_and_grad() + .step(): colour forward, background forward, ncw_appfit_loss, the two
                        data-path backwards, ncw_appfit_step;
  composed_ms_per_iter  one render() (perturb 0) + L1 + backward() with only a one-row embedding requiring a gradient: sampler,
                        SDF forward, second-order SDF backward, compositor backward and every weight-gradient GEMM included --
                        the only way to run this fit without appfit.py;
  ratio                 composed / frozen;
  freeze_ms             the one-off freeze_rays() cost (median of --repeats);
  dead_sample_share     share of the frozen samples with weight == 0 (what a later compaction of dead samples would be judged by).
--parent DIR: a checkout of the parent commit with its library built; bench.py --gpus 1 is then run --rounds times in each
tree, alternating, and the medians of ms_per_step are reported (`default_step`): the default training step must not have moved.
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


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--n_outside", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50, help="iterations per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per path (medians are reported)")
    ap.add_argument("--prec", default="f16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "appfit"))
    ap.add_argument("--parent", default=None, help="checkout of the parent commit (library built) for the bench.py rounds")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench_steps", type=int, default=20)
    ap.add_argument("--bench_warmup", type=int, default=5)
    return ap


def _bench_rounds(parent, rounds, steps, warmup):
    """bench.py --gpus 1 in this tree and in the parent's, alternating; every run a fresh process with its own time limit."""
    ms = {"this": [], "parent": []}
    cmd = ["bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-pmc",
           "--no-parity-mode"]
    for _ in range(rounds):
        for name, tree in (("parent", parent), ("this", ROOT)):
            r = subprocess.run([sys.executable] + cmd, cwd=tree, capture_output=True, text=True, timeout=420)
            if r.returncode != 0:  # nothing more is started on the GPU after a failed run
                raise SystemExit("bench.py failed in %s (exit %d):\n%s" % (tree, r.returncode, (r.stdout + r.stderr)[-2000:]))
            line = [l for l in r.stdout.splitlines() if l.startswith("{") and '"ms_per_step"' in l][-1]
            ms[name].append(json.loads(line)["ms_per_step"])
    return {"rounds": rounds, "steps": steps, "warmup": warmup, "ms_per_step_this": ms["this"], "ms_per_step_parent": ms["parent"],
            "median_this": statistics.median(ms["this"]), "median_parent": statistics.median(ms["parent"]),
            "this_over_parent": statistics.median(ms["this"]) / statistics.median(ms["parent"])}


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch

    import bench
    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import appfit

    if not torch.cuda.is_available():
        raise SystemExit("bench_appfit.py needs a GPU: nothing is timed on a CPU")
    dev = torch.device("cuda", 0)
    prec = {"bf16": nw.PREC_BF16, "f16": nw.PREC_F16, "f32": nw.PREC_F32}[args.prec]
    emb, neuconw, nerf, rdr = bench.build_models(dev, prec)
    rdr.n_outside = args.n_outside
    rdr.sync_free = False
    rdr.mesh_mask_list, rdr.depth_loss = None, False
    R = args.rays
    rays, _, label, rgbs = bench.synth_batch(R, 1000, dev)
    rays = rays[:, :8].contiguous()
    label = torch.zeros_like(label)
    code0 = emb.weight.detach().mean(0)
    n_a = code0.numel()

    def sync_ms(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    # ---- frozen path ----
    def freeze():
        ctx = appfit.freeze_rays(rdr, rays, chunk=R)
        appfit.release_contexts(ctx)

    freeze()  # warm: the same shapes
    freeze_ms = [sync_ms(freeze, 1) for _ in range(args.repeats)]
    ctxs = appfit.freeze_rays(rdr, rays, chunk=R)
    dead = appfit.dead_sample_share(ctxs)
    fit = appfit.AppearanceFit(rdr, ctxs, rgbs, code0, lr=appfit.DEFAULT_LR)

    def frozen_iter():
        fit.loss_and_grad()
        fit.step()

    # ---- composed path: only a one-row embedding requires a gradient ----
    for m in (neuconw, nerf):
        for p in m.parameters():
            p.requires_grad_(False)
    emb1 = torch.nn.Embedding(1, n_a).to(dev)
    with torch.no_grad():
        emb1.weight.copy_(code0.reshape(1, -1))
    rdr_emb = rdr.embeddings
    ts0 = torch.zeros(R, dtype=torch.long, device=dev)
    opt = torch.optim.Adam(emb1.parameters(), lr=appfit.DEFAULT_LR, eps=1e-7)

    def composed_iter():
        rdr.embeddings = {"a": emb1}
        try:
            opt.zero_grad(set_to_none=True)
            out = rdr.render(rays, ts0, label, perturb_overwrite=0)
            loss = (out["color"] - rgbs).abs().sum() / (R + 1e-5)
            loss.backward()
            opt.step()
        finally:
            rdr.embeddings = rdr_emb

    for _ in range(5):  # warm runs of both paths
        frozen_iter()
        composed_iter()
    torch.cuda.synchronize()
    frozen, composed = [], []
    for _ in range(args.repeats):  # alternating windows in one call
        frozen.append(sync_ms(frozen_iter, args.iters))
        composed.append(sync_ms(composed_iter, args.iters))
    f_ms, c_ms = statistics.median(frozen), statistics.median(composed)
    line = {"metric": "appearance_fit_iteration", "rays": R, "n_samples": rdr.n_samples, "n_importance": rdr.n_importance,
            "n_outside": rdr.n_outside, "prec": args.prec, "iters_per_window": args.iters, "windows": args.repeats,
            "frozen_ms_per_iter": round(f_ms, 4), "composed_ms_per_iter": round(c_ms, 4), "ratio": round(c_ms / f_ms, 3),
            "frozen_windows_ms": [round(x, 4) for x in frozen], "composed_windows_ms": [round(x, 4) for x in composed],
            "freeze_ms": round(statistics.median(freeze_ms), 4), "freeze_windows_ms": [round(x, 4) for x in freeze_ms],
            "dead_sample_share": round(dead, 5), "skipped_steps": fit.skipped_steps, "loss_after": float(fit.loss()),
            "device": torch.cuda.get_device_name(0)}
    appfit.release_contexts(ctxs)
    del fit, ctxs
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    if args.parent:
        line["default_step"] = _bench_rounds(os.path.abspath(args.parent), args.rounds, args.bench_steps, args.bench_warmup)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "appfit_bench.json"), "w") as fh:
        fh.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
