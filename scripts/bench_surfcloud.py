"""Times the surface-cloud fusion (neuralrecon_w_amd.surfcloud, csrc/ncw_fuse.hip): the table kernels against a torch composition
on synthetic samples, and the fusion's share of traced views on the flagship networks of bench.py.

    python scripts/bench_surfcloud.py [--views 64 --samples 500000] [--cells 1024,256] [--repeats 7] [--trace_views 16]
        [--width 1024 --height 768] [--out DIR] [--ab_parent DIR]

One JSON line (also written to <out>/surfcloud_bench.json, default profiles/surfcloud/).  One call, HIP events, after a warm-up
pass of each side; medians of --repeats passes, the sides ALTERNATING inside the call.
  synthetic   per cell size 2 / N: --views views of --samples samples on a curved sheet (z = 0.2 sin 3x cos 2y over [-0.8, 0.8]^2,
              every view a random window of it, gradients analytic, colours random), all generated before the clock starts.
              insert_ms_per_view: SurfaceCloud.add from the default capacity, growth included; presized_ms_per_view: the same
              into a table that has its final size (the insert kernel alone); resolve_ms: finish(); table_bytes, growths,
              cells.  torch_ms_per_view / torch_peak_bytes: the SAME table (compared bit for bit: same_table) composed from torch
              ops -- the quantiser in float64 tensor ops, torch.unique + index_add_ on int64 per view, merged into the running
              table per view -- with its peak allocation above the inputs; kernel_peak_bytes: the same measure for the cloud.
  traced      --trace_views views of --width x --height around the networks of bench.py at initialisation (W = 256):
              view_ms / view_fused_ms: trace_view alone and under fuse_views, alternating; split_ms: one further fused pass
              with every C-ABI call bracketed by events (lib.PROFILE), summed per view into SDF values / trace kernels /
              shading / fusion (upper bounds: an interval also holds the host gap between two launches); fusion_share.
--ab_parent DIR: `bench.py --gpus 1 --steps 20 --warmup 5` of the parent commit's built tree in DIR and of this tree as child
processes, alternating, order swapped every round (scripts/bench_trace.py's step_ab).
The weights are at initialisation: NOT a trained scene (not measured).  A GPU is required; nothing here is timed on a CPU.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = {"sdf_value": ("ncw_sdf_infer",), "trace_kernels": ("ncw_trace_", "ncw_view_rays", "ncw_ray_prologue"),
          "shading": ("ncw_sdf_fwd", "ncw_color_", "ncw_aux_ray_bias", "ncw_pack_weights", "ncw_inv_s"), "fusion": ("ncw_fuse_",)}


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--samples", type=int, default=500000)
    ap.add_argument("--cells", default="1024,256", help="cell sizes 2 / N")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--trace_views", type=int, default=16)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--prec", default="f16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--ab_parent", default=None, help="a built checkout of the parent commit: A/B of the default bench.py step")
    ap.add_argument("--ab_rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surfcloud"))
    return ap


def sheet_views(n_views, n, dev):
    """[(points, grads, dirs, colours)] float32 device tensors: a random window of the sheet per view, seen from above."""
    import torch

    g = torch.Generator(device=dev).manual_seed(0)
    out = []
    for _ in range(n_views):
        c = torch.rand(2, device=dev, generator=g) * 0.8 - 0.4
        xy = (torch.rand(n, 2, device=dev, generator=g) - 0.5) * 0.8 + c
        x, y = xy[:, 0], xy[:, 1]
        z = 0.2 * torch.sin(3 * x) * torch.cos(2 * y)
        grad = torch.stack([-0.6 * torch.cos(3 * x) * torch.cos(2 * y), 0.4 * torch.sin(3 * x) * torch.sin(2 * y), torch.ones_like(x)], 1)
        grad = grad * (0.8 + 0.4 * torch.rand(n, 1, device=dev, generator=g))
        eye = torch.cat([c, torch.full((1,), 2.0, device=dev)])
        p = torch.stack([x, y, z], 1)
        d = torch.nn.functional.normalize(p - eye, dim=1)
        out.append(tuple(t.float().contiguous() for t in (p, grad, d, torch.rand(n, 3, device=dev, generator=g))))
    return out


class TorchTable:
    """The fusion's table composed from torch ops: QUANTISE in float64 tensor ops (each rounded on its own), torch.unique +
    index_add_ on int64 per view, merged into the running table per view.  Same bits as the kernels' table."""

    def __init__(self, cloud):
        import torch

        dev = cloud.device
        self.lo = torch.tensor(cloud.lo, device=dev, dtype=torch.float64)
        self.off = torch.tensor(cloud.offset, device=dev, dtype=torch.float64)
        self.dims = torch.tensor(cloud.dims, device=dev, dtype=torch.int64)
        self.h, self.scale, self.cos_min = cloud.cell, cloud.scale, cloud.cos_min
        self.keys = torch.empty(0, device=dev, dtype=torch.int64)
        self.acc = torch.empty(0, 10, device=dev, dtype=torch.int64)
        self.views = torch.empty(0, device=dev, dtype=torch.int32)

    def add(self, p, n, d, c):
        import torch

        x = p.double() * self.scale + self.off
        g = (x - self.lo) / self.h
        cf = torch.floor(g)
        ok = torch.isfinite(p).all(1) & torch.isfinite(n).all(1) & torch.isfinite(d).all(1)
        ok &= ((cf >= 0) & (cf < self.dims.double())).all(1)
        n64, d64 = n.double(), d.double()
        nn = (n64[:, 0] * n64[:, 0] + n64[:, 1] * n64[:, 1]) + n64[:, 2] * n64[:, 2]
        ok &= torch.isfinite(nn) & (nn > 0)
        ln = torch.sqrt(nn)
        if self.cos_min is not None:
            ok &= -((n64[:, 0] * d64[:, 0] + n64[:, 1] * d64[:, 1]) + n64[:, 2] * d64[:, 2]) >= self.cos_min * ln
        cell = cf[ok].long()
        keys = (cell[:, 2] * self.dims[1] + cell[:, 1]) * self.dims[0] + cell[:, 0]
        c64 = c.double()[ok]
        c64 = torch.where(c64 > 0, c64, torch.zeros_like(c64))
        c64 = torch.where(c64 < 1, c64, torch.ones_like(c64))
        pay = torch.cat([torch.ones(keys.numel(), 1, device=p.device, dtype=torch.int64),
                         torch.floor((g - cf)[ok] * 65536.0).clamp(max=65535.0).long(),
                         torch.round(n64[ok] / ln[ok, None] * 32767.0).long(), torch.round(c64 * 255.0).long()], 1)
        uk, inv = torch.unique(keys, return_inverse=True)
        acc = torch.zeros(uk.numel(), 10, device=p.device, dtype=torch.int64).index_add_(0, inv, pay)
        mk, minv = torch.unique(torch.cat([self.keys, uk]), return_inverse=True)
        macc = torch.zeros(mk.numel(), 10, device=p.device, dtype=torch.int64)
        macc.index_add_(0, minv, torch.cat([self.acc, acc]))
        mviews = torch.zeros(mk.numel(), device=p.device, dtype=torch.int32)
        mviews.index_add_(0, minv, torch.cat([self.views, torch.ones(uk.numel(), device=p.device, dtype=torch.int32)]))
        self.keys, self.acc, self.views = mk, macc, mviews


def _events():
    import torch

    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def synthetic(args, dev):
    import torch

    from neuralrecon_w_amd import surfcloud

    data = sheet_views(args.views, args.samples, dev)
    res = {}
    for N in [int(v) for v in args.cells.split(",")]:
        def cloud_of(capacity=surfcloud.DEFAULT_CAPACITY):
            return surfcloud.SurfaceCloud(-1.0, 1.0, 2.0 / N, cos_min=0.1, device=dev, capacity=capacity)

        def kernel_pass(capacity=surfcloud.DEFAULT_CAPACITY):
            cloud = cloud_of(capacity)
            e0, e1 = _events()
            e0.record()
            for v, s in enumerate(data):
                cloud.add(*s, v)
            e1.record()
            r0, r1 = _events()
            r0.record()
            out = cloud.finish()
            r1.record()
            torch.cuda.synchronize()
            return cloud, out, e0.elapsed_time(e1) / len(data), r0.elapsed_time(r1)

        def torch_pass():
            tab = TorchTable(cloud_of())
            e0, e1 = _events()
            e0.record()
            for s in data:
                tab.add(*s)
            e1.record()
            torch.cuda.synchronize()
            return tab, e0.elapsed_time(e1) / len(data)

        cloud, out, _, _ = kernel_pass()  # warm-up, and the table the composition must reproduce
        final_capacity = cloud.stats()["capacity"]
        kernel_pass(final_capacity)
        tab, _ = torch_pass()
        t = cloud.table()
        same = bool(torch.equal(t["keys"], tab.keys) and torch.equal(t["acc"], tab.acc) and torch.equal(t["views"], tab.views))
        if not same:
            print("WARNING: the torch composition's table differs from the kernels' at cell 2/%d" % N, file=sys.stderr)
        stats = cloud.stats()
        del cloud, tab, t
        k_ms, p_ms, r_ms, t_ms = [], [], [], []
        for _ in range(args.repeats):
            _, _, a, r = kernel_pass()
            _, _, b, _ = kernel_pass(final_capacity)
            _, c = torch_pass()
            k_ms.append(a), r_ms.append(r), p_ms.append(b), t_ms.append(c)
        peak = {}
        for name, fn in (("kernel", kernel_pass), ("torch", torch_pass)):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            keep = fn()
            torch.cuda.synchronize()
            peak[name] = int(torch.cuda.max_memory_allocated() - base)
            del keep
        res["2/%d" % N] = {"cell": 2.0 / N, "insert_ms_per_view": round(statistics.median(k_ms), 4),
                           "insert_ms_per_view_all": [round(v, 4) for v in k_ms],
                           "presized_ms_per_view": round(statistics.median(p_ms), 4),
                           "presized_ms_per_view_all": [round(v, 4) for v in p_ms],
                           "resolve_ms": round(statistics.median(r_ms), 4), "torch_ms_per_view": round(statistics.median(t_ms), 4),
                           "torch_ms_per_view_all": [round(v, 4) for v in t_ms], "same_table": same,
                           "table_bytes": stats["table_bytes"], "capacity": stats["capacity"], "growths": stats["growths"],
                           "cells": stats["cells"], "valid": stats["valid"], "offered": stats["offered"],
                           "cells_resolved": int(out["keys"].numel()), "kernel_peak_bytes": peak["kernel"],
                           "torch_peak_bytes": peak["torch"]}
    return res


def traced(args, dev):
    import numpy as np
    import torch

    import bench
    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import surfcloud, views

    prec = {"bf16": nw.PREC_BF16, "f16": nw.PREC_F16, "f32": nw.PREC_F32}[args.prec]
    emb, neuconw, nerf, rdr = bench.build_models(dev, prec)
    W, H = args.width, args.height
    fx = 0.5 * W / np.tan(np.deg2rad(20.0))  # scripts/bench_view.py's camera, on a circle around the origin
    K = [[fx, 0, 0.5 * W - 0.3], [0, fx, 0.5 * H + 0.4], [0, 0, 1]]
    cams = []
    for i in range(args.trace_views):
        a = 2 * np.pi * i / args.trace_views
        back = np.array([np.sin(a), 0.0, np.cos(a)])
        right = np.cross([0.0, 1.0, 0.0], back)
        cams.append((views.Camera(K, np.stack([right, np.cross(back, right), back, 2.0 * back], 1), W, H, 1.0, 3.0), 7))
    a_code = surfcloud.mean_appearance(rdr)

    def plain():
        for cam, ts in cams:
            views.trace_view(rdr, cam, ts, a_code=a_code)

    def fused():
        cloud = surfcloud.SurfaceCloud(-1.0, 1.0, 2.0 / 1024, cos_min=0.1, device=dev)
        tot = surfcloud.fuse_views(rdr, cams, cloud)
        return cloud, tot

    def timed(fn):
        e0, e1 = _events()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / len(cams), out

    plain(), fused()
    torch.cuda.synchronize()
    p_ms, f_ms = [], []
    for _ in range(args.repeats):
        p_ms.append(timed(plain)[0])
        ms, (cloud, tot) = timed(fused)
        f_ms.append(ms)
    L.PROFILE = {}
    try:
        fused()
        torch.cuda.synchronize()
        prof = {k: sum(a.elapsed_time(b) for a, b in v) / len(cams) for k, v in L.PROFILE.items()}
    finally:
        L.PROFILE = None
    split = {g: round(sum(v for k, v in prof.items() if k.startswith(pre)), 4) for g, pre in GROUPS.items()}
    split["other"] = round(sum(prof.values()) - sum(split.values()), 4)
    out = cloud.finish(min_views=2)
    st = cloud.stats()
    return {"views": len(cams), "width": W, "height": H, "prec": args.prec, "view_ms": round(statistics.median(p_ms), 3),
            "view_ms_all": [round(v, 3) for v in p_ms], "view_fused_ms": round(statistics.median(f_ms), 3),
            "view_fused_ms_all": [round(v, 3) for v in f_ms], "split_ms_per_view": split,
            "fusion_share": round(split["fusion"] / max(1e-9, sum(split.values())), 5),
            "rays": tot["rays"], "hit": tot["hit"], "samples_valid": st["valid"], "cells": st["cells"],
            "cells_min_views_2": int(out["keys"].numel()), "growths": st["growths"], "table_bytes": st["table_bytes"],
            "weights": "initialisation, no fine octree: not a trained scene"}


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_surfcloud.py needs a GPU: nothing is timed on a CPU")
    dev = torch.device("cuda", 0)
    line = {"metric": "surfcloud", "views": args.views, "samples_per_view": args.samples, "repeats": args.repeats,
            "device": torch.cuda.get_device_name(0)}
    line["synthetic"] = synthetic(args, dev)
    torch.cuda.empty_cache()
    if args.trace_views > 0:
        line["traced"] = traced(args, dev)
        torch.cuda.empty_cache()
    if args.ab_parent:
        from bench_trace import step_ab  # the same A/B every profile of this repository records

        line["step_ab"] = {"metric": "bench.py --gpus 1 --steps 20 --warmup 5, ms_per_step, parent commit and this tree alternating, "
                                     "order swapped every round", "ms_per_step": step_ab(os.path.abspath(args.ab_parent), args.ab_rounds)}
    print(json.dumps(line), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "surfcloud_bench.json"), "w") as fh:
        fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
