"""Times the per-view depth / normal comparison (neuralrecon_w_amd.depthmetrics, csrc/ncw_depthmetrics.hip) on one 1024 x 768 view.

    python scripts/bench_depth_eval.py [--size 1024x768] [--repeat 7] [--no_trace] [--out profiles/depthmetrics/depth_eval_1024x768.json]

All in one call, warm, device events, medians over --repeat, alternating:
  * the fused launch (ViewScorer.score: memset of the histogram words + kernel + fold) in both modes, with and without the three
    optional planes, beside the SAME numbers composed from torch ops (masks, float64 sums, torch.bucketize + bincount), with the
    distance between the two results and whether two runs of each agree bit for bit;
  * a traced view of the same size (views.trace_view, a W = 256 network at its geometric initialisation, shade on) and the
    comparison of ITS planes, both in the same alternating rounds, and the share of the view that the comparison costs.
The planes: a synthetic depth field with holes, a prediction 0..3 % off with other holes, unit normals a few degrees apart, a mask
over 5 % of the pixels.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import depthmetrics as DM  # noqa: E402
from neuralrecon_w_amd import lib as L  # noqa: E402
from neuralrecon_w_amd import views  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def planes(H, W, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    y, x = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    zg = 3.0 + 0.8 * torch.sin(3 * x) * torch.cos(2 * y) + 0.3 * x
    zp = zg * (1.0 + 0.03 * (r(H, W) - 0.3))
    zg = torch.where(r(H, W) < 0.08, torch.zeros(()), zg)
    zp = torch.where(r(H, W) < 0.06, torch.zeros(()), zp)
    gn = torch.nn.functional.normalize(torch.stack([-2.4 * torch.cos(3 * x) * torch.cos(2 * y) - 0.3, 1.6 * torch.sin(3 * x) * torch.sin(2 * y),
                                                    -torch.ones(H, W)], 0), dim=0)
    pn = torch.nn.functional.normalize(gn + 0.08 * (r(3, H, W) - 0.5), dim=0)
    mask = (r(H, W) < 0.05).to(torch.uint8)
    return [t.to(dev).contiguous() for t in (zg.float(), zp.float(), gn.float(), pn.float(), mask)]


def torch_compare(zg, zp, gn, pn, mask, cos_edges, rel_edges, thr):
    """The row's numbers composed from torch ops (float32 terms, float64 sums in torch's order; mode z)."""
    live = mask == 0
    vg, vp = torch.isfinite(zg) & (zg > 0), torch.isfinite(zp) & (zp > 0)
    both = live & vg & vp
    counts = [both.sum(), (live & vg & ~vp).sum(), (live & ~vg & vp).sum(), (live & ~vg & ~vp).sum(), (~live).sum()]
    g, p = zg[both], zp[both]
    e = p - g
    a = e.abs()
    r = a / g
    q = torch.maximum(p / g, g / p)
    ee = e * e
    sums = [a.double().sum(), e.double().sum(), ee.double().sum(), r.double().sum(), (ee / g).double().sum()]
    counts += [(q < t).sum() for t in thr["delta"]]
    hist_rel = torch.bincount(torch.bucketize(r, rel_edges, right=True), minlength=rel_edges.numel() + 1)
    gb, pb = gn[:, both], pn[:, both]
    ok = torch.isfinite(gb).all(0) & torch.isfinite(pb).all(0) & (gb != 0).any(0) & (pb != 0).any(0)
    c = ((gb[0] * pb[0] + gb[1] * pb[1]) + gb[2] * pb[2]).clamp(-1.0, 1.0)[ok]
    sums.append(c.double().sum())
    counts += [ok.sum()] + [(c >= t).sum() for t in thr["cos"]]
    hist_cos = torch.bincount(torch.bucketize(-c, -cos_edges, right=False), minlength=cos_edges.numel() + 1)
    return torch.stack(sums), torch.stack(counts), hist_rel, hist_cos


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1024x768", help="WxH")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--no_trace", action="store_true", help="skip the traced view")
    ap.add_argument("--out", default=os.path.join("profiles", "depthmetrics", "depth_eval_1024x768.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise L.NeuconwHipError("bench_depth_eval needs a GPU: nothing here is measured on the CPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    W, H = [int(v) for v in args.size.lower().split("x")]
    zg, zp, gn, pn, mask = planes(H, W, dev)
    sc = DM.ViewScorer(1, 0.1, None, dev)
    thr = {k: [torch.tensor(float(v), device=dev) for v in sc.thr[k]] for k in ("delta", "cos")}
    cam = views.Camera([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1]], np.eye(4)[:3], W, H, 0.5, 8.0)
    enc = (pn / 2 + 0.5).contiguous()
    res = {"what": "per-view depth / normal comparison: fused launch beside torch ops", "width": W, "height": H, "repeat": args.repeat,
           "device": torch.cuda.get_device_name(dev), "angle_edges": sc.na, "rel_edges": sc.nr,
           "blocks": (H * W + L.DM_BLOCK - 1) // L.DM_BLOCK}

    runs = {"fused_z": lambda: sc.score(0, zg, zp, gt_n=gn, pred_n=pn, mask=mask),
            "fused_z_planes": lambda: sc.score(0, zg, zp, gt_n=gn, pred_n=pn, mask=mask, want_planes=True),
            "fused_z_depth_only": lambda: sc.score(0, zg, zp, mask=mask),
            "fused_t": lambda: sc.score(0, zg, zp, gt_n=gn, pred_n=enc, mask=mask, mode="t", camera=cam, scale=1.0),
            "torch_z": lambda: torch_compare(zg, zp, gn, pn, mask, sc.cos_edges, sc.rel_edges, thr)}
    if not args.no_trace:
        import bench  # the flagship models (W = 256) at their initialisation, as scripts/bench_trace.py traces them
        import neuralrecon_w_amd as nw

        _, _, _, rdr = bench.build_models(dev, nw.PREC_F16)
        fx = 0.5 * W / np.tan(np.deg2rad(20.0))  # scripts/bench_trace.py's camera
        tcam = views.Camera([[fx, 0, 0.5 * W - 0.3], [0, fx, 0.5 * H + 0.4], [0, 0, 1]], [[-1, 0, 0, 0.0], [0, 1, 0, 0.0], [0, 0, -1, -2.0]],
                            W, H, 1.0, 3.0)
        out = views.trace_view(rdr, tcam, ts=7)
        tz, tn = out["depth"], out["normal"]
        res["trace_view_hit_share"] = out["stats"]["hit"] / float(H * W)
        # both join the alternating rounds below: the traced view and the comparison of ITS planes (mode t, the renderer's radius)
        runs["trace_view"] = lambda: views.trace_view(rdr, tcam, ts=7)
        runs["fused_traced"] = lambda: sc.score(0, zg, tz, gt_n=gn, pred_n=tn, mask=mask, mode="t", camera=tcam, scale=float(rdr.radius))
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(args.repeat):
        for k, fn in runs.items():  # alternating
            ms[k].append(timed(fn)[0])
    res["ms"] = {k: float(np.median(v)) for k, v in ms.items()}
    res["min_max_ms"] = {k: [min(v), max(v)] for k, v in ms.items()}
    res["torch_over_fused"] = res["ms"]["torch_z"] / res["ms"]["fused_z"]
    res["torch_over_fused_of_minima"] = min(ms["torch_z"]) / min(ms["fused_z"])
    if "trace_view" in ms:
        res["comparison_share_of_traced_view"] = res["ms"]["fused_traced"] / res["ms"]["trace_view"]
    res["fused_outside_torch_spread"] = bool(max(ms["fused_z"]) < min(ms["torch_z"]))
    # bytes the fused launch has to read: 2 depth planes, 6 normal planes, the mask
    res["bytes_read"] = H * W * (8 * 4 + 1)
    res["fused_z_GBps"] = res["bytes_read"] / (res["ms"]["fused_z"] * 1e-3) / 1e9

    runs["fused_z"]()
    t1 = sc.table.clone()
    runs["fused_z"]()
    res["fused_two_runs_bit_equal"] = bool(torch.equal(t1, sc.table))
    row = sc.rows()[0]
    s1, c1, hr1, hc1 = runs["torch_z"]()
    s2, c2, _, _ = runs["torch_z"]()
    res["torch_two_runs_bit_equal"] = bool(torch.equal(s1, s2))
    fs = np.array([row[k] for k in DM.ROW_SUMS])
    res["max_rel_difference_of_sums"] = float(np.max(np.abs(fs - s1.cpu().numpy()) / np.maximum(np.abs(fs), 1e-300)))
    res["counts_equal"] = bool([row[k] for k in DM.ROW_COUNTS] == c1.cpu().tolist())
    res["hists_equal"] = bool(np.array_equal(row["hist_rel"], hr1.cpu().numpy()) and np.array_equal(row["hist_cos"], hc1.cpu().numpy()))
    res["scores"] = {k: v for k, v in DM.summarise([row])["pooled"].items() if k in ("abs_rel", "rmse", "delta1", "completeness",
                                                                                      "mean_angle", "median_angle")}

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
