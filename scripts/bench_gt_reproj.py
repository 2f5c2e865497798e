"""Times the nearest-on-pixel pass of the alignment check (neuralrecon_w_amd.gtreproj, csrc/ncw_gtreproj.hip) on a seeded
synthetic scene built on the device: --points cloud points in a box, --queries views of --width x --height on a shell around it,
each with the key-point where one of the cloud's points projects (so every query is hit).

    python scripts/bench_gt_reproj.py [--points 20000000 --queries 4096 --width 1024 --height 768] [--reps 5] [--out profiles/gtreproj]

One JSON line (also written to <out>/gtreproj_<points>x<queries>.json), everything in one call, warm, device events, medians:
  fused_ms, fused_per_query_ms    ONE `ncw_pixel_nearest` launch over all queries (cloud and query table on the device);
  pairs_per_s                     points x queries / fused time;
  composed_per_query_ms           the same result composed in torch the way reproj_error.py:21-51 does it, two queries at a time
                                  over [2, points, 4] tensors, on the first --composed-queries queries; reported PER QUERY and
                                  not extrapolated to a total;
  same_points                     both paths choose the same point on those queries (`n_same` of `composed_queries`);
  roofline                        lane operations per pair counted from the kernel's inner loop (LANE_OPS below), their rate, and
                                  its share of the float32 vector peak.  The contract forbids contraction, so a product and its
                                  sum are two instructions: the ceiling of this kernel is the vector ISSUE rate (one lane
                                  operation per lane and clock), half the FMA peak.  Memory traffic is 12 bytes per point per
                                  launch whatever the number of queries.
A GPU is required; nothing here is timed on a CPU.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the inner loop of pixel_nearest_kernel per (point, query) pair, as compiled (one instruction each, none fused):
#   c_0, c_1, c_2: 3 x (3 products + 3 sums) = 18;  the two numerators: 2 x (2 products + 1 sum) = 6;
#   the bound: X c_2, Y c_2, two differences, two half-widths x c_2 = 6, two compares = 2;
#   the range of c_2: one integer add, one integer compare, one float compare = 3
LANE_OPS = {"float_mul_add": 30, "float_compare": 3, "integer": 2}
PEAK_FP32_VECTOR_TFLOPS = 157.3  # MI355X: 256 CUs x 4 SIMDs x 32 lanes x 2 (an FMA counts twice) x 2.4 GHz


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--composed-queries", type=int, default=64)
    ap.add_argument("--composed-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gtreproj"))
    return ap


def make_queries(nq, W, H, seed=0):
    """World -> camera matrices float64 [nq,3,4] of cameras on a shell of radius 3 .. 4 about the origin that look at points near
    it, and their intrinsics [nq,4]."""
    import numpy as np

    rs = np.random.RandomState(seed)
    f = 0.5 * W / np.tan(np.deg2rad(25.0))
    w2c = np.zeros((nq, 3, 4))
    for q in range(nq):
        u = rs.normal(size=3)
        pos = u / np.linalg.norm(u) * rs.uniform(3.0, 4.0)
        z = rs.uniform(-0.3, 0.3, 3) - pos
        z /= np.linalg.norm(z)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        w2c[q, :, :3], w2c[q, :, 3] = R, -R @ pos
    intr = np.tile(np.array([f, f, 0.5 * W, 0.5 * H]), (nq, 1))
    return w2c, intr


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def composed_pair(pcd_h, w4, k3, xy):
    """reproj_error.py:30-49 for one batch of queries, op for op, with the world -> camera matrices given (the reference inverts
    the camera poses first).  Returns the chosen index per query, -1 where nothing hits (the reference has no such answer)."""
    import torch

    in_cam = w4 @ pcd_h.transpose(0, 1)
    in_cam[:, 0] /= in_cam[:, 3]
    in_cam[:, 1] /= in_cam[:, 3]
    in_cam[:, 2] /= in_cam[:, 3]
    in_cam = in_cam[:, :3, :]
    proj = torch.bmm(k3, in_cam).permute(0, 2, 1)
    proj[:, :, 0] /= proj[:, :, 2]
    proj[:, :, 1] /= proj[:, :, 2]
    mask = torch.round(proj[:, :, :2]) == torch.round(xy.unsqueeze(1))
    mask = mask[:, :, 0] * mask[:, :, 1] * (proj[:, :, 2] >= 0)
    any_hit = mask.any(dim=1)
    far = torch.max(proj[mask][:, 2]) + 10 if bool(mask.any()) else 0.0
    proj[~mask] = far
    idx = torch.argmin(proj[:, :, 2], dim=1)
    return torch.where(any_hit, idx, torch.full_like(idx, -1))


def main(argv=None):
    args = build_parser().parse_args(argv)
    import numpy as np
    import torch

    from neuralrecon_w_amd import gtreproj as G
    from neuralrecon_w_amd import lib as L

    if not torch.cuda.is_available():
        raise SystemExit("bench_gt_reproj.py needs a GPU: nothing is timed on a CPU")
    dev = torch.device("cuda", 0)
    n, nq, W, H = args.points, args.queries, args.width, args.height
    gen = torch.Generator(device=dev).manual_seed(0)
    pts = (torch.rand(n, 3, device=dev, generator=gen) * 2 - 1) * torch.tensor([1.0, 0.8, 0.6], device=dev)
    w2c, intr = make_queries(nq, W, H)
    # the key-point of query q: where cloud point (q * 7919) % n projects, if inside the image; else the image centre
    pick = (torch.arange(nq, device=dev) * 7919) % n
    w_d = torch.from_numpy(w2c).to(dev)
    c = torch.einsum("qij,qj->qi", w_d[:, :, :3], pts[pick].double()) + w_d[:, :, 3]
    xy = torch.stack([intr[0, 0] * c[:, 0] / c[:, 2] + intr[0, 2], intr[0, 1] * c[:, 1] / c[:, 2] + intr[0, 3]], -1)
    inside = (xy[:, 0] > 0) & (xy[:, 0] < W - 1) & (xy[:, 1] > 0) & (xy[:, 1] < H - 1)
    xy = torch.where(inside[:, None], xy, torch.tensor([0.5 * W, 0.5 * H], device=dev, dtype=torch.float64)).cpu().numpy()
    table = G.query_table(w2c, intr, xy, np.zeros(3))
    q_d = torch.frombuffer(bytearray(table.tobytes()), dtype=torch.uint8).to(dev)
    best = torch.empty(nq, device=dev, dtype=torch.int64)
    lib = L.get_lib()

    def fused():
        L.check(lib.ncw_pixel_nearest(L.ptr(q_d), nq, L.ptr(pts), 0, n, 1, L.ptr(best), L.stream_ptr(dev)), "ncw_pixel_nearest")

    nc = min(args.composed_queries, nq) // 2 * 2
    pcd_h = torch.cat([pts, torch.ones(n, 1, device=dev)], -1)
    w4 = torch.zeros(nq, 4, 4, device=dev)
    w4[:, :3, :] = torch.from_numpy(table["w2c"].reshape(-1, 3, 4)).to(dev)
    w4[:, 3, 3] = 1
    k3 = torch.zeros(nq, 3, 3, device=dev)
    k3[:, 0, 0], k3[:, 1, 1], k3[:, 0, 2], k3[:, 1, 2], k3[:, 2, 2] = [torch.from_numpy(table["intr"][:, i].copy()).to(dev) for i in (0, 1, 2, 3)] + [1.0]
    xy_d = torch.from_numpy(table["xy"].copy()).to(dev)
    comp_idx = torch.empty(nc, device=dev, dtype=torch.int64)

    def composed():
        for a in range(0, nc, 2):
            comp_idx[a:a + 2] = composed_pair(pcd_h, w4[a:a + 2], k3[a:a + 2], xy_d[a:a + 2])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    fused()
    composed()  # warm
    torch.cuda.synchronize()
    t_f, t_c = [], []
    for r in range(max(args.reps, args.composed_reps)):  # alternate: other work shares the machine
        if r < args.reps:
            t_f.append(timed(fused))
        if r < args.composed_reps:
            t_c.append(timed(composed))
    fused()
    torch.cuda.synchronize()
    idx, _ = G.split_keys(best.cpu().numpy().view(np.uint64))
    ci = comp_idx.cpu().numpy()
    fused_ms, comp_ms = median(t_f), median(t_c)
    pairs = float(n) * nq
    lane_ops = sum(LANE_OPS.values())
    rate = pairs / (fused_ms * 1e-3)
    line = {"metric": "gt_reproj_pixel_nearest", "points": n, "queries": nq, "width": W, "height": H, "reps": args.reps,
            "fused_ms": round(fused_ms, 3), "fused_per_query_ms": round(fused_ms / nq, 6), "pairs_per_s": float("%.4g" % rate),
            "composed_queries": nc, "composed_ms_for_those": round(comp_ms, 2), "composed_per_query_ms": round(comp_ms / nc, 3),
            "per_query_ratio": round((comp_ms / nc) / (fused_ms / nq), 1), "fused_faster_per_query": bool(fused_ms / nq < comp_ms / nc),
            "rounds_ms": {"fused": [round(x, 3) for x in t_f], "composed": [round(x, 2) for x in t_c]},
            "n_same": int((idx[:nc] == ci).sum()), "same_points": bool(np.array_equal(idx[:nc], ci)), "queries_hit": int((idx >= 0).sum()),
            "roofline": {"lane_ops_per_pair": LANE_OPS, "lane_ops_per_s": float("%.4g" % (rate * lane_ops)),
                         "share_of_fp32_vector_peak": round(rate * lane_ops / (PEAK_FP32_VECTOR_TFLOPS * 1e12), 4),
                         "share_of_vector_issue_rate": round(rate * lane_ops / (PEAK_FP32_VECTOR_TFLOPS * 0.5e12), 4),
                         "bytes_per_launch": 12 * n + 72 * nq, "bound": "vector issue (separately rounded products and sums: no FMA)"},
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "gtreproj_%dx%d.json" % (n, nq)), "w") as fh:
        fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
