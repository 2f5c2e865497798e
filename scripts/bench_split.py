"""Times the view selection of the split writer (neuralrecon_w_amd.sceneprep) on a synthetic scene built in memory: --views
cameras of --width x --height on a shell around the scene sphere, looking at points scattered about it, so that ROI shares
spread from 0 to 1.

    python scripts/bench_split.py [--views 1500 --width 1024 --height 768] [--reps 7] [--composed-reps 3] [--out profiles/split]

One JSON line (also written to <out>/split_<views>x<W>x<H>.json):
  fused_ms             device events around ONE `ncw_views_roi` launch for all views (camera table and prefix already on the
                       device, no mask), warm, median of --reps; rounds alternate with the composed path;
  fused_upload_ms      the same window around sceneprep.roi_shares as the tool calls it: building and uploading the table, the
                       launch, the counts copied back (wall clock, median);
  composed_ms          the same shares composed PER IMAGE from what existed before: views.view_rays + the predicate written
                       term by term in torch (what dataset_filter_utils.py:171-178 does), the count kept on the device -- NOT
                       the reference's path, which also decodes every image and builds the directions on the host; warm,
                       median of --composed-reps;
  counts_equal         fused counts == composed counts for every view (`max_count_diff` otherwise: the two round differently
                       only on pixels that graze the sphere);
  host                 the host part of the tool for the same scene written to a temporary directory: --views image files
                       opened for their header (PIL), --views compressed label maps loaded and counted (numpy).
A GPU is required; nothing here is timed on a CPU.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=1500)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--composed-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split"))
    return ap


def make_cameras(n, W, H, origin, radius, seed=0):
    import numpy as np

    from neuralrecon_w_amd import views

    rs = np.random.RandomState(seed)
    cams = []
    f = 0.5 * W / np.tan(np.deg2rad(30.0))
    K = np.array([[f, 0, 0.5 * W], [0, f, 0.5 * H], [0, 0, 1]])
    for _ in range(n):
        u = rs.normal(size=3)
        pos = origin + u / np.linalg.norm(u) * radius * rs.uniform(1.5, 4.0)
        target = origin + rs.uniform(-1.5, 1.5, 3) * radius
        z = target - pos
        z /= np.linalg.norm(z)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        c2w = np.stack([x, -y, -z, pos], 1)  # columns: right, up, back, centre
        cams.append(views.Camera(K, c2w, W, H, 0.1, 10.0))
    return cams


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def host_part(n, W, H):
    """Seconds for n header reads and n label histograms of a scene on disk (one JPEG and one npz, copied n times)."""
    import numpy as np
    from PIL import Image

    from neuralrecon_w_amd import sceneprep

    rs = np.random.RandomState(1)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.clip(np.stack([255 * xx / (W - 1), 255 * yy / (H - 1), 127 + 100 * np.sin(0.05 * xx + 0.03 * yy)], -1) + rs.normal(0, 6, (H, W, 3)), 0, 255)
    lab = rs.randint(0, 150, size=(H // 16 + 1, W // 16 + 1)).repeat(16, 0).repeat(16, 1)[:H, :W].astype(np.uint8)
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "images"))
        os.makedirs(os.path.join(d, "semantic_maps"))
        Image.fromarray(img.astype(np.uint8)).save(os.path.join(d, "images", "im0000.jpg"), quality=90)
        np.savez_compressed(os.path.join(d, "semantic_maps", "im0000.npz"), lab)
        names = ["im%04d.jpg" % k for k in range(n)]
        for k in range(1, n):
            shutil.copy(os.path.join(d, "images", "im0000.jpg"), os.path.join(d, "images", names[k]))
            shutil.copy(os.path.join(d, "semantic_maps", "im0000.npz"), os.path.join(d, "semantic_maps", "im%04d.npz" % k))
        t0 = time.perf_counter()
        for name in names:
            with Image.open(os.path.join(d, "images", name)) as im:
                assert im.size == (W, H)
        t1 = time.perf_counter()
        sceneprep.static_shares(d, "semantic_maps", names)
        t2 = time.perf_counter()
        size = os.path.getsize(os.path.join(d, "images", "im0000.jpg"))
    return {"images": n, "jpeg_bytes": size, "headers_s": round(t1 - t0, 4), "label_maps_s": round(t2 - t1, 4)}


def main(argv=None):
    args = build_parser().parse_args(argv)
    import ctypes as C

    import numpy as np
    import torch

    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import sceneprep, views

    if not torch.cuda.is_available():
        raise SystemExit("bench_split.py needs a GPU: nothing is timed on a CPU")
    dev = torch.device("cuda", 0)
    n, W, H = args.views, args.width, args.height
    origin, radius = np.array([0.5, -0.1, 6.0]), 4.0
    cams = make_cameras(n, W, H, origin, radius)
    prefix = sceneprep.pixel_prefix(cams)
    table = (L.NcwViewCamera * n)(*[c.struct() for c in cams])
    cams_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    prefix_d = torch.from_numpy(prefix).to(dev)
    count_d = torch.empty(n, device=dev, dtype=torch.int32)
    org = (C.c_float * 3)(*[float(v) for v in origin])
    lib = L.get_lib()

    def fused():
        L.check(lib.ncw_views_roi(L.ptr(cams_d), L.ptr(prefix_d), n, org, float(radius), L.ptr(count_d), None, L.stream_ptr(dev)),
                "ncw_views_roi")

    origin_t = torch.tensor(origin, dtype=torch.float32, device=dev)
    comp_counts = torch.empty(n, device=dev, dtype=torch.int64)
    rays = torch.empty(W * H, 8, device=dev, dtype=torch.float32)

    def composed():
        for k, cam in enumerate(cams):
            r = views.view_rays(cam, device=dev, out=rays)
            o, d = r[:, 0:3], r[:, 3:6]
            # the predicate of include/neuconw_hip.h ("View selection"), one torch op per term (dataset_filter_utils.py:171-178)
            c = origin_t - o
            dot = ((origin_t - o) * d).sum(-1, keepdim=True)
            p = dot * d
            dist_ray = (c - p).norm(dim=-1)
            dist_cam = c.norm(dim=-1)
            roi = ((dist_cam < radius) | (dot[:, 0] > 0)) & (dist_ray < radius)
            comp_counts[k] = roi.sum()

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
    t_f, t_c, t_u = [], [], []
    rounds = max(args.reps, args.composed_reps)
    for r in range(rounds):  # alternate: other work shares the machine
        if r < args.reps:
            t_f.append(timed(fused))
            t0 = time.perf_counter()
            shares, counts = sceneprep.roi_shares(cams, origin, radius, dev)
            t_u.append(1e3 * (time.perf_counter() - t0))
        if r < args.composed_reps:
            t_c.append(timed(composed))
    fused()
    torch.cuda.synchronize()
    fc = count_d.cpu().numpy().astype(np.int64)
    cc = comp_counts.cpu().numpy()
    pixels = int(prefix[-1])
    fused_ms, comp_ms = median(t_f), median(t_c)
    line = {"metric": "split_roi", "views": n, "width": W, "height": H, "pixels": pixels, "reps": args.reps, "composed_reps": args.composed_reps,
            "fused_ms": round(fused_ms, 4), "fused_gpix_per_s": round(pixels / fused_ms / 1e6, 2), "fused_upload_ms": round(median(t_u), 3),
            "composed_ms": round(comp_ms, 3), "composed_per_image_ms": round(comp_ms / n, 4), "ratio": round(comp_ms / fused_ms, 2),
            "fused_faster": bool(fused_ms < comp_ms), "rounds_ms": {"fused": [round(x, 4) for x in t_f], "composed": [round(x, 3) for x in t_c]},
            "counts_equal": bool(np.array_equal(fc, cc)), "max_count_diff": int(np.abs(fc - cc).max()), "counts_equal_roi_shares": bool(np.array_equal(fc, counts)),
            "share_min_median_max": [round(float(v), 4) for v in (shares.min(), np.median(shares), shares.max())],
            "kept_at_0.5": int((shares >= 0.5).sum()), "host": host_part(n, W, H), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "split_%dx%dx%d.json" % (n, W, H)), "w") as fh:
        fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
