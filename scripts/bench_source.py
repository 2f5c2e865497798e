"""Times the ray source (neuralrecon_w_amd.raysource) against the ray cache it stands beside, on a synthetic scene built in
memory like scripts/bench_cache.py's: --images views of 1024 x 768 around a sphere-shell SfM octree pair (levels 7 / 8), ~4 k
key-points each, so that the kept rays number in the millions.

    python scripts/bench_source.py [--images 8] [--reps 50] [--rounds 5] [--parent_dir <checkout of the parent commit, built>]

One JSON line (also written to <out>/source_<W>x<H>.json).  Everything on the device is timed with device events after a
warm-up; the two paths alternate and swap order every round; medians are reported and every round is kept.
  batch_us[B]          per `RaySource.batch(idx)` and per `RayCache.batch(idx)` over the dense rows of the SAME rays, uniformly
                       random idx (a fresh one per call), B = 2048 and 8192: the whole call as the training loop makes it
                       (allocations, the launch) -- and `launch_us`, the entry point alone on preallocated outputs, also with
                       range == NULL (`source_no_walk`: everything but the range-octree walk);
  identical            the two paths' batches are bit-identical (checked on one idx per B);
  bytes_per_ray        resident bytes per ray of both;
  build_ms_per_image   `RaySource.from_images` against `build_image` + np.savez_compressed + np.load + upload of the same images
                       (wall clock, device synchronised; the images are decoded and in host memory in both);
  step_vs_parent       with --parent_dir: `bench.py --gpus 1` of this tree and of the parent, alternating, order swapped every
                       round (ms_per_step of every run, the medians and their difference).
A GPU is required; nothing here is timed on a CPU.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--keypoints", type=int, default=4000)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50, help="batches per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--parent_dir", default=None, help="a built checkout of the parent commit: bench.py runs there too")
    ap.add_argument("--step_rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "source"))
    return ap


def make_items(args, dev):
    """--images views of the bench_cache.py scene (the camera moves sideways from one to the next), decoded and in host memory."""
    import numpy as np

    from bench_cache import shell
    from neuralrecon_w_amd import views, voxel

    W, H, n_kp = args.width, args.height, args.keypoints
    rs = np.random.RandomState(0)
    origin, scale_hit, voxel_size = [0.5, -0.1, 6.0], 31.8, 0.25
    hit = voxel.occupancy_from_dense(shell(7, 0.5, 1.5 / 128, dev), origin, scale_hit, voxel_size)
    rng = voxel.occupancy_from_dense(shell(8, 0.5 / 1.5, 3.0 / 256, dev), origin, scale_hit * 1.5, voxel_size)
    fx = 0.5 * W / np.tan(np.deg2rad(25.0))
    K = np.array([[fx, 0, 0.5 * W - 0.3], [0, fx, 0.5 * H + 0.4], [0, 0, 1]])
    dist = 2.2 * scale_hit
    yy, xx = np.mgrid[0:H, 0:W]
    items = []
    for k in range(args.images):
        shift = (k - 0.5 * (args.images - 1)) * 0.08 * scale_hit
        c2w = np.array([[1.0, 0, 0, origin[0] + shift], [0, 1.0, 0, origin[1]], [0, 0, 1.0, origin[2] + dist]])
        w2c = np.eye(4)
        w2c[:3, :3] = np.diag([1.0, -1.0, -1.0])
        w2c[:3, 3] = -w2c[:3, :3] @ c2w[:, 3]
        cam = views.Camera(K, c2w, W, H, dist - 0.6 * scale_hit, dist + 0.6 * scale_hit)
        img = np.clip(np.stack([255 * xx / (W - 1), 255 * yy / (H - 1), 127 + 100 * np.sin(0.05 * xx + 0.03 * yy + k)], -1)
                      + rs.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
        lab = rs.randint(0, 150, size=(H // 16 + 1, W // 16 + 1)).repeat(16, 0).repeat(16, 1)[:H, :W].astype(np.uint8)
        u = rs.normal(size=(n_kp, 3))
        xyz = (np.array(origin) + 0.5 * scale_hit * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
        camp = xyz.astype(np.float64) @ w2c[:3, :3].T + w2c[:3, 3]
        px = np.rint(np.stack([fx * camp[:, 0] / camp[:, 2] + K[0, 2], fx * camp[:, 1] / camp[:, 2] + K[1, 2]], -1)).astype(np.int32)
        err = rs.uniform(0.3, 1.8, n_kp).astype(np.float32)
        items.append((cam, img, k + 1, (xyz, err, px, float(err.astype(np.float64).mean())), w2c, lab))
    return items, hit, rng, voxel_size


def window_us(fn, idxs):
    """Device events around one call of fn per idx; µs per call."""
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in idxs:
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / len(idxs)


def med(v):
    import numpy as np

    return float(np.median(v))


def bench_steps(args):
    if not args.parent_dir:
        return None
    runs = {"this": [], "parent": []}
    dirs = {"this": ROOT, "parent": os.path.abspath(args.parent_dir)}
    for r in range(args.step_rounds):
        for who in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup)],
                               cwd=dirs[who], capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise SystemExit("bench.py failed in %s:\n%s\n%s" % (dirs[who], p.stdout[-2000:], p.stderr[-3000:]))
            line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
            runs[who].append(float(json.loads(line)["ms_per_step"]))
    return {"steps": args.steps, "warmup": args.warmup, "ms_per_step": {k: [round(x, 4) for x in v] for k, v in runs.items()},
            "median_ms": {k: round(med(v), 4) for k, v in runs.items()}, "this_minus_parent_ms": round(med(runs["this"]) - med(runs["parent"]), 4)}


def main(argv=None):
    args = build_parser().parse_args(argv)
    import numpy as np
    import torch

    from neuralrecon_w_amd import cachebuild, raycache, raysource
    from neuralrecon_w_amd import lib as L

    if not torch.cuda.is_available():
        raise SystemExit("bench_source.py needs a GPU: nothing is timed on a CPU")
    dev = torch.device("cuda", 0)
    items, hit, rng, vs = make_items(args, dev)

    # ---- building: records against rows + files + reload
    def build_source():
        s = raysource.RaySource.from_images(items, hit, rng, vs, device=dev)
        torch.cuda.synchronize()
        return s

    def build_rows(tmp):
        rows = []
        for k, it in enumerate(items):
            rays, rgbs = cachebuild.build_image(*it, hit, rng, vs, device=dev)
            f = os.path.join(tmp, "im%d" % k)
            np.savez_compressed(f + "_rays.npz", rays.cpu().numpy())
            np.savez_compressed(f + "_rgbs.npz", rgbs.cpu().numpy())
            rows.append((torch.from_numpy(np.load(f + "_rays.npz")["arr_0"]).to(dev), torch.from_numpy(np.load(f + "_rgbs.npz")["arr_0"]).to(dev)))
        torch.cuda.synchronize()
        return rows

    build_source()  # warm: library load, allocator
    t_src, t_rows = [], []
    for r in range(3):
        for who in (("s", "c") if r % 2 == 0 else ("c", "s")):
            t0 = time.perf_counter()
            if who == "s":
                src = build_source()
                t_src.append(1e3 * (time.perf_counter() - t0) / len(items))
            else:
                with tempfile.TemporaryDirectory() as tmp:
                    rows = build_rows(tmp)
                t_rows.append(1e3 * (time.perf_counter() - t0) / len(items))
    rc = raycache.RayCache.__new__(raycache.RayCache)  # the dense rows of the same rays, resident as RayCache holds them
    rc.device, rc.with_semantics, rc.mask_ids, rc._ids_arr, rc.prefiltered = dev, True, [], (C.c_int * 4)(), False
    rc.all_rays = torch.cat([r[0] for r in rows], 0).contiguous()
    rc.all_rgbs = torch.cat([r[1] for r in rows], 0).contiguous()
    del rows
    n = len(src)
    assert n == len(rc)

    # ---- batches
    lib, st = L.get_lib(), L.stream_ptr(dev)
    tree = cachebuild._octree_struct(rng)
    out = {"identical": True, "batch_us": {}, "launch_us": {}, "rounds_us": {}}
    g = torch.Generator(device=dev).manual_seed(0)
    for B in args.batches:
        idxs = [torch.randint(0, n, (B,), device=dev, generator=g) for _ in range(args.reps)]
        a, b = src.batch(idxs[0]), rc.batch(idxs[0])
        out["identical"] = bool(out["identical"] and all(torch.equal(a[k], b[k]) for k in a))
        rays, ts, lab = torch.empty(B, 11, device=dev), torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
        rgbs, keep = torch.empty(B, 3, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
        P = L.ptr

        def launch_source(i):
            lib.ncw_source_batch(P(src.recs), n, P(src.images), P(src.row_start), P(src.kp_start), src.n_img, P(src.kp_pix),
                                 P(src.kp_depth), P(src.kp_weight), C.byref(tree), vs, P(i), B, 1, P(rays), P(ts), P(lab), P(rgbs),
                                 rc._ids_arr, 0, P(keep), st)

        def launch_source_no_walk(i):  # range == NULL: the camera's near / far -- everything but the octree walk
            lib.ncw_source_batch(P(src.recs), n, P(src.images), P(src.row_start), P(src.kp_start), src.n_img, P(src.kp_pix),
                                 P(src.kp_depth), P(src.kp_weight), None, vs, P(i), B, 1, P(rays), P(ts), P(lab), P(rgbs),
                                 rc._ids_arr, 0, P(keep), st)

        def launch_cache(i):
            lib.ncw_batch_assemble(P(rc.all_rays), 13, P(rc.all_rgbs), P(i), n, B, 1, P(rays), P(ts), P(lab), P(rgbs), rc._ids_arr, 0,
                                   P(keep), st)

        fns = {"source": src.batch, "cache": rc.batch, "source_launch": launch_source, "cache_launch": launch_cache,
               "source_launch_no_walk": launch_source_no_walk}
        rounds = {k: [] for k in fns}
        for k in fns:
            window_us(fns[k], idxs[:5])  # warm
        for r in range(args.rounds):
            order = list(fns) if r % 2 == 0 else list(fns)[::-1]
            for k in order:
                rounds[k].append(window_us(fns[k], idxs))
        out["batch_us"][str(B)] = {"source": round(med(rounds["source"]), 2), "cache": round(med(rounds["cache"]), 2)}
        out["launch_us"][str(B)] = {"source": round(med(rounds["source_launch"]), 2), "cache": round(med(rounds["cache_launch"]), 2),
                                    "source_no_walk": round(med(rounds["source_launch_no_walk"]), 2)}
        out["rounds_us"][str(B)] = {k: [round(x, 2) for x in v] for k, v in rounds.items()}
    cache_bytes = rc.all_rays.numel() * 4 + rc.all_rgbs.numel() * 4
    line = {"metric": "ray_source", "width": args.width, "height": args.height, "images": len(items), "keypoints": args.keypoints,
            "levels": [int(hit["level"]), int(rng["level"])], "n_rows": n, "key_point_entries": int(src.kp_pix.numel()),
            "reps": args.reps, "rounds": args.rounds, **out,
            "bytes_per_ray": {"source": round(src.nbytes() / n, 3), "cache": round(cache_bytes / n, 3)},
            "build_ms_per_image": {"source": round(med(t_src), 2), "rows_npz_reload": round(med(t_rows), 2),
                                   "rounds": {"source": [round(x, 2) for x in t_src], "rows_npz_reload": [round(x, 2) for x in t_rows]}},
            "device": torch.cuda.get_device_name(0)}
    del src, rc
    torch.cuda.empty_cache()
    line["step_vs_parent"] = bench_steps(args)
    print(json.dumps(line), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "source_%dx%d.json" % (args.width, args.height)), "w") as fh:
        fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
