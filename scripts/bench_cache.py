"""Times the per-image work of the ray-cache writer (neuralrecon_w_amd.cachebuild) on a synthetic scene built in memory: one
1024 x 768 image, ~4 k key-points, a sphere-shell SfM octree pair at the levels brandenburg_gate's config.yaml gives (voxel_size
0.25 in a 63.6-unit box: level 7 for the hit octree, level 8 for the range octree at radius 1.5).

    python scripts/bench_cache.py [--width 1024 --height 768] [--keypoints 4000] [--reps 20] [--out profiles/cache]

One JSON line (also written to <out>/cache_<W>x<H>.json):
  (three rounds alternate the paths; the medians are reported and every round is kept in rounds_ms)
  fused_ms             HIP events around --reps x (ncw_sfm_depth_splat + ncw_cache_rows + keep.nonzero() + ncw_batch_assemble), after a
                       warm-up, per image: cachebuild.build_image on device-resident inputs;
  fused_rows_ms        the same window around the ONE ncw_cache_rows launch alone;
  composed_ms          the same rows composed from the launches that existed before: views.view_rays + two voxel.get_near_far +
                       torch (index_put of the key-points, the dir_norm plane, image / 255, the label gather, torch.cat of the
                       13 columns, boolean masks), device-resident inputs, no host round trip -- NOT the reference's path, which
                       also copies every 100 k-ray chunk to the host;
  max_abs_diff         fused vs composed rows (the two must agree: same rays, same walk);
  d2h_bytes            bytes that leave the device for the image (kept rows x 16 floats) and what all pixels would be;
  build_cache          a whole cachebuild.build_cache (4 chunks) of --images copies of that view written to a temporary scene
                       directory (JPEGs, COLMAP model, label maps, config.yaml; the octrees come from the key-points there): wall
                       time, and the shares of host decode (PIL + label map), of the device part (upload, kernels, copy back)
                       and of np.savez_compressed; the rest is reading the COLMAP model and building the octrees.
A GPU is required; nothing here is timed on a CPU.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--keypoints", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=6, help="images of the scene the whole build_cache runs on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cache"))
    return ap


def shell(level, r0, thick, device):
    import torch

    G = 1 << level
    c = (torch.arange(G, device=device).float() + 0.5) * (2.0 / G) - 1.0
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    return ((x * x + y * y + z * z).sqrt() - r0).abs() < thick


def write_scene(root, n_images, img, lab, xyz, err, camp, K, w2c, origin, scale, voxel_size):
    """The benchmark view as a scene directory: n_images registered copies of it (same pose), all in the train split."""
    import struct

    import numpy as np
    import yaml
    from PIL import Image

    sp = os.path.join(root, "dense", "sparse")
    for sub in (sp, os.path.join(root, "dense", "images"), os.path.join(root, "semantic_maps")):
        os.makedirs(sub)
    H, W = img.shape[:2]
    uv = np.stack([K[0, 0] * camp[:, 0] / camp[:, 2] + K[0, 2], K[1, 1] * camp[:, 1] / camp[:, 2] + K[1, 2]], -1)
    with open(os.path.join(sp, "points3D.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(xyz)))
        for i, p in enumerate(xyz):
            fh.write(struct.pack("<QdddBBBd", i + 1, *[float(v) for v in p], 128, 128, 128, float(err[i])) + struct.pack("<Qii", 1, 1, i))
    with open(os.path.join(sp, "cameras.bin"), "wb") as fh:
        fh.write(struct.pack("<QiiQQdddd", 1, 1, 1, W, H, K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    with open(os.path.join(sp, "images.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", n_images))
        for k in range(n_images):
            name = "im%03d.jpg" % k
            fh.write(struct.pack("<i7di", k + 1, 0.0, 1.0, 0.0, 0.0, *[float(v) for v in w2c[:3, 3]], 1) + name.encode() + b"\x00")  # R = diag(1, -1, -1)
            fh.write(struct.pack("<Q", len(xyz)) + b"".join(struct.pack("<ddq", float(u), float(v), i + 1) for i, (u, v) in enumerate(uv)))
            Image.fromarray(img).save(os.path.join(root, "dense", "images", name), quality=92)
            np.savez_compressed(os.path.join(root, "semantic_maps", "im%03d.npz" % k), lab)
    with open(os.path.join(root, "bench_scene.tsv"), "w") as fh:
        fh.write("filename\tid\tsplit\tdataset\n" + "".join("im%03d.jpg\t%d\ttrain\tsynthetic\n" % (k, k) for k in range(n_images)))
    o = np.array(origin, dtype=np.float64)
    with open(os.path.join(root, "config.yaml"), "w") as fh:
        yaml.safe_dump({"name": "bench_scene", "origin": o.tolist(), "radius": float(scale), "eval_bbx": [(o - scale).tolist(), (o + scale).tolist()],
                        "voxel_size": float(voxel_size), "min_track_length": 0, "sfm2gt": np.eye(4).tolist()}, fh)


def timed(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def main(argv=None):
    args = build_parser().parse_args(argv)
    import numpy as np
    import torch

    from neuralrecon_w_amd import cachebuild, views, voxel

    if not torch.cuda.is_available():
        raise SystemExit("bench_cache.py needs a GPU: nothing is timed on a CPU")
    dev = torch.device("cuda", 0)
    W, H, n_kp = args.width, args.height, args.keypoints
    rs = np.random.RandomState(0)
    # the scene: cube = origin +- scale in SfM units; a shell of radius 0.5 scale; voxel_size as 2 scale / 254
    origin, scale_hit = [0.5, -0.1, 6.0], 31.8
    voxel_size = 0.25
    hit = voxel.occupancy_from_dense(shell(7, 0.5, 1.5 / 128, dev), origin, scale_hit, voxel_size)
    rng = voxel.occupancy_from_dense(shell(8, 0.5 / 1.5, 3.0 / 256, dev), origin, scale_hit * 1.5, voxel_size)
    fx = 0.5 * W / np.tan(np.deg2rad(25.0))
    K = np.array([[fx, 0, 0.5 * W - 0.3], [0, fx, 0.5 * H + 0.4], [0, 0, 1]])
    dist = 2.2 * scale_hit
    c2w = np.array([[1.0, 0, 0, origin[0]], [0, 1.0, 0, origin[1]], [0, 0, 1.0, origin[2] + dist]])  # looks down -z at the shell
    w2c = np.eye(4)
    w2c[:3, :3] = np.diag([1.0, -1.0, -1.0])  # COLMAP axes: right down front
    w2c[:3, 3] = -w2c[:3, :3] @ c2w[:, 3]
    cam = views.Camera(K, c2w, W, H, dist - 0.6 * scale_hit, dist + 0.6 * scale_hit)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.clip(np.stack([255 * xx / (W - 1), 255 * yy / (H - 1), 127 + 100 * np.sin(0.05 * xx + 0.03 * yy)], -1)
                  + rs.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
    lab = rs.randint(0, 150, size=(H // 16 + 1, W // 16 + 1)).repeat(16, 0).repeat(16, 1)[:H, :W].astype(np.uint8)
    u = rs.normal(size=(n_kp, 3))
    xyz = (np.array(origin) + 0.5 * scale_hit * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    camp = xyz.astype(np.float64) @ w2c[:3, :3].T + w2c[:3, 3]
    px = np.rint(np.stack([fx * camp[:, 0] / camp[:, 2] + K[0, 2], fx * camp[:, 1] / camp[:, 2] + K[1, 2]], -1)).astype(np.int32)
    err = rs.uniform(0.3, 1.8, n_kp).astype(np.float32)
    em = float(err.astype(np.float64).mean())
    img_d, lab_d = torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)
    kp_d = (torch.from_numpy(xyz).to(dev), torch.from_numpy(err).to(dev), torch.from_numpy(px).to(dev), em)

    def fused():
        return cachebuild.build_image(cam, img_d, 7, kp_d, w2c, lab_d, hit, rng, voxel_size, device=dev)

    dz, wt = cachebuild.sfm_depth_planes(*kp_d, w2c, W, H, dev)

    def fused_rows():
        return cachebuild.cache_rows(cam, img_d, 7, dz, wt, lab_d, hit, rng, voxel_size)

    z_row = torch.tensor(w2c[2], dtype=torch.float32, device=dev)
    ii, jj = torch.meshgrid(torch.arange(W, device=dev, dtype=torch.float32), torch.arange(H, device=dev, dtype=torch.float32), indexing="xy")

    def composed():
        rays = views.view_rays(cam, device=dev)
        o, d = rays[:, 0:3], rays[:, 3:6]
        hn, _ = voxel.get_near_far(o, d, hit)
        rn, rf = voxel.get_near_far(o, d, rng)
        keep = (hn > 0).reshape(-1)
        rf = torch.where(rn > 0, rf + voxel_size, rf)
        # get_colmap_depth with torch ops (assignment with repeated indices: unordered on the device, as in the reference)
        p = kp_d[2].long()
        ok = (p[:, 0] >= 0) & (p[:, 0] < W) & (p[:, 1] >= 0) & (p[:, 1] < H)
        depth = torch.zeros(H, W, device=dev)
        weight = torch.zeros(H, W, device=dev)
        z = kp_d[0][ok] @ z_row[:3] + z_row[3]
        depth[p[ok, 1], p[ok, 0]] = z
        weight[p[ok, 1], p[ok, 0]] = 2 * torch.exp(-((kp_d[1][ok] / em) ** 2))
        norm = torch.sqrt(((ii - float(K[0, 2])) / float(fx)) ** 2 + ((jj - float(K[1, 2])) / float(fx)) ** 2 + 1)
        rgb = img_d.reshape(-1, 3).float() / 255
        rows = torch.cat([rays[:, :6], rn, rf, torch.full_like(rn, 7.0), lab_d.reshape(-1, 1).float(), (depth * norm).reshape(-1, 1),
                          weight.reshape(-1, 1), torch.zeros_like(rn)], 1)
        return rows[keep], rgb[keep]

    # three rounds, alternating the two paths (other work shares the machine): the medians are reported, the rounds kept
    rounds = {"fused": [], "rows": [], "composed": []}
    for _ in range(3):
        ms, (f_rows, f_rgb) = timed(fused, args.reps)
        rounds["fused"].append(ms)
        rounds["rows"].append(timed(fused_rows, args.reps)[0])
        ms, (c_rows, c_rgb) = timed(composed, args.reps)
        rounds["composed"].append(ms)
    fused_ms, rows_ms, comp_ms = [sorted(rounds[k])[1] for k in ("fused", "rows", "composed")]
    same_shape = tuple(f_rows.shape) == tuple(c_rows.shape)
    # the key-point columns differ where the composed path's unordered assignment picked another key-point of a collision
    diff = float((f_rows[:, :10] - c_rows[:, :10]).abs().max()) if same_shape and f_rows.shape[0] else float("nan")
    rgb_same = bool(same_shape and torch.equal(f_rgb, c_rgb))
    n_kept = int(f_rows.shape[0])
    # a whole build_cache of the same view as a scene on disk: --images JPEGs, COLMAP model, label maps, config.yaml
    with tempfile.TemporaryDirectory() as d:
        root = os.path.join(d, "bench_scene")
        write_scene(root, args.images, img, lab, xyz, err, camp, K, w2c, origin, scale_hit, voxel_size)
        stats = {}
        t0 = time.perf_counter()
        cachebuild.build_cache(root, "cache", 1, "semantic_maps", 4, "sparse", device=dev, stats=stats)
        t_all = time.perf_counter() - t0
    t_dec, t_dev, t_npz = stats["t_decode"], stats["t_device"], stats["t_write"]
    line = {"metric": "cache_image", "width": W, "height": H, "keypoints": n_kp, "levels": [int(hit["level"]), int(rng["level"])],
            "reps": args.reps, "kept_rays": n_kept, "pixels": W * H, "fused_ms": round(fused_ms, 4), "fused_rows_ms": round(rows_ms, 4),
            "composed_ms": round(comp_ms, 4), "rounds_ms": {k: [round(x, 4) for x in v] for k, v in rounds.items()}, "fused_faster": bool(fused_ms < comp_ms), "same_shape": same_shape,
            "max_abs_diff_cols0_9": diff, "rgb_identical": rgb_same, "d2h_bytes": 64 * n_kept, "d2h_bytes_all_pixels": 64 * W * H,
            "build_cache": {"images": stats["n_images"], "pixels": stats["n_pixels"], "kept_rays": stats["n_rays"], "d2h_bytes": stats["d2h_bytes"],
                            "total_s": round(t_all, 3), "decode_s": round(t_dec, 3), "device_s": round(t_dev, 3), "npz_s": round(t_npz, 3),
                            "share_decode": round(t_dec / t_all, 4), "share_device": round(t_dev / t_all, 4), "share_npz": round(t_npz / t_all, 4)}, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "cache_%dx%d.json" % (W, H)), "w") as fh:
        fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
