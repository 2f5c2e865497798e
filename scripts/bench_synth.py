"""Times the per-image passes of the synthetic-scene generator (neuralrecon_w_amd.synth) on the built-in facade: one image of
--width x --height at --ss x --ss samples per pixel and --points key-point candidates.

    python scripts/bench_synth.py [--width 1024 --height 768 --ss 2] [--points 40000] [--reps 7] [--out profiles/synth]

One JSON line (also written to <out>/synth_<W>x<H>_ss<ss>.json), one call, device events, warm, medians of --reps (min / max in
`rounds_ms`), the variants alternating:
  raster_ms       reproj.RasterMesh.rasterize + resolve of the (H ss) x (W ss) planes;
  shade_ms        ONE `ncw_synth_shade` launch (image, label map, depth);
  composed_ms     the same three planes composed from torch ops on the same inputs: the Philox rounds in int64 tensors, the
                  lattice gathers, the trilinear blends, shading, the mean over the sub-samples -- what one would write without the
                  kernel; `composed_max_rgb_diff` is its largest difference from the kernel's image in 8-bit steps (torch
                  contracts and reorders: not bit for bit);
  observe_ms      ONE `ncw_synth_observe` launch over --points points;
  encode_write_s  host: the image as PNG (views.write_png) and the label map as npz to a temporary directory (wall clock).
A GPU is required; nothing here is timed on a CPU except the file writes."""
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
    ap.add_argument("--ss", type=int, default=2)
    ap.add_argument("--points", type=int, default=40000)
    ap.add_argument("--max_edge", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth"))
    return ap


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def philox_word0(torch, ix, iy, iz, seed, octave):
    """First word of Philox4x32-10 of counter (ix, iy, iz, seed), key (octave, 0), on int64 tensors holding 32-bit words."""
    M = 0xFFFFFFFF
    c0, c1, c2 = ix & M, iy & M, iz & M
    c3 = torch.full_like(c0, seed & M)
    k0, k1 = octave & M, 0

    def mulhilo(a, b):  # a: python int < 2^32, b: int64 tensor < 2^32; the 64-bit product in two halves without overflow
        lo16, hi16 = b & 0xFFFF, b >> 16
        p_lo, p_hi = a * lo16, a * hi16        # each < 2^48
        low = p_lo + ((p_hi & 0xFFFF) << 16)   # < 2^49
        return ((p_hi >> 16) + (low >> 32)) & M, low & M

    for _ in range(10):
        h0, l0 = mulhilo(0xD2511F53, c0)
        h1, l1 = mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return c0


def main(argv=None):
    args = build_parser().parse_args(argv)
    import numpy as np
    import torch

    from neuralrecon_w_amd import evalmesh, reproj, synth, views

    if not torch.cuda.is_available():
        raise SystemExit("bench_synth.py needs a GPU: nothing is timed on a CPU")
    dev = torch.device("cuda", 0)
    W, H, ss = args.width, args.height, args.ss
    mesh = synth.facade_mesh(0, args.max_edge)
    lo, hi = synth.building_box(mesh)
    sfm2gt = synth.random_sfm2gt(0, (lo + hi) / 2, float(np.linalg.norm(hi - lo)))
    inv = synth.invert_similarity(sfm2gt)
    scale = float(np.sqrt((sfm2gt[0, :3] ** 2).sum()))
    verts = mesh.verts @ inv[:3, :3].T + inv[:3, 3]
    cam = synth.make_cameras(0, 1, (W, H), lo, hi)[0]
    cam.update(width=W, height=H, K=(cam["K"][0], cam["K"][1], W / 2.0, H / 2.0))
    R, t = synth.to_sfm_pose(cam["w2c"], sfm2gt)
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = R, t
    app = synth.draw_appearance(np.random.default_rng(0))
    nrm = synth.face_normals(mesh.verts, mesh.faces)[0]
    mats = mesh.materials
    img = synth.image_struct(cam["K"], np.linalg.inv(w2c), sfm2gt, H, W, ss, app, 0, synth.labels.label_id("sky"))
    rm = reproj.RasterMesh(verts, mesh.faces, dev)
    rs = rm.view_struct(synth.raster_K(cam["K"], ss), w2c, H * ss, W * ss, znear=0.01, zfar=1000.0)
    zbuf = torch.empty(H * ss * W * ss, dtype=torch.int64, device=dev)
    nrm_d, mat_d = torch.from_numpy(nrm.astype(np.float32)).to(dev), torch.from_numpy(mesh.material).to(dev)
    tab = synth.material_table(mats, dev)
    pts, tri = evalmesh.sample_surface(mesh.verts, mesh.faces, args.points, seed=0, return_index=True, device=dev)
    pts_d = torch.from_numpy(pts.cpu().numpy() @ inv[:3, :3].T + inv[:3, 3]).to(dev)
    pn_d = torch.from_numpy(np.ascontiguousarray(nrm[tri.cpu().numpy().astype(np.int64)] @ (sfm2gt[:3, :3] / scale))).to(dev)
    idx_d = torch.arange(pts_d.shape[0], dtype=torch.int64, device=dev)
    vs = synth.view_struct(w2c, cam["K"], H, W, 0.01, 0.5, synth.DEPTH_TOL, 0, 1)
    state = {}

    def raster():
        rm.rasterize(rs, zbuf)
        state["planes"] = reproj.resolve(zbuf, H * ss, W * ss)

    def shade():
        state["out"] = synth.shade(state["planes"][0], state["planes"][1], img, nrm_d, mat_d, tab, len(mats))

    def observe():
        state["obs"] = synth.observe(pts_d, pn_d, idx_d, vs, state["out"][2])

    base = torch.tensor([m["base"] for m in mats], dtype=torch.float32, device=dev)
    freq = torch.tensor([m["freq"] for m in mats], dtype=torch.float32, device=dev)
    amp = torch.tensor([m["amp"] for m in mats], dtype=torch.float32, device=dev)
    c2w_t = torch.tensor(np.linalg.inv(w2c)[:3], dtype=torch.float32, device=dev)
    s2g_t = torch.tensor(sfm2gt[:3], dtype=torch.float32, device=dev)
    light = torch.tensor(app["light"], dtype=torch.float32, device=dev)
    gain, bias = torch.tensor(app["gain"], dtype=torch.float32, device=dev), torch.tensor(app["bias"], dtype=torch.float32, device=dev)
    top, bot = torch.tensor(app["sky_top"], dtype=torch.float32, device=dev), torch.tensor(app["sky_bottom"], dtype=torch.float32, device=dev)
    rr, cc = torch.meshgrid(torch.arange(H * ss, device=dev), torch.arange(W * ss, device=dev), indexing="ij")
    px = (cc // ss).float() + ((cc % ss).float() + 0.5) / ss - 0.5
    py = (rr // ss).float() + ((rr % ss).float() + 0.5) / ss - 0.5
    trow = ((rr // ss).float() / H)[..., None]

    def composed():
        d, f = state["planes"]
        hit = (f >= 0) & (d > 0)
        fs = torch.where(hit, f, torch.zeros_like(f)).long()
        cam_p = torch.stack([(px - cam["K"][2]) / cam["K"][0] * d, (py - cam["K"][3]) / cam["K"][1] * d, d], -1)
        g = (cam_p @ c2w_t[:, :3].T + c2w_t[:, 3]) @ s2g_t[:, :3].T + s2g_t[:, 3]
        m = mat_d[fs].long()
        n, wgt, f0 = torch.zeros_like(d), 0.5, freq[m]
        for o in range(3):
            q = g * f0[..., None]
            fl = torch.floor(q)
            tt = q - fl
            i = fl.long()
            h = lambda dx, dy, dz: (philox_word0(torch, i[..., 0] + dx, i[..., 1] + dy, i[..., 2] + dz, 0, o) >> 8).float() * 2.0 ** -24
            lerp = lambda a, b, t_: a + t_ * (b - a)
            c00, c10 = lerp(h(0, 0, 0), h(1, 0, 0), tt[..., 0]), lerp(h(0, 1, 0), h(1, 1, 0), tt[..., 0])
            c01, c11 = lerp(h(0, 0, 1), h(1, 0, 1), tt[..., 0]), lerp(h(0, 1, 1), h(1, 1, 1), tt[..., 0])
            n = n + wgt * lerp(lerp(c00, c10, tt[..., 1]), lerp(c01, c11, tt[..., 1]), tt[..., 2])
            f0, wgt = f0 * 2, wgt * 0.5
        lam = app["ambient"] + app["diffuse"] * (nrm_d[fs] @ light).clamp_min(0)
        v = (gain * (base[m] * (1 + amp[m] * (n - 0.4375))[..., None] * lam[..., None]) + bias).clamp(0, 1)
        v = torch.where(hit[..., None], v, (top + trow * (bot - top)).clamp(0, 1))
        rgb = (v.reshape(H, ss, W, ss, 3).mean((1, 3)) * 255 + 0.5).to(torch.uint8)
        state["composed"] = rgb

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for fn in (raster, shade, observe, composed):  # warm
        fn()
    torch.cuda.synchronize()
    names = ("raster", "shade", "composed", "observe")
    fns = {"raster": raster, "shade": shade, "composed": composed, "observe": observe}
    times = {k: [] for k in names}
    for r in range(args.reps):
        for k in (names if r % 2 == 0 else names[::-1]):
            times[k].append(timed(fns[k]))
    rgb, label, depth = [x.cpu().numpy() for x in state["out"]]
    diff = int((state["composed"].cpu().numpy().astype(np.int64) - rgb.astype(np.int64)).__abs__().max())
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        views.write_png(os.path.join(d, "a.png"), rgb)
        synth.write_npz(os.path.join(d, "a.npz"), label)
        enc = time.perf_counter() - t0
        png_bytes = os.path.getsize(os.path.join(d, "a.png"))
    med = {k: median(v) for k, v in times.items()}
    line = {"metric": "synth_image", "width": W, "height": H, "ss": ss, "faces": int(len(mesh.faces)), "points": int(pts_d.shape[0]),
            "reps": args.reps, "raster_ms": round(med["raster"], 4), "shade_ms": round(med["shade"], 4),
            "composed_ms": round(med["composed"], 3), "observe_ms": round(med["observe"], 4), "ratio": round(med["composed"] / med["shade"], 2),
            "shade_faster": bool(med["shade"] < med["composed"]), "composed_max_rgb_diff": diff,
            "shade_gsamples_per_s": round(W * H * ss * ss / med["shade"] / 1e6, 3), "encode_write_s": round(enc, 4), "png_bytes": png_bytes,
            "covered_share": round(float((depth > 0).mean()), 4), "visible_points": int(state["obs"][2].sum()),
            "rounds_ms": {k: [round(x, 4) for x in v] for k, v in times.items()}, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "synth_%dx%d_ss%d.json" % (W, H, ss)), "w") as fh:
        fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
