"""Fuse the sphere-traced surface of a scene's views into ONE oriented, coloured point cloud (not in the reference).

    python scripts/surface_cloud.py --cfg_path config/train_brandenburg_gate.yaml --ckpt_path ckpts/exp/last.ckpt \
        --root_dir data/heritage-recon/brandenburg_gate [--split train] [--max_views N] [--view_stride K] [--img_downscale D] \
        [--cell H] [--box sphere|eval_bbx] [--min_views 2] [--cos_min 0.1] [--appearance mean|view|<id>] \
        [--trace_eps 1e-3 --trace_iters 64 --trace_step 1.0] [--out surface_cloud.ply]
    python scripts/eval_mesh.py --file_pred surface_cloud.ply --file_trgt gt.ply --scene_config_path <root_dir>/config.yaml

  * the views are the rows of the scene's split file (*.tsv) that are registered in the COLMAP model, in file order, each with
    the camera views.scene_view(load_image=False) gives it (K rescale, pose flip, per-image near / far); no image is decoded;
  * every view is sphere-traced (views.trace_view) and the rays that HIT -- surface point, SDF gradient, colour -- are
    accumulated per grid cell on the GPU (neuralrecon_w_amd.surfcloud, csrc/ncw_fuse.hip); the samples are never held: the
    table follows the occupied cells.  A hit lies on the zero level set to --trace_eps and is seen by its camera by construction;
  * --cell: the cell size in SfM units, default 2 radius / 1024 -- the spacing of the level-10 lattice scripts/extract_mesh.py
    --eval_level 10 samples, so the two outputs are comparable;
  * --box: the grid's extent: `sphere` = origin +- radius of the scene's config.yaml, `eval_bbx` = its evaluation box carried to
    SfM coordinates through inv(sfm2gt), as the octree builder carries it;
  * --min_views: a cell is written iff at least that many DIFFERENT views hit it; --cos_min: a hit counts iff the cosine
    between its gradient and the direction back to the camera is at least that (negative value = no such test);
  * --appearance: mean = every view is shaded with the mean appearance embedding (the default: one exposure for the whole
    cloud), view = each with its own image's row, <id> = all with that row;
  * the PLY (binary little-endian: double x y z, float nx ny nz, uchar red green blue) is in SfM coordinates like
    extract_mesh's, and scripts/eval_mesh.py scores it as it stands (its point branch).  <out>.report.json holds views, rays,
    state shares, samples valid / invalid, cells, cells kept, growths and ms per stage.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cfg_path", required=True, help="experiment yaml")
    ap.add_argument("--ckpt_path", required=True, help="checkpoint in the reference's layout (trainer.save_checkpoint / PL)")
    ap.add_argument("--root_dir", default=None, help="overrides DATASET.ROOT_DIR")
    ap.add_argument("--split", default="train", choices=["train", "test", "all"], help="rows of the split file to trace")
    ap.add_argument("--max_views", type=int, default=None, help="at most that many views (after --view_stride)")
    ap.add_argument("--view_stride", type=int, default=1, help="every K-th row")
    ap.add_argument("--img_downscale", type=int, default=None, help="default: DATASET.PHOTOTOURISM.IMG_DOWNSCALE")
    ap.add_argument("--sfm_path", default=None, help="COLMAP model directory under <root_dir>/dense/ (default: the reference's "
                                                     "per-scene choice)")
    ap.add_argument("--cell", type=float, default=None, help="cell size in SfM units (default: 2 radius / 1024)")
    ap.add_argument("--box", default="sphere", choices=["sphere", "eval_bbx"], help="extent of the grid")
    ap.add_argument("--min_views", type=int, default=2, help="keep a cell iff that many different views hit it")
    ap.add_argument("--min_count", type=int, default=1, help="keep a cell iff it holds that many samples")
    ap.add_argument("--cos_min", type=float, default=0.1, help="least cosine between gradient and the way back to the camera; "
                                                               "a negative value switches the test off")
    ap.add_argument("--appearance", default="mean", help="mean | view | <embedding row>")
    ap.add_argument("--chunk", type=int, default=None, help="rays per trace call (default: views.TRACE_CHUNK)")
    ap.add_argument("--prec", default=None, choices=["bf16", "f16", "f32"], help="default: the package default")
    ap.add_argument("--trace_eps", type=float, default=1e-3, help="|sdf| <= eps is a hit (unit-sphere units)")
    ap.add_argument("--trace_iters", type=int, default=64, help="most SDF evaluations per ray")
    ap.add_argument("--trace_step", type=float, default=1.0, help="step factor in (0, 1]; < 1 where |grad sdf| > 1")
    ap.add_argument("--out", default="surface_cloud.ply", help="PLY path; the report goes to <out>.report.json")
    return ap


def select_ids(scene, split, stride, max_views):
    """The image ids of the split file's rows (file order) that `split` names, every stride-th, at most max_views."""
    train = set(scene["ids_train"])
    ids = {"all": scene["ids"], "train": scene["ids_train"], "test": [i for i in scene["ids"] if i not in train]}[split]
    ids = list(ids)[::max(1, int(stride))]
    return ids if max_views is None else ids[:max(0, int(max_views))]


def grid_box(scene_cfg, box):
    """(lo, hi) [3] of the grid in SfM coordinates."""
    import numpy as np

    if box == "sphere":
        o, r = np.asarray(scene_cfg["origin"], dtype=np.float64), float(scene_cfg["radius"])
        return o - r, o + r
    gt_to_sfm = np.linalg.inv(np.array(scene_cfg["sfm2gt"], dtype=np.float64))  # voxel.sfm_cube's carry (generate_voxel.py:87-118)
    v1 = gt_to_sfm[:3, :3] @ np.array(scene_cfg["eval_bbx"][0], dtype=np.float64) + gt_to_sfm[:3, 3]
    v2 = gt_to_sfm[:3, :3] @ np.array(scene_cfg["eval_bbx"][1], dtype=np.float64) + gt_to_sfm[:3, 3]
    return np.minimum(v1, v2), np.maximum(v1, v2)


def appearance_of(text):
    return text if text in ("mean", "view") else int(text)


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch

    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import config as C
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import ply, surfcloud, trainer, views

    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    cfg = C.load_config(args.cfg_path, {"DATASET": {"ROOT_DIR": args.root_dir}} if args.root_dir else None)
    prec = {None: None, "bf16": nw.PREC_BF16, "f16": nw.PREC_F16, "f32": nw.PREC_F32}[args.prec]
    emb, neuconw, nerf, rdr, scene_cfg = C.build_system(cfg, dev, prec)
    trainer.load_checkpoint(args.ckpt_path, emb, neuconw, nerf)
    for m in (emb, neuconw, nerf):
        m.eval()
    root = cfg["DATASET"]["ROOT_DIR"]
    downscale = args.img_downscale if args.img_downscale is not None else int(cfg["DATASET"]["PHOTOTOURISM"]["IMG_DOWNSCALE"])
    # scene_view(load_image=False) per row, with the scene files read once (its own pieces: read_scene / image_pose / image_near_far)
    scene = views.read_scene(root, args.sfm_path)
    ids = select_ids(scene, args.split, args.view_stride, args.max_views)
    if not ids:
        raise SystemExit("no view selected: %s lists no %s image registered in %s" % (scene["tsv"], args.split, scene["sp"]))
    cams = []
    for iid in ids:
        K, w2c, c2w, w_, h_ = views.image_pose(scene, iid, downscale)
        near, far = views.image_near_far(scene, w2c)
        cams.append((views.Camera(K, c2w, w_, h_, near, far), iid))
    radius = float(scene_cfg["radius"])
    cell = args.cell if args.cell is not None else 2.0 * radius / 1024.0
    lo, hi = grid_box(scene_cfg, args.box)
    cloud = surfcloud.SurfaceCloud(lo, hi, cell, scale=radius, offset=scene_cfg["origin"],
                                   cos_min=args.cos_min if args.cos_min >= 0 else None, device=dev)
    app = appearance_of(args.appearance)
    if isinstance(app, int):
        app = emb.weight[app].detach().float()
    L.PROFILE = {}  # device events around every entry point: the ms per stage of the report
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tot = surfcloud.fuse_views(rdr, cams, cloud, appearance=app, chunk=args.chunk, eps=args.trace_eps, max_iter=args.trace_iters,
                               step=args.trace_step, far_override=bool(cfg["NEUCONW"]["NEAR_FAR_OVERRIDE"]))
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    out = cloud.finish(min_views=args.min_views, min_count=args.min_count)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    prof, L.PROFILE = L.PROFILE, None
    stage = {}
    for name, evs in prof.items():
        key = ("fuse" if name.startswith("ncw_fuse_") else "trace" if name.startswith(("ncw_trace_", "ncw_view_", "ncw_ray_"))
               else "networks")
        stage[key] = stage.get(key, 0.0) + sum(a.elapsed_time(b) for a, b in evs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ply.write(args.out, out["positions"].cpu().numpy(), rgb=out["colours"].cpu().numpy(), normals=out["normals"].cpu().numpy())
    st = cloud.stats()
    n = float(max(1, tot["rays"]))
    report = {"views": tot["views"], "image_ids": ids, "rays": tot["rays"], "cell": cell,
              "box": [list(map(float, lo)), list(map(float, hi))], "dims": [int(d) for d in cloud.dims],
              "state_share": {k: tot[k] / n for k in ("hit", "miss", "inside", "stalled")},
              "samples": tot["samples"], "samples_valid": st["valid"], "samples_invalid": st["invalid"], "cells": st["cells"],
              "cells_kept": int(out["keys"].numel()), "cells_degenerate": out["degenerate"], "growths": st["growths"],
              "capacity": st["capacity"], "table_bytes": st["table_bytes"], "min_views": args.min_views, "cos_min": cloud.cos_min,
              "appearance": args.appearance,
              "ms": {"views_wall": 1e3 * (t1 - t0), "resolve_wall": 1e3 * (t2 - t1),
                     "device_trace": stage.get("trace", 0.0), "device_networks": stage.get("networks", 0.0),
                     "device_fuse": stage.get("fuse", 0.0)}}
    with open(args.out + ".report.json", "w") as fh:
        json.dump(report, fh, indent=1)
    print("%d views, %d rays (hit %.1f %%), %d samples (%d valid) -> %d cells, %d kept (min_views %d) -> %s; %.1f ms per view, "
          "fusion %.2f ms per view"
          % (tot["views"], tot["rays"], 100 * tot["hit"] / n, tot["samples"], st["valid"], st["cells"], report["cells_kept"],
             args.min_views, args.out, 1e3 * (t1 - t0) / max(1, tot["views"]), stage.get("fuse", 0.0) / max(1, tot["views"])))


if __name__ == "__main__":
    main()
