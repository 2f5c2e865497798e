"""PL-free training driver on a real scene (SURVEY 8f N4 + N3): the reference's `train.py` / `NeuconWSystem` recipe
(train.py:16-64, neuconw_system.py:60-184, 266-400) without PyTorch-Lightning 1.4.8 -- one process per GPU.

    python scripts/train.py --cfg_path config/train_brandenburg_gate.yaml --root_dir data/heritage-recon/brandenburg_gate \
        --batch_size 2048 --num_epochs 20 --exp_name bg            (N GPUs: python -m torch.distributed.run --nproc-per-node N ...)

  * experiment yaml + scene config.yaml as the reference reads them (neuralrecon_w_amd.config);
  * this rank's share of the npz ray-cache chunks (datasets/data.py:83-119) uploaded to HBM once, batches assembled on
    the device, black-listed labels (RAY_MASK_LIST) removed once at load time -> fixed-size, sync-free steps;
  * --ray_source scene (opt-in): no cache files -- the scene's images, COLMAP model and label maps become 8-byte records on the
    device and every batch's rows are rebuilt by one launch (neuralrecon_w_amd.raysource); same rows, same steps;
  * Adam(eps 1e-7), lr = CANONICAL_LR * world * batch / CANONICAL_BS, grad-norm clip 0.99, ONE flat RCCL all-reduce;
  * cos_anneal_ratio = min(1, step / ANNEAL_END); every UPDATE_FREQ steps the fine octree is rebuilt from the current SDF
    (coarse octree from the COLMAP points: voxel.octree_from_sfm); checkpoints every SAVE_FREQ steps in the reference's
    PyTorch-Lightning layout (state_dict keys + torch.optim.Adam optimizer state), readable by its load_ckpt;
  * LR_SCHEDULER none / cosine / steplr stepped per epoch like PL steps the reference's scheduler (config.lr_at_epoch);
  * --val_mesh_every N (opt-in): every N steps the meshes of the reference's validation_step (neuconw_system.py:466-530) --
    128^3 over the unit sphere and 256^3 over `eval_bbx_detail` -- go to <SAVE_DIR>/<exp_name>/meshes/, and when
    <root_dir>/gt.ply exists rank 0 scores the detailed one at 0.1 (neuralrecon_w_amd.evalmesh);
  * --val_every N (opt-in): every N steps rank 0 renders the validation view (the dataset's `val` item: first training image,
    downscale >= 8; neuconw_system.py:404-464, 533-546) with the forward-only render, prints val/psnr and writes the
    GT | prediction | depth | normal panel to <SAVE_DIR>/<exp_name>/val/<step:08d>.png (neuralrecon_w_amd.views).  It draws no
    random numbers and touches no training state: the training stream computes what it computes without it.
"""
import argparse
import os
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import neuralrecon_w_amd as nw  # noqa: E402
from neuralrecon_w_amd import config as C  # noqa: E402
from neuralrecon_w_amd import raycache, trainer, voxel  # noqa: E402


def validation_meshes(rdr, scene, root, save_dir, step, rank, log_detail_skip=True):
    """neuconw_system.py:466-530: the 128^3 mesh over the unit sphere and the 256^3 mesh over the scene's eval_bbx_detail
    (carried into SfM space by inv(sfm2gt)), extracted on EVERY rank (the grid sweep is collective); rank 0 writes
    meshes/<step:08d>.ply and <step:08d>_detail.ply and, when <root>/gt.ply exists, scores the detailed mesh at 0.1
    (evalmesh.eval_mesh, is_mesh=False, bbx_name=eval_bbx_detail).  Returns the metrics dict or None."""
    import numpy as np

    from neuralrecon_w_amd import evalmesh, mesh

    mesh_dir = os.path.join(save_dir, "meshes")
    m = mesh.extract_mesh(rdr, 128, scene["radius"], scene["origin"], with_color=False)
    if rank == 0:
        os.makedirs(mesh_dir, exist_ok=True)
        mesh.write_ply(os.path.join(mesh_dir, "%08d.ply" % step), m["vertices"], m["faces"])
    if "eval_bbx_detail" not in scene:
        if rank == 0 and log_detail_skip:
            print("[val] step %d: the scene config has no eval_bbx_detail: detail mesh and evaluation skipped" % step)
        return None
    gt_to_sfm = np.linalg.inv(np.array(scene["sfm2gt"], dtype=np.float64))
    v1 = gt_to_sfm[:3, :3] @ np.array(scene["eval_bbx_detail"][0], dtype=np.float64) + gt_to_sfm[:3, 3]
    v2 = gt_to_sfm[:3, :3] @ np.array(scene["eval_bbx_detail"][1], dtype=np.float64) + gt_to_sfm[:3, 3]
    bmin, bmax = np.minimum(v1, v2), np.maximum(v1, v2)
    centre, half = (bmax + bmin) / 2, np.max(bmax - bmin) / 2
    so, radius = np.asarray(scene["origin"], dtype=np.float64), float(scene["radius"])
    md = mesh.extract_mesh(rdr, 256, radius, scene["origin"], origin=((centre - so) / radius).tolist(), radius=half / radius,
                           with_color=False)
    if rank != 0:
        return None
    detail = os.path.join(mesh_dir, "%08d_detail.ply" % step)
    mesh.write_ply(detail, md["vertices"], md["faces"])
    gt_path = os.path.join(root, "gt.ply")
    if not os.path.exists(gt_path):
        return None
    met = evalmesh.eval_mesh(detail, gt_path, scene, is_mesh=False, threshold=0.1, bbx_name="eval_bbx_detail", verbose=False)
    print("[val] step %d: prec %.6f recal %.6f fscore %.6f" % (step, met["prec"], met["recal"], met["fscore"]))
    return met


def validation_view(rdr, cfg, view, save_dir, step, chunk):
    """neuconw_system.py:404-464, 533-546 on rank 0: renders `view` = (camera, gt, image id) of views.scene_view, prints
    val/psnr (+ ssim) and writes val/<step:08d>.png.  Returns the render_view dictionary."""
    from neuralrecon_w_amd import views

    cam, gt, image_id = view
    out = views.render_view(rdr, cam, ts=image_id, chunk=chunk, gt=gt,
                            nerf_far_override=bool(cfg["NEUCONW"]["NEAR_FAR_OVERRIDE"]))  # :407
    path = os.path.join(save_dir, "val", "%08d.png" % step)
    views.write_panel(path, gt, out["color"], out["depth_vis"], out["normal"])
    print("[val] step %d: val/psnr %.4f  val/ssim %.4f  (image %d, %d x %d) -> %s"
          % (step, float(out["psnr"]), float(out["ssim"]), image_id, cam.width, cam.height, path))
    return out


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg_path", required=True)
    ap.add_argument("--root_dir", default=None, help="overrides DATASET.ROOT_DIR")
    ap.add_argument("--batch_size", type=int, default=2048, help="rays per GPU per step (scripts/train.sh: 2048)")
    ap.add_argument("--num_epochs", type=int, default=20)
    ap.add_argument("--max_steps", type=int, default=0, help="stop after this many steps (0 = run the epochs out)")
    ap.add_argument("--exp_name", default="exp")
    ap.add_argument("--prec", default=None, choices=["bf16", "f16", "f32"],
                    help="training precision; default = the package default (NEUCONW_PREC, f16: neuconw.default_prec)")
    ap.add_argument("--ckpt_path", default="", help="resume from this checkpoint")
    ap.add_argument("--log_every", type=int, default=100)
    ap.add_argument("--val_mesh_every", type=int, default=0,
                    help="every N steps: validation meshes (128^3 + 256^3 eval_bbx_detail) and, with <root_dir>/gt.ply, "
                         "their F-score at 0.1 (0 = off)")
    ap.add_argument("--val_every", type=int, default=0,
                    help="every N steps rank 0 renders the validation view, prints val/psnr and writes the GT | prediction | "
                         "depth | normal panel to <SAVE_DIR>/<exp_name>/val/ (0 = off)")
    ap.add_argument("--val_chunk", type=int, default=0, help="rays per render launch of --val_every (0 = views.DEFAULT_CHUNK)")
    ap.add_argument("--val_sfm_path", default=None,
                    help="COLMAP model of --val_every under <root_dir>/dense/ -- the one the ray cache was built from (default: the "
                         "reference's per-scene choice, ../neuralsfm for brandenburg_gate and palacio_de_bellas_artes, else sparse)")
    ap.add_argument("--ray_source", default="cache", choices=["cache", "scene"],
                    help="cache: the npz ray cache under DATASET.PHOTOTOURISM.CACHE_DIR (scripts/prepare_data_cache.py); scene: no cache -- rays are "
                         "rebuilt per batch on the GPU from the scene directory itself (neuralrecon_w_amd.raysource)")
    ap.add_argument("--semantic_map_path", default=None,
                    help="--ray_source scene: directory of the label maps under the scene (default: DATASET.PHOTOTOURISM."
                         "SEMANTIC_MAP_PATH, 'semantic_maps', when the config has WITH_SEMANTICS)")
    ap.add_argument("--sfm_path", default=None,
                    help="--ray_source scene: COLMAP model under <root_dir>/dense/ (default: the reference's per-scene choice)")
    ap.add_argument("--depth_percent", type=float, default=None,
                    help="--ray_source scene: share of rays with a key-point depth each image is padded up to (default: the "
                         "reference's per-scene value)")
    ap.add_argument("--source_seed", type=int, default=0, help="--ray_source scene: seed of the depth_percent padding draws")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.ckpt_path:
        # the interrupted epoch's permutation indexes the rows of the source it was drawn for; the other source holds another
        # row set in another order.  Checked before anything is built.
        kind = (torch.load(args.ckpt_path, map_location="cpu").get("ncw_resume") or {}).get("ray_source", "cache")
        if kind != args.ray_source:
            raise SystemExit("%s was written with --ray_source %s: resuming it with --ray_source %s would permute a different set "
                             "of rays; pass --ray_source %s" % (args.ckpt_path, kind, args.ray_source, kind))
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("NCW_TRAIN_ONE_GPU_TEST"):  # plumbing test: the ranks share GPU 0 (collectives over gloo)
        local = 0
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        backend = os.environ.get("NCW_DIST_BACKEND", "nccl")  # nccl = RCCL over xGMI
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    dev = torch.device("cuda", local)
    cfg = C.load_config(args.cfg_path, {"DATASET": {"ROOT_DIR": args.root_dir}} if args.root_dir else None)
    lr = C.scale_lr(cfg, world, args.batch_size)
    torch.manual_seed(cfg["TRAINER"]["SEED"])  # pl.seed_everything (train.py:18): identical initial weights on every rank
    prec = {None: None, "bf16": nw.PREC_BF16, "f16": nw.PREC_F16, "f32": nw.PREC_F32}[args.prec]
    emb, neuconw, nerf, rdr, scene = C.build_system(cfg, dev, prec)
    rdr.sync_free = True
    n, pt = cfg["NEUCONW"], cfg["DATASET"]["PHOTOTOURISM"]
    root = cfg["DATASET"]["ROOT_DIR"]
    if args.ray_source == "scene":
        from neuralrecon_w_amd import raysource

        sem_path = args.semantic_map_path
        if sem_path is None and pt["WITH_SEMANTICS"]:
            sem_path = pt.get("SEMANTIC_MAP_PATH") or "semantic_maps"
        cache = raysource.RaySource.from_scene(root, img_downscale=pt["IMG_DOWNSCALE"], semantic_map_path=sem_path,
                                               sfm_path=args.sfm_path, seed=args.source_seed, depth_percent=args.depth_percent,
                                               ray_mask_list=n["RAY_MASK_LIST"], prefilter=True, world_size=world, rank=rank,
                                               device=dev)
    else:
        names = raycache.local_splits(raycache.list_splits(root, pt["CACHE_DIR"]), world, rank)
        cache = raycache.RayCache(root, pt["CACHE_DIR"], names, dev, img_downscale=pt["IMG_DOWNSCALE"],
                                  with_semantics=pt["WITH_SEMANTICS"], ray_mask_list=n["RAY_MASK_LIST"], prefilter=True)
    # Every rank runs the SAME number of steps per epoch: with the black-listed rays removed at load time the ranks'
    # caches differ in length, and a rank that leaves the loop early would strand the others in the gradient all-reduce
    # (the reference pads its chunks to equal length and filters inside the batch: datasets/data.py:83-119).
    steps_per_epoch = len(cache) // args.batch_size
    if world > 1:
        t = torch.tensor([steps_per_epoch], device=dev, dtype=torch.int64)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        steps_per_epoch = int(t.item())
    if steps_per_epoch < 1:
        raise SystemExit("a rank holds fewer than --batch_size rays (%d)" % len(cache))
    if rank == 0 and args.ray_source == "scene":
        print("[rank 0] ray source: scene (%d images), %d rays resident on %s at %.2f B/ray; %d steps/epoch; lr %.3g"
              % (cache.n_img, len(cache), dev, cache.nbytes() / max(1, len(cache)), steps_per_epoch, lr))
    elif rank == 0:
        print("[rank 0] %d cache chunk(s), %d rays resident on %s; %d steps/epoch; lr %.3g"
              % (len(names), len(cache), dev, steps_per_epoch, lr))
    step_fn = nw.TrainStep(rdr, [emb, neuconw, nerf], C.neuconw_loss(cfg), lr=lr, eps=1e-7, clip=0.99, world_size=world)
    order = trainer.reference_param_order(emb, neuconw, nerf)
    step, resume = 0, None
    if args.ckpt_path:
        ck = trainer.load_checkpoint(args.ckpt_path, emb, neuconw, nerf, flat_params=step_fn.fp)
        step = int(ck.get("global_step", 0))
        if ck.get("optimizer_states"):
            step_fn.opt.load_state_dict(ck["optimizer_states"][0], order)
        resume = ck.get("ncw_resume")
    update_freq = int(n["UPDATE_FREQ"])
    train_level = C.surface_level(n["TRAIN_VOXEL_SIZE"], scene["eval_bbx"]) if update_freq > 0 else None
    save_dir = os.path.join(cfg["TRAINER"]["SAVE_DIR"], args.exp_name)
    bg = torch.zeros(1, 3, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(cfg["TRAINER"]["SEED"] + rank)
    t0, t_last, done = time.perf_counter(), time.perf_counter(), False
    # Resume: continue the interrupted epoch where it stopped -- same permutation (the generator goes back to its state at
    # the start of that epoch), the consumed batches skipped, the fp16 loss scale and its counters restored -- so a resumed
    # run executes the same steps as an uninterrupted one.  (Checkpoints without `ncw_resume`, e.g. the reference's own:
    # the epoch restarts from its first batch with a fresh generator, as before.)
    first_epoch, skip = step // steps_per_epoch, 0
    if resume is not None:
        first_epoch, skip, gstate = trainer.apply_resume_state(resume, step_fn.opt, rdr)
        if world > 1:  # per-rank generator states are not in rank 0's checkpoint: only rank 0 continues its permutation
            gstate = gstate if rank == 0 else None
        if gstate is not None:
            gen.set_state(gstate.to(gen.get_state().device))
        if skip >= steps_per_epoch:  # the checkpoint was written after the LAST batch of its epoch: consume that epoch's
            torch.randperm(len(cache), device=dev, generator=gen)  # permutation draw, the next epoch then draws its own
            first_epoch, skip = first_epoch + 1, 0
    if resume is not None and update_freq > 0 and step >= update_freq:
        # the fine octree is not part of a checkpoint: rebuild it from the restored SDF (identical to the uninterrupted run's
        # when the checkpoint was written right after a refresh, i.e. at a multiple of UPDATE_FREQ steps)
        if rdr.octree_data is None:  # normally built by the first render (NEAR_FAR_OVERRIDE) -- here before any
            rdr.octree_data = rdr.get_octree(dev)
        voxel.octree_update(rdr, train_level, n["SDF_THRESHOLD"])
    sched_kind = cfg["TRAINER"].get("LR_SCHEDULER", "none")

    def sched_state(epoch_):  # torch _LRScheduler.state_dict() entries PL restores (utils/__init__.py:45-61)
        if sched_kind in (None, "none"):
            return None
        cur = C.lr_at_epoch(cfg, lr, epoch_, args.num_epochs)
        return {"last_epoch": int(epoch_), "_step_count": int(epoch_) + 1, "_last_lr": [cur], "base_lrs": [lr], "kind": sched_kind}

    def resume_extra(epoch_, in_epoch_, gstate_):
        st = trainer.resume_state(step_fn.opt, rdr, epoch_, in_epoch_, gstate_)
        st["ray_source"] = args.ray_source
        return {"ncw_resume": st}

    # bound before the loop: a checkpoint whose epoch is already >= --num_epochs (or a loop whose body never runs) still
    # writes last.ckpt below
    epoch, in_epoch, gen_state0 = first_epoch, skip, gen.get_state()
    val_logged = False  # the "no eval_bbx_detail" line is printed once
    val_view = None
    if args.val_every > 0 and rank == 0:  # the dataset's `val` item, read once (data.py:80: no scene origin -> SfM percentiles)
        from neuralrecon_w_amd import views

        cam_, gt_, id_ = views.scene_view(root, img_downscale=int(pt["IMG_DOWNSCALE"]), split="val", sfm_path=args.val_sfm_path)
        val_view = (cam_, gt_.to(dev), id_)
    for epoch in range(first_epoch, args.num_epochs):
        if hasattr(step_fn.opt, "lr"):  # utils/__init__.py:45-61: the scheduler steps once per epoch
            step_fn.opt.lr = C.lr_at_epoch(cfg, lr, epoch, args.num_epochs)
        gen_state0 = gen.get_state()  # the permutation of this epoch is drawn from here
        in_epoch = skip if epoch == first_epoch else 0
        for b in cache.epoch(args.batch_size, generator=gen, drop_last=True, max_batches=steps_per_epoch, skip_batches=in_epoch):
            rdr.nerf_far_override = False  # neuconw_system.py:343: training always reads near / far from the cache
            ratio = 1.0 if n["ANNEAL_END"] == 0 else min(1.0, step / n["ANNEAL_END"])
            loss, out = step_fn(b["rays"], b["ts"], b["semantics"], b["rgbs"], background_rgb=bg, cos_anneal_ratio=ratio)
            if update_freq > 0 and (step + 1) % update_freq == 0:  # :361-365
                voxel.octree_update(rdr, train_level, n["SDF_THRESHOLD"])
            in_epoch += 1
            if step % cfg["TRAINER"]["SAVE_FREQ"] == 0 and rank == 0:  # :367-374  (written AFTER the step: global_step + 1 done)
                os.makedirs(save_dir, exist_ok=True)
                trainer.save_checkpoint(os.path.join(save_dir, "iter_%d.ckpt" % step), emb, neuconw, nerf,
                                        optimizer=step_fn.opt, global_step=step + 1, epoch=epoch, lr_scheduler=sched_state(epoch),
                                        extra=resume_extra(epoch, in_epoch, gen_state0))
            if rank == 0 and step % args.log_every == 0:
                now = time.perf_counter()
                gn = float(getattr(step_fn, "last_grad_norm", float("nan")))
                print("epoch %d step %d  loss %.5f  s_val %.5f  |grad| %.4g  (%.1f ms/step)%s"
                      % (epoch, step, float(loss), float(out["s_val"]), gn, 1e3 * (now - t_last) / max(1, args.log_every),
                         "" if gn == gn and abs(gn) != float("inf") else
                         "  <- non-finite gradient norm: this update was skipped and the fp16 loss scale halved (now %g; "
                         "%d skipped so far)" % (rdr.grad_scale, step_fn.opt.skipped_steps)))
                t_last = now
            step += 1
            if args.val_mesh_every > 0 and step % args.val_mesh_every == 0:  # neuconw_system.py:466-530
                validation_meshes(rdr, scene, root, save_dir, step, rank, log_detail_skip=not val_logged)
                val_logged = True
            if val_view is not None and step % args.val_every == 0:  # neuconw_system.py:404-464, 533-546 (rank 0)
                validation_view(rdr, cfg, val_view, save_dir, step, args.val_chunk or views.DEFAULT_CHUNK)
            if args.max_steps and step >= args.max_steps:
                done = True
                break
        if done:
            break
    torch.cuda.synchronize()
    if rank == 0:
        os.makedirs(save_dir, exist_ok=True)
        trainer.save_checkpoint(os.path.join(save_dir, "last.ckpt"), emb, neuconw, nerf, optimizer=step_fn.opt, global_step=step,
                                epoch=epoch, lr_scheduler=sched_state(epoch),
                                extra=resume_extra(epoch, in_epoch, gen_state0))
        print("%d steps in %.1f s; wrote %s" % (step, time.perf_counter() - t0, os.path.join(save_dir, "last.ckpt")))
    print("[rank %d] finished after %d steps with %d rays resident" % (rank, step, len(cache)))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
