"""Held-out views: fit the appearance code on frozen geometry, score PSNR -- the NeRF-W evaluation protocol.

A test image has no trained row in the appearance embedding, so its PSNR cannot be read off the checkpoint.  The reference's
dataset hands out every test image as a left half to fit on and a right half to score (datasets/phototourism.py:520-556,
726-748: `rays_train` / `rgbs_train_gt`, `rays_eval` / `rgbs_eval_gt`) and nothing ever consumes it; this module does:

    res = eval_view(rdr, camera, gt)                      # fit on the left half, render, score the right half
    res = eval_views(root_dir, cfg, ckpt)                 # every `test` row of the scene's split file

With every network weight frozen and perturb = 0 the sample depths, the SDF values / gradients / features, the NeuS weights and
the background densities are constants of a ray: `freeze_rays` computes them once.  Only the colour network and the background
NeRF's colour head see the code, and the rendered colour is linear in their outputs, so an iteration of `AppearanceFit` is:
colour forward, background forward, `ncw_appfit_loss` (compose + L1 + adjoints), the two data-path backwards with per-point code
adjoints, and `ncw_appfit_step` (order-fixed reduction, non-finite guard, Adam on n_a floats, broadcast) -- no sampler, no SDF
pass, no compositor backward, no weight-gradient GEMM, and no parameter's `.grad` is touched.

`steps` and `lr` are this project's choice: the reference has no consumer of its `eval` item that could fix them.
"""
import ctypes as C
import json
import os

import numpy as np
import torch

from . import lib as L
from . import rayops
from .neuconw import points_struct
from .packing import pack_many
from .stash import StashArena, StashCache

DEFAULT_STEPS = 200   # full-batch Adam iterations per view (ours: see the module docstring)
DEFAULT_LR = 0.02     # Adam's step bound: a component moves at most steps * lr = 4, the scale of an N(0, 1) embedding row
DEFAULT_N_RAYS = 8192


# -----------------------------------------------------------------------------------------------------------------------
# host side: which pixels, which images
# -----------------------------------------------------------------------------------------------------------------------
def half_pixel_indices(width, height):
    """Row-major pixel indices (left, right) of the columns [0, W // 2) and [W // 2, W): the slicing of
    datasets/phototourism.py:728-733 (an odd width gives the right half the extra column)."""
    width, height = int(width), int(height)
    idx = np.arange(width * height, dtype=np.int64).reshape(height, width)
    return idx[:, : width // 2].reshape(-1), idx[:, width // 2:].reshape(-1)


def ray_subset(width, height, n_rays, seed=0):
    """A seeded subset of `n_rays` left-half pixels (all of them if there are fewer), ascending."""
    left, _ = half_pixel_indices(width, height)
    if n_rays is None or int(n_rays) >= left.size:
        return left
    pick = np.random.default_rng(int(seed)).choice(left.size, int(n_rays), replace=False)
    return left[np.sort(pick)]


def held_out_rows(root_dir):
    """File names of the `test` rows of the scene's split file (scripts/prepare_data_split.py writes them), in file order."""
    from . import colmap

    _, rows = colmap.split_rows(root_dir)
    return [r["filename"] for r in rows if r.get("split") == "test"]


# -----------------------------------------------------------------------------------------------------------------------
# frozen geometry
# -----------------------------------------------------------------------------------------------------------------------
class FrozenRays:
    """The constants of one ray chunk.  Holds the lease of the SDF network's forward-only stash (its `feat` vector is the colour
    network's input) until `release()` or garbage collection."""

    def release(self):
        StashCache.release(self.__dict__.pop("sdf_lease", None))

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def _use_bg(rdr):
    return bool(rdr.render_bg and rdr.n_outside > 0)


def _bg_choice(rdr, z, n_out):
    """(select, refine) exactly as _RenderFn.forward chooses them."""
    select = refine = None
    if rdr.trim_sphere:
        refine = (z, n_out)
        if not rdr.bg_dense:
            select = refine
    return select, refine


@torch.no_grad()
def freeze_rays(rdr, rays, background_rgb=None, chunk=1024, cos_anneal_ratio=0.0, far_override=None):
    """Everything of render() that does not depend on the appearance code, once per ray: ray prologue, the sampler at perturb 0,
    the forward-only SDF pass (sdf, gradients, feat), the background pass for its densities and the compositor, of whose outputs
    `weights`, `inside`, `weights_sum` (and `z_feed`) are kept.  rays [R, >= 8] on the GPU -> a list of FrozenRays, `chunk` rays
    each.  cos_anneal_ratio / far_override: as render() / views.render_view take them (defaults: theirs)."""
    if not (torch.is_tensor(rays) and rays.is_cuda):
        raise L.NeuconwHipError("appfit.freeze_rays: rays are not on a GPU; the hot path has no CPU fallback")
    dev, prec, lib = rays.device, rdr.prec, L.get_lib()
    neuconw, nerf = rdr.neuconw, rdr.nerf
    if rdr.origin.device != dev:
        rdr.origin = rdr.origin.to(dev).float()
        rdr.sfm_to_gt = rdr.sfm_to_gt.to(dev).float()
    use_bg = _use_bg(rdr)
    if rdr.__dict__.get("sampler_prec") is None:
        pack_many([(m, m.plan(prec)) for m in [neuconw.sdf_net, neuconw.color_net] + ([nerf] if use_bg else [])])
    origin = (C.c_float * 3)(*[float(v) for v in rdr.origin.reshape(-1).tolist()])
    n_a = int(neuconw.color_net.n_a)
    bgc = None
    if background_rgb is not None:
        if background_rgb.numel() != 3:
            raise ValueError("background_rgb must hold ONE colour (3 values): got shape %s" % (tuple(background_rgb.shape),))
        bgc = background_rgb.detach().to(dev).reshape(3).float().contiguous()
    variance = neuconw.deviation_network.variance
    inv_s, s_val = torch.empty(1, device=dev), torch.empty(1, device=dev)
    L.check(lib.ncw_inv_s_fwd(L.ptr(variance.detach().reshape(1).float().contiguous()), L.ptr(inv_s), L.ptr(s_val),
                              L.stream_ptr(dev)), "ncw_inv_s_fwd")
    rays = rays.contiguous().float()
    out = []
    for r0 in range(0, rays.shape[0], max(1, int(chunk))):
        rc = rays[r0:r0 + max(1, int(chunk))].contiguous()
        R = rc.shape[0]
        rays_o, rays_d = torch.empty(R, 3, device=dev), torch.empty(R, 3, device=dev)
        near, far = torch.empty(R, 1, device=dev), torch.empty(R, 1, device=dev)
        dgt, dw = torch.empty(R, device=dev), torch.empty(R, device=dev)
        L.check(lib.ncw_ray_prologue(L.ptr(rc), rc.shape[1], R, origin, float(rdr.radius), L.ptr(rays_o), L.ptr(rays_d),
                                     L.ptr(near), L.ptr(far), L.ptr(dgt), L.ptr(dw), L.stream_ptr(dev)), "ncw_ray_prologue")
        _, z, z_out, sample_dist = rdr.sparse_sampler(rays_o, rays_d, near, far, 0, None, far_override)
        S = z.shape[1]
        g = FrozenRays()
        g.R, g.S, g.use_bg, g.background_rgb = R, S, bool(use_bg and z_out is not None), bgc
        a0 = torch.zeros(R, n_a, device=dev)  # the constants do not depend on the code: any will do
        z_feed = density = bg_rgb = None
        g.O = 0
        if g.use_bg:
            g.O = z_out.shape[1]
            g.select, g.refine = _bg_choice(rdr, z, g.O)
            z_feed, _ = rayops.sort_merge(z, z_out)
            g.pts_bg = points_struct(rays_o=rays_o, rays_d=rays_d, z=z_feed, sample_dist=sample_dist, mode=2)
            density, bg_rgb, nctx = nerf.fwd_stash(g.pts_bg, R * (S + g.O), prec, a0, select=g.select, train=False, refine=g.refine)
            StashCache.release(nctx["lease"])
            density, bg_rgb = density.view(R, S + g.O), bg_rgb.view(R, S + g.O, 3)
        g.M = S + g.O
        g.pts_in = points_struct(rays_o=rays_o, rays_d=rays_d, z=z, sample_dist=sample_dist, mode=2)
        sdf, grad, sctx = neuconw.sdf_net.fwd_stash(g.pts_in, R * S, prec, train=False)
        g.sdf_lease, g.sdf_arena = sctx["lease"], sctx["arena"]
        g.feat_ptr = sctx["arena"].ptr(sctx["ids"]["feat"])
        g.grad = grad
        comp = rayops.CompositeCtx(rays_o, rays_d, z, sample_dist, sdf.view(R, S), grad.view(R, S, 3),
                                   torch.zeros(R, S, 3, device=dev), inv_s, cos_anneal_ratio, z_feed, density, bg_rgb, bgc,
                                   rdr.trim_sphere)
        o = comp.forward()
        g.weights, g.inside, g.weights_sum, g.z_feed, g.z = o["weights"], o["inside"], o["weights_sum"], z_feed, z
        out.append(g)
    return out


def release_contexts(contexts):
    for g in contexts:
        g.release()


def dead_sample_share(contexts):
    """Share of the frozen samples whose weight is exactly 0 (a later compaction of dead samples would be judged by it)."""
    dead = sum(int((g.weights == 0).sum()) for g in contexts)
    return dead / float(max(1, sum(g.weights.numel() for g in contexts)))


# -----------------------------------------------------------------------------------------------------------------------
# the fit
# -----------------------------------------------------------------------------------------------------------------------
class AppearanceFit:
    """Full-batch Adam on ONE appearance code over frozen rays.

        fit = AppearanceFit(rdr, contexts, targets, init, lr)
        for _ in range(steps):
            loss = fit.loss_and_grad()      # device scalar: sum |color - target| / (R + 1e-5), losses.py:25-27
            fit.step()
        fit.code                            # [n_a]

    Every iteration sees every frozen ray, so the loss is a deterministic function of the code; every reduction has a fixed
    order (no atomics), so two fits from one start are bitwise identical.  fp16 mode: the cotangents carry a private loss-scale
    pair that starts at the renderer's initial scale and halves after a step with a non-finite gradient (`skipped_steps`).
    eps defaults to the training recipe's 1e-7 (utils/__init__.py:23-31)."""

    def __init__(self, rdr, contexts, targets, init, lr=DEFAULT_LR, betas=(0.9, 0.999), eps=1e-7):
        if not contexts:
            raise ValueError("AppearanceFit: no frozen rays")
        if not (torch.is_tensor(targets) and targets.is_cuda and torch.is_tensor(init) and init.is_cuda):
            raise L.NeuconwHipError("AppearanceFit: targets / init are not on a GPU; the hot path has no CPU fallback")
        self.rdr, self.ctxs = rdr, list(contexts)
        dev = targets.device
        self.dev, self.prec = dev, rdr.prec
        self.n_a = n_a = int(rdr.neuconw.color_net.n_a)
        self.R_total = sum(g.R for g in self.ctxs)
        self.targets = targets.detach().reshape(-1, 3).float().contiguous()
        if self.targets.shape[0] != self.R_total:
            raise ValueError("AppearanceFit: %d targets for %d frozen rays" % (self.targets.shape[0], self.R_total))
        if init.numel() != n_a:
            raise ValueError("AppearanceFit: the code holds %d values, the networks take %d" % (init.numel(), n_a))
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.inv_denom = 1.0 / (self.R_total + 1e-5)
        self.code = init.detach().reshape(n_a).float().clone().contiguous()
        self.exp_avg, self.exp_avg_sq = torch.zeros(n_a, device=dev), torch.zeros(n_a, device=dev)
        self.grad_acc = torch.zeros(n_a, device=dev)
        self.state = torch.zeros(8, device=dev, dtype=torch.int32)  # NcwAdamState
        self.scale = None
        if self.prec == L.PREC_F16:
            s0 = float(rdr.loss_scale.init)
            self.scale = torch.tensor([s0, 1.0 / s0], device=dev, dtype=torch.float32)
        Rm = max(g.R for g in self.ctxs)
        nS, nM = max(g.R * g.S for g in self.ctxs), max(g.R * g.M for g in self.ctxs)
        any_bg = any(g.use_bg for g in self.ctxs)
        self.a_rows = self.code.reshape(1, n_a).expand(Rm, n_a).contiguous()  # what the forward launches read per ray
        self.color = torch.empty(self.R_total, 3, device=dev)
        self.ray_loss = torch.zeros(self.R_total, device=dev)
        # buffers shared by the chunks (one stream: a chunk is finished before the next begins)
        self.d_rgb, self.rows = torch.empty(nS, 3, device=dev), torch.empty(nS, n_a, device=dev)
        # what the existing backward writes and nobody reads here: d(normals) is ADDED into d_grad, d(feat) is stored
        self.d_grad = torch.zeros(nS, 3, device=dev)
        rbf = int(rdr.neuconw.color_net.d_feature) // 32
        self.dfeat = StashArena(dev, self.prec, nS)
        self.dfeat.new(rbf)
        self.dfeat.allocate()
        if any_bg:
            self.d_bg_rgb, self.rows_bg = torch.empty(nM, 3, device=dev), torch.empty(nM, n_a, device=dev)
            self.d_density = torch.zeros(nM, device=dev)
        lib = L.get_lib()
        self.scratch = torch.empty(max(1, int(lib.ncw_appfit_step_scratch_floats(max(nS, nM), n_a))), device=dev)

    # ---- one pass over the frozen rays ---------------------------------------------------------------------------------
    def _step_call(self, rows, n, accumulate, final):
        dev = self.dev
        L.check(L.get_lib().ncw_appfit_step(L.ptr(rows), int(n), self.n_a, L.ptr(self.scratch), L.ptr(self.grad_acc),
                                            int(accumulate), int(final), L.ptr(self.code), L.ptr(self.exp_avg),
                                            L.ptr(self.exp_avg_sq), L.ptr(self.state), self.lr, self.betas[0], self.betas[1],
                                            self.eps, L.ptr(self.scale), 1.0, L.ptr(self.a_rows), self.a_rows.shape[0],
                                            L.stream_ptr(dev)), "ncw_appfit_step")

    def _pass(self, backward):
        rdr, prec, lib, dev, n_a = self.rdr, self.prec, L.get_lib(), self.dev, self.n_a
        color_net, nerf = rdr.neuconw.color_net, rdr.nerf
        r0, first = 0, True
        for g in self.ctxs:
            R, S, M = g.R, g.S, g.M
            a = self.a_rows[:R]
            leases = []
            try:
                rgb, cctx = color_net.fwd_stash(g.pts_in, R * S, prec, g.grad, a, g.feat_ptr, train=backward)
                leases.append(cctx["lease"])
                bg_rgb = nctx = None
                if g.use_bg:
                    _, bg_rgb, nctx = nerf.fwd_stash(g.pts_bg, R * M, prec, a, select=g.select, train=backward, refine=g.refine)
                    leases.append(nctx["lease"])
                d_bg = self.d_bg_rgb[:R * M] if g.use_bg else None
                L.check(lib.ncw_appfit_loss(L.ptr(g.weights), L.ptr(g.inside), L.ptr(g.weights_sum), L.ptr(rgb), L.ptr(bg_rgb),
                                            L.ptr(g.background_rgb), L.ptr(self.targets[r0:r0 + R]), R, S, g.O, self.inv_denom,
                                            L.ptr(self.scale), L.ptr(self.color[r0:r0 + R]), L.ptr(self.ray_loss[r0:r0 + R]),
                                            L.ptr(self.d_rgb[:R * S]), L.ptr(d_bg), L.stream_ptr(dev)), "ncw_appfit_loss")
                if backward:
                    rows = self.rows[:R * S]
                    color_net.bwd_stash(cctx, self.d_rgb[:R * S], self.d_grad[:R * S], None, self.dfeat.ptr(0), d_a_rows=rows)
                    self._step_call(rows, R * S, not first, False)
                    first = False
                    if g.use_bg:
                        rows_bg = self.rows_bg[:R * M]
                        if nctx.get("sel_count") is not None:  # only the selected samples store their row: the others are exact zeros
                            rows_bg.zero_()
                        nerf.bwd_stash(nctx, self.d_density[:R * M], d_bg, None, d_a_rows=rows_bg)
                        self._step_call(rows_bg, R * M, True, False)
            finally:
                for l in leases:
                    StashCache.release(l)
            r0 += R
        return self.ray_loss.sum() * self.inv_denom  # torch's sum: one fixed reduction tree per shape

    def loss_and_grad(self):
        """The loss at the current code (device scalar) and, in `grad`, its [n_a] gradient."""
        with torch.no_grad():
            return self._pass(True)

    def loss(self):
        """The loss alone (forward-only launches); `colors()` then holds the composed colours of the current code."""
        with torch.no_grad():
            return self._pass(False)

    def step(self):
        """Ends an iteration: non-finite guard, one Adam step on the code, broadcast to the rays."""
        self._step_call(None, 0, True, True)

    @property
    def grad(self):
        """[n_a] gradient of the last loss_and_grad(), loss scale divided out."""
        return self.grad_acc * self.scale[1] if self.scale is not None else self.grad_acc.clone()

    def colors(self):
        """[R, 3] colours composed by the last pass."""
        return self.color

    @property
    def skipped_steps(self):
        return int(self.state[2])

    @property
    def applied_steps(self):
        return int(self.state[0])


# -----------------------------------------------------------------------------------------------------------------------
# one view, all test views
# -----------------------------------------------------------------------------------------------------------------------
def _planar(gt, H, W, dev):
    g = gt.to(dev).float()
    if g.dim() == 2:  # [H * W, 3], the dataset's layout
        g = g.reshape(H, W, 3).permute(2, 0, 1)
    return g.reshape(3, H, W).contiguous()


def initial_code(rdr, init="mean", train_ids=None):
    """"mean": the mean of the embedding rows of the split's train images (`train_ids`; None = every row); "zeros"; or a tensor."""
    w = rdr.embeddings["a"].weight.detach()
    if torch.is_tensor(init):
        return init.detach().to(w.device).float().reshape(-1)
    if init == "zeros":
        return torch.zeros(w.shape[1], device=w.device)
    if init != "mean":
        raise ValueError("init must be 'mean', 'zeros' or a tensor, got %r" % (init,))
    if train_ids is not None and len(train_ids) > 0:
        ids = torch.as_tensor([int(i) for i in train_ids if 0 <= int(i) < w.shape[0]], device=w.device, dtype=torch.int64)
        if ids.numel() > 0:
            w = w.index_select(0, ids)
    return w.float().mean(0)


def fit_view(rdr, camera, gt, n_rays=DEFAULT_N_RAYS, steps=DEFAULT_STEPS, lr=DEFAULT_LR, seed=0, init="mean", train_ids=None,
             chunk=1024, background_rgb=None, nerf_far_override=None):
    """Fits the appearance code of one held-out view on its LEFT half (columns [0, W // 2), datasets/phototourism.py:730-733):
    a seeded subset of `n_rays` left-half pixels (all if fewer), rays from `views.view_rays` gathered by index, geometry frozen
    once, `steps` full-batch Adam iterations at `lr` (DEFAULT_STEPS / DEFAULT_LR are this project's choice: the reference never
    runs this fit).  gt: [3, H, W] or [H * W, 3].  Returns dict(code [n_a], loss_start, loss_end (device scalars),
    skipped_steps, n_rays, init [n_a])."""
    from . import views

    H, W = camera.height, camera.width
    dev = next(rdr.neuconw.parameters()).device
    if dev.type != "cuda":
        raise L.NeuconwHipError("appfit.fit_view: the renderer is not on a GPU; the hot path has no CPU fallback")
    pix = torch.from_numpy(ray_subset(W, H, n_rays, seed)).to(dev)
    rays = views.view_rays(camera, device=dev).index_select(0, pix)
    targets = _planar(gt, H, W, dev).reshape(3, H * W).t().index_select(0, pix).contiguous()
    code0 = initial_code(rdr, init, train_ids)
    ctxs = freeze_rays(rdr, rays, background_rgb=background_rgb, chunk=chunk, far_override=nerf_far_override)
    try:
        fit = AppearanceFit(rdr, ctxs, targets, code0, lr=lr)
        loss_start = fit.loss().clone()
        for _ in range(int(steps)):
            fit.loss_and_grad()
            fit.step()
        loss_end = fit.loss().clone()
        res = dict(code=fit.code.clone(), loss_start=loss_start, loss_end=loss_end, skipped_steps=fit.skipped_steps,
                   n_rays=int(pix.numel()), init=code0.clone())
    finally:
        release_contexts(ctxs)
    return res


def score_halves(color, gt, ssim_window=3):
    """psnr / ssim / mse of a rendered [3, H, W] image on its right half (columns [W // 2, W): `views.psnr(valid_mask=...)`,
    `views.ssim` on the cropped planes) and on the whole image, as device scalars."""
    from . import views

    _, H, W = color.shape
    _, right = half_pixel_indices(W, H)
    mask = torch.zeros(H * W, dtype=torch.uint8, device=color.device)
    mask[torch.from_numpy(right).to(color.device)] = 1
    out = {"psnr_right": views.psnr(color, gt, valid_mask=mask), "mse_right": views.mse(color, gt, valid_mask=mask),
           "psnr_full": views.psnr(color, gt), "mse_full": views.mse(color, gt)}
    nan = torch.full((), float("nan"), device=color.device)
    pad = (ssim_window - 1) // 2
    cr, gr = color[:, :, W // 2:].contiguous(), gt[:, :, W // 2:].contiguous()
    out["ssim_right"] = views.ssim(cr, gr, ssim_window) if min(H, W - W // 2) > pad else nan
    out["ssim_full"] = views.ssim(color, gt, ssim_window) if min(H, W) > pad else nan
    return out


def eval_view(rdr, camera, gt, n_rays=DEFAULT_N_RAYS, steps=DEFAULT_STEPS, lr=DEFAULT_LR, seed=0, init="mean", train_ids=None,
              chunk=1024, render_chunk=None, background_rgb=None, nerf_far_override=None, ssim_window=3):
    """The NeRF-W evaluation of one held-out view: `fit_view` on the left half, then the whole view rendered with the fitted
    code (`views.render_view(a_code=...)`) and scored on the right half and on the whole image.  Returns fit_view's entries,
    `score_halves`' (psnr_right, ssim_right, mse_right, psnr_full, ssim_full, mse_full) and the rendered planes."""
    from . import views

    fit = fit_view(rdr, camera, gt, n_rays=n_rays, steps=steps, lr=lr, seed=seed, init=init, train_ids=train_ids, chunk=chunk,
                   background_rgb=background_rgb, nerf_far_override=nerf_far_override)
    dev = fit["code"].device
    g = _planar(gt, camera.height, camera.width, dev)
    planes = views.render_view(rdr, camera, ts=0, chunk=render_chunk or views.DEFAULT_CHUNK, background_rgb=background_rgb,
                               nerf_far_override=nerf_far_override, a_code=fit["code"])
    res = dict(fit)
    res.update(score_halves(planes["color"], g, ssim_window))
    res.update({k: planes[k] for k in ("color", "depth", "normal", "depth_vis")})
    return res


METRIC_KEYS = ("psnr_right", "ssim_right", "psnr_full", "loss_start", "loss_end", "skipped_steps")


def eval_views(root_dir, cfg, ckpt, img_downscale=None, n_rays=DEFAULT_N_RAYS, steps=DEFAULT_STEPS, lr=DEFAULT_LR, seed=0,
               init="mean", chunk=1024, out_dir=None, sfm_path=None, prec=None, device=None, image_names=None):
    """Runs `eval_view` over the `test` rows of the scene's split file.  cfg: a loaded experiment config (config.load_config) or
    its yaml path; ckpt: a checkpoint path.  Returns {"images": {file name: {psnr_right, ssim_right, psnr_full, loss_start,
    loss_end, skipped_steps}}, "mean": {...}}; with out_dir also writes <out_dir>/metrics.json and one GT | prediction | depth |
    normal panel per image.  init = "mean" starts from the mean embedding row of the split's train images."""
    from . import config as Cfg
    from . import trainer, views

    if isinstance(cfg, str):
        cfg = Cfg.load_config(cfg, {"DATASET": {"ROOT_DIR": root_dir}} if root_dir else None)
    root_dir = root_dir or cfg["DATASET"]["ROOT_DIR"]
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    emb, neuconw, nerf, rdr, _ = Cfg.build_system(cfg, dev, prec)
    trainer.load_checkpoint(ckpt, emb, neuconw, nerf)
    for m in (emb, neuconw, nerf):
        m.eval()
        for p in m.parameters():
            p.requires_grad_(False)
    downscale = int(img_downscale) if img_downscale is not None else int(cfg["DATASET"]["PHOTOTOURISM"]["IMG_DOWNSCALE"])
    names = list(image_names) if image_names is not None else held_out_rows(root_dir)
    scene = views.read_scene(root_dir, sfm_path)
    far = bool(cfg["NEUCONW"]["NEAR_FAR_OVERRIDE"])
    images = {}
    for name in names:
        cam, gt, image_id = views.scene_view(root_dir, image_name=name, img_downscale=downscale, sfm_path=sfm_path,
                                             split="test_train")
        r = eval_view(rdr, cam, gt.to(dev), n_rays=n_rays, steps=steps, lr=lr, seed=seed, init=init,
                      train_ids=scene["ids_train"], chunk=chunk, nerf_far_override=far)
        images[name] = {k: (int(r[k]) if k == "skipped_steps" else float(r[k])) for k in METRIC_KEYS}
        if out_dir:
            views.write_panel(os.path.join(out_dir, os.path.splitext(name)[0] + ".png"), gt, r["color"], r["depth_vis"],
                              r["normal"])
    mean = {k: (float(np.mean([v[k] for v in images.values()])) if images else float("nan")) for k in METRIC_KEYS}
    res = {"images": images, "mean": mean, "steps": int(steps), "lr": float(lr), "n_rays": int(n_rays), "seed": int(seed)}
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "metrics.json"), "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
    return res
