"""GPU: the appearance-code fit on frozen geometry (neuralrecon_w_amd/appfit.py) against the path the project already trusts --
render() + L1 + backward() with a one-row embedding -- and both against float64 autograd of the oracle through the same loss.

Every test prints its measured figures; those of an MI355X run are kept in profiles/appfit/README.md."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._build import build_system, state_dict_cpu
from tests._util import ROOT, rel_err, synth_rays

pytestmark = pytest.mark.gpu

R_, N_A = 12, 16
LR, B1, B2, EPS = 0.05, 0.9, 0.999, 1e-7


def _cfg(trim):
    return dict(n_samples=8, n_importance=8, n_outside=4, up_sample_steps=2, s_val_base=3, render_bg=True, trim_sphere=trim,
                mesh_mask_list=None, depth_loss=False, skip_in=(4,), multires=6, multires_view=4)


def _system(prec, trim=True, seed=0):
    emb, neuconw, nerf, rdr = build_system(seed=seed, prec=prec, n_samples=8, n_importance=8, trim_sphere=trim, mesh_mask_list=None,
                                           depth_loss=False, n_a=N_A)
    return emb, neuconw, nerf, rdr


def _inputs(seed=1):
    rays, _, _, rgbs = synth_rays(R_, seed, 64)
    code = 0.5 * torch.randn(N_A, generator=torch.Generator().manual_seed(seed + 100))
    return rays[:, :8].contiguous(), rgbs, code, torch.tensor([[0.25, 0.5, 0.125]])


def _oracle(emb, neuconw, nerf, trim, rays, rgbs, code, bg):
    """(colour, loss, d loss / d code) in float64: the oracle's render() with a one-row embedding and the L1 colour loss."""
    from oracle import neuconw_oracle as O

    sd = state_dict_cpu(emb, neuconw, nerf, torch.float64)
    a = code.double().reshape(1, -1).clone().requires_grad_(True)
    sd["embedding_a.weight"] = a
    ref = O.render(sd, _cfg(trim), rays.double(), torch.zeros(R_, dtype=torch.long), torch.zeros(R_, dtype=torch.long), 0.0,
                   bg.double())
    loss = (ref["color"] - rgbs.double()).abs().sum() / (R_ + 1e-5)
    (g,) = torch.autograd.grad(loss, a)
    return ref["color"].detach(), float(loss.detach()), g.reshape(-1)


def _composed(rdr, rays, rgbs, code, bg):
    """What the parent offers: render() + L1 + backward() with a one-row embedding requiring a gradient."""
    emb1 = torch.nn.Embedding(1, N_A).cuda()
    with torch.no_grad():
        emb1.weight.copy_(code.reshape(1, -1))
    saved = rdr.embeddings
    rdr.embeddings = {"a": emb1}
    try:
        out = rdr.render(rays.cuda(), torch.zeros(R_, dtype=torch.long).cuda(), torch.zeros(R_, dtype=torch.long).cuda(),
                         perturb_overwrite=0, background_rgb=bg.cuda(), cos_anneal_ratio=0.0)
        loss = (out["color"] - rgbs.cuda()).abs().sum() / (R_ + 1e-5)
        loss.backward()
    finally:
        rdr.embeddings = saved
    return out["color"].detach().cpu(), float(loss.detach()), emb1.weight.grad[0].detach().cpu()


@pytest.mark.parametrize("trim", [True, False])
def test_frozen_path_matches_render_and_is_as_close_to_the_oracle(trim):
    """Acceptance: the frozen path's error against the float64 oracle is at most twice the composed path's (the same MLP launches,
    another reduction order).  Measured on an MI355X, both settings: colour 1.9e-07 / 1.9e-07 (frozen bitwise equal to render()'s),
    d loss / d code 1.15e-07 frozen against 1.5e-07 composed."""
    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import appfit

    emb, neuconw, nerf, rdr = _system(nw.PREC_F32, trim)
    rays, rgbs, code, bg = _inputs()
    grads_before = [p.grad for p in list(neuconw.parameters()) + list(nerf.parameters())]
    ctxs = appfit.freeze_rays(rdr, rays.cuda(), background_rgb=bg.cuda(), chunk=5)  # 5 + 5 + 2 rays: three chunks
    assert [g.R for g in ctxs] == [5, 5, 2]
    fit = appfit.AppearanceFit(rdr, ctxs, rgbs.cuda(), code.cuda(), lr=LR, betas=(B1, B2), eps=EPS)
    loss_f = float(fit.loss_and_grad())
    col_f, g_f = fit.colors().cpu().clone(), fit.grad.cpu().clone()
    assert all(p.grad is g0 for p, g0 in zip(list(neuconw.parameters()) + list(nerf.parameters()), grads_before))  # no .grad touched
    col_c, loss_c, g_c = _composed(rdr, rays, rgbs, code, bg)
    col_o, loss_o, g_o = _oracle(emb, neuconw, nerf, trim, rays, rgbs, code, bg)
    e = dict(color_frozen=rel_err(col_f, col_o), color_composed=rel_err(col_c, col_o), grad_frozen=rel_err(g_f, g_o),
             grad_composed=rel_err(g_c, g_o), color_frozen_vs_composed=rel_err(col_f, col_c), grad_frozen_vs_composed=rel_err(g_f, g_c))
    lines = ["trim_sphere=%s: colour vs oracle frozen %.3g composed %.3g (frozen vs composed %.3g%s); d loss / d code vs oracle "
             "frozen %.3g composed %.3g (frozen vs composed %.3g); loss frozen %.8f composed %.8f oracle %.8f"
             % (trim, e["color_frozen"], e["color_composed"], e["color_frozen_vs_composed"],
                ", bitwise" if torch.equal(col_f, col_c) else "", e["grad_frozen"], e["grad_composed"], e["grad_frozen_vs_composed"],
                loss_f, loss_c, loss_o)]
    print(lines[0])
    assert e["color_composed"] < 1e-4 and e["grad_composed"] < 2e-3  # the trusted path is where smoke() holds it
    # the acceptance: the same MLP launches, another reduction order -- at most twice the composed path's error
    assert e["color_frozen"] <= 2 * e["color_composed"], e
    assert e["grad_frozen"] <= 2 * e["grad_composed"], e
    assert abs(loss_f - loss_c) <= 1e-6 * abs(loss_c)
    appfit.release_contexts(ctxs)


def _adam64(code, grads, steps):
    """`steps` Adam steps in float64 on the kernel's float32 arguments.  grads: a function code -> float64 gradient, or a list of
    gradients (one per step).  Returns (code, the gradients used)."""
    lr, b1, b2, eps = (float(np.float32(x)) for x in (LR, B1, B2, EPS))
    p, m, v = code.copy(), 0.0, 0.0
    used = []
    for t in range(1, steps + 1):
        g = grads(p) if callable(grads) else grads[t - 1]
        used.append(g)
        m = m + (1 - b1) * (g - m)
        v = v * b2 + (1 - b2) * g * g
        p = p - (lr / (1 - b1 ** t)) * (m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps))
    return p, used


def test_three_adam_steps_against_float64_steps_on_the_oracles_gradients():
    """Bound: the gradient bound of the test above (2 x the composed path's relative error against the oracle, as a share of
    max |g| of each step) pushed through the float64 Adam restatement: the oracle's three gradients moved by +bound and by
    -bound, the larger displacement per component; plus the fp32 arithmetic of the update itself, 3 steps x 10 roundings x 2^-24 of
    max(1, |code|).  Measured on an MI355X: max |code - float64| 3.75e-08 under a bound of 1.95e-06."""
    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import appfit

    emb, neuconw, nerf, rdr = _system(nw.PREC_F32, True)
    rays, rgbs, code, bg = _inputs()
    _, _, g_c = _composed(rdr, rays, rgbs, code, bg)
    _, _, g_o = _oracle(emb, neuconw, nerf, True, rays, rgbs, code, bg)
    e_g = 2 * rel_err(g_c, g_o)
    grad_fn = lambda p: _oracle(emb, neuconw, nerf, True, rays, rgbs, torch.from_numpy(p), bg)[2].numpy()  # noqa: E731
    want, gs = _adam64(code.double().numpy(), grad_fn, 3)
    hi, _ = _adam64(code.double().numpy(), [g + e_g * np.abs(g).max() for g in gs], 3)
    lo, _ = _adam64(code.double().numpy(), [g - e_g * np.abs(g).max() for g in gs], 3)
    tol = np.maximum(np.abs(hi - want), np.abs(lo - want)) + 3 * 10 * 2.0 ** -24 * max(1.0, float(np.abs(want).max()))
    ctxs = appfit.freeze_rays(rdr, rays.cuda(), background_rgb=bg.cuda(), chunk=5)
    fit = appfit.AppearanceFit(rdr, ctxs, rgbs.cuda(), code.cuda(), lr=LR, betas=(B1, B2), eps=EPS)
    for _ in range(3):
        fit.loss_and_grad()
        fit.step()
    diff = np.abs(fit.code.cpu().double().numpy() - want)
    line = "three Adam steps: max |code - float64| %.3g (bound %.3g .. %.3g per component, gradient bound %.3g of max |g|)" % (
        float(diff.max()), float(tol.min()), float(tol.max()), e_g)
    print(line)
    assert fit.applied_steps == 3 and fit.skipped_steps == 0
    assert np.all(diff <= tol), (diff, tol)
    assert float(np.abs(want - code.double().numpy()).max()) > 0.05
    appfit.release_contexts(ctxs)


# ------------------------------------------------------------------------------------------------------------------------
# whole views
# ------------------------------------------------------------------------------------------------------------------------
W_, H_ = 21, 12


def _camera():
    from neuralrecon_w_amd.views import Camera

    fx = 0.5 * W_ / np.tan(np.deg2rad(15.0))
    return Camera([[fx, 0, 0.5 * W_ - 0.3], [0, 1.05 * fx, 0.5 * H_ + 0.4], [0, 0, 1]],
                  [[-1, 0, 0, 0.05], [0, 1, 0, -0.02], [0, 0, -1, -2.0]], W_, H_, 1.0, 3.0)


def _vivid(neuconw, nerf):
    """Make the rendered colour depend visibly on the code: the appearance columns of both heads' first layers scaled up."""
    with torch.no_grad():
        neuconw.color_net.static_encoding[0].weight[:, -N_A:].mul_(6.0)
        nerf.apperence_encoding[0].weight[:, -N_A:].mul_(6.0)


def _recovery(prec):
    from neuralrecon_w_amd import appfit, views

    emb, neuconw, nerf, rdr = _system(prec, True, seed=3)
    _vivid(neuconw, nerf)
    cam = _camera()
    known = 0.8 * torch.randn(N_A, generator=torch.Generator().manual_seed(11)).cuda()
    gt = views.render_view(rdr, cam, ts=0, chunk=256, a_code=known)["color"].clone()
    res = appfit.eval_view(rdr, cam, gt, n_rays=100, steps=25, lr=0.05, seed=4, init="zeros", chunk=64, render_chunk=256)
    start = views.render_view(rdr, cam, ts=0, chunk=256, a_code=torch.zeros(N_A).cuda())["color"]
    return res, appfit.score_halves(start, gt), gt


def test_fit_recovers_a_known_code_and_is_reproducible():
    import neuralrecon_w_amd as nw

    res, start, gt = _recovery(nw.PREC_F32)
    print("fit from zeros: loss %.6f -> %.6f, right-half PSNR %.3f -> %.3f dB, SSIM %.4f -> %.4f (%d rays, %d skipped)"
          % (float(res["loss_start"]), float(res["loss_end"]), float(start["psnr_right"]), float(res["psnr_right"]),
             float(start["ssim_right"]), float(res["ssim_right"]), res["n_rays"], res["skipped_steps"]))
    assert res["n_rays"] == 100 and res["skipped_steps"] == 0
    assert float(res["loss_end"]) < float(res["loss_start"])
    assert float(res["psnr_right"]) > float(start["psnr_right"])
    assert np.isfinite(float(res["ssim_right"])) and np.isfinite(float(res["psnr_full"]))
    again, _, _ = _recovery(nw.PREC_F32)
    assert torch.equal(again["code"], res["code"]) and torch.equal(again["loss_end"], res["loss_end"])
    assert torch.equal(again["color"], res["color"])


def test_fit_in_fp16_runs_skips_nothing_and_its_loss_falls():
    import neuralrecon_w_amd as nw

    res, _, _ = _recovery(nw.PREC_F16)
    print("fp16 fit: loss %.6f -> %.6f, %d skipped" % (float(res["loss_start"]), float(res["loss_end"]), res["skipped_steps"]))
    assert res["skipped_steps"] == 0 and torch.isfinite(res["code"]).all()
    assert float(res["loss_end"]) < float(res["loss_start"])


def test_render_view_without_a_code_is_the_parents_render_view():
    """a_code=None takes today's path: the planes are bit for bit those of the chunks rendered by render() with the embedding row
    (what the parent's render_view is pinned to, tests/test_gpu_render_view.py); a_code = that row gives the same bits."""
    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import views

    emb, neuconw, nerf, rdr = _system(nw.PREC_F32, True, seed=5)
    cam = _camera()
    hw = W_ * H_
    a = views.render_view(rdr, cam, ts=21, chunk=100)
    b = views.render_view(rdr, cam, ts=21, chunk=100, a_code=None)
    color, depth = torch.empty(hw, 3).cuda(), torch.empty(hw).cuda()
    with torch.no_grad():
        for p0 in range(0, hw, 100):
            n = min(100, hw - p0)
            o = rdr.render(views.view_rays(cam, p0, n), torch.full((n,), 21).cuda(), torch.zeros(n, dtype=torch.long).cuda(),
                           perturb_overwrite=0)
            color[p0:p0 + n], depth[p0:p0 + n] = o["color"], o["depth"]
    for k in ("color", "depth", "normal", "depth_vis"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["color"], color.reshape(H_, W_, 3).permute(2, 0, 1)) and torch.equal(a["depth"], depth.reshape(H_, W_))
    c = views.render_view(rdr, cam, ts=0, chunk=100, a_code=emb.weight[21].detach())
    assert torch.equal(c["color"], a["color"]) and torch.equal(c["depth"], a["depth"])


def test_cpu_tensors_are_refused_on_a_gpu_box():
    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import appfit

    emb, neuconw, nerf, rdr = _system(nw.PREC_F32)
    with pytest.raises(nw.NeuconwHipError, match="no CPU fallback"):
        appfit.freeze_rays(rdr, torch.zeros(4, 8))


# ------------------------------------------------------------------------------------------------------------------------
# scripts/eval_views.py end to end
# ------------------------------------------------------------------------------------------------------------------------
def test_eval_views_script_on_the_synthetic_scene(tmp_path):
    pytest.importorskip("PIL.Image")
    import struct

    from neuralrecon_w_amd import config as Cfg
    from neuralrecon_w_amd import trainer, views
    from tests.test_gpu_train_driver import _write_scene

    root = str(tmp_path / "scene")
    cfg_path = _write_scene(root, n_chunks=1)
    sp = os.path.join(root, "dense", "sparse")
    iw, ih = 40, 24
    with open(os.path.join(sp, "cameras.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", 1) + struct.pack("<iiQQ", 1, 1, iw, ih) + struct.pack("<4d", 52.0, 52.0, iw / 2, ih / 2))
    names = [(5, "a.png", "train"), (6, "t0.png", "test"), (7, "t1.png", "test")]
    with open(os.path.join(sp, "images.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(names)))
        for iid, name, _ in names:
            fh.write(struct.pack("<i7di", iid, 1.0, 0.0, 0.0, 0.0, 0.02 * iid, 0.0, 2.0, 1) + name.encode() + b"\x00" + struct.pack("<Q", 0))
    with open(os.path.join(root, "synth.tsv"), "w") as fh:
        fh.write("filename\tid\tsplit\tdataset\n" + "".join("%s\t%d\t%s\tsynthetic\n" % (n, i, s) for i, n, s in names))
    yy, xx = np.mgrid[0:ih, 0:iw]
    for iid, name, _ in names:
        img = np.stack([255 * xx / (iw - 1), 255 * yy / (ih - 1), 127 + 100 * np.sin(0.3 * xx + 0.2 * yy + iid)], -1)
        views.write_png(os.path.join(root, "dense", "images", name), np.clip(img, 0, 255).astype(np.uint8))
    cfg = Cfg.load_config(cfg_path)
    torch.manual_seed(0)
    emb, neuconw, nerf, rdr, _ = Cfg.build_system(cfg, torch.device("cuda"), None)
    ckpt = os.path.join(root, "w.ckpt")
    trainer.save_checkpoint(ckpt, emb, neuconw, nerf)
    out_dir = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_views.py"), "--cfg_path", cfg_path, "--ckpt_path", ckpt,
                        "--root_dir", root, "--n_rays", "150", "--steps", "4", "--chunk", "100", "--prec", "f32", "--out_dir", out_dir],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    m = json.load(open(os.path.join(out_dir, "metrics.json")))
    assert sorted(m["images"]) == ["t0.png", "t1.png"]
    keys = {"psnr_right", "ssim_right", "psnr_full", "loss_start", "loss_end", "skipped_steps"}
    for v in list(m["images"].values()) + [m["mean"]]:
        assert keys <= set(v) and all(np.isfinite(v[k]) for k in keys)
    for name in ("t0", "t1"):
        assert os.path.isfile(os.path.join(out_dir, name + ".png"))
    assert "mean over 2 image(s)" in r.stdout
