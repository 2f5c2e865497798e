"""GPU: `views.render_view` -- a whole camera view rendered chunk by chunk on the device (ncw_view_rays -> the forward-only
render -> ncw_view_store, then the depth colour map and the metrics) -- against the same chunks rendered by `rdr.render` under
no_grad and assembled by torch in the test (lightning_modules/neuconw_system.py:404-464, 533-546)."""
import numpy as np
import pytest
import torch

from tests import _view_ref as VR
from tests._build import build_system

pytestmark = pytest.mark.gpu

BIG = dict(n_a=48, n_vocab=100, nerf_w=256, color_hidden=256, head=128)
W_, H_ = 37, 23


def _camera():
    """At (0, 0, -2) looking along +z at the unit sphere ("right up back" axes), 30 degrees across, off-centre principal point."""
    from neuralrecon_w_amd.views import Camera

    fx = 0.5 * W_ / np.tan(np.deg2rad(15.0))
    return Camera([[fx, 0, 0.5 * W_ - 0.3], [0, 1.05 * fx, 0.5 * H_ + 0.4], [0, 0, 1]],
                  [[-1, 0, 0, 0.05], [0, 1, 0, -0.02], [0, 0, -1, -2.0]], W_, H_, 1.0, 3.0)


def _system(W, prec_name, ns, ni):
    import neuralrecon_w_amd as nw

    prec = {"f32": nw.PREC_F32, "f16": nw.PREC_F16}[prec_name]
    emb, neuconw, nerf, rdr = build_system(W=W, prec=prec, n_samples=ns, n_importance=ni, seed=5, **(BIG if W >= 256 else {}))
    with torch.no_grad():
        for n, p in neuconw.named_parameters():
            if n.endswith("weight_g"):
                p.mul_(1.0 + 0.1 * torch.randn_like(p))
    return emb, neuconw, nerf, rdr


def test_planes_equal_the_chunks_rendered_by_render_and_assembled_by_torch():
    """37 x 23 view, chunk 256: three full chunks and one of 83 rays.  Colour and depth planes are BITWISE what `rdr.render`
    under no_grad returns for the same chunks' rays; the normal plane is sum_s gradients weights[:, :S] of render()'s own
    dictionary, normalised and mapped to [0, 1], within 1e-6 (measured 7.6e-8); PSNR / MSE are the test's own formula on the assembled colour;
    the depth panel is the reference's colour map of the depth plane."""
    from neuralrecon_w_amd import views

    emb, neuconw, nerf, rdr = _system(64, "f32", 8, 8)
    cam = _camera()
    hw = W_ * H_
    assert hw == 3 * 256 + 83
    gt = torch.rand(3, H_, W_, generator=torch.Generator().manual_seed(3)).cuda()
    bg = torch.full((1, 3), 0.25).cuda()
    out = views.render_view(rdr, cam, ts=21, chunk=256, gt=gt, background_rgb=bg)
    assert out["color"].shape == (3, H_, W_) and out["depth"].shape == (H_, W_) and out["normal"].shape == (3, H_, W_)
    assert out["depth_vis"].shape == (3, H_, W_) and all(out[k].is_cuda for k in out)
    assert rdr.sync_free is False and rdr.nerf_far_override is False  # the renderer's attributes are not touched
    color, depth, normal = torch.empty(hw, 3).cuda(), torch.empty(hw).cuda(), torch.empty(hw, 3).cuda()
    S = rdr.n_samples + rdr.n_importance
    with torch.no_grad():
        for p0 in range(0, hw, 256):
            n = min(256, hw - p0)
            rays = views.view_rays(cam, p0, n)
            o = rdr.render(rays, torch.full((n,), 21).cuda(), torch.zeros(n, dtype=torch.long).cuda(), perturb_overwrite=0,
                           background_rgb=bg)
            color[p0:p0 + n], depth[p0:p0 + n] = o["color"], o["depth"]
            assert o["gradients"].shape == (n, S, 3)
            normal[p0:p0 + n] = (o["gradients"] * o["weights"][:, :S, None]).sum(1)
    assert torch.equal(out["color"], color.reshape(H_, W_, 3).permute(2, 0, 1))
    assert torch.equal(out["depth"], depth.reshape(H_, W_))
    want_n = VR.normal_plane(normal.cpu(), H_, W_)
    got_n = out["normal"].cpu().double()
    assert torch.equal(torch.isnan(got_n), torch.isnan(want_n))
    ok = ~torch.isnan(want_n)
    err_n = float((got_n[ok] - want_n[ok]).abs().max())
    print("normal plane: max |diff| %.3g" % err_n)
    assert err_n <= 1e-6
    assert float(got_n[ok].min()) >= 0 and float(got_n[ok].max()) <= 1
    # metrics: the test's own formula on the assembled colour
    g = gt.permute(1, 2, 0).reshape(hw, 3)
    mse = float(((color.double() - g.double()) ** 2).mean())
    assert abs(float(out["mse"]) - mse) <= 2e-6 * mse
    assert abs(float(out["psnr"]) + 10 * np.log10(mse)) <= 1e-4
    assert abs(float(out["ssim"]) - float(VR.ssim(out["color"].cpu(), gt.cpu(), 3))) <= 1e-5
    # the [H * W, 3] layout of the dataset's rgbs gives the same metrics
    out2 = views.render_view(rdr, cam, ts=21, chunk=256, gt=g, background_rgb=bg)
    assert torch.equal(out2["psnr"], out["psnr"]) and torch.equal(out2["ssim"], out["ssim"]) and torch.equal(out2["color"], out["color"])
    idx = VR.depth_index(depth.reshape(H_, W_).cpu().numpy())
    assert np.array_equal(out["depth_vis"].cpu().numpy(), (views.JET[idx].astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
    assert len(np.unique(idx)) > 20  # a real depth range


@pytest.mark.parametrize("W,prec_name,ns,ni", [(64, "f32", 8, 8), (64, "f16", 8, 8), (256, "f16", 16, 16)])
def test_chunk_invariance(W, prec_name, ns, ni):
    """chunk = 256 (four launches, the last of 83 rays) against one chunk of all 851 rays.  A ray's arithmetic does not depend
    on its neighbours in the launch, so the planes are expected to be bitwise equal; asserted is the project's per-ray bound
    of 1e-4, and the measured maximum is printed.  Measured on an MI355X: 0 (bitwise) for colour, depth and normal in all
    three configurations."""
    from neuralrecon_w_amd import views

    emb, neuconw, nerf, rdr = _system(W, prec_name, ns, ni)
    cam = _camera()
    a = views.render_view(rdr, cam, ts=3, chunk=256)
    b = views.render_view(rdr, cam, ts=3, chunk=W_ * H_)
    assert set(a) == {"color", "depth", "normal", "depth_vis"}  # no gt: no metrics
    worst = 0.0
    for k in ("color", "depth", "normal"):
        x, y = a[k], b[k]
        assert torch.equal(torch.isnan(x), torch.isnan(y)), k
        d = float(torch.nan_to_num(x - y, nan=0.0).abs().max())
        print("chunk invariance W=%d %s %d+%d %s: max |diff| %.3g%s" % (W, prec_name, ns, ni, k, d, " (bitwise)" if torch.equal(
            torch.nan_to_num(x), torch.nan_to_num(y)) else ""))
        worst = max(worst, d)
    assert worst <= 1e-4
    assert torch.isfinite(a["color"]).all() and torch.isfinite(a["depth"]).all()


def test_training_render_still_runs_after_render_view():
    """The forward-only view render leaves the training path intact: a training render() + backward() issued BEFORE the view
    still back-propagates after it, and matches a fresh one (the arena-reuse check of tests/test_gpu_render_only.py)."""
    from neuralrecon_w_amd import views
    from tests._util import synth_rays

    emb, neuconw, nerf, rdr = _system(64, "f32", 8, 8)
    rays, ts, label, rgbs = [t.cuda() for t in synth_rays(77, 21, 64)]
    bg = torch.full((1, 3), 0.25).cuda()
    train = rdr.render(rays, ts, label, perturb_overwrite=0, background_rgb=bg, cos_anneal_ratio=0.4)
    assert train["color"].requires_grad
    keys_before = set(train)
    views.render_view(rdr, _camera(), ts=21, chunk=256, gt=torch.rand(3, H_, W_).cuda())
    loss = (train["color"] - rgbs).abs().mean() + 0.1 * train["gradient_error"].mean()
    loss.backward()
    g1 = neuconw.sdf_net.lin3.weight_v.grad.clone()
    for p_ in list(emb.parameters()) + list(neuconw.parameters()) + list(nerf.parameters()):
        p_.grad = None
    again = rdr.render(rays, ts, label, perturb_overwrite=0, background_rgb=bg, cos_anneal_ratio=0.4)
    assert set(again) == keys_before and "normals" not in again  # render()'s dictionary is unchanged
    assert torch.equal(again["color"].detach(), train["color"].detach())
    ((again["color"] - rgbs).abs().mean() + 0.1 * again["gradient_error"].mean()).backward()
    g2 = neuconw.sdf_net.lin3.weight_v.grad
    assert torch.isfinite(g1).all() and float((g1 - g2).abs().max()) <= 2e-3 * float(g2.abs().max()) + 1e-12
