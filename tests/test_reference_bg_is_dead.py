"""CPU, against the REAL reference: the premise of the product's dead-background elimination.  With
trim_sphere, NeuconWRenderer.render_core (rendering/renderer.py:570-783 of the reference) multiplies the background NeRF's
alpha and colour at every primary sample inside the unit sphere by 1 - inside_sphere = 0 (:637, :693-708): whatever
render_core_outside returned there never reaches an output, and no gradient flows back into it.  Also pins oracle.bg_needed,
the CPU statement of the selection ncw_bg_select makes on the device.  Where the reference tree is present the reference runs
live; elsewhere the same assertions hold on what it returned for this case (tests/golden/ref_checks.npz, written by
tests/golden/make_golden_refchecks.py)."""
import os

import numpy as np
import torch

from oracle import ref_import
from tests._util import GOLDEN, synth_rays

OUT_KEYS = ("color", "depth", "weights", "weights_sum", "color_bg", "gradient_error")


def _geometry():
    R, S, O = 48, 32, 4
    rays, ts, label, rgbs = synth_rays(R, 21, 64)
    o, d = rays[:, 0:3], rays[:, 3:6]
    near, far = torch.full((R, 1), 0.6), torch.full((R, 1), 3.6)  # the interval leaves the unit sphere on both ends
    z = near + (far - near) * torch.linspace(0, 1, S)[None]
    sample_dist = (far - near) / S
    z_out = far / torch.flip(torch.linspace(1e-3, 1 - 1 / (O + 1.0), O), dims=[-1]) + 1.0 / S
    zf, _ = torch.sort(torch.cat([z, z_out], -1), -1)
    return ts, rgbs, o, d, z, zf, sample_dist, R, S, O


def bg_case(ns):
    from tests.golden.make_golden import build_reference

    emb, neuconw, nerf, renderer = build_reference(ns, 64, 2, (), seed=2, n_samples=32, n_importance=0)
    ts, rgbs, o, d, z, zf, sample_dist, R, S, O = _geometry()
    a = emb(ts)
    return renderer, nerf, o, d, z, zf, sample_dist, a, rgbs, R, S, O


def render_core_loss(renderer, o, d, z, sample_dist, a, rgbs, R, bg_alpha, bg_col):
    rc = renderer.render_core(o, d, z, sample_dist, a, cos_anneal_ratio=0.3, background_alpha=bg_alpha,
                              background_sampled_color=bg_col, background_rgb=torch.zeros(1, 3))
    loss = (rc["color"] - rgbs).abs().sum() / R + 0.1 * rc["gradient_error"] + 0.05 * rc["weights_sum"].mean() \
        + 0.05 * rc["depth"].mean() + 0.01 * rc["color_bg"].sum()
    return rc, loss


def perturb_inside(alpha, color, ins, S):
    """Arbitrary background values at the inside samples (seed 0)."""
    torch.manual_seed(0)
    al2, col2 = alpha.clone(), color.clone()
    al2[:, :S][ins] = torch.rand(int(ins.sum()))
    col2[:, :S][ins] = torch.randn(int(ins.sum()), 3) * 5.0
    return al2, col2


def _golden():
    return np.load(os.path.join(GOLDEN, "ref_checks.npz"))


def test_reference_ignores_background_at_inside_samples():
    S = _geometry()[8]
    if ref_import.available():
        renderer, nerf, o, d, z, zf, sample_dist, a, rgbs, R, S, O = bg_case(ref_import.load())
        with torch.no_grad():
            ro = renderer.render_core_outside(o, d, zf, sample_dist, nerf, a_embedded=a)
        al = ro["alpha"].clone().requires_grad_(True)
        col = ro["sampled_color"].clone().requires_grad_(True)
        # (render_core writes into background_alpha in place, :706: no leaves)
        rc0, loss0 = render_core_loss(renderer, o, d, z, sample_dist, a, rgbs, R, al * 1.0, col * 1.0)
        g_al, g_col = torch.autograd.grad(loss0, [al, col])
        ins = rc0["inside_sphere"] > 0  # [R, S]
        al2, col2 = perturb_inside(ro["alpha"], ro["sampled_color"], ins, S)
        rc1, loss1 = render_core_loss(renderer, o, d, z, sample_dist, a, rgbs, R, al2, col2)
        out0, out1 = {k: rc0[k] for k in OUT_KEYS}, {k: rc1[k] for k in OUT_KEYS}
        loss0, loss1 = float(loss0), float(loss1)
    else:
        g = _golden()
        ins, g_al, g_col = (torch.from_numpy(g[k]) for k in ("bg_inside", "bg_grad_alpha", "bg_grad_color"))
        out0 = {k: torch.from_numpy(g["bg_out0/" + k]) for k in OUT_KEYS}
        out1 = {k: torch.from_numpy(g["bg_out1/" + k]) for k in OUT_KEYS}
        loss0, loss1 = (float(x) for x in g["bg_loss"])
    assert 0.1 < float(ins.float().mean()) < 0.9
    # no gradient reaches the background values of an inside sample
    assert float(g_al[:, :S][ins].abs().max()) == 0.0 and float(g_col[:, :S][ins].abs().max()) == 0.0
    assert float(g_al[:, :S][~ins].abs().max()) > 0.0 and float(g_al[:, S:].abs().max()) > 0.0
    # and arbitrary values there change nothing the reference returns
    for k in OUT_KEYS:
        assert torch.equal(out0[k], out1[k]), k
    assert loss0 == loss1


def test_oracle_selection_is_the_reference_mask():
    from oracle import neuconw_oracle as O

    ts, rgbs, o, d, z, zf, sample_dist, R, S, O_ = _geometry()
    if ref_import.available():
        renderer, nerf, o, d, z, zf, sample_dist, a, rgbs, R, S, O_ = bg_case(ref_import.load())
        with torch.no_grad():
            ro = renderer.render_core_outside(o, d, zf, sample_dist, nerf, a_embedded=a)
        rc = renderer.render_core(o, d, z, sample_dist, a, cos_anneal_ratio=0.3, background_alpha=ro["alpha"],
                                  background_sampled_color=ro["sampled_color"], background_rgb=torch.zeros(1, 3))
        inside = rc["inside_sphere"] > 0
    else:
        inside = torch.from_numpy(_golden()["bg_inside"])
    need = O.bg_needed(o, d, z, sample_dist, O_)
    assert need.shape == (R, S + O_) and bool(need[:, S:].all())
    assert torch.equal(need[:, :S], ~inside)
