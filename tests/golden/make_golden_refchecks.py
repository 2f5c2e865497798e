"""Golden vectors for the CPU checks that otherwise need the reference tree itself (tests/golden/ref_checks.npz), produced
by RUNNING the reference (imported on CPU under the stub recipe of oracle/ref_import.py):

  * `init_*`: a fingerprint of the reference's freshly constructed NeuconW + NeRF at torch.manual_seed(7) (the configuration
    of tests/test_abi_and_host.py::test_same_seed_same_init_as_reference): per state_dict key the float64 sum, the float64
    sum of |x| and 16 values at fixed flat indices -- the whole state (2 M values) would not fit a fixture;
  * `bg_*`: the case of tests/test_reference_bg_is_dead.py (W = 64, 48 rays x 32 + 4 samples): the reference's
    inside_sphere mask, the gradients its loss sends into the background alpha / colour, and its outputs with the
    background values at inside samples replaced by arbitrary ones, beside the unmodified outputs.

Run where the reference tree is present:   python tests/golden/make_golden_refchecks.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402

N_PICK = 16


def init_fingerprint(sd):
    """-> keys, sums, abs sums, picked values [K, 16] (flat indices linspace(0, n - 1, 16), repeats for small tensors)."""
    keys, s, a, pick = [], [], [], []
    for k, v in sd.items():
        v = v.detach().double().reshape(-1)
        idx = torch.linspace(0, v.numel() - 1, N_PICK).round().long()
        keys.append(k)
        s.append(float(v.sum()))
        a.append(float(v.abs().sum()))
        pick.append(v[idx].numpy())
    return np.array(keys), np.array(s), np.array(a), np.stack(pick)


def same_seed_init(ns):
    sdf_cfg = dict(d_in=3, d_out=257, d_hidden=256, n_layers=8, skip_in=(4,), multires=6, bias=0.5, scale=1,
                   geometric_init=True, weight_norm=True, inside_outside=False)
    color_cfg = dict(d_in=9, d_feature=256, mode="idr", d_out=3, d_hidden=256, n_layers=4, head_channels=128,
                     static_head_layers=2, weight_norm=True, multires_view=4)
    torch.manual_seed(7)
    ref = ns.NeuconW(sdf_cfg, color_cfg, dict(init_val=0.3), 48, True)
    ref_bg = ns.NeRF(D=8, d_in=4, d_in_view=3, W=256, multires=10, multires_view=4, output_ch=4, skips=[4],
                     encode_appearance=True, in_channels_a=48, in_channels_dir=27, use_viewdirs=True)
    out = {}
    for tag, mod in (("nc", ref), ("bg", ref_bg)):
        keys, s, a, pick = init_fingerprint(mod.state_dict())
        out.update({"init_%s_keys" % tag: keys, "init_%s_sum" % tag: s, "init_%s_abs" % tag: a, "init_%s_pick" % tag: pick})
    return out


def bg_is_dead(ns):
    from tests.test_reference_bg_is_dead import OUT_KEYS, bg_case, perturb_inside, render_core_loss

    renderer, nerf, o, d, z, zf, sample_dist, a, rgbs, R, S, O = bg_case(ns)
    with torch.no_grad():
        ro = renderer.render_core_outside(o, d, zf, sample_dist, nerf, a_embedded=a)
    al = ro["alpha"].clone().requires_grad_(True)
    col = ro["sampled_color"].clone().requires_grad_(True)
    rc0, loss0 = render_core_loss(renderer, o, d, z, sample_dist, a, rgbs, R, al * 1.0, col * 1.0)
    g_al, g_col = torch.autograd.grad(loss0, [al, col])
    ins = rc0["inside_sphere"] > 0
    al2, col2 = perturb_inside(ro["alpha"], ro["sampled_color"], ins, S)
    rc1, loss1 = render_core_loss(renderer, o, d, z, sample_dist, a, rgbs, R, al2, col2)
    out = {"bg_inside": ins.numpy(), "bg_grad_alpha": g_al.numpy(), "bg_grad_color": g_col.numpy(),
           "bg_loss": np.array([float(loss0), float(loss1)])}
    for k in OUT_KEYS:
        out["bg_out0/" + k] = rc0[k].detach().numpy()
        out["bg_out1/" + k] = rc1[k].detach().numpy()
    return out


def main():
    ns = ref_import.load()
    out = same_seed_init(ns)
    out.update(bg_is_dead(ns))
    path = os.path.join(HERE, "ref_checks.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
