"""GPU: the weights-stationary background-NeRF kernels (csrc/ncw_sdf8.hip nerf_fwdB / nerf_bwdB, W = 256, 16-bit) at their shape
edges.  Every comparison here is EXACT: a column of an MFMA depends on nothing but its own point, so the same points evaluated
in another launch decomposition -- another workgroup, another tile of the workgroup, another lane group of the tile -- must give
the same bits; any difference is an LDS fragment read from the wrong tile, k-unit or buffer (the fragment ring of the MFMA loops,
the slice reloaded in place).  The accuracy of these kernels against the fp64 oracle is pinned by
tests/test_gpu_color_nerf.py::test_nerf_train_vs_oracle."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 419                     # 13 tiles + 3 points: 3 full workgroups + one workgroup holding one full tile and a 3-point tile
SLICES = (1, 33, 129, 256)  # consecutive slices of the same points (sum = N)
N_A = 48
TRUNKS = [(8, 4), (2, 0), (3, 1)]  # (D, skip): the headline;  the smallest trunk (the first hidden layer is the skip layer and the
#                                    "next slice" is already w_feat);  the skip on the last hidden layer


def _prec(name):
    import neuralrecon_w_amd as nw

    return {"bf16": nw.PREC_BF16, "f16": nw.PREC_F16}[name]


def _nerf(D, skip, seed=21):
    import neuralrecon_w_amd as nw

    torch.manual_seed(seed)
    nerf = nw.NeRF(D=D, d_in=4, d_in_view=3, W=256, multires=10, multires_view=4, output_ch=4, skips=[skip],
                   encode_appearance=True, in_channels_a=N_A, in_channels_dir=27, use_viewdirs=True).cuda()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():  # biases away from 0: both signs of every pre-activation occur
        for n, p in nerf.named_parameters():
            if n.endswith("bias"):
                p.add_(0.05 * torch.randn(p.shape, generator=g).to(p.device))
    return nerf


def _inputs(seed=22):
    g = torch.Generator().manual_seed(seed)

    def unit(n):
        d = torch.randn(n, 3, generator=g)
        return d / d.norm(dim=-1, keepdim=True)

    x4 = torch.cat([unit(N), torch.rand(N, 1, generator=g) * 0.9 + 0.05], -1)  # inverted-sphere points [x / r, 1 / r]
    return dict(x4=x4.cuda(), dirs=unit(N).cuda(), a=torch.randn(N, N_A, generator=g).cuda(),
                w_den=torch.randn(N, generator=g).cuda(), w_rgb=torch.randn(N, 3, generator=g).cuda())


def _run(nerf, prec, inp, lo, hi, train=True, backward=True):
    """points lo .. hi-1 as one launch: (density, rgb, d_a) -- with x4 every point is its own ray, so d_a gets exactly one atomic
    per element: no summation order"""
    from neuralrecon_w_amd.neuconw import points_struct
    from neuralrecon_w_amd.stash import StashCache

    n = hi - lo
    x4 = inp["x4"][lo:hi].contiguous()
    pts = points_struct(x=x4[:, :3].contiguous(), rays_d=inp["dirs"][lo:hi].contiguous())
    density, rgb, ctx = nerf.fwd_stash(pts, n, prec, inp["a"][lo:hi].contiguous(), x4=x4, train=train)
    d_a = None
    if train and backward:
        d_a = torch.zeros(n, N_A, device="cuda")
        nerf.bwd_stash(ctx, inp["w_den"][lo:hi], inp["w_rgb"][lo:hi], d_a)
    torch.cuda.synchronize()
    StashCache.release(ctx["lease"])
    return density.clone(), rgb.clone(), d_a, ctx["stash"].aux_bias is not None


@pytest.mark.parametrize("D,skip", TRUNKS)
@pytest.mark.parametrize("prec_name", ["f16", "bf16"])
def test_launch_decomposition_invariance(D, skip, prec_name):
    prec = _prec(prec_name)
    nerf, inp = _nerf(D, skip), _inputs()
    den, rgb, d_a, _ = _run(nerf, prec, inp, 0, N)
    assert bool(torch.isfinite(den).all()) and bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(d_a).all())
    assert float(den.abs().max()) > 0 and float(rgb.abs().max()) > 0 and float(d_a.abs().max()) > 0
    lo = 0
    for m in SLICES:
        den_s, rgb_s, d_a_s, _ = _run(nerf, prec, inp, lo, lo + m)
        assert torch.equal(den_s, den[lo:lo + m]), ("density", D, prec_name, lo, m)
        assert torch.equal(rgb_s, rgb[lo:lo + m]), ("rgb", D, prec_name, lo, m)
        assert torch.equal(d_a_s, d_a[lo:lo + m]), ("d_a", D, prec_name, lo, m)
        lo += m
    assert lo == N


@pytest.mark.parametrize("ray_bias", [True, False])
@pytest.mark.parametrize("prec_name", ["f16", "bf16"])
def test_forward_only_render_equals_training_forward(ray_bias, prec_name):
    """nerf_fwdB<false> (nothing stashed, AUX1 rebuilt in the kernel) against nerf_fwdB<true>; with the per-ray fp32 head rows
    (aux_bias) head layer 0 never reads the AUX1 units of xbuf, without them it multiplies them: both paths."""
    prec = _prec(prec_name)
    nerf, inp = _nerf(8, 4), _inputs()
    nerf.ray_bias = ray_bias
    den, rgb, _, has_rows = _run(nerf, prec, inp, 0, N, backward=False)
    assert has_rows == ray_bias
    with torch.no_grad():
        den_r, rgb_r, _, has_rows_r = _run(nerf, prec, inp, 0, N, train=False)
    assert has_rows_r == ray_bias
    assert float(den.abs().max()) > 0 and float(rgb.abs().max()) > 0
    assert torch.equal(den_r, den) and torch.equal(rgb_r, rgb)


@pytest.mark.parametrize("prec_name", ["f16", "bf16"])
def test_small_selection_dense_vs_eliminated(prec_name):
    """mode-4 launches below one workgroup: 3 rays x ((16 + 16) + 4 samples), so the selection's device count is at most 108 (< 128,
    in general no multiple of 32) -- tests/test_gpu_bg_select.py renders 96 and 70 rays, whose counts span many workgroups.  (A count
    of 0 cannot occur: the outside samples are always selected.)"""
    from tests._build import build_system
    from tests._util import synth_rays

    prec = _prec(prec_name)
    res = {}
    for dense in (True, False):
        emb, neuconw, nerf, rdr = build_system(W=256, n_a=48, n_vocab=64, nerf_w=256, color_hidden=256, head=128, seed=5,
                                               prec=prec, n_samples=16, n_importance=16)
        rdr.bg_dense = dense
        rays, ts, label, _ = synth_rays(3, 7, 64)
        rays = rays.clone()
        rays[:, 6], rays[:, 7] = 0.6, 3.6  # near / far outside the unit sphere on both ends (test_gpu_bg_select.py)
        res[dense] = rdr.render(rays.cuda(), ts.cuda(), label.cuda(), perturb_overwrite=0,
                                background_rgb=torch.zeros(1, 3).cuda(), cos_anneal_ratio=0.3)
    od, oe = res[True], res[False]
    frac = float(od["inside_sphere"].float().mean())
    assert 0.0 < frac < 1.0, frac  # both kinds of primary samples: the list is a proper subset
    for k in ("color", "depth", "weights_sum", "weights", "color_bg"):
        assert torch.equal(od[k], oe[k]), (k, float((od[k] - oe[k]).abs().max()))
