"""GPU: the colour-network kernels (csrc/ncw_color.hip color_fwd_kernel / color_render_kernel / color_bwd_kernel) at their shape
edges: every compiled width key, the depths that take another branch of the weight-ring prefetch chain (n_head = 1, n_head >= 3,
n_lin = 2, n_lin = 8), n_a at the end of the AUX1 operand (27 + 69 = 96), ray-indexed points (NcwPoints mode 1 / 2) with the three
paths of accumulate_d_a, and the forward-only render of every instance.

  K0 (64, 32, 64)   K1 (64, 128, 256)   K2 (256, 128, 256)   K3 (512, 128, 256)      = (d_feature, head_channels, d_hidden)

1. EXACT: a column of an MFMA depends on nothing but its own point, so the same points in another launch decomposition give the
   same bits (rgb, d normals, d_a, d_feat).  2. EXACT: color_render_kernel = color_fwd_kernel, every instance, per-ray fp32 head
   rows on and off.  3. / 4. against the fp64 oracle + autograd: rgb in the max norm, the adjoints of (normals, feat, a) and every
   parameter gradient in L2 (tests/test_gpu_color_nerf.py says why).

Bounds of 3. and 4.  Default depth (static_head_layers 2, n_layers 4; all of part 4): TOL of tests/test_gpu_color_nerf.py as it is.
Every other depth: max(TOL[prec], 2 x floor), where the floor is the error against the same oracle of the oracle's own network with
the weight and the input of every Linear rounded ONCE to the 16-bit type, accumulated in fp64 (tests/_color_emul.py) -- a number that
does not come from the kernels.  fp32: TOL["f32"], and at most n // 200 points whose adjoint leaves the oracle by more than 1e-4
of the tensor's max (ReLU masks that flip in fp32).  That cap is a condition on the SEEDS: torch's own fp32 evaluation of the same
networks on the CPU stays within it for every case here (test_fp32_flip_cap_on_the_cpu, no GPU needed): it flips no row at all in
any of them, and neither do the fp32 kernels (0 of 4003 points in every case of part 3).

Measured on MI355X (printed by the tests: `gpu` = out / adj / grad of the kernels, `floor` = of the emulation):
  part 3, n = 4003, key head/trunk/n_a (static_head_layers / n_layers / n_a):
  K0 1/1/1  f32   gpu 1.09e-07 / 2.16e-07 / 3.27e-07   floor -
  K0 1/1/1  f16   gpu 5.53e-05 / 1.19e-02 / 1.14e-02   floor 1.09e-04 / 1.93e-02 / 1.75e-02
  K0 1/1/1  bf16  gpu 7.95e-04 / 4.88e-02 / 4.40e-02   floor 6.90e-04 / 5.08e-02 / 4.52e-02
  K0 3/2/69 f32   gpu 1.17e-07 / 2.54e-07 / 4.66e-07   floor -
  K0 3/2/69 f16   gpu 3.06e-05 / 1.62e-02 / 3.34e-02   floor 4.01e-05 / 2.41e-02 / 3.29e-02
  K0 3/2/69 bf16  gpu 3.54e-04 / 6.67e-02 / 1.51e-01   floor 3.45e-04 / 8.02e-02 / 1.17e-01
  K0 4/7/48 f32   gpu 1.16e-07 / 3.50e-07 / 1.77e-06   floor -
  K0 4/7/48 f16   gpu 1.25e-05 / 3.84e-02 / 2.51e-02   floor 1.47e-05 / 2.76e-02 / 2.63e-02
  K0 4/7/48 bf16  gpu 1.38e-04 / 9.66e-02 / 9.57e-02   floor 1.37e-04 / 1.04e-01 / 1.01e-01
  K1 2/4/48 f32   gpu 1.27e-07 / 4.97e-07 / 1.01e-06   floor -
  K1 2/4/48 f16   gpu 1.21e-05 / 2.45e-02 / 2.53e-02   floor 1.46e-05 / 3.31e-02 / 3.27e-02   (bound: TOL)
  K1 2/4/48 bf16  gpu 1.05e-04 / 8.21e-02 / 8.28e-02   floor 1.10e-04 / 9.36e-02 / 1.00e-01   (bound: TOL)
  K1 1/1/16 f32   gpu 1.24e-07 / 3.06e-07 / 8.36e-07   floor -
  K1 1/1/16 f16   gpu 4.20e-05 / 1.28e-02 / 1.28e-02   floor 6.02e-05 / 2.08e-02 / 2.13e-02
  K1 1/1/16 bf16  gpu 6.04e-04 / 4.72e-02 / 4.69e-02   floor 5.25e-04 / 5.20e-02 / 5.31e-02
  K2 1/4/48 f32   gpu 1.17e-07 / 5.39e-07 / 1.02e-06   floor -
  K2 1/4/48 f16   gpu 9.91e-07 / 1.24e-02 / 1.39e-02   floor 1.53e-05 / 3.01e-02 / 3.25e-02
  K2 1/4/48 bf16  gpu 1.21e-04 / 8.00e-02 / 8.83e-02   floor 1.07e-04 / 8.32e-02 / 8.88e-02
  K2 4/1/69 f32   gpu 1.19e-07 / 4.65e-07 / 4.81e-07   floor -
  K2 4/1/69 f16   gpu 9.55e-07 / 1.24e-02 / 1.26e-02   floor 4.02e-05 / 3.12e-02 / 3.13e-02
  K2 4/1/69 bf16  gpu 3.12e-04 / 7.47e-02 / 7.45e-02   floor 3.64e-04 / 8.22e-02 / 8.27e-02
  K3 2/4/48 f32   gpu 1.21e-07 / 6.33e-07 / 7.01e-07   floor -
  K3 2/4/48 f16   gpu 4.21e-07 / 1.25e-02 / 1.35e-02   floor 1.48e-05 / 3.20e-02 / 3.32e-02   (bound: TOL)
  K3 2/4/48 bf16  gpu 1.06e-04 / 8.57e-02 / 8.95e-02   floor 1.08e-04 / 8.95e-02 / 1.10e-01   (bound: TOL)
  K3 3/7/1  f32   gpu 1.23e-07 / 7.63e-07 / 8.20e-07   floor -
  K3 3/7/1  f16   gpu 1.21e-07 / 3.22e-02 / 2.08e-02   floor 1.30e-05 / 3.82e-02 / 3.79e-02
  K3 3/7/1  bf16  gpu 9.92e-05 / 1.22e-01 / 1.08e-01   floor 1.15e-04 / 1.19e-01 / 1.10e-01
  part 4, static_head_layers 2, n_layers 4, n_a 48, R x S rays (bound: TOL; fp32: no flipped point in any case):
  K0 mode 1 13 x 5  f32   gpu 1.01e-07 / 3.46e-07 / 3.76e-07   floor -
  K0 mode 1 13 x 5  f16   gpu 7.46e-06 / 8.01e-03 / 8.91e-03   floor 1.09e-05 / 4.13e-02 / 5.57e-02
  K0 mode 1  7 x 32 f32   gpu 1.06e-07 / 3.19e-07 / 3.87e-07   floor -
  K0 mode 1  7 x 32 f16   gpu 7.82e-06 / 1.94e-02 / 2.20e-02   floor 9.65e-06 / 2.09e-02 / 2.44e-02
  K0 mode 1  5 x 40 f32   gpu 1.08e-07 / 3.08e-07 / 2.68e-06   floor -
  K0 mode 1  5 x 40 f16   gpu 1.14e-05 / 3.62e-03 / 1.12e-02   floor 9.70e-06 / 2.66e-02 / 2.53e-02
  K0 mode 2 13 x 5  f32   gpu 1.01e-07 / 3.29e-07 / 3.57e-07   floor -
  K0 mode 2 13 x 5  f16   gpu 9.33e-06 / 9.96e-03 / 1.20e-02   floor 8.49e-06 / 3.32e-02 / 5.33e-02
  K0 mode 2  7 x 32 f32   gpu 9.93e-08 / 3.04e-07 / 3.82e-07   floor -
  K0 mode 2  7 x 32 f16   gpu 9.30e-06 / 1.50e-02 / 1.58e-02   floor 1.17e-05 / 1.89e-02 / 2.12e-02
  K0 mode 2  5 x 40 f32   gpu 1.05e-07 / 3.34e-07 / 2.53e-06   floor -
  K0 mode 2  5 x 40 f16   gpu 8.58e-06 / 1.43e-02 / 3.82e-02   floor 9.69e-06 / 2.05e-02 / 2.07e-02
  K2 mode 1 13 x 5  f32   gpu 1.04e-07 / 5.90e-07 / 1.48e-06   floor -
  K2 mode 1 13 x 5  f16   gpu 3.06e-07 / 1.63e-03 / 1.51e-03   floor 1.33e-05 / 4.27e-02 / 5.26e-02
  K2 mode 1  7 x 32 f32   gpu 1.08e-07 / 5.72e-07 / 6.10e-07   floor -
  K2 mode 1  7 x 32 f16   gpu 3.49e-07 / 1.63e-02 / 1.69e-02   floor 1.40e-05 / 3.20e-02 / 3.94e-02
  K2 mode 1  5 x 40 f32   gpu 1.12e-07 / 5.66e-07 / 1.84e-06   floor -
  K2 mode 1  5 x 40 f16   gpu 2.51e-07 / 3.74e-03 / 4.56e-03   floor 1.46e-05 / 4.26e-02 / 4.35e-02
  K2 mode 2 13 x 5  f32   gpu 9.77e-08 / 5.69e-07 / 1.08e-06   floor -
  K2 mode 2 13 x 5  f16   gpu 2.94e-07 / 1.84e-03 / 1.77e-03   floor 1.29e-05 / 6.46e-03 / 6.76e-03
  K2 mode 2  7 x 32 f32   gpu 1.13e-07 / 5.64e-07 / 1.12e-06   floor -
  K2 mode 2  7 x 32 f16   gpu 3.15e-07 / 1.42e-03 / 1.70e-03   floor 1.17e-05 / 3.71e-02 / 4.28e-02
  K2 mode 2  5 x 40 f32   gpu 1.02e-07 / 5.74e-07 / 1.24e-06   floor -
  K2 mode 2  5 x 40 f16   gpu 2.89e-07 / 1.50e-03 / 1.94e-03   floor 1.33e-05 / 2.86e-02 / 2.99e-02
  d_a_rows: largest |sum of a ray's rows - d_a| / (S x 2^-23 x sum |rows|) over all of part 4: 0.19
"""
import pytest
import torch

from tests import _color_emul as E
from tests.test_gpu_color_nerf import TOL, _jitter, _prec, _unit, _wgrads, flipped_points, fro_err  # noqa: F401

gpu = pytest.mark.gpu
NCW_E_BADARG, NCW_E_UNSUPPORTED = -1, -2  # include/neuconw_hip.h

N = 419                     # 13 tiles + 3 points: 3 full workgroups + one workgroup with a full tile, a 3-point tile and two idle waves
SLICES = (1, 33, 129, 256)  # consecutive slices of the same points (sum = N)
N_ORACLE = 4003             # 125 tiles + 3 points: the size class the project's tolerances were measured at
KEYS = list(E.KEYS)
# (width key, static_head_layers, n_layers, n_a)
DEPTHS = [("K0", 1, 1, 1),    # both shortest branches at once: n_head = 1, n_lin = 2
          ("K0", 3, 2, 69),   # AUX1 completely full
          ("K0", 4, 7, 48),   # n_lin = 8: the bound of the struct arrays
          ("K1", 2, 4, 48),   # the key no unit test trained, default depth
          ("K1", 1, 1, 16),
          ("K2", 1, 4, 48),
          ("K2", 4, 1, 69),
          ("K3", 2, 4, 48),   # backward and weight gradients at the shipped width
          ("K3", 3, 7, 1)]
RAY_SHAPES = [(13, 5),   # 65 points: every tile spans several rays (per-lane atomics), the last tile holds one point
              (7, 32),   # every tile is exactly one ray: the wave-uniform shuffle-reduced atomic
              (5, 40)]   # tiles straddle a ray boundary at varying offsets


def _dev(inp, lo=None, hi=None):
    return {k: v[lo:hi].contiguous().cuda() for k, v in inp.items()}


def _feat_arena(prec, n, W, feat):
    from neuralrecon_w_amd.stash import StashArena

    ar = StashArena("cuda", prec, n)
    fid, dfid = ar.new(W // 32), ar.new(W // 32)
    ar.allocate(zero=True)
    ar.from_rows(fid, feat)
    return ar, fid, dfid


def _train_step(cn, prec, d, n):
    """mode 0, one launch each: fwd_stash(train=True) + bwd_stash with d_a -> (rgb, d_grad, d_a, d_feat, ctx)"""
    from neuralrecon_w_amd.neuconw import points_struct

    ar, fid, dfid = _feat_arena(prec, n, cn.d_feature, d["feat"])
    rgb, ctx = cn.fwd_stash(points_struct(x=d["x"], rays_d=d["dirs"]), n, prec, d["normals"], d["a"], ar.ptr(fid))
    d_grad, d_a = torch.zeros(n, 3, device="cuda"), torch.zeros(n, cn.n_a, device="cuda")
    cn.bwd_stash(ctx, d["w_rgb"], d_grad, d_a, ar.ptr(dfid))
    d_feat = ar.to_rows(dfid, cn.d_feature)
    torch.cuda.synchronize()
    ctx["_feat_arena"] = ar
    return rgb.clone(), d_grad, d_a, d_feat, ctx


# ---- 1. launch decomposition -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("prec_name", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("key", KEYS)
def test_launch_decomposition_invariance(key, prec_name):
    """fp16 runs its defaults: weights as hi + lo pairs, activations too at K2 / K3.  In mode 0 every element of d_a receives one
    atomic (plus zeros from idle waves): no summation order."""
    from neuralrecon_w_amd.stash import StashCache

    prec = _prec(prec_name)
    cn = E.make_net(key, 2, 4, 48, seed=41).cuda()
    inp = E.point_inputs(N, cn.d_feature, cn.n_a, seed=42)
    full = _train_step(cn, prec, _dev(inp), N)
    StashCache.release(full[4]["lease"])
    if prec_name == "f16":
        assert full[4]["plan"].net.act_split == int(key in ("K2", "K3")) and full[4]["plan"].net.w_f_lo
    names = ("rgb", "d_grad", "d_a", "d_feat")
    for name, t in zip(names, full):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0, name
    lo = 0
    for m in SLICES:
        part = _train_step(cn, prec, _dev(inp, lo, lo + m), m)
        StashCache.release(part[4]["lease"])
        for name, whole, got in zip(names, full, part):
            assert torch.equal(got, whole[lo:lo + m]), (name, key, prec_name, lo, m)
        lo += m
    assert lo == N


# ---- 2. forward-only render --------------------------------------------------------------------------------------------------------
def _render_cases():
    out = []
    for key in KEYS:
        out.append((key, "f32", None, None, None))
        for rb in (True, False):
            out.append((key, "bf16", None, None, rb))
            out.append((key, "f16", False, None, rb))
            out.append((key, "f16", True, False, rb))
            if key in ("K2", "K3"):
                out.append((key, "f16", True, True, rb))
    return out


@gpu
@pytest.mark.parametrize("key,prec_name,weight_split,act_split,ray_bias", _render_cases())
def test_forward_only_render_equals_training_forward(key, prec_name, weight_split, act_split, ray_bias):
    """color_render_kernel (nothing stashed) against color_fwd_kernel: the plain instances, fp16 with the weights as pairs, with the
    activations as pairs too; with the per-ray fp32 head rows layer 0 of the head multiplies a zero AUX1 operand, without them the
    real one.  The switches are set before the first forward of a fresh module (the plan is built once per precision)."""
    from neuralrecon_w_amd.neuconw import points_struct
    from neuralrecon_w_amd.stash import StashCache

    prec = _prec(prec_name)
    cn = E.make_net(key, 2, 4, 48, seed=41).cuda()
    if weight_split is not None:
        cn.weight_split = weight_split
    if act_split is not None:
        cn.act_split = act_split
    if ray_bias is not None:
        cn.ray_bias = ray_bias
    d = _dev(E.point_inputs(N, cn.d_feature, cn.n_a, seed=42))
    ar, fid, _ = _feat_arena(prec, N, cn.d_feature, d["feat"])
    pts = points_struct(x=d["x"], rays_d=d["dirs"])
    out = {}
    for train in (True, False):
        with torch.set_grad_enabled(train):
            rgb, ctx = cn.fwd_stash(pts, N, prec, d["normals"], d["a"], ar.ptr(fid), train=train)
        torch.cuda.synchronize()
        net = ctx["plan"].net
        assert bool(net.w_f_lo) == bool(weight_split) and net.act_split == int(bool(weight_split) and bool(act_split))
        assert (ctx["stash"].aux_bias is not None) == bool(ray_bias)
        assert (ctx["stash"].aux1 is not None) == train  # NULL aux1 selects color_render_kernel
        out[train] = rgb.clone()
        StashCache.release(ctx["lease"])
    assert bool(torch.isfinite(out[True]).all()) and float(out[True].abs().max()) > 0
    assert torch.equal(out[False], out[True])


# ---- 3. / 4. against the fp64 oracle -----------------------------------------------------------------------------------------------
def _bounds(c, prec_name, default_depth):
    t = TOL[prec_name]
    if prec_name == "f32":
        return (t["out"], t["adj"], t["grad"]), None
    fl = E.floor(c, prec_name)
    if default_depth:
        return (t["out"], t["adj"], t["grad"]), fl
    return (max(t["out"], 2 * fl[0]), max(t["adj"], 2 * fl[1]), max(t["grad"], 2 * fl[2])), fl


def _check_vs_oracle(tag, c, prec_name, got, default_depth, n, per_point):
    """got: dict(rgb=, adj=dict(normals, feat, a), grads=) from the kernels; per_point: the adjoints that have one row per point"""
    errs = E.errors(got, c["ref"])
    bound, fl = _bounds(c, prec_name, default_depth)
    per = {k: fro_err(got["grads"][k], c["ref"]["grads"][k]) for k in c["ref"]["grads"]}
    print("%s %s: gpu %.2e / %.2e / %.2e   floor %s   bound %.2e / %.2e / %.2e   (worst gradient: %s)"
          % ((tag, prec_name) + errs + ("-" if fl is None else "%.2e / %.2e / %.2e" % fl,) + bound + (max(per, key=per.get),)))
    assert set(got["grads"]) == set(c["ref"]["grads"])
    if prec_name == "f32":
        nflip = max(flipped_points(got["adj"][k], c["ref"]["adj"][k]) for k in per_point)
        print("   fp32: %d of %d points beyond 1e-4 (ReLU mask flips against fp64)" % (nflip, n))
        assert nflip <= n // 200
    assert errs[0] < bound[0] and errs[1] < bound[1] and errs[2] < bound[2], (errs, bound)


@gpu
@pytest.mark.parametrize("prec_name", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("key,n_head,n_layers,n_a", DEPTHS)
def test_depths_and_n_a_vs_oracle(key, n_head, n_layers, n_a, prec_name):
    """the harness of tests/test_gpu_color_nerf.py::test_color_net_train_vs_oracle over the depths and n_a edges"""
    from neuralrecon_w_amd.stash import StashCache

    prec = _prec(prec_name)
    c = E.case(key, n_head, n_layers, n_a, n=N_ORACLE)
    cn = E.gpu_net(c)
    assert (cn.n_head, cn.n_lin, cn.n_a) == (n_head, n_layers + 1, n_a)
    rgb, d_grad, d_a, d_feat, ctx = _train_step(cn, prec, _dev(c["inp"]), N_ORACLE)
    grads, _keep = _wgrads(cn, ctx, prec, N_ORACLE)
    StashCache.release(ctx["lease"])
    got = dict(rgb=rgb.cpu(), adj=dict(normals=d_grad.cpu(), feat=d_feat.cpu(), a=d_a.cpu()), grads=grads)
    _check_vs_oracle("colour %s head %d trunk %d n_a %d" % (key, n_head, n_layers, n_a), c, prec_name, got,
                     (n_head, n_layers) == (2, 4), N_ORACLE, ("normals", "feat", "a"))


@gpu
@pytest.mark.parametrize("prec_name", ["f32", "f16"])
@pytest.mark.parametrize("R,S", RAY_SHAPES)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("key", ["K0", "K2"])
def test_ray_indexed_points(key, mode, R, S, prec_name):
    """NcwPoints mode 1 / 2: a, the per-ray head rows and d_a are indexed by ray = p / per_ray.  Against the oracle on the fp64 points;
    then the d_a_rows form of the backward on the same forward: same d_grad / d_feat bit for bit, every row written and nothing
    beyond them, rows that add up to the atomically accumulated d_a (S x 2^-23 x sum |rows|: the worst case of an fp32 sum of S
    terms in any order), and ncw_ray_sum_rows = the fp32 sum in ascending sample order, bit for bit."""
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd.neuconw import points_struct
    from neuralrecon_w_amd.stash import StashCache

    prec, n = _prec(prec_name), R * S
    c = E.case(key, 2, 4, 48, rays=(R, S), mode=mode)
    cn = E.gpu_net(c)
    n_a, W = cn.n_a, cn.d_feature
    d = _dev(c["inp"])
    pts = points_struct(rays_o=d["rays_o"], rays_d=d["dirs"], z=d["z"], sample_dist=d["sample_dist"], mode=mode)
    assert pts.per_ray == S and pts.mode == mode
    ar, fid, dfid = _feat_arena(prec, n, W, d["feat"])
    rgb, ctx = cn.fwd_stash(pts, n, prec, d["normals"], d["a"], ar.ptr(fid))
    assert (ctx["stash"].aux_bias is not None) == (prec_name != "f32")  # 16-bit: one fp32 head row per RAY
    d_grad, d_a = torch.zeros(n, 3, device="cuda"), torch.zeros(R, n_a, device="cuda")
    cn.bwd_stash(ctx, d["w_rgb"], d_grad, d_a, ar.ptr(dfid))
    d_feat = ar.to_rows(dfid, W)
    grads, _keep = _wgrads(cn, ctx, prec, n)
    got = dict(rgb=rgb.cpu(), adj=dict(normals=d_grad.cpu(), feat=d_feat.cpu(), a=d_a.cpu()), grads=grads)
    _check_vs_oracle("colour %s mode %d %d x %d" % (key, mode, R, S), c, prec_name, got, True, n, ("normals", "feat"))
    # ---- the d_a_rows form: exactly [n, n_a], a filled neighbour allocated right after it
    rows = torch.full((n, n_a), float("nan"), device="cuda")
    guard = torch.full((4096,), 7.25, device="cuda")
    d_grad2 = torch.zeros(n, 3, device="cuda")
    ar2, _, dfid2 = _feat_arena(prec, n, W, d["feat"])
    cn.bwd_stash(ctx, d["w_rgb"], d_grad2, None, ar2.ptr(dfid2), d_a_rows=rows)
    d_feat2 = ar2.to_rows(dfid2, W)
    summed = torch.empty(R, n_a, device="cuda")
    L.check(L.get_lib().ncw_ray_sum_rows(L.ptr(rows), R, S, n_a, L.ptr(summed), 0, L.stream_ptr(rows.device)), "ncw_ray_sum_rows")
    torch.cuda.synchronize()
    StashCache.release(ctx["lease"])
    assert bool(torch.isfinite(rows).all()) and bool((guard == 7.25).all())
    assert torch.equal(d_grad2, d_grad) and torch.equal(d_feat2, d_feat)
    r3 = rows.view(R, S, n_a)
    slack = S * 2.0 ** -23 * r3.double().abs().sum(1)
    diff = (r3.double().sum(1) - d_a.double()).abs()
    print("   d_a_rows: largest |sum of rows - d_a| / bound %.3g" % float((diff / slack.clamp_min(1e-300)).max()))
    assert bool((diff <= slack).all())
    acc = torch.zeros(R, n_a, device="cuda")
    for i in range(S):
        acc += r3[:, i]
    assert torch.equal(summed, acc)


# ---- 5. host-side edges ------------------------------------------------------------------------------------------------------------
def _ctor(**kw):
    import neuralrecon_w_amd as nw

    args = dict(d_feature=256, mode="idr", d_in=9, d_out=3, d_hidden=256, n_layers=4, head_channels=128, in_channels_dir_a=48,
                static_head_layers=2, weight_norm=True, multires_view=4)
    args.update(kw)
    return nw.RenderingNetwork(**args)


@pytest.mark.parametrize("kw", [dict(d_feature=128), dict(d_feature=64, head_channels=64, d_hidden=64), dict(d_hidden=128),
                                dict(d_feature=256, head_channels=32, d_hidden=64), dict(d_feature=80),
                                dict(static_head_layers=5), dict(n_layers=8), dict(in_channels_dir_a=70)])
def test_constructor_refuses_what_no_kernel_covers(kw):
    with pytest.raises(NotImplementedError):
        _ctor(**kw)


@pytest.mark.parametrize("key", KEYS)
def test_constructor_accepts_the_bounds(key):
    W, head, hidden = E.KEYS[key]
    cn = _ctor(d_feature=W, head_channels=head, d_hidden=hidden, static_head_layers=4, n_layers=7, in_channels_dir_a=69)
    assert (cn.n_head, cn.n_lin, cn.n_a) == (4, 8, 69)


def _ray_cases():
    return [(k, 2, 4, 48, None, rs, m) for k in ("K0", "K2") for rs in RAY_SHAPES for m in (1, 2)]


@pytest.mark.parametrize("key,n_head,n_layers,n_a,n,rays,mode", [d + (N_ORACLE, None, 0) for d in DEPTHS] + _ray_cases())
def test_fp32_flip_cap_on_the_cpu(key, n_head, n_layers, n_a, n, rays, mode):
    """the seeds of parts 3 and 4 leave room under the flipped-rows cap: torch's fp32 evaluation of the same network and inputs on the
    CPU flips at most n // 200 rows against the fp64 oracle"""
    c = E.case(key, n_head, n_layers, n_a, n=n, rays=rays, mode=mode)
    total = n if rays is None else rays[0] * rays[1]
    nflip = E.flipped_rows_fp32(c)
    print("fp32 on the CPU, %s: %d of %d rows flipped (cap %d)" % ((key, n_head, n_layers, n_a, rays, mode), nflip, total, total // 200))
    assert nflip <= total // 200


@gpu
def test_entry_points_refuse_before_any_launch():
    """NcwPoints mode 4 (point selections are the background NeRF's): NCW_E_UNSUPPORTED; an fp32 call with residual matrices
    (w_f_lo set: they are 16-bit): NCW_E_BADARG.  Both without a launch: the outputs keep their fill."""
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd.neuconw import points_struct
    from neuralrecon_w_amd.stash import StashCache

    prec, n = L.PREC_F32, 65
    cn = E.make_net("K0", 2, 4, 16, seed=41).cuda()
    d = _dev(E.point_inputs(n, cn.d_feature, cn.n_a, seed=42))
    ar, fid, dfid = _feat_arena(prec, n, cn.d_feature, d["feat"])
    pts = points_struct(x=d["x"], rays_d=d["dirs"])
    rgb, ctx = cn.fwd_stash(pts, n, prec, d["normals"], d["a"], ar.ptr(fid))
    net, st, lib, stream = ctx["plan"].net, ctx["stash"], L.get_lib(), L.stream_ptr(rgb.device)
    assert not net.w_f_lo

    def both(net_, pts_):
        out = torch.full((n, 3), 7.25, device="cuda")
        r_f = lib.ncw_color_fwd(net_, prec, pts_, n, L.ptr(d["normals"]), L.ptr(d["a"]), ar.ptr(fid), L.ptr(out), st, stream)
        d_grad, d_a = torch.full((n, 3), 7.25, device="cuda"), torch.full((n, cn.n_a), 7.25, device="cuda")
        r_b = lib.ncw_color_bwd(net_, prec, pts_, n, L.ptr(rgb), L.ptr(d["w_rgb"]), L.ptr(d_grad), L.ptr(d_a), None, ar.ptr(dfid), st,
                                stream)
        torch.cuda.synchronize()
        assert bool((out == 7.25).all()) and bool((d_grad == 7.25).all()) and bool((d_a == 7.25).all())
        return r_f, r_b

    sel = L.NcwPoints.from_buffer_copy(pts)
    sel.mode = 4
    assert both(net, sel) == (NCW_E_UNSUPPORTED, NCW_E_UNSUPPORTED)
    bad = L.NcwColorNet.from_buffer_copy(net)
    bad.w_f_lo = net.w_f
    assert both(bad, pts) == (NCW_E_BADARG, NCW_E_BADARG)
    assert float(ar.to_rows(dfid, cn.d_feature).abs().max()) == 0  # (allocated zeroed, never written)
    StashCache.release(ctx["lease"])
