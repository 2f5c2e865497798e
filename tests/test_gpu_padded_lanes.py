"""Lanes past n contribute nothing: the other half of a ragged launch.

tests/test_gpu_wgrad.py proves the weight-gradient GEMMs given X = 0 in the padded lanes of the last tile; here the modules
that WRITE those stashes (SDF net, colour net, background NeRF; forward, backward, weight gradients) are held to it.  Each
network runs
  (a)  n = 453 points: 15 tiles, 5 valid lanes in the last one,
  (a') the same again with the leased stash arena pre-filled with the byte 0x3C (a finite non-zero value in f32, bf16 and
       fp16): whatever a kernel leaves unwritten in a tile the GEMMs read is then not zero,
  (b)  n = 480: the same 453 points followed by 27 real points whose upstream cotangents are all zero.
At 15 tiles every split-K factor of stash.WgradBatch._plan is 1, so a dense element receives one addend per product.
fp32 (ordered GEMMs): the packed gradient arena is bit-identical across the three runs.  16-bit modes: per tensor the runs differ
by at most 8 x 2^-24 x max|g| -- the reordering of the few f32 atomic addends of a dense element; one unmasked lane adds a whole
point, about 1/453 of the gradient, three orders of magnitude more.  The per-point outputs and input adjoints of the first 453
points are bit-identical between the runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N_A, N_B = 453, 480
FILL = 0x3C


def _prec(name):
    import neuralrecon_w_amd as nw

    return {"f32": nw.PREC_F32, "bf16": nw.PREC_BF16, "f16": nw.PREC_F16}[name]


def _unit(n, g):
    d = torch.randn(n, 3, generator=g)
    return d / d.norm(dim=-1, keepdim=True)


def _masked(t):
    """a cotangent of the 480-point run: zero for the 27 extra points"""
    t = t.clone()
    t[N_A:] = 0
    return t


def _grad_arena(mod, ctx, prec, n):
    from neuralrecon_w_amd.stash import WgradBatch

    plan = ctx["plan"]
    plan.g_arena.zero_()
    batch = WgradBatch(plan.g_arena.device, prec, n)
    mod.add_wgrads(ctx, batch)
    assert (n + 31) // 32 < 16  # fewer than 16 tiles: every split-K factor of WgradBatch._plan is 1 (tiles // 8 <= 1)
    batch.run()
    torch.cuda.synchronize()
    return plan.g_arena.clone()


def _tensors(plan, g):
    """the dense gradient matrices and bias gradients packed in a gradient arena"""
    for (off, r, c), boff in zip(plan._dense, plan._dense_b):
        yield g[off:off + r * c]
        if boff is not None:
            yield g[boff:boff + r]


def _check(prec_name, plan, runs):
    """runs: {name: (gradient arena, [per-point tensors])}"""
    ga, pa = runs["a"]
    assert float(ga.abs().max()) > 0
    for name in ("a_filled", "b"):
        g, per = runs[name]
        for k, (u, v) in enumerate(zip(pa, per)):
            assert torch.equal(u[:N_A].view(torch.int32), v[:N_A].view(torch.int32)), (name, "per-point tensor %d" % k)
        if prec_name == "f32":
            assert torch.equal(ga.view(torch.int32), g.view(torch.int32)), name
        else:
            worst = 0.0
            for k, (u, v) in enumerate(zip(_tensors(plan, ga), _tensors(plan, g))):
                bound = 8 * 2.0 ** -24 * float(u.abs().max())
                diff = float((u - v).abs().max())
                worst = max(worst, diff / bound if bound > 0 else (0.0 if diff == 0 else float("inf")))
                assert diff <= bound, (name, "tensor %d" % k, diff, bound)
            print("padded lanes %s, run %s: largest difference / bound %.3g" % (prec_name, name, worst))


def _three_runs(run, arenas):
    """run(n, filled) -> (ctx, gradient arena, per-point tensors); arenas(ctx) -> the stash arenas to pre-fill"""
    from neuralrecon_w_amd.stash import StashCache

    out = {}
    ctx, g, per = run(N_A, None)
    out["a"] = (g, per)
    StashCache.release(ctx["lease"])  # the next forward of the same size takes this arena again
    for ar in arenas(ctx):
        ar.buf.fill_(FILL)
    ctx2, g, per = run(N_A, ctx)
    assert ctx2["arena"] is ctx["arena"]
    out["a_filled"] = (g, per)
    _, g, per = run(N_B, None)
    out["b"] = (g, per)
    return ctx["plan"], out


@pytest.mark.parametrize("prec_name", ["f32", "bf16", "f16"])
def test_sdf_net_padded_lanes(prec_name):
    from neuralrecon_w_amd.neuconw import points_struct
    from tests.test_gpu_sdf import _mk

    W, prec = 64, _prec(prec_name)
    net = _mk(W, 8, (4,), seed=3)
    g = torch.Generator().manual_seed(9)
    x = ((torch.rand(N_B, 3, generator=g) * 2 - 1) * 0.9).cuda()
    w_sdf, w_grad = torch.randn(N_B, generator=g).cuda(), torch.randn(N_B, 3, generator=g).cuda()
    w_feat = (torch.randn(N_B, W, generator=g) * 0.1).cuda()

    def run(n, _prev):
        cot = [t[:n].contiguous() for t in ((w_sdf, w_grad, w_feat) if n == N_A else map(_masked, (w_sdf, w_grad, w_feat)))]
        sdf, grad, ctx = net.fwd_stash(points_struct(x=x[:n].contiguous()), n, prec)
        feat = ctx["arena"].to_rows(ctx["ids"]["feat"], W)
        ctx["arena"].from_rows(ctx["ids"]["dfeat"], cot[2])
        net.bwd_stash(ctx, cot[0], cot[1])
        return ctx, _grad_arena(net, ctx, prec, n), [sdf.clone(), grad.clone(), feat.clone()]

    plan, runs = _three_runs(run, lambda ctx: [ctx["arena"]])
    _check(prec_name, plan, runs)


@pytest.mark.parametrize("prec_name", ["f32", "bf16", "f16"])
def test_color_net_padded_lanes(prec_name):
    from neuralrecon_w_amd.neuconw import points_struct
    from neuralrecon_w_amd.stash import StashArena
    from tests._build import build_system
    from tests.test_gpu_color_nerf import _jitter

    W, n_a, prec = 64, 16, _prec(prec_name)
    _, neuconw, _, _ = build_system(W=W, n_a=n_a, color_hidden=W, head=32, nerf_w=64, seed=11, prec=prec)
    cn = neuconw.color_net
    _jitter(cn, 1)
    g = torch.Generator().manual_seed(2)
    x = ((torch.rand(N_B, 3, generator=g) * 2 - 1) * 0.9).cuda()
    normals, dirs = torch.randn(N_B, 3, generator=g).cuda(), _unit(N_B, g).cuda()
    feat, a = (0.5 * torch.randn(N_B, W, generator=g)).cuda(), torch.randn(N_B, n_a, generator=g).cuda()
    w_rgb = torch.randn(N_B, 3, generator=g).cuda()

    def run(n, prev):
        d_rgb = (w_rgb if n == N_A else _masked(w_rgb))[:n].contiguous()
        pts = points_struct(x=x[:n].contiguous(), rays_d=dirs[:n].contiguous())
        ar = StashArena("cuda", prec, n)
        fid, dfid = ar.new(W // 32), ar.new(W // 32)
        ar.allocate(zero=True)
        if prev is not None:  # the feature stashes this test owns are pre-filled like the leased arena
            ar.buf.fill_(FILL)
        ar.from_rows(fid, feat[:n].contiguous())
        rgb, ctx = cn.fwd_stash(pts, n, prec, normals[:n].contiguous(), a[:n].contiguous(), ar.ptr(fid))
        d_grad, d_a = torch.zeros(n, 3, device="cuda"), torch.zeros(n, n_a, device="cuda")
        cn.bwd_stash(ctx, d_rgb, d_grad, d_a, ar.ptr(dfid))
        d_feat = ar.to_rows(dfid, W)
        return ctx, _grad_arena(cn, ctx, prec, n), [rgb.clone(), d_grad, d_feat, d_a]

    plan, runs = _three_runs(run, lambda ctx: [ctx["arena"]])
    _check(prec_name, plan, runs)


@pytest.mark.parametrize("prec_name", ["f32", "bf16", "f16"])
def test_nerf_padded_lanes(prec_name):
    """explicit [n, 4] points (NcwPoints mode 0)"""
    from neuralrecon_w_amd.neuconw import points_struct
    from tests._build import build_system
    from tests.test_gpu_color_nerf import _jitter

    n_a, prec = 16, _prec(prec_name)
    _, _, nerf, _ = build_system(W=64, n_a=n_a, nerf_w=64, seed=12, prec=prec)
    _jitter(nerf, 4)
    g = torch.Generator().manual_seed(5)
    x4 = torch.cat([_unit(N_B, g), torch.rand(N_B, 1, generator=g) * 0.9 + 0.05], -1).cuda()
    dirs, a = _unit(N_B, g).cuda(), torch.randn(N_B, n_a, generator=g).cuda()
    w_den, w_rgb = torch.randn(N_B, generator=g).cuda(), torch.randn(N_B, 3, generator=g).cuda()

    def run(n, _prev):
        cot = [t[:n].contiguous() for t in ((w_den, w_rgb) if n == N_A else map(_masked, (w_den, w_rgb)))]
        pts = points_struct(x=x4[:n, :3].contiguous(), rays_d=dirs[:n].contiguous())
        assert pts.mode == 0
        density, rgb, ctx = nerf.fwd_stash(pts, n, prec, a[:n].contiguous(), x4=x4[:n].contiguous())
        d_a = torch.zeros(n, n_a, device="cuda")
        nerf.bwd_stash(ctx, cot[0], cot[1], d_a)
        return ctx, _grad_arena(nerf, ctx, prec, n), [density.clone(), rgb.clone(), d_a]

    plan, runs = _three_runs(run, lambda ctx: [ctx["arena"]])
    _check(prec_name, plan, runs)
