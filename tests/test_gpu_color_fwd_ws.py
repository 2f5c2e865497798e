"""GPU: the weights-stationary colour forward (csrc/ncw_split.hip color_fwdS_kernel: fp16, d_feature 256 / head 128 / trunk 256,
weights and activations as hi + lo pairs, eight waves per workgroup) against the generic register-resident kernel it replaces
(csrc/ncw_color.hip color_fwd_kernel / color_render_kernel <PrecBF16, 8, 4, 8, 2>, still selectable: `.ws_forward = False`,
NcwColorNet.act_split = 2).  The new kernel keeps the generic one's accumulation order per accumulator, so everything is EXACT:
`torch.equal` on rgb and on every forward stash field (aux1, aux2, f, e_i, x_l) over the whole tiles the launch covers, padded
lanes included.

1. new against generic: n = 129 / 419 explicit points, four depths, per-ray fp32 head rows on and off, training and render form;
2. ray-indexed points (NcwPoints mode 1 / 2) whose tiles and workgroups straddle rays;
3. launch decomposition: the same points in launches that end on and next to the tile (32), tile-pair (64) and workgroup (128) edges;
4. the render form = the training form in rgb; with the arena prefilled with NaN the training form writes every forward field
   completely and nothing else, the render form nothing at all.

Depths are (static_head_layers, n_layers, n_a).  The deepest case is (4, 7, 69): n_layers = 7 is n_lin = 8, the bound of the
NcwColorNet arrays -- RenderingNetwork refuses n_layers = 8."""
import copy

import pytest
import torch

from tests import _color_emul as E

gpu = pytest.mark.gpu

KEY = "K2"
DEPTHS = [(2, 4, 48), (1, 2, 1), (4, 7, 69), (3, 3, 16)]
RAY_SHAPES = [(13, 5), (7, 32), (5, 40)]
LAUNCHES = (1, 32, 33, 64, 65, 127, 128, 129)
N = 419
FWD_FIELDS = ("aux1", "aux2", "f", "e", "x")


def _prec():
    from neuralrecon_w_amd import lib as L

    return L.PREC_F16


def _pair(n_head, n_layers, n_a, ray_bias=True, seed=41):
    """the same network twice: through the weights-stationary kernel and through the generic one"""
    base = E.make_net(KEY, n_head, n_layers, n_a, seed=seed)
    nets = {}
    for ws in (True, False):
        cn = copy.deepcopy(base).cuda()
        cn.ws_forward = ws
        cn.ray_bias = ray_bias
        nets[ws] = cn
    return nets


def _dev(inp):
    return {k: v.contiguous().cuda() for k, v in inp.items()}


def _feat_arena(n, W, feat):
    from neuralrecon_w_amd.stash import StashArena

    ar = StashArena("cuda", _prec(), n)
    fid = ar.new(W // 32)
    ar.allocate(zero=True)
    ar.from_rows(fid, feat)
    return ar, fid


def _field_ids(ids):
    out = []
    for name in FWD_FIELDS:
        v = ids[name]
        out += [(name, v)] if isinstance(v, int) else [("%s[%d]" % (name, i), j) for i, j in enumerate(v)]
    return out


def _covered_tiles(n):
    return ((n + 31) // 32 + 3) // 4 * 4  # whole workgroups of four tiles


def _stash_bits(ctx, n):
    """every forward stash field over the tiles the launch covers, as raw 16-bit words"""
    ar = ctx["arena"]
    out = {}
    for name, i in _field_ids(ctx["ids"]):
        off, rb = ar._off[i]
        out[name] = ar.buf[off:off + _covered_tiles(n) * rb * 2048].view(torch.int16).clone()
    return out


def _forward(cn, pts, n, d, feat_ptr, train):
    from neuralrecon_w_amd.stash import StashCache

    with torch.set_grad_enabled(train):
        rgb, ctx = cn.fwd_stash(pts, n, _prec(), d["normals"], d["a"], feat_ptr, train=train)
    torch.cuda.synchronize()
    net = ctx["plan"].net
    assert net.w_f_lo and net.act_split == (1 if cn.ws_forward else 2)
    assert (ctx["stash"].aux_bias is not None) == bool(cn.ray_bias)
    assert (ctx["stash"].aux1 is not None) == train
    out = dict(rgb=rgb.clone(), bits=_stash_bits(ctx, n) if train else None, ctx=ctx)
    StashCache.release(ctx["lease"])
    return out


def _check_pair(nets, pts, n, d, W, tag):
    ar, fid = _feat_arena(n, W, d["feat"])
    got = {ws: {train: _forward(nets[ws], pts, n, d, ar.ptr(fid), train) for train in (True, False)} for ws in (True, False)}
    ref = got[False][True]
    assert bool(torch.isfinite(ref["rgb"]).all()) and float(ref["rgb"].abs().max()) > 0, tag
    assert torch.equal(got[False][False]["rgb"], ref["rgb"]), tag  # (the generic pair: tests/test_gpu_color_edges.py)
    assert torch.equal(got[True][True]["rgb"], ref["rgb"]), ("training form rgb",) + tag
    assert torch.equal(got[True][False]["rgb"], ref["rgb"]), ("render form rgb",) + tag
    assert set(got[True][True]["bits"]) == set(ref["bits"])
    for name, want in ref["bits"].items():
        have = got[True][True]["bits"][name]
        bad = int((have != want).sum())
        assert bad == 0, ("stash field %s: %d of %d words differ" % (name, bad, want.numel()),) + tag


@gpu
@pytest.mark.parametrize("ray_bias", [True, False])
@pytest.mark.parametrize("n_head,n_layers,n_a", DEPTHS)
@pytest.mark.parametrize("n", [129, N])
def test_new_kernel_equals_generic_kernel(n, n_head, n_layers, n_a, ray_bias):
    from neuralrecon_w_amd.neuconw import points_struct

    nets = _pair(n_head, n_layers, n_a, ray_bias)
    W = nets[True].d_feature
    d = _dev(E.point_inputs(n, W, n_a, seed=42))
    _check_pair(nets, points_struct(x=d["x"], rays_d=d["dirs"]), n, d, W, (n, n_head, n_layers, n_a, ray_bias))


@gpu
@pytest.mark.parametrize("R,S", RAY_SHAPES)
@pytest.mark.parametrize("mode", [1, 2])
def test_ray_indexed_points(mode, R, S):
    from neuralrecon_w_amd.neuconw import points_struct

    nets = _pair(2, 4, 48)
    W, n = nets[True].d_feature, R * S
    d = _dev(E.ray_inputs(R, S, W, 48, seed=43))
    pts = points_struct(rays_o=d["rays_o"], rays_d=d["dirs"], z=d["z"], sample_dist=d["sample_dist"], mode=mode)
    assert pts.per_ray == S and pts.mode == mode
    _check_pair(nets, pts, n, d, W, (mode, R, S))


def _rows(cn, d, lo, m):
    """training forward of points [lo, lo + m) in one launch -> rgb and every forward stash field as rows [m, features]"""
    from neuralrecon_w_amd.neuconw import points_struct
    from neuralrecon_w_amd.stash import StashCache

    s = {k: v[lo:lo + m].contiguous() for k, v in d.items()}
    ar, fid = _feat_arena(m, cn.d_feature, s["feat"])
    rgb, ctx = cn.fwd_stash(points_struct(x=s["x"], rays_d=s["dirs"]), m, _prec(), s["normals"], s["a"], ar.ptr(fid))
    out = {"rgb": rgb.clone()}
    for name, i in _field_ids(ctx["ids"]):
        out[name] = ctx["arena"].to_rows(i, 32 * ctx["arena"].rb(i))
    torch.cuda.synchronize()
    assert ctx["plan"].net.act_split == 1
    StashCache.release(ctx["lease"])
    return out


@gpu
def test_launch_decomposition():
    """a column of an MFMA depends on nothing but its own point: the 419 points in one launch against launches of 1 .. 129 points
    taken from them at staggered offsets (so that a point changes its lane, tile, tile pair and workgroup)"""
    cn = _pair(2, 4, 48)[True]
    d = _dev(E.point_inputs(N, cn.d_feature, cn.n_a, seed=42))
    whole = _rows(cn, d, 0, N)
    lo = 0
    for m in LAUNCHES:
        if lo + m > N:
            lo = (lo + m) % (N - m)
        part = _rows(cn, d, lo, m)
        assert set(part) == set(whole)
        for name, t in part.items():
            assert torch.equal(t, whole[name][lo:lo + m]), (name, lo, m)
        lo += m


@gpu
@pytest.mark.parametrize("ray_bias", [True, False])
def test_render_form_and_what_each_form_writes(ray_bias):
    from neuralrecon_w_amd.neuconw import points_struct
    from neuralrecon_w_amd.stash import StashCache

    cn = _pair(2, 4, 48, ray_bias)[True]
    W, n = cn.d_feature, N
    d = _dev(E.point_inputs(n, W, cn.n_a, seed=42))
    far, fid = _feat_arena(n, W, d["feat"])
    pts = points_struct(x=d["x"], rays_d=d["dirs"])
    rgb = {}
    for train in (True, False):
        # the arena of this (n, form) is cached by the module: lease it once, fill it, lease it again
        with torch.set_grad_enabled(train):
            _, ctx = cn.fwd_stash(pts, n, _prec(), d["normals"], d["a"], far.ptr(fid), train=train)
        torch.cuda.synchronize()
        ar = ctx["arena"]
        StashCache.release(ctx["lease"])
        ar.buf.fill_(0xFF)  # every 16-bit word a NaN
        with torch.set_grad_enabled(train):
            out, ctx2 = cn.fwd_stash(pts, n, _prec(), d["normals"], d["a"], far.ptr(fid), train=train)
        torch.cuda.synchronize()
        assert ctx2["arena"] is ar and ctx2["plan"].net.act_split == 1
        rgb[train] = out.clone()
        untouched = torch.ones(ar.buf.numel(), dtype=torch.bool, device="cuda")
        if train:
            for name, i in _field_ids(ctx2["ids"]):
                off, rb = ar._off[i]
                nb = _covered_tiles(n) * rb * 2048
                field = ar.buf[off:off + nb].view(torch.float16)
                assert not bool(torch.isnan(field).any()), name  # fully written (the inputs are finite)
                untouched[off:off + nb] = False
        assert bool((ar.buf[untouched] == 0xFF).all())
        StashCache.release(ctx2["lease"])
    assert bool(torch.isfinite(rgb[True]).all()) and float(rgb[True].abs().max()) > 0
    assert torch.equal(rgb[False], rgb[True])
