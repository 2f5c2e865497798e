"""CPU side of tests/test_gpu_color_edges.py: colour networks of any supported depth, their inputs, the fp64 oracle's outputs and
gradients (computed once per configuration and shared), and the ROUNDING FLOOR of a 16-bit evaluation -- the oracle's network in
fp64 with the weight and the input of every Linear rounded once to the 16-bit type (straight-through for the gradients:
the backward sees the rounded weights and inputs and the ReLU masks of the rounded forward, which is what moves the adjoints).
Its errors against the unrounded oracle are what a correct 16-bit kernel cannot be expected to beat by much."""
import copy

import torch
import torch.nn.functional as F

from tests._util import rel_err
from tests.test_gpu_color_nerf import _jitter, flipped_points, fro_err

KEYS = {"K0": (64, 32, 64), "K1": (64, 128, 256), "K2": (256, 128, 256), "K3": (512, 128, 256)}
DTYPE = {"f16": torch.float16, "bf16": torch.bfloat16}


def make_net(key, n_head=2, n_layers=4, n_a=48, seed=31):
    """RenderingNetwork on the CPU (move a deepcopy to the GPU), biases and weight-norm gains jittered away from their init."""
    import neuralrecon_w_amd as nw

    W, head, hidden = KEYS[key]
    torch.manual_seed(seed)
    cn = nw.RenderingNetwork(d_feature=W, mode="idr", d_in=9, d_out=3, d_hidden=hidden, n_layers=n_layers, head_channels=head,
                             in_channels_dir_a=n_a, static_head_layers=n_head, weight_norm=True, multires_view=4)
    _jitter(cn, seed + 1)
    return cn


def state_dict64(cn, grad=True):
    return {"color_net." + k: v.detach().cpu().double().requires_grad_(grad) for k, v in cn.state_dict().items()}


def _unit(n, g):
    d = torch.randn(n, 3, generator=g)
    return d / d.norm(dim=-1, keepdim=True)


def point_inputs(n, W, n_a, seed):
    """mode 0: every point is its own ray (the inputs of tests/test_gpu_color_nerf.py::test_color_net_train_vs_oracle)"""
    g = torch.Generator().manual_seed(seed)
    return dict(x=(torch.rand(n, 3, generator=g) * 2 - 1) * 0.9, normals=torch.randn(n, 3, generator=g), dirs=_unit(n, g),
                feat=0.5 * torch.randn(n, W, generator=g), a=torch.randn(n, n_a, generator=g), w_rgb=torch.randn(n, 3, generator=g))


def ray_inputs(R, S, W, n_a, seed):
    """modes 1 / 2: rays (origin, direction, appearance row), S increasing depths per ray and the last sample's distance"""
    g = torch.Generator().manual_seed(seed)
    n = R * S
    return dict(rays_o=(torch.rand(R, 3, generator=g) * 2 - 1) * 0.3, dirs=_unit(R, g),
                z=0.1 + torch.cumsum(torch.rand(R, S, generator=g) * 0.04 + 0.005, dim=1),
                sample_dist=torch.rand(R, generator=g) * 0.04 + 0.005, normals=torch.randn(n, 3, generator=g),
                feat=0.5 * torch.randn(n, W, generator=g), a=torch.randn(R, n_a, generator=g), w_rgb=torch.randn(n, 3, generator=g))


def ray_points64(inp, mode):
    """the points csrc/ncw_mlp.h load_point evaluates, formed in fp64 from the fp32 inputs: mode 1 o + d z; mode 2 o + d (z_i + dist_i / 2)
    with dist_i = z_{i+1} - z_i and sample_dist for the last sample"""
    z = inp["z"].double()
    if mode == 2:
        dist = torch.cat([z[:, 1:] - z[:, :-1], inp["sample_dist"].double()[:, None]], 1)
        z = z + 0.5 * dist
    x = inp["rays_o"].double()[:, None, :] + inp["dirs"].double()[:, None, :] * z[..., None]
    return x.reshape(-1, 3)


def _ste(t, dt):
    """t rounded once to dt, identity for the gradient"""
    return t if dt is None else t + (t.detach().to(dt).double() - t.detach())


def color_net(sd, points, normals, view_dirs, feat, a, dt=None):
    """oracle.neuconw_oracle.color_net; dt: every Linear's weight and input rounded once to that type, fp64 accumulation"""
    from oracle import neuconw_oracle as O

    def lin(x, name):
        if name + ".weight_g" in sd:
            w = O.weight_norm_eff(sd[name + ".weight_g"], sd[name + ".weight_v"])
        else:
            w = sd[name + ".weight"]
        return F.linear(_ste(x, dt), _ste(w, dt), sd[name + ".bias"])

    p = "color_net."
    e = torch.cat([lin(feat, p + "xyz_encoding_final"), O.freq_encode(view_dirs, 4), a], 1)
    i = 0
    while (p + "static_encoding.static_linear_%d.weight" % i) in sd:
        e = F.relu(lin(e, p + "static_encoding.static_linear_%d" % i))
        i += 1
    h = torch.cat([points, normals, e], -1)
    n_lin = 0
    while (p + "lin%d.bias" % n_lin) in sd:
        n_lin += 1
    for l in range(n_lin):
        h = lin(h, p + "lin%d" % l)
        if l < n_lin - 1:
            h = F.relu(h)
    return torch.sigmoid(h)


def evaluate(cn, inp, x64=None, S=1, dt=None, dtype=torch.float64):
    """rgb, the adjoints of (normals, feat, a) and every parameter gradient under sum(rgb * w_rgb).  x64 / S: ray-indexed inputs
    (dirs and a are per ray, repeated over the S samples inside the graph, so the a-adjoint is the per-ray sum).
    dtype float32: the same network evaluated by torch in fp32 (the flipped-rows check)."""
    sd = {k: v.to(dtype).detach().requires_grad_(True) for k, v in state_dict64(cn, grad=False).items()}
    x = (inp["x"].double() if x64 is None else x64).to(dtype)
    ins = [inp[k].to(dtype).requires_grad_(True) for k in ("normals", "feat", "a")]
    dirs, a = inp["dirs"].to(dtype), ins[2]
    if S > 1:
        dirs, a = dirs.repeat_interleave(S, 0), a.repeat_interleave(S, 0)
    if dtype == torch.float64:
        rgb = color_net(sd, x, ins[0], dirs, ins[1], a, dt)
    else:
        from oracle import neuconw_oracle as O

        rgb = O.color_net(sd, x, ins[0], dirs, ins[1], a)
    names = list(sd)
    gr = torch.autograd.grad((rgb * inp["w_rgb"].to(dtype)).sum(), [sd[k] for k in names] + ins)
    return dict(rgb=rgb.detach(), grads={k[len("color_net."):]: v for k, v in zip(names, gr[:len(names)])},
                adj=dict(zip(("normals", "feat", "a"), gr[len(names):])))


def errors(got, ref):
    """(max-norm relative error of rgb, worst L2 error of the three input adjoints, worst L2 error of a parameter gradient)"""
    return (rel_err(got["rgb"], ref["rgb"]), max(fro_err(got["adj"][k], ref["adj"][k]) for k in ref["adj"]),
            max(fro_err(got["grads"][k], ref["grads"][k]) for k in ref["grads"]))


_CASES = {}


def case(key, n_head, n_layers, n_a, n=None, rays=None, mode=0, seed=31):
    """One configuration, computed once per process: the network (CPU), its inputs, the fp64 reference and, on demand
    (`floor(c, prec)`), the 16-bit rounding floors.  rays = (R, S) with mode 1 / 2, or n points with mode 0."""
    k = (key, n_head, n_layers, n_a, n, rays, mode, seed)
    c = _CASES.get(k)
    if c is None:
        cn = make_net(key, n_head, n_layers, n_a, seed)
        W = KEYS[key][0]
        if rays is None:
            inp, x64, S = point_inputs(n, W, n_a, seed + 2), None, 1
        else:
            inp = ray_inputs(rays[0], rays[1], W, n_a, seed + 2)
            x64, S = ray_points64(inp, mode), rays[1]
        c = _CASES[k] = dict(cn=cn, inp=inp, x64=x64, S=S, ref=evaluate(cn, inp, x64, S), floors={})
    return c


def gpu_net(c):
    return copy.deepcopy(c["cn"]).cuda()


def floor(c, prec_name):
    """(out, adj, grad) errors of the rounded-once fp64 emulation against the unrounded oracle"""
    if prec_name not in c["floors"]:
        c["floors"][prec_name] = errors(evaluate(c["cn"], c["inp"], c["x64"], c["S"], dt=DTYPE[prec_name]), c["ref"])
    return c["floors"][prec_name]


def flipped_rows_fp32(c):
    """rows of the three per-point adjoints where torch's own fp32 evaluation leaves the fp64 oracle by more than 1e-4 of the
    tensor's max (tests/test_gpu_color_nerf.py flipped_points): ReLU masks that flip in fp32"""
    got = evaluate(c["cn"], c["inp"], c["x64"], c["S"], dtype=torch.float32)
    ks = ("normals", "feat") if c["S"] > 1 else ("normals", "feat", "a")  # (per-ray a-adjoints are sums: no row of a point)
    return max(flipped_points(got["adj"][k], c["ref"]["adj"][k]) for k in ks)
