"""CPU side of tests/test_gpu_sdf_bwd_edges.py and tests/test_sdf_bwd_ref_host.py: the fp64 STATEMENT of what `ncw_sdf_bwd` stores.

`statement()` writes SDFNetwork's forward plus the explicit adjoint sweep of oracle.neuconw_oracle.sdf_net (the analytic input
gradient) in the kernels' convention and adds a zero perturbation at every stashed quantity: e_l to z_l, a_l to q_l = t_l M_l.
ONE first-order torch.autograd.grad of

    loss = (sdf d_sdf).sum() + (grad d_grad).sum() + (feat d_feat).sum()

with respect to the perturbations then yields every per-point field of the second-order backward:

    zbar[l]  l <= L-2   d loss / d e_l                                 qbar[0]  d loss / d a_0 = J_gamma nbar (39 features)
    zsdf                d loss / d e_{L-1}[0] = d_sdf / scale          qbar[l]  l >= 1: d loss / d a_l (at the skip layer its gamma
    one                 1                                                       columns repeat qbar[0]; the kernels store the rest)

Convention (csrc/ncw_sdf.hip): M_l = the weight-normed matrix of Linear l, the skip layer's divided by sqrt 2 and applied to
cat[h, gamma]; xs = x scale; sdf = z_{L-1}[0] / scale; a_{L-1} = e_0, so q_{L-1} = row 0 of M_{L-1}.  `param_grads()` forms the
per-point products the weight-gradient GEMMs form -- sum_p zbar_l (x) in_l + t_l (x) qbar_l, and at the last Linear
zsdf (x) h + one (x) qbar (row 0), dfeat (x) h (rows 1..W) -- and chains them through weight-norm.

The ROUNDING FLOOR of a 16-bit backward (`floors()`; in the manner of tests/_color_emul.py) is the error, per field, of the SAME
statement in fp64 with every rounding a 16-bit kernel cannot avoid, each made once:
  * every matrix M_l (the packed `w` and `wt` hold the same rounded values); biases stay fp32;
  * the operands of the forward's products: gamma, h_l (the stash holds the same bits), and t_l of the adjoint sweep;
  * phi'(z_l) = 1 - exp(-100 h_{l+1}) from the ROUNDED h (load_sprime_block);
  * the operands of the backward's products: qbar_0, abar_l = qbar_{l+1}, zbar_l before the next `wt` product, dfeat and the d_sdf
    block (the stashes hold the same bits);
  * the parked zbar2_l: stash_store_block_keep converts to the stash's 16-bit element like every other store, so the second-order
    term is rounded once on its own before pass 2 adds u phi' to it (here: the cotangent entering phi' is rounded).
Backward-side roundings are expressed by `_Round`, which rounds its input forward and / or its cotangent backward.  Everything
else -- accumulation, Softplus, the products of the epilogues -- stays fp64.  The fp32 floor is the unrounded statement evaluated
by torch in float32."""
import copy
import math

import torch

from oracle import neuconw_oracle as O
from tests._util import rel_err

E = 39  # width of gamma: 3 + 3 * 2 * 6
DTYPE = {"f16": torch.float16, "bf16": torch.bfloat16}
PRECS = ("f32", "bf16", "f16")
COTS = ("first", "second", "both")
# (n_layers, skip_in) of SDFNetwork; the kernels' L = n_layers + 1
NETS = [(8, (4,)), (1, ()), (2, (1,)), (3, (1,)), (3, ()), (11, (10,))]
N_EDGE = 419     # tests/test_gpu_sdf_fwd_edges.py: 13 tiles + 3 points
N_ORACLE = 777   # tests/test_gpu_sdf_train.py: the size class the project's tolerances were measured at
RAY_SHAPES = [(13, 5), (7, 32), (5, 40)]


class _Round(torch.autograd.Function):
    """v rounded once to `dt` in the forward (fwd) and / or its cotangent rounded once in the backward (bwd)"""

    @staticmethod
    def forward(ctx, v, dt, fwd, bwd):
        ctx.dt, ctx.bwd = dt, bwd
        return v.to(dt).to(v.dtype) if fwd else v.clone()

    @staticmethod
    def backward(ctx, g):
        return (g.to(ctx.dt).to(g.dtype) if ctx.bwd else g), None, None, None


def _r(v, dt, fwd=False, bwd=False):
    return v if dt is None else _Round.apply(v, dt, fwd, bwd)


# ---- networks, points, cotangents ------------------------------------------------------------------------------------------------
def make_net(W, n_layers, skip, scale=1.0, seed=31):
    """the `_net` recipe of tests/test_gpu_sdf_fwd_edges.py at any width, on the CPU (move a deepcopy to the GPU)"""
    import neuralrecon_w_amd as nw

    torch.manual_seed(seed)
    net = nw.SDFNetwork(d_in=3, d_out=W + 1, d_hidden=W, n_layers=n_layers, skip_in=skip, scale=scale)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("weight_g"):
                p.mul_(1.0 + 0.1 * torch.randn_like(p))
            if n.endswith("weight_v") and not n.startswith("lin%d" % (net.n_lin - 1)):
                p.add_(0.02 * torch.randn_like(p))  # make the encoding / skip columns non-zero
    return net


def state_dict64(net):
    return {"sdf_net." + k: v.detach().cpu().double() for k, v in net.state_dict().items()}


def points(n, seed=32, radius=1.2):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 3, generator=g) * 2 - 1) * radius


def cotangents(n, W, seed=9):
    """`both`: the recipe of tests/test_gpu_sdf_train.py; `first`: d_grad = 0 (what remains is the first-order backward);
    `second`: d_sdf = 0 and d_feat = 0 (the backward of the adjoint sweep alone)"""
    g = torch.Generator().manual_seed(seed)
    both = dict(d_sdf=torch.randn(n, generator=g), d_grad=torch.randn(n, 3, generator=g), d_feat=torch.randn(n, W, generator=g) * 0.1)
    first = dict(both, d_grad=torch.zeros(n, 3))
    second = dict(both, d_sdf=torch.zeros(n), d_feat=torch.zeros(n, W))
    return dict(first=first, second=second, both=both)


def dyadic_rays(R, S, seed=33):
    """rays whose points are exact in fp32: o, d, z and sample_dist are multiples of 2^-6 (|o| <= 0.3, |d| <= 0.5, z <= 1.4), so
    d z and d (z + dist / 2) are multiples of 2^-13 below 1 and the sums with o fit 24 bits"""
    g = torch.Generator().manual_seed(seed)

    def q(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float() / 64.0

    z = 6.0 / 64.0 + torch.cumsum(q(1, 2, R, S), dim=1)
    return dict(rays_o=q(-19, 19, R, 3), rays_d=q(-32, 32, R, 3), z=z, sample_dist=q(1, 2, R))


def ray_points(inp, mode, dtype):
    """the points csrc/ncw_mlp.h load_point forms (mode 1: o + d z; mode 2: o + d (z_i + dist_i / 2), dist_i = z_{i+1} - z_i and
    sample_dist for a ray's last sample), in its order of operations, evaluated in `dtype`"""
    o, d, z = inp["rays_o"].to(dtype), inp["rays_d"].to(dtype), inp["z"].to(dtype)
    if mode == 2:
        dist = torch.cat([z[:, 1:] - z[:, :-1], inp["sample_dist"].to(dtype)[:, None]], 1)
        z = z + dist * 0.5
    return (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3)


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def kernel_matrices(sd, skip, prefix="sdf_net."):
    """[(M_l, b_l)] from a state dict: M_l = weight_norm_eff(g, v), divided by sqrt 2 at the skip layer"""
    mats = []
    for l in range(O._count_layers(sd, prefix)):
        w, b = O._lin_eff(sd, prefix + "lin%d" % l)
        mats.append((w / math.sqrt(2.0) if l in skip else w, b))
    return mats


def statement(sd, skip, scale, x, cot, dt=None, dtype=torch.float64):
    """-> dict of per-point fields (module docstring).  dt: a 16-bit torch dtype = the rounded-once emulation; dtype float32 (dt None):
    the unrounded statement in torch's fp32."""
    skip_l = skip[0] if skip else -1
    mats = [(m.detach().to(dtype), b.detach().to(dtype)) for m, b in kernel_matrices(sd, skip)]
    if dt is not None:
        mats = [(m.to(dt).to(dtype), b) for m, b in mats]
    L, n = len(mats), x.shape[0]
    xs = x.to(dtype) * scale
    gamma = _r(O.freq_encode(xs, 6), dt, fwd=True)
    e = [torch.zeros(n, m.shape[0], dtype=dtype, requires_grad=True) for m, _ in mats]
    a = [torch.zeros(n, m.shape[1], dtype=dtype, requires_grad=True) for m, _ in mats]
    # ---- forward: z_l = M_l in_l + b_l (+ e_l), h_{l+1} = Softplus(z_l)
    ins, h, s = [], {}, []
    inp = gamma
    for l, (m, b) in enumerate(mats):
        if l == skip_l:
            inp = torch.cat([inp, gamma], 1)
        ins.append(inp)
        z = _r(inp @ m.t() + b + e[l], dt, bwd=True)       # zbar_l (at L-1: the d_sdf block and dfeat) as a 16-bit operand
        if l < L - 1:
            inp = h[l + 1] = _r(O.softplus100(z), dt, fwd=True)
            # phi'(z_l): exact, or recomputed from the rounded h with the second-order cotangent (zbar2_l) parked in 16 bits
            s.append(O.softplus100_d1(z) if dt is None else 1.0 - torch.exp(-100.0 * _r(inp, dt, bwd=True)))
    sdf, feat = z[:, 0] / scale, z[:, 1:]
    # ---- adjoint sweep: a_{L-1} = e_0, t_l = a_l phi'(z_l), q_l = t_l M_l (+ a_l); the gamma columns of q_skip and q_0 add up
    q = mats[L - 1][0][0:1].expand(n, -1) + a[L - 1]
    g_gamma = 0.0
    t = {}
    for l in range(L - 2, -1, -1):
        if l + 1 == skip_l:
            g_gamma, q = g_gamma + q[:, -E:], q[:, :-E]
        t[l] = _r(_r(q, dt, bwd=True) * s[l], dt, fwd=True)  # abar_l = qbar_{l+1} as a 16-bit operand; t_l as one
        q = t[l] @ mats[l][0] + a[l]
    g_gamma = _r(g_gamma + q, dt, bwd=True)                   # qbar_0 as a 16-bit operand
    grad = O.freq_encode_jacobian_t_times(xs, 6, g_gamma)
    loss = (sdf * cot["d_sdf"].to(dtype)).sum() + (grad * cot["d_grad"].to(dtype)).sum() + (feat * cot["d_feat"].to(dtype)).sum()
    gr = torch.autograd.grad(loss, e + a)
    ge, ga = gr[:L], gr[L:]
    det = lambda v: v.detach()  # noqa: E731
    return dict(L=L, skip=skip_l, sdf=det(sdf), grad=det(grad), feat=det(feat), gamma=det(gamma), ins=[det(v) for v in ins],
                h={l: det(v) for l, v in h.items()}, t={l: det(v) for l, v in t.items()},
                zbar={l: ge[l] for l in range(L - 1)}, zsdf=ge[L - 1][:, 0], dfeat=ge[L - 1][:, 1:],
                qbar={l: ga[l] for l in range(L)}, one=torch.ones(n, dtype=dtype))


def matrix_grads(f):
    """[(dM_l, db_l)]: the per-point products of the weight-gradient GEMMs, summed over the points"""
    L = f["L"]
    out = []
    for l in range(L - 1):
        out.append((f["zbar"][l].t() @ f["ins"][l] + f["t"][l].t() @ f["qbar"][l], f["zbar"][l].sum(0)))
    hl = f["ins"][L - 1]
    row0 = f["zsdf"][None, :] @ hl + f["one"][None, :] @ f["qbar"][L - 1]
    out.append((torch.cat([row0, f["dfeat"].t() @ hl], 0), torch.cat([f["zsdf"].sum()[None], f["dfeat"].sum(0)])))
    return out


def param_grads(sd, skip, f, prefix="sdf_net."):
    """matrix_grads chained through the 1 / sqrt 2 of the skip layer and weight-norm (fp64) -> {state-dict key: gradient}"""
    out = {}
    for l, (dm, db) in enumerate(matrix_grads(f)):
        name = prefix + "lin%d" % l
        g = sd[name + ".weight_g"].detach().double().requires_grad_(True)
        v = sd[name + ".weight_v"].detach().double().requires_grad_(True)
        dw = dm.double() / math.sqrt(2.0) if l == f["skip"] else dm.double()
        out[name + ".weight_g"], out[name + ".weight_v"] = torch.autograd.grad((O.weight_norm_eff(g, v) * dw).sum(), [g, v])
        out[name + ".bias"] = db.double()
    return out


def oracle_grads(sd, skip, scale, x, cot):
    """torch.autograd.grad of oracle.neuconw_oracle.sdf_net under the same loss -> (outputs, {key: gradient})"""
    sdg = {k: v.detach().double().requires_grad_(True) for k, v in sd.items()}
    sdf, feat, grad = O.sdf_net(sdg, x.double(), skip_in=skip, scale=scale)
    loss = (sdf * cot["d_sdf"].double()).sum() + (grad * cot["d_grad"].double()).sum() + (feat * cot["d_feat"].double()).sum()
    names = list(sdg)
    return dict(sdf=sdf.detach(), feat=feat.detach(), grad=grad.detach()), dict(zip(names, torch.autograd.grad(loss, [sdg[k] for k in names])))


# ---- the fields as the kernels lay them out ----------------------------------------------------------------------------------------
def _pad(v, width):
    return torch.cat([v, torch.zeros(v.shape[0], width - v.shape[1], dtype=v.dtype)], 1) if v.shape[1] < width else v


def stored_fields(f, W):
    """{name: [n, F] rows} as arena.to_rows reads them: zbar[l] / qbar[l >= 1] W wide (the W - 39 outputs in front of a skip layer
    padded with zeros; of qbar[skip] the h columns, its gamma columns are qbar[0]), qbar[0] 64 wide, zsdf the first of 32"""
    L = f["L"]
    out = {"zsdf": _pad(f["zsdf"][:, None], 32), "qbar0": _pad(f["qbar"][0], 64)}
    for l in range(L - 1):
        out["zbar%d" % l] = _pad(f["zbar"][l], W)
    for l in range(1, L):
        out["qbar%d" % l] = _pad(f["qbar"][l][:, :-E] if l == f["skip"] else f["qbar"][l], W)
    return out


def err(got, want):
    """tests/_util.rel_err; where the reference is identically zero (qbar under `first`; zsdf and the last bias' gradient under
    `second`) the largest magnitude, so that anything but zeros is an error of at least its own size over 1e-12"""
    return rel_err(got, want) if float(want.abs().max()) > 0 else float(got.detach().abs().max()) / 1e-12


def field_errors(got, ref):
    return {k: err(got[k], b) for k, b in ref.items()}


# ---- cases: computed once per process ----------------------------------------------------------------------------------------------
_CASES = {}


def case(W, n_layers, skip, scale=1.0, n=N_ORACLE):
    """network (CPU), points, the three cotangent sets, and per cotangent set the fp64 statement (`ref`), its stored fields and
    oracle.sdf_net's parameter gradients; floors on demand"""
    k = (W, n_layers, tuple(skip), n, scale)
    c = _CASES.get(k)
    if c is None:
        net = make_net(W, n_layers, skip, scale)
        sd = state_dict64(net)
        # the oracle size takes the points of tests/test_gpu_sdf_train.py (inside 0.9), the edge sizes those of the forward file (1.2)
        x = points(n, seed=9, radius=0.9) if n == N_ORACLE else points(n)
        c = _CASES[k] = dict(W=W, net=net, sd=sd, skip=tuple(skip), scale=scale, x=x, cots=cotangents(n, W), ref={}, floors={})
    return c


def ref(c, cot):
    if cot not in c["ref"]:
        f = statement(c["sd"], c["skip"], c["scale"], c["x"], c["cots"][cot])
        outs, grads = oracle_grads(c["sd"], c["skip"], c["scale"], c["x"], c["cots"][cot])
        c["ref"][cot] = dict(f=f, fields=stored_fields(f, c["W"]), outs=outs, grads=grads)
    return c["ref"][cot]


def floors(c, cot, prec_name):
    """(per stored field, per parameter gradient) errors against the exact statement / the oracle's gradients of the 16-bit
    rounded-once emulation (bf16 / f16) or of torch's fp32 evaluation of the statement (f32)"""
    k = (cot, prec_name)
    if k not in c["floors"]:
        r = ref(c, cot)
        kw = dict(dtype=torch.float32) if prec_name == "f32" else dict(dt=DTYPE[prec_name])
        f = statement(c["sd"], c["skip"], c["scale"], c["x"], c["cots"][cot], **kw)
        g = param_grads(c["sd"], c["skip"], f)
        c["floors"][k] = (field_errors(stored_fields(f, c["W"]), r["fields"]), {n: err(g[n], r["grads"][n]) for n in r["grads"]})
    return c["floors"][k]


def gpu_net(c):
    return copy.deepcopy(c["net"]).cuda()
