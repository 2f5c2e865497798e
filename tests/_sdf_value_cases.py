"""CPU side of tests/test_gpu_sdf_value_edges.py and tests/test_sdf_value_host.py: which kernel `sdf_infer_any` (csrc/ncw_sdf.hip)
launches for a width, a precision and a depth, the networks and point sources the value-only kernels are pinned at, and the rounding
floor of the sdf value.  The network recipe, points, rays and the fp64 statement are those of tests/_sdf_bwd_ref.py; `case()` adds
non-zero biases.

The ROUNDING FLOOR of the sdf value (`floor()`) is the error against the fp64 statement of the same statement with every rounding a
16-bit value chain cannot avoid made once (tests/_sdf_bwd_ref.py lists them; of those only the forward's enter `sdf`: the matrices,
gamma and h_l), or, for the exact-fp32 and the split-precision kernels, of the statement evaluated by torch in fp32."""
import torch

from tests import _sdf_bwd_ref as R
from tests._util import rel_err

# (n_layers, skip_in[, scale]) of SDFNetwork; the kernels' L = n_layers + 1.  tests/test_gpu_sdf_value_edges.py says per entry what
# the value-only kernels do differently
NETS = [(nl, sk) for nl, sk in R.NETS] + [(9, (4,)), (8, (4,), 1.7)]
WIDTHS = (64, 256, 512)
PRECS = ("f32", "bf16", "f16", "f16-split")
TOL = {"bf16": 3e-2, "f16": 2e-3}  # tests/test_gpu_sdf.py TOL_BF16 / TOL_F16: the project's bounds of the plain 16-bit value chains
TOL_EXACT = 5e-6                   # tests/test_gpu_sdf.py test_split_precision_value_path: the split chain (and the exact-fp32 kernels)

# (W, precision name, SDFNetwork.sdf_split): `f16` switches the split value chain off, `f16-split` leaves the default (on at
# W = 256 / 512 for n_layers >= 2: SDFNetwork.split_value).  At W = 64 the default IS the plain chain (same plan, same kernel), so
# the width has no `f16-split` route.
ROUTES = [(W, p, False if p == "f16" else None) for W in WIDTHS for p in PRECS if not (W == 64 and p == "f16-split")]

# the rows of sdf_infer_any: (widths, precision names, n_layers from, to (inclusive), kernel)
KERNELS = [
    ((64,), PRECS, 1, 11, "sdf_infer_kernel<., 2>"),
    ((256,), ("f32",), 1, 11, "sdf_infer_kernel<PrecF32, 8>"),
    ((512,), ("f32",), 1, 1, "sdf_infer_kernel<PrecF32, 16>"),   # sdf16f_on needs L >= 3
    ((256,), ("bf16", "f16"), 2, 11, "sdf_inferC_kernel"),
    ((256, 512), ("bf16", "f16", "f16-split"), 1, 1, "sdf_infer_kernel<PrecBF16, 8 / 16>"),
    ((256,), ("f16-split",), 2, 8, "sdf_inferS2_kernel"),
    ((256,), ("f16-split",), 9, 11, "sdf_inferS_kernel"),
    ((512,), ("f32",), 2, 11, "sdf_infer16f_kernel"),
    ((512,), ("bf16", "f16"), 2, 11, "sdf_infer16_kernel<T>"),
    ((512,), ("f16-split",), 2, 11, "sdf_inferS16_kernel"),
]


def net_id(net):
    nl, sk = net[:2]
    return "n%ds%s" % (nl, sk[0] if sk else "x") + ("-scale%g" % net[2] if len(net) > 2 else "")


def route_id(route):
    return "W%d-%s" % route[:2]


def kernels(W, prec_name, n_layers):
    """every row of KERNELS that claims the case (the host test: exactly one)"""
    return [k for ws, ps, lo, hi, k in KERNELS if W in ws and prec_name in ps and lo <= n_layers <= hi]


def route_plan(route, n_layers):
    """what the packed plan of a route must look like, and the precision its accuracy is held to:
    -> dict(kernel, rb = plan.net.rb, w_lo = whether plan.net.w_lo[0] is set, bound = the precision name whose bound applies).
    `f16-split` at n_layers = 1 falls back to the plain chain (SDFNetwork.split_value needs n_lin >= 3; sdf_split_on L >= 3):
    no residual matrices, the plain fp16 bound."""
    W, p, _ = route
    k, = kernels(W, p, n_layers)
    split = p == "f16-split" and W in (256, 512) and n_layers >= 2
    return dict(kernel=k, rb=W // 32, w_lo=split, bound="f16" if p == "f16-split" and not split else p)


def lib_prec(prec_name):
    from neuralrecon_w_amd import lib as L

    return {"f32": L.PREC_F32, "bf16": L.PREC_BF16, "f16": L.PREC_F16, "f16-split": L.PREC_F16}[prec_name]


def lattice(gdim=9):
    """a mode-3 lattice (NcwPoints gmin / gmax / gdim / gorigin / gradius) whose points are exact in fp32: step 0.25, origin on the
    lattice, radius a power of two -> (keywords of grid.sdf_grid_range, fn(dtype) -> the expected points [gdim^3, 3], x slowest)"""
    kw = dict(dim=gdim, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), origin=(0.25, -0.5, 0.0), radius=2.0)

    def expected(dtype):
        ax = [torch.linspace(kw["bound_min"][a], kw["bound_max"][a], gdim, dtype=dtype) for a in range(3)]
        p = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
        return (p - torch.tensor(kw["origin"], dtype=dtype)) / kw["radius"]

    return kw, expected


_CASES = {}


def case(W, net, n=R.N_ORACLE):
    """as _sdf_bwd_ref.case -- its network recipe, its points -- with the biases of the Softplus layers made non-zero: the geometric
    initialisation leaves them all at 0, and a kernel that staged or read the bias of another layer (PP_BIAS / S2_BIAS slots,
    `read_bias(l)`, `bias_of(l)`) would compute the same values"""
    k = (W,) + tuple(net) + (n,)
    c = _CASES.get(k)
    if c is None:
        nl, sk = net[:2]
        scale = net[2] if len(net) > 2 else 1.0
        m = R.make_net(W, nl, sk, scale)
        g = torch.Generator().manual_seed(34)
        with torch.no_grad():
            for l in range(nl):
                b = getattr(m, "lin%d" % l).bias
                b.add_(0.05 * torch.randn(b.shape, generator=g))
        x = R.points(n, seed=9, radius=0.9) if n == R.N_ORACLE else R.points(n)
        c = _CASES[k] = dict(W=W, net=m, sd=R.state_dict64(m), skip=tuple(sk), scale=scale, x=x)
    return c


def exact_sdf(c):
    """the unrounded fp64 statement's sdf of a case, computed once per process"""
    v = c.setdefault("value", {})
    if "exact" not in v:
        v["exact"] = _sdf(c)
    return v["exact"]


def _sdf(c, **kw):
    n = c["x"].shape[0]
    zero = dict(d_sdf=torch.zeros(n), d_grad=torch.zeros(n, 3), d_feat=torch.zeros(n, c["W"]))  # the cotangents do not enter sdf
    return R.statement(c["sd"], c["skip"], c["scale"], c["x"], zero, **kw)["sdf"]


def floor(c, prec_name):
    """rounding floor of the sdf value: rel_err against the fp64 statement of the rounded-once statement (bf16 / f16) or of the
    statement in torch's fp32 (f32 / f16-split); cached on the case"""
    v = c.setdefault("value", {})
    k = "f32" if prec_name in ("f32", "f16-split") else prec_name
    if k not in v:
        kw = dict(dtype=torch.float32) if k == "f32" else dict(dt=R.DTYPE[k])
        v[k] = rel_err(_sdf(c, **kw), exact_sdf(c))
    return v[k]


def bound(c, route, n_layers):
    """the bound of part d of the GPU file -- none comes from the kernels: plain 16-bit chains 2 x floor, never looser than the project's
    tolerance so far; the exact-fp32 and split-precision kernels 5e-6 -> (bound, floor)"""
    b = route_plan(route, n_layers)["bound"]
    fl = floor(c, b)
    return (min(2 * fl, TOL[b]) if b in TOL else TOL_EXACT), fl
