"""composite_bwd_kernel with a cotangent for `normals` (NcwCompositeGrad.d_normals: the floor-normal loss), called directly through
rayops.CompositeCtx at both LDS capacities.

Reference: oracle/neuconw_oracle.py `composite` with autograd, the loss of tests/_ray_cases.comp_reference_on plus
(normals * d_normals).sum() with a seeded d_normals (tests/_floor_ref.py), in float64 -- which arbitrates -- and in float32 on the CPU
(the fp32 restatement).  Bound: the per-ray kernels' own rule, err <= max(FLOOR_ADJ, 4 * err_fp32_restatement), both errors against
float64 (tests/_ray_cases.bound).  The guard-band conditions of the reused cases are asserted by tests/test_ray_cases_host.py.
Every comparison prints its (kernel, restatement) pair (run with -s)."""
import pytest
import torch

from tests import _floor_ref as F
from tests import _ray_cases as C
from tests._util import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(1, 0), (1, 1), (65, 0), (61, 4), (512, 0), (509, 4), (1056, 32)]
OPTION_SHAPES = [(61, 4), (509, 4)]  # one per capacity


def _shape_cases():
    return [C.comp_case(S, O_) for S, O_ in SHAPES] + [C.comp_case(64, 0, with_bg=False)]


def _option_cases():
    cs = []
    for S, O_ in OPTION_SHAPES:
        cs += [C.comp_case(S, O_, trim=False), C.comp_case(S, O_, brgb=False), C.comp_case(S, O_, values=True),
               C.comp_case(S, O_, cot="no_depth_eik")]
    return cs


def _cu(t):
    return t.cuda() if t is not None else None


def _run_bwd(c, d_normals, only_normals=False, **kw):
    """The compositor backward on the case's inputs -> adjoints on the CPU under the reference's names (inv_s summed over rays)."""
    from neuralrecon_w_amd import rayops

    I = C.comp_case_inputs(c)
    ctx = rayops.CompositeCtx(*(_cu(I[k]) for k in ("o", "d", "z", "sample_dist", "sdf", "grad", "rgb", "inv_s")), c.cos,
                              _cu(I["z_feed"]), _cu(I["density"]), _cu(I["bg_rgb"]), background_rgb=_cu(I["background_rgb"]),
                              trim_sphere=c.trim)
    ct = I["cot"]
    ups = [None] * 4 if only_normals else [_cu(ct[k]) for k in ("d_color", "d_weights_sum", "d_depth", "d_eik_num")]
    got = ctx.backward(*ups, d_normals=_cu(d_normals), **kw)
    adj = {k[2:]: v.cpu() for k, v in got.items() if v is not None}
    adj["inv_s"] = adj["inv_s"].sum().reshape(1)  # per-ray terms: the caller reduces them
    torch.cuda.synchronize()
    return adj


def _compare(c, adj, a64, a32, keys=None):
    assert set(adj) == set(a64)
    bad, line = [], []
    for k in (keys or a64):
        assert bool(torch.isfinite(adj[k]).all()), k
        e, e32 = rel_err(adj[k].reshape(a64[k].shape), a64[k]), rel_err(a32[k], a64[k])
        line.append("%s %.1e/%.1e" % (k, e, e32))
        if not e <= C.bound(C.FLOOR_ADJ, e32):
            bad.append((k, e, e32))
    print("\n%s [%s]: kernel/fp32: %s" % (C.case_id(c), "large-ray" if c.S + c.O > 512 else "standard", " ".join(line)))
    assert not bad, bad


@pytest.mark.parametrize("c", _shape_cases(), ids=C.case_id)
def test_d_normals_shapes(c):
    """Every adjoint with all five cotangents, R = 5 (one full workgroup and one wave): S below, at and past a multiple of 64, both
    capacities on both sides of 512, a ragged last lane chunk, S = 1, and no background."""
    _compare(c, _run_bwd(c, F.d_normals_of(c)), *F.comp_reference_normals(c))


@pytest.mark.parametrize("c", _option_cases(), ids=C.case_id)
def test_d_normals_options(c):
    """trim_sphere off, no background colour, the value switches (a ray that misses the sphere: its normal's adjoint leaves through
    d_density alone; a grad = 0 column; densities beyond +-20), and d_depth / d_eik_num = None."""
    _compare(c, _run_bwd(c, F.d_normals_of(c)), *F.comp_reference_normals(c))


@pytest.mark.parametrize("S,O_", OPTION_SHAPES)
def test_only_d_normals(S, O_):
    """d_normals alone, every other cotangent zero: a missing or wrong term cannot hide behind the others.  grad gets both the
    direct term w dn and the one through alpha; sdf, density and inv_s only the latter; rgb and bg_rgb get nothing."""
    c = C.comp_case(S, O_)
    a64, a32 = F.comp_reference_normals(c, only_normals=True)
    adj = _run_bwd(c, F.d_normals_of(c), only_normals=True)
    for k in ("grad", "sdf", "density", "inv_s"):
        assert float(a64[k].abs().max()) > 0, k
    _compare(c, adj, a64, a32, keys=("grad", "sdf", "density", "inv_s"))
    assert not adj["rgb"].any() and not adj["bg_rgb"].any()


@pytest.mark.parametrize("S,O_", OPTION_SHAPES)
def test_zero_d_normals_equals_none(S, O_):
    """d_normals = zeros runs the other instantiation of the kernel and gives the adjoints of d_normals = None."""
    c = C.comp_case(S, O_)
    a0 = _run_bwd(c, None)
    az = _run_bwd(c, torch.zeros(c.R, 3))
    for k in a0:
        assert torch.equal(a0[k], az[k]), k


@pytest.mark.parametrize("S,O_", OPTION_SHAPES)
def test_d_normals_under_the_loss_scale(S, O_):
    """grad_scale = 8 with grad_scale_dev = [0.5]: d_normals is multiplied on load like the other cotangents -- held to the references
    with every cotangent times 4."""
    c = C.comp_case(S, O_)
    adj = _run_bwd(c, F.d_normals_of(c), grad_scale=8.0, grad_scale_dev=torch.tensor([0.5], device="cuda"))
    _compare(c, adj, *F.comp_reference_normals(c, scale=4.0))
