"""CPU: the reference of tests/test_gpu_sdf_bwd_edges.py checks itself.  tests/_sdf_bwd_ref.py restates oracle.neuconw_oracle.sdf_net
with a perturbation at every quantity the SDF backward stashes; here its outputs are the oracle's outputs and its per-point
products, chained through weight-norm, are autograd's parameter gradients of the oracle (1e-10; measured <= 2e-14), every compared
field is non-zero, the split cotangent sets separate the first- from the second-order part exactly, the dyadic rays of the
ray-indexed cases generate their points without a rounding, and SDFNetwork refuses more Linears than the kernels' struct arrays hold."""
import pytest
import torch

from tests import _sdf_bwd_ref as R
from tests._util import rel_err

W = 64
N = 131  # four tiles and three points; the identities hold per point


def _small(n_layers, skip, scale=1.0):
    return R.case(W, n_layers, skip, n=N, scale=scale)


@pytest.mark.parametrize("n_layers,skip,scale", [(nl, sk, 1.0) for nl, sk in R.NETS] + [(8, (4,), 1.7), (2, (1,), 0.6)])
@pytest.mark.parametrize("cot", R.COTS)
def test_statement_is_the_oracle(n_layers, skip, scale, cot):
    c = _small(n_layers, skip, scale)
    r = R.ref(c, cot)
    f = r["f"]
    assert f["L"] == n_layers + 1
    for k in ("sdf", "feat", "grad"):
        assert rel_err(f[k], r["outs"][k]) < 1e-10, (k, rel_err(f[k], r["outs"][k]))
    got = R.param_grads(c["sd"], c["skip"], f)
    assert set(got) == set(r["grads"]) and len(got) == 3 * (n_layers + 1)
    for k, g in r["grads"].items():
        zero = cot == "second" and k == "sdf_net.lin%d.bias" % n_layers   # d_sdf = 0, d_feat = 0: nothing reaches the last bias
        assert got[k].shape == g.shape and (float(g.abs().max()) > 0) != zero, k
        assert R.err(got[k], g) < 1e-10, (k, R.err(got[k], g))
    assert torch.equal(f["zsdf"], c["cots"][cot]["d_sdf"].double() / scale)


@pytest.mark.parametrize("n_layers,skip", R.NETS)
def test_fields_are_nonzero_and_the_cotangent_sets_split_the_orders(n_layers, skip):
    c = _small(n_layers, skip)
    L = n_layers + 1
    both, first, second = (R.ref(c, k)["fields"] for k in ("both", "first", "second"))
    assert set(both) == {"zsdf", "qbar0"} | {"zbar%d" % l for l in range(L - 1)} | {"qbar%d" % l for l in range(1, L)}
    for k, v in both.items():
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, k
    for k in both:
        if k.startswith("qbar"):
            assert float(first[k].abs().max()) == 0 and float(second[k].abs().max()) > 0, k   # no d_grad: nothing enters the sweep
        elif k == "zsdf":
            assert float(second[k].abs().max()) == 0 and torch.equal(first[k], both[k])
        else:
            assert float(first[k].abs().max()) > 0 and float(second[k].abs().max()) > 0, k
        # the backward is linear in its cotangents: the parts add up
        assert rel_err(first[k] + second[k], both[k]) < 1e-10, k
    if skip:  # the W - 39 outputs in front of the skip layer: padded columns are zeros
        assert float(both["zbar%d" % (skip[0] - 1)][:, W - R.E:].abs().max()) == 0
        assert float(both["qbar%d" % skip[0]][:, W - R.E:].abs().max()) == 0


@pytest.mark.parametrize("prec_name", R.PRECS)
def test_floors_are_small_and_ordered(prec_name):
    """the emulation rounds and does nothing else: its error has the size of the format's rounding (fp32 < f16 < bf16)"""
    c = _small(8, (4,))
    fl, gr = R.floors(c, "both", prec_name)
    worst = max(max(fl.values()), max(gr.values()))
    lo, hi = {"f32": (0.0, 1e-4), "f16": (1e-5, 0.05), "bf16": (1e-4, 0.4)}[prec_name]
    assert lo < worst < hi, worst
    assert fl["zsdf"] <= {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}[prec_name]


@pytest.mark.parametrize("R_,S", R.RAY_SHAPES)
@pytest.mark.parametrize("mode", [1, 2])
def test_dyadic_rays_generate_their_points_exactly(R_, S, mode):
    inp = R.dyadic_rays(R_, S)
    for v in inp.values():
        assert torch.equal(v * 64, (v * 64).round())
    assert bool((inp["z"][:, 1:] > inp["z"][:, :-1]).all())
    x32, x64 = R.ray_points(inp, mode, torch.float32), R.ray_points(inp, mode, torch.float64)
    assert x32.dtype == torch.float32 and x32.shape == (R_ * S, 3)
    assert torch.equal(x32.double(), x64)
    assert float(x64.abs().max()) < 1.2 and float(x64.abs().max()) > 0.3


def test_constructor_refuses_more_linears_than_the_kernels_hold():
    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import lib as L

    net = nw.SDFNetwork(d_in=3, d_out=65, d_hidden=64, n_layers=11, skip_in=(10,))
    assert net.n_lin == L.MAX_LAYERS == 12
    with pytest.raises(NotImplementedError):
        nw.SDFNetwork(d_in=3, d_out=65, d_hidden=64, n_layers=12, skip_in=(4,))
    with pytest.raises(NotImplementedError):
        nw.SDFNetwork(d_in=3, d_out=65, d_hidden=64, n_layers=12, skip_in=())
