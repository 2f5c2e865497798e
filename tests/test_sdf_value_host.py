"""CPU: the reference side of tests/test_gpu_sdf_value_edges.py checks itself (tests/_sdf_value_cases.py).  The point sources of its
exact comparisons -- dyadic rays in NcwPoints mode 1 / 2, the mode-3 lattice -- generate their points without a rounding, so a fused
or unfused multiply-add in load_point (csrc/ncw_mlp.h) cannot matter; the fp64 statement's sdf is the oracle's; twice the rounding
floor of the plain 16-bit value chains never exceeds the project's tolerance so far (3e-2 bf16, 2e-3 fp16: the new bounds are the
tighter ones); and the table of kernels names exactly one kernel for every width, precision and depth."""
import pytest
import torch

from tests import _sdf_bwd_ref as R
from tests import _sdf_value_cases as V
from tests._util import rel_err


@pytest.mark.parametrize("R_,S", R.RAY_SHAPES)
@pytest.mark.parametrize("mode", [1, 2])
def test_ray_sources_generate_their_points_exactly(R_, S, mode):
    inp = R.dyadic_rays(R_, S)
    x32, x64 = R.ray_points(inp, mode, torch.float32), R.ray_points(inp, mode, torch.float64)
    assert x32.dtype == torch.float32 and x32.shape == (R_ * S, 3)
    assert torch.equal(x32.double(), x64)
    assert len(torch.unique(x32, dim=0)) > R_ * S // 2  # points, not one point


def test_ray_shapes_straddle_a_tile():
    """per-ray counts below, equal to and above a 32-point tile; no launch a whole number of workgroups"""
    assert sorted(S for _, S in R.RAY_SHAPES) == [5, 32, 40]
    assert [R_ * S for R_, S in R.RAY_SHAPES] == [65, 224, 200]


def test_lattice_generates_its_points_exactly():
    kw, expected = V.lattice()
    x32, x64 = expected(torch.float32), expected(torch.float64)
    assert x32.dtype == torch.float32 and x32.shape == (729, 3) and kw["dim"] == 9
    assert torch.equal(x32.double(), x64)
    # x slowest, and the step of 0.25 over the radius of 2 between neighbours along z
    assert torch.equal(x64[1] - x64[0], torch.tensor([0.0, 0.0, 0.125], dtype=torch.float64))
    assert torch.equal(x64[81] - x64[0], torch.tensor([0.125, 0.0, 0.0], dtype=torch.float64))
    assert torch.equal(x64[0], torch.tensor([-0.625, -0.25, -0.5], dtype=torch.float64))
    # the device's linspace (csrc/ncw_mlp.h grid_linspace: start + step i below the middle, end - step (steps - 1 - i) above)
    step = (kw["bound_max"][0] - kw["bound_min"][0]) / (kw["dim"] - 1)
    dev = torch.tensor([kw["bound_min"][0] + step * i if i < kw["dim"] // 2 else kw["bound_max"][0] - step * (kw["dim"] - 1 - i)
                        for i in range(kw["dim"])], dtype=torch.float64)
    assert step == 0.25 and torch.equal(dev, torch.linspace(-1, 1, 9, dtype=torch.float64))


@pytest.mark.parametrize("W", [64, 256])
@pytest.mark.parametrize("net", V.NETS, ids=V.net_id)
def test_statement_sdf_is_the_oracle(net, W):
    from oracle import neuconw_oracle as O

    c = V.case(W, net)
    assert c["x"].shape == (R.N_ORACLE, 3) and c["scale"] == (net[2] if len(net) > 2 else 1.0)
    got = V.exact_sdf(c)
    want = O.sdf_net(c["sd"], c["x"].double(), skip_in=c["skip"], scale=c["scale"], with_grad=False)[0]
    assert got.dtype == torch.float64 and float(want.abs().max()) > 0.1
    assert rel_err(got, want) < 1e-12, rel_err(got, want)


def test_every_layer_has_a_bias_of_its_own():
    """a bias read from another layer's slot must change the value: no Softplus layer's bias is zero or another layer's"""
    c = V.case(64, (11, (10,)))
    b = [c["sd"]["sdf_net.lin%d.bias" % l] for l in range(12)]
    for l in range(11):
        assert float(b[l].abs().min()) > 0 and 0.02 < float(b[l].std()) < 0.1, l
        for k in range(l):
            assert b[k].shape != b[l].shape or float((b[k] - b[l]).abs().max()) > 0.05, (k, l)
    assert float(b[11][0]) == -0.5  # the sdf row's: geometric initialisation


@pytest.mark.parametrize("prec_name", ["bf16", "f16"])
@pytest.mark.parametrize("W", V.WIDTHS)
@pytest.mark.parametrize("net", V.NETS, ids=V.net_id)
def test_twice_the_floor_is_within_the_tolerance_so_far(net, W, prec_name):
    """the plain 16-bit route runs at every width; 2 x floor <= the tolerance tests/test_gpu_sdf.py holds these chains to (worst
    cases, both at W = 64: bf16 1.02e-2 at (8, (4,)), fp16 9.6e-4 at (9, (4,)); V.bound caps at the tolerance in any case), so the
    bound of a case is never looser than before.  And the floor is a 16-bit rounding, not zero: above half an ulp of the format / 8"""
    c = V.case(W, net)
    fl = V.floor(c, prec_name)
    print("SDFVALUE floor W%d %-14s %-4s %.2e" % (W, V.net_id(net), prec_name, fl))
    assert 2 * fl <= V.TOL[prec_name], fl
    route = (W, prec_name, False if prec_name == "f16" else None)
    assert V.bound(c, route, net[0]) == (min(2 * fl, V.TOL[prec_name]), fl)
    assert fl > {"bf16": 2.0 ** -9, "f16": 2.0 ** -12}[prec_name] / 8, fl


def test_f32_floor_is_an_fp32_rounding():
    c = V.case(256, (8, (4,)))
    assert 0 < V.floor(c, "f32") < V.TOL_EXACT and V.floor(c, "f16-split") == V.floor(c, "f32")


def test_every_case_runs_on_exactly_one_kernel():
    for W in V.WIDTHS:
        for p in V.PRECS:
            for nl in range(1, 12):
                assert len(V.kernels(W, p, nl)) == 1, (W, p, nl, V.kernels(W, p, nl))
    # every row is reached by a route and a network of the GPU file
    reached = {V.route_plan(r, net[0])["kernel"] for r in V.ROUTES for net in V.NETS}
    assert reached == {k for _, _, _, _, k in V.KERNELS}
    assert len(V.ROUTES) == 11 and len(set(V.ROUTES)) == 11
    for r in V.ROUTES:
        assert r[2] is (False if r[1] == "f16" else None)


def test_route_plans():
    """residual matrices exactly where the split chain runs; where it cannot (n_layers = 1) the plain fp16 bound"""
    assert V.route_plan((256, "f16-split", None), 8) == dict(kernel="sdf_inferS2_kernel", rb=8, w_lo=True, bound="f16-split")
    assert V.route_plan((256, "f16-split", None), 9)["kernel"] == "sdf_inferS_kernel"
    assert V.route_plan((512, "f16-split", None), 1) == dict(kernel="sdf_infer_kernel<PrecBF16, 8 / 16>", rb=16, w_lo=False, bound="f16")
    assert V.route_plan((512, "f16", False), 8) == dict(kernel="sdf_infer16_kernel<T>", rb=16, w_lo=False, bound="f16")
    assert V.route_plan((64, "bf16", None), 11) == dict(kernel="sdf_infer_kernel<., 2>", rb=2, w_lo=False, bound="bf16")
    # ... which is what SDFNetwork.split_value decides
    for W, p, split in V.ROUTES:
        for nl, sk in [(8, (4,)), (2, (1,)), (1, ())]:
            net = R.make_net(W, nl, sk)
            if split is not None:
                net.sdf_split = split
            assert net.split_value(V.lib_prec(p)) == V.route_plan((W, p, split), nl)["w_lo"], (W, p, nl)
