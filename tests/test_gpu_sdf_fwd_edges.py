"""GPU: the 16-bit `ncw_sdf_fwd` at W = 256 at its shape edges -- in fp16 the split-precision kernels of csrc/ncw_split.hip
(sdf_fwdSA with the adjoint sweep's weights as hi + lo pairs, the default; sdf_fwdS without them), in bf16 the plain kernel of
csrc/ncw_sdf8.hip.  Every comparison here is EXACT: a column of an MFMA depends on nothing but its own point, so the same points
evaluated in another launch decomposition -- another workgroup, another tile of the workgroup, another lane group of the tile --
must give the same bits; any difference is an LDS fragment read from the wrong tile, k-unit, plane or buffer (the fragment rings
of the MFMA loops, the slices reloaded in place, the first sweep step's operand taken from the split buffer).  The accuracy of
these kernels against the fp64 oracle is pinned by tests/test_gpu_sdf.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

W = 256
N = 419                     # 13 tiles + 3 points: 3 full workgroups + one workgroup holding one full tile and a 3-point tile
SLICES = (1, 33, 129, 256)  # consecutive slices of the same points (sum = N): the partial tile, one point over a tile, one
#                             over a workgroup, two workgroups
# (n_layers, skip_in) of SDFNetwork; the kernels' L = n_layers + 1: L = 9 / skip 4 is the headline network; L = 3 / skip 1: the
# only hidden layer of the chain is the skip layer and the sweep's first layer is its last (the slices reloaded in place are
# never used, the gamma job follows at once); L = 4 without a skip: no gamma job inside the sweep
NETS = [(8, (4,)), (2, (1,)), (3, ())]
# (precision, adj_split): fp16 with and without the transposed residuals (sdf_fwdSA / sdf_fwdS), bf16 (no split path)
MODES = [("f16", True), ("f16", False), ("bf16", None)]


def _net(n_layers, skip, adj, seed=31):
    import neuralrecon_w_amd as nw

    torch.manual_seed(seed)
    net = nw.SDFNetwork(d_in=3, d_out=W + 1, d_hidden=W, n_layers=n_layers, skip_in=skip)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("weight_g"):
                p.mul_(1.0 + 0.1 * torch.randn_like(p))
            if n.endswith("weight_v") and not n.startswith("lin%d" % (net.n_lin - 1)):
                p.add_(0.02 * torch.randn_like(p))  # make the encoding / skip columns non-zero
    if adj is not None:
        net.adj_split = adj
    return net.cuda()


def _points(seed=32):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(N, 3, generator=g) * 2 - 1) * 1.2).cuda()


def _run(net, prec_name, adj, x, lo, hi, train=True):
    """points lo .. hi-1 as one launch: {field: rows of the valid points}"""
    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd.neuconw import points_struct
    from neuralrecon_w_amd.stash import StashCache

    prec = {"bf16": nw.PREC_BF16, "f16": nw.PREC_F16}[prec_name]
    n = hi - lo
    sdf, grad, c = net.fwd_stash(points_struct(x=x[lo:hi].contiguous()), n, prec, train=train)
    pn = c["plan"].net
    assert bool(pn.w_lo[0]) == (prec_name == "f16")       # the split value chain ...
    assert bool(pn.wt_lo[0]) == bool(adj)                 # ... and the sweep with hi + lo weights
    ar, ids = c["arena"], c["ids"]
    out = {"sdf": sdf.clone(), "grad": grad.clone(), "feat": ar.to_rows(ids["feat"], W)}
    for l, i in ids["h"].items():
        out["h%d" % l] = ar.to_rows(i, W)
    if train:
        out["gamma"] = ar.to_rows(ids["gamma"], 64)
        for l, i in ids["t"].items():
            out["t%d" % l] = ar.to_rows(i, W)
    torch.cuda.synchronize()
    StashCache.release(c["lease"])
    return out


@pytest.mark.parametrize("n_layers,skip", NETS)
@pytest.mark.parametrize("prec_name,adj", MODES)
def test_launch_decomposition_invariance(n_layers, skip, prec_name, adj):
    net, x = _net(n_layers, skip, adj), _points()
    full = _run(net, prec_name, adj, x, 0, N)
    assert set(full) == {"sdf", "grad", "feat", "gamma"} | {"h%d" % l for l in range(1, n_layers + 1)} | {"t%d" % l for l in range(n_layers)}
    for k, v in full.items():
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, k
    lo = 0
    for m in SLICES:
        part = _run(net, prec_name, adj, x, lo, lo + m)
        for k, v in full.items():
            assert torch.equal(part[k], v[lo:lo + m]), (k, n_layers, prec_name, adj, lo, m)
        lo += m
    assert lo == N


@pytest.mark.parametrize("n_layers,skip", NETS)
@pytest.mark.parametrize("prec_name,adj", MODES)
def test_forward_only_render_equals_training_forward(n_layers, skip, prec_name, adj):
    """the forward-only launch (NcwSdfStash.t[0] == NULL: sdf_fwdSA<false> / sdf_fwdS<false> / sdf_fwdB<false>) against the
    training launch: sdf, grad and feat bit for bit"""
    net, x = _net(n_layers, skip, adj), _points()
    full = _run(net, prec_name, adj, x, 0, N)
    with torch.no_grad():
        rend = _run(net, prec_name, adj, x, 0, N, train=False)
    for k in ("sdf", "grad", "feat"):
        assert float(full[k].abs().max()) > 0, k
        assert torch.equal(rend[k], full[k]), (k, n_layers, prec_name, adj)
