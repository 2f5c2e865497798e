"""GPU: the value-only SDF evaluations -- `ncw_sdf_infer`, `ncw_sdf_infer_rays`, `ncw_sdf_infer_points` -- on every kernel
`sdf_infer_any` (csrc/ncw_sdf.hip) routes them to, at their shape edges, depths, skip positions and point sources.  The routes
(tests/_sdf_value_cases.py KERNELS; n_layers is SDFNetwork's, the kernels' L = n_layers + 1):

  W = 64,  any precision                              sdf_infer_kernel<., 2>                       (ncw_sdf.hip)
  W = 256, f32                                        sdf_infer_kernel<PrecF32, 8>
  W = 512, f32, n_layers = 1                          sdf_infer_kernel<PrecF32, 16>                (sdf16f_on needs L >= 3)
  W = 256, bf16 / plain f16, n_layers >= 2            sdf_inferC_kernel                            (ncw_pp.hip: pipelined, two tile groups)
  W = 256 / 512, any 16-bit, n_layers = 1             sdf_infer_kernel<PrecBF16, 8 / 16>           (the streamed / pipelined kernels need L >= 3)
  W = 256, f16 split (default), 2 <= n_layers <= 8    sdf_inferS2_kernel                           (ncw_split.hip: pipelined, 8 layers of bias staging)
  W = 256, f16 split, 9 <= n_layers <= 11             sdf_inferS_kernel                            (burst)
  W = 512, f32, n_layers >= 2                         sdf_infer16f_kernel                          (ncw_sdf16f.hip)
  W = 512, bf16 / plain f16, n_layers >= 2            sdf_infer16_kernel<T>, T = 2 / 3 / 4         (ncw_sdf16.hip)
  W = 512, f16 split, n_layers >= 2                   sdf_inferS16_kernel                          (ncw_sdf16.hip)

Every case asserts the packed plan of its route first (plan.net.rb, residual matrices present or not), so that it cannot silently
run on another kernel than the one it names.

a. EXACT: a column of an MFMA depends on nothing but its own point, so the same points in another launch decomposition -- another
   workgroup, tile group, tile, lane group -- give the same bits.  419 points (13 tiles + 3) against consecutive slices of 1, 33, 129
   and 256 points.  T = 3 / 4 of sdf_infer16_kernel: s16_tiles_per_wg minimises ceil(workgroups / 256) x (12 + 10.7 T) over T = 2, 3, 4
   (workgroups = ceil(tiles / T)); up to 512 tiles T = 2 runs in one round (33.4), from 513 to 768 tiles T = 2 needs two rounds (66.8)
   and T = 3 one (44.1), from 769 to 1024 tiles T = 3 needs two (88.2) and T = 4 one (54.8).  16,421 points = 514 tiles pick T = 3,
   24,613 points = 770 tiles pick T = 4, and chunks of 4,000 points = 125 tiles (and the rests of 421 / 613 points) pick T = 2.  The
   test cannot observe T: this arithmetic has to be redone when the cost model changes.
b. EXACT: the kernel writes what it owns -- through the C ABI into a buffer of n + 160 floats filled with one NaN bit pattern,
   n = 1, 31, 33, 127, 129, 419: floats n .. keep their bytes, floats 0 .. n-1 equal the plain run.
c. EXACT: point sources.  Rays whose points are exact in fp32 (tests/test_sdf_value_host.py) through NcwPoints mode 1, mode 2 and
   `ncw_sdf_infer_rays` equal `net.sdf` of the same points; per-ray counts 5, 32 and 40 (65, 224 and 200 points).  Mode 3: a lattice
   with exact points, a ragged range of it in one launch and in two.
d. Against the fp64 statement of tests/_sdf_bwd_ref.py (777 points, tests/_util.rel_err), every route x every network.  Bounds --
   none comes from the kernels: the plain 16-bit chains 2 x the rounding floor of the sdf value (tests/_sdf_value_cases.py), capped
   by the tolerance tests/test_gpu_sdf.py holds them to (bf16 3e-2, fp16 2e-3); the exact-fp32 and the split-precision kernels
   5e-6 (test_split_precision_value_path).  The factor 2 is the margin of tests/test_gpu_color_edges.py and
   tests/test_gpu_sdf_bwd_edges.py for the same construction: f32 accumulation order, the fast exp, ties -- and here that the
   value-only kernels round h in t-units (NCW_TU h) where the floor rounds h: the same distribution, not the same bits.  `f16-split`
   at n_layers = 1 has no split chain (SDFNetwork.split_value needs n_lin >= 3) and takes the plain fp16 bound.
e. Returns before any launch: the codes of include/neuconw_hip.h, the output keeps its bytes.

Networks -- what the value-only kernels do differently:
  (8, (4,))    L = 9, the headline network.  sdf_inferC_kernel loads the gamma columns of layer 4 (units 16 .. 18 of w[4]) into `wx`
               while layer 3's last segment runs; sdf_inferS2_kernel loads them at the head of layer 4 (`gh` / `gl`) and sits at its
               bias-staging limit (NL = 8 layers); NL is even on sdf_inferC_kernel.  Also with scale = 1.7: net.scale enters at the
               prologue (xs = x scale) and at the final division by scale x NCW_TU.
  (1, ())      L = 2.  No hidden product at all; the generic kernel at every width, also in 16-bit (and in fp32 at W = 512).
  (2, (1,))    L = 3, skip_layer == 1: sdf_inferC_kernel reloads `wx` from w[1] units 16 .. 18 straight after layer 0; the hidden loop
               runs once and its prefetch re-reads its own slice (`more` false; sdf_inferS2_kernel the same); the first s16_prefetch of
               the W = 512 kernels is the last.
  (3, (1,))    L = 4, skip_layer == 1 with a following layer (`more` true); NL = 3 is odd, so the drain of sdf_inferC_kernel lands in
               the other parity buffer and the sdf row reads that one.
  (3, ())      no gamma job after layer 0; `wx` is never reloaded.
  (9, (4,))    L = 10.  The first depth on the burst split kernel (sdf_inferS_kernel: NL = 9 > 8); NL is odd on sdf_inferC_kernel.
  (11, (10,))  L = 12 = NCW_MAX_LAYERS.  The last slot of every per-layer array and of PP_BIAS (12 KiB: NL = 11 of 12 slots; slot 11
               is the sdf row's bias, read from global memory) is live; the skip layer is the last hidden layer, so sdf_inferC_kernel
               fetches its gamma columns under the last-but-one layer's last segment.

The networks are those of tests/_sdf_bwd_ref.py with non-zero biases in the Softplus layers (tests/_sdf_value_cases.py case(): the
geometric initialisation leaves them all at 0, and a bias read from another layer's slot would go unseen).

Measured on MI355X (printed by part d on its first run; every case within its bound, no bound moved):
  W64-f32        n8s4           sdf_infer_kernel<., 2>             gpu 4.72e-07 floor 4.44e-07 bound 5.00e-06
  W64-f32        n1sx           sdf_infer_kernel<., 2>             gpu 2.07e-07 floor 3.64e-07 bound 5.00e-06
  W64-f32        n11s10         sdf_infer_kernel<., 2>             gpu 3.42e-07 floor 4.16e-07 bound 5.00e-06
  W64-bf16       n8s4           sdf_infer_kernel<., 2>             gpu 1.02e-02 floor 1.02e-02 bound 2.03e-02
  W64-bf16       n1sx           sdf_infer_kernel<., 2>             gpu 3.55e-03 floor 3.55e-03 bound 7.11e-03
  W64-bf16       n11s10         sdf_infer_kernel<., 2>             gpu 5.96e-03 floor 5.96e-03 bound 1.19e-02
  W64-f16        n8s4           sdf_infer_kernel<., 2>             gpu 8.50e-04 floor 8.50e-04 bound 1.70e-03
  W64-f16        n1sx           sdf_infer_kernel<., 2>             gpu 3.84e-04 floor 3.83e-04 bound 7.67e-04
  W64-f16        n11s10         sdf_infer_kernel<., 2>             gpu 9.11e-04 floor 9.11e-04 bound 1.82e-03
  W256-f32       n8s4           sdf_infer_kernel<PrecF32, 8>       gpu 7.16e-07 floor 4.25e-07 bound 5.00e-06
  W256-f32       n1sx           sdf_infer_kernel<PrecF32, 8>       gpu 4.97e-07 floor 4.58e-07 bound 5.00e-06
  W256-f32       n2s1           sdf_infer_kernel<PrecF32, 8>       gpu 6.19e-07 floor 4.18e-07 bound 5.00e-06
  W256-f32       n3s1           sdf_infer_kernel<PrecF32, 8>       gpu 5.34e-07 floor 3.62e-07 bound 5.00e-06
  W256-f32       n3sx           sdf_infer_kernel<PrecF32, 8>       gpu 4.85e-07 floor 4.47e-07 bound 5.00e-06
  W256-f32       n11s10         sdf_infer_kernel<PrecF32, 8>       gpu 8.53e-07 floor 4.15e-07 bound 5.00e-06
  W256-f32       n9s4           sdf_infer_kernel<PrecF32, 8>       gpu 7.42e-07 floor 4.21e-07 bound 5.00e-06
  W256-f32       n8s4-scale1.7  sdf_infer_kernel<PrecF32, 8>       gpu 6.26e-07 floor 3.76e-07 bound 5.00e-06
  W256-bf16      n8s4           sdf_inferC_kernel                  gpu 3.04e-03 floor 2.57e-03 bound 5.15e-03
  W256-bf16      n1sx           sdf_infer_kernel<PrecBF16, 8 / 16> gpu 1.93e-03 floor 1.93e-03 bound 3.87e-03
  W256-bf16      n2s1           sdf_inferC_kernel                  gpu 2.06e-03 floor 1.86e-03 bound 3.72e-03
  W256-bf16      n3s1           sdf_inferC_kernel                  gpu 2.46e-03 floor 2.12e-03 bound 4.24e-03
  W256-bf16      n3sx           sdf_inferC_kernel                  gpu 1.89e-03 floor 1.84e-03 bound 3.68e-03
  W256-bf16      n11s10         sdf_inferC_kernel                  gpu 4.60e-03 floor 3.82e-03 bound 7.64e-03
  W256-bf16      n9s4           sdf_inferC_kernel                  gpu 2.69e-03 floor 3.51e-03 bound 7.02e-03
  W256-bf16      n8s4-scale1.7  sdf_inferC_kernel                  gpu 3.40e-03 floor 3.28e-03 bound 6.55e-03
  W256-f16       n8s4           sdf_inferC_kernel                  gpu 3.21e-04 floor 3.19e-04 bound 6.37e-04
  W256-f16       n1sx           sdf_infer_kernel<PrecBF16, 8 / 16> gpu 1.79e-04 floor 1.79e-04 bound 3.58e-04
  W256-f16       n2s1           sdf_inferC_kernel                  gpu 3.03e-04 floor 2.23e-04 bound 4.46e-04
  W256-f16       n3s1           sdf_inferC_kernel                  gpu 3.21e-04 floor 2.70e-04 bound 5.40e-04
  W256-f16       n3sx           sdf_inferC_kernel                  gpu 3.55e-04 floor 4.01e-04 bound 8.02e-04
  W256-f16       n11s10         sdf_inferC_kernel                  gpu 3.71e-04 floor 4.35e-04 bound 8.70e-04
  W256-f16       n9s4           sdf_inferC_kernel                  gpu 3.40e-04 floor 3.18e-04 bound 6.37e-04
  W256-f16       n8s4-scale1.7  sdf_inferC_kernel                  gpu 3.63e-04 floor 3.39e-04 bound 6.78e-04
  W256-f16-split n8s4           sdf_inferS2_kernel                 gpu 6.44e-07 floor 4.25e-07 bound 5.00e-06
  W256-f16-split n1sx           sdf_infer_kernel<PrecBF16, 8 / 16> gpu 1.79e-04 floor 1.79e-04 bound 3.58e-04
  W256-f16-split n2s1           sdf_inferS2_kernel                 gpu 4.55e-07 floor 4.18e-07 bound 5.00e-06
  W256-f16-split n3s1           sdf_inferS2_kernel                 gpu 4.20e-07 floor 3.62e-07 bound 5.00e-06
  W256-f16-split n3sx           sdf_inferS2_kernel                 gpu 5.25e-07 floor 4.47e-07 bound 5.00e-06
  W256-f16-split n11s10         sdf_inferS_kernel                  gpu 6.63e-07 floor 4.15e-07 bound 5.00e-06
  W256-f16-split n9s4           sdf_inferS_kernel                  gpu 6.96e-07 floor 4.21e-07 bound 5.00e-06
  W256-f16-split n8s4-scale1.7  sdf_inferS2_kernel                 gpu 5.36e-07 floor 3.76e-07 bound 5.00e-06
  W512-f32       n8s4           sdf_infer16f_kernel                gpu 9.29e-07 floor 4.18e-07 bound 5.00e-06
  W512-f32       n1sx           sdf_infer_kernel<PrecF32, 16>      gpu 6.74e-07 floor 4.43e-07 bound 5.00e-06
  W512-f32       n2s1           sdf_infer16f_kernel                gpu 1.20e-06 floor 5.80e-07 bound 5.00e-06
  W512-f32       n3s1           sdf_infer16f_kernel                gpu 6.89e-07 floor 4.97e-07 bound 5.00e-06
  W512-f32       n3sx           sdf_infer16f_kernel                gpu 8.60e-07 floor 4.99e-07 bound 5.00e-06
  W512-f32       n11s10         sdf_infer16f_kernel                gpu 1.00e-06 floor 3.94e-07 bound 5.00e-06
  W512-f32       n9s4           sdf_infer16f_kernel                gpu 1.01e-06 floor 4.00e-07 bound 5.00e-06
  W512-f32       n8s4-scale1.7  sdf_infer16f_kernel                gpu 9.65e-07 floor 4.39e-07 bound 5.00e-06
  W512-bf16      n8s4           sdf_infer16_kernel<T>              gpu 2.28e-03 floor 1.79e-03 bound 3.58e-03
  W512-bf16      n1sx           sdf_infer_kernel<PrecBF16, 8 / 16> gpu 1.83e-03 floor 1.83e-03 bound 3.66e-03
  W512-bf16      n2s1           sdf_infer16_kernel<T>              gpu 2.15e-03 floor 2.14e-03 bound 4.29e-03
  W512-bf16      n3s1           sdf_infer16_kernel<T>              gpu 2.12e-03 floor 1.87e-03 bound 3.74e-03
  W512-bf16      n3sx           sdf_infer16_kernel<T>              gpu 1.85e-03 floor 1.68e-03 bound 3.36e-03
  W512-bf16      n11s10         sdf_infer16_kernel<T>              gpu 2.78e-03 floor 2.70e-03 bound 5.40e-03
  W512-bf16      n9s4           sdf_infer16_kernel<T>              gpu 2.16e-03 floor 2.47e-03 bound 4.94e-03
  W512-bf16      n8s4-scale1.7  sdf_infer16_kernel<T>              gpu 1.90e-03 floor 2.43e-03 bound 4.86e-03
  W512-f16       n8s4           sdf_infer16_kernel<T>              gpu 3.01e-04 floor 3.00e-04 bound 6.00e-04
  W512-f16       n1sx           sdf_infer_kernel<PrecBF16, 8 / 16> gpu 1.83e-04 floor 1.83e-04 bound 3.66e-04
  W512-f16       n2s1           sdf_infer16_kernel<T>              gpu 2.22e-04 floor 2.09e-04 bound 4.17e-04
  W512-f16       n3s1           sdf_infer16_kernel<T>              gpu 2.15e-04 floor 2.05e-04 bound 4.10e-04
  W512-f16       n3sx           sdf_infer16_kernel<T>              gpu 2.68e-04 floor 2.77e-04 bound 5.54e-04
  W512-f16       n11s10         sdf_infer16_kernel<T>              gpu 2.82e-04 floor 2.64e-04 bound 5.27e-04
  W512-f16       n9s4           sdf_infer16_kernel<T>              gpu 2.27e-04 floor 2.69e-04 bound 5.39e-04
  W512-f16       n8s4-scale1.7  sdf_infer16_kernel<T>              gpu 3.03e-04 floor 3.30e-04 bound 6.60e-04
  W512-f16-split n8s4           sdf_inferS16_kernel                gpu 7.62e-07 floor 4.18e-07 bound 5.00e-06
  W512-f16-split n1sx           sdf_infer_kernel<PrecBF16, 8 / 16> gpu 1.83e-04 floor 1.83e-04 bound 3.66e-04
  W512-f16-split n2s1           sdf_inferS16_kernel                gpu 6.79e-07 floor 5.80e-07 bound 5.00e-06
  W512-f16-split n3s1           sdf_inferS16_kernel                gpu 5.10e-07 floor 4.97e-07 bound 5.00e-06
  W512-f16-split n3sx           sdf_inferS16_kernel                gpu 6.43e-07 floor 4.99e-07 bound 5.00e-06
  W512-f16-split n11s10         sdf_inferS16_kernel                gpu 7.28e-07 floor 3.94e-07 bound 5.00e-06
  W512-f16-split n9s4           sdf_inferS16_kernel                gpu 7.24e-07 floor 4.00e-07 bound 5.00e-06
  W512-f16-split n8s4-scale1.7  sdf_inferS16_kernel                gpu 8.09e-07 floor 4.39e-07 bound 5.00e-06
The generic kernel rounds h itself and sits on its floor (gpu = floor to three digits); the t-unit kernels (sdf_inferC_kernel,
sdf_infer16_kernel) are at 0.77 .. 1.36 x the floor, at most 0.68 of their bound (W256-f16 n2s1): the supposition of part d holds.
Wall time of the file on MI355X: 7 s for its 212 tests; no case is left out.
"""
import pytest
import torch

from tests import _sdf_bwd_ref as R
from tests import _sdf_value_cases as V
from tests._util import rel_err

pytestmark = pytest.mark.gpu
NCW_E_BADARG, NCW_E_UNSUPPORTED = -1, -2  # include/neuconw_hip.h

N = R.N_EDGE                # 13 tiles + 3 points
SLICES = (1, 33, 129, 256)  # consecutive slices of the same points (sum = N): inside a tile, one point past a tile, one past a workgroup
NAN_BITS = 0x7FC12345       # a quiet NaN no kernel produces
HEAD = (8, (4,))

routes = pytest.mark.parametrize("route", V.ROUTES, ids=V.route_id)
wide_routes = [r for r in V.ROUTES if r[0] != 64]
_GPU_NETS = {}


def _net(route, net):
    """one module per (W, network) for the whole file (the W = 512 packing is the expensive part); the route's switch set on it, its
    packed plan asserted -> (module, plan, precision)"""
    W, prec_name, split = route
    key = (W,) + tuple(net)
    if key not in _GPU_NETS:
        _GPU_NETS[key] = R.gpu_net(V.case(W, net))
    m = _GPU_NETS[key]
    m.sdf_split = split  # None: the default (SDFNetwork.split_value)
    prec = V.lib_prec(prec_name)
    plan, want = m.packed(prec), V.route_plan(route, net[0])
    assert plan.net.rb == want["rb"] and bool(plan.net.w_lo[0]) == want["w_lo"], (route, net, want)
    assert plan.net.n_layers == net[0] + 1 and plan.net.skip_layer == (net[1][0] if net[1] else -1)
    return m, plan, prec


def _nan_buffer(n):
    return torch.full((n,), NAN_BITS, dtype=torch.int32, device="cuda")


def _infer(plan, prec, x, n, out_i32):
    """lib.ncw_sdf_infer straight through the C ABI into an int32-typed buffer"""
    from neuralrecon_w_amd import lib as L

    r = L.get_lib().ncw_sdf_infer(plan.net, prec, L.ptr(x), n, L.ptr(out_i32), L.stream_ptr(x.device))
    torch.cuda.synchronize()
    return r


# ---- a. launch decomposition -------------------------------------------------------------------------------------------------------
def _decomposition_cases():
    out = []
    for r in V.ROUTES:
        nets = [HEAD, (1, ())] if r[0] == 64 else [HEAD, (2, (1,)), (3, ()), (1, ()), (11, (10,))]
        if r[:2] == (256, "f16-split"):
            nets.append((9, (4,)))
        out += [pytest.param(r, n, id="%s-%s" % (V.route_id(r), V.net_id(n))) for n in nets]
    return out


@pytest.mark.parametrize("route,net", _decomposition_cases())
def test_launch_decomposition_invariance(route, net):
    m, _, prec = _net(route, net)
    x = V.case(route[0], net, n=N)["x"].cuda()
    full = m.sdf(x, prec)
    assert full.shape == (N, 1) and bool(torch.isfinite(full).all()) and float(full.abs().max()) > 0
    lo = 0
    for k in SLICES:
        part = m.sdf(x[lo:lo + k].contiguous(), prec)
        assert torch.equal(part, full[lo:lo + k]), (route, net, lo, k)
        lo += k
    assert lo == N


@pytest.mark.parametrize("n", [16421, 24613])
@pytest.mark.parametrize("prec_name", ["bf16", "f16"])
def test_w512_three_and_four_tiles_per_workgroup(prec_name, n):
    """sdf_infer16_kernel<3> (16,421 points = 514 tiles) and <4> (24,613 points = 770 tiles) against <2> (chunks of 4,000 points =
    125 tiles): the module docstring has the arithmetic of s16_tiles_per_wg"""
    route = (512, prec_name, False if prec_name == "f16" else None)
    m, _, prec = _net(route, HEAD)
    x = R.points(n).cuda()
    full = m.sdf(x, prec)
    assert bool(torch.isfinite(full).all()) and float(full.abs().max()) > 0
    for lo in range(0, n, 4000):
        assert torch.equal(m.sdf(x[lo:lo + 4000].contiguous(), prec), full[lo:lo + 4000]), (prec_name, n, lo)


# ---- b. what the kernel writes ------------------------------------------------------------------------------------------------------
# every W = 256 / 512 route on the headline network, and the kernels it does not reach: the burst split kernel, the generic kernel in
# 16-bit at both widths and in fp32 at W = 512 (n_layers = 1), the W = 64 kernel
OWNS = [(r, HEAD) for r in wide_routes] + [((256, "f16-split", None), (9, (4,))), ((256, "bf16", None), (1, ())),
                                           ((512, "f16", False), (1, ())), ((512, "f32", None), (1, ())), ((64, "f32", None), HEAD)]


@pytest.mark.parametrize("route,net", [pytest.param(r, n, id="%s-%s" % (V.route_id(r), V.net_id(n))) for r, n in OWNS])
def test_kernel_writes_what_it_owns(route, net):
    m, plan, prec = _net(route, net)
    x = V.case(route[0], net, n=N)["x"].cuda()
    for n in (1, 31, 33, 127, 129, 419):
        xs = x[:n].contiguous()
        plain = m.sdf(xs, prec)[:, 0]
        buf = _nan_buffer(n + 160)
        assert _infer(plan, prec, xs, n, buf) == 0
        assert bool((buf[n:] == NAN_BITS).all()), (route, net, n)
        assert torch.equal(buf[:n], plain.view(torch.int32)) and bool(torch.isfinite(plain).all()), (route, net, n)


# ---- c. point sources ---------------------------------------------------------------------------------------------------------------
source_routes = pytest.mark.parametrize("route", wide_routes + [(64, "f32", None)], ids=V.route_id)
source_nets = pytest.mark.parametrize("net", [HEAD, (2, (1,))], ids=V.net_id)


@source_routes
@source_nets
@pytest.mark.parametrize("R_,S", R.RAY_SHAPES)
def test_ray_sources(route, net, R_, S):
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd.neuconw import points_struct

    m, plan, prec = _net(route, net)
    n = R_ * S
    inp = R.dyadic_rays(R_, S)
    d = {k: v.cuda().contiguous() for k, v in inp.items()}
    lib, stream = L.get_lib(), L.stream_ptr(d["z"].device)
    want = {mode: m.sdf(R.ray_points(inp, mode, torch.float32).cuda(), prec)[:, 0] for mode in (1, 2)}
    assert float(want[1].abs().max()) > 0 and not torch.equal(want[1], want[2])
    for mode in (1, 2):
        pts = points_struct(rays_o=d["rays_o"], rays_d=d["rays_d"], z=d["z"], sample_dist=d["sample_dist"] if mode == 2 else None,
                            mode=mode)
        assert pts.per_ray == S and pts.mode == mode
        out = _nan_buffer(n).view(torch.float32)
        assert lib.ncw_sdf_infer_points(plan.net, prec, pts, n, L.ptr(out), stream) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, want[mode]), (route, net, R_, S, mode)
    out = _nan_buffer(n).view(torch.float32)
    assert lib.ncw_sdf_infer_rays(plan.net, prec, L.ptr(d["rays_o"]), L.ptr(d["rays_d"]), L.ptr(d["z"]), R_, S, L.ptr(out), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want[1]), (route, net, R_, S, "rays")


@source_routes
@source_nets
def test_lattice_source(route, net):
    """NcwPoints mode 3 through grid.sdf_grid_range: grid points 37 .. 728 of a 9^3 lattice, in one launch and in two ragged ones"""
    from neuralrecon_w_amd import grid

    m, _, prec = _net(route, net)
    kw, expected = V.lattice()
    start, count = 37, 692
    assert start + count == kw["dim"] ** 3
    want = m.sdf(expected(torch.float32)[start:start + count].cuda(), prec)[:, 0]
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    one = grid.sdf_grid_range(m, start=start, count=count, prec=prec, **kw)
    two = torch.cat([grid.sdf_grid_range(m, start=start, count=301, prec=prec, **kw),
                     grid.sdf_grid_range(m, start=start + 301, count=count - 301, prec=prec, **kw)])
    assert torch.equal(one, want) and torch.equal(two, want), (route, net)


# ---- d. against the fp64 statement --------------------------------------------------------------------------------------------------
def _accuracy_cases():
    out = []
    for r in V.ROUTES:
        nets = [HEAD, (1, ()), (11, (10,))] if r[0] == 64 else V.NETS
        out += [pytest.param(r, n, id="%s-%s" % (V.route_id(r), V.net_id(n))) for n in nets]
    return out


@pytest.mark.parametrize("route,net", _accuracy_cases())
def test_sdf_vs_statement(route, net):
    m, _, prec = _net(route, net)
    c = V.case(route[0], net)
    assert c["x"].shape[0] == R.N_ORACLE
    bound, fl = V.bound(c, route, net[0])
    got = m.sdf(c["x"].cuda(), prec).cpu()[:, 0]
    err = rel_err(got, V.exact_sdf(c))
    print("SDFVALUE %-14s %-14s %-34s gpu %.2e floor %.2e bound %.2e"
          % (V.route_id(route), V.net_id(net), V.route_plan(route, net[0])["kernel"], err, fl, bound))
    assert bool(torch.isfinite(got).all()) and err < bound, (route, net, err, fl, bound)


# ---- e. returns before any launch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [(64, "f32", None), (256, "f16-split", None), (512, "bf16", None)], ids=V.route_id)
def test_entry_points_return_before_any_launch(route):
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd.neuconw import points_struct

    m, plan, prec = _net(route, HEAD)
    R_, S = R.RAY_SHAPES[0]
    n = R_ * S
    d = {k: v.cuda().contiguous() for k, v in R.dyadic_rays(R_, S).items()}
    x = R.ray_points(R.dyadic_rays(R_, S), 1, torch.float32).cuda()
    lib, stream = L.get_lib(), L.stream_ptr(x.device)
    out = _nan_buffer(n)
    o, dd, z = L.ptr(d["rays_o"]), L.ptr(d["rays_d"]), L.ptr(d["z"])
    pts = points_struct(x=x)
    rays = points_struct(rays_o=d["rays_o"], rays_d=d["rays_d"], z=d["z"], sample_dist=d["sample_dist"], mode=2)
    sel = L.NcwPoints.from_buffer_copy(rays)
    sel.mode = 4

    def untouched(code):
        torch.cuda.synchronize()
        assert bool((out == NAN_BITS).all())
        return code

    assert untouched(lib.ncw_sdf_infer_points(plan.net, prec, sel, n, L.ptr(out), stream)) == NCW_E_UNSUPPORTED
    for bad in (7, -1, 3):
        assert untouched(lib.ncw_sdf_infer(plan.net, bad, L.ptr(x), n, L.ptr(out), stream)) == NCW_E_BADARG
        assert untouched(lib.ncw_sdf_infer_points(plan.net, bad, pts, n, L.ptr(out), stream)) == NCW_E_BADARG
        assert untouched(lib.ncw_sdf_infer_rays(plan.net, bad, o, dd, z, R_, S, L.ptr(out), stream)) == NCW_E_BADARG
    assert untouched(lib.ncw_sdf_infer(plan.net, prec, L.ptr(x), -1, L.ptr(out), stream)) == NCW_E_BADARG
    assert untouched(lib.ncw_sdf_infer_points(plan.net, prec, pts, -1, L.ptr(out), stream)) == NCW_E_BADARG
    assert untouched(lib.ncw_sdf_infer_points(plan.net, prec, None, n, L.ptr(out), stream)) == NCW_E_BADARG
    assert untouched(lib.ncw_sdf_infer_rays(plan.net, prec, o, dd, z, R_, 0, L.ptr(out), stream)) == NCW_E_BADARG
    assert untouched(lib.ncw_sdf_infer(plan.net, prec, L.ptr(x), 0, L.ptr(out), stream)) == 0
    assert untouched(lib.ncw_sdf_infer_points(plan.net, prec, pts, 0, L.ptr(out), stream)) == 0
    assert untouched(lib.ncw_sdf_infer_points(plan.net, prec, rays, 0, L.ptr(out), stream)) == 0
    assert untouched(lib.ncw_sdf_infer_rays(plan.net, prec, o, dd, z, 0, S, L.ptr(out), stream)) == 0
    # ... and the same arguments do launch
    assert lib.ncw_sdf_infer_rays(plan.net, prec, o, dd, z, R_, S, L.ptr(out), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.float32), m.sdf(x, prec)[:, 0])
