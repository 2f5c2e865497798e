"""Time the four LDS kernels of csrc/ncw_rays.hip (upsample, sort_merge, composite_fwd, composite_bwd) with device events.

Shapes: the headline step (R = 1024, S = 128, O = 4, and the sampler's calls for 64 + 64 samples in two up-sampling steps) and
the reference's defaults on the large capacity (S = 1056, O = 32, up-sampling at n = 1023).  Buffers and ABI structs are made
once through rayops and the launches replayed through the C ABI, so a window holds kernels and not allocations.  Every shape is
warmed up; a timed window holds at least half a second of launches and ends in a synchronise.  Prints one JSON line: us per
launch.  Inputs are those of the per-ray tests (tests/_ray_cases.py: comp_inputs).

--floor adds what the floor-normal loss costs: composite_bwd with a d_normals buffer (the other instantiation of the kernel) at
both shapes, and the two launches of the floor term (ncw_ray_floor_fwd / _bwd) at R = 1024."""
import argparse
import ctypes
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralrecon_w_amd import lib as L  # noqa: E402
from neuralrecon_w_amd import rayops  # noqa: E402
from tests._ray_cases import comp_inputs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--floor", action="store_true", help="also time composite_bwd with d_normals and the floor-term launches")
args = ap.parse_args()

R = 1024
dev = torch.device("cuda:0")
lib, st = L.get_lib(), L.stream_ptr(dev)


def timeit(launch, window_ms=600.0):
    """us per launch over a window of >= 500 ms; the launch count is grown until the window is that long."""
    for _ in range(20):
        launch()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 50
    while True:
        start.record()
        for _ in range(n):
            launch()
        end.record()
        torch.cuda.synchronize()
        ms = start.elapsed_time(end)
        if ms >= 500.0:
            return 1e3 * ms / n
        n = int(math.ceil(n * window_ms / max(ms, 1e-3)))


def composite(S, O):
    """-> (inputs on the device, us per forward, us per backward)"""
    I = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in comp_inputs(R, S, O, 7).items()}
    ctx = rayops.CompositeCtx(I["o"], I["d"], I["z"], I["sample_dist"], I["sdf"], I["grad"], I["rgb"], I["inv_s"], 0.3,
                              I["z_feed"], I["density"], I["bg_rgb"], background_rgb=torch.zeros(3, device=dev))
    out = ctx.forward()
    out_struct = L.NcwCompositeOut()
    for k, v in out.items():
        setattr(out_struct, k, v.data_ptr())
    upstream = dict(d_color=torch.randn(R, 3, device=dev), d_weights_sum=torch.randn(R, device=dev),
                    d_depth=torch.randn(R, device=dev), d_eik_num=torch.randn(R, device=dev))
    adjoints = ctx.backward(*upstream.values())
    grad_struct = L.NcwCompositeGrad()
    for k, v in list(upstream.items()) + list(adjoints.items()):
        setattr(grad_struct, k, v.data_ptr())
    grad_struct.grad_scale = 1.0
    fwd = timeit(lambda: lib.ncw_composite_fwd(ctx.cin, out_struct, st))
    bwd = timeit(lambda: lib.ncw_composite_bwd(ctx.cin, grad_struct, st))
    if args.floor:
        d_normals = torch.randn(R, 3, device=dev)
        grad_struct.d_normals = d_normals.data_ptr()
        res["composite_bwd_dn_%d+%d" % (S, O)] = timeit(lambda: lib.ncw_composite_bwd(ctx.cin, grad_struct, st))
    return I, fwd, bwd


def floor_term(I):
    normals, d_fe = torch.randn(R, 3, device=dev), torch.randn(R, 3, device=dev)
    label = torch.where(torch.rand(R, device=dev) < 0.3, 6, 0)
    depth, fe, scal, dn = torch.rand(R, device=dev) + 1.5, torch.empty(R, 3, device=dev), torch.empty(2, device=dev), torch.empty(R, 3, device=dev)
    ids, gt = (ctypes.c_int * 4)(6, 0, 0, 0), (ctypes.c_float * 3)(0.6, 0.0, 0.8)
    a = [L.ptr(t) for t in (normals, label, I["o"], I["d"], depth, fe, scal, d_fe, dn)]
    fwd = timeit(lambda: lib.ncw_ray_floor_fwd(a[0], a[1], ids, 1, gt, a[2], a[3], a[4], R, 1, a[5], a[6], st))
    bwd = timeit(lambda: lib.ncw_ray_floor_bwd(a[0], a[1], ids, 1, gt, R, 1, a[6], a[7], a[8], st))
    return fwd, bwd


def upsample(I, n, n_new):
    z, sdf = I["z"][:, :n].contiguous(), I["sdf"][:, :n].contiguous()
    out = rayops.upsample(I["o"], I["d"], z, sdf, n_new, 64.0)
    return timeit(lambda: lib.ncw_upsample(L.ptr(I["o"]), L.ptr(I["d"]), L.ptr(z), L.ptr(sdf), R, n, 64.0, n_new, L.ptr(out), st))


def merge(I, na, nb, payload):
    a, b = I["z"][:, :na].contiguous(), torch.rand(R, nb, device=dev) * 3 + 1
    pa, pb = (I["sdf"][:, :na].contiguous(), torch.rand(R, nb, device=dev)) if payload else (None, None)
    out, pout = rayops.sort_merge(a, b, pa, pb)
    return timeit(lambda: lib.ncw_sort_merge(L.ptr(a), na, L.ptr(b), nb, L.ptr(pa), L.ptr(pb), R, L.ptr(out), L.ptr(pout), st))


res = {}
I, fwd, bwd = composite(128, 4)
res["composite_fwd_128+4"], res["composite_bwd_128+4"] = fwd, bwd
res["upsample_64"] = upsample(I, 64, 32)
res["upsample_96"] = upsample(I, 96, 32)
res["sort_merge_64+32"] = merge(I, 64, 32, True)
res["sort_merge_96+32"] = merge(I, 96, 32, True)
res["sort_merge_128+4"] = merge(I, 128, 4, False)
I, fwd, bwd = composite(1056, 32)
res["composite_fwd_1056+32"], res["composite_bwd_1056+32"] = fwd, bwd
res["upsample_1023"] = upsample(I, 1023, 128)
res["sort_merge_1056+32"] = merge(I, 1056, 32, False)
if args.floor:
    res["ray_floor_fwd"], res["ray_floor_bwd"] = floor_term(I)
print(json.dumps({"unit": "us per launch, R = 1024", **{k: round(v, 3) for k, v in res.items()}}))
