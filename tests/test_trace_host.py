"""Sphere tracer without a GPU: the numpy restatement's own conditions (tests/_trace_ref.py), the fixtures of
tests/test_gpu_trace.py inside their caps on the fp64 oracle, and the refusals of the binding and of the entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import _trace_ref as TR
from tests._util import ROOT

NAMES = ["ncw_trace_scratch_bytes", "ncw_trace_begin", "ncw_trace_step", "ncw_trace_finish", "ncw_trace_store"]


def _rays_along_z(xs, z0=2.0):
    """Rays from (x, 0, z0) looking down -z."""
    n = len(xs)
    o = np.stack([np.asarray(xs, dtype=np.float32), np.zeros(n, np.float32), np.full(n, z0, np.float32)], 1)
    d = np.tile(np.array([0, 0, -1], np.float32), (n, 1))
    return o, d


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_on_a_sphere(dtype):
    """A ray at a sphere hits at the analytic depth within eps; a ray past it misses; far <= near is a MISS with 0 evaluations;
    an interval that starts inside is INSIDE with depth near."""
    eps = 1e-3
    o, d = _rays_along_z([0.0, 0.3, 0.8, 0.0, 0.0, 0.0])
    near = np.array([0.2, 0.2, 0.2, 1.0, 1.0, 1.8], dtype)
    far = np.array([4.0, 4.0, 4.0, 1.0, 0.5, 4.0], dtype)
    r = TR.march(o, d, near, far, TR.sphere_sdf(0.5), eps, 1.0, 64, dtype)
    assert r["state"].tolist() == [TR.HIT, TR.HIT, TR.MISS, TR.MISS, TR.MISS, TR.INSIDE]
    assert abs(r["t"][0] - 1.5) <= eps and abs(r["t"][1] - (2.0 - np.sqrt(0.25 - 0.09))) <= eps / 0.8 + 1e-6  # slope 0.8 along the ray
    assert r["iters"][3] == 0 and r["iters"][4] == 0 and r["iters"][5] == 1 and r["t"][5] == near[5]
    assert r["t"].dtype == dtype and r["points"].dtype == dtype
    assert np.array_equal(r["points"], o.astype(dtype) + r["t"][:, None] * d.astype(dtype))
    assert r["lists"][0].tolist() == [0, 1, 2, 5] and all(np.all(np.diff(a) > 0) for a in r["lists"])
    assert r["evaluated"] == int(r["iters"].sum())


def test_restatement_gradient_three_converges_through_the_bracket():
    """An SDF scaled by 3 overshoots with t += s into the sphere, changes sign, and still converges: false position / bisection
    take over.  From further away the first step leaps over the whole sphere (both crossings inside one step: the documented
    limitation); step = 1 / 3 restores a true sphere trace from there."""
    xs = [0.0, 0.2, 0.3]
    o, d = _rays_along_z(xs)
    t_true = 2.0 - np.sqrt(0.25 - np.square(xs))
    near, far = np.full(3, 1.3, np.float32), np.full(3, 9.0, np.float32)
    sdf3 = TR.sphere_sdf(0.5, 3.0)
    r = TR.march(o, d, near, far, sdf3, 1e-3, 1.0, 64)
    assert r["state"].tolist() == [TR.HIT] * 3 and r["iters"].max() < 40 and r["iters"].min() > 2
    assert np.all(np.abs(r["t"] - t_true) <= 1e-3)  # |sdf| <= eps with slope >= 3 * 0.8 along the ray
    first = TR.march(o, d, near, far, sdf3, 1e-3, 1.0, 1)  # one evaluation: where the plain walk lands
    assert np.all(sdf3(first["points"]) < 0)              # inside: the sign changed
    far_start = TR.march(o, d, np.full(3, 0.2, np.float32), far, sdf3, 1e-3, 1.0, 64)
    assert far_start["state"].tolist() == [TR.MISS] * 3   # 3 * 1.3 from z = 1.8 lands behind the sphere
    r3 = TR.march(o, d, np.full(3, 0.2, np.float32), far, sdf3, 1e-3, 1.0 / 3.0, 200)
    assert r3["state"].tolist() == [TR.HIT] * 3 and np.all(np.abs(r3["t"] - t_true) <= 1e-3)


def test_restatement_stalls():
    """A NaN or infinite value is STALLED at once; the cap is STALLED before and after bracketing."""
    o, d = _rays_along_z([0.0, 0.0, 0.0])
    near, far = np.full(3, 0.2, np.float32), np.full(3, 4.0, np.float32)
    vals = {0: np.nan, 1: np.inf, 2: -np.inf}
    r = TR.march(o, d, near, far, lambda p: np.array([vals[i] for i in range(len(p))], np.float32), 1e-3, 1.0, 64)
    assert r["state"].tolist() == [TR.STALLED] * 3 and r["iters"].tolist() == [1, 1, 1]
    o, d = _rays_along_z([0.2])  # off the axis: the SDF is not linear along the ray, false position does not land at once
    for cap in (1, 3):
        r = TR.march(o, d, np.full(1, 1.3, np.float32), far[:1], TR.sphere_sdf(0.5, 3.0), 1e-3, 1.0, cap)
        assert r["state"].tolist() == [TR.STALLED] and r["iters"].tolist() == [cap]


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "D0"])
def test_fixtures_stay_inside_their_caps_on_the_fp64_oracle(name):
    """The view and networks of tests/test_gpu_trace.py, marched in fp64 on the CPU oracle: no STALLED, no INSIDE; the rays left
    out of the depth comparison (grazing, D < 0.2) are at most 10 % of the hit rays; on A (and the spheres D / D0) no MISS ray
    crosses the surface and the silhouette band holds at most 5 % of all rays.  B and C do jump surfaces (|grad| up to 9.6 / 4.5):
    printed, not asserted -- the documented limitation."""
    fx = TR.FIXTURES[name]
    net = TR.mk_net(fx["W"], fx["n_layers"], fx["skip"], jitter=fx["jitter"])
    sdf64, grad64, scale = TR.oracle_of(net, fx["skip"])
    rays = TR.view_rays64()
    eps, delta = 1e-3, (TR.TOL_SPLIT if fx["W"] == 256 else TR.TOL_F32) * scale
    ref = TR.march(rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7], sdf64, eps, 1.0, fx.get("max_iter", 64), np.float64)
    st = TR.fixture_stats(sdf64, grad64, rays, ref, ref, eps, delta)
    print(name, "scale %.3f delta %.2e" % (scale, delta), st, "iters max", int(ref["iters"].max()))
    assert st["n_stalled"] == 0 and st["n_inside"] == 0
    assert st["residual"] <= eps
    assert st["left_out"] <= 0.10 * st["n_hit"]
    if name in ("A", "D", "D0"):
        assert st["crossed"] == 0 and st["band"] <= 0.05 * len(rays)
    if name != "D":
        assert st["n_hit"] >= 19  # the fixtures are not vacuous (D: no surface in front of this camera, see _trace_ref.FIXTURES)


def test_binding_matches_header():
    from neuralrecon_w_amd import lib as L, trace

    assert set(NAMES) <= set(L.exported_symbols()) and L.ABI_VERSION >= 36
    hdr = open(os.path.join(ROOT, "include", "neuconw_hip.h")).read()
    for n in NAMES:
        assert n + "(" in hdr
    for name, val in (("HIT", 1), ("MISS", 2), ("INSIDE", 3), ("STALLED", 4)):  # the ABI's state codes
        assert "#define NCW_TRACE_%s %d" % (name, val) in hdr and getattr(trace, name) == val == getattr(TR, name)
    assert "#define NCW_TRACE_MAX_ITER %d" % trace.MAX_ITER in hdr and "#define NCW_TRACE_REC_WORDS 6" in hdr


def test_entry_points_refuse_bad_arguments_without_a_launch():
    """NULL / misaligned pointers, eps <= 0, step outside (0, 1], max_iter < 1 and counts out of range give NCW_E_BADARG; R == 0,
    m == 0 and n == 0 give 0.  Neither launches, so this runs without a GPU (the pointers are never dereferenced)."""
    from neuralrecon_w_amd import lib as L

    lib = L.get_lib()
    p, q, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(4098)
    bg = (ctypes.c_float * 3)(0, 0, 0)

    def begin(R, x=p):
        return lib.ncw_trace_begin(x, p, p, p, R, p, p, p, p, p, None)

    def step(m, x=p, eps=1e-3, stp=1.0, it=64, R=16, out=q, cnt=q):
        return lib.ncw_trace_step(x, p, p, m, p, p, p, R, eps, stp, it, p, out, cnt, p, p, None)

    def finish(R, x=p):
        return lib.ncw_trace_finish(x, p, p, R, p, p, p, p, None)

    def store(n, x=p, p0=0, npix=16, h=0):
        return lib.ncw_trace_store(x, p, p, p, p, p, h, bg, p0, n, npix, p, p, p, p, p, None)

    for name, fn in (("begin", begin), ("step", step), ("finish", finish), ("store", store)):
        assert fn(0) == 0, name
        assert fn(1, None) == -1 and fn(1, odd) == -1, name
        assert fn(-1) == -1 and fn(1 << 31) == -1, name
    assert step(17) == -1                                         # more listed rays than rays
    for eps in (0.0, -1.0, float("nan")):
        assert step(1, eps=eps) == -1 and step(0, eps=eps) == -1  # refused even for an empty list
    for stp in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert step(1, stp=stp) == -1
    for it in (0, -1, 16384):
        assert step(1, it=it) == -1
    assert step(1, out=p) == -1 and step(1, cnt=p) == -1          # the next list must not alias the current one
    assert store(4, p0=13) == -1 and store(4, p0=-1) == -1 and store(2, h=3) == -1
    assert lib.ncw_trace_scratch_bytes(0) == 4 and lib.ncw_trace_scratch_bytes(257) == 8 and lib.ncw_trace_scratch_bytes(-1) == 0


def test_python_refusals():
    from neuralrecon_w_amd import trace, views
    from neuralrecon_w_amd.lib import NeuconwHipError
    from tests._build import build_system

    _, _, _, rdr = build_system(device="cpu")
    rays = torch.zeros(4, 8)
    with pytest.raises(NeuconwHipError):
        trace.trace_rays(rdr, rays)
    K, c2w, W, H, near, far = TR.view_camera_args()
    with pytest.raises(NeuconwHipError):
        views.trace_view(rdr, views.Camera(K, c2w, W, H, near, far), 0)
    for kw in (dict(eps=0.0), dict(eps=float("nan")), dict(step=0.0), dict(step=1.5), dict(max_iter=0), dict(max_iter=1 << 14),
               dict(sync_every=0)):
        with pytest.raises(ValueError):
            trace.trace_rays(rdr, rays, **kw)


def _script(name):
    import importlib.util

    spec = importlib.util.spec_from_file_location("_script_" + name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_line_arguments():
    """--surface is opt-in: without it the parsed arguments of render_view.py are what they were."""
    rv = _script("render_view").build_parser()
    a = rv.parse_args(["--cfg_path", "c", "--ckpt_path", "k"])
    assert a.surface is False and (a.trace_eps, a.trace_iters, a.trace_step) == (1e-3, 64, 1.0)
    a = rv.parse_args(["--cfg_path", "c", "--ckpt_path", "k", "--surface", "--trace_eps", "2e-3", "--trace_iters", "96", "--trace_step", "0.5"])
    assert a.surface is True and (a.trace_eps, a.trace_iters, a.trace_step) == (2e-3, 96, 0.5)
    bt = _script("bench_trace").build_parser().parse_args([])
    assert (bt.width, bt.height, bt.repeats, bt.sync_every, bt.ab_parent) == (1024, 768, 7, "1,4,16", None)
