"""GPU: the two launches of the appearance-code fit (csrc/ncw_appfit.hip) called directly.

`ncw_appfit_loss` against a float64 numpy restatement, held to the per-ray kernels' convention (tests/_ray_cases.py `bound`:
max(floor, 4 x the error of the same expression evaluated in float32 numpy), both errors against float64), and bit for bit
against the compositor's own `color`.  `ncw_appfit_step`: integer-valued rows against an int64 sum bit for bit (also split into
two accumulating calls), run-to-run bitwise, the Adam update against a float64 restatement, and the non-finite guard."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests._ray_cases import FLOOR_ADJ, FLOOR_FWD, bound, comp_case, comp_case_inputs
from tests._util import rel_err

pytestmark = pytest.mark.gpu

BRGB = (0.1, 0.2, 0.3)


def _loss_inputs(R, S, O_, with_bg, with_brgb, pattern, seed):
    """Ray 0 carries ONE non-zero weight (0.5, on sample 0) and the same colour in rgb and bg_rgb there, so its composed colour is
    exact in any summation order: its channel 1 is made the target to hit sign(0)."""
    g = np.random.RandomState(seed)
    M = S + O_ if with_bg else S
    w = (g.rand(R, M) * (g.rand(R, M) < 0.8)).astype(np.float32) / np.float32(M)  # some exact zeros
    if pattern == "all":
        ins = np.ones((R, S), np.float32)
    elif pattern == "none":
        ins = np.zeros((R, S), np.float32)
    else:
        ins = (np.arange(S)[None] + np.arange(R)[:, None]) % 2 == 0
        ins = ins.astype(np.float32)
    rgb = g.rand(R, S, 3).astype(np.float32)
    bg = g.rand(R, M, 3).astype(np.float32) if with_bg else None
    w[0] = 0
    w[0, 0] = 0.5
    rgb[0, 0] = (0.25, 0.5, 0.75)
    if with_bg:
        bg[0, 0] = (0.25, 0.5, 0.75)
    wsum = (w[:, :S] * ins).sum(-1).astype(np.float32)
    target = g.rand(R, 3).astype(np.float32)
    return dict(w=w, ins=ins, wsum=wsum, rgb=rgb, bg=bg, brgb=np.asarray(BRGB, np.float32) if with_brgb else None,
                target=target, S=S, O=O_, M=M, R=R)


def _restate(I, dt, inv_denom, scale):
    w, ins, S, M = I["w"].astype(dt), I["ins"] > 0, I["S"], I["M"]
    sel = np.zeros((I["R"], M), bool)
    sel[:, :S] = ins
    rgb = np.zeros((I["R"], M, 3), dt)
    rgb[:, :S] = I["rgb"].astype(dt)
    other = I["bg"].astype(dt) if I["bg"] is not None else np.zeros((I["R"], M, 3), dt)
    col = np.where(sel[..., None], rgb, other)
    color = (w[..., None] * col).sum(1, dtype=dt)
    if I["brgb"] is not None:
        color = color + I["brgb"].astype(dt)[None] * (dt(1) - I["wsum"].astype(dt))[:, None]
    e = color - I["target"].astype(dt)
    k = np.sign(e) * dt(inv_denom) * dt(scale)
    full = w[..., None] * k[:, None, :]
    return dict(color=color, ray_loss=np.abs(e).sum(-1, dtype=dt), d_rgb=np.where(sel[:, :S, None], full[:, :S], dt(0)),
                d_bg=np.where(sel[..., None], dt(0), full))


def _run_loss(I, inv_denom, scale):
    from neuralrecon_w_amd import lib as L

    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    R, S, M = I["R"], I["S"], I["M"]
    w, ins, wsum, rgb, bg, brgb, target = (t(I[k]) for k in ("w", "ins", "wsum", "rgb", "bg", "brgb", "target"))
    sc = torch.tensor([scale, 1.0 / scale], device="cuda") if scale is not None else None
    color, ray_loss = torch.full((R, 3), np.nan).cuda(), torch.full((R,), np.nan).cuda()
    d_rgb = torch.full((R, S, 3), np.nan).cuda()
    d_bg = torch.full((R, M, 3), np.nan).cuda() if bg is not None else None
    L.check(L.get_lib().ncw_appfit_loss(L.ptr(w), L.ptr(ins), L.ptr(wsum), L.ptr(rgb), L.ptr(bg), L.ptr(brgb), L.ptr(target), R, S,
                                        I["O"], float(inv_denom), L.ptr(sc), L.ptr(color), L.ptr(ray_loss), L.ptr(d_rgb),
                                        L.ptr(d_bg), L.stream_ptr("cuda")), "ncw_appfit_loss")
    torch.cuda.synchronize()
    return dict(color=color.cpu(), ray_loss=ray_loss.cpu(), d_rgb=d_rgb.cpu(), d_bg=None if d_bg is None else d_bg.cpu())


@pytest.mark.parametrize("pattern", ["all", "none", "alt"])
@pytest.mark.parametrize("with_bg,with_brgb", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("S,O_", [(1, 0), (1, 4), (64, 0), (64, 4), (65, 0), (65, 4)])
@pytest.mark.parametrize("R", [1, 5])
def test_appfit_loss_vs_float64(R, S, O_, with_bg, with_brgb, pattern):
    I = _loss_inputs(R, S, O_, with_bg, with_brgb, pattern, seed=100 * S + 10 * O_ + R)
    R_total, scale = 37, 1024.0  # the denominator is the whole fit set's, not the launch's
    inv_denom = 1.0 / (R_total + 1e-5)
    # sign(0): ray 0's colour is exact (one weight of 0.5), so its channel 1 can be made the target
    r32 = _restate(I, np.float32, inv_denom, scale)
    I["target"][0, 1] = r32["color"][0, 1]
    r64, r32 = _restate(I, np.float64, inv_denom, scale), _restate(I, np.float32, inv_denom, scale)
    got = _run_loss(I, inv_denom, scale)
    assert float(got["color"][0, 1]) == float(I["target"][0, 1]), "the sign(0) ray does not hit its target exactly"
    assert torch.all(got["d_rgb"][0, :, 1] == 0)
    if with_bg:
        assert torch.all(got["d_bg"][0, :, 1] == 0)
    for k, floor in (("color", FLOOR_FWD), ("ray_loss", FLOOR_FWD), ("d_rgb", FLOOR_ADJ), ("d_bg", FLOOR_ADJ)):
        if got[k] is None:
            continue
        assert torch.isfinite(got[k]).all(), k
        e32 = rel_err(torch.from_numpy(r32[k]), torch.from_numpy(r64[k]))
        e = rel_err(got[k], torch.from_numpy(r64[k]))
        print("appfit_loss R%d S%d O%d bg%d brgb%d %s %s: kernel %.3g, fp32 restatement %.3g" % (R, S, O_, with_bg, with_brgb,
                                                                                              pattern, k, e, e32))
        assert e <= bound(floor, e32), (k, e, e32)
    # where a sample is inside, only d_rgb carries its adjoint, and the other way round: exact zeros
    ins = torch.from_numpy(I["ins"]) > 0
    assert torch.all(got["d_rgb"][~ins] == 0)
    if with_bg:
        assert torch.all(got["d_bg"][:, :S][ins] == 0)


def test_appfit_loss_without_scale_is_the_scaled_one_divided():
    I = _loss_inputs(5, 65, 4, True, True, "alt", seed=3)
    a, b = _run_loss(I, 0.125, None), _run_loss(I, 0.125, 1024.0)
    assert torch.equal(a["color"], b["color"]) and torch.equal(a["ray_loss"], b["ray_loss"])
    assert torch.equal(a["d_rgb"] * 1024.0, b["d_rgb"]) and torch.equal(a["d_bg"] * 1024.0, b["d_bg"])


@pytest.mark.parametrize("S,O_,with_bg,brgb", [(61, 4, True, True), (64, 0, False, True), (127, 2, True, False), (509, 4, True, True)])
def test_appfit_loss_color_is_the_compositors_bit_for_bit(S, O_, with_bg, brgb):
    """The cached weights / inside / weights_sum of ncw_composite_fwd, the same rgb and bg_rgb: `color` must be the compositor's
    own, bit for bit (same lane-strided order, same wave reduction)."""
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import rayops

    c = comp_case(S, O_, with_bg=with_bg, brgb=brgb)
    I = comp_case_inputs(c)
    cu = lambda x: None if x is None else x.cuda()  # noqa: E731
    comp = rayops.CompositeCtx(cu(I["o"]), cu(I["d"]), cu(I["z"]), cu(I["sample_dist"]), cu(I["sdf"]), cu(I["grad"]), cu(I["rgb"]),
                               cu(I["inv_s"]), c.cos, cu(I["z_feed"]), cu(I["density"]), cu(I["bg_rgb"]), cu(I["background_rgb"]),
                               c.trim)
    o = comp.forward()
    R, M = c.R, S + (O_ if with_bg else 0)
    color, ray_loss = torch.empty(R, 3).cuda(), torch.empty(R).cuda()
    d_rgb, d_bg = torch.empty(R, S, 3).cuda(), (torch.empty(R, M, 3).cuda() if with_bg else None)
    target = torch.rand(R, 3).cuda()
    L.check(L.get_lib().ncw_appfit_loss(L.ptr(o["weights"]), L.ptr(o["inside"]), L.ptr(o["weights_sum"]), L.ptr(comp.t["rgb"]),
                                        L.ptr(comp.t["bg_rgb"]), L.ptr(comp.t["background_rgb"]), L.ptr(target), R, S, O_, 1.0,
                                        None, L.ptr(color), L.ptr(ray_loss), L.ptr(d_rgb), L.ptr(d_bg), L.stream_ptr("cuda")),
            "ncw_appfit_loss")
    same = torch.equal(color, o["color"])
    print("S%d O%d bg%d: colour %s the compositor's (max |diff| %.3g)" % (S, O_, with_bg, "bit for bit" if same else "NOT bitwise",
                                                                        float((color - o["color"]).abs().max())))
    assert same


# ------------------------------------------------------------------------------------------------------------------------
# ncw_appfit_step
# ------------------------------------------------------------------------------------------------------------------------
LR, B1, B2, EPS = 0.05, 0.9, 0.999, 1e-7


class _Step:
    def __init__(self, n_a, R_rows=3, scale=None, code=None):
        self.n_a = n_a
        self.code = (torch.linspace(-1, 1, n_a) if code is None else code).cuda().contiguous()
        self.m, self.v, self.acc = torch.zeros(n_a).cuda(), torch.zeros(n_a).cuda(), torch.full((n_a,), 7.0).cuda()
        self.state = torch.zeros(8, dtype=torch.int32).cuda()
        self.scale = torch.tensor([scale, 1.0 / scale]).cuda() if scale is not None else None
        self.a_rows = torch.full((R_rows, n_a), -5.0).cuda()

    def call(self, rows, accumulate, final):
        from neuralrecon_w_amd import lib as L

        lib = L.get_lib()
        n = 0 if rows is None else rows.shape[0]
        scratch = torch.empty(max(1, int(lib.ncw_appfit_step_scratch_floats(n, self.n_a)))).cuda()
        L.check(lib.ncw_appfit_step(L.ptr(rows), n, self.n_a, L.ptr(scratch), L.ptr(self.acc), int(accumulate), int(final),
                                    L.ptr(self.code), L.ptr(self.m), L.ptr(self.v), L.ptr(self.state), LR, B1, B2, EPS,
                                    L.ptr(self.scale), 1.0, L.ptr(self.a_rows), self.a_rows.shape[0], L.stream_ptr("cuda")),
                "ncw_appfit_step")
        torch.cuda.synchronize()


def _int_rows(n, n_a, seed):
    return torch.randint(-8, 9, (n, n_a), generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("n_a", [1, 48, 69])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_appfit_step_integer_rows_sum_exactly_in_one_call_and_in_two(n, n_a):
    rows = _int_rows(n, n_a, 1000 * n + n_a)
    want = rows.long().sum(0)
    assert int(want.abs().max()) < 2 ** 24
    s = _Step(n_a)
    s.call(rows.cuda(), accumulate=False, final=False)  # accumulate off: the 7.0 the accumulator held is overwritten
    assert torch.equal(s.acc.cpu().long(), want) and torch.equal(s.acc.cpu(), want.float())
    assert int(s.state[0]) == 0 and torch.all(s.a_rows == -5.0)  # not final: no step, no broadcast
    k = n // 2
    t = _Step(n_a)
    t.call(rows[:k].cuda().contiguous() if k else None, accumulate=False, final=False)
    t.call(rows[k:].cuda().contiguous(), accumulate=True, final=False)
    assert torch.equal(t.acc.cpu(), want.float())


def test_appfit_step_float_rows_are_bitwise_reproducible_and_split_independent_at_block_multiples():
    n, n_a = 4097, 48
    rows = torch.randn(n, n_a, generator=torch.Generator().manual_seed(5)).cuda()
    a, b = _Step(n_a), _Step(n_a)
    a.call(rows, False, False)
    b.call(rows, False, False)
    assert torch.equal(a.acc, b.acc)
    ref = rows.double().sum(0)
    # 64 sequential adds in a wave, 2 across the waves, 17 across the blocks: at most 83 roundings of partial sums bounded by sum |x|
    assert rel_err(a.acc.cpu(), ref.cpu()) <= 83 * 2.0 ** -24 * float(rows.abs().sum(0).max() / ref.abs().max())
    c = _Step(n_a)  # a split at a multiple of NCW_APPFIT_BLOCK_ROWS (256) rows: the same block sums, added in the same order
    c.call(rows[:1024].contiguous(), False, False)
    c.call(rows[1024:].contiguous(), True, False)
    assert torch.equal(a.acc, c.acc)


def _adam64(code, grads, lr, b1, b2, eps):
    """torch.optim.Adam (no weight decay, no amsgrad) in float64 on the kernel's own float32 arguments."""
    lr, b1, b2, eps = (float(np.float32(x)) for x in (lr, b1, b2, eps))
    p, m, v = code.astype(np.float64).copy(), 0.0, 0.0
    for t, g in enumerate(grads, 1):
        m = m + (1 - b1) * (g - m)
        v = v * b2 + (1 - b2) * g * g
        p = p - (lr / (1 - b1 ** t)) * (m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps))
    return p


@pytest.mark.parametrize("n_a", [1, 48, 69])
def test_appfit_step_adam_vs_float64_and_broadcast(n_a):
    """Three final calls with integer-valued rows (exact gradient sums; loss scale 8 divided back out exactly).  Tolerance: about ten
    fp32 roundings per step and component, each at most 2^-24 of a quantity bounded by max(1, |code|): 3 x 10 x 6e-8 ~ 2e-6."""
    s = _Step(n_a, R_rows=5, scale=8.0)
    code0 = s.code.cpu().numpy().copy()
    grads = []
    for it in range(3):
        rows = _int_rows(65, n_a, 77 + it) * 8.0
        s.call(rows.cuda(), False, True)
        grads.append(rows.double().sum(0).numpy() / 8.0)
        assert torch.equal(s.a_rows, s.code.reshape(1, n_a).expand(5, n_a))
    want = _adam64(code0, grads, LR, B1, B2, EPS)
    err = float(np.abs(s.code.cpu().numpy().astype(np.float64) - want).max())
    print("adam n_a=%d: max |code - float64| after 3 steps %.3g" % (n_a, err))
    assert err <= 2e-6 * max(1.0, float(np.abs(want).max()))
    assert int(s.state[0]) == 3 and int(s.state[2]) == 0 and float(s.scale[0]) == 8.0
    assert float(np.abs(want - code0).max()) > 0.5 * LR  # the steps moved the code (the first one alone moves a component by lr)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_appfit_step_non_finite_row_skips_the_step_and_halves_the_scale(bad):
    n_a = 48
    s = _Step(n_a, scale=1024.0)
    code0 = s.code.clone()
    rows = _int_rows(65, n_a, 9)
    rows[17, 5] = bad
    s.call(rows.cuda(), False, True)
    assert torch.equal(s.code, code0) and torch.all(s.m == 0) and torch.all(s.v == 0) and torch.all(s.a_rows == -5.0)
    assert int(s.state[0]) == 0 and int(s.state[2]) == 1
    assert float(s.scale[0]) == 512.0 and float(s.scale[1]) == 1.0 / 512.0
    s.call(_int_rows(65, n_a, 10).cuda(), False, True)  # the next, finite, step is applied
    assert int(s.state[0]) == 1 and int(s.state[2]) == 1 and not torch.equal(s.code, code0)


def test_appfit_entry_points_refuse_bad_arguments():
    from neuralrecon_w_amd import lib as L

    lib = L.get_lib()
    x = torch.zeros(8).cuda()
    assert lib.ncw_appfit_step(L.ptr(x), 1, 129, L.ptr(x), L.ptr(x), 0, 0, None, None, None, None, LR, B1, B2, EPS, None, 1.0, None, 0,
                               L.stream_ptr("cuda")) != 0
    assert lib.ncw_appfit_step(None, 1, 4, L.ptr(x), L.ptr(x), 0, 0, None, None, None, None, LR, B1, B2, EPS, None, 1.0, None, 0,
                               L.stream_ptr("cuda")) != 0
    assert lib.ncw_appfit_loss(L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), None, L.ptr(x), 1, 1, 0, 1.0, None, L.ptr(x),
                               L.ptr(x), L.ptr(x), None, L.stream_ptr("cuda")) != 0  # bg_rgb without d_bg_rgb
    assert isinstance(C.c_int64(lib.ncw_appfit_step_scratch_floats(257, 3)).value, int)
    assert lib.ncw_appfit_step_scratch_floats(257, 3) == 6
