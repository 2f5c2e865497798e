"""GPU: NeuconWRenderer.render(), _RenderFn.backward and TrainStep across the renderer's option branches (tests/_render_options.py:
background off, trim_sphere off, 1 / 4 up-sampling steps, s_val_base 0, no importance samples, 8 / 32 outside samples, no mask list, no
depth loss, another scene frame, config/defaults.py's combination) -- the composed code above the per-point and per-ray kernels, which the
other composed tests run in ONE configuration.  W = 64 networks, 48 rays, 16 + 16 samples.

a. every case, fp32 mode, against the fp64 oracle: outputs and the eikonal term 1e-4, parameter gradients 2e-3 of their network's largest
   gradient, loss 1e-4 -- the project's fp32 bounds (tests/test_gpu_fullsize.py); tests/test_render_options_host.py shows the reference's own
   fp32 arithmetic a factor two or more inside them on these inputs.
b. exact invariances in f32 / f16 / bf16 (torch.equal on every entry of render()'s dictionary; parameter gradients bitwise in the
   order-fixed f32 mode, within twice the reference's own f32 reordering spread in the 16-bit modes, whose d_a / weight gradients are f32
   atomics).
c. the 16-bit modes against the fp32 oracle where the launch structure changes (no background, no dead-background elimination), at the
   shapes and with the bounds of test_train_step_vs_oracle_real_widths.
d. TrainStep (flat parameters, adopted gradient buffer, capture and replay) in those configurations.

MEASURED on MI355X (printed by the tests):
a. fp32 mode against the fp64 oracle: worst output (entry) / worst gradient (tensor); the loss agrees to 1e-6 in every case
     base, n_out8, trim_off 6.3e-6 (mask_error) / 2.0e-5 (sdf_net.lin4.weight_v)     no_bg, n_out0 6.3e-6 (mask_error) / 2.1e-5 (lin4.weight_v)
     steps1 5.0e-6 (mask_error) / 1.3e-5 (lin4.weight_v)       steps4 1.1e-5 (depth) / 2.2e-5 (lin4.weight_v)
     sbase0 1.7e-5 (depth) / 4.0e-4 (lin4.weight_v)            no_imp 2.4e-6 (mask_error) / 9.2e-6 (lin4.weight_v)
     no_mask 1.8e-6 (depth) / 4.4e-6 (variance)                no_depth 6.3e-6 (mask_error) / 2.85e-5 (lin4.weight_v)
     no_mask_no_depth 1.8e-6 (depth) / 1.2e-5 (variance)       defaults_like 1.6e-5 (gradient_error) / 3.0e-4 (sdf_net.lin0.weight_v)
     moved 6.3e-6 (mask_error) / 2.0e-5 (lin4.weight_v)
   -- the reference's own fp32 floor case by case (tests/test_render_options_host.py: sbase0 1.7e-5 / 4.1e-4, defaults_like 1.6e-5 / 3.0e-4).
b. every invariance bitwise in the outputs (three precisions) and in the f32 gradients; 16-bit gradients of the two runs 4.5e-8 .. 1.4e-7 of
   the network's largest gradient apart (sdf_net.lin4.weight_v, lin5.bias, lin6.bias), one stream against two included, bound 7.0e-7;
   colour(0.25) - colour(None) against the oracle's 0.25 (1 - weights_sum), f32 only: 3.8e-7 (16-bit modes: against the run's own weights_sum).
c. W = 256, 16 + 16, R = 40 (colour / depth / weights_sum / eikonal; loss difference; worst gradient; set-aside embedding row):
     no_bg    f16  1.3e-5 / 2.3e-5 / 2.4e-5 / 2.4e-5; 2e-6; 1.6e-3 (embedding_a.weight); 8.8e-3
     no_bg    bf16 1.2e-3 / 2.3e-3 / 2.3e-3 / 2.4e-3; 1e-5; 5.3e-2 (sdf_net.lin4.weight_v); 5.2e-2
     trim_off f16  3.0e-5 / 2.3e-5 / 2.4e-5 / 2.4e-5; <1e-6; 6.2e-4 (embedding_a.weight); 1.3e-3
     trim_off bf16 1.3e-3 / 2.3e-3 / 2.3e-3 / 2.4e-3; 1.8e-5; 4.3e-2 (sdf_net.lin4.weight_v); 8.0e-2
   against F16_TOL (8e-5, 8e-3, 1e-4), BF16_TOL (1e-2, 0.175, 1e-2), LOSS_TOL 5e-5 / 1.4e-3, set-aside row 0.15 / 0.16.
d. TrainStep against the per-tensor recipe: parameters after step 1 3e-8 .. 1.2e-7, after four steps max 1.5e-5 (no_bg), 1.2e-6 (trim_off),
   2.4e-7 (no_mask_no_depth), 4.3e-6 (defaults_like), median 0, nothing above 2e-5.  Replay against eager: f32 bitwise (losses and parameters);
   two free f16 runs do not hold that test's bounds against each other, eager or replayed (test_captured_step_replays_like_eager has the
   figures), so f16 is compared step by step from equal state (no_bg, trim_off, base): loss difference 0 in f32 and f16, parameters bitwise
   in f32, 7.5e-8 .. 6.0e-7 apart in f16.
Each of these Python-only changes of renderer.py fails tests here: `True` for rdr.trim_sphere into CompositeCtx (a. trim_off: color_bg);
`s_val_base` for `s_val_base + i` in sparse_sampler (a. in 12 cases, b. single stream f32, c. f16); no plans.append(nctx["plan"]) in the
single-stream backward (a. in every case with a background, b. single stream in all three precisions, d. per-tensor recipe).
"""
from types import SimpleNamespace

import pytest
import torch

from tests import _render_options as RO
from tests._build import named_params
from tests._util import rel_err

pytestmark = pytest.mark.gpu

TOL_OUT, TOL_GRAD, TOL_LOSS = 1e-4, 2e-3, 1e-4  # tests/test_gpu_fullsize.py: fp32, W = 256 row
PRECS = ["f32", "f16", "bf16"]
OUT_KEYS = ("color", "depth", "weights_sum", "gradient_error", "color_bg", "mask_error")


def _prec(name):
    import neuralrecon_w_amd as nw

    return {"f32": nw.PREC_F32, "bf16": nw.PREC_BF16, "f16": nw.PREC_F16}[name]


def _run(case, prec_name, inp=None, background="given", loss_case=None, W=64, backward=True, **attrs):
    """One composed step of `case`: render(perturb_overwrite=0, cos_anneal_ratio=0.3) + NeuconWLoss of `loss_case` (default: the case's
    own terms) + backward.  attrs: renderer attributes set before the first render (use_bg_stream)."""
    import neuralrecon_w_amd as nw

    emb, neuconw, nerf, rdr = RO.system(case, prec=_prec(prec_name), W=W)
    for k, v in attrs.items():
        assert hasattr(rdr, k), k
        setattr(rdr, k, v)
    inp = RO.inputs(case=case) if inp is None else inp
    bg = inp["background_rgb"] if isinstance(background, str) else background
    out = rdr.render(inp["rays"].cuda(), inp["ts"].cuda(), inp["label"].cuda(), perturb_overwrite=0,
                     background_rgb=None if bg is None else bg.cuda(), cos_anneal_ratio=RO.COS_ANNEAL)
    loss = nw.NeuconWLoss(**RO.loss_kw(loss_case or case))(out, inp["rgbs"].cuda())
    grads = None
    if backward:
        loss.backward()
        grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in named_params(emb, neuconw, nerf).items()}
    torch.cuda.synchronize()
    return SimpleNamespace(out={k: v.detach() for k, v in out.items()}, loss=float(loss.detach()), grads=grads, rdr=rdr)


def _score_grads(grads, ref, exact):
    """-> (worst error over the network's largest reference gradient, its tensor, {tensor: error}, set-aside embedding row)."""
    from tests._parity import embedding_grad_err

    errs, flip = {}, 0.0
    for k, g in ref["grads"].items():
        if g is None:
            continue
        s = ref["scale"][RO.net_of(k)]
        if k == "embedding_a.weight":
            errs[k], flip = embedding_grad_err(grads[k].cpu(), g, s, exact=exact)
        else:
            errs[k] = float((grads[k].cpu().double() - g.double()).abs().max()) / s
    name = max(errs, key=errs.get)
    return errs[name], name, errs, flip


def _check_grad_pattern(grads, ref):
    for k, g in ref["grads"].items():
        if g is None:  # took no part: no gradient, or the exact zeros of a parameter that is in ctx.params all the same
            assert grads[k] is None or not bool(grads[k].any()), k
        else:
            assert grads[k] is not None and bool(torch.isfinite(grads[k]).all()), k


# ---- a. every case against the fp64 oracle, fp32 mode ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(RO.CASES))
def test_step_vs_oracle_fp32(case):
    o = RO.options(case)
    ref = RO.oracle(case)
    run = _run(case, "f32")
    out = run.out
    n_bg = o["n_outside"] if RO.has_bg(case) else 0
    assert out["weights"].shape == (RO.R, o["n_samples"] + o["n_importance"] + n_bg)
    assert out["weights"].shape == ref["out"]["weights"].shape
    if o["mesh_mask_list"] is None:
        assert out["mask_error"].shape == (RO.R, 1) and not bool(out["mask_error"].any())
    if not o["depth_loss"]:
        assert out["sfm_depth_loss"].shape == (RO.R,) and not bool(out["sfm_depth_loss"].any())
    assert out["sfm_depth_loss"].shape == ref["out"]["sfm_depth_loss"].shape  # the reference's selected rows (sync_free off)
    errs = {k: rel_err(out[k].cpu(), ref["out"][k]) for k in OUT_KEYS}
    worst, name, gerrs, _ = _score_grads(run.grads, ref, exact=True)
    k_out = max(errs, key=errs.get)
    print("%-17s f32: worst output %.2e (%s), worst gradient %.2e (%s), loss %.6f vs %.6f; [unbounded: weights %.2e, sfm_depth_loss %.2e]"
          % (case, errs[k_out], k_out, worst, name, run.loss, ref["loss"], rel_err(out["weights"].cpu(), ref["out"]["weights"]),
             rel_err(out["sfm_depth_loss"].cpu(), ref["out"]["sfm_depth_loss"])))
    for k, e in errs.items():
        assert e < TOL_OUT, (k, e)
    assert abs(run.loss - ref["loss"]) < TOL_LOSS
    _check_grad_pattern(run.grads, ref)
    for k, e in gerrs.items():
        assert e < TOL_GRAD, (k, e)


# ---- b. exact invariances -----------------------------------------------------------------------------------------------------------
_SPREAD = {}


def _spread_bound(case):
    """Twice the spread of the reference's own f32 gradient sums under reordering (the margin tests/test_gpu_color_edges.py gives an
    accumulation order), measured on the CPU: 3.5e-7 of the network's largest gradient for base and trim_off -> 7.0e-7; the two
    stream orders of the 16-bit modes measure 4.5e-8 .. 1.4e-7 on MI355X."""
    key = "trim_off" if case == "trim_off" else "base"
    if key not in _SPREAD:
        _SPREAD[key] = RO.reorder_spread(key)
        print("reordering spread of the fp32 oracle's gradients (%s): %.2e" % (key, _SPREAD[key]))
    return 2.0 * _SPREAD[key]


def _assert_same(a, b, prec_name, case, what, skip=()):
    """Every entry of render()'s dictionary bitwise; gradients bitwise in f32, within the reordering bound in the 16-bit modes."""
    assert a.out.keys() == b.out.keys()
    for k in a.out:
        if k not in skip:
            assert a.out[k].shape == b.out[k].shape and torch.equal(a.out[k], b.out[k]), (what, prec_name, k)
    if a.grads is None:
        return
    scale, worst = RO.oracle(case)["scale"], (0.0, "")
    for k, g in a.grads.items():
        assert (g is None) == (b.grads[k] is None), (what, k)
        if g is None:
            continue
        if prec_name == "f32":
            assert torch.equal(g, b.grads[k]), (what, prec_name, k)
        else:
            e = float((g.double() - b.grads[k].double()).abs().max()) / scale.get(RO.net_of(k), 1.0)
            worst = max(worst, (e, k))
    if prec_name != "f32":
        bound = _spread_bound(case)
        print("%s, %s: worst gradient difference %.2e (%s), bound %.2e" % (what, prec_name, worst[0], worst[1], bound))
        assert worst[0] <= bound, (what, prec_name, worst, bound)


@pytest.mark.parametrize("prec_name", PRECS)
def test_n_outside_0_is_render_bg_off(prec_name):
    a, b = _run("n_out0", prec_name), _run("no_bg", prec_name)
    assert a.out["weights"].shape == (RO.R, 32) and not bool(a.out["color_bg"].any())
    _assert_same(a, b, prec_name, "no_bg", "n_out0 == no_bg")


@pytest.mark.parametrize("prec_name", PRECS)
@pytest.mark.parametrize("case,entry", [("no_mask", "mask_error"), ("no_depth", "sfm_depth_loss")])
def test_mask_and_depth_options_touch_their_entry_only(case, entry, prec_name):
    """The loss of both runs is the CASE's (without the term): the option-off renderer and the base renderer whose entry the loss does not
    read must hand back the same gradients."""
    a, b = _run(case, prec_name), _run("base", prec_name, loss_case=case)
    assert not torch.equal(a.out[entry], b.out[entry]) and not bool(a.out[entry].any()) and bool(b.out[entry].any())
    _assert_same(a, b, prec_name, "base", "%s == base but %s" % (case, entry), skip=(entry,))


@pytest.mark.parametrize("prec_name", PRECS)
def test_8_column_rays_are_10_column_rays_without_depth_weight(prec_name):
    inp = RO.inputs()
    r10 = inp["rays"].clone()
    r10[:, 9] = 0.0
    a = _run("base", prec_name, inp=dict(inp, rays=inp["rays"][:, :8].contiguous()))
    b = _run("base", prec_name, inp=dict(inp, rays=r10))
    assert a.out["sfm_depth_loss"].shape == (RO.R,) and not bool(a.out["sfm_depth_loss"].any())
    _assert_same(a, b, prec_name, "base", "8 columns == 10 columns, depth_weight 0")


@pytest.mark.parametrize("prec_name", PRECS)
def test_moved_scene_frame_is_the_base_render(prec_name):
    """Ray origins on multiples of 2^-10: (o * 2 + origin - origin) / 2 is exact in fp32, the normalised rays are bitwise the base ones."""
    ia, ib = RO.inputs(case="moved", quantise=True), RO.inputs(quantise=True)
    assert not torch.equal(ia["rays"], ib["rays"])
    a, b = _run("moved", prec_name, inp=ia), _run("base", prec_name, inp=ib)
    for x, y, n in zip(a.rdr.ray_prologue(ia["rays"].cuda()), b.rdr.ray_prologue(ib["rays"].cuda()),
                       ("rays_o", "rays_d", "near", "far", "depth_gt", "depth_weight")):
        assert torch.equal(x, y), "ray_prologue: " + n
    _assert_same(a, b, prec_name, "base", "moved == base")


@pytest.mark.parametrize("prec_name", PRECS)
@pytest.mark.parametrize("case", ["base", "trim_off"])
def test_single_stream_is_the_two_stream_step(case, prec_name):
    """use_bg_stream=False: the background NeRF on the main stream, forward and backward -- in the 16-bit modes the ONLY run of the
    single-stream backward with f32 atomics into the colour network's d_a (in f32 the order-fixed branch runs on one stream either way)."""
    a, b = _run(case, prec_name, use_bg_stream=False), _run(case, prec_name, use_bg_stream=True)
    assert a.rdr.__dict__.get("_bg_streams") is None and b.rdr.__dict__.get("_bg_streams")  # the side stream was (not) used
    assert bool(a.grads["nerf.rgb_linear.weight"].any()) and bool(a.grads["embedding_a.weight"].any())
    _assert_same(a, b, prec_name, case, "%s: one stream == two streams" % case)
    # ... and the gradients of the single-stream step are the oracle's (a plan missing from the weight-norm backward leaves zeros)
    if prec_name == "f32":
        worst, name, _, _ = _score_grads(a.grads, RO.oracle(case), exact=True)
        assert worst < TOL_GRAD, (name, worst)
    else:
        for k, g in RO.oracle(case)["grads"].items():
            if g is not None and k.startswith("nerf.") and bool(g.any()):
                assert bool(a.grads[k].any()), k


@pytest.mark.parametrize("prec_name", PRECS)
def test_background_rgb_none_is_zero_and_adds_its_share(prec_name):
    """In every precision the colour moves by 0.25 (1 - weights_sum) of the run's OWN weights_sum to 1e-6 (the compositor is f32 in all three);
    against the ORACLE's weights_sum in f32 only -- a 16-bit mode's weights_sum is itself further than 1e-6 from the oracle's."""
    inp = RO.inputs()
    none = _run("base", prec_name, background=None, backward=False)
    zero = _run("base", prec_name, background=torch.zeros(1, 3), backward=False)
    quarter = _run("base", prec_name, backward=False)
    _assert_same(none, zero, prec_name, "base", "background_rgb None == zeros")
    for k in quarter.out:  # the colour moves, nothing else does
        assert torch.equal(quarter.out[k], none.out[k]) == (k != "color"), k
    d = (quarter.out["color"] - none.out["color"]).cpu().double()
    own = float((d - 0.25 * (1.0 - none.out["weights_sum"].cpu().double())).abs().max())
    assert float(inp["background_rgb"][0, 0]) == 0.25 and own < 1e-6, own
    if prec_name == "f32":  # renderer.py:753-754 with the ORACLE's weights_sum
        e = float((d - 0.25 * (1.0 - RO.oracle("base")["out"]["weights_sum"])).abs().max())
        print("colour(0.25) - colour(None) against the oracle's 0.25 (1 - weights_sum): %.2e" % e)
        assert e < 1e-6, e


# ---- c. 16-bit modes where the launch structure changes ---------------------------------------------------------------------------
@pytest.mark.parametrize("prec_name", ["f16", "bf16"])
@pytest.mark.parametrize("case", ["no_bg", "trim_off"])
def test_16_bit_step_vs_oracle_real_widths(case, prec_name):
    """W = 256, 16 + 16 samples, R = 40, fp32 oracle, and the bounds of test_train_step_vs_oracle_real_widths itself (measured there on
    the base configuration: outputs / gradients 3.2e-5 / 3.7e-3 in f16, 2.6e-3 / 8.7e-2 in bf16)."""
    from tests._parity import FLIP_ROW_TOL, FLIP_ROW_TOL_BF16, is_relu_tensor, relu_tol
    from tests.test_gpu_fullsize import BF16_TOL, F16_TOL, LOSS_TOL

    W, R = 256, 40
    tol_out, tol_grad, tol_eik = (F16_TOL if prec_name == "f16" else BF16_TOL)[(16, 16)]
    ref = RO.oracle(case, torch.float32, W=W, R=R)
    run = _run(case, prec_name, inp=RO.inputs(R, case), W=W)
    errs = {k: rel_err(run.out[k].cpu(), ref["out"][k]) for k in ("color", "depth", "weights_sum", "gradient_error")}
    worst, name, gerrs, flip = _score_grads(run.grads, ref, exact=False)
    print("%s W=256 16+16 %s:" % (case, prec_name), {k: "%.2e" % v for k, v in errs.items()},
          "loss %.6f vs %.6f, worst gradient %.2e (%s), set-aside embedding row %.2e" % (run.loss, ref["loss"], worst, name, flip))
    for k, e in errs.items():
        assert e < (tol_eik if k == "gradient_error" else tol_out), (k, e)
    assert abs(run.loss - ref["loss"]) < LOSS_TOL[prec_name]
    _check_grad_pattern(run.grads, ref)
    assert flip < (FLIP_ROW_TOL_BF16 if prec_name == "bf16" else FLIP_ROW_TOL), flip
    for k, e in gerrs.items():
        assert e < (relu_tol(False, tol_grad) if is_relu_tensor(k) else tol_grad), (k, e)


# ---- d. the train step ------------------------------------------------------------------------------------------------------------
def _batch(case):
    inp = RO.inputs(case=case)
    return [inp[k].cuda() for k in ("rays", "ts", "label", "rgbs")], inp["background_rgb"].cuda()


@pytest.mark.parametrize("case", ["no_bg", "trim_off", "no_mask_no_depth", "defaults_like"])
def test_train_step_matches_per_tensor_recipe(case):
    """tests/test_gpu_trainer.py::test_train_step_matches_per_tensor_recipe (its steps, its bounds) in the option cases."""
    import neuralrecon_w_amd as nw

    steps = 4
    (rays, ts, label, rgbs), bg = _batch(case)
    loss_fn = nw.NeuconWLoss(**RO.loss_kw(case))
    emb, neuconw, nerf, rdr = RO.system(case, prec=nw.PREC_F32)
    params = [p for m in (emb, neuconw, nerf) for p in m.parameters()]
    opt = torch.optim.Adam(params, lr=1e-3, eps=1e-7)
    losses_a, first_a = [], None
    for i in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(rdr.render(rays, ts, label, perturb_overwrite=0, background_rgb=bg, cos_anneal_ratio=0.1 * i), rgbs)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 0.99)
        opt.step()
        losses_a.append(float(loss))
        if i == 0:
            first_a = {k: p.detach().clone() for k, p in named_params(emb, neuconw, nerf).items()}
    emb2, neuconw2, nerf2, rdr2 = RO.system(case, prec=nw.PREC_F32)
    nerf0 = {k: p.detach().clone() for k, p in nerf2.named_parameters()}
    train = nw.TrainStep(rdr2, [emb2, neuconw2, nerf2], loss_fn, lr=1e-3, eps=1e-7, clip=0.99)
    losses_b, first_b = [], None
    for i in range(steps):
        loss, _ = train(rays, ts, label, rgbs, background_rgb=bg, cos_anneal_ratio=0.1 * i, perturb_overwrite=0)
        losses_b.append(float(loss))
        if i == 0:
            first_b = {k: p.detach().clone() for k, p in named_params(emb2, neuconw2, nerf2).items()}
    assert rdr2.flat_grad_buffer().data_ptr() == train.fp.flat_grad.data_ptr()
    assert train.opt.step_count == steps
    for a, b in zip(losses_a, losses_b):
        assert abs(a - b) <= 2e-5 * max(1.0, abs(a)), (losses_a, losses_b)
    assert losses_a[0] != losses_a[-1]
    worst1 = max(float((first_a[k] - first_b[k]).abs().max()) for k in first_a)
    pa, pb = named_params(emb, neuconw, nerf), named_params(emb2, neuconw2, nerf2)
    diffs = torch.cat([(pa[k] - pb[k]).abs().reshape(-1) for k in pa])
    print("%s: step 1 parameters %.2e; after %d steps max %.2e, median %.2e, share above 2e-5 %.2e"
          % (case, worst1, steps, float(diffs.max()), float(diffs.median()), float((diffs > 2e-5).float().mean())))
    assert worst1 < 2e-6, worst1
    assert float(diffs.max()) < 1e-3, float(diffs.max())
    assert float(diffs.median()) < 2e-6, float(diffs.median())
    assert float((diffs > 2e-5).float().mean()) < 2e-3, float((diffs > 2e-5).float().mean())
    moved = {k: not torch.equal(p.detach(), nerf0[k]) for k, p in nerf2.named_parameters()}
    if RO.has_bg(case):
        assert moved["rgb_linear.weight"] and moved["pts_linears.0.weight"]
    else:  # no background: a zero gradient is a zero Adam update -- in the flat step and in the stock one
        assert not any(moved.values()), [k for k, v in moved.items() if v]
        assert all(torch.equal(p.detach(), nerf0[k]) for k, p in nerf.named_parameters())


@pytest.mark.parametrize("case", ["no_bg", "trim_off"])
def test_captured_step_replays_like_eager(case, prec_name="f32"):
    """tests/test_gpu_trainer.py::test_captured_step_replays_like_eager (its bounds) in the option cases, two eager steps then replays,
    both runs free: in the order-fixed f32 mode they are bitwise equal, losses and parameters.

    f32 ONLY.  Two free runs of four f16 steps do not hold these bounds against EACH OTHER, replay or not, in any configuration measured on
    MI355X: the f32 atomics of the weight gradients re-draw the sign of ~0 gradients, Adam turns each into a +-lr step, and
      W = 64 (plain-fp16 sampler): parameters 4e-6 apart after three steps move 8 % of the f16 sampler's depths by up to 6.8e-2 (the f32
        sampler: 4e-5) and the step-4 loss by 3e-5 .. 2.0e-4 (bound 2e-5) -- eager against eager 0.911473 / 0.911296, trim_off and base alike;
        the f16 forward is a fixed function of the parameters (three evaluations: equal to the last digit), the f32 forward at either
        parameter set gives 0.911289 / 0.911290;
      W = 256 (split-precision SDF value path), 5 eager + 3 replayed runs, all pairs: loss 2.0e-5 (no_bg) / 5.5e-6 (trim_off) / 5.8e-6 (base),
        largest parameter difference 1.4e-3 / 9.7e-4 / 2.3e-3 (bound 1e-3), share above 1e-4 at most 4.4e-4.
    A comparison of two such runs is red or green by chance and says nothing about the replay; what a replayed f16 step computes is held to
    the same bounds, at every one of the four steps, from EQUAL state in test_captured_step_matches_eager_step_from_equal_state."""
    import neuralrecon_w_amd as nw

    steps = 4
    (rays, ts, label, rgbs), bg = _batch(case)
    loss_fn = nw.NeuconWLoss(**RO.loss_kw(case))
    runs = []
    for capture in (False, True):
        emb, neuconw, nerf, rdr = RO.system(case, prec=_prec(prec_name))
        rdr.sync_free = True
        train = nw.TrainStep(rdr, [emb, neuconw, nerf], loss_fn, lr=1e-3, eps=1e-7, clip=0.99, capture=capture, capture_warmup=2)
        losses = []
        for i in range(steps):
            loss, out = train(rays, ts, label, rgbs, background_rgb=bg, cos_anneal_ratio=0.15 * i, perturb_overwrite=0)
            losses.append(float(loss))
            assert train.opt.step_count == i + 1  # advanced once per call, eager or replayed
        assert (train._graphs is not None) == capture
        assert train.native and train.opt.skipped_steps == 0
        runs.append((losses, named_params(emb, neuconw, nerf), float(out["color"].abs().sum())))
    (la, pa, ca), (lb, pb, cb) = runs
    diffs = torch.cat([(pa[k] - pb[k]).abs().reshape(-1) for k in pa])
    print("%s %s: losses %s vs %s; parameters max %.2e, median %.2e, share above 1e-4 %.2e"
          % (case, prec_name, ["%.6f" % v for v in la], ["%.6f" % v for v in lb], float(diffs.max()), float(diffs.median()),
             float((diffs > 1e-4).float().mean())))
    for a, b in zip(la, lb):
        assert abs(a - b) <= 2e-5 * max(1.0, abs(a)), (la, lb)
    assert la[0] != la[-1]
    assert float(diffs.max()) < 1e-3, float(diffs.max())
    assert float(diffs.median()) < 5e-6, float(diffs.median())
    assert float((diffs > 1e-4).float().mean()) < 2e-3, float((diffs > 1e-4).float().mean())
    assert abs(ca - cb) <= 1e-4 * max(1.0, abs(ca))


@pytest.mark.parametrize("prec_name", ["f32", "f16"])
@pytest.mark.parametrize("case", ["no_bg", "trim_off", "base"])
def test_captured_step_matches_eager_step_from_equal_state(case, prec_name):
    """What ONE replayed step computes, without three steps of Adam between the comparison and its cause: before every call the eager
    twin takes over the captured trainer's parameters, Adam moments, step state and loss scale, then both take the step (capture_warmup 2,
    four steps: two eager, the capture, one more replay).  The forward is a fixed function of the parameters in every precision, so the
    losses agree to the bound of the free-running test at EVERY step, f16 included; the updated parameters differ by the weight-gradient
    atomics' order through ONE Adam step and are held to that test's parameter bounds after every step.  Adam's step counter advances once
    per call and no f16 step is skipped."""
    import neuralrecon_w_amd as nw

    steps = 4
    (rays, ts, label, rgbs), bg = _batch(case)
    loss_fn = nw.NeuconWLoss(**RO.loss_kw(case))
    pair = []
    for capture in (False, True):
        emb, neuconw, nerf, rdr = RO.system(case, prec=_prec(prec_name))
        rdr.sync_free = True
        pair.append((nw.TrainStep(rdr, [emb, neuconw, nerf], loss_fn, lr=1e-3, eps=1e-7, clip=0.99, capture=capture, capture_warmup=2), rdr))
    (eager, rdr_e), (cap, rdr_c) = pair
    assert eager.fp.flat.numel() == cap.fp.flat.numel()
    dev = cap.fp.flat.device
    scale_ptrs = (rdr_e.loss_scale.tensor(dev).data_ptr(), rdr_c.loss_scale.tensor(dev).data_ptr())
    worst_loss = worst_max = worst_share = 0.0
    for i in range(steps):
        with torch.no_grad():
            eager.fp.flat.data.copy_(cap.fp.flat.data)
            eager.opt.exp_avg.copy_(cap.opt.exp_avg)
            eager.opt.exp_avg_sq.copy_(cap.opt.exp_avg_sq)
            eager.opt.state.copy_(cap.opt.state)
            # (the device WITH its index: LossScale.tensor() replaces its buffer when the device it is asked for differs from the buffer's,
            # and the optimiser and the captured graph hold the buffer's address)
            rdr_e.loss_scale.tensor(dev).copy_(rdr_c.loss_scale.tensor(dev))
        eager.fp.mark_updated()
        # only the number is kept: an eager step's autograd graph must not be alive when the other trainer captures (trainer.TrainStep)
        la = float(eager(rays, ts, label, rgbs, background_rgb=bg, cos_anneal_ratio=0.15 * i, perturb_overwrite=0)[0].detach())
        lb = float(cap(rays, ts, label, rgbs, background_rgb=bg, cos_anneal_ratio=0.15 * i, perturb_overwrite=0)[0].detach())
        d = (eager.fp.flat.detach() - cap.fp.flat.detach()).abs()
        worst_loss, worst_max = max(worst_loss, abs(la - lb)), max(worst_max, float(d.max()))
        worst_share = max(worst_share, float((d > 1e-4).float().mean()))
        assert abs(la - lb) <= 2e-5 * max(1.0, abs(la)), (i, la, lb)
        assert float(d.max()) < 1e-3 and float(d.median()) < 5e-6 and float((d > 1e-4).float().mean()) < 2e-3, (i, float(d.max()))
        assert eager.opt.step_count == cap.opt.step_count == i + 1
    assert cap._graphs is not None and eager._graphs is None
    assert scale_ptrs == (rdr_e.loss_scale.tensor(dev).data_ptr(), rdr_c.loss_scale.tensor(dev).data_ptr())
    assert cap.opt.skipped_steps == 0 and eager.opt.skipped_steps == 0
    print("%s %s, step by step from equal state: loss difference %.2e, parameters max %.2e, share above 1e-4 %.2e"
          % (case, prec_name, worst_loss, worst_max, worst_share))


# ---- host-side bookkeeping around the step: the sampler's sample count, the loss scale's device buffer ------------------------------------
def test_sampler_reports_the_samples_it_returns():
    """n_importance = 16 in 3 steps adds 3 x 5 samples: sparse_sampler's first return is z's width (it said n_samples + n_importance)."""
    import neuralrecon_w_amd as nw

    emb, neuconw, nerf, rdr = RO.system("base", prec=nw.PREC_F32, up_sample_steps=3)
    inp = RO.inputs()
    rays_o, rays_d, near, far, _, _ = rdr.ray_prologue(inp["rays"].cuda())
    n, z, z_out, _ = rdr.sparse_sampler(rays_o, rays_d, near, far, 0)
    assert n == z.shape[1] == 16 + 3 * 5 and z_out.shape == (RO.R, 4)
    assert bool((z[:, 1:] >= z[:, :-1]).all())
    out = rdr.render(inp["rays"].cuda(), inp["ts"].cuda(), inp["label"].cuda(), perturb_overwrite=0, background_rgb=inp["background_rgb"].cuda())
    assert out["weights"].shape == (RO.R, 31 + 4) and bool(torch.isfinite(out["color"]).all())
    for steps, width in ((1, 32), (2, 32), (4, 32)):
        rdr.up_sample_steps = steps
        n, z, _, _ = rdr.sparse_sampler(rays_o, rays_d, near, far, 0)
        assert n == z.shape[1] == width, (steps, n, z.shape)


def test_loss_scale_buffer_has_one_address_per_device():
    """The optimiser and a captured graph hold the ADDRESS of the loss-scale buffer: "cuda", "cuda:0" and the indexed torch.device name the
    same buffer (the renderer and the trainer pass indexed devices; device("cuda") != device("cuda:0") must not make a second one)."""
    import neuralrecon_w_amd as nw

    *_, rdr = RO.system("base", prec=nw.PREC_F16)
    dev = torch.device("cuda", torch.cuda.current_device())
    t = rdr.loss_scale.tensor(dev)
    assert rdr.loss_scale.tensor("cuda").data_ptr() == t.data_ptr() == rdr.loss_scale.tensor(str(dev)).data_ptr()
    rdr.grad_scale = 256.0
    assert rdr.loss_scale.tensor("cuda").tolist() == [256.0, 1.0 / 256.0] and rdr.grad_scale == 256.0
