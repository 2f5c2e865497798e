"""CPU: the case table of tests/_render_options.py does what tests/test_gpu_render_options.py needs of it -- with the oracle alone.

Every case populates both sides of every per-ray branch (sky / not sky, depth weight / none, inside / outside the sphere), differs
from `base` where its option should show, and the reference's OWN fp32 arithmetic on these inputs stays at least a factor of two
inside the fp32 bounds the GPU test holds the kernels to (outputs 1e-4, gradients 2e-3 of the network's largest gradient).

Measured (fp32 oracle against fp64 oracle: worst output / worst parameter gradient over its network's largest gradient):
  sbase0 1.7e-5 / 4.1e-4, defaults_like 1.6e-5 / 3.0e-4, every other case under 1.1e-5 / 2.8e-5 (no_depth 2.79e-5, on the GPU 2.85e-5; the rest under 2.2e-5);
  loss: base 1.0946, no_bg 1.1214, no_mask_no_depth 0.8760; 9 sky rays, 13 depth rays, inside share 0.87 .. 0.93;
  spread of the fp32 gradients under a reversed ray order: 3.5e-7 of the network's largest gradient.
If a case misses a condition after a later change of the oracle, change the inputs, not the condition."""
import pytest
import torch

from tests import _render_options as RO

OUT_FLOOR, GRAD_FLOOR = 5e-5, 1e-3  # half of the GPU test's 1e-4 / 2e-3


@pytest.mark.parametrize("case", list(RO.CASES))
def test_inputs_populate_every_branch(case):
    inp, ref = RO.inputs(case=case), RO.oracle(case)
    n_sky, n_depth = int((inp["label"] == 2).sum()), int((inp["rays"][:, 9] > 0).sum())
    inside = float(ref["out"]["inside_sphere"].mean())
    print("%s: %d sky rays, %d depth rays, inside share %.3f, loss %.4f" % (case, n_sky, n_depth, inside, ref["loss"]))
    assert n_sky >= 4 and n_depth >= 4
    assert int((inp["label"] != 2).sum()) >= 4 and int((inp["rays"][:, 9] == 0).sum()) >= 4
    assert 0.5 <= inside <= 0.97, inside
    assert float(inp["background_rgb"].abs().min()) > 0


def _same(a, b, tol=1e-12):
    for k in ("color", "depth", "weights_sum", "gradient_error", "color_bg", "mask_error", "sfm_depth_loss", "z_vals", "weights"):
        assert a["out"][k].shape == b["out"][k].shape and float((a["out"][k] - b["out"][k]).abs().max()) <= tol, k
    assert abs(a["loss"] - b["loss"]) <= tol
    for k, g in a["grads"].items():
        assert (g is None) == (b["grads"][k] is None), k
        if g is not None:
            assert float((g - b["grads"][k]).abs().max()) <= tol * max(1.0, float(g.abs().max())), k


def test_cases_differ_from_base_where_they_should():
    base = RO.oracle("base")
    for case in ("no_bg", "no_mask", "no_depth"):
        d = abs(RO.oracle(case)["loss"] - base["loss"])
        print("|loss(%s) - loss(base)| = %.4f" % (case, d))
        assert d > 1e-3, (case, d)
    assert float((RO.oracle("trim_off")["out"]["color_bg"] - base["out"]["color_bg"]).abs().max()) > 1e-6
    for case in ("steps1", "steps4", "sbase0", "no_imp"):
        z = RO.oracle(case)["out"]["z_vals"]
        assert z.shape != base["out"]["z_vals"].shape or float((z - base["out"]["z_vals"]).abs().max()) > 1e-4, case
    assert RO.oracle("n_out8")["out"]["weights"].shape[1] == base["out"]["weights"].shape[1] + 4
    assert RO.oracle("defaults_like")["out"]["weights"].shape[1] == 16 + 16 + 32
    # ... and is the same function where the option is only another way of saying the same thing (fp64)
    _same(RO.oracle("n_out0"), RO.oracle("no_bg"))
    _same(RO.oracle("moved"), base)
    # gradient pattern the GPU test relies on: the background NeRF takes no part without a background, its view branch never does
    for case in ("no_bg", "n_out0"):
        g = RO.oracle(case)["grads"]
        assert all(v is None for k, v in g.items() if k.startswith("nerf.")), case
    g = base["grads"]
    assert all((v is None) == k.startswith("nerf.views_linears") for k, v in g.items()), [k for k, v in g.items() if v is None]


def test_reference_fp32_floor_is_inside_the_gpu_bounds():
    worst_out = worst_grad = 0.0
    for case in RO.CASES:
        out, grad, name = RO.floors(case)
        print("%-17s fp32 floor: outputs %.2e, gradients %.2e (%s)" % (case, out, grad, name))
        worst_out, worst_grad = max(worst_out, out), max(worst_grad, grad)
    print("worst output floor %.2e, worst gradient floor %.2e" % (worst_out, worst_grad))
    assert worst_out < OUT_FLOOR and worst_grad < GRAD_FLOOR, (worst_out, worst_grad)


def test_reorder_spread_is_defined_for_the_16_bit_comparison():
    """tests/test_gpu_render_options.py bounds the two background-stream paths of the 16-bit modes (f32 atomics either way) by the
    spread of the reference's own f32 sum under reordering: the fp32 oracle's gradients with the rays reversed against the same in
    the given order, over the network's largest gradient.  It must be a positive, small number for both trim_sphere values."""
    for case in ("base", "trim_off"):
        s = RO.reorder_spread(case)
        print("%s: fp32 gradient spread under ray reversal %.2e" % (case, s))
        assert 0.0 < s < 1e-4, s
