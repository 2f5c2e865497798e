"""The renderer's option branches as a case table, with the inputs and the oracle every case is judged against: shared by
tests/test_render_options_host.py (CPU: the inputs populate every branch, the reference's own fp32 floor) and
tests/test_gpu_render_options.py (GPU: render(), the backward and the train step per case).

A case is a dict of overrides applied BOTH to tests/_build.build_system(**kw) (the renderer's constructor keywords) and to the
oracle's cfg; everything else is BASE -- the one configuration the other composed tests use."""
import math

import torch

from tests._build import build_system, state_dict_cpu
from tests._parity import CFG, perturb_weights
from tests._util import synth_rays

R = 48
N_VOCAB = 64
SEED = 2
COS_ANNEAL = 0.3

# build_system's own option set at 16 + 16 samples; the oracle's cfg for it is CFG (tests/_parity.py == tests/test_gpu_edges.py)
BASE = dict(n_samples=16, n_importance=16, n_outside=4, up_sample_steps=2, s_val_base=3, render_bg=True, trim_sphere=True,
            mesh_mask_list=["sky"], depth_loss=True, origin=[0.0, 0.0, 0.0], radius=1.0)
assert all(CFG[k] == BASE[k] for k in CFG if k in BASE)

MOVED_ORIGIN, MOVED_RADIUS = [0.5, -0.25, 1.0], 2.0

CASES = {
    "base": {},
    "no_bg": dict(render_bg=False),
    "n_out0": dict(n_outside=0),
    "n_out8": dict(n_outside=8),
    "trim_off": dict(trim_sphere=False),
    "steps1": dict(up_sample_steps=1),
    "steps4": dict(up_sample_steps=4),
    "sbase0": dict(s_val_base=0),
    "no_imp": dict(n_importance=0),
    "no_mask": dict(mesh_mask_list=None),
    "no_depth": dict(depth_loss=False),
    "no_mask_no_depth": dict(mesh_mask_list=None, depth_loss=False),
    # config/defaults.py's values of the five options (at this file's 16 + 16 samples)
    "defaults_like": dict(up_sample_steps=4, n_outside=32, mesh_mask_list=None, depth_loss=False, s_val_base=0),
    # the same normalised rays seen from another scene frame: inputs() maps the ray origins and depths accordingly
    "moved": dict(origin=MOVED_ORIGIN, radius=MOVED_RADIUS),
}


def options(case):
    """-> the full option set of `case` (BASE + overrides): build_system(**options(case)) builds its renderer."""
    return dict(BASE, **CASES[case])


def has_bg(case):
    o = options(case)
    return bool(o["render_bg"] and o["n_outside"] > 0)


def oracle_cfg(case, dtype=torch.float64):
    cfg = dict(CFG, **options(case))
    cfg["origin"] = torch.tensor(cfg["origin"], dtype=dtype)
    return cfg


def loss_kw(case):
    """NeuconWLoss keywords of the case: the mask / depth terms follow the renderer's options (losses.py:31-35)."""
    o = options(case)
    return dict(coef=1.0, igr_weight=CFG["igr_weight"], mask_weight=CFG["mask_weight"], depth_weight=CFG["depth_weight"],
                use_mask=o["mesh_mask_list"] is not None, use_depth=bool(o["depth_loss"]))


def inputs(R=R, case="base", quantise=False, dtype=torch.float32):
    """-> dict(rays [R,10], ts, label, rgbs, background_rgb [1,3]) on the CPU in `dtype` (the values are fp32 ones; only the `moved`
    case's frame change is carried out in fp64 first, where it is exact).
    synth_rays(48, 77, 64) alone draws ONE sky ray, ONE depth ray and one depth value: every 8th ray is made sky, every 6th
    (from 1) gets a depth weight 0.5, 0.6, ..., and the depth targets vary per ray.  The background colour is NOT zero: a zero
    colour hides the (1 - weights_sum) term of renderer.py:753-754.
    quantise: ray origins rounded to multiples of 2^-10, so that the `moved` case's (o * 2 + origin - origin) / 2 is exact in fp32.
    case "moved": the same rays expressed in a frame with that case's origin / radius."""
    rays, ts, label, rgbs = synth_rays(R, 77, N_VOCAB)
    rays, label = rays.clone(), label.clone()
    label[::8] = 2
    n = rays[1::6].shape[0]
    rays[1::6, 9] = 0.5 + 0.1 * torch.arange(n, dtype=torch.float32)
    rays[:, 8] = 2.0 + 0.2 * torch.sin(torch.arange(R, dtype=torch.float32))
    if quantise:
        rays[:, 0:3] = torch.round(rays[:, 0:3] * 1024.0) / 1024.0
    o = options(case)
    rays = rays.double()
    if o["origin"] != BASE["origin"] or o["radius"] != BASE["radius"]:
        rays[:, 0:3] = rays[:, 0:3] * o["radius"] + torch.tensor(o["origin"], dtype=torch.float64)
        rays[:, 6:9] = rays[:, 6:9] * o["radius"]
    return dict(rays=rays.to(dtype), ts=ts, label=label, rgbs=rgbs.to(dtype), background_rgb=torch.full((1, 3), 0.25, dtype=dtype))


def weights(neuconw):
    """A non-sphere SDF with exercised weight-norm (the geometric initialisation alone is a distance-to-sphere function)."""
    perturb_weights(neuconw, 0.1, 0.05)


def system(case="base", device="cuda", prec=None, W=64, **kw):
    """-> (emb, neuconw, nerf, renderer) of `case` with the perturbed weights; the weights do not depend on the case."""
    big = dict(n_a=48, n_vocab=100, nerf_w=256, color_hidden=256, head=128) if W != 64 else {}
    s = build_system(W=W, seed=SEED, device=device, prec=prec, **dict(big, **dict(options(case), **kw)))
    weights(s[1])
    return s


def net_of(k):
    """The network a state-dict key belongs to (tests/_parity.run_case): gradients are scored over its largest gradient."""
    return k.split(".")[0] if not k.startswith("neuconw.") else ".".join(k.split(".")[:2])


def grad_scales(gref):
    scale = {}
    for k, g in gref.items():
        if g is not None:
            scale[net_of(k)] = max(scale.get(net_of(k), 0.0), float(g.abs().max()))
    return scale


_SD = {}
_ORACLE = {}


def state_dict(dtype=torch.float64, W=64):
    if W not in _SD:
        emb, neuconw, nerf, _ = system("base", device="cpu", W=W)
        _SD[W] = state_dict_cpu(emb, neuconw, nerf, torch.float64)
    return {k: v.to(dtype).clone() for k, v in _SD[W].items()}


def run_oracle(cfg, sd, inp, dtype, cos_anneal=COS_ANNEAL, background_rgb="given"):
    """render + loss + gradients of the whole state dict with the oracle -> dict(out, loss, grads, scale)."""
    from oracle import neuconw_oracle as O

    sd = {k: v.requires_grad_(True) for k, v in sd.items()}
    bg = inp["background_rgb"] if isinstance(background_rgb, str) else background_rgb
    ref = O.render(sd, cfg, inp["rays"].to(dtype), inp["ts"], inp["label"], cos_anneal, None if bg is None else bg.to(dtype))
    lref = O.neuconw_loss(ref, inp["rgbs"].to(dtype), cfg)
    names = list(sd)
    gref = dict(zip(names, torch.autograd.grad(lref, [sd[k] for k in names], allow_unused=True)))
    return dict(out={k: (v.detach() if torch.is_tensor(v) else v) for k, v in ref.items()}, loss=float(lref.detach()), grads=gref,
                scale=grad_scales(gref))


def oracle(case, dtype=torch.float64, W=64, R=R):
    """The oracle's render + neuconw_loss + torch.autograd.grad over the whole state dict for `case` on inputs(R, case), computed
    once per (case, dtype, W, R) and shared -> dict(out, loss, grads {key: tensor or None}, scale {network: largest |gradient|})."""
    key = (case, dtype, W, R)
    if key not in _ORACLE:
        _ORACLE[key] = run_oracle(oracle_cfg(case, dtype), state_dict(dtype, W), inputs(R, case, dtype=dtype), dtype)
    return _ORACLE[key]


def reorder_spread(case):
    """The spread of the reference's own f32 sums under reordering: the fp32 oracle's parameter gradients with the rays in reversed
    order against the same in the given order, the largest difference over the tensor's network's largest gradient."""
    a = oracle(case, torch.float32)
    inp = inputs(case=case)
    rev = {k: (v.flip(0) if k != "background_rgb" else v) for k, v in inp.items()}
    b = run_oracle(oracle_cfg(case, torch.float32), state_dict(torch.float32), rev, torch.float32)
    return max(float((b["grads"][k] - g).abs().max()) / a["scale"][net_of(k)] for k, g in a["grads"].items() if g is not None)


def floors(case):
    """rel_err(oracle in float32, oracle in float64): -> (worst of colour / depth / weights_sum / gradient_error, worst parameter
    gradient over its network's largest gradient, that tensor's name).  What the reference's OWN fp32 arithmetic is off by on
    these inputs: an fp32 bound on the GPU must sit above it, and is not owed anything tighter."""
    from tests._util import rel_err

    a, b = oracle(case, torch.float32), oracle(case, torch.float64)
    out = max(rel_err(a["out"][k], b["out"][k]) for k in ("color", "depth", "weights_sum", "gradient_error"))
    worst, name = 0.0, None
    for k, g in b["grads"].items():
        if g is None:
            assert a["grads"][k] is None, k
            continue
        e = float((a["grads"][k].double() - g).abs().max()) / b["scale"][net_of(k)]
        if e > worst:
            worst, name = e, k
    assert math.isfinite(out) and math.isfinite(worst)
    return out, worst, name
