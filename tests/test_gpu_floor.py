"""The floor-normal loss on the GPU: the two launches of the floor term (ncw_ray_floor_fwd / _bwd, through renderer._RayFloorFn)
against the float64 restatement of tests/_floor_ref.py, and render() + NeuconWLoss + backward with the option on against the REAL
reference's outputs and parameter gradients (tests/golden/render_w64_floor.npz), in the fp32 parity mode."""
import functools
import os

import numpy as np
import pytest
import torch
import yaml

from tests import _floor_ref as F
from tests._util import load_golden, rel_err

pytestmark = pytest.mark.gpu

GOLDEN = "render_w64_floor"
PER_SAMPLE = ("weights", "weights_max", "cdf_fine", "gradients")  # tests/test_gpu_render.py
IDS4 = [6, 3, 11, 52]  # road, floor, sidewalk, path


# --------------------------------------------------------------------------------------------------------------------
# the two launches
# --------------------------------------------------------------------------------------------------------------------
def _floor_case(R, n_floor, ids, seed=0):
    g = torch.Generator().manual_seed(1000 * R + 10 * len(ids) + seed)
    normals = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * (1 + 0.1 * torch.randn(R, 1, generator=g))
    label = torch.zeros(R, dtype=torch.int64)
    if n_floor == 1:
        label[R // 2] = ids[-1]
    elif n_floor == R:
        label = torch.tensor([ids[r % len(ids)] for r in range(R)], dtype=torch.int64)
    rays_o = torch.tensor([0.0, 0.0, -2.0]) + 0.1 * torch.randn(R, 3, generator=g)
    rays_d = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0]) + 0.1 * torch.randn(R, 3, generator=g), dim=-1)
    depth = 1.5 + torch.rand(R, generator=g)
    d_fe = torch.randn(R, 3, generator=g)
    n_gt = torch.nn.functional.normalize(torch.tensor([0.3, -0.5, 0.8]), dim=0)
    return normals, label, rays_o, rays_d, depth, d_fe, n_gt


def _launch(normals, label, rays_o, rays_d, depth, d_fe, n_gt, ids, scaled):
    from neuralrecon_w_amd.renderer import _RayFloorFn

    x = normals.cuda().requires_grad_(True)
    fe, scal = _RayFloorFn.apply(x, label.cuda(), rays_o.cuda(), rays_d.cuda(), depth.cuda(), tuple(ids),
                                 tuple(float(v) for v in n_gt), scaled)
    (d_normals,) = torch.autograd.grad(fe, x, d_fe.cuda())
    return fe.detach().cpu(), scal.cpu(), d_normals.cpu()


@pytest.mark.parametrize("R", [1, 5, 257, 1000])
def test_floor_launches_vs_restatement(R):
    """R below one wave, across the 256-thread stride (257) and several trips (1000); no floor ray, one, and all of them; one label id
    and four; scaled and not.  Elementwise arithmetic: 1e-6 relative to float64 on the same fp32 inputs; n_floor exact."""
    worst = 0.0
    for n_floor in sorted({0, 1, R}):
        for ids in ([6], IDS4):
            for scaled in (False, True):
                case = _floor_case(R, n_floor, ids)
                normals, label, rays_o, rays_d, depth, d_fe, n_gt = case
                fe, scal, dn = _launch(*case, ids, scaled)
                fe64, n, y64 = F.floor_forward(normals, label, ids, n_gt, rays_o, rays_d, depth, scaled)
                dn64 = F.floor_backward(normals, label, ids, n_gt, d_fe, scaled)
                tag = (R, n_floor, len(ids), scaled)
                assert n == n_floor and float(scal[0]) == n_floor, tag
                if n_floor == 0:
                    assert not fe.any() and not dn.any() and float(scal[1]) == 0.0, tag
                    continue
                e = (rel_err(fe, fe64), rel_err(dn, dn64), abs(float(scal[1]) - float(y64)) / float(y64))
                worst = max(worst, *e)
                assert max(e) < 1e-6, (tag, e)
                assert bool((fe[label == 0] == 0).all()) and bool((dn[label == 0] == 0).all()), tag
    print("\nfloor launches R=%d: worst rel err %.1e" % (R, worst))


def test_floor_sign_at_zero_and_repeatable():
    """A component of normals equal to n_gt exactly: the error is 0 and so is its gradient (torch's L1: sign(0) = 0), whatever the
    cotangent.  Two runs of the same call are bitwise identical (one workgroup, order-fixed sums)."""
    case = list(_floor_case(257, 257, IDS4, seed=1))
    n_gt = case[6]
    case[0][3, 1] = n_gt[1]
    case[0][200] = n_gt
    assert float(case[5][3, 1]) != 0.0
    a, b = _launch(*case, IDS4, True), _launch(*case, IDS4, True)
    fe, _, dn = a
    assert float(fe[3, 1]) == 0.0 and float(dn[3, 1]) == 0.0 and not fe[200].any() and not dn[200].any()
    assert float(dn[3, 0]) != 0.0
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# --------------------------------------------------------------------------------------------------------------------
# render() + loss + backward against the real reference
# --------------------------------------------------------------------------------------------------------------------
def _loss_fn(floor):
    from neuralrecon_w_amd.losses import NeuconWLoss

    cfg = {"NEUCONW": {"MESH_MASK_LIST": ["sky"], "DEPTH_LOSS": True, "FLOOR_NORMAL": floor}}
    return NeuconWLoss(coef=1.0, igr_weight=0.1, mask_weight=0.1, depth_weight=0.1, floor_weight=0.01, config=cfg)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """A scene directory whose config.yaml carries the fixture's sfm2gt (what renderer.py:103-112 reads)."""
    d = tmp_path_factory.mktemp("floor_scene")
    m = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN + ".npz"))["sfm2gt"]
    with open(d / "config.yaml", "w") as f:
        yaml.safe_dump({"origin": [0.0, 0.0, 0.0], "radius": 1.0, "sfm2gt": m.tolist()}, f)
    return str(d)


@functools.lru_cache(maxsize=None)
def _render(scene, floor=True, sync_free=False, road=True):
    """One render + loss + backward on the fixture's weights and rays in the fp32 parity mode -> (outputs, loss, loss
    terms, parameter gradients), all on the CPU.  road=False relabels the road rays: no floor ray is left."""
    import neuralrecon_w_amd as nw
    from tests._build import build_system, load_golden_weights, named_params

    sd, _, _, m = load_golden(GOLDEN)
    emb, neuconw, nerf, rdr = build_system(prec=nw.PREC_F32, floor_normal=floor,
                                           spc_options={"recontruct_path": scene, "voxel_size": 0.1, "min_track_length": 1})
    load_golden_weights(sd, emb, neuconw, nerf)
    rdr.sync_free = sync_free
    label = m["label"] if road else torch.where(m["label"] == 6, torch.zeros_like(m["label"]), m["label"])
    out = rdr.render(m["rays"].cuda(), m["ts"].cuda(), label.cuda(), perturb_overwrite=0, background_rgb=torch.zeros(1, 3).cuda(),
                     cos_anneal_ratio=0.25)
    fn = _loss_fn(floor)
    loss = fn(out, m["rgbs"].cuda())
    terms = {k: float(v.detach()) for k, v in fn.terms(out, m["rgbs"].cuda()).items()}
    loss.backward()
    grads = {k: p.grad.cpu() for k, p in named_params(emb, neuconw, nerf).items() if p.grad is not None}
    return {k: v.detach().cpu() for k, v in out.items()}, float(loss.detach()), terms, grads


def test_render_matches_reference_golden_with_floor_normal(scene):
    """tests/test_gpu_render.py on the fixture with the option on, same tolerances: 1e-4 per ray (floor_normal_error and
    floor_y_error among them, in the reference's shapes [n_floor,3]), 5e-4 per sample, the loss to 2e-5, every parameter gradient
    below 1e-3 relative to the reference's."""
    _, grads_ref, outs, m = load_golden(GOLDEN)
    out, loss, terms, grads = _render(scene)
    for k, ref in outs.items():
        assert out[k].shape == ref.shape, (k, out[k].shape, ref.shape)
        e = rel_err(out[k], ref)
        assert e < (5e-4 if k in PER_SAMPLE else 1e-4), (k, e)
    assert outs["floor_normal_error"].shape == (15, 3) == out["floor_y_error"].shape
    assert abs(loss - float(m["loss"])) < 2e-5
    assert abs(terms["floor_normal_error"] - float(m["loss/floor_normal_error"])) < 2e-5
    worst = 0.0
    for k, gref in grads_ref.items():
        assert k in grads, k
        e = rel_err(grads[k], gref)
        worst = max(worst, e)
        assert e < 1e-3, (k, e)
    print("\n%s: worst param-grad rel err vs reference %.2e" % (GOLDEN, worst))
    assert "neuconw.xyz_encoding_final.weight" not in grads  # the reference never touches it


def test_floor_gradient_is_what_the_option_adds(scene):
    """The reference's gradients cannot be met without the floor term: the same render with the option off is far outside the
    1e-3 of the test above on the SDF network.  (In the reference's own autograd the term carries 0.70 of max |d loss / d
    lin0.weight_v| on this fixture: tests/golden/make_golden_floor.py prints it.)"""
    _, grads_ref, _, _ = load_golden(GOLDEN)
    _, _, _, g_off = _render(scene, floor=False)
    k = "neuconw.sdf_net.lin0.weight_v"
    assert rel_err(g_off[k], grads_ref[k]) > 1e-2


def test_sync_free_floor_rows(scene):
    """sync_free: the dense rows [R,3] scaled by R / n_floor -- the same mean, the same parameter gradients."""
    out, loss, _, grads = _render(scene)
    out_s, loss_s, _, grads_s = _render(scene, sync_free=True)
    R = out["color"].shape[0]
    assert out_s["floor_normal_error"].shape == (R, 3) == out_s["floor_y_error"].shape
    mean, mean_s = float(out["floor_normal_error"].mean()), float(out_s["floor_normal_error"].mean())
    assert abs(mean - mean_s) <= 1e-6 * abs(mean), (mean, mean_s)
    assert abs(float(out["floor_y_error"].mean()) - float(out_s["floor_y_error"].mean())) <= 1e-6 * float(out["floor_y_error"].mean())
    assert abs(loss - loss_s) < 1e-6
    assert set(grads) == set(grads_s)
    for k in grads:
        assert rel_err(grads_s[k], grads[k]) < 1e-5, (k, rel_err(grads_s[k], grads[k]))


def test_no_floor_ray_is_the_option_off(scene):
    """No ray carries a floor label: zeros [R,3] like the reference, a loss term of 0, and -- the compositor backward gets no
    cotangent for normals, so it is the launch of the option-off render -- bit-identical parameter gradients (fp32 mode)."""
    out, loss, terms, grads = _render(scene, road=False)
    out0, loss0, _, grads0 = _render(scene, floor=False, road=False)
    R = out["color"].shape[0]
    for k in ("floor_normal_error", "floor_y_error"):
        assert out[k].shape == (R, 3) and not out[k].any(), k
    assert terms["floor_normal_error"] == 0.0 and loss == loss0
    assert set(grads) == set(grads0)
    for k in grads:
        assert torch.equal(grads[k], grads0[k]), k


def test_fp16_train_step_with_floor_normal(scene):
    """One fp16 TrainStep with the option on: finite loss and gradient norm, the step is applied, and the SDF network's first-layer
    gradient differs from the option-off step's -- the cotangent reached the network through the loss scale."""
    import neuralrecon_w_amd as nw
    from tests._build import build_system, load_golden_weights

    sd, _, _, m = load_golden(GOLDEN)
    rays, ts, label, rgbs = (m[k].cuda() for k in ("rays", "ts", "label", "rgbs"))
    got = {}
    for floor in (True, False):
        emb, neuconw, nerf, rdr = build_system(prec=nw.PREC_F16, floor_normal=floor,
                                               spc_options={"recontruct_path": scene, "voxel_size": 0.1, "min_track_length": 1})
        load_golden_weights(sd, emb, neuconw, nerf)
        train = nw.TrainStep(rdr, [emb, neuconw, nerf], _loss_fn(floor), lr=1e-3, eps=1e-7, clip=0.99)
        loss, out = train(rays, ts, label, rgbs, background_rgb=torch.zeros(1, 3).cuda(), cos_anneal_ratio=0.25, perturb_overwrite=0)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(train.last_grad_norm).all())
        assert train.opt.skipped_steps == 0 and train.opt.step_count == 1
        got[floor] = (float(loss.detach()), neuconw.sdf_net.lin0.weight_v.grad.detach().cpu().clone())
    assert bool(torch.isfinite(got[True][1]).all())
    assert got[True][0] > got[False][0] + 0.05  # the floor term of this fixture is 0.09
    assert rel_err(got[True][1], got[False][1]) > 1e-2


def test_captured_step_with_floor_normal_replays_like_eager(scene):
    """TrainStep(capture=True) with the option on (sync_free: the dense rows, no host decision inside the graph): the HIP-graph
    replays follow the eager steps -- the loss curve to the 2e-5 of tests/test_gpu_trainer.py's captured-step test -- and the
    floor term is in both (the curve lies above the option-off step's by the term)."""
    import neuralrecon_w_amd as nw
    from tests._build import build_system, load_golden_weights

    sd, _, _, m = load_golden(GOLDEN)
    rays, ts, label, rgbs = (m[k].cuda() for k in ("rays", "ts", "label", "rgbs"))
    bg = torch.zeros(1, 3, device="cuda")
    curves = []
    for capture in (False, True):
        emb, neuconw, nerf, rdr = build_system(prec=nw.PREC_F32, floor_normal=True,
                                               spc_options={"recontruct_path": scene, "voxel_size": 0.1, "min_track_length": 1})
        load_golden_weights(sd, emb, neuconw, nerf)
        rdr.sync_free = True
        train = nw.TrainStep(rdr, [emb, neuconw, nerf], _loss_fn(True), lr=1e-3, eps=1e-7, clip=0.99, capture=capture, capture_warmup=3)
        curves.append([float(train(rays, ts, label, rgbs, background_rgb=bg, cos_anneal_ratio=0.25, perturb_overwrite=0)[0].detach())
                       for _ in range(6)])
        if capture:
            assert train._graphs is not None  # steps 3.. were graph replays
        assert train.opt.step_count == 6 and train.opt.skipped_steps == 0
    for a, b in zip(*curves):
        assert abs(a - b) <= 2e-5 * max(1.0, abs(a)), curves
    assert abs(curves[0][0] - float(m["loss"])) < 2e-5  # step 0 is the fixture's loss, floor term included
    assert curves[0][-1] != curves[0][0]
