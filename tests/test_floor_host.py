"""The floor-normal loss without a GPU: the option constructs, the loss term reproduces the reference's (fixture
tests/golden/render_w64_floor.npz, written by the real reference with FLOOR_NORMAL on), and the restatement the GPU tests hold
the kernels to (tests/_floor_ref.py) reproduces the reference's floor_loss outputs."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import _floor_ref as F
from tests._util import load_golden, rel_err

ROAD, GOLDEN = 6, "render_w64_floor"


def _fixture_sfm2gt():
    here = os.path.dirname(os.path.abspath(__file__))
    return np.load(os.path.join(here, "golden", GOLDEN + ".npz"))["sfm2gt"]  # float64, as the reference had it


def test_renderer_accepts_floor_normal():
    """NeuconWRenderer(floor_normal=True) constructs (it raised NotImplementedError before the option existed); the debug dumps
    are still refused, an unknown label name and a fifth label are refused at construction."""
    from tests._build import build_system

    *_, rdr = build_system(device="cpu", floor_normal=True, floor_labels=["road"])
    assert rdr.floor_normal and rdr.floor_labels == ["road"]
    with pytest.raises(NotImplementedError):
        build_system(device="cpu", floor_normal=True, save_sample=True)
    with pytest.raises(KeyError):
        build_system(device="cpu", floor_normal=True, floor_labels=["no such label"])
    with pytest.raises(ValueError):
        build_system(device="cpu", floor_normal=True, floor_labels=["road", "floor", "sidewalk", "earth", "path"])


def test_config_builds_renderer_and_loss_with_floor_normal(tmp_path):
    """A scene yaml with FLOOR_NORMAL: True goes through config.build_system / config.neuconw_loss: the renderer carries the
    option, the labels and the scene's sfm2gt; the loss has the term, weighted by depth_weight."""
    from neuralrecon_w_amd import config

    m = _fixture_sfm2gt()
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump({"origin": [0.0, 0.0, 0.0], "radius": 1.0, "sfm2gt": m.tolist(), "voxel_size": 0.1,
                        "min_track_length": 2, "eval_bbx": [[-1, -1, -1], [1, 1, 1]]}, f)
    exp = tmp_path / "train.yaml"
    with open(exp, "w") as f:
        yaml.safe_dump({"NEUCONW": {"FLOOR_NORMAL": True, "FLOOR_LABELS": ["road", "sidewalk"], "N_VOCAB": 8,
                                    "LOSS": {"depth_weight": 0.2, "floor_weight": 0.01}},
                        "DATASET": {"ROOT_DIR": str(tmp_path)}}, f)
    cfg = config.load_config(str(exp))
    *_, rdr, _scene = config.build_system(cfg, "cpu")
    assert rdr.floor_normal is True and rdr.floor_labels == ["road", "sidewalk"]
    assert np.allclose(rdr.sfm_to_gt.numpy(), m)
    assert torch.equal(torch.tensor(rdr._floor_normal_gt()), F.floor_n_gt(m))
    loss_fn = config.neuconw_loss(cfg)
    assert loss_fn.use_floor and loss_fn.floor_weight == 0.2


def test_loss_terms_reproduce_reference_floor_term():
    """NeuconWLoss.terms() on the reference's own outputs (CPU tensors): every term, the floor term among them, to 1e-6 relative
    -- with floor_weight = 0.01 passed and ignored: the reference weighs the term by depth_weight = 0.1 (its losses.py:17)."""
    from neuralrecon_w_amd.losses import NeuconWLoss

    _, _, outs, m = load_golden(GOLDEN)
    cfg = {"NEUCONW": {"MESH_MASK_LIST": ["sky"], "DEPTH_LOSS": True, "FLOOR_NORMAL": True}}
    fn = NeuconWLoss(coef=1.0, igr_weight=0.1, mask_weight=0.1, depth_weight=0.1, floor_weight=0.01, config=cfg)
    terms = fn.terms(outs, m["rgbs"])
    want = {k[5:]: v for k, v in m.items() if k.startswith("loss/")}
    assert set(terms) == set(want) and "floor_normal_error" in terms
    for k, v in want.items():
        assert abs(float(terms[k]) - float(v)) <= 1e-6 * abs(float(v)), (k, float(terms[k]), float(v))
    assert abs(float(sum(terms.values())) - float(m["loss"])) <= 1e-6 * abs(float(m["loss"]))
    assert abs(float(terms["floor_normal_error"]) - 0.1 * float(outs["floor_normal_error"].mean())) < 1e-7
    # the keyword form, and the option off: the term is absent
    assert "floor_normal_error" in NeuconWLoss(depth_weight=0.1, use_floor=True).terms(outs, m["rgbs"])
    assert "floor_normal_error" not in NeuconWLoss(depth_weight=0.1).terms(outs, m["rgbs"])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_reproduces_reference_floor_loss(dtype):
    """tests/_floor_ref.py against rendering/renderer.py:918-945 as the reference ran it: floor_normal_error [n_floor,3] and
    floor_y_error from the fixture's own outputs and inputs, to 1e-5.  `normals` is not in render()'s dictionary: it is
    sum_s gradients weights[:, :S]."""
    _, _, outs, m = load_golden(GOLDEN)
    S = outs["gradients"].shape[1]
    normals = (outs["gradients"] * outs["weights"][:, :S, None]).sum(1)
    rays = m["rays"]  # origin 0, radius 1: the rays are in unit-sphere units already
    n_gt = F.floor_n_gt(_fixture_sfm2gt())
    fe, n, y_var = F.floor_forward(normals, m["label"], [ROAD], n_gt, rays[:, 0:3], rays[:, 3:6], outs["depth"], False, dtype)
    mask = F.floor_mask(m["label"], [ROAD])
    assert n == int(mask.sum()) == outs["floor_normal_error"].shape[0] and 0 < n < rays.shape[0]
    assert outs["floor_normal_error"].shape == (n, 3) == outs["floor_y_error"].shape
    assert rel_err(fe[mask], outs["floor_normal_error"]) < 1e-5
    assert bool((fe[~mask] == 0).all())
    assert rel_err(y_var.expand(n, 3), outs["floor_y_error"]) < 1e-5
    # the sync-free form: its mean over all R rows is the reference's mean over the floor rows
    fs, _, _ = F.floor_forward(normals, m["label"], [ROAD], n_gt, rays[:, 0:3], rays[:, 3:6], outs["depth"], True, dtype)
    assert abs(float(fs.mean()) - float(outs["floor_normal_error"].mean())) < 1e-5 * float(outs["floor_normal_error"].mean())
    # n_gt is not axis-aligned in this fixture: no component of it may be mistaken for another
    assert float(n_gt.abs().min()) > 0.1 and abs(float(n_gt.norm()) - 1.0) < 1e-6
