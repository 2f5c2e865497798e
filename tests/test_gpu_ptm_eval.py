"""GPU: eval_mesh(exact_recall=True) -- the recall side of the mesh evaluation from exact point-to-triangle distances
(csrc/ncw_ptm.hip) -- against the sampled path it refines: the distance to the surface is never above the distance to a
sample of it, so recall can only rise, and the precision side must not move."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from neuralrecon_w_amd import evalmesh, mesh
from tests import _ptm_ref as R
from tests._util import ROOT

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
DEV = "cuda:0"
SFM2GT = np.array([[0.0, -1.0, 0, 10.0], [1.0, 0.0, 0, -5.0], [0, 0, 1.0, 3.0], [0, 0, 0, 1]])  # rigid
THRESHOLDS = "0.01,0.035,0.01"  # 0.01, 0.02, 0.03: of the order of the sample spacing (about 0.018 here)


def _cli(scene, save_name, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_mesh.py"), "--file_pred", scene["pred"], "--file_trgt",
                        scene["gt"], "--scene_config_path", scene["cfg"], "--mesh", "--threshold", THRESHOLDS, "--save_name", save_name]
                       + list(flags), capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = os.path.join(os.path.dirname(scene["pred"]), "eval_" + save_name)
    return out, open(os.path.join(out, "metrics.json"), "rb").read()


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ptm")
    v, f = R.height_field(24, seed=1)
    pred = str(tmp / "pred" / "field.ply")
    os.makedirs(os.path.dirname(pred))
    mesh.write_ply(pred, torch.from_numpy(v), torch.from_numpy(f))
    g, _ = R.interior_queries(v, f, 300, seed=3, lift=0.004)  # a GT cloud 4 mm off the surface
    g_gt = g @ SFM2GT[:3, :3].T + SFM2GT[:3, 3]
    gt = str(tmp / "gt.ply")
    mesh.write_ply(gt, torch.from_numpy(g_gt), torch.zeros(0, 3, dtype=torch.int64))
    c = SFM2GT[:3, 3]
    # the box cuts the mesh: the triangles with a corner outside are dropped on both sides alike
    cfg_d = {"sfm2gt": SFM2GT.tolist(), "eval_bbx": [(c + [-0.8, 0.1, -1.0]).tolist(), (c + [-0.1, 0.9, 1.0]).tolist()]}
    cfg = str(tmp / "config.yaml")
    yaml.safe_dump(cfg_d, open(cfg, "w"))
    s = {"tmp": tmp, "pred": pred, "gt": gt, "cfg": cfg, "scene": cfg_d, "v_gt": v @ SFM2GT[:3, :3].T + SFM2GT[:3, 3], "f": f}
    s["exact"] = _cli(s, "exact", "--sample_surface", "--exact_recall")
    s["sampled"] = _cli(s, "sampled", "--sample_surface")
    return s


def test_exact_distance_is_at_most_the_sampled_distance(scene):
    box = scene["scene"]["eval_bbx"]
    g = evalmesh.bbx_crop(torch.from_numpy(evalmesh.read_ply_points(scene["gt"])).to(DEV), box)
    assert 100 < g.shape[0] < 300
    d_exact, tri = evalmesh.mesh_distances(scene["v_gt"], scene["f"], g, box=box)
    samples = evalmesh.sample_surface(scene["v_gt"], scene["f"], 10 * g.shape[0], seed=0, box=box, device=DEV)
    d_samp, _ = evalmesh.nn_distances(samples, g)
    both = torch.cat([samples, g])
    bound = 8 * EPS32 * float((both - (both.amin(0) + both.amax(0)) / 2).abs().max())  # tests/test_gpu_nn.py
    over = float((d_exact - d_samp.double()).max())
    print("exact - sampled: max %.3e (f32 bound %.3e), mean %.3e; mean exact %.4e" % (over, bound, float((d_exact - d_samp.double()).mean()),
                                                                                     float(d_exact.mean())))
    assert over <= bound
    assert float((d_samp.double() - d_exact).mean()) > 0  # and the sampled distance really is the larger one
    t = scene["v_gt"][scene["f"][tri.cpu().numpy()]]
    assert ((t >= np.array(box[0])) & (t <= np.array(box[1]))).all()


def test_command_line_exact_recall(scene):
    (out_e, raw_e), (out_s, raw_s) = scene["exact"], scene["sampled"]
    e, s = json.loads(raw_e), json.loads(raw_s)
    assert e["recal_mode"] == "exact" and len(e["thresholds"]) == 3 and e["thresholds"] == s["thresholds"]
    print("recall exact %s, sampled %s" % (e["recals"], s["recals"]))
    assert all(a >= b for a, b in zip(e["recals"], s["recals"])) and e["recals"][0] > s["recals"][0]
    assert e["precs"] == s["precs"]  # the same samples (seed 0) against the same GT
    a, b = (open(os.path.join(o, "down_pred_in_gt.ply"), "rb").read() for o in (out_e, out_s))
    assert a == b
    for t in e["thresholds"]:
        pe, ps = (json.load(open(os.path.join(o, "visualize", "%.2f" % t, "metrics.json"))) for o in (out_e, out_s))
        assert pe["prec"] == ps["prec"] and pe["dist1"] == ps["dist1"] and pe["dist2"] <= ps["dist2"]


def test_option_off_writes_what_it_wrote_before(scene):
    out_s, raw_s = scene["sampled"]
    s = json.loads(raw_s)
    assert list(s) == ["thresholds", "fscores", "precs", "recals"]  # no new key
    per = [json.load(open(os.path.join(out_s, "visualize", "%.2f" % t, "metrics.json"))) for t in s["thresholds"]]
    want = json.dumps({"thresholds": s["thresholds"], "fscores": [p["fscore"] for p in per], "precs": [p["prec"] for p in per],
                       "recals": [p["recal"] for p in per]}).encode()
    assert raw_s == want
    files = sorted(os.path.join(dp, f)[len(out_s):] for dp, _, fs in os.walk(out_s) for f in fs)
    assert files == ["/down_gt.ply", "/down_pred_in_gt.ply", "/metrics.json"] + ["/visualize/%.2f/metrics.json" % t for t in s["thresholds"]]
    # and the function with the option off is the function as it was: the same bytes as the command line without the flag
    evalmesh.eval_mesh(scene["pred"], scene["gt"], scene["scene"], is_mesh=True, threshold=s["thresholds"], save_name="off",
                       verbose=False, surface=10, exact_recall=False)
    assert open(os.path.join(os.path.dirname(scene["pred"]), "eval_off", "metrics.json"), "rb").read() == raw_s


def test_vertex_precision_with_exact_recall(scene):
    """surface=None: the precision side is the vertices, the recall side the surface."""
    m = evalmesh.eval_mesh(scene["pred"], scene["gt"], scene["scene"], is_mesh=True, threshold=[0.01], save_name="vx", verbose=False,
                           exact_recall=True)
    m0 = evalmesh.eval_mesh(scene["pred"], scene["gt"], scene["scene"], is_mesh=True, threshold=[0.01], save_name="vx0", verbose=False)
    assert m["prec"] == m0["prec"] and m["dist1"] == m0["dist1"]
    assert m["recal"] > 0.7 > m0["recal"]  # 4 mm from the surface (but for the rim the box cut away), centimetres from a vertex


def test_a_file_without_faces_is_refused(scene):
    with pytest.raises(ValueError, match="no faces"):
        evalmesh.eval_mesh(scene["gt"], scene["gt"], scene["scene"], is_mesh=True, threshold=[0.01], save_name="nofaces", verbose=False,
                           exact_recall=True)
