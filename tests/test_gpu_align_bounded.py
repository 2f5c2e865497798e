"""GPU: the sfm2gt loop with the radius-bounded query (align.icp_similarity(bounded=True)) against the plain run on the fixture of
tests/_align_cases.py -- every iteration's mask, pairs, rms and matrix bit for bit, idx changed only outside the mask and only
towards -1 -- and the command line with and without --no_bounded: the same sfm2gt.yaml byte for byte.
The fixture's grid has cells of 0.093 units, so with the default 8 shells far_reach (0.747) lies above its first gate (0.4) and
skip_far would cover every iteration; the results do not depend on max_shell, so the comparison also runs on a target built with
max_shell = 2 (far_reach 0.187): there the first gates are above far_reach, and the bounded path must leave sources at -1 there."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import _align_cases as K
from tests._util import ROOT

from neuralrecon_w_amd import align, ply

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(fx, max_shell, **kw):
    target = align.AlignTarget(fx["gt"], DEV, gate_max=K.GATE0, max_shell=max_shell)
    st = {"keep_pairs": True}
    src = torch.from_numpy(np.ascontiguousarray(fx["src"])).to(DEV)
    T = align.icp_similarity(src, target, fx["init"], gate0=K.GATE0, shrink=K.SHRINK, gate_min=K.GATE_MIN, stats=st, **kw)
    return T, st, target


@pytest.mark.parametrize("max_shell", [8, 2])
def test_bounded_gives_the_same_pairs_and_matrices_bit_for_bit(max_shell):
    fx = K.fixture()
    T, st, target = _run(fx, max_shell)
    T2, st2, _ = _run(fx, max_shell, bounded=True)
    reach = align.far_reach(target.grid)
    assert np.array_equal(T, T2) and st["iterations"] == st2["iterations"] and st["converged"] == st2["converged"]
    above = 0
    for k, (a, b) in enumerate(zip(st["history"], st2["history"])):
        assert a["gate"] == b["gate"] and a["pairs"] == b["pairs"] and a["rms"] == b["rms"] and a["matrix"] == b["matrix"], k
        assert a["max_residual"] == b["max_residual"] and a["mean_distance"] == b["mean_distance"], k
        assert np.array_equal(a["mask"], b["mask"]), k
        differ = a["idx"] != b["idx"]
        assert (b["idx"][differ] == -1).all() and not a["mask"][differ].any(), k
        assert int(differ.sum()) == b["beyond"], (k, int(differ.sum()), b["beyond"])
        assert b["escaped"] == 0 and b["skipped_far"] == 0, k
        above += int(a["gate"] > reach and b["beyond"] > 0)
    print("bounded: far_reach %.3f, gates %s, beyond per iteration %s, escaped in the plain run %s"
          % (reach, ["%.3f" % h["gate"] for h in st2["history"]], [h["beyond"] for h in st2["history"]],
             [h["escaped"] for h in st["history"]]))
    if max_shell == 2:
        assert above > 0      # the bounded path was taken at a gate above far_reach, where skip_far cannot help


def test_command_line_writes_the_same_yaml_with_and_without_the_bound(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import estimate_sfm2gt
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    scene = os.path.join(ROOT, "tests", "golden", "cache_scene")
    case = K.scene_case(os.path.join(scene, "dense", "sparse", "points3D.bin"))
    gt_path, pairs_path = str(tmp_path / "gt.ply"), str(tmp_path / "pairs.txt")
    ply.write(gt_path, case["gt"])
    np.savetxt(pairs_path, case["pairs"], fmt="%.17g")
    out = {}
    for tag, extra in (("bounded", []), ("plain", ["--no_bounded"])):
        out[tag] = str(tmp_path / tag)
        estimate_sfm2gt.main(["--data_dir", scene, "--gt_pcd_path", gt_path, "--pairs", pairs_path, "--track_length", "0",
                              "--reproj_error", "1e9", "--out_dir", out[tag]] + extra)
    capsys.readouterr()
    a = open(os.path.join(out["bounded"], "sfm2gt.yaml"), "rb").read()
    b = open(os.path.join(out["plain"], "sfm2gt.yaml"), "rb").read()
    assert a == b and len(a) > 0
    ra = json.load(open(os.path.join(out["bounded"], "report.json")))
    rb = json.load(open(os.path.join(out["plain"], "report.json")))
    assert ra["matrix"] == rb["matrix"] and ra["iterations"] == rb["iterations"] and ra["pairs"] == rb["pairs"] and ra["rms"] == rb["rms"]
    for ha, hb in zip(ra["history"], rb["history"]):
        assert ha["pairs"] == hb["pairs"] and ha["rms"] == hb["rms"] and ha["matrix"] == hb["matrix"]
        assert ha["escaped"] == 0 and ha["skipped_far"] == 0 and "beyond" in ha
