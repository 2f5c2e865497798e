"""Host side of the radius-bounded 1-NN (evalmesh.NNGrid.query_within, csrc/ncw_nn.hip): the binding, the argument checks that
need no GPU, the command-line switch, and -- in numpy -- the conditions the GPU cases of tests/test_gpu_nn_within.py rest on."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import _nn_within_cases as W
from tests._util import ROOT

from neuralrecon_w_amd import evalmesh
from neuralrecon_w_amd import lib as L


def test_binding_and_header_declare_the_entry_points():
    assert {"ncw_nn_coarse", "ncw_nn_query_within"} <= set(L.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "neuconw_hip.h")).read()
    assert "int ncw_nn_coarse(" in hdr and "int ncw_nn_query_within(" in hdr
    assert L.ABI_VERSION >= 35


@pytest.mark.parametrize("bad", [0, -1, float("nan")])
def test_max_dist_must_be_positive(bad):
    grid = evalmesh.NNGrid.__new__(evalmesh.NNGrid)  # the check comes before anything of the grid is read
    pts = torch.zeros(4, 3)
    with pytest.raises(ValueError):
        grid.query_within(pts, bad)
    with pytest.raises(ValueError):
        evalmesh.nn_distances(pts, pts, max_dist=bad)


def test_cpu_tensors_raise():
    grid = evalmesh.NNGrid.__new__(evalmesh.NNGrid)
    pts = torch.zeros(4, 3)
    with pytest.raises(L.NeuconwHipError):
        grid.query_within(pts, 1.0)
    with pytest.raises(L.NeuconwHipError):
        evalmesh.nn_distances(pts, pts, max_dist=1.0)


def test_no_bounded_switch_parses():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import estimate_sfm2gt
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    ap = estimate_sfm2gt.build_parser()
    assert ap.parse_args(["--data_dir", "d", "--gt_pcd_path", "g", "--no_bounded"]).no_bounded is True
    assert ap.parse_args(["--data_dir", "d", "--gt_pcd_path", "g"]).no_bounded is False


def test_gate_bound_admits_every_pair_the_sums_admit():
    """sqrtf(d2) <= gate must imply d2 <= float32(bound)^2 for the float32 neighbours of gate^2."""
    from neuralrecon_w_amd import align

    rng = np.random.RandomState(0)
    for gate in np.float32(10.0 ** rng.uniform(-4, 3, 2000)):
        b = np.float32(align.gate_bound(float(gate)))
        r2 = b * b
        d2 = np.float32(gate) * np.float32(gate)
        for _ in range(8):  # walk up through the float32 values above gate^2 while their root still passes the gate
            if not np.sqrt(d2) <= gate:
                break
            assert d2 <= r2, (gate, d2, r2)
            d2 = np.nextafter(d2, np.float32(np.inf))
        else:
            raise AssertionError("the walk did not leave the gate: %r" % gate)


@pytest.mark.parametrize("name", W.NAMES)
def test_random_cases_have_both_outcomes_and_a_thin_band(name):
    c = W.case(name)
    assert max(c["dims"]) <= 64, c["dims"]                   # NNGrid(max_shell=64).query resolves every query in its shells
    d, _ = W.brute64_numpy(c["P"], c["Q"])
    b = W.bound(c["P"], c["Q"])
    for R in c["radii"]:
        inside = int((d < R - b).sum())
        beyond = int((d > R + b).sum())
        band = d.shape[0] - inside - beyond
        assert inside > 0 and beyond > 0, (name, R / c["h"], inside, beyond)
        assert band <= 0.01 * d.shape[0], (name, R / c["h"], band)
    if name == "clusters":
        assert 2.0 / c["h"] >= 50                            # the clusters' centres are 2 apart
    if name == "outside":
        far = np.abs(c["Q"][1000:2900]).max() - 1.0          # the uniform queries reach this far outside P's box
        assert 25 * c["h"] <= far <= 30 * c["h"]
    if name == "outliers":
        assert np.abs(c["P"][-6:]).max() > 600 * c["h"]       # clamped from far away


def test_lattice_case_is_exact_in_float32():
    P, Q, d2, idx = W.lattice_case()
    both = np.concatenate([P, Q])
    c = (both.min(0) + both.max(0)) / 2
    assert (c == 3.5).all()
    for a in (P - c, Q - c):
        assert (a.astype(np.float32).astype(np.float64) == a).all() and (np.round(a * 2) == a * 2).all()
    assert (d2.astype(np.float32).astype(np.float64) == d2).all()
    vals = set(np.unique(d2).tolist())
    assert {0.0, 9.0, 12.25} <= vals and 0.25 not in vals   # R = 3 has its boundary and its near miss; R = 0.5: coincident only
    assert 2.0 in vals                                       # float32(sqrt 2)^2 rounds below 2: the rounding rule decides
    r = np.float32(np.sqrt(2.0))
    assert float(r * r) < 2.0
    assert (idx < 512).all()                                 # a duplicate (index >= 512) never wins: ties go to the smaller index
