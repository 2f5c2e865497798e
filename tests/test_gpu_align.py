"""GPU: the sfm2gt estimation (neuralrecon_w_amd/align.py, csrc/ncw_align.hip) against the numpy restatement tests/_align_ref.py.

ncw_align_transform must EQUAL the restatement bit for bit (float32 queries and flags).  ncw_align_sums: the count is equal; the
20 sums lie within 4 x the restatement's own deviation from its long-double run, with a floor of one ulp of the sum, and every
case prints whether they were in fact bit-identical (the contract fixes every rounding and the whole order, so they are expected
to be).  The loop on the fixture of tests/_align_cases.py is compared iteration by iteration: idx and pair mask equal (the
conditions that rests on are asserted on the restated run by tests/test_align_host.py), the matrix within the sums' bound, the
final matrix within 16 x the error of the closed-form solve on the true pairs, the same number of iterations."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import _align_cases as K
from tests import _align_ref as R
from tests._util import ROOT

from neuralrecon_w_amd import align, ply
from neuralrecon_w_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, LANES = R.BLOCK, R.LANES


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Box:
    """What transform_points reads of an AlignTarget."""

    def __init__(self, centre, lo, hi):
        self.centre, self.box_lo, self.box_hi = np.asarray(centre, np.float64), np.asarray(lo, np.float32), np.asarray(hi, np.float32)


# ---------------------------------------------------------------------------------------------------
# ncw_align_transform
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_transform_bitwise(N):
    g = np.random.RandomState(N)
    T = K.similarity(3.7, [0.3, -0.5, 0.8], 40.0, [100.3, -50.7, 20.1])
    box = _Box([101.0, -49.5, 21.25], [-3.0, -2.0, -1.5], [3.5, 2.25, 1.0])
    gate = 0.4
    P = g.randn(N, 3) * 0.45         # images spread over about 1.7 units: a good part lands in the grown box, the rest outside
    if N > 1:
        P[N // 2, g.randint(3)] = np.nan
    q, ins = align.transform_points(_dev(P), T, box, gate)
    rq, rins = R.query(P, T, box.centre, box.box_lo, box.box_hi, gate)
    assert q.dtype == torch.float32 and ins.dtype == torch.uint8
    assert np.array_equal(q.cpu().numpy().view(np.uint32), rq.view(np.uint32))      # bit for bit, the NaN included
    assert np.array_equal(ins.cpu().numpy(), rins)
    if N > 1:
        assert rins[N // 2] == 0            # the NaN row
    if N >= 63:
        assert 0 < rins.sum() < N - 1       # both outcomes occur


def test_transform_points_exactly_on_the_grown_faces():
    """T = 2 I | t with t and the centre on a binary grid: x - centre is exact, so a query can be put ON a face of the grown box, one
    float32 step inside it and one step outside it, on every face."""
    box = _Box([64.0, -32.0, 16.0], [-3.0, -2.0, -1.5], [3.5, 2.25, 1.0])
    gate = np.float32(0.4)
    T = np.eye(4)
    T[:3, :3] *= 2.0
    T[:3, 3] = [60.0, -30.0, 10.0]
    lo, hi = box.box_lo - gate, box.box_hi + gate                                   # float32, as the kernel forms them
    rows, want = [], []
    for a in range(3):
        for face, step_out in ((lo[a], np.float32(-np.inf)), (hi[a], np.float32(np.inf))):
            for v, inside in ((face, 1), (np.nextafter(face, step_out), 0), (np.nextafter(face, -step_out), 1)):
                q = np.zeros(3, dtype=np.float32)
                q[a] = v
                rows.append((q.astype(np.float64) + box.centre - T[:3, 3]) / 2.0)   # exact: a division by two
                want.append(inside)
    P = np.array(rows)
    q, ins = align.transform_points(_dev(P), T, box, float(gate))
    rq, rins = R.query(P, T, box.centre, box.box_lo, box.box_hi, float(gate))
    assert np.array_equal(rins, np.array(want, dtype=np.uint8))                      # the restatement puts them where intended
    assert np.array_equal(q.cpu().numpy().view(np.uint32), rq.view(np.uint32)) and np.array_equal(ins.cpu().numpy(), rins)


# ---------------------------------------------------------------------------------------------------
# ncw_align_sums
# ---------------------------------------------------------------------------------------------------
class _Cloud:
    def __init__(self, Q, cq):
        self.points, self.m, self.centre = _dev(Q), len(Q), np.asarray(cq, np.float64)


def _sums_case(N, seed, M=500, gate=0.25, all_out=False):
    """Coordinates offset by 1e3 (cp / cq take it out), idx with repeats (M << N), a fifth -1, a few beyond M; dist around the gate
    with rows exactly ON it (they take part) and NaN rows (they do not)."""
    g = np.random.RandomState(seed)
    P = g.randn(N, 3) * [3.0, 2.0, 1.0] + [1000.0, -1000.0, 1000.0]
    Q = g.randn(M, 3) * 7.4 + [2000.0, 500.0, -1000.0]
    idx = g.randint(0, M, N).astype(np.int64)
    idx[g.rand(N) < 0.2] = -1
    idx[g.rand(N) < 0.01] = M + 3
    dist = (2 * gate * g.rand(N)).astype(np.float32)
    dist[g.rand(N) < 0.1] = np.float32(gate)
    dist[g.rand(N) < 0.05] = np.nan
    if all_out:
        dist = np.where(np.isnan(dist), dist, np.float32(gate) + np.float32(0.5) * (1 + dist))
    T = K.similarity(2.1, [0.5, 0.1, -0.7], 33.0, [1.0, 2.0, 3.0])
    return P, Q, idx, dist, np.float32(gate), T, P.mean(0), np.array([2000.0, 500.0, -1000.0])


def _check_sums(N, seed, name, **kw):
    P, Q, idx, dist, gate, T, cp, cq = _sums_case(N, seed, **kw)
    s, c = align.correspondence_sums(_dev(P), cp, _Cloud(Q, cq), _dev(idx), _dev(dist), float(gate), T)
    s2, c2 = align.correspondence_sums(_dev(P), cp, _Cloud(Q, cq), _dev(idx), _dev(dist), float(gate), T)
    assert torch.equal(s, s2) and torch.equal(c, c2), "repeated calls differ"
    s, c = s.cpu().numpy(), c.cpu().numpy()
    r, rc = R.sums(P, cp, Q, cq, idx, dist, gate, T)
    ld, _ = R.sums(P, cp, Q, cq, idx, dist, gate, T, dtype=np.longdouble)
    own = np.abs(r.astype(np.longdouble) - ld).astype(np.float64)
    tol = np.maximum(4.0 * own, np.spacing(np.abs(r)))
    err = np.abs(s - r)
    print("%s: N %d, %d pairs; max |gpu - restatement| / tolerance %.3g, restatement vs long double %.3e, bit-identical: %s"
          % (name, N, rc[0], float((err / tol).max()), float(own.max()), bool(np.array_equal(s, r))))
    assert c[0] == rc[0] and c[1] == rc[1]
    assert (err <= tol).all(), (err, tol)
    return s, c, rc


@pytest.mark.parametrize("N", [1, B - 1, B, B + 1, LANES * B + 1])
def test_sums_at_the_block_edges(N):
    s, c, rc = _check_sums(N, N % 1000 + 1, "mixed")
    assert N < 100 or 0 < rc[0] < N


def test_sums_single_pair_and_dist_on_the_gate():
    P, Q, idx, dist, gate, T, cp, cq = _sums_case(1, 7)
    idx[0], dist[0] = 5, gate                                                        # dist == gate: takes part
    s, c = align.correspondence_sums(_dev(P), cp, _Cloud(Q, cq), _dev(idx), _dev(dist), float(gate), T)
    r, rc = R.sums(P, cp, Q, cq, idx, dist, gate, T)
    assert rc[0] == 1 and c.cpu().numpy()[0] == 1 and np.array_equal(s.cpu().numpy(), r)
    dist[0] = np.nextafter(gate, np.float32(np.inf))                                 # one float32 step beyond: does not
    s, c = align.correspondence_sums(_dev(P), cp, _Cloud(Q, cq), _dev(idx), _dev(dist), float(gate), T)
    assert c.cpu().numpy().tolist() == [0, 0] and not s.cpu().numpy().any()


def test_sums_every_pair_gated_out_and_empty():
    s, c, rc = _check_sums(B + 1, 11, "all gated out", all_out=True)
    assert rc[0] == 0 and c[0] == 0 and c[1] == 0 and not s.any()
    P, Q, idx, dist, gate, T, cp, cq = _sums_case(4, 3)
    s, c = align.correspondence_sums(_dev(P[:0]), cp, _Cloud(Q, cq), _dev(idx[:0]), _dev(dist[:0]), float(gate), T)
    assert c.cpu().numpy().tolist() == [0, 0] and not s.cpu().numpy().any()         # N == 0 gives zeros


def test_bad_arguments_are_refused_without_a_launch():
    import ctypes as C

    lib = L.get_lib()
    z3, z12 = (C.c_double * 3)(), (C.c_double * 12)()
    f3 = (C.c_float * 3)()
    t = torch.zeros(64, dtype=torch.float64, device=DEV)
    null, s = C.c_void_p(0), L.stream_ptr(t.device)
    assert lib.ncw_align_transform(L.ptr(t), -1, z12, z3, f3, f3, 0.1, L.ptr(t), L.ptr(t), s) == -1
    assert lib.ncw_align_transform(null, 4, z12, z3, f3, f3, 0.1, L.ptr(t), L.ptr(t), s) == -1
    assert lib.ncw_align_sums(null, 4, z3, L.ptr(t), 4, z3, L.ptr(t), L.ptr(t), 0.1, z12, L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), s) == -1
    assert lib.ncw_align_sums(L.ptr(t), -1, z3, L.ptr(t), 4, z3, L.ptr(t), L.ptr(t), 0.1, z12, L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), s) == -1
    assert lib.ncw_align_sums(L.ptr(t), 4, z3, L.ptr(t), 4, z3, L.ptr(t), L.ptr(t), 0.1, z12, L.ptr(t), L.ptr(t), null, L.ptr(t), s) == -1
    assert lib.ncw_align_sums_blocks(0) == 0 and lib.ncw_align_sums_blocks(B) == 1 and lib.ncw_align_sums_blocks(B + 1) == 2
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------
def _run(fx, init, **kw):
    target = align.AlignTarget(fx["gt"], DEV, gate_max=K.GATE0)
    st = {"keep_pairs": True}
    T = align.icp_similarity(_dev(fx["src"]), target, init, gate0=K.GATE0, shrink=K.SHRINK, gate_min=K.GATE_MIN, stats=st, **kw)
    return T, st, target


def test_loop_on_the_fixture_iteration_by_iteration():
    fx = K.fixture()
    Tr, hist, rt = K.restated()
    T, st, target = _run(fx, fx["init"])
    assert np.array_equal(target.centre, rt.centre) and np.array_equal(target.box_lo, rt.box_lo) and np.array_equal(target.box_hi, rt.box_hi)
    identical = []
    for k, (h, r) in enumerate(zip(st["history"], hist)):
        assert h["gate"] == r["gate"] and h["pairs"] == r["pairs"], k
        assert np.array_equal(h["mask"], r["mask"]), (k, int((h["mask"] != r["mask"]).sum()))
        assert np.array_equal(h["idx"], r["idx"]), (k, int((h["idx"] != r["idx"]).sum()))
        m = np.array(h["matrix"])
        own = float(np.abs(r["matrix"] - r["matrix_ld"]).max())
        tol = np.maximum(4.0 * own, np.spacing(np.abs(r["matrix"])))
        assert (np.abs(m - r["matrix"]) <= tol).all(), (k, np.abs(m - r["matrix"]).max(), own)
        identical.append(bool(np.array_equal(m, r["matrix"])))
    yard = K.true_pairs_error(fx)
    err = K.matrix_error(T, fx["truth"])
    print("loop: %d iterations (restatement %d), matrices bit-identical per iteration: %s; final max |T - T_true| / max |T_true| = "
          "%.3e, true pairs %.3e" % (st["iterations"], len(hist), identical, err, yard))
    assert st["iterations"] == len(hist) and st["converged"]
    assert err <= 16 * yard
    assert st["history"][-1]["pairs"] == K.N_SRC and st["history"][-1]["rms"] < 1e-12


def test_skip_far_gives_the_same_pairs_and_matrices_bit_for_bit():
    """skip_far leaves the queries the grid cannot resolve at idx = -1 once the gate is below far_reach: every iteration's mask,
    pairs and matrix are the bits of the plain run; idx differs only on sources that take no part, and only towards -1."""
    fx = K.fixture()
    T, st, target = _run(fx, fx["init"])
    T2, st2, _ = _run(fx, fx["init"], skip_far=True)
    reach = align.far_reach(target.grid)
    assert np.array_equal(T, T2) and st["iterations"] == st2["iterations"]
    for k, (a, b) in enumerate(zip(st["history"], st2["history"])):
        assert a["pairs"] == b["pairs"] and a["matrix"] == b["matrix"] and a["rms"] == b["rms"], k
        assert np.array_equal(a["mask"], b["mask"]), k
        differ = a["idx"] != b["idx"]
        assert (b["idx"][differ] == -1).all() and not a["mask"][differ].any(), k
        assert int(differ.sum()) == b["skipped_far"] == (a["escaped"] if a["gate"] < reach else 0), k
    print("skip_far: far_reach %.3f, skipped per iteration %s" % (reach, [h["skipped_far"] for h in st2["history"]]))
    assert sum(h["skipped_far"] for h in st2["history"]) > 0                        # far outliers exist: the path was taken


def test_rigid_variant_without_scale():
    fx = K.fixture(True)
    T, st, _ = _run(fx, fx["init"], with_scale=False)
    yard = K.true_pairs_error(fx)
    err = K.matrix_error(T, fx["truth"])
    print("rigid: %d iterations, error %.3e, true pairs %.3e" % (st["iterations"], err, yard))
    assert st["converged"] and err <= 16 * yard
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() <= 1e-14               # no scale crept in


def test_min_pairs_raises_when_the_start_is_far_off():
    fx = K.fixture()
    with pytest.raises(ValueError, match="too far off"):
        _run(fx, fx["far"])


def test_default_gates_come_from_the_cloud():
    fx = K.fixture()
    target = align.AlignTarget(fx["gt"], DEV)
    st = {}
    T = align.icp_similarity(fx["src"], target, fx["init"], stats=st)                # numpy source: moved to the target's device
    lo, hi = fx["gt"].min(0), fx["gt"].max(0)
    assert st["gate0"] == float(np.float32(0.2 * (hi - lo).max()))
    # 12 000 points on 12.5 units of area: spacing about 0.5 sqrt(area / n) = 0.016 (a Poisson surface sample)
    assert 0.008 < target.spacing() < 0.032 and st["gate_min"] == 4 * target.spacing()
    assert K.matrix_error(T, fx["truth"]) <= 16 * K.true_pairs_error(fx)


# ---------------------------------------------------------------------------------------------------
# the command line, end to end
# ---------------------------------------------------------------------------------------------------
def test_estimate_sfm2gt_command(tmp_path, capsys):
    import yaml

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import estimate_sfm2gt
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    scene = os.path.join(ROOT, "tests", "golden", "cache_scene")
    cfg_before = open(os.path.join(scene, "config.yaml"), "rb").read()
    case = K.scene_case(os.path.join(scene, "dense", "sparse", "points3D.bin"))
    gt_path, pairs_path, out = str(tmp_path / "gt.ply"), str(tmp_path / "pairs.txt"), str(tmp_path / "out")
    ply.write(gt_path, case["gt"])
    np.savetxt(pairs_path, case["pairs"], fmt="%.17g")
    T, rep = estimate_sfm2gt.main(["--data_dir", scene, "--gt_pcd_path", gt_path, "--pairs", pairs_path, "--track_length", "0",
                                   "--reproj_error", "1e9", "--out_dir", out])
    assert "reproj_error.py" in capsys.readouterr().out
    written = np.array(yaml.safe_load(open(os.path.join(out, "sfm2gt.yaml")))["sfm2gt"])
    assert np.array_equal(written, T)
    yard = K.matrix_error(align.similarity_from_pairs(case["src"], K.apply(case["truth"], case["src"])), case["truth"])
    err = K.matrix_error(written, case["truth"])
    print("command: %d iterations, %d pairs, error %.3e, true pairs %.3e" % (rep["iterations"], rep["pairs"], err, yard))
    assert err <= 16 * yard
    saved = json.load(open(os.path.join(out, "report.json")))
    for key in ("initial_matrix", "matrix", "correction", "iterations", "pairs", "inlier_share", "rms", "matched_bbx", "gate0",
                "gate_min", "converged", "history"):
        assert key in saved, key
    assert set(saved["correction"]) == {"scale", "rotation_deg", "translation"}
    assert saved["source_points"] == len(case["src"]) == saved["pairs"] and saved["inlier_share"] == 1.0
    own = K.apply(case["truth"], case["src"])
    assert np.allclose(saved["matched_bbx"], [own.min(0), own.max(0)], rtol=0, atol=1e-9)
    assert 0 < saved["correction"]["rotation_deg"] < 5 and abs(saved["correction"]["scale"] - 1) < 0.05
    assert open(os.path.join(scene, "config.yaml"), "rb").read() == cfg_before      # untouched without --write_config
    assert not os.path.exists(os.path.join(scene, "config.yaml.bak"))
