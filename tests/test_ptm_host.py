"""Host-side checks of the exact point-to-triangle distances (csrc/ncw_ptm.hip): the numpy restatement of the contract
(tests/_ptm_ref.py) against its own run in extended precision and against an independently written closest-point routine,
the degenerate cases, the command-line flag and the ctypes mirror of the grid struct.  No GPU."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import _ptm_ref as R
from tests._util import ROOT

EPS = R.EPS64


def _cases():
    v, f = R.height_field(24, seed=1)
    uni = R.uniform_queries(v, 600, seed=2)
    near, _ = R.interior_queries(v, f, 600, seed=1)
    # a sliver: two corners 1e-9 apart; queries in the box 0.2 beyond the mesh, as in the uniform case (the bound is in units
    # of C, so the distances must stay within the scene's own scale: rounding the final sqrt alone costs eps64 d / 2)
    sv = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1e-9, 0.0], [0.3, 0.7, 0.2]])
    sf = np.array([[0, 1, 2], [0, 2, 3]])
    sq = R.uniform_queries(sv, 600, seed=5)
    return [("uniform", v, f, uni), ("interior", v, f, near), ("sliver", sv, sf, sq)]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_restatement_against_longdouble(case):
    """The float64 restatement is within 1 eps64 C of the same code in longdouble on the same recentred float64 inputs
    (C = the largest |recentred coordinate| over vertices and queries).  Measured: 0.94 (uniform), 0.84 (1e-9 sliver)."""
    _, v, f, q = case
    c = R.centre_of(v, q)
    C = R.coord_scale(v, q, c)
    a = R.mesh_ref(v, f, q, c)
    b = R.mesh_ref(v, f, q, c, dtype=np.longdouble)
    err = float(np.abs(a["dist"] - b["dist"]).max()) / (EPS * C)
    print("max |d64 - d80| = %.3f eps64 C" % err)
    assert err <= 1.0


def _ericson(p, a, b, c):
    """Closest point on triangle abc to p, by Voronoi region (C. Ericson, Real-Time Collision Detection, 5.1.5), written for
    row-wise arrays [n,3] with masks; independent of the restatement (barycentric form, no face / segment split)."""
    dot = lambda x, y: (x * y).sum(-1)
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = p - b
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = p - c
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    out = np.full(p.shape, np.nan)
    todo = np.ones(p.shape[0], bool)

    def take(mask, val):
        m = todo & mask
        out[m] = val[m]
        todo[m] = False

    with np.errstate(all="ignore"):
        take((d1 <= 0) & (d2 <= 0), a)
        take((d3 >= 0) & (d4 <= d3), b)
        take((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (d1 / (d1 - d3))[:, None] * ab)
        take((d6 >= 0) & (d5 <= d6), c)
        take((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (d2 / (d2 - d6))[:, None] * ac)
        take((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * (c - b))
        den = 1.0 / (va + vb + vc)
        take(np.ones_like(todo), a + ab * (vb * den)[:, None] + ac * (vc * den)[:, None])
    return out


def test_restatement_against_region_based_closest_point():
    """Per (query, triangle) pair on the well-shaped triangles of the height field (minimum angle about 14 degrees): the
    restatement's distance equals |p - ericson(p)|.  Bound 256 eps64 C: the barycentric weights are ratios of differences of
    products of dot products, each a few eps relative, amplified by 1 / sin^2(minimum angle) < 20."""
    v, f = R.height_field(24, seed=1)
    assert 8.0 < R.min_angle_deg(v, f) < 25.0
    rng = np.random.RandomState(3)
    q = R.uniform_queries(v, 20000, seed=4)
    idx = rng.randint(0, f.shape[0], q.shape[0])
    c = R.centre_of(v, q)
    C = R.coord_scale(v, q, c)
    d = R.pair_dist(v, f, q, idx, c)
    t = v[f[idx]] - c
    e = np.linalg.norm((q - c) - _ericson(q - c, t[:, 0], t[:, 1], t[:, 2]), axis=1)
    err = float(np.abs(d - e).max()) / (EPS * C)
    print("max |d - d_ericson| = %.2f eps64 C" % err)
    assert err <= 256.0


def _seg_dist(p, u, w):
    d = w - u
    l = (d * d).sum()
    s = 0.0 if l == 0 else min(1.0, max(0.0, ((p - u) * d).sum(-1) / l))
    return np.linalg.norm(p - (u + np.asarray(s)[..., None] * d), axis=-1)


def test_degenerate_triangles_equal_segment_or_point_distance():
    rng = np.random.RandomState(7)
    q = rng.uniform(-2, 2, (500, 3))
    a, b = np.array([0.125, 0.25, 0.375]), np.array([0.875, -0.5, 0.5])
    mid = a + 0.25 * (b - a)  # dyadic coordinates: exactly collinear with a, b, the cross product is exactly zero
    c = np.zeros(3)
    cases = {
        "two equal corners": (np.stack([a, a, b]), [_seg_dist(p, a, b) for p in q]),
        "collinear corners": (np.stack([a, mid, b]), [_seg_dist(p, a, b) for p in q]),
        "all corners equal": (np.stack([a, a, a]), [np.linalg.norm(p - a) for p in q]),
    }
    for name, (v, want) in cases.items():
        r = R.mesh_ref(v, np.array([[0, 1, 2]]), q, c)
        err = float(np.abs(r["dist"] - np.array(want)).max()) / (EPS * 2.0)
        print("%s: %.2f eps64 C" % (name, err))
        assert err <= 16.0, name
        assert (r["idx"] == 0).all()
        # the closest point lies on the segment / is the point
        back = np.linalg.norm(q - r["closest"], axis=1)
        assert np.abs(back - r["dist"]).max() <= 16 * EPS * 2.0, name


def test_reference_cases_are_clear():
    """What the GPU cases rely on: over triangle interiors the reference names the source triangle every time; on uniform
    queries every minimum is either an exact tie (shared edge / vertex: bit-identical d^2 by the canonical endpoint order) or
    clear of the next distinct distance by more than the bound."""
    v, f = R.height_field(24, seed=1)
    assert f.shape[0] == 1058
    q, src = R.interior_queries(v, f, 1000, seed=1)
    c = R.centre_of(v, q)
    r = R.mesh_ref(v, f, q, c)
    assert (r["idx"] == src).all() and not r["tie"].any()
    q = R.uniform_queries(v, 1000, seed=2)
    c = R.centre_of(v, q)
    r = R.mesh_ref(v, f, q, c)
    bound = 16 * EPS * R.coord_scale(v, q, c)
    clear = r["tie"] | (r["next"] - r["dist"] > bound)
    print("exact ties %.1f %%, unclear %.2f %%" % (100 * r["tie"].mean(), 100 * (~clear).mean()))
    assert r["tie"].mean() > 0.05 and clear.all()


def test_validity_rule_of_the_reference():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [5, 5, 5.0]])
    f = np.array([[0, 1, 2], [0, 1, -1], [0, 1, 5], [0, 1, 3], [0, 1, 4]])
    _, ok = R.pack(v, f, np.zeros(3))
    assert ok.tolist() == [True, False, False, False, True]
    _, ok = R.pack(v, f, np.zeros(3), box=[[0, 0, 0], [1, 1, 1]])
    assert ok.tolist() == [True, False, False, False, False]
    with pytest.raises(ValueError):
        R.mesh_ref(v, f[1:4], np.zeros((2, 3)), np.zeros(3))


def test_eval_mesh_cli_parses_exact_recall():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import eval_mesh as cli
    finally:
        sys.path.pop(0)
    base = ["--file_pred", "a.ply", "--file_trgt", "b.ply", "--scene_config_path", "c.yaml"]
    assert cli.get_opts(base).exact_recall is False
    assert cli.get_opts(base + ["--exact_recall"]).exact_recall is True
    a = cli.get_opts(base + ["--exact_recall", "--sample_surface"])
    assert a.exact_recall is True and a.sample_surface == 10


def test_eval_pipeline_refuses_exact_recall():
    """reprojected.ply is a point cloud: the pipeline refuses the flag with a message that says so, before any work."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_pipeline.py"), "--scene_name", "brandenburg_gate",
                        "--pred_dir", os.path.join(tempfile.gettempdir(), "no_such_run"), "--exact_recall"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0
    assert "point cloud" in r.stderr and "--exact_recall" in r.stderr


def test_ptm_grid_struct_size_matches_c_layout():
    from neuralrecon_w_amd import lib as L

    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "neuconw_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n", ' \
           'sizeof(NcwPtmGrid), offsetof(NcwPtmGrid, h), offsetof(NcwPtmGrid, inv_h), offsetof(NcwPtmGrid, dim));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size, o_h, o_inv, o_dim = map(int, subprocess.check_output([exe]).decode().split())
    assert ctypes.sizeof(L.NcwPtmGrid) == size
    assert (L.NcwPtmGrid.h.offset, L.NcwPtmGrid.inv_h.offset, L.NcwPtmGrid.dim.offset) == (o_h, o_inv, o_dim)


def test_entry_points_refuse_bad_arguments_without_a_launch():
    """NULL pointers, a bad grid and counts out of range give NCW_E_BADARG; an empty range gives 0.  Neither launches, so
    this runs without a GPU (the pointers handed in are never dereferenced)."""
    from neuralrecon_w_amd import lib as L

    lib = L.get_lib()
    g = L.NcwPtmGrid()
    for a in range(3):
        g.lo[a], g.dim[a] = 0.0, 4
    g.h, g.inv_h = 0.25, 4.0
    bad = L.NcwPtmGrid()  # h = 0, dim = 0
    p = ctypes.c_void_p(4096)  # non-NULL, never read
    c3 = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    G, B = ctypes.byref(g), ctypes.byref(bad)
    calls = {
        "pack": (lambda n, x=p: lib.ncw_ptm_pack(p, 3, x, n, c3, None, p, p, None)),
        "count": (lambda n, x=p, gr=G, m=8: lib.ncw_ptm_count(x, p, n, gr, m, p, p, None)),
        "emit": (lambda n, x=p, gr=G: lib.ncw_ptm_emit(x, p, p, n, gr, n, p, p, None)),
        "ranges": (lambda n, x=p, c=64: lib.ncw_ptm_ranges(x, p, p, n, c, p, p, None)),
        "cell_keys": (lambda n, x=p, gr=G: lib.ncw_ptm_cell_keys(x, n, gr, p, None)),
        "query": (lambda n, x=p, gr=G, sh=8, mg=0.0, nl=0: lib.ncw_ptm_query(x, 10, p, p, None, nl, p, p, n, gr, sh, mg, p, p, None, p, p,
                                                                              None)),
        "brute": (lambda n, x=p: lib.ncw_ptm_brute(x, p, 10, p, 5, p, n, p, p, p, None, None)),
    }
    for name, fn in calls.items():
        assert fn(0) == 0, name                      # empty range: 0 without a launch
        assert fn(1, None) == -1, name               # NULL pointer
        assert fn(-1) == -1 and fn(1 << 31) == -1, name  # counts out of range
    for name in ("count", "emit", "cell_keys", "query"):
        assert calls[name](1, p, B) == -1, name       # bad grid
    assert calls["count"](1, p, G, 0) == -1 and calls["count"](1, p, G, (1 << 30) + 1) == -1
    assert calls["ranges"](1, p, 0) == -1
    assert calls["query"](1, p, G, -1) == -1 and calls["query"](1, p, G, 8, -1.0) == -1 and calls["query"](1, p, G, 8, float("nan")) == -1
    assert calls["query"](1, p, G, 8, 0.0, 3) == -1  # a large list without its ids
    assert calls["brute"](6) == -1                    # more escaped queries than queries


def test_no_cpu_fallback():
    import torch

    from neuralrecon_w_amd import evalmesh
    from neuralrecon_w_amd.lib import NeuconwHipError

    v, f = R.height_field(4)
    if not torch.cuda.is_available():
        with pytest.raises(NeuconwHipError):
            evalmesh.mesh_distances(v, f, np.zeros((3, 3)))
    with pytest.raises(NeuconwHipError):  # host tensors are refused with or without a GPU
        evalmesh.TriGrid(torch.from_numpy(v), torch.from_numpy(f).int(), np.zeros(3), 1.0)
    c, cmax = evalmesh.ptm_centre(torch.from_numpy(v), torch.zeros(2, 3, dtype=torch.float64))
    assert np.array_equal(c, R.centre_of(v, np.zeros((2, 3)))) and cmax == R.coord_scale(v, np.zeros((2, 3)), c)
