"""GPU: meshops.simplify (csrc/ncw_simplify.hip) against the numpy restatement tests/_simplify_ref.py.

EXACT EQUALITY is required for everything discrete: cluster_index, faces, the vertex order (the cluster of every output vertex),
colours and the placed-at-the-mean flags.  Coordinates must lie within 4 x the restatement's own deviation from its long-double
run on that case, with a floor of one ulp of h; every case prints whether they were in fact bit-identical (the contract fixes
every rounding and every summation order, so they are expected to be).  The cases are the smallest at which the kernels can go
wrong: cluster counts around a wave and a workgroup, one very long incidence list, total collapse, rank-1 / 2 / 3 quadrics with
both placements taken, coordinates exactly on cell boundaries, faces that take no part, duplicates, both input dtypes."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import _simplify_cases as K
from tests import _simplify_ref as R
from tests._util import ROOT

from neuralrecon_w_amd import meshops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _gpu(verts, faces, h, colors=None, eps=1e-3, fdtype=torch.int64):
    st = {}
    out = meshops.simplify(_dev(verts), _dev(faces, fdtype), h, None if colors is None else _dev(colors), eps=eps, stats=st)
    return out, st


def _check(verts, faces, h, colors=None, eps=1e-3, fdtype=torch.int64, name=""):
    (v, f, c, ci), st = _gpu(verts, faces, h, colors, eps, fdtype)
    r = R.simplify(verts, faces, h, colors, eps)
    ld = R.simplify(verts, faces, h, colors, eps, dtype=np.longdouble)
    assert f.dtype == torch.int32 and ci.dtype == torch.int64 and v.dtype == _dev(verts).dtype
    assert np.array_equal(ci.cpu().numpy(), r["cluster_index"])
    assert np.array_equal(f.cpu().numpy().reshape(-1, 3), r["faces"])
    assert v.shape[0] == r["vertices"].shape[0]                          # with cluster_index: the vertex order
    assert (c is None) == (colors is None) and (c is None or np.array_equal(c.cpu().numpy(), r["colors"]))
    assert np.array_equal(st["at_mean"].cpu().numpy(), r["at_mean"])
    assert (st["clusters"], st["clusters_at_mean"]) == (r["clusters"], r["clusters_at_mean"])
    assert (st["vertices_before"], st["faces_before"], st["vertices_after"], st["faces_after"]) == (
        len(verts), len(faces), len(r["vertices"]), len(r["faces"]))
    got = v.cpu().numpy().astype(np.float64)
    own = float(np.abs(r["vertices"].astype(np.longdouble) - ld["vertices"]).max()) if len(got) else 0.0
    tol = max(4.0 * own, float(np.spacing(np.float64(h))))
    err = float(np.abs(got - r["vertices"]).max()) if len(got) else 0.0
    print("%s: %d clusters (%d at the mean), %d -> %d faces; max |gpu - restatement| %.3e, restatement vs long double %.3e, "
          "tolerance %.3e, bit-identical: %s" % (name, r["clusters"], r["clusters_at_mean"], len(faces), len(r["faces"]), err, own,
                                                 tol, bool(np.array_equal(got, r["vertices"]))))
    assert err <= tol
    return (v, f, c, ci), st, r


def _strip(C, seed):
    """C vertices, one per cell along x (h = 1), C - 2 triangles (i, i + 1, i + 2): one member per cluster, every face survives."""
    g = np.random.RandomState(seed)
    x = np.arange(C) + 0.1 + 0.8 * g.rand(C)
    x[0] = 0.0
    verts = np.stack([x, 0.9 * g.rand(C), 0.9 * g.rand(C)], -1)
    i = np.arange(C - 2)
    return verts, np.stack([i, i + 1, i + 2], -1)


@pytest.mark.parametrize("C", [63, 64, 65, 255, 256, 257])
def test_strip_one_vertex_per_cell(C):
    verts, faces = _strip(C, C)
    _, st, r = _check(verts, faces, 1.0, fdtype=torch.int32, name="strip %d" % C)   # int32 faces here, int64 everywhere else
    assert st["clusters"] == C and st["faces_after"] == C - 2 and st["vertices_after"] == C
    assert np.array_equal(r["cluster_index"], np.arange(C))


def _fan(n=2048):
    a = 2 * np.pi * np.arange(n + 1) / (n + 1)
    rim = np.stack([10 * np.cos(a), 10 * np.sin(a), 0.4 * np.sin(7 * a)], -1)
    verts = np.concatenate([rim, [[0.05, -0.02, 0.3]]])
    i = np.arange(n)
    faces = np.stack([np.full(n, n + 1), i, i + 1], -1)
    faces[1::2] = faces[1::2][:, [1, 2, 0]]                              # the hub is not always corner 0
    return verts, faces


def test_fan_long_incidence_list():
    """2048 triangles around one hub: its cluster walks 2048 incidences in one lane; the rim is spread over many cells."""
    verts, faces = _fan()
    _, st, r = _check(verts, faces, 1.0, name="fan")
    hub = r["cluster"][len(verts) - 1]
    assert (r["cluster"] == hub).sum() == 1 and st["clusters"] > 40


def test_whole_mesh_in_one_cell():
    verts, faces, _ = K.cube(2)
    cols = np.full((len(verts), 3), 7, dtype=np.uint8)
    (v, f, c, ci), st, _ = _check(verts, faces, 10.0, cols, name="one cell")
    assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3) and bool((ci == -1).all())
    assert st["clusters"] == 1 and st["faces_after"] == 0


def test_plane_and_cube_take_both_placements():
    """A tilted plane (rank-1 quadrics: only the regularisation makes the solve regular) and the offset cube at 16 quads per side
    (rank 2 along its edges, rank 3 at its corners): the regularised solve AND the fall-back to the member mean are taken."""
    verts, faces = K.plane(24)
    verts[:, 2] = 0.25 + 0.3 * verts[:, 0] + 0.2 * verts[:, 1]
    _, st_p, _ = _check(verts, faces, 0.11, name="plane")
    verts, faces, _ = K.cube(16)
    _, st_c, _ = _check(verts, faces, 0.11, name="cube 16")
    flags = torch.cat([st_p["at_mean"], st_c["at_mean"]])
    assert bool((flags == 0).any()) and bool((flags == 1).any())
    assert 0 < st_c["clusters_at_mean"] + st_p["clusters_at_mean"] < st_c["clusters"] + st_p["clusters"]


@pytest.mark.parametrize("h", [0.25, 0.5])
def test_boundary_and_clamp(h):
    """Every coordinate is a multiple of 0.25 and lo = 0: x - lo = k h exactly, the upper cell takes it; the maximal vertices
    (x = 1) open the last cell n - 1 = 1 / h on their own."""
    verts, faces, _ = K.cube(4, offset=0.0)
    _, st, r = _check(verts, faces, h, name="boundary h %g" % h)
    n = int(round(1.0 / h)) + 1
    cells = np.floor(verts / h).astype(np.int64)
    key = (cells[:, 0] * n + cells[:, 1]) * n + cells[:, 2]
    assert np.array_equal(np.unique(key, return_inverse=True)[1], r["cluster"]) and cells.max() == n - 1


def test_faces_that_take_no_part():
    """Zero-area, out-of-range and repeated-corner faces, unused vertices, int64 indices beyond int32."""
    verts, faces, _ = K.cube(8)
    V = len(verts)
    verts = np.concatenate([verts, verts[:3], [[40.0, 40.0, 40.0], [np.nan, np.inf, 0.0]]])  # 3 coincident copies, 2 unused
    extra = np.array([[0, V, 5],               # corners 0 and V coincide: zero area, takes part, adds zeros
                      [V, V + 1, V + 2],       # copies of 0, 1, 2: a face of its own indices
                      [3, 3, 4], [5, 6, V + 5], [-1, 2, 3], [1, 2, 1 << 40], [7, 2 ** 31 + 3, 9]])
    faces = np.concatenate([faces[:100], extra, faces[100:]])
    cols = np.random.RandomState(4).randint(0, 256, (len(verts), 3)).astype(np.uint8)
    (_, _, _, ci), _, r = _check(verts, faces, 0.3, cols, name="no part")
    assert ci[V + 3:].tolist() == [-1, -1] and int(ci[V]) == int(ci[0])


def test_duplicates_and_opposite_orientation():
    v = np.array([[2.5, 0, 0], [0.5, 0, 0], [1.5, 0.5, 0], [1.75, 0.25, 0.1], [0.75, 0.1, 0.2], [2.75, 0.3, 0.1]])
    # clusters along x (h = 1, lo = 0.5): vertex 0 -> 2, 1 -> 0, 2 -> 1, 3 -> 1, 4 -> 0, 5 -> 2
    two = np.array([[0, 1, 2], [5, 4, 3]])
    (_, f, _, _), _, _ = _check(v, two, 1.0, name="two duplicates")
    assert f.tolist() == [[0, 1, 2]]
    three = np.array([[2, 0, 1], [5, 4, 3], [4, 3, 5], [3, 4, 5], [1, 2, 0]])
    (_, f, _, _), _, _ = _check(v, three, 1.0, name="three duplicates + opposite")
    assert f.tolist() == [[0, 1, 2], [0, 2, 1]]                          # face 0 wins over 1, 2, 4; face 3 is the opposite pair
    (_, f, _, _), _, _ = _check(v, three[::-1].copy(), 1.0, name="reversed order")
    assert f.tolist() == [[0, 1, 2], [0, 2, 1]]


def test_float32_input():
    verts, faces, _ = K.cube(16)
    v32 = verts.astype(np.float32)
    (a, fa, _, cia), st_a = _gpu(v32, faces, 0.11)
    (b, fb, _, cib), st_b, _ = _check(v32.astype(np.float64), faces, 0.11, name="float32 values")
    assert a.dtype == torch.float32 and b.dtype == torch.float64
    assert torch.equal(a, b.to(torch.float32)) and torch.equal(fa, fb) and torch.equal(cia, cib)
    assert torch.equal(st_a["at_mean"], st_b["at_mean"])


def test_colours_round_half_up():
    verts, faces, _ = K.cube(8)
    cols = np.random.RandomState(6).randint(0, 4, (len(verts), 3)).astype(np.uint8)
    _, _, r = _check(verts, faces, 0.3, cols, name="colours")
    s = np.zeros((r["clusters"], 3), dtype=np.int64)
    np.add.at(s, r["cluster"], cols.astype(np.int64))
    n = np.bincount(r["cluster"], minlength=r["clusters"])[:, None]
    assert ((2 * s) % (2 * n) == n).sum() >= 5                           # sum / count lands on .5 in several cells


def test_determinism():
    verts, faces = _fan()
    cols = np.random.RandomState(8).randint(0, 256, (len(verts), 3)).astype(np.uint8)
    a, sa = _gpu(verts, faces, 1.0, cols)
    b, sb = _gpu(verts, faces, 1.0, cols)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(sa["at_mean"], sb["at_mean"])
    verts, faces, _ = K.cube(16)
    a, b = _gpu(verts, faces, 0.11)[0], _gpu(verts, faces, 0.11)[0]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])


def test_no_participating_face_is_refused():
    verts = torch.zeros(6, 3, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="no face takes part"):
        meshops.simplify(verts, torch.tensor([[0, 0, 1], [2, 3, 6]], device=DEV), 1.0)
    with pytest.raises(ValueError, match="2\\^62"):
        meshops.simplify(torch.rand(6, 3, dtype=torch.float64, device=DEV), torch.tensor([[0, 1, 2], [3, 4, 5]], device=DEV), 1e-300)


def test_extract_mesh_end_to_end(monkeypatch):
    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import mesh
    from tests._build import build_system

    emb, neuconw, nerf, rdr = build_system(seed=2, prec=nw.PREC_F32)      # geometric init: a sphere of radius ~0.5
    kw = dict(dim=48, scene_radius=2.0, scene_origin=[1.0, 2.0, 3.0], with_color=True, embedding_a=emb.weight[3].detach())
    plain = mesh.extract_mesh(rdr, **kw)
    off = mesh.extract_mesh(rdr, simplify_cells=0, **kw)
    for key in ("vertices", "faces", "vertices_training", "colors"):
        assert torch.equal(plain[key], off[key]), key
    calls = []
    real = meshops.simplify

    def spy(vertices, faces, cell, *a, **k):
        out = real(vertices, faces, cell, *a, **k)
        calls.append((vertices, faces, cell, out))
        return out

    monkeypatch.setattr(meshops, "simplify", spy)
    simp = mesh.extract_mesh(rdr, simplify_cells=2, **kw)
    assert len(calls) == 1 and calls[0][2] == 2.0
    F, V = simp["faces"].shape[0], simp["vertices"].shape[0]
    assert 0 < F < plain["faces"].shape[0] and V < plain["vertices"].shape[0]
    assert simp["colors"].shape == (V, 3) and simp["colors"].dtype == torch.uint8
    assert int(simp["faces"].min()) == 0 and int(simp["faces"].max()) == V - 1
    # every output vertex lies inside the cell of the vertices it stands for (grid-index units, h = 2)
    x, f, h, (v_new, _, _, ci) = calls[0]
    x, v_new, ci = x.double().cpu().numpy(), v_new.double().cpu().numpy(), ci.cpu().numpy()
    lo = x[np.unique(f.cpu().numpy())].min(0)
    centre = lo + (np.floor((x - lo) / h) + 0.5) * h
    m = ci >= 0
    assert m.sum() > 1000
    assert np.abs(v_new[ci[m]] - centre[m]).max() <= h / 2 + 1e-5        # float32 output: half an ulp of a coordinate < 48


def test_clean_mesh_command(tmp_path, capsys):
    from neuralrecon_w_amd import ply

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import clean_mesh
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    verts, faces, _ = K.cube(16)
    verts = np.concatenate([verts, [[3.0, 3.0, 3.0], [3.1, 3.0, 3.0], [3.0, 3.1, 3.0]]])  # a floater of one face
    faces = np.concatenate([faces, [[len(verts) - 3, len(verts) - 2, len(verts) - 1]]])
    cols = np.random.RandomState(3).randint(0, 256, (len(verts), 3)).astype(np.uint8)
    src, plain, simp, want = (str(tmp_path / n) for n in ("in.ply", "plain.ply", "simp.ply", "want.ply"))
    ply.write(src, verts, faces, rgb=cols)
    # what the command has always written: the clean-up alone
    v, f, c, _ = meshops.clean(_dev(verts), _dev(faces), _dev(cols), 2, None)
    ply.write(want, v.cpu().numpy(), f.cpu().numpy(), rgb=c.cpu().numpy())
    clean_mesh.main(["--file_in", src, "--file_out", plain, "--min_component_faces", "2"])
    assert open(plain, "rb").read() == open(want, "rb").read()
    assert "simplified" not in capsys.readouterr().out
    clean_mesh.main(["--file_in", src, "--file_out", simp, "--min_component_faces", "2", "--simplify_cell", "0.11"])
    out = capsys.readouterr().out
    r = R.simplify(v.cpu().numpy(), f.cpu().numpy(), 0.11, c.cpu().numpy())
    sv, sf, sc = ply.read_mesh(simp)
    assert np.array_equal(sf, r["faces"]) and np.array_equal(sc, r["colors"]) and np.abs(sv - r["vertices"]).max() <= 1e-12
    assert 0 < len(sf) < len(f) and "%d -> %d vertices, %d -> %d faces" % (len(v), len(sv), len(f), len(sf)) in out
