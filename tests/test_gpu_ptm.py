"""GPU: exact point-to-triangle-mesh distances (csrc/ncw_ptm.hip through evalmesh.mesh_distances) against the numpy float64
restatement of the contract (tests/_ptm_ref.py, a brute force over all pairs).

Numerical bound: |d - d_ref| <= 16 eps64 C, C = the largest |recentred coordinate| over vertices and queries.  The
restatement's own error is below 1 eps64 C (tests/test_ptm_host.py, against longdouble); the kernel may contract products
into FMAs and sum in another order; sixteen times that leaves room and is still about 1e-15 of the scene.
Index rule: idx equals the reference's first argmin where the reference's best d^2 is an exact tie (shared edges and
vertices: the tie rule) or where the gap to the next distinct distance exceeds the bound; elsewhere (at most 2 % of a case's
queries; the reference alone gives 0 %) the returned triangle's reference distance is within the bound of the minimum.
Closest point: |q - closest| equals dist and the reference distance from closest to the returned triangle is 0, both within
the bound.  Repeated calls and chunked calls (chunk=257) are bit-identical.  Every test prints its measured maximum in
units of eps64 C."""
import numpy as np
import pytest
import torch

from neuralrecon_w_amd import evalmesh
from tests import _ptm_ref as R

pytestmark = pytest.mark.gpu

EPS = R.EPS64
DEV = "cuda:0"


def _run(v, f, q, **kw):
    out = evalmesh.mesh_distances(torch.from_numpy(np.ascontiguousarray(v)).to(DEV), torch.from_numpy(np.ascontiguousarray(f)).to(DEV),
                                  torch.from_numpy(np.ascontiguousarray(q)).to(DEV), return_closest=True, **kw)
    assert out[0].dtype == torch.float64 and out[1].dtype == torch.int64 and out[2].dtype == torch.float64
    assert out[0].shape == (q.shape[0],) and out[1].shape == (q.shape[0],) and out[2].shape == (q.shape[0], 3)
    return out


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _check(name, v, f, q, box=None, rep=0.0, **kw):
    """Runs the case three times (twice whole, once in chunks of 257) and checks it against the reference.  `rep`: what
    the closest point loses by being returned in the caller's coordinates (0 unless those are far from the centre)."""
    st = {}
    out = _run(v, f, q, box=box, stats=st, **kw)
    assert _same(out, _run(v, f, q, box=box, **kw)), "repeated calls differ"
    if q.shape[0] > 257:
        assert _same(out, _run(v, f, q, box=box, chunk=257, **kw)), "chunked calls differ"
    d, i, cp = (t.cpu().numpy() for t in out)
    c = R.centre_of(v, q)
    C = R.coord_scale(v, q, c)
    bound = 16 * EPS * C
    ref = R.mesh_ref(v, f, q, c, box=box)
    err = np.abs(d - ref["dist"])
    assert ((i >= 0) & (i < f.shape[0])).all() and ref["valid"][i].all(), "an invalid triangle was returned"
    must = ref["tie"] | (ref["next"] - ref["dist"] > bound)
    d_of_i = R.pair_dist(v, f, q, i, c)
    back = np.abs(np.linalg.norm(q - cp, axis=1) - d)
    on_tri = R.pair_dist(v, f, cp, i, c)
    print("%s: |d - d_ref| %.2f, |d_ref(idx) - d_ref| %.2f, ||q - closest| - d| %.2f, d_ref(closest, idx) %.2f eps64 C; "
          "ties %.1f %%, elsewhere %.2f %%; %s" % (name, err.max() / (EPS * C), np.abs(d_of_i - ref["dist"]).max() / (EPS * C),
                                                   back.max() / (EPS * C), on_tri.max() / (EPS * C), 100 * ref["tie"].mean(),
                                                   100 * (~must).mean(), st))
    assert err.max() <= bound
    assert (i[must] == ref["idx"][must]).all(), int((i[must] != ref["idx"][must]).sum())
    assert (~must).mean() <= 0.02
    assert (np.abs(d_of_i - ref["dist"]) <= bound).all()
    assert back.max() <= bound + rep and on_tri.max() <= bound + rep
    return d, i, cp, st, ref


MESH = R.height_field(24, seed=1)


def test_interior_queries_name_their_source_triangle():
    v, f = MESH
    assert f.shape[0] == 1058
    q, src = R.interior_queries(v, f, 4000, seed=1)
    _, i, _, st, ref = _check("interior", v, f, q)
    assert not ref["tie"].any() and (ref["idx"] == src).all()  # the reference is 100 % clear here
    assert (i == src).all()
    assert st["cells"] > 1 and st["escaped"] == 0


def test_uniform_queries_shared_edges_and_vertices():
    v, f = MESH
    q = R.uniform_queries(v, 4000, seed=2)
    _, _, _, st, ref = _check("uniform", v, f, q)
    assert ref["tie"].mean() > 0.05  # heavy in exact ties
    assert st["pairs"] >= f.shape[0]


@pytest.mark.parametrize("n", [1, 257])
def test_one_triangle(n):
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.3]])
    f = np.array([[0, 1, 2]])
    q = R.uniform_queries(v, n, seed=3)
    _, i, _, st, _ = _check("F=1 N=%d" % n, v, f, q)
    assert (i == 0).all()


def test_single_cell_grid():
    v, f = MESH
    q = R.uniform_queries(v, 1000, seed=4)
    _, _, _, st, _ = _check("single cell", v, f, q, target_cells=1)
    assert st["dims"] == [1, 1, 1] and st["escaped"] == 0  # the block covers the grid at shell 0


def test_non_cubic_extents():
    v, f = MESH
    v = v * np.array([100.0, 1.0, 0.03])  # 100 x 1 x 0.01
    ext = v.max(0) - v.min(0)
    assert ext[0] > 99 and 0.9 < ext[1] < 1.1 and ext[2] < 0.011
    q = R.uniform_queries(v, 2000, seed=5, pad=0.05)
    _, _, _, st, _ = _check("100 x 1 x 0.01", v, f, q)
    assert st["dims"][0] > st["dims"][1] >= st["dims"][2]


def test_large_triangle_list():
    v, f = MESH
    big = np.array([[-1.0, -1.0, -0.25], [3.0, -1.0, -0.25], [-1.0, 3.0, -0.25]])  # one triangle under the whole mesh
    v2 = np.concatenate([v, big])
    f2 = np.concatenate([f[:500], [[v.shape[0], v.shape[0] + 1, v.shape[0] + 2]], f[500:]])
    q = R.uniform_queries(v, 3000, seed=6)
    d, i, cp, st, _ = _check("large list", v2, f2, q, max_cells_per_tri=8)
    assert st["large"] > 0
    assert (i == 500).any() and (i != 500).any()
    st0 = {}
    d0, i0, cp0 = _run(v2, f2, q, stats=st0, max_cells_per_tri=evalmesh.PTM_NO_LARGE)
    assert st0["large"] == 0 and st0["pairs"] > st["pairs"]
    assert np.array_equal(d, d0.cpu().numpy()) and np.array_equal(i, i0.cpu().numpy()) and np.array_equal(cp, cp0.cpu().numpy())


@pytest.mark.parametrize("n_side", [24, 6], ids=["F above the brute tile", "F below one tile"])
def test_far_queries_escape_to_the_brute_path(n_side):
    v, f = R.height_field(n_side, seed=1)
    assert (f.shape[0] > 128) == (n_side == 24)
    rng = np.random.RandomState(7)
    q = R.uniform_queries(v, 600, seed=7)
    far = rng.rand(600) < 0.5
    q[far] += np.array([1000.0, 0.0, 0.0])  # in place: every query keeps its position in the outputs
    _, _, _, st, _ = _check("far, F=%d" % f.shape[0], v, f, q, max_shell=1, target_cells=4096)
    assert st["escaped"] > 0


def test_copies_of_one_triangle_tie_to_the_first():
    v, f = MESH
    f2 = np.concatenate([f[:100], np.repeat(f[700:701], 1000, 0), f[100:]])
    q, _ = R.interior_queries(v, f[700:701], 500, seed=8)
    _, i, _, _, ref = _check("1000 copies", v, f2, q)
    assert ref["tie"].all()
    assert (i == 100).all()  # the first copy


def _degenerate_mesh():
    v, f = R.height_field(8, seed=1)
    nv = v.shape[0]
    a, b = np.array([0.125, 0.25, 0.375]), np.array([0.875, -0.5, 0.5])  # dyadic: a + (b - a) / 4 is exactly collinear
    up, down = np.array([0.0, 0.5, 0.5]), np.array([0.0, 0.5, -0.75])
    extra = np.stack([a + up, b + up,                                      # a segment above the mesh: nv, nv+1
                      a + down, a + 0.25 * (b - a) + down, b + down,       # three collinear corners below it: nv+2 .. nv+4
                      [0.5, 1.15, 0.0],                                    # a point beside it: nv+5
                      [np.nan, 0.0, 0.0]])                                 # nv+6
    v2 = np.concatenate([v, extra])
    degenerate = [[nv, nv, nv + 1], [nv + 2, nv + 3, nv + 4], [nv + 5, nv + 5, nv + 5]]
    invalid = [[-1, 0, 1], [0, 1, v2.shape[0]], [0, 1, nv + 6]]
    f2 = np.concatenate([invalid, f[:40], degenerate, f[40:], invalid])
    return v2, f2, 3 + 40


def test_degenerate_and_invalid_triangles():
    v, f, k = _degenerate_mesh()
    q = R.uniform_queries(v[np.isfinite(v).all(1)], 3000, seed=9)
    _, i, _, _, ref = _check("degenerate / invalid", v, f, q)
    assert ref["valid"].sum() == f.shape[0] - 6
    assert (i == k).any() and (i == k + 1).any() and (i == k + 2).any()  # each answers the queries next to it
    assert not np.isin(i, [0, 1, 2, f.shape[0] - 3, f.shape[0] - 2, f.shape[0] - 1]).any()


def test_all_faces_invalid_raises():
    v, f, _ = _degenerate_mesh()
    bad = np.concatenate([f[:3], f[-3:]])
    with pytest.raises(ValueError):
        evalmesh.mesh_distances(torch.from_numpy(v).to(DEV), torch.from_numpy(bad).to(DEV), torch.zeros(5, 3, dtype=torch.float64, device=DEV))
    d, i = evalmesh.mesh_distances(v, bad, np.zeros((0, 3)))  # an empty query answers before the mesh is looked at
    assert d.shape == (0,) and i.shape == (0,) and d.is_cuda


def test_offset_coordinates():
    """Coordinates on a 2^-20 lattice, so that adding the offset is exact: the recentred coordinates are then the same numbers
    with and without it, and so are the distances and triangles.  The closest points come back in the caller's coordinates,
    where one rounding costs eps64 |coordinate| / 2 per axis (`rep`)."""
    quantum = 2.0 ** -20
    v, f = R.height_field(24, seed=1, quantum=quantum)
    q = np.round(R.uniform_queries(v, 2000, seed=10) / quantum) * quantum
    off = np.array([1000.0, -2000.0, 1500.0])
    rep = 2 * EPS * 2001.0
    d0, i0, cp0, _, _ = _check("no offset", v, f, q)
    d1, i1, cp1, _, _ = _check("offset", v + off, f, q + off, rep=rep)
    C = R.coord_scale(v, q, R.centre_of(v, q))
    print("offset: |d - d0| %.2f eps64 C" % (np.abs(d1 - d0).max() / (EPS * C)))
    assert np.abs(d1 - d0).max() <= 16 * EPS * C and (i1 == i0).all()
    assert np.abs((cp1 - off) - cp0).max() <= 16 * EPS * C + rep


def test_box_crop():
    v, f = MESH
    box = [[0.25, 0.25, -1.0], [0.75, 0.75, 1.0]]
    q = R.uniform_queries(v, 3000, seed=11)
    _, i, _, _, ref = _check("box", v, f, q, box=box)
    t = v[f[i]]
    assert ((t >= np.array(box[0])) & (t <= np.array(box[1]))).all()
    assert 0 < ref["valid"].sum() < f.shape[0]
