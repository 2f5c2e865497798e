"""GPU: the mesh operation kernels (csrc/ncw_meshops.hip through neuralrecon_w_amd.meshops) against the numpy restatement
tests/_meshops_ref.py.  Everything is integer work with a schedule-independent contract, so every comparison is EXACT EQUALITY:
labels, sizes, keep flags, compacted faces, vertices and index map.  The cases are the smallest at which the kernels can go wrong
(long find paths, one contended word, many interleaved components, invalid faces, masks, shapes around a wave and a workgroup)."""
import numpy as np
import pytest
import torch

from tests import _meshops_ref as R

from neuralrecon_w_amd import meshops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCK = 256         # the workgroup of the kernels of csrc/ncw_meshops.hip: one lane per face / vertex ...
SIZES_BLOCK = 1024  # ... but ncw_mesh_cc_sizes, whose workgroup combines its adds in LDS (128 slots: the many-components case overflows them)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _check_components(faces, V, keep=None, dtype=torch.int64):
    labels, sizes = meshops.components(_dev(faces, dtype), V, None if keep is None else _dev(np.asarray(keep, dtype=np.uint8)))
    rl, rs = R.components(faces, V, keep)
    assert labels.dtype == torch.int32 and sizes.dtype == torch.int32 and labels.shape == (V,) and sizes.shape == (V,)
    assert np.array_equal(labels.cpu().numpy(), rl), np.flatnonzero(labels.cpu().numpy() != rl)[:10]
    assert np.array_equal(sizes.cpu().numpy(), rs), np.flatnonzero(sizes.cpu().numpy() != rs)[:10]
    return labels, sizes


def _check_submesh(verts, faces, keep, colors=None):
    v, f, c, idx = meshops.submesh(_dev(verts), _dev(faces), _dev(np.asarray(keep, dtype=np.uint8)),
                                   None if colors is None else _dev(colors))
    rv, rf, rc, ridx = R.submesh(verts, faces, keep, colors)
    assert f.dtype == torch.int32 and idx.dtype == torch.int64
    assert np.array_equal(idx.cpu().numpy(), ridx) and np.array_equal(f.cpu().numpy().reshape(-1, 3), rf)
    assert np.array_equal(v.cpu().numpy(), rv) and v.dtype == _dev(verts).dtype
    assert (c is None) == (colors is None) and (c is None or np.array_equal(c.cpu().numpy(), rc))
    return v, f, c, idx


def _strip(n, index):
    """n triangles (i, i + 1, i + 2) along a strip of n + 2 vertices, vertex i of the strip renamed index[i]."""
    i = np.arange(n)
    return index[np.stack([i, i + 1, i + 2], -1)]


@pytest.mark.parametrize("order", ["random", "descending"])
def test_long_strip(order):
    """One component of 4096 triangles: long find paths, flatten, chains that cross workgroups."""
    n = 4096
    index = np.random.RandomState(11).permutation(n + 2) if order == "random" else np.arange(n + 2)[::-1].copy()
    faces = _strip(n, index)
    labels, sizes = _check_components(faces, n + 2, dtype=torch.int32)
    assert int(labels.max()) == 0 and int(sizes[0]) == n


def test_high_degree_fan():
    """2048 triangles around the vertex with the LARGEST index: contention on one atomicMin word, the retry branch."""
    n = 2048
    hub = n + 1
    i = np.arange(n)
    faces = np.stack([np.full(n, hub), i, i + 1], -1)
    faces[1::2] = faces[1::2][:, [1, 2, 0]]  # the hub is not always corner 0
    labels, sizes = _check_components(faces, n + 2)
    assert int(labels.max()) == 0 and int(sizes[0]) == n
    # the same fan with disjoint rim vertices: the hub is all that joins the faces
    faces = np.stack([np.full(n, 2 * n), 2 * i, 2 * i + 1], -1)
    labels, _ = _check_components(faces, 2 * n + 1)
    assert int(labels.max()) == 0


def _many_components(seed=5, n_comp=300):
    """About 300 strips of 1..300 faces, their faces interleaved by a seeded permutation, their vertices scattered by another;
    20 isolated vertices that no face uses."""
    rng = np.random.RandomState(seed)
    lengths = rng.randint(1, 301, n_comp)
    faces, base = [], 0
    for n in lengths:
        faces.append(_strip(n, np.arange(base, base + n + 2)))
        base += n + 2
    V = base + 20
    rename = rng.permutation(V)
    faces = rename[np.concatenate(faces)]
    return faces[rng.permutation(len(faces))], V, lengths


def test_many_small_components_and_reproducibility():
    faces, V, lengths = _many_components()
    labels, sizes = _check_components(faces, V)
    s = sizes.cpu().numpy()
    assert (s > 0).sum() == len(lengths) and sorted(s[s > 0].tolist()) == sorted(lengths.tolist())
    lab = labels.cpu().numpy()
    assert (lab[s == 0] != np.flatnonzero(s == 0)).sum() == V - 20 - len(lengths)  # 20 isolated vertices label themselves
    # the largest case again: bit-identical
    labels2, sizes2 = meshops.components(_dev(faces), V)
    assert torch.equal(labels, labels2) and torch.equal(sizes, sizes2)
    ok = meshops.select_components(sizes, min_faces=150)
    keep = meshops.face_select(_dev(faces), V, labels=labels, comp_ok=ok)
    rk = R.face_select(faces, V, None, 1, lab, R.select_components(s, min_faces=150))
    assert np.array_equal(keep.cpu().numpy(), rk) and 0 < rk.sum() < len(faces)
    verts = np.random.RandomState(1).rand(V, 3).astype(np.float32)
    cols = np.random.RandomState(2).randint(0, 256, (V, 3)).astype(np.uint8)
    a = _check_submesh(verts, faces, rk, cols)
    b = meshops.submesh(_dev(verts), _dev(faces), keep, _dev(cols))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # clean() is the same chain
    st = {}
    c = meshops.clean(_dev(verts), _dev(faces), _dev(cols), min_component_faces=150, stats=st)
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    assert st == {"components_before": len(lengths), "components_after": int((lengths >= 150).sum()),
                  "faces_before": len(faces), "faces_after": int(rk.sum())}


def _octahedron(base, centre):
    p = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64) + centre
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]) + base
    return p, f


def test_touching_and_coincident_closed_meshes():
    """Two closed meshes that touch in one WELDED vertex are one component; with that vertex duplicated (same coordinates,
    two indices) they are two: connectivity goes by index, not by coordinates."""
    pa, fa = _octahedron(0, [0, 0, 0])
    pb, fb = _octahedron(6, [2, 0, 0])  # b's vertex 7 (-1, 0, 0) + (2, 0, 0) coincides with a's vertex 0
    assert np.array_equal(pa[0], pb[1])
    dup = np.concatenate([fa, fb])
    labels, sizes = _check_components(dup, 12)
    assert sorted(set(labels.tolist())) == [0, 6] and int(sizes[0]) == 8 and int(sizes[6]) == 8
    welded = np.where(dup == 7, 0, dup)
    labels, sizes = _check_components(welded, 12)
    assert sorted(set(labels.tolist())) == [0, 7] and int(sizes[0]) == 16  # vertex 7 is unused now: its own label


def test_invalid_faces_are_never_kept_hooked_or_counted():
    V = 40
    rng = np.random.RandomState(3)
    faces = _strip(30, np.arange(32)).astype(np.int64)
    faces[4] = [4, 5, V]            # out of range (would join nothing, but must not be read)
    faces[9] = [9, 9, 11]           # repeated corner
    faces[14] = [-1, 15, 16]        # negative
    faces[19] = [19, 20, 1 << 40]   # beyond int32: must not wrap into range
    faces[20] = [20, 22, 22]
    faces[21] = [21, 2 ** 31 + 3, 23]
    faces = faces[rng.permutation(len(faces))]
    labels, sizes = _check_components(faces, V)
    assert int(sizes.sum()) == 24
    keep = meshops.face_select(_dev(faces), V)
    assert np.array_equal(keep.cpu().numpy(), R.face_select(faces, V)) and int(keep.sum()) == 24
    verts = rng.rand(V, 3)
    _, f, _, _ = _check_submesh(verts, faces, np.ones(len(faces), dtype=np.uint8))  # an all-ones mask still drops them
    assert f.shape[0] == 24 and int(f.min()) >= 0


def test_masked_component():
    """A keep mask that cuts a component in two."""
    n = 600
    faces = _strip(n, np.random.RandomState(8).permutation(n + 2))
    keep = np.ones(n, dtype=np.uint8)
    keep[299:302] = 0  # three consecutive faces: no kept face spans the gap
    labels, sizes = _check_components(faces, n + 2, keep)
    s = sizes.cpu().numpy()
    assert sorted(s[s > 0].tolist()) == [298, 299]
    _check_components(faces, n + 2, np.zeros(n, dtype=np.uint8))  # nothing takes part: every vertex is its own label


@pytest.mark.parametrize("F", [1, 63, 64, 65, BLOCK + 1, SIZES_BLOCK + 1])
def test_shape_edges(F):
    rng = np.random.RandomState(F)
    V = F + 7
    faces = rng.randint(0, V, (F, 3))  # random corners: some faces repeat one and are invalid
    labels, sizes = _check_components(faces, V)
    flags = rng.randint(0, 2, V).astype(np.uint8)
    keep = meshops.face_select(_dev(faces), V, vflags=_dev(flags), min_corners=2)
    rk = R.face_select(faces, V, flags, 2)
    assert np.array_equal(keep.cpu().numpy(), rk)
    _check_submesh(rng.rand(V, 3), faces, rk)


@pytest.mark.parametrize("min_corners", [1, 2, 3])
def test_face_rule(min_corners):
    rng = np.random.RandomState(21)
    V, F = 700, 3000
    faces = rng.randint(0, V, (F, 3))
    flags = (rng.rand(V) < 0.4).astype(np.uint8) * rng.randint(1, 256, V).astype(np.uint8)  # any nonzero value counts
    keep = meshops.face_select(_dev(faces), V, vflags=_dev(flags), min_corners=min_corners)
    rk = R.face_select(faces, V, flags, min_corners)
    assert np.array_equal(keep.cpu().numpy(), rk) and 0 < rk.sum() < F
    assert np.array_equal(meshops.face_select(_dev(faces), V, vflags=_dev(flags != 0), min_corners=min_corners).cpu().numpy(), rk)


def test_selection_with_tied_sizes():
    # strips of 5, 9, 9, 3, 9, 5 faces: the three 9s tie, the two 5s tie
    lengths, faces, base = [5, 9, 9, 3, 9, 5], [], 0
    for n in lengths:
        faces.append(_strip(n, np.arange(base, base + n + 2)))
        base += n + 2
    faces = np.concatenate(faces)
    labels, sizes = _check_components(faces, base)
    s = sizes.cpu().numpy()
    for K in range(0, 8):
        ok = meshops.select_components(sizes, largest=K)
        assert np.array_equal(ok.cpu().numpy(), R.select_components(s, largest=K)), K
    assert np.flatnonzero(meshops.select_components(sizes, largest=2).cpu().numpy()).tolist() == [7, 18]  # the first two 9s
    assert np.flatnonzero(meshops.select_components(sizes, largest=4).cpu().numpy()).tolist() == [0, 7, 18, 34]
    for mf, K in ((0, None), (5, None), (6, 2), (9, 5), (10, 1)):
        assert np.array_equal(meshops.select_components(sizes, mf, K).cpu().numpy(), R.select_components(s, mf, K)), (mf, K)
    verts = np.arange(base * 3, dtype=np.float64).reshape(base, 3)
    v, f, _, idx = meshops.clean(_dev(verts), _dev(faces), largest_components=1)
    assert f.shape[0] == 9 and idx.tolist() == list(range(7, 18)) and np.array_equal(v.cpu().numpy(), verts[7:18])


def test_empty_result_is_a_valid_mesh():
    faces = _strip(10, np.arange(12))
    verts = np.random.RandomState(0).rand(12, 3).astype(np.float32)
    cols = np.zeros((12, 3), dtype=np.uint8)
    v, f, c, idx = _check_submesh(verts, faces, np.zeros(10, dtype=np.uint8), cols)
    assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3) and idx.shape == (0,)
    v, f, c, idx = meshops.clean(_dev(verts), _dev(faces), _dev(cols), min_component_faces=11)
    assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3) and idx.shape == (0,)
