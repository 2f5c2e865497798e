"""Surface-cloud fusion on the GPU (csrc/ncw_fuse.hip, neuralrecon_w_amd/surfcloud.py): the keys, the table and the resolved
outputs BIT FOR BIT against the numpy restatement tests/_fuse_ref.py -- sizes around the wave and the workgroup, every edge of
the quantiser, one crowded cell, long probe chains, repeated growth, distinct-view counts, split and permuted input, two runs.
The overflow path is reached ONLY through the host check: no test fills a table on the device."""
import numpy as np
import pytest
import torch

from tests import _fuse_ref as FR

pytestmark = pytest.mark.gpu

LO, HI, H = (-0.5, -0.25, 0.0), (1.5, 1.25, 1.125), 0.125   # dims 16 x 12 x 9 = 1728 cells
SCALE, OFF = 2.0, (0.5, -0.25, 1.0)                          # x = 2 p + off: every number here is dyadic, so exact in float32
COS = 0.1
OUT_KEYS = ("positions", "normals", "colours", "count", "views", "keys")


def _cloud(cos_min=COS, **kw):
    from neuralrecon_w_amd import surfcloud

    return surfcloud.SurfaceCloud(LO, HI, H, scale=SCALE, offset=OFF, cos_min=cos_min, **kw)


def _grid(cos_min=COS):
    g = FR.grid_of(LO, HI, H, SCALE, OFF, cos_min)
    assert g["dims"].tolist() == [16, 12, 9]
    return g


def _p_of(x):
    """float32 network-frame points whose image 2 p + off is x (exact for the dyadic x used here)."""
    return ((np.asarray(x, dtype=np.float64) - np.asarray(OFF)) / SCALE).astype(np.float32)


def _cell_points(cells, frac=0.5):
    """One point per cell index triple, at `frac` of the cell."""
    return _p_of(np.asarray(LO) + (np.asarray(cells, dtype=np.float64) + frac) * H)


def _mixed(m, seed):
    """m samples: points over a box somewhat larger than the grid, random gradients, directions roughly against them,
    colours beyond [0, 1]."""
    g = np.random.RandomState(seed)
    x = g.uniform(np.asarray(LO) - 0.1, np.asarray(HI) + 0.1, (m, 3))
    p = ((x - np.asarray(OFF)) / SCALE).astype(np.float32)
    n = (g.normal(size=(m, 3)) * g.uniform(0.1, 30.0, (m, 1))).astype(np.float32)
    d = -n / np.linalg.norm(n, axis=1, keepdims=True) + 0.8 * g.normal(size=(m, 3)).astype(np.float32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    c = g.uniform(-0.2, 1.2, (m, 3)).astype(np.float32)
    return p, n, d, c


def _add(cloud, s, view, a=None, b=None):
    cloud.add(*(torch.from_numpy(np.ascontiguousarray(v[a:b])).cuda() for v in s), view)


def _check(cloud, batches, cos_min=COS, **filters):
    """The cloud's table and its resolved arrays equal the restatement's over `batches`, bit for bit."""
    grid = _grid(cos_min)
    ref = FR.accumulate(batches, grid)
    tab = cloud.table()
    for k in ("keys", "acc", "views"):
        got = tab[k].cpu().numpy()
        assert got.dtype == ref[k].dtype and np.array_equal(got, ref[k]), k
    out, want = cloud.finish(**filters), FR.resolve(ref, grid, **filters)
    for k in OUT_KEYS:
        got = out[k].cpu().numpy()
        assert got.dtype == want[k].dtype and got.shape == want[k].shape and np.array_equal(got, want[k]), k
    assert (out["cells"], out["degenerate"]) == (want["cells"], want["degenerate"])
    assert FR.inside_cells(out["positions"].cpu().numpy(), out["keys"].cpu().numpy(), grid)
    st = cloud.stats()
    assert st["valid"] == ref["valid"] and st["cells"] == ref["keys"].shape[0] and st["overflow"] == 0
    assert st["offered"] == sum(len(b[0]) for b in batches) and 2 * st["cells"] <= st["capacity"]
    return ref, out


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_bit_for_bit(m):
    s = _mixed(m, m)
    cloud = _cloud(capacity=4096)
    half = m // 2
    _add(cloud, s, 0, 0, half)
    _add(cloud, s, 2, half, m)
    ref, _ = _check(cloud, [tuple(v[:half] for v in s) + (0,), tuple(v[half:] for v in s) + (2,)])
    if m >= 63:
        assert 0 < ref["valid"] < m  # both kinds of sample are in the batch


def _edge_samples():
    lo, hi = np.asarray(LO), np.asarray(HI)
    up, dn = np.float32([0, 0, 3.0]), np.float32([0, 0, -1.0])  # gradient, direction: facing the camera
    mid = lo + 2.5 * H
    x = [lo, lo + H, lo + 3 * H, hi - H, hi, [hi[0], mid[1], mid[2]], [mid[0], hi[1], mid[2]], [mid[0], mid[1], hi[2]],
         lo - 1e-3, hi + 1.0, [lo[0] - H, mid[1], mid[2]], hi, mid]
    rows = [(_p_of(v), up, dn, np.float32([0.2, 0.4, 0.6])) for v in x]
    rows[11] = (np.nextafter(rows[11][0], np.float32(-9.0)),) + rows[11][1:]  # the last float32 below lo + dims h: the last cell
    pm = _p_of(mid)
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(3):
            for which in range(4):  # NaN / inf in each input, each axis
                r = [pm.copy(), up.copy(), dn.copy(), np.float32([0.2, 0.4, 0.6])]
                r[which][a] = bad
                rows.append(tuple(r))
    rows += [(pm, np.float32([0, 0, 0]), dn, np.float32([1, 1, 1])), (pm, -up, dn, np.float32([1, 1, 1])),
             (pm, np.float32([0, 1e-30, 0]), np.float32([0, -1, 0]), np.float32([1, 1, 1])),  # nn underflows in float32, not in float64
             (pm, np.float32([3e38, 3e38, 3e38]), np.float32([-1, 0, 0]), np.float32([0, 0, 0])),  # nn overflows in float32 only
             (pm, np.float32([1, 0, 0]), np.float32([0, 1, 0]), np.float32([0.5, 0.5, 0.5]))]  # perpendicular: cosine 0
    return [tuple(np.asarray(v, dtype=np.float32) for v in r) for r in rows]


@pytest.mark.parametrize("cos_min", [COS, None, 0.0])
def test_quantiser_edges_batch_and_one_by_one(cos_min):
    """Coordinates exactly on cell boundaries, on lo and on lo + dims h (excluded), points outside, NaN / inf in each input, a
    zero gradient, back-facing and perpendicular gradients: as one batch, and every sample alone (its own key and payload)."""
    rows = _edge_samples()
    s = tuple(np.stack([r[i] for r in rows]) for i in range(4))
    cloud = _cloud(cos_min, capacity=256)
    _add(cloud, s, 0)
    ref, _ = _check(cloud, [s + (0,)], cos_min)
    assert 0 < ref["valid"] < len(rows)
    keys, _ = FR.quantise(*s, _grid(cos_min))
    assert keys[4] == -1 and keys[0] == 0 and keys[1] == (1 * 12 + 1) * 16 + 1 and (keys[5:11] == -1).all() and keys[11] == 1727
    for i in range(len(rows)):
        one = tuple(v[i:i + 1] for v in s)
        cloud = _cloud(cos_min, capacity=16)
        _add(cloud, one, 0)
        _check(cloud, [one + (0,)], cos_min)
        assert cloud.stats()["valid"] == int(keys[i] >= 0)


def test_facing_test_exactly_at_cos_min():
    """-n.d == cos_min |n| exactly is kept; one ulp more of cos_min drops it; with the test off a back-facing sample stays."""
    pm = _p_of(np.asarray(LO) + 2.5 * H)[None]
    n, d = np.float32([[0, 0, 2.0]]), np.float32([[0, np.sqrt(0.75), -0.5]])
    c = np.float32([[0.1, 0.2, 0.3]])
    for cos_min, valid in ((0.5, 1), (float(np.nextafter(0.5, 1.0)), 0), (float(np.nextafter(0.5, 0.0)), 1)):
        cloud = _cloud(cos_min, capacity=16)
        _add(cloud, (pm, n, d, c), 0)
        _check(cloud, [(pm, n, d, c, 0)], cos_min)
        assert cloud.stats()["valid"] == valid
    cloud = _cloud(None, capacity=16)
    _add(cloud, (pm, -n, d, c), 0)
    _check(cloud, [(pm, -n, d, c, 0)], None)
    assert cloud.stats()["valid"] == 1


def test_1000_samples_in_1000_cells_and_colour_rounding():
    """Every sample in a cell of its own, so the table shows each sample's payload: colours below 0 and above 1, on the one
    exact tie (0.5 -> 127.5 -> 128) and on the float32 neighbours of every (k + 0.5) / 255."""
    idx = np.arange(1000)
    cells = np.stack([idx % 16, (idx // 16) % 12, idx // 192], 1)
    g = np.random.RandomState(5)
    p = _cell_points(cells, g.uniform(0.05, 0.95, (1000, 3)))
    n = g.normal(size=(1000, 3)).astype(np.float32)
    d = (-n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    t = ((np.arange(3000) % 255 + 0.5) / 255.0).astype(np.float32).reshape(1000, 3)
    c = t.copy()
    c[1::3] = np.nextafter(t[1::3], np.float32(2.0))
    c[2::3] = np.nextafter(t[2::3], np.float32(-1.0))
    c[0] = (0.5, -0.5, 1.5)
    c[1] = (-0.0, 1.0, 0.0)
    c[2] = (1e-30, 7.0, -1e-30)
    s = (p, n, d, c)
    cloud = _cloud(capacity=2048)
    _add(cloud, s, 0)
    ref, out = _check(cloud, [s + (0,)])
    assert ref["keys"].shape[0] == 1000 and (ref["acc"][:, 0] == 1).all() and cloud.stats()["growths"] == 0
    assert out["colours"][0].tolist() == [128, 0, 255]


def test_capacity_at_exactly_twice_the_cells():
    """1024 cells in 2048 rows: the fullest table the host allows (long probe chains), no growth."""
    idx = np.arange(1024)
    cells = np.stack([idx % 16, (idx // 16) % 12, idx // 192], 1)
    s3 = _mixed(3 * 1024, 9)
    p = _cell_points(np.tile(cells, (3, 1)), np.random.RandomState(3).uniform(0.05, 0.95, (3072, 3)))
    s = (p,) + s3[1:]
    cloud = _cloud(None, capacity=2048)
    _add(cloud, s, 0, 0, 1024)      # 2 * (0 + 1024) = capacity: stays
    assert cloud.stats()["growths"] == 0 and cloud.stats()["cells"] == 1024
    ref, _ = _check(cloud, [tuple(v[:1024] for v in s) + (0,)], None)
    assert ref["keys"].shape[0] == 1024
    _add(cloud, s, 1, 1024, 3072)   # the bound says grow; the true count says 2 * (1024 + 2048) -> 8192 rows
    st = cloud.stats()
    assert st["growths"] == 1 and st["capacity"] == 8192 and st["cells"] == 1024
    _check(cloud, [tuple(v[:1024] for v in s) + (0,), tuple(v[1024:] for v in s) + (1,)], None)


def test_4096_samples_in_one_cell():
    g = np.random.RandomState(11)
    p = _cell_points(np.tile([[7, 5, 3]], (4096, 1)), g.uniform(0.05, 0.95, (4096, 3)))
    s = (p,) + _mixed(4096, 12)[1:]
    cloud = _cloud(None, capacity=16)
    _add(cloud, s, 4)
    ref, out = _check(cloud, [s + (4,)], None)
    assert ref["keys"].tolist() == [(3 * 12 + 5) * 16 + 7] and ref["acc"][0, 0] == 4096 and out["views"].tolist() == [1]
    assert cloud.stats()["growths"] == 1  # 2 * 4096 rows asked before the insert: the bound counts samples, not cells


def test_growth_from_16_rows_and_one_serial_in_1_or_7_calls():
    """An initial capacity of 16 grows again and again; one serial fed in 1 / 7 calls gives the same table and the same output."""
    s = _mixed(1000, 21)
    one, seven = _cloud(capacity=1 << 14), _cloud(capacity=16)
    _add(one, s, 3)
    cuts = [0, 1, 8, 40, 41, 300, 650, 1000]
    for a, b in zip(cuts[:-1], cuts[1:]):
        _add(seven, s, 3, a, b)
    assert one.stats()["growths"] == 0 and seven.stats()["growths"] >= 2
    _check(one, [s + (3,)])
    _check(seven, [s + (3,)])
    ta, tb = one.table(), seven.table()
    fa, fb = one.finish(), seven.finish()
    assert all(torch.equal(ta[k], tb[k]) for k in ta) and all(torch.equal(fa[k], fb[k]) for k in OUT_KEYS)


def test_three_serials_in_one_cell_and_the_filters():
    """views counts DISTINCT serials (several samples each, serials with gaps, one of them in two calls); min_views / min_count."""
    g = np.random.RandomState(31)
    cells = np.array([[2, 2, 2]] * 12 + [[3, 2, 2]] * 5 + [[4, 2, 2]] * 2 + [[5, 2, 2]])
    p = _cell_points(cells, g.uniform(0.05, 0.95, (20, 3)))
    n = np.tile(np.float32([[0.1, 0.2, 1.0]]), (20, 1))
    d = np.tile(np.float32([[0, 0, -1.0]]), (20, 1))
    c = g.uniform(0, 1, (20, 3)).astype(np.float32)
    s = (p, n, d, c)
    parts = [(0, 4, 0), (4, 6, 5), (6, 8, 5), (8, 12, 9), (12, 15, 9), (15, 17, 9), (17, 18, 9), (18, 19, 11), (19, 20, 11)]
    cloud = _cloud(capacity=64)
    for a, b, v in parts:
        _add(cloud, s, v, a, b)
    batches = [tuple(x[a:b] for x in s) + (v,) for a, b, v in parts]
    ref, out = _check(cloud, batches)
    assert ref["views"].tolist() == [3, 1, 2, 1] and ref["acc"][:, 0].tolist() == [12, 5, 2, 1]
    assert out["views"].dtype == torch.int32
    for filters, kept in ((dict(min_views=2), 2), (dict(min_count=3), 2), (dict(min_views=2, min_count=3), 1),
                          (dict(min_views=4), 0), (dict(min_views=1, min_count=1), 4)):
        _, out = _check(cloud, batches, **filters)
        assert out["keys"].numel() == kept and out["cells"] == 4


def test_opposite_normals_give_degenerate_cells_that_are_dropped():
    cells = np.array([[1, 1, 1], [1, 1, 1], [2, 1, 1], [2, 1, 1], [2, 1, 1]])
    p = _cell_points(cells, 0.25)
    n = np.float32([[0, 0, 2], [0, 0, -7], [0, 3, 0], [0, -3, 0], [0, 0, 1]])
    d = np.float32([[0, 0, -1]] * 5)
    c = np.float32([[0.5, 0.5, 0.5]] * 5)
    cloud = _cloud(None, capacity=16)
    _add(cloud, (p, n, d, c), 0)
    ref, out = _check(cloud, [(p, n, d, c, 0)], None)
    assert ref["acc"][:, 4:7].tolist() == [[0, 0, 0], [0, 0, 32767]]
    assert out["cells"] == 2 and out["degenerate"] == 1 and out["keys"].numel() == 1 and out["normals"].tolist() == [[0.0, 0.0, 1.0]]


def test_two_runs_and_a_permuted_order_are_equal():
    s = _mixed(1000, 41)
    perm = np.random.RandomState(42).permutation(1000)
    outs, tabs = [], []
    for order in (slice(None), slice(None), perm):
        cloud = _cloud(capacity=64)
        q = tuple(v[order] for v in s)
        _add(cloud, q, 0, 0, 500)
        _add(cloud, q, 0, 500, 1000)
        outs.append(cloud.finish())
        tabs.append(cloud.table())
    for o, t in zip(outs[1:], tabs[1:]):
        assert all(torch.equal(o[k], outs[0][k]) for k in OUT_KEYS) and all(torch.equal(t[k], tabs[0][k]) for k in t)
    assert outs[0]["keys"].numel() > 300


def test_overflow_is_reached_only_through_the_host_check():
    """A table the host refuses to insert into: growth beyond max_capacity raises BEFORE the launch and inserts nothing; a
    non-zero overflow counter (set here by hand -- never by running a full table on the device) turns into an exception."""
    from neuralrecon_w_amd import lib as L

    s = _mixed(64, 51)
    cloud = _cloud(None, capacity=16, max_capacity=16)
    _add(cloud, s, 0, 0, 8)          # 2 * 8 = 16 rows: fits
    before = cloud.table()
    with pytest.raises(L.NeuconwHipError, match="max_capacity"):
        _add(cloud, s, 0, 8, 17)
    st = cloud.stats()
    assert st["offered"] == 8 and st["growths"] == 0 and st["capacity"] == 16 and st["overflow"] == 0
    assert all(torch.equal(v, cloud.table()[k]) for k, v in before.items())
    _check(cloud, [tuple(v[:8] for v in s) + (0,)], None)
    cloud._table["counters"][1] = 3
    for call in (cloud.finish, cloud.stats, cloud.table, lambda: _add(cloud, s, 0, 0, 8)):
        with pytest.raises(L.NeuconwHipError, match="found no slot"):
            call()
