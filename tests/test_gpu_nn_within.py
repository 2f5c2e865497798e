"""GPU: the radius-bounded exact 1-NN (evalmesh.NNGrid.query_within, ncw_nn_coarse / ncw_nn_query_within of csrc/ncw_nn.hip).

Reference 1: NNGrid(max_shell=64).query on grids of at most 64 cells a side -- nothing escapes, every answer is the shell
kernel's -- compared with torch.equal wherever its dist < sqrtf(r2); -1 / +inf wherever its dist > sqrtf(r2); either where equal.
Reference 2: the float64 brute force of tests/test_gpu_nn.py under its bound 8 eps32 x extent: membership outside the band
|d - R| <= bound, the distance within the bound, the index where the runner-up is clear.
The cases are those of tests/_nn_within_cases.py; tests/test_nn_within_host.py checks in numpy what they rest on."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _nn_within_cases as W

from neuralrecon_w_amd import evalmesh
from neuralrecon_w_amd import lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INF = float("inf")


def _brute64(P, Q, chunk=1 << 24):
    """(d [N], first argmin [N], runner-up distance [N]) in float64 on the GPU, differences squared (no expansion)."""
    p = torch.from_numpy(P).to(DEV)
    q = torch.from_numpy(Q).to(DEV)
    rows = max(1, chunk // max(1, p.shape[0]))
    d, i, d2nd = [], [], []
    for s in range(0, q.shape[0], rows):
        dd = ((q[s:s + rows, None, :] - p[None, :, :]) ** 2).sum(-1)
        i.append(torch.argmin(dd, 1))
        k = min(2, p.shape[0])
        v = torch.topk(dd, k, 1, largest=False).values
        d.append(v[:, 0].sqrt())
        d2nd.append(v[:, 1].sqrt() if k == 2 else torch.full_like(v[:, 0], INF))
    return torch.cat(d).cpu().numpy(), torch.cat(i).cpu().numpy(), torch.cat(d2nd).cpu().numpy()


def _grid(P, Q, target_cells, max_shell=64):
    r32, q32, cmax, _ = evalmesh.recentre(torch.from_numpy(P).to(DEV), torch.from_numpy(Q).to(DEV))
    return evalmesh.NNGrid(r32, cmax, max_shell=max_shell, target_cells=target_cells), q32


def _sqrt_r2(R):
    """sqrtf(r2) of the contract: r2 = float32(R) * float32(R) rounded once."""
    r = np.float32(R)
    return float(np.sqrt(r * r))


def _check_against_shells(d, i, rd, ri, R):
    """torch.equal below sqrtf(r2), -1 / +inf above it, either of the two at it."""
    sr = _sqrt_r2(R)
    lo, hi, at = rd < sr, rd > sr, rd == sr
    assert torch.equal(d[lo], rd[lo]) and torch.equal(i[lo], ri[lo]), (R, int((d[lo] != rd[lo]).sum()), int((i[lo] != ri[lo]).sum()))
    assert (i[hi] == -1).all() and (d[hi] == INF).all(), (R, int((i[hi] != -1).sum()))
    hit = i[at] >= 0
    assert torch.equal(d[at][hit], rd[at][hit]) and torch.equal(i[at][hit], ri[at][hit])
    assert (d[at][~hit] == INF).all() and (i[at][~hit] == -1).all()
    return int(lo.sum()), int(hi.sum())


def _check_against_float64(d, i, e, ei, e2, b, R):
    d, i = d.double().cpu().numpy(), i.cpu().numpy()
    member = i >= 0
    out = np.abs(e - R) > b
    assert (member[out] == (e[out] < R)).all(), (R, int((member[out] != (e[out] < R)).sum()))
    assert (np.isinf(d[~member])).all()
    assert (np.abs(d[member] - e[member]) <= b).all(), (R, np.abs(d[member] - e[member]).max(), b)
    clear = member & (e2 - e > b)
    assert (i[clear] == ei[clear]).all(), (R, int((i[clear] != ei[clear]).sum()))


_SHARED = {}


def _shared(name):
    """The grid, the queries and both references of a case: computed once, read by every test that needs them."""
    if name not in _SHARED:
        c = W.case(name)
        grid, q32 = _grid(c["P"], c["Q"], c["target_cells"])
        assert max(grid.dims) <= 64, grid.dims
        st = {}
        rd, ri = grid.query(q32, st)
        assert st["escaped"] == 0                                   # every reference answer is the shell kernel's
        _SHARED[name] = (c, grid, q32, rd, ri, _brute64(c["P"], c["Q"]), W.bound(c["P"], c["Q"]))
    return _SHARED[name]


# ---------------------------------------------------------------------------------------------------
# 1. the exact boundary
# ---------------------------------------------------------------------------------------------------
def test_exact_boundary_on_a_lattice():
    P, Q, d2, want = W.lattice_case()
    grid, q32 = _grid(P, Q, 512)
    rd, ri = grid.query(q32)
    for R in (3.0, float(np.float32(np.sqrt(2.0))), 0.5):
        r = np.float32(R)
        r2 = float(r * r)
        st = {}
        d, i = grid.query_within(q32, R, st)
        hit = d2 <= r2                                                # inclusive, on exact numbers
        exp_i = np.where(hit, want, -1)
        exp_d = np.where(hit, np.sqrt(d2.astype(np.float32)), np.float32(INF)).astype(np.float32)
        assert np.array_equal(i.cpu().numpy(), exp_i), (R, int((i.cpu().numpy() != exp_i).sum()))
        assert np.array_equal(d.cpu().numpy(), exp_d), R
        assert st["beyond"] == int((~hit).sum())
        _check_against_shells(d, i, rd, ri, R)
    assert (d2 == 9.0).any() and (d2 == 12.25).any() and (d2 == 2.0).any()


# ---------------------------------------------------------------------------------------------------
# 2. radii x distributions
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", W.NAMES)
def test_radii(name):
    c, grid, q32, rd, ri, (e, ei, e2), b = _shared(name)
    for R in list(c["radii"]) + [INF]:
        st = {}
        d, i = grid.query_within(q32, R, st)
        assert d.dtype == torch.float32 and i.dtype == torch.int64 and d.shape == i.shape == (c["Q"].shape[0],)
        below, above = _check_against_shells(d, i, rd, ri, R)
        _check_against_float64(d, i, e, ei, e2, b, R)
        assert st["beyond"] == int((i < 0).sum()) and "escaped" not in st
        print("%s R = %g h: %d within, %d beyond" % (name, R / c["h"], below, above))
        if R == INF:
            assert torch.equal(d, rd) and torch.equal(i, ri)          # the exact unbounded answer, bit for bit
        else:
            assert below > 0 and above > 0


def test_nn_distances_routes_max_dist():
    c, grid, q32, rd, ri, _, _ = _shared("uniform")
    P, Q = torch.from_numpy(c["P"]).to(DEV), torch.from_numpy(c["Q"]).to(DEV)
    R = c["radii"][1]
    st = {}
    d, i = evalmesh.nn_distances(P, Q, stats=st, max_dist=R)
    d0, i0 = evalmesh.nn_distances(P, Q)
    keep = i >= 0
    assert torch.equal(d[keep], d0[keep]) and torch.equal(i[keep], i0[keep]) and (d[~keep] == INF).all()
    assert (d0[~keep] > _sqrt_r2(R) * (1 - 1e-6)).all() and (d0[keep] <= _sqrt_r2(R)).all()
    assert st["beyond"] == int((~keep).sum()) > 0 and int(keep.sum()) > 0


# ---------------------------------------------------------------------------------------------------
# 3. shapes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_query_counts(n):
    rng = np.random.RandomState(n)
    P, Q = rng.uniform(-1, 1, (40, 3)), rng.uniform(-1.5, 1.5, (n, 3))
    grid, q32 = _grid(P, Q, 27)
    rd, ri = grid.query(q32)
    e, ei, e2 = _brute64(P, Q)
    for R in (0.3, 0.8, INF):
        d, i = grid.query_within(q32, R)
        _check_against_shells(d, i, rd, ri, R)
        _check_against_float64(d, i, e, ei, e2, W.bound(P, Q), R)


def test_single_point_single_cell_and_large_block():
    rng = np.random.RandomState(11)
    P, Q = np.array([[0.5, -1.0, 2.0]]), rng.uniform(-3, 3, (65, 3))
    grid, q32 = _grid(P, Q, None)
    assert grid.dims == [1, 1, 1]
    rd, ri = grid.query(q32)
    for block in (None, 1, 64):                                     # 64: larger than every grid side
        grid.build_coarse(block)
        for R in (2.0, INF):
            d, i = grid.query_within(q32, R)
            _check_against_shells(d, i, rd, ri, R)
    assert (i == 0).all()


@pytest.mark.parametrize("block", [1, 2, 4, 8, 64])
def test_grid_sides_that_are_no_multiple_of_the_block(block):
    rng = np.random.RandomState(12)
    P = np.concatenate([rng.uniform(0, 1, (300, 3)) * [13.0, 5.0, 0.0], [[0, 0, 0], [13.0, 5.0, 0.0]]])
    Q = np.concatenate([rng.uniform(0, 1, (257, 3)) * [13.0, 5.0, 0.0] + rng.randn(257, 3) * 0.5, [[40.0, -20.0, 9.0]]])
    grid, q32 = _grid(P, Q, 65)
    assert grid.dims == [13, 5, 1], grid.dims
    rd, ri = grid.query(q32)
    e, ei, e2 = _brute64(P, Q)
    assert grid.build_coarse(block).shape[0] == -(-13 // block) * -(-5 // block)
    assert int(grid.coarse.sum()) == P.shape[0]                    # every point counted once
    for R in (0.2, 1.5, 6.0, INF):
        d, i = grid.query_within(q32, R)
        _check_against_shells(d, i, rd, ri, R)
        _check_against_float64(d, i, e, ei, e2, W.bound(P, Q), R)


def test_empty_queries_tiny_radius_and_a_nan_query():
    c, grid, q32, rd, ri, _, _ = _shared("uniform")
    st = {}
    d, i = grid.query_within(q32[:0], 1.0, st)
    assert d.shape == (0,) and i.shape == (0,) and st["beyond"] == 0
    d, i = grid.query_within(q32, 1e-30)                            # nothing is that close
    assert (i == -1).all() and (d == INF).all()
    q = q32[:65].clone()
    q[17, 1] = float("nan")
    R = c["radii"][2]
    d, i = grid.query_within(q, R)
    torch.cuda.synchronize()                                        # the launch returns
    assert int(i[17]) == -1 and float(d[17]) == INF
    ok = torch.arange(65, device=DEV) != 17
    d0, i0 = grid.query_within(q32[:65], R)
    assert torch.equal(d[ok], d0[ok]) and torch.equal(i[ok], i0[ok])
    q[17, 1] = INF                                                  # every d2 is +inf: index 0 without a bound, nothing within one
    d, i = grid.query_within(q, R)
    assert int(i[17]) == -1 and float(d[17]) == INF and torch.equal(i[ok], i0[ok])
    d, i = grid.query_within(q, INF)
    assert int(i[17]) == 0 and float(d[17]) == INF


# ---------------------------------------------------------------------------------------------------
# 4. grids where NNGrid.query does escape
# ---------------------------------------------------------------------------------------------------
def test_where_the_unbounded_query_escapes():
    rng = np.random.RandomState(3)
    v = rng.randn(20000, 3)
    P = v / np.linalg.norm(v, axis=1, keepdims=True)
    Q = np.concatenate([P[:5000] + rng.randn(5000, 3) * 1e-3, rng.uniform(-1, 1, (200, 3)) + [1000.0, 0, 0], rng.randn(20, 3) * 300.0])
    r32, q32, cmax, _ = evalmesh.recentre(torch.from_numpy(P).to(DEV), torch.from_numpy(Q).to(DEV))
    grid = evalmesh.NNGrid(r32, cmax, max_shell=8)
    st0, st = {}, {}
    d0, i0 = grid.query(q32, st0)
    assert st0["escaped"] > 0
    d, i = grid.query_within(q32, INF, st)
    assert "escaped" not in st and st["beyond"] == 0
    e, ei, e2 = _brute64(P, Q)
    clear = torch.from_numpy(e2 - e > W.bound(P, Q)).to(DEV)
    assert torch.equal(i[clear], i0[clear]) and (i[clear].cpu().numpy() == ei[clear.cpu().numpy()]).all()
    ulp = torch.from_numpy(np.spacing(d0.cpu().numpy())).to(DEV)
    assert ((d - d0).abs() <= ulp).all()
    print("escaping grid: %d escaped, dist bit-identical: %s" % (st0["escaped"], bool(torch.equal(d, d0))))


# ---------------------------------------------------------------------------------------------------
# 5. split independence, 6. bad arguments, 7. scipy
# ---------------------------------------------------------------------------------------------------
def test_split_and_repeat_give_the_same_bits():
    c, grid, q32, _, _, _, _ = _shared("clusters")
    for R in (c["radii"][1], c["radii"][3], INF):
        d, i = grid.query_within(q32, R)
        d2, i2 = grid.query_within(q32, R)
        assert torch.equal(d, d2) and torch.equal(i, i2)
        h = q32.shape[0] // 2 + 1
        da, ia = grid.query_within(q32[:h].contiguous(), R)
        db, ib = grid.query_within(q32[h:].contiguous(), R)
        assert torch.equal(torch.cat([da, db]), d) and torch.equal(torch.cat([ia, ib]), i)


def test_bad_arguments_through_the_abi():
    c, grid, q32, _, _, _, _ = _shared("uniform")
    lib = L.get_lib()
    grid.build_coarse()
    n = 8
    q = q32[:n].contiguous()
    dist = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    idx = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    order = torch.arange(n, dtype=torch.int64, device=DEV)
    s = L.stream_ptr(torch.device(DEV))

    def call(coarse=None, block=None, max_dist=1.0, count=n):
        return lib.ncw_nn_query_within(L.ptr(grid.pts), L.ptr(grid.range), L.ptr(grid.coarse) if coarse is None else coarse,
                                       grid.coarse_block if block is None else block, L.ptr(q), L.ptr(order), count,
                                       C.byref(grid.cgrid), float(grid.margin), max_dist, L.ptr(dist), L.ptr(idx), s)

    for bad in (0.0, -1.0, float("nan")):
        assert call(max_dist=bad) == -1
    assert call(coarse=C.c_void_p(None)) == -1 and call(block=0) == -1 and call(block=3) == -1
    assert call(count=0) == 0
    assert lib.ncw_nn_coarse(L.ptr(grid.range), C.byref(grid.cgrid), 0, L.ptr(grid.coarse), s) == -1
    assert lib.ncw_nn_coarse(C.c_void_p(None), C.byref(grid.cgrid), 4, L.ptr(grid.coarse), s) == -1
    torch.cuda.synchronize()
    assert (dist == -7.0).all() and (idx == -7).all()               # no launch wrote anything
    assert call() == 0
    torch.cuda.synchronize()
    assert (idx != -7).all()


def test_against_ckdtree_with_an_upper_bound():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.RandomState(8)
    v = rng.randn(20000, 3)
    P = v / np.linalg.norm(v, axis=1, keepdims=True) * 10 + rng.randn(20000, 3) * 1e-3
    Q = P[rng.choice(20000, 20000)] * rng.uniform(0.9, 1.1, (20000, 1)) + rng.randn(20000, 3) * 0.02
    R = 0.3
    d, i = evalmesh.nn_distances(torch.from_numpy(P).to(DEV), torch.from_numpy(Q).to(DEV), max_dist=R)
    d, i = d.double().cpu().numpy(), i.cpu().numpy()
    kd, ki = spatial.cKDTree(P).query(Q, k=2, distance_upper_bound=R)   # misses: dist inf, index len(P)
    b = W.bound(P, Q)
    full = spatial.cKDTree(P).query(Q, k=2)[0]
    out = np.abs(full[:, 0] - R) > b
    assert ((i >= 0)[out] == (ki[:, 0] < P.shape[0])[out]).all()
    assert 0.05 < (i < 0).mean() < 0.95                              # both outcomes
    clear = (i >= 0) & out & (full[:, 1] - full[:, 0] > b)
    assert (i[clear] == ki[clear, 0]).all() and (np.abs(d[clear] - kd[clear, 0]) <= b).all()
