"""GPU: the exact k-NN grid walk and the per-point PCA (ncw_knn_query / ncw_knn_pca of csrc/ncw_knn.hip through
evalmesh.NNGrid.query_k, evalmesh.knn and cloudops.pca).

Everything is compared BIT FOR BIT with the numpy restatements of tests/_knn_ref.py (knn32, pca_ref) on the float32 tensors the
grid holds; tests/test_knn_host.py checks those restatements against independent float64 references without a GPU.  The
clouds are those of tests/_nn_within_cases.py: `clusters` and `outliers` force the coarse phase, `outside` the clamped cells."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _knn_ref as K
from tests import _nn_within_cases as W

from neuralrecon_w_amd import cloudops, evalmesh
from neuralrecon_w_amd import lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INF = float("inf")
KS = (1, 2, 8, 16, 31, 32)


def _grid(P, Q, target_cells):
    r32, q32, cmax, _ = evalmesh.recentre(torch.from_numpy(np.asarray(P, dtype=np.float64)).to(DEV),
                                          torch.from_numpy(np.asarray(Q, dtype=np.float64)).to(DEV))
    return evalmesh.NNGrid(r32, cmax, max_shell=64, target_cells=target_cells), q32


def _same(got, want, what=""):
    """(dist, idx, count) tensors against knn32's arrays, bit for bit (+inf == +inf)."""
    d, i, c = (t.cpu().numpy() for t in got)
    wd, wi, wc = want
    assert d.dtype == np.float32 and i.dtype == np.int32 and c.dtype == np.int32 and d.shape == wd.shape == i.shape
    assert np.array_equal(c, wc), (what, "count", int((c != wc).sum()))
    assert np.array_equal(i, wi), (what, "idx", int((i != wi).any(1).sum()))
    assert np.array_equal(d, wd), (what, "dist", int((d != wd).any(1).sum()))


def _no_repeats(idx, count):
    i = idx.cpu().numpy().astype(np.int64)
    big = np.where(i < 0, np.arange(i.shape[1])[None, :] + (1 << 40), i)    # the -1 of a short row are not repeats
    assert (np.diff(np.sort(big, axis=1), axis=1) != 0).all()
    assert ((i >= 0).sum(1) == count.cpu().numpy()).all()


_SHARED = {}


def _shared(name):
    """The grid, the queries and the float32 d2 matrix of a case: computed once, read by every test that needs them."""
    if name not in _SHARED:
        _SHARED.clear()                                               # one d2 matrix (48 MB) at a time
        c = W.case(name)
        grid, q32 = _grid(c["P"], c["Q"], c["target_cells"])
        p, q = grid.ref.cpu().numpy(), q32.cpu().numpy()
        _SHARED[name] = (c, grid, q32, p, q, K.d2_matrix(p, q))
    return _SHARED[name]


# ---------------------------------------------------------------------------------------------------
# 1. distributions x k x radii
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", W.NAMES)
def test_clouds_k_and_radii(name, k):
    c, grid, q32, p, q, d2 = _shared(name)
    for R in list(c["radii"]) + [INF]:
        st = {}
        got = grid.query_k(q32, k, max_dist=R, stats=st)
        want = K.knn32(p, q, k, r=R, d2=d2)
        _same(got, want, (name, k, R / c["h"]))
        _no_repeats(got[1], got[2])
        assert st["evals"] >= int(want[2].sum()) and st["inserts"] >= int(want[2].sum())
        if R == INF:
            assert (want[2] == k).all()
        else:
            assert (want[2] < k).any()                                # the radius cuts rows short
    assert (K.knn32(p, q, k, r=c["radii"][3], d2=d2)[2] > 0).any()


def test_lattice_ties_duplicates_and_self_query():
    P, Q, _, _ = W.lattice_case()
    grid, q32 = _grid(P, Q, 512)
    p, q = grid.ref.cpu().numpy(), q32.cpu().numpy()
    d2 = K.d2_matrix(p, q)
    for k in (8, 32):
        for R in (INF, 3.0, 0.5):
            _same(grid.query_k(q32, k, max_dist=R), K.knn32(p, q, k, r=R, d2=d2), ("lattice", k, R))
    # the cloud queries itself: the own index never appears, a duplicate of the point stays at d = 0
    own = torch.arange(P.shape[0], dtype=torch.int32, device=DEV)
    for k in (1, 8, 32):
        got = grid.query_k(grid.ref, k, exclude=own)
        _same(got, K.knn32(p, p, k, exclude=np.arange(P.shape[0])), ("lattice self", k))
        assert not (got[1] == own[:, None]).any()
        _no_repeats(got[1], got[2])
    dup = np.arange(512, 576)
    assert (got[0][dup, 0] == 0).all() and (got[1][dup, 0] < 512).all()      # a duplicate finds its original at d = 0
    d, i, cnt = evalmesh.knn(torch.from_numpy(P).to(DEV), torch.from_numpy(P).to(DEV), 8, exclude_self=True)
    _same((d, i, cnt), K.knn32(p, p, 8, exclude=np.arange(P.shape[0])), "evalmesh.knn")


# ---------------------------------------------------------------------------------------------------
# 2. shapes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_query_counts_and_workgroup_sizes(n):
    rng = np.random.RandomState(n)
    P, Q = rng.uniform(-1, 1, (300, 3)), rng.uniform(-1.5, 1.5, (n, 3))
    grid, q32 = _grid(P, Q, 512)
    p, q = grid.ref.cpu().numpy(), q32.cpu().numpy()
    for k, R in ((8, INF), (32, 0.5), (1, INF)):
        want = K.knn32(p, q, k, r=R)
        for wg in (0, 64, 128, 256):
            _same(grid.query_k(q32, k, max_dist=R, wg=wg), want, (n, k, R, wg))


def test_fewer_points_than_k_and_a_single_point():
    rng = np.random.RandomState(4)
    Q = rng.uniform(-2, 2, (130, 3))
    for m in (5, 1):
        P = rng.uniform(-1, 1, (m, 3))
        grid, q32 = _grid(P, Q, None)
        p, q = grid.ref.cpu().numpy(), q32.cpu().numpy()
        for R in (INF, 1.5):
            got = grid.query_k(q32, 8, max_dist=R)
            _same(got, K.knn32(p, q, 8, r=R), (m, R))
        assert int(got[2].max()) <= m and (got[1][:, m:] == -1).all() and (got[0][:, m:] == INF).all()
    d, i, c = evalmesh.knn(torch.zeros(0, 3, device=DEV), torch.from_numpy(Q).to(DEV), 4)
    assert d.shape == (130, 4) and (i == -1).all() and (c == 0).all() and (d == INF).all()
    d, i, c = evalmesh.knn(torch.from_numpy(Q).to(DEV), torch.zeros(0, 3, device=DEV), 4)
    assert d.shape == (0, 4) and i.shape == (0, 4) and c.shape == (0,)


def test_nan_and_infinite_queries():
    c, grid, q32, p, q, _ = _shared("uniform")
    qq = q32[:130].clone()
    qq[17, 1] = float("nan")
    qq[64, 0] = INF
    qq[65, 2] = -INF
    for R in (INF, c["radii"][2]):
        got = grid.query_k(qq, 8, max_dist=R)
        torch.cuda.synchronize()                                      # the launch returns
        _same(got, K.knn32(p, qq.cpu().numpy(), 8, r=R), R)
        assert (got[2][[17, 64, 65]] == 0).all() and (got[1][[17, 64, 65]] == -1).all()


# ---------------------------------------------------------------------------------------------------
# 3. reproducibility, agreement with the 1-NN kernel, bad arguments
# ---------------------------------------------------------------------------------------------------
def test_split_and_repeat_give_the_same_bits():
    c, grid, q32, _, _, _ = _shared("clusters")
    for k, R in ((16, INF), (32, c["radii"][3])):
        d, i, n = grid.query_k(q32, k, max_dist=R)
        d2, i2, n2 = grid.query_k(q32, k, max_dist=R)
        assert torch.equal(d, d2) and torch.equal(i, i2) and torch.equal(n, n2)
        parts = [grid.query_k(ch.contiguous(), k, max_dist=R) for ch in torch.chunk(q32, 7)]
        assert len(parts) == 7
        for a, whole in enumerate((d, i, n)):
            assert torch.equal(torch.cat([pt[a] for pt in parts]), whole)
        _no_repeats(i, n)


@pytest.mark.parametrize("name", ["uniform", "outliers"])
def test_k1_agrees_with_the_1nn_kernel(name):
    """query_within contracts d2 to fma, so its bits are not promised here: indices where the float64 runner-up is clear,
    distances within the bound."""
    c, grid, q32, p, q, _ = _shared(name)
    P, Q = torch.from_numpy(c["P"]).to(DEV), torch.from_numpy(c["Q"]).to(DEV)
    b = W.bound(c["P"], c["Q"])
    dd = torch.cdist(Q, P, compute_mode="donot_use_mm_for_euclid_dist")   # float64, from coordinate differences
    two = torch.topk(dd, 2, 1, largest=False).values
    clear = (two[:, 1] - two[:, 0]) > 2 * b
    for R in (INF, c["radii"][2]):
        d1, i1 = grid.query_within(q32, R)
        d, i, n = grid.query_k(q32, 1, max_dist=R)
        both = (i1 >= 0) & (n == 1)
        edge = (two[:, 0] - R).abs() <= b                             # membership may differ only in the band around R
        assert ((i1 >= 0) == (n == 1))[~edge].all()
        assert (i[:, 0].long() == i1)[both & clear].all()
        assert ((d[:, 0].double() - d1.double()).abs() <= b)[both].all()
        assert int((both & clear).sum()) > 0.9 * int(both.sum()) > 0


def test_bad_arguments_through_the_abi():
    c, grid, q32, _, _, _ = _shared("uniform")
    lib = L.get_lib()
    grid.build_coarse()
    n, k = 8, 4
    q = q32[:n].contiguous()
    dist = torch.full((n, k), -7.0, dtype=torch.float32, device=DEV)
    idx = torch.full((n, k), -7, dtype=torch.int32, device=DEV)
    cnt = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    order = torch.arange(n, dtype=torch.int64, device=DEV)
    s = L.stream_ptr(torch.device(DEV))

    def call(coarse=None, block=None, max_dist=1.0, count=n, kk=k, wg=0):
        return lib.ncw_knn_query(L.ptr(grid.pts), L.ptr(grid.range), L.ptr(grid.coarse) if coarse is None else coarse,
                                 grid.coarse_block if block is None else block, L.ptr(q), L.ptr(order), None, count,
                                 C.byref(grid.cgrid), float(grid.margin), max_dist, kk, wg, L.ptr(idx), L.ptr(dist), L.ptr(cnt),
                                 None, s)

    for bad in (0.0, -1.0, float("nan")):
        assert call(max_dist=bad) == -1
    assert call(coarse=C.c_void_p(None)) == -1 and call(block=3) == -1
    assert call(kk=0) == -1 and call(kk=33) == -1 and call(wg=96) == -1
    assert call(count=0) == 0
    assert lib.ncw_knn_pca(L.ptr(q), L.ptr(grid.ref), grid.m, L.ptr(idx), L.ptr(cnt), n, 0, 1, None, L.ptr(dist), L.ptr(dist),
                           L.ptr(dist), L.ptr(idx), s) == -1
    torch.cuda.synchronize()
    assert (dist == -7.0).all() and (idx == -7).all() and (cnt == -7).all()   # no launch wrote anything
    assert call() == 0
    torch.cuda.synchronize()
    assert (cnt >= 0).all()


# ---------------------------------------------------------------------------------------------------
# 4. ncw_knn_pca
# ---------------------------------------------------------------------------------------------------
def _pca_same(got, want, what=""):
    normal, eig, curv, valid = (t.cpu().numpy() for t in got)
    wn, we, wc, wv = want
    assert normal.dtype == np.float32 and eig.dtype == np.float64 and curv.dtype == np.float32
    rel = np.abs(eig - we).max() / max(np.abs(we).max(), 1e-300)
    print("%s: eig max rel diff %.3g, normals differ on %d rows, curvature on %d" %
          (what, rel, int((normal != wn).any(1).sum()), int((curv != wc).sum())))
    assert np.array_equal(valid, wv), what
    assert np.array_equal(eig, we), (what, rel)
    assert np.array_equal(normal, wn), what
    assert np.array_equal(curv, wc), what


def _sphere(n, seed=9, radius=1.0, centre=(0, 0, 0)):
    v = np.random.RandomState(seed).randn(n, 3)
    return v / np.linalg.norm(v, axis=1, keepdims=True) * radius + np.asarray(centre, dtype=np.float64)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2000])
def test_pca_bit_for_bit_and_the_sign_rule(n):
    P = _sphere(max(n, 20)) * [1.0, 0.7, 1.3] + [10.0, -20.0, 5.0]
    grid, _ = _grid(P, P, None)
    p32 = grid.ref[:n].contiguous()
    own = torch.arange(n, dtype=torch.int32, device=DEV)
    _, idx, cnt = grid.query_k(p32, 16, exclude=own)
    p, i, c = grid.ref.cpu().numpy(), idx.cpu().numpy(), cnt.cpu().numpy()
    for with_query in (True, False):
        got = cloudops.pca(p32, grid.ref, idx, cnt, with_query=with_query)
        _pca_same(got, K.pca_ref(p[:n], p, i, c, with_query=with_query), ("n = %d, with_query = %s" % (n, with_query)))
    normal = got[0].cpu().numpy()
    big = np.abs(normal).argmax(1)
    assert (normal[np.arange(n), big] > 0).all()
    for tw in ([0.1, -0.2, 0.05], [30.0, 2.0, -9.0]):                  # inside the ellipsoid, and far outside
        got = cloudops.pca(p32, grid.ref, idx, cnt, toward=tw)
        _pca_same(got, K.pca_ref(p[:n], p, i, c, toward=tw), ("n = %d toward %s" % (n, tw)))
        nn = got[0].double().cpu().numpy()
        t32 = np.asarray(tw, dtype=np.float32).astype(np.float64)
        assert ((nn * (t32 - p[:n].astype(np.float64))).sum(1) >= -1e-7).all()
    assert bool(got[3].all())


def test_pca_short_rows_collinear_and_coincident_members():
    rng = np.random.RandomState(6)
    P = rng.uniform(-1, 1, (64, 3)).astype(np.float32)
    P[40:46] = np.arange(6, dtype=np.float32)[:, None] * np.array([[0.5, 0.25, -1.0]], dtype=np.float32)   # collinear
    P[50:54] = P[50]                                                  # coincident
    idx = np.tile(np.arange(8, dtype=np.int32), (64, 1))
    idx[40] = [41, 42, 43, 44, 45, -1, -1, -1]
    idx[50] = [51, 52, 53, -1, -1, -1, -1, -1]
    idx[60] = [3, 64, 5, 6, 7, 8, 9, 10]                              # an index outside the cloud ends the list
    cnt = np.full(64, 8, dtype=np.int32)
    cnt[:3] = [0, 1, 2]
    cnt[40], cnt[50] = 5, 3
    tp, ti, tc = (torch.from_numpy(a).to(DEV) for a in (P, idx, cnt))
    for with_query in (True, False):
        got = cloudops.pca(tp, tp, ti, tc, with_query=with_query)
        _pca_same(got, K.pca_ref(P, P, idx, cnt, with_query=with_query), "edge rows, with_query = %s" % with_query)
        valid, normal = got[3].cpu().numpy(), got[0].cpu().numpy()
        assert not valid[[0, 1, 40, 50]].any() and (normal[[0, 1, 40, 50]] == 0).all()
        assert valid[2] == with_query                                 # 2 neighbours + the point itself: a triangle
        assert valid[3:40].all()
