"""numpy restatements of csrc/ncw_knn.hip (tests/test_knn_host.py checks them against independent references without a GPU;
tests/test_gpu_knn.py and tests/test_gpu_cloudops.py hold the kernels to them bit for bit).  numpy only."""
import numpy as np

INF32 = np.float32(np.inf)


def recentre32(*clouds):
    """evalmesh.recentre in numpy: the clouds moved to the centre of their common box in float64, then cast to float32.
    Returns ([float32 clouds], centre)."""
    both = np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in clouds if len(c)])
    centre = (both.min(0) + both.max(0)) / 2.0
    return [(np.asarray(c, dtype=np.float64).reshape(-1, 3) - centre).astype(np.float32) for c in clouds], centre


def d2_matrix(P32, Q32):
    """[N,M] float32: d2 = dx*dx + dy*dy + dz*dz with dx = P.x - q.x, every operation rounded to float32 (no fma)."""
    P32, Q32 = np.asarray(P32, dtype=np.float32), np.asarray(Q32, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = P32[None, :, 0] - Q32[:, None, 0]
        dy = P32[None, :, 1] - Q32[:, None, 1]
        dz = P32[None, :, 2] - Q32[:, None, 2]
        return (dx * dx + dy * dy) + dz * dz


def knn32(P32, Q32, k, r=np.inf, exclude=None, d2=None):
    """The contract of ncw_knn_query on the recentred float32 coordinates: per query the k smallest (d2, index) pairs in
    lexicographic order (np.lexsort((idx, d2))) among the points with d2 <= float32(r)^2 (inclusive) and index !=
    exclude[j]; a NaN or infinite query gets nothing.  Returns (dist [N,k] float32 = sqrt(d2), idx [N,k] int32, count [N]
    int32), rows beyond count +inf / -1.  `d2`: d2_matrix(P32, Q32) if the caller has it already."""
    P32, Q32 = np.asarray(P32, dtype=np.float32).reshape(-1, 3), np.asarray(Q32, dtype=np.float32).reshape(-1, 3)
    n, m = Q32.shape[0], P32.shape[0]
    if d2 is None:
        d2 = d2_matrix(P32, Q32)
    rr = np.float32(r)
    r2 = rr * rr
    with np.errstate(invalid="ignore"):
        adm = d2 <= r2
    adm &= np.isfinite(Q32).all(1)[:, None]
    if exclude is not None:
        ex = np.asarray(exclude).astype(np.int64)
        adm &= np.arange(m)[None, :] != ex[:, None]
    dist = np.full((n, k), INF32, dtype=np.float32)
    idx = np.full((n, k), -1, dtype=np.int32)
    count = np.minimum(adm.sum(1), k).astype(np.int32)
    if m == 0:
        return dist, idx, count
    # only the points at or below the k-th smallest admitted d2 can enter a row: sort those, by (d2, index)
    d2m = np.where(adm, d2, INF32)
    kth = np.partition(d2m, min(k, m) - 1, axis=1)[:, min(k, m) - 1] if m else None
    cand = adm & (d2m <= kth[:, None])
    for j in range(n):
        ids = np.nonzero(cand[j])[0]
        if ids.size == 0:
            continue
        order = np.lexsort((ids, d2[j, ids]))[:k]
        sel = ids[order]
        assert sel.size == count[j]
        idx[j, :sel.size] = sel
        dist[j, :sel.size] = np.sqrt(d2[j, sel])
    return dist, idx, count


JACOBI_SWEEPS = 8


def _rot(A, V, p, q, r):
    """One Jacobi rotation of ncw_knn_pca in the (p, q) plane; r the third index.  A: dict of the six entries keyed (i, j), i <=
    j; V: [3][3] list of arrays (row, column).  Skipped, row by row, where the off-diagonal is exactly 0."""
    key = lambda i, j: (i, j) if i <= j else (j, i)
    app, aqq, apq = A[(p, p)], A[(q, q)], A[key(p, q)]
    arp, arq = A[key(r, p)], A[key(r, q)]
    go = apq != 0.0
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * apq)
        tm = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        t = np.where(theta < 0.0, -tm, tm)
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        tap = t * apq
        A[(p, p)] = np.where(go, app - tap, app)
        A[(q, q)] = np.where(go, aqq + tap, aqq)
        A[key(p, q)] = np.where(go, 0.0, apq)
        A[key(r, p)] = np.where(go, c * arp - s * arq, arp)
        A[key(r, q)] = np.where(go, s * arp + c * arq, arq)
        for i in range(3):
            vp, vq = V[i][p], V[i][q]
            V[i][p] = np.where(go, c * vp - s * vq, vp)
            V[i][q] = np.where(go, s * vp + c * vq, vq)


def pca_ref(pts32, ref32, idx, count, with_query=True, toward=None, return_normal64=False):
    """ncw_knn_pca op for op in float64: (normal [N,3] float32, eig [N,3] float64 ascending, curvature [N] float32, valid [N]
    bool).  toward: 3 numbers, used as float32.  return_normal64: also the float64 vector the float32 normal is cast from."""
    pts = np.asarray(pts32, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    ref = np.asarray(ref32, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    idx = np.asarray(idx).astype(np.int64)
    n, k = idx.shape
    cnt = np.clip(np.asarray(count).astype(np.int64), 0, k)
    bad = (idx < 0) | (idx >= ref.shape[0])                              # a list ends at an index outside the cloud
    first_bad = np.where(bad.any(1), bad.argmax(1), k)
    cnt = np.minimum(cnt, first_bad)
    safe = np.where(bad, 0, idx)
    m = cnt + (1 if with_query else 0)
    dn = np.maximum(m, 1).astype(np.float64)
    members = ([(np.ones(n, dtype=bool), pts)] if with_query else []) + \
        [(r < cnt, ref[safe[:, r]] if ref.shape[0] else np.zeros((n, 3))) for r in range(k)]
    s = [np.zeros(n), np.zeros(n), np.zeros(n)]
    for on, a in members:
        for c in range(3):
            s[c] = np.where(on, s[c] + a[:, c], s[c])
    mean = [s[c] / dn for c in range(3)]
    cov = {(i, j): np.zeros(n) for i in range(3) for j in range(i, 3)}
    for on, a in members:
        d = [a[:, c] - mean[c] for c in range(3)]
        for (i, j) in cov:
            cov[(i, j)] = np.where(on, cov[(i, j)] + d[i] * d[j], cov[(i, j)])
    A = {key: v / dn for key, v in cov.items()}
    V = [[np.full(n, 1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
    for _ in range(JACOBI_SWEEPS):
        _rot(A, V, 0, 1, 2)
        _rot(A, V, 0, 2, 1)
        _rot(A, V, 1, 2, 0)
    lam = [A[(0, 0)], A[(1, 1)], A[(2, 2)]]
    vec = [[V[0][c], V[1][c], V[2][c]] for c in range(3)]           # vec[c] = column c = (x, y, z)

    def swap(a, b):
        sw = lam[b] < lam[a]
        lam[a], lam[b] = np.where(sw, lam[b], lam[a]), np.where(sw, lam[a], lam[b])
        for c in range(3):
            vec[a][c], vec[b][c] = np.where(sw, vec[b][c], vec[a][c]), np.where(sw, vec[a][c], vec[b][c])

    swap(0, 1)
    swap(1, 2)
    swap(0, 1)
    e = vec[0]
    with np.errstate(all="ignore"):
        length = np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
        nrm = [e[c] / length for c in range(3)]
    none = m == 0
    lam = [np.where(none, 0.0, v) for v in lam]
    valid = (m >= 3) & (lam[1] > 1e-10 * lam[2])
    if toward is not None:
        t = np.asarray(toward, dtype=np.float32).astype(np.float64)
        sdot = nrm[0] * (t[0] - pts[:, 0]) + nrm[1] * (t[1] - pts[:, 1]) + nrm[2] * (t[2] - pts[:, 2])
        flip = sdot < 0.0
    else:
        big = nrm[0]
        big = np.where(np.abs(nrm[1]) > np.abs(big), nrm[1], big)
        big = np.where(np.abs(nrm[2]) > np.abs(big), nrm[2], big)
        flip = big < 0.0
    normal64 = np.stack([np.where(valid, np.where(flip, -v, v), 0.0) for v in nrm], -1)
    normal = normal64.astype(np.float32)
    eig = np.stack(lam, -1)
    tot = lam[0] + lam[1] + lam[2]
    with np.errstate(all="ignore"):
        curv = np.where(tot == 0.0, 0.0, lam[0] / tot).astype(np.float32)
    return (normal, eig, curv, valid, normal64) if return_normal64 else (normal, eig, curv, valid)


def outliers_ref(P, k=16, ratio=2.0):
    """cloudops.remove_statistical_outliers in numpy: (keep [N] bool, mean_dist [N] float64).  The k float32 distances of a
    row sum exactly in float64, so mean_dist does not depend on the order of the sum."""
    (p32,), _ = recentre32(P)
    if p32.shape[0] <= k:
        raise ValueError("outliers_ref: %d points are no more than k = %d" % (p32.shape[0], k))
    dist, _, _ = knn32(p32, p32, k, exclude=np.arange(p32.shape[0]))
    m = dist.astype(np.float64).sum(1) / float(k)
    mu, sigma = m.mean(), m.std()
    return m <= mu + float(ratio) * sigma, m
