"""GPU: area-weighted surface sampling (csrc/ncw_surf.hip) and the surface scoring of evalmesh.eval_mesh.

The kernels are compared with the numpy restatement of tests/_surf_ref.py on a mesh of F = 1000 random triangles at offset
(1000, -2000, 500) with edges of about 1e-2 -- where f32 vertices would already cost 1e-4 -- holding two degenerate triangles,
corner indices out of range on both sides, an overflowing (non-finite) area, zero-weight triangles in first and last
position, a corner exactly on the crop box and a box that removes about a third of the triangles.  The triangles are
well-shaped on purpose (edges 0.8e-2 .. 1.2e-2, angle at A 50 .. 70 degrees): a coordinate near 2000 carries 2.3e-13 of
rounding, which is 1e-10 of such a triangle's height, so the barycentric bound of -1e-9 checks the kernel and not the
conditioning of a sliver."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from tests import _surf_ref as R
from tests._util import ROOT

from neuralrecon_w_amd import evalmesh, lib as L, mesh, reproj

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
F = 1000
OFFSET = np.array([1000.0, -2000.0, 500.0])
BOX = [[999.0, -2001.0, 499.0], [1000.17, -1999.0, 501.0]]  # cuts x: triangle bases are uniform in offset +- 0.5
ZERO_FACES = (0, 10, 11, 20, 21, 30, F - 1)               # weight 0 with or without the box
ON_BOX = 40                                               # a corner exactly on the box's upper x face: kept (closed box)


def _mesh():
    rng = np.random.RandomState(0)
    base = OFFSET + rng.uniform(-0.5, 0.5, (F, 3))
    q = np.linalg.qr(rng.randn(F, 3, 3))[0]
    e1, e2 = q[:, :, 0], q[:, :, 1]
    l1, l2 = rng.uniform(0.8e-2, 1.2e-2, (2, F, 1))
    th = np.deg2rad(rng.uniform(50, 70, (F, 1)))
    tri = np.stack([base, base + l1 * e1, base + l2 * (np.cos(th) * e1 + np.sin(th) * e2)], 1)
    tri[ON_BOX] += [BOX[1][0] - tri[ON_BOX, :, 0].max(), 0, 0]
    tri[ON_BOX, np.argmax(tri[ON_BOX, :, 0]), 0] = BOX[1][0]
    verts = tri.reshape(-1, 3).copy()
    faces = np.arange(3 * F, dtype=np.int64).reshape(F, 3)
    faces[0] = [0, 0, 1]                 # degenerate (A == B), first position
    faces[10] = [30, 31, 31]             # degenerate (B == C)
    faces[11] = [33, 33, 33]
    faces[20] = [60, 3 * F + 7, 62]      # corner index past the end
    faces[21] = [-1, 64, 65]             # negative corner index
    verts[90] = [1e200, -1e200, 1e200]   # face 30: the area overflows
    faces[F - 1] = [3 * F, 5, 6]         # last position, first index past the end
    return verts, faces


@pytest.fixture(scope="module")
def case():
    verts, faces = _mesh()
    v = torch.from_numpy(verts).to(DEV)
    f = torch.from_numpy(faces).int().to(DEV)
    w = evalmesh.surface_weights(v, f, BOX)
    cdf = evalmesh.surface_cdf(w)
    torch.cuda.synchronize()
    return {"verts": verts, "faces": faces, "v": v, "f": f, "w": w.cpu().numpy(), "cdf_t": cdf, "cdf": cdf.cpu().numpy()}


def _pick(cdf, x):
    cdf_t = torch.as_tensor(np.asarray(cdf, dtype=np.float64)).to(DEV).contiguous()
    x_t = torch.as_tensor(np.asarray(x, dtype=np.float64)).to(DEV).contiguous()
    tri = torch.full((x_t.shape[0],), -7, dtype=torch.int32, device=DEV)
    L.check(L.get_lib().ncw_surf_pick(L.ptr(cdf_t), cdf_t.shape[0], L.ptr(x_t), x_t.shape[0], L.ptr(tri), L.stream_ptr(tri.device)),
            "ncw_surf_pick")
    return tri.cpu().numpy().astype(np.int64)


def _sample(c, seed, i0, n, n_total, mode):
    pts = torch.empty(n, 3, dtype=torch.float64, device=DEV)
    tri = torch.empty(n, dtype=torch.int32, device=DEV)
    urr = torch.empty(n, 3, dtype=torch.float64, device=DEV)
    L.check(L.get_lib().ncw_surf_sample(L.ptr(c["v"]), L.ptr(c["f"]), L.ptr(c["cdf_t"]), c["f"].shape[0], seed, i0, n, n_total, mode,
                                        L.ptr(pts), L.ptr(tri), L.ptr(urr), L.stream_ptr(pts.device)), "ncw_surf_sample")
    return pts.cpu().numpy(), tri.cpu().numpy().astype(np.int64), urr.cpu().numpy()


# ---------------------------------------------------------------------------------------------------
# 1. weights
# ---------------------------------------------------------------------------------------------------
def test_weights_match_the_restatement_and_the_zeros_are_exact(case):
    for box in (None, BOX):
        got = evalmesh.surface_weights(case["v"], case["f"], box).cpu().numpy()
        ref = R.weights(case["verts"], case["faces"], box)
        err = np.abs(got - ref)
        print("weights box=%s: max rel err %.3e, zeros %d" % (box is not None, float((err[ref > 0] / ref[ref > 0]).max()),
                                                              int((got == 0).sum())))
        assert (err <= 1e-13 * ref).all()
        assert np.array_equal(got == 0, ref == 0) and all(got[k] == 0 for k in ZERO_FACES)
        assert got[ON_BOX] > 0 and np.isfinite(got).all() and (got >= 0).all()
    n_cut = int(((ref == 0) & (R.weights(case["verts"], case["faces"]) > 0)).sum())
    assert F // 4 < n_cut < F // 2  # the box removes about a third
    # one ulp less box and the triangle with a corner on the face goes
    tight = [BOX[0], [np.nextafter(BOX[1][0], 0), BOX[1][1], BOX[1][2]]]
    assert float(evalmesh.surface_weights(case["v"], case["f"], tight)[ON_BOX]) == 0.0
    assert evalmesh.surface_weights(case["v"], case["f"][:0], BOX).shape == (0,)


def test_cdf_repeats_its_predecessor_at_every_zero_weight(case):
    w, cdf = case["w"], case["cdf"]
    assert cdf[0] == 0 and (np.diff(cdf) >= 0).all()
    z = np.nonzero(w == 0)[0]
    assert (cdf[z[z > 0]] == cdf[z[z > 0] - 1]).all()
    assert abs(cdf[-1] - w.sum()) <= 1e-12 * w.sum()


# ---------------------------------------------------------------------------------------------------
# 2. pick
# ---------------------------------------------------------------------------------------------------
def _probe(cdf):
    cdf = np.asarray(cdf, dtype=np.float64)
    return np.concatenate([cdf, np.nextafter(cdf, -np.inf), np.nextafter(cdf, np.inf),
                           [0.0, -1.0, np.nan, cdf[-1], 2 * cdf[-1], -0.0, np.inf, -np.inf]])


def test_pick_is_searchsorted_right_with_the_end_rule(case):
    x = _probe(case["cdf"])
    got = _pick(case["cdf"], x)
    assert np.array_equal(got, R.pick(case["cdf"], x))
    assert (case["w"][got] > 0).all()  # a triangle of weight 0 is never returned
    last_pos = int(np.nonzero(case["w"] > 0)[0][-1])
    assert got[-5] == last_pos and got[-4] == last_pos and got[-2] == last_pos  # cdf[-1], 2 cdf[-1], +inf
    first_pos = int(np.nonzero(case["w"] > 0)[0][0])
    assert got[-8] == first_pos and got[-7] == first_pos and got[-6] == first_pos and got[-1] == first_pos  # 0, -1, NaN, -inf


@pytest.mark.parametrize("weights, want_end", [([0.37], 0), ([0.0, 0.37], 1), ([0.37, 0.0], 0), ([0.25, 0.0, 0.0, 0.5, 0.0], 3)])
def test_pick_on_tiny_tables(weights, want_end):
    cdf = np.cumsum(np.array(weights))
    x = _probe(cdf)
    got = _pick(cdf, x)
    assert np.array_equal(got, R.pick(cdf, x)) and (np.array(weights)[got] > 0).all()
    assert got[-4] == want_end  # x = 2 cdf[-1]


# ---------------------------------------------------------------------------------------------------
# 3. random stream
# ---------------------------------------------------------------------------------------------------
N = 4097
SEED = 0x9E3779B97F4A7C15


def test_stream_matches_the_restatement_bit_for_bit(case):
    _, _, first = _sample(case, SEED, 0, N, N, 0)
    u, r1, r2, _ = R.stream(np.arange(N), SEED)
    assert np.array_equal(first, np.stack([u, r1, r2], -1))
    i0 = 2 ** 32 - 3  # the carry into the second counter word
    _, _, urr = _sample(case, SEED, i0, 8, 2 ** 32 + 5, 0)
    u, r1, r2, _ = R.stream(i0 + np.arange(8, dtype=np.uint64), SEED)
    assert np.array_equal(urr, np.stack([u, r1, r2], -1))
    _, _, urr0 = _sample(case, SEED + 1, 0, 64, 64, 0)
    assert not np.array_equal(urr0, first[:64]) and len(np.unique(urr0[:, 0])) == 64  # the seed is the key


def test_stratified_u_and_split_launches(case):
    _, _, urr = _sample(case, SEED, 0, N, N, 1)
    u, r1, r2, xi = R.stream(np.arange(N), SEED, 1, N)
    err = np.abs(urr[:, 0] - (np.arange(N) + xi) / N)
    print("stratified: max |u - (i + xi) / N| = %.3e" % err.max())
    assert (err <= 2.0 ** -52).all() and np.array_equal(urr[:, 1:], np.stack([r1, r2], -1))
    assert (np.diff(urr[:, 0]) > 0).all()  # u grows with the sample index
    for mode in (0, 1):
        whole = _sample(case, SEED, 0, N, N, mode)
        a, b = _sample(case, SEED, 0, 1500, N, mode), _sample(case, SEED, 1500, N - 1500, N, mode)
        for x, xa, xb in zip(whole, a, b):
            assert np.array_equal(x, np.concatenate([xa, xb]))  # pts, tri, urr: bitwise


def test_bad_arguments_are_refused(case):
    lib, s = L.get_lib(), L.stream_ptr(torch.device(DEV))
    pts = torch.empty(8, 3, dtype=torch.float64, device=DEV)
    args = lambda **k: [k.get("v", L.ptr(case["v"])), L.ptr(case["f"]), L.ptr(case["cdf_t"]), k.get("nf", F), 1, k.get("i0", 0), 8,  # noqa: E731
                        k.get("nt", 8), k.get("mode", 1), L.ptr(pts), None, None, s]
    assert lib.ncw_surf_sample(*args()) == 0
    for bad in (dict(v=None), dict(nf=0), dict(mode=2), dict(i0=1), dict(nt=0), dict(i0=-1)):
        assert lib.ncw_surf_sample(*args(**bad)) == -1, bad
    assert lib.ncw_surf_pick(L.ptr(case["cdf_t"]), 0, L.ptr(pts), 8, L.ptr(pts), s) == -1
    torch.cuda.synchronize()
    # an area table without area: nothing is read through the faces (here all out of range), NaN points, triangle -1
    empty = dict(case, f=torch.full((F, 3), 1 << 30, dtype=torch.int32, device=DEV), cdf_t=torch.zeros(F, dtype=torch.float64, device=DEV))
    p, t, urr = _sample(empty, SEED, 0, 100, 100, 1)
    assert np.isnan(p).all() and (t == -1).all() and np.array_equal(urr[:, 1], R.stream(np.arange(100), SEED)[1])


# ---------------------------------------------------------------------------------------------------
# 4. selection and geometry
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_selection_and_geometry(case, mode):
    pts, tri, urr = _sample(case, 3, 0, N, N, mode)
    assert np.array_equal(tri, R.pick(case["cdf"], urr[:, 0] * case["cdf"][-1]))
    assert (case["w"][tri] > 0).all() and len(np.unique(tri)) > 500
    want = R.points(case["verts"], case["faces"], tri, urr[:, 1], urr[:, 2])
    coord_max = float(np.abs(case["verts"][case["faces"][case["w"] > 0]]).max())
    err = float(np.abs(pts - want).max())
    print("mode %d: max |p - formula| = %.3e (bound %.3e)" % (mode, err, 64 * EPS64 * coord_max))
    assert err <= 64 * EPS64 * coord_max
    # barycentric coordinates recomputed in float64 from the points read back
    A, B, Cc = (case["verts"][case["faces"][tri, j]] for j in range(3))
    e1, e2, d = B - A, Cc - A, pts - A
    g11, g12, g22 = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
    b1, b2 = (d * e1).sum(-1), (d * e2).sum(-1)
    det = g11 * g22 - g12 * g12
    lb, lc = (b1 * g22 - b2 * g12) / det, (b2 * g11 - b1 * g12) / det
    bary = np.stack([1 - lb - lc, lb, lc], -1)
    off = np.abs(d - lb[:, None] * e1 - lc[:, None] * e2).max()
    print("mode %d: min barycentric %.3e, off-plane %.3e" % (mode, bary.min(), off))
    assert bary.min() >= -1e-9 and off <= 64 * EPS64 * coord_max


# ---------------------------------------------------------------------------------------------------
# 5. distribution
# ---------------------------------------------------------------------------------------------------
TWO_V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 1], [3, 0, 1], [0, 2, 1]])  # areas 1 and 3
TWO_F = np.array([[0, 1, 2], [3, 4, 5]])


@pytest.mark.parametrize("mode", ["stratified", "iid"])
def test_distribution_over_two_triangles(mode):
    n = 40000
    pts, tri = evalmesh.sample_surface(TWO_V, TWO_F, n, seed=11, mode=mode, return_index=True, device=DEV)
    assert pts.shape == (n, 3) and pts.dtype == torch.float64 and tri.dtype == torch.int32 and pts.is_cuda
    pts, tri = pts.cpu().numpy(), tri.cpu().numpy()
    counts = np.bincount(tri, minlength=2)
    print("%s: counts %s" % (mode, counts))
    tol = 1 if mode == "stratified" else 5 * math.sqrt(n * 0.25 * 0.75)
    assert abs(counts[0] - 10000) <= tol and abs(counts[1] - 30000) <= tol and counts.sum() == n
    for k in range(2):
        T = TWO_V[TWO_F[k]]
        p = pts[tri == k]
        # a uniform point of a triangle: mean = centroid, variance per axis = (sum x_i^2 - sum_{i<j} x_i x_j) / 18
        var = ((T * T).sum(0) - T[0] * T[1] - T[1] * T[2] - T[2] * T[0]) / 18
        dev = np.abs(p.mean(0) - T.mean(0))
        print("%s: triangle %d mean off by %s (5 sigma %s)" % (mode, k, dev, 5 * np.sqrt(var / len(p))))
        assert (dev <= 5 * np.sqrt(var / len(p)) + 1e-15).all()


def test_sample_surface_edges():
    one = evalmesh.sample_surface(TWO_V, TWO_F, 1, device=DEV)
    assert one.shape == (1, 3) and min(abs(one[0, 2].item()), abs(one[0, 2].item() - 1)) <= 4 * EPS64
    whole, tw = evalmesh.sample_surface(TWO_V, TWO_F, 5000, seed=5, return_index=True, device=DEV)
    parts, tp = evalmesh.sample_surface(torch.from_numpy(TWO_V).to(DEV), torch.from_numpy(TWO_F), 5000, seed=5, return_index=True, chunk=777)
    assert torch.equal(whole, parts) and torch.equal(tw, tp)
    assert not torch.equal(whole, evalmesh.sample_surface(TWO_V, TWO_F, 5000, seed=6, device=DEV))
    assert torch.equal(whole, evalmesh.sample_surface(TWO_V.astype(np.float32), TWO_F.astype(np.int16), 5000, seed=5, device=DEV))
    # a box that holds the first triangle only; an index that would wrap into range as int32
    only0 = evalmesh.sample_surface(TWO_V, TWO_F, 300, box=[[-1, -1, -0.5], [4, 3, 0.5]], return_index=True, device=DEV)[1]
    assert (only0 == 0).all()
    wrap = np.array([[0, 1, 2], [3, 4, 5 + 2 ** 32]])
    assert (evalmesh.sample_surface(TWO_V, wrap, 300, return_index=True, device=DEV)[1] == 0).all()
    # nothing to draw from
    for v, f in ((TWO_V, TWO_F[:0]), (TWO_V[:0], TWO_F), (TWO_V, np.array([[0, 0, 1], [2, 2, 2]]))):
        p, t = evalmesh.sample_surface(v, f, 100, return_index=True, device=DEV)
        assert p.shape == (0, 3) and t.shape == (0,) and p.dtype == torch.float64
    assert evalmesh.sample_surface(TWO_V, TWO_F, 100, box=[[5, 5, 5], [6, 6, 6]], device=DEV).shape == (0, 3)
    assert evalmesh.sample_surface(TWO_V, TWO_F, 0, device=DEV).shape == (0, 3)


def test_crops_on_the_device_select_the_numpy_rows():
    rng = np.random.RandomState(4)
    p = rng.uniform(-1.5, 1.5, (5000, 3)) + OFFSET
    p[0] = [OFFSET[0] + 1.0, OFFSET[1], OFFSET[2]]  # exactly on a face: dropped
    box = [(OFFSET - 1.0).tolist(), (OFFSET + [1.0, 0.5, 0.75]).tolist()]
    sfm = rng.uniform(-1.2, 1.2, (300, 3)) + OFFSET
    sfm[0] = OFFSET + [0, 0, 50.0]  # a cell outside [0, res)^3
    pt = torch.from_numpy(p).to(DEV)
    got = evalmesh.bbx_crop(pt, box)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), evalmesh.bbx_crop(p, box))
    got = evalmesh.sfm_crop(pt, sfm, 0.21, box)
    want = evalmesh.sfm_crop(p, sfm, 0.21, box)
    assert got.is_cuda and 100 < len(want) < 4900 and np.array_equal(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------
# 6. end to end
# ---------------------------------------------------------------------------------------------------
C30, S30 = math.cos(math.pi / 6), math.sin(math.pi / 6)
SFM2GT = np.array([[C30, -S30, 0, 10.0], [S30, C30, 0, -5.0], [0, 0, 1.0, 3.0], [0, 0, 0, 1]])  # rigid: the GT density stays
T03 = 0.03


def _to_gt(p):
    return p @ SFM2GT[:3, :3].T + SFM2GT[:3, 3]


def _to_sfm(p):
    return (p - SFM2GT[:3, 3]) @ SFM2GT[:3, :3]


@pytest.fixture(scope="module")
def square(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("surf")
    pred = str(tmp / "pred" / "square.ply")
    os.makedirs(os.path.dirname(pred))
    mesh.write_ply(pred, torch.tensor([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]), torch.tensor([[0, 1, 2], [0, 2, 3]]))
    rng = np.random.RandomState(7)
    g = np.concatenate([rng.uniform(0, 1, (2000, 2)), np.zeros((2000, 1))], 1)
    gt = str(tmp / "gt.ply")
    mesh.write_ply(gt, torch.from_numpy(_to_gt(g)), torch.zeros(0, 3, dtype=torch.int64))
    c = SFM2GT[:3, 3]
    scene = {"sfm2gt": SFM2GT.tolist(), "eval_bbx": [(c - 3.0).tolist(), (c + 3.0).tolist()]}
    m = evalmesh.eval_mesh(pred, gt, scene, is_mesh=True, threshold=[T03, 0.1], save_name="surf", verbose=False, surface=10,
                           error_clouds=[T03])
    return {"tmp": tmp, "pred": pred, "gt": gt, "scene": scene, "m": m, "out": os.path.join(os.path.dirname(pred), "eval_surf")}


def _brute(a, b):
    """float64: for every point of b its distance to the nearest point of a."""
    A, B = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    return torch.cat([((B[i:i + 256, None] - A[None]) ** 2).sum(-1).min(1).values.sqrt() for i in range(0, len(B), 256)]).cpu().numpy()


def _check_metrics(per, ts, vp, vt):
    d1, d2 = _brute(vp, vt), _brute(vt, vp)
    both = np.concatenate([vp, vt])
    bound = 8 * EPS32 * float(np.abs(both - (both.min(0) + both.max(0)) / 2).max())  # f32 after recentring (evalmesh.recentre)
    for t, got in zip(ts, per):
        for key, d in (("prec", d2), ("recal", d1)):
            lo_c, hi_c = int((d < t - bound).sum()), int((d < t + bound).sum())
            assert lo_c - 1e-6 <= got[key] * len(d) <= hi_c + 1e-6, (t, key, got[key] * len(d), lo_c, hi_c)
            if lo_c == hi_c:
                assert got[key] == max(lo_c / len(d), 1e-6), (t, key)
        # every distance is within `bound` of its float64 value, so the means are too
        print("t %.2f: dist1 off by %.3e, dist2 off by %.3e (bound %.3e)" % (t, abs(got["dist1"] - d2.mean()), abs(got["dist2"] - d1.mean()), bound))
        assert abs(got["dist1"] - d2.mean()) <= bound and abs(got["dist2"] - d1.mean()) <= bound
    return d1, d2


def test_eval_mesh_scores_the_surface(square):
    out = square["out"]
    assert sorted(os.listdir(out)) == ["down_gt.ply", "down_pred_in_gt.ply", "metrics.json", "visualize"]
    vp = reproj.read_ply_mesh(os.path.join(out, "down_pred_in_gt.ply"))[0]
    vt = evalmesh.read_ply_points(os.path.join(out, "down_gt.ply"))
    assert vt.shape == (2000, 3) and vp.shape == (20000, 3)
    s = _to_sfm(vp)
    print("surface samples: |z| <= %.3e, x, y in [%.3e, 1 + %.3e]" % (np.abs(s[:, 2]).max(), s[:, :2].min(), s[:, :2].max() - 1))
    assert np.abs(s[:, 2]).max() <= 1e-9 and s[:, :2].min() >= -1e-9 and s[:, :2].max() <= 1 + 1e-9
    assert 9000 < int((s[:, 1] > s[:, 0]).sum()) < 11000  # both triangles
    per = [json.load(open(os.path.join(out, "visualize", "%.2f" % t, "metrics.json"))) for t in (T03, 0.1)]
    d1, _ = _check_metrics(per, [T03, 0.1], vp, vt)
    print("surface=10: recal %.6f at %.2f, max GT -> sample distance %.4f" % (per[0]["recal"], T03, d1.max()))
    assert per[0]["recal"] == 1.0 and square["m"] == per[1]
    allm = json.load(open(os.path.join(out, "metrics.json")))
    assert allm["thresholds"] == [T03, 0.1] and allm["recals"] == [p["recal"] for p in per]


def test_eval_mesh_without_surface_scores_the_vertices_as_before(square):
    outs = []
    for name in ("v1", "v2"):
        m = evalmesh.eval_mesh(square["pred"], square["gt"], square["scene"], is_mesh=True, threshold=[T03], save_name=name,
                               verbose=False)
        out = os.path.join(os.path.dirname(square["pred"]), "eval_" + name)
        files = sorted(os.path.join(dp, f)[len(out):] for dp, _, fs in os.walk(out) for f in fs)
        assert files == ["/down_gt.ply", "/down_pred_in_gt.ply", "/metrics.json", "/visualize/0.03/metrics.json"]
        outs.append([open(out + f, "rb").read() for f in files])
        assert m["recal"] < 0.01
    assert outs[0] == outs[1]
    # down_pred_in_gt.ply: the four vertices in GT coordinates, float x / y / z with an empty face element
    ref = str(square["tmp"] / "ref.ply")
    corners = np.array([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    mesh.write_ply(ref, torch.from_numpy((SFM2GT[:3] @ np.c_[corners, np.ones(4)].T).T), torch.zeros(0, 3, dtype=torch.int64))
    assert outs[0][1] == open(ref, "rb").read()
    vt = evalmesh.read_ply_points(os.path.join(os.path.dirname(square["pred"]), "eval_v1", "down_gt.ply"))
    _check_metrics([json.loads(outs[0][3])], [T03], (SFM2GT[:3] @ np.c_[corners, np.ones(4)].T).T, vt)


def test_command_line_sample_surface_writes_the_same_metrics(square):
    cfg = str(square["tmp"] / "config.yaml")
    yaml.safe_dump(square["scene"], open(cfg, "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_mesh.py"), "--file_pred", square["pred"], "--file_trgt",
                        square["gt"], "--scene_config_path", cfg, "--mesh", "--threshold", "0.03,0.11,0.07", "--sample_surface",
                        "--save_name", "cli"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    cli = json.load(open(os.path.join(os.path.dirname(square["pred"]), "eval_cli", "metrics.json")))
    ref = json.load(open(os.path.join(square["out"], "metrics.json")))
    assert cli["thresholds"] == [float(v) for v in np.arange(0.03, 0.11, 0.07)] and len(cli["thresholds"]) == 2
    assert cli["fscores"][0] == ref["fscores"][0] and cli["precs"][0] == ref["precs"][0] and cli["recals"][0] == ref["recals"][0]
    a, b = (open(os.path.join(os.path.dirname(square["pred"]), d, "down_pred_in_gt.ply"), "rb").read() for d in ("eval_cli", "eval_surf"))
    assert a == b


def test_box_that_cuts_a_corner_leaves_the_other_triangle(square):
    # in GT coordinates corner 1 = (1, 0, 0) has the largest x (t_x + 0.866; the others: 0, 0.366, -0.5): the box drops
    # the triangle (0, 1, 2) that owns it and keeps (0, 2, 3)
    c = SFM2GT[:3, 3]
    scene = {"sfm2gt": SFM2GT.tolist(), "eval_bbx": [(c - 3.0).tolist(), (c + [0.7, 3.0, 3.0]).tolist()]}
    evalmesh.eval_mesh(square["pred"], square["gt"], scene, is_mesh=True, threshold=[T03], save_name="cut", verbose=False,
                       surface=10, surface_mode="iid", surface_seed=3)
    out = os.path.join(os.path.dirname(square["pred"]), "eval_cut")
    n_gt = evalmesh.read_ply_points(os.path.join(out, "down_gt.ply")).shape[0]
    s = _to_sfm(reproj.read_ply_mesh(os.path.join(out, "down_pred_in_gt.ply"))[0])
    assert 1000 < n_gt < 2000 and s.shape == (10 * n_gt, 3)
    assert (s[:, 1] >= s[:, 0] - 1e-9).all() and np.abs(s[:, 2]).max() <= 1e-9
    with pytest.raises(ValueError, match="no faces"):
        evalmesh.eval_mesh(square["gt"], square["gt"], scene, is_mesh=True, threshold=[T03], save_name="nofaces", verbose=False,
                           surface=10)


def test_error_clouds_are_the_table_lookup_of_the_distances(square):
    d = os.path.join(square["out"], "visualize", "%.2f" % T03)
    assert sorted(os.listdir(d)) == ["error_gt_recal.ply", "error_pred_precision.ply", "metrics.json"]
    assert sorted(os.listdir(os.path.join(square["out"], "visualize", "0.10"))) == ["metrics.json"]  # only the listed threshold
    pp, _, pc = reproj.read_ply_mesh(os.path.join(d, "error_pred_precision.ply"))
    gp, _, gc = reproj.read_ply_mesh(os.path.join(d, "error_gt_recal.ply"))
    assert pp.shape == (20000, 3) and gp.shape == (2000, 3) and pc.dtype == np.uint8 and gc.dtype == np.uint8
    assert np.array_equal(pp, reproj.read_ply_mesh(os.path.join(square["out"], "down_pred_in_gt.ply"))[0])
    P, G = torch.from_numpy(pp).to(DEV), torch.from_numpy(gp).to(DEV)
    for pts, cols, dist in ((gp, gc, evalmesh.nn_distances(P, G)[0]), (pp, pc, evalmesh.nn_distances(G, P)[0])):
        dd = dist.double().cpu().numpy()
        idx = np.minimum((np.minimum(dd, 3 * T03) / (3 * T03) * 256).astype(np.int64), 255)
        assert np.array_equal(cols, evalmesh.JET_U8[idx]) and len(np.unique(idx)) > 10
