"""GPU: `ncw_pixel_nearest` (csrc/ncw_gtreproj.hip) called directly, with canary bytes around `best`: bit for bit against the
float32 restatement of its contract (tests/_gtreproj_ref.py) at the shape edges, at the 0.5 boundaries of the pixel (which pins
"the prefilter is a superset of the exact test") and on the fixture of tests/golden/make_golden_gtreproj.py, against float64 on
the band-free fixture, and for any split of the cloud into launches."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import _gtreproj_ref as GR
from tests._util import GOLDEN

pytestmark = pytest.mark.gpu

CANARY = 0x5A
PAD = 64
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def _launch(table, xyz, p0=0, clear=1, best=None, null=(), n_queries=None, n=None):
    """One direct call; `best` lives inside a larger buffer of canary bytes (prefilled with `best`, or with canaries).  Returns
    (code, keys uint64 [Q], canaries intact)."""
    from neuralrecon_w_amd import lib as L

    nq = len(table)
    q_d = torch.frombuffer(bytearray(table.tobytes()), dtype=torch.uint8).cuda()
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    x_d = torch.from_numpy(xyz if len(xyz) else np.zeros((1, 3), dtype=np.float32)).cuda()
    buf = torch.full((8 * nq + 2 * PAD,), CANARY, dtype=torch.uint8, device="cuda")
    if best is not None:
        buf[PAD:PAD + 8 * nq] = torch.from_numpy(np.asarray(best, dtype=np.uint64).view(np.uint8).copy()).cuda()
    ptrs = {"queries": q_d.data_ptr(), "xyz": x_d.data_ptr(), "best": buf.data_ptr() + PAD}
    for k in null:
        ptrs[k] = 0
    code = L.get_lib().ncw_pixel_nearest(C.c_void_p(ptrs["queries"]), nq if n_queries is None else n_queries, C.c_void_p(ptrs["xyz"]), p0,
                                         len(xyz) if n is None else n, clear, C.c_void_p(ptrs["best"]), L.stream_ptr())
    torch.cuda.synchronize()
    intact = bool((buf[:PAD] == CANARY).all() and (buf[-PAD:] == CANARY).all())
    return code, buf[PAD:PAD + 8 * nq].cpu().numpy().view(np.uint64).copy(), intact


def _table(w2c, intr, xy):
    from neuralrecon_w_amd import gtreproj

    return gtreproj.query_table(w2c, intr, xy, np.zeros(3))


# ---------------------------------------------------------------------------------------------------------------------
# a small synthetic scene: 16 x 12 images, so that every query is hit by many of a few thousand points
# ---------------------------------------------------------------------------------------------------------------------
W_, H_ = 16, 12


@pytest.fixture(scope="module")
def synth():
    """513 queries (two query tiles + 1) over 3 * 2048 + 77 points; the restatement's keys are computed per slice, on demand."""
    from neuralrecon_w_amd import lib as L

    assert (L.PIXNN_WG_POINTS, L.PIXNN_QUERY_TILE) == (2048, 256)
    rs = np.random.RandomState(11)
    nq, n = 2 * L.PIXNN_QUERY_TILE + 1, 3 * L.PIXNN_WG_POINTS + 77
    w2c = np.zeros((nq, 3, 4))
    for q in range(nq):
        u = rs.normal(size=3)
        pos = u / np.linalg.norm(u) * rs.uniform(2.5, 3.5)
        z = rs.uniform(-0.2, 0.2, 3) - pos
        z /= np.linalg.norm(z)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        w2c[q, :, :3], w2c[q, :, 3] = R, -R @ pos
    intr = np.tile(np.array([14.0, 15.0, W_ / 2 + 0.25, H_ / 2 - 0.5]), (nq, 1))
    xy = rs.uniform(0, [W_ - 1, H_ - 1], size=(nq, 2))
    xy[::7] = np.floor(xy[::7]) + 0.5  # key-points at k + 0.5: ties to even
    pts = rs.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    pts[5::97] = pts[4::97][:len(pts[5::97])]  # exact duplicates: equal depths resolve to the lower index
    return _table(w2c, intr, xy), pts


def _edges():
    wg, qt = 2048, 256
    pts = [1, 63, 64, 65, wg - 1, wg, wg + 1, 3 * wg + 77]
    qs = [1, qt - 1, qt, qt + 1, 2 * qt + 1]
    cases = [(n, 3) for n in pts] + [(n, qt + 1) for n in (1, 65, wg + 1, 3 * wg + 77)] + [(wg + 1, q) for q in qs] + [(3 * wg + 77, 2 * qt + 1)]
    return sorted(set(cases))


@pytest.mark.parametrize("n,nq", _edges())
def test_shape_edges_bitwise(synth, n, nq):
    table, pts = synth
    code, keys, intact = _launch(table[:nq], pts[:n])
    assert code == 0 and intact
    want = GR.pixel_nearest_f32(table[:nq], pts[:n])
    assert np.array_equal(keys, want)
    if n >= 2048:
        assert (keys != ALL_ONES).mean() > 0.5  # the scene does exercise the hit path


# ---------------------------------------------------------------------------------------------------------------------
# the 0.5 boundaries, exactly: identity view, fx = fy = 64, so that u = 64 x / z + cx is exact in float32
# ---------------------------------------------------------------------------------------------------------------------
def _boundary_case():
    eye = np.zeros((3, 4))
    eye[:, :3] = np.eye(3)
    fx = fy = 64.0
    cx, cy = 32.0, 24.0
    qxy = [(10.0, 7.0), (11.0, 8.0), (10.5, 7.5), (11.5, 8.5), (0.0, 0.0), (63.0, 47.0), (40.3, 20.7)]
    pts = []
    for X, Y in {(float(np.rint(np.float32(a))), float(np.rint(np.float32(b)))) for a, b in qxy}:
        for z in (1.0, 2.0, 0.75, 3.0):
            for axis in (0, 1):
                for side in (-0.5, 0.5):
                    for ulps in range(-4, 5):
                        uv = np.array([X + 0.1, Y - 0.2], dtype=np.float32)
                        b = np.float32((X, Y)[axis] + side)
                        for _ in range(abs(ulps)):
                            b = np.nextafter(b, np.float32(np.inf if ulps > 0 else -np.inf), dtype=np.float32)
                        uv[axis] = b
                        # x = (u - cx) z / fx in float64, then float32: at z = 1, 2 the float32 projection lands on u exactly, at
                        # z = 0.75, 3 within an ulp or two of it
                        pts.append(((float(uv[0]) - cx) * z / fx, (float(uv[1]) - cy) * z / fy, z))
    pts = np.array(pts, dtype=np.float32)
    n = len(qxy)
    table = _table(np.tile(eye, (n, 1, 1)), np.tile([fx, fy, cx, cy], (n, 1)), np.array(qxy))
    return table, pts


def test_boundaries_bitwise_prefilter_is_a_superset():
    table, pts = _boundary_case()
    want = GR.pixel_nearest_f32(table, pts)
    # the case does straddle the boundary: per query, points on the boundary itself, inside and outside it
    w, k, xy = GR._rows(table)
    edge_in = edge_out = 0
    for q in range(len(table)):
        u, v, c2 = GR.project_f32(w[q], k[q], pts)
        X, Y = np.rint(xy[q])
        on_edge = ((np.abs(u - X) == 0.5) & (np.abs(v - Y) < 0.5)) | ((np.abs(v - Y) == 0.5) & (np.abs(u - X) < 0.5))
        hit = (np.rint(u) == X) & (np.rint(v) == Y)
        assert on_edge.sum() >= 8
        edge_in, edge_out = edge_in + int((on_edge & hit).sum()), edge_out + int((on_edge & ~hit).sum())
        just_in = hit & ((np.abs(u - X) > 0.4999) | (np.abs(v - Y) > 0.4999))
        assert just_in.sum() >= 16
    assert edge_in >= 50 and edge_out >= 50  # ties to even: an edge at an even pixel belongs to it, at an odd one it does not
    code, keys, intact = _launch(table, pts)
    assert code == 0 and intact and np.array_equal(keys, want)
    # every point alone against every query: a pair the prefilter drops although the exact test passes shows here as all-ones
    for i in np.flatnonzero(np.isin(np.arange(len(pts)), np.arange(0, len(pts), 11))):
        code, k1, intact = _launch(table, pts[i:i + 1], p0=int(i))
        assert code == 0 and intact and np.array_equal(k1, GR.pixel_nearest_f32(table, pts[i:i + 1], p0=int(i)))


# ---------------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "gtreproj_golden.npz"))


@pytest.fixture(scope="module")
def fixture_queries(gold):
    """The fixture's queries as the host module feeds them (recentred), the band-free cloud and the cloud with the marked band
    points appended, all float32."""
    from neuralrecon_w_amd import gtreproj

    cloud = gold["cloud"].astype(np.float64)
    centre = gtreproj.cloud_centre(cloud)
    table = gtreproj.query_table(gold["query_w2c"], gold["query_intr"], gold["sel_obs_xy"][gold["sel_seg_start"][:-1]], centre)
    free = (cloud - centre).astype(np.float32)
    band = (gold["band_points"].astype(np.float64) - centre).astype(np.float32)
    return table, free, np.concatenate([free, band])


def test_fixture_bitwise_with_band_points(fixture_queries):
    table, free, both = fixture_queries
    code, keys, intact = _launch(table, both)
    assert code == 0 and intact
    assert np.array_equal(keys, GR.pixel_nearest_f32(table, both))
    # the band points do matter to the float32 answer of some query, or at least project onto its pixel
    w, k, xy = GR._rows(table)
    on = 0
    for q in range(6):
        u, v, c2 = GR.project_f32(w[q], k[q], both[len(free):])
        on += int(((np.rint(u) == np.rint(xy[q, 0])) & (np.rint(v) == np.rint(xy[q, 1]))).sum())
    assert on >= 20


def test_fixture_equals_float64_and_the_reference(fixture_queries, gold):
    from neuralrecon_w_amd import gtreproj

    table, free, _ = fixture_queries
    code, keys, intact = _launch(table, free)
    assert code == 0 and intact
    idx, depth = gtreproj.split_keys(keys)
    assert np.array_equal(idx, gold["index_f64"])      # every query, none left out
    assert np.array_equal(idx, gold["ref_gt_index"])   # and the reference's own choice
    assert (depth > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# depth and ordering
# ---------------------------------------------------------------------------------------------------------------------
def test_depth_and_ordering_cases():
    eye = np.zeros((3, 4))
    eye[:, :3] = np.eye(3)
    neg = eye.copy()
    neg[2] = [-0.0, -0.0, 1.0, -0.0]  # with x, y > 0 and z = -0.0 every term of c_2 is -0: c_2 == -0.0
    f, cx, cy = 64.0, 32.0, 24.0

    def at(u, v, z):
        return ((u - cx) * z / f, (v - cy) * z / f, z)

    pts = np.array([
        at(10.0, 7.0, -1.0),    # 0: BEHIND the camera, projects onto (10, 7)
        at(10.0, 7.0, 3.0),     # 1: on (10, 7), far
        at(10.2, 6.9, 2.0),     # 2: on (10, 7), nearest  -> query 0
        at(11.0, 7.0, 1.0),     # 3: nearer, but on the neighbouring pixel (11, 7)
        at(20.0, 9.0, 2.5),     # 4: on (20, 9)
        at(20.0, 9.0, 2.5),     # 5: the same point again: equal depth -> the lower index, 4
        (0.0, 0.0, 0.0),        # 6: c_2 == 0, numerators 0
        (0.3, 0.2, 0.0),        # 7: c_2 == 0, numerators not 0
        (0.3, 0.2, -0.0),       # 8: with the view `neg`: c_2 == -0.0
        at(30.0, 30.0, 1e-30),  # 9: c_2 far below the range the bound is argued for: goes to the exact test, and hits (30, 30)
        at(5.0, 40.0, 1e30),    # 10: c_2 far above it: hits (5, 40)
    ], dtype=np.float32)
    qxy = np.array([(10.0, 7.0), (20.0, 9.0), (50.0, 40.0), (32.0, 24.0), (32.0, 24.0), (30.0, 30.0), (5.0, 40.0)])
    w2c = np.tile(eye, (len(qxy), 1, 1))
    w2c[4] = neg
    table = _table(w2c, np.tile([f, f, cx, cy], (len(qxy), 1)), qxy)
    table["w2c"][4, 11] = np.float32(-0.0)  # query_table adds the (zero) shift to the translation, which makes it +0.0
    assert np.signbit(table["w2c"][4][8]) and np.signbit(table["w2c"][4][11])  # the -0.0 reached the table
    code, keys, intact = _launch(table, pts, p0=100)
    assert code == 0 and intact
    assert np.array_equal(keys, GR.pixel_nearest_f32(table, pts, p0=100))

    def key(depth, i):
        return np.uint64((int(np.float32(depth).view(np.uint32)) << 32) | (100 + i))

    assert keys[0] == key(2.0, 2)    # not 0 (behind), not 1 (farther), not 3 (nearer, other pixel)
    assert keys[1] == key(2.5, 4)    # equal depths: the lower index
    assert keys[2] == ALL_ONES       # nothing hits
    assert keys[3] == ALL_ONES       # c_2 == 0 at the principal point: 0 / 0 and x / 0 hit nothing
    assert keys[4] == ALL_ONES       # c_2 == -0.0 hits nothing either
    assert keys[5] == key(1e-30, 9) and keys[6] == key(1e30, 10)


# ---------------------------------------------------------------------------------------------------------------------
# splits, repeats, permutation
# ---------------------------------------------------------------------------------------------------------------------
def test_splits_repeats_and_permutation(fixture_queries):
    from neuralrecon_w_amd import gtreproj

    table, _, both = fixture_queries
    code, whole, intact = _launch(table, both)
    assert code == 0 and intact
    for cut in (1, 64, 1000):
        code, part, intact = _launch(table, both[:cut])
        assert code == 0 and intact
        code, part, intact = _launch(table, both[cut:], p0=cut, clear=0, best=part)
        assert code == 0 and intact and np.array_equal(part, whole)
    # in the other order too, and in three pieces
    code, part, intact = _launch(table, both[1000:], p0=1000)
    code, part, _ = _launch(table, both[:64], p0=0, clear=0, best=part)
    code, part, _ = _launch(table, both[64:1000], p0=64, clear=0, best=part)
    assert np.array_equal(part, whole)
    code, again, intact = _launch(table, both)
    assert np.array_equal(again, whole)
    # the points permuted: the same POINT on every query whose nearest depth is not shared by two hits
    perm = np.random.RandomState(3).permutation(len(both))
    code, pk, intact = _launch(table, both[perm])
    assert code == 0 and intact
    i0, d0 = gtreproj.split_keys(whole)
    i1, d1 = gtreproj.split_keys(pk)
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    w, k, xy = GR._rows(table)
    checked = 0
    for q in range(len(table)):
        u, v, c2 = GR.project_f32(w[q], k[q], both)
        hit = (np.rint(u) == np.rint(xy[q, 0])) & (np.rint(v) == np.rint(xy[q, 1])) & (c2 >= 0)
        if (c2[hit] == d0[q]).sum() == 1:
            assert np.array_equal(both[i0[q]], both[perm][i1[q]])
            checked += 1
    assert checked >= len(table) - 2


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_and_clear(synth):
    table, pts = synth
    table, pts = table[:5], pts[:100]
    untouched = np.frombuffer(bytes([CANARY]) * 40, dtype=np.uint64)
    for kw in (dict(null=("queries",)), dict(null=("xyz",)), dict(null=("best",)), dict(n_queries=0), dict(n_queries=-3), dict(n=-1),
               dict(p0=-1), dict(p0=2 ** 32 - 1 - 99), dict(p0=2 ** 32), dict(p0=2 ** 40, n=0)):
        code, keys, intact = _launch(table, pts, **kw)
        assert code == -1, kw  # NCW_E_BADARG
        assert intact and np.array_equal(keys, untouched), kw
    # the largest range that is allowed: p0 + n == 2^32 - 1
    code, keys, intact = _launch(table, pts, p0=2 ** 32 - 1 - 100)
    assert code == 0 and intact and np.array_equal(keys, GR.pixel_nearest_f32(table, pts, p0=2 ** 32 - 1 - 100))
    assert (keys != ALL_ONES).any() and ((keys[keys != ALL_ONES] & np.uint64(0xFFFFFFFF)) >= np.uint64(2 ** 32 - 1 - 100)).all()
    # n == 0 with clear set only clears; without it nothing is written
    code, keys, intact = _launch(table, pts, n=0, clear=1)
    assert code == 0 and intact and (keys == ALL_ONES).all()
    code, keys, intact = _launch(table, pts, n=0, clear=0)
    assert code == 0 and intact and np.array_equal(keys, untouched)
