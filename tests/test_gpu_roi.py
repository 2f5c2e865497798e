"""GPU: `ncw_views_roi` (csrc/ncw_roi.hip) -- the region-of-interest test of every view of a scene in ONE launch -- on the nine
ragged views of tests/golden/split_scene, against the float64 restatement of dataset_filter_utils.py:168-177 (tests/_roi_ref.py)
outside its ambiguous band and against the counts the reference's own float32 run gave (tests/golden/split_golden.npz)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import _roi_ref as RR
from tests._util import GOLDEN

pytestmark = pytest.mark.gpu

CANARY = 0x5A


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "split_golden.npz"))


def _cameras(gold):
    from neuralrecon_w_amd.views import Camera

    return [Camera(gold["K"][v], gold["c2w"][v], int(gold["wh"][v, 0]), int(gold["wh"][v, 1]), 0.0, 1.0) for v in range(len(gold["wh"]))]


def _launch(cams, origin, radius, with_mask=True, pad=64):
    """One direct call with count and mask inside larger buffers filled with canary bytes.  Returns (code, counts int64 [n],
    mask uint8 [P] or None, canaries_intact)."""
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import sceneprep

    n = len(cams)
    prefix = sceneprep.pixel_prefix(cams)
    P = int(prefix[-1])
    table = (L.NcwViewCamera * n)(*[c.struct() for c in cams])
    cams_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    prefix_d = torch.from_numpy(prefix).cuda()
    cbuf = torch.full((4 * n + 2 * pad,), CANARY, dtype=torch.uint8, device="cuda")
    mbuf = torch.full((P + 2 * pad,), CANARY, dtype=torch.uint8, device="cuda")
    count, mask = cbuf[pad:pad + 4 * n], mbuf[pad:pad + P]
    code = L.get_lib().ncw_views_roi(L.ptr(cams_d), L.ptr(prefix_d), n, (C.c_float * 3)(*[float(v) for v in origin]), float(radius),
                                     C.c_void_p(count.data_ptr()), C.c_void_p(mask.data_ptr() if with_mask else 0), L.stream_ptr())
    torch.cuda.synchronize()
    intact = bool((cbuf[:pad] == CANARY).all() and (cbuf[-pad:] == CANARY).all() and (mbuf[:pad] == CANARY).all()
                  and (mbuf[-pad:] == CANARY).all())
    if not with_mask:
        intact = intact and bool((mbuf == CANARY).all())
    counts = count.cpu().numpy().view(np.uint32).astype(np.int64)
    return code, counts, (mask.cpu().numpy() if with_mask else None), intact


@pytest.fixture(scope="module")
def nine(gold):
    """The nine views in one launch with a mask: shared by the tests below and left unchanged."""
    code, counts, mask, intact = _launch(_cameras(gold), gold["origin"], float(gold["radius"]))
    assert code == 0
    return counts, mask, intact


def test_nine_views_one_launch(gold, nine):
    """Every pixel outside the band equals the float64 predicate; count[v] == mask[v].sum() exactly; against the reference's
    float32 counts |count - golden| is at most the view's band count (only a pixel in the band may round the other way)."""
    counts, mask, intact = nine
    prefix = gold["prefix"]
    assert intact and set(np.unique(mask)) <= {0, 1}
    out = gold["band"] == 0
    n_diff = int((mask[out] != gold["roi64"][out]).sum())
    in_band = int((mask[~out] != gold["roi64"][~out]).sum())
    print("pixels outside the band that differ from float64: %d of %d; inside the band: %d of %d" % (n_diff, int(out.sum()), in_band, int((~out).sum())))
    assert n_diff == 0
    for v in range(len(counts)):
        m = mask[int(prefix[v]):int(prefix[v + 1])]
        print("%-10s count %5d  float32 reference %5d  float64 %5d  band %d" % (gold["names"][v], counts[v], gold["ref_count"][v], gold["count64"][v], gold["band_count"][v]))
        assert counts[v] == int(m.sum())
        assert abs(int(counts[v]) - int(gold["ref_count"][v])) <= int(gold["band_count"][v])
        assert abs(int(counts[v]) - int(gold["count64"][v])) <= int(gold["band_count"][v])


def test_counts_without_a_mask_and_a_second_launch(gold, nine):
    counts, mask, _ = nine
    cams = _cameras(gold)
    code, c2, m2, intact = _launch(cams, gold["origin"], float(gold["radius"]), with_mask=False)
    assert code == 0 and intact and m2 is None and np.array_equal(c2, counts)  # the mask buffer was not touched at all
    code, c3, m3, intact = _launch(cams, gold["origin"], float(gold["radius"]))
    assert code == 0 and intact and np.array_equal(c3, counts) and np.array_equal(m3, mask)  # bitwise the first launch


def test_permuted_view_order(gold, nine):
    counts, mask, _ = nine
    cams = _cameras(gold)
    prefix = gold["prefix"]
    order = [7, 5, 0, 6, 8, 2, 1, 4, 3]  # `big` first, `row` and `col` apart, other views meeting inside a wave
    code, c2, m2, intact = _launch([cams[i] for i in order], gold["origin"], float(gold["radius"]))
    assert code == 0 and intact and np.array_equal(c2, counts[order])
    assert np.array_equal(m2, np.concatenate([mask[int(prefix[i]):int(prefix[i + 1])] for i in order]))


@pytest.mark.parametrize("v", range(9))
def test_each_view_alone(gold, nine, v):
    counts, mask, _ = nine
    prefix = gold["prefix"]
    code, c1, m1, intact = _launch([_cameras(gold)[v]], gold["origin"], float(gold["radius"]))
    assert code == 0 and intact and c1.tolist() == [counts[v]] and np.array_equal(m1, mask[int(prefix[v]):int(prefix[v + 1])])


def test_many_tiles_per_workgroup():
    """More pixels than the launch has workgroups x 1024: every workgroup walks a RUN of tiles and carries its view across them
    (two views of 1201 x 901 around a one-row view and a 97 x 53 view, so runs start inside, at and across view borders)."""
    from neuralrecon_w_amd import sceneprep
    from neuralrecon_w_amd.views import Camera

    origin, radius = np.array([0.1, -0.1, 0.2]), 1.2

    def cam(pos, target, w, h, f):
        pos, target = np.array(pos, dtype=np.float64), np.array(target, dtype=np.float64)
        z = (target - pos) / np.linalg.norm(target - pos)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        c2w = np.stack([x, -np.cross(z, x), -z, pos], 1)
        return Camera([[f * w, 0, w / 2], [0, f * w, h / 2], [0, 0, 1]], c2w, w, h, 0.0, 1.0)

    cams = [cam((3.0, 0.5, 1.1), origin + [0.4, 0.9, 0.0], 1201, 901, 0.8), cam((0.2, 3.3, -0.8), origin, 777, 1, 1.0),
            cam((-2.4, -2.0, 1.5), origin + [0.0, 0.0, 0.9], 1201, 901, 0.6), cam((2.6, -1.9, 0.4), origin, 97, 53, 1.1)]
    prefix = sceneprep.pixel_prefix(cams)
    assert int(prefix[-1]) > 2048 * 1024
    code, counts, mask, intact = _launch(cams, origin, radius)
    assert code == 0 and intact
    for v, c in enumerate(cams):
        f = RR.roi_f64(c.K, c.c2w, c.width, c.height, origin, radius)
        m = mask[int(prefix[v]):int(prefix[v + 1])]
        out = ~f["band"]
        assert float(f["band"].mean()) <= 0.01 and 0.05 < float(f["roi"].mean()) < 0.95
        assert np.array_equal(m[out] != 0, f["roi"][out]) and counts[v] == int(m.sum())


def test_more_views_in_a_run_than_lds_slots():
    """40 views of 5 x 7 pixels and one of 3 x 3: the first workgroup's run of 1024 pixels touches 30 views, more than the 8 it
    sums in LDS, so the later ones take the per-wave global add; every wave meets several views in one step."""
    from neuralrecon_w_amd import sceneprep
    from neuralrecon_w_amd.views import Camera

    origin, radius = np.array([0.1, -0.1, 0.2]), 1.2
    rs = np.random.RandomState(5)
    cams = []
    for k in range(41):
        u = rs.normal(size=3)
        pos = origin + u / np.linalg.norm(u) * radius * rs.uniform(1.3, 3.0)
        target = origin + rs.uniform(-1.2, 1.2, 3) * radius
        z = (target - pos) / np.linalg.norm(target - pos)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        w, h = (3, 3) if k == 17 else (5, 7)
        cams.append(Camera([[0.8 * w, 0, w / 2], [0, 0.8 * w, h / 2], [0, 0, 1]], np.stack([x, -np.cross(z, x), -z, pos], 1), w, h, 0.0, 1.0))
    prefix = sceneprep.pixel_prefix(cams)
    assert 1024 < int(prefix[-1]) < 2048 and int(np.searchsorted(prefix, 1024)) > 8 + 8
    code, counts, mask, intact = _launch(cams, origin, radius)
    assert code == 0 and intact
    n_roi = 0
    for v, c in enumerate(cams):
        f = RR.roi_f64(c.K, c.c2w, c.width, c.height, origin, radius)
        m = mask[int(prefix[v]):int(prefix[v + 1])]
        out = ~f["band"]
        assert np.array_equal(m[out] != 0, f["roi"][out]) and counts[v] == int(m.sum()), v
        n_roi += int(f["roi"].sum())
    assert 0.2 * int(prefix[-1]) < n_roi < 0.9 * int(prefix[-1])  # the counts are not trivially all or nothing
    code, c2, _, intact = _launch(cams, origin, radius, with_mask=False)
    assert code == 0 and intact and np.array_equal(c2, counts)


def test_bad_arguments_launch_nothing(gold):
    """NULL cams / pix_start / origin / count, n_views < 1 and radius <= 0 (or NaN) return NCW_E_BADARG; count keeps its canary
    bytes (the entry point clears count before the launch, so an untouched count shows that nothing was enqueued)."""
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import sceneprep

    cams = _cameras(gold)
    n = len(cams)
    table = (L.NcwViewCamera * n)(*[c.struct() for c in cams])
    cams_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    prefix_d = torch.from_numpy(sceneprep.pixel_prefix(cams)).cuda()
    count = torch.full((4 * n,), CANARY, dtype=torch.uint8, device="cuda")
    org = (C.c_float * 3)(*[float(v) for v in gold["origin"]])
    null = C.c_void_p(0)
    ok = dict(cams=L.ptr(cams_d), prefix=L.ptr(prefix_d), n=n, origin=org, radius=1.2, count=L.ptr(count))
    bad = [dict(cams=null), dict(prefix=null), dict(origin=None), dict(count=null), dict(n=0), dict(n=-3), dict(radius=0.0),
           dict(radius=-1.0), dict(radius=float("nan"))]
    for b in bad:
        a = dict(ok, **b)
        code = L.get_lib().ncw_views_roi(a["cams"], a["prefix"], a["n"], a["origin"], a["radius"], a["count"], null, L.stream_ptr())
        assert code == -1, b
    torch.cuda.synchronize()
    assert bool((count == CANARY).all())


def test_roi_shares_binding(gold, nine):
    from neuralrecon_w_amd import sceneprep

    counts, mask, _ = nine
    cams = sceneprep.scene_cameras(os.path.join(GOLDEN, "split_scene"))
    shares, c2 = sceneprep.roi_shares(cams, gold["origin"], float(gold["radius"]))
    npix = np.diff(gold["prefix"])
    assert shares.dtype == np.float64 and c2.dtype == np.int64 and np.array_equal(c2, counts)
    assert np.array_equal(shares, counts.astype(np.float64) / npix.astype(np.float64))
    s3, c3, m3 = sceneprep.roi_shares(cams, gold["origin"], float(gold["radius"]), with_mask=True)
    assert np.array_equal(c3, counts) and m3.is_cuda and np.array_equal(m3.cpu().numpy(), mask)
