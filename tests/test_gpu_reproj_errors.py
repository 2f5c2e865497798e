"""GPU: `ncw_reproj_errors` (csrc/ncw_gtreproj.hip) called directly: err against float64 with the bound of tests/_ray_cases.py
(4 x the float32 restatement's own error) and bit for bit against that restatement; seg_sum against the float64 sum of the
kernel's own err, in the kernel's fixed order bit for bit, and the same on a second launch; refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _gtreproj_ref as GR

pytestmark = pytest.mark.gpu

CANARY = 0x5A
PAD = 64
SEGMENTS = [0, 1, 63, 64, 65, 1000, 0, 129, 2]  # lengths; one wave per segment, four segments per workgroup


def _case(seed=4):
    rs = np.random.RandomState(seed)
    n_cams, n_pts = 7, 301
    proj = np.zeros((n_cams, 3, 4))
    for c in range(n_cams):
        u = rs.normal(size=3)
        pos = u / np.linalg.norm(u) * rs.uniform(3.0, 4.0) + [40.0, -25.0, 10.0]
        z = [40.0, -25.0, 10.0] + rs.uniform(-0.2, 0.2, 3) - pos
        z /= np.linalg.norm(z)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        K = np.array([[900.0, 0, 512.3], [0, 910.0, 383.6], [0, 0, 1]])
        proj[c] = K @ np.concatenate([R, (-R @ pos)[:, None]], 1)
    xyz = (rs.uniform(-1, 1, size=(n_pts, 3)) + [40.0, -25.0, 10.0]).astype(np.float32)
    seg = np.concatenate([[0], np.cumsum(SEGMENTS)]).astype(np.int64)
    n = int(seg[-1])
    cam_idx = rs.randint(0, n_cams, n).astype(np.int32)
    pt_idx = rs.randint(0, n_pts, n).astype(np.int32)
    proj = proj.astype(np.float32)
    h = np.einsum("nij,nj->ni", proj[cam_idx][:, :, :3].astype(np.float64), xyz[pt_idx].astype(np.float64)) + proj[cam_idx][:, :, 3]
    xy = (h[:, :2] / h[:, 2:3] + rs.normal(0, 1.5, (n, 2))).astype(np.float32)  # key-points a pixel or two off the projection
    return proj, xyz, cam_idx, pt_idx, xy, seg


def _launch(proj, xyz, cam_idx, pt_idx, xy, seg, null=(), **over):
    from neuralrecon_w_amd import lib as L

    n_obs, n_seg = len(cam_idx), len(seg) - 1
    d = {"proj": torch.from_numpy(proj).cuda(), "xyz": torch.from_numpy(xyz).cuda(), "cam_idx": torch.from_numpy(cam_idx).cuda(),
         "pt_idx": torch.from_numpy(pt_idx).cuda(), "xy": torch.from_numpy(xy).cuda(), "seg": torch.from_numpy(seg).cuda()}
    ebuf = torch.full((4 * n_obs + 2 * PAD,), CANARY, dtype=torch.uint8, device="cuda")
    sbuf = torch.full((8 * n_seg + 2 * PAD,), CANARY, dtype=torch.uint8, device="cuda")
    p = {k: v.data_ptr() for k, v in d.items()}
    p.update(err=ebuf.data_ptr() + PAD, seg_sum=sbuf.data_ptr() + PAD)
    for k in null:
        p[k] = 0
    a = dict(n_cams=len(proj), n_pts=len(xyz), n_obs=n_obs, n_seg=n_seg)
    a.update(over)
    code = L.get_lib().ncw_reproj_errors(C.c_void_p(p["proj"]), a["n_cams"], C.c_void_p(p["xyz"]), a["n_pts"], C.c_void_p(p["cam_idx"]),
                                         C.c_void_p(p["pt_idx"]), C.c_void_p(p["xy"]), a["n_obs"], C.c_void_p(p["seg"]), a["n_seg"],
                                         C.c_void_p(p["err"]), C.c_void_p(p["seg_sum"]), L.stream_ptr())
    torch.cuda.synchronize()
    intact = bool((ebuf[:PAD] == CANARY).all() and (ebuf[-PAD:] == CANARY).all() and (sbuf[:PAD] == CANARY).all() and (sbuf[-PAD:] == CANARY).all())
    err = ebuf[PAD:PAD + 4 * n_obs].cpu().numpy().view(np.float32).copy()
    seg_sum = sbuf[PAD:PAD + 8 * n_seg].cpu().numpy().view(np.float64).copy()
    return code, err, seg_sum, intact


@pytest.fixture(scope="module")
def case():
    return _case()


@pytest.fixture(scope="module")
def result(case):
    code, err, seg_sum, intact = _launch(*case)
    assert code == 0
    return err, seg_sum, intact


def test_err_against_float64_and_the_restatement(case, result):
    err, _, intact = result
    assert intact
    e64 = GR.reproj_errors_f64(*case[:5])
    e32 = GR.reproj_errors_f32(*case[:5])
    assert 0.5 < e64.mean() < 5  # a pixel or two
    scale = np.abs(e64).max()
    err32 = np.abs(e32.astype(np.float64) - e64).max() / scale   # the float32 restatement's own error
    got = np.abs(err.astype(np.float64) - e64).max() / scale
    print("reproj err: kernel %.3e, float32 restatement %.3e (relative to max |err| = %.3f px)" % (got, err32, scale))
    assert err32 > 0 and got <= 4 * err32
    assert np.array_equal(err.view(np.uint32), e32.view(np.uint32))  # bit for bit: IEEE products, sums, division and square root


def test_seg_sum_fixed_order(case, result):
    err, seg_sum, intact = result
    seg = case[5]
    assert intact
    want = GR.seg_sums_f64(err, seg)
    assert seg_sum[0] == 0.0 and seg_sum[6] == 0.0  # empty segments
    nz = want != 0
    assert (np.abs(seg_sum - want)[nz] <= 1e-12 * np.abs(want[nz])).all()
    assert np.array_equal(seg_sum, GR.seg_sums_wave(err, seg))  # the kernel's order, bit for bit
    code, err2, seg_sum2, intact2 = _launch(*case)
    assert code == 0 and intact2
    assert np.array_equal(err2.view(np.uint32), err.view(np.uint32)) and np.array_equal(seg_sum2.view(np.uint64), seg_sum.view(np.uint64))


def test_index_outside_its_table_reads_nothing(case):
    proj, xyz, cam_idx, pt_idx, xy, seg = case
    cam_idx, pt_idx = cam_idx.copy(), pt_idx.copy()
    a, b = int(seg[5]) + 3, int(seg[5]) + 70  # two observations of the long segment
    cam_idx[a], pt_idx[b] = len(proj), -1
    code, err, seg_sum, intact = _launch(proj, xyz, cam_idx, pt_idx, xy, seg)
    assert code == 0 and intact
    assert np.isnan(err[a]) and np.isnan(err[b]) and np.isnan(err).sum() == 2 and np.isnan(seg_sum[5]) and np.isnan(seg_sum).sum() == 1


def test_refusals(case):
    untouched_e = np.frombuffer(bytes([CANARY]) * (4 * len(case[2])), dtype=np.float32)
    untouched_s = np.frombuffer(bytes([CANARY]) * (8 * (len(case[5]) - 1)), dtype=np.float64)
    bad = [dict(null=(k,)) for k in ("proj", "xyz", "cam_idx", "pt_idx", "xy", "seg", "err", "seg_sum")]
    bad += [dict(n_cams=0), dict(n_pts=0), dict(n_obs=-1), dict(n_seg=-1)]
    for kw in bad:
        code, err, seg_sum, intact = _launch(*case, **kw)
        assert code == -1, kw  # NCW_E_BADARG
        assert intact and np.array_equal(err.view(np.uint32), untouched_e.view(np.uint32)), kw
        assert np.array_equal(seg_sum.view(np.uint64), untouched_s.view(np.uint64)), kw
    code, err, seg_sum, intact = _launch(*case, n_seg=0)  # nothing to do: no launch
    assert code == 0 and intact and np.array_equal(err.view(np.uint32), untouched_e.view(np.uint32))
