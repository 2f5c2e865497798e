"""GPU: the image metrics and the depth colour map of csrc/ncw_view.hip -- `ncw_image_sqerr` (metrics.py:5-14),
`ncw_image_ssim` (metrics.py:16-21 over kornia's ssim), `ncw_image_minmax` + `ncw_depth_colormap`
(utils/visualization.py:13-25) -- against the float64 restatements of tests/_view_ref.py.

The figures measured on an MI355X are in the docstrings of the squared-error and SSIM tests; the tests print them (-s)."""
import numpy as np
import pytest
import torch

from tests import _view_ref as VR

pytestmark = pytest.mark.gpu

_CACHE = {}


def _pair(n, seed=0):
    if ("pair", n, seed) not in _CACHE:
        g = torch.Generator().manual_seed(seed + n)
        pred, gt = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
        mask = torch.rand(n, generator=g) < 0.6
        _CACHE[("pair", n, seed)] = (pred, gt, mask)
    return _CACHE[("pair", n, seed)]


# ---------------------------------------------------------------------------------------------------
# squared error / PSNR
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64 * 256 + 1])
@pytest.mark.parametrize("masked", [False, True])
def test_sqerr_sum_count_and_psnr(n, masked):
    """Sum within 2e-6 relative of the float64 sum (a pairwise tree over <= 2^20 terms gives (log2 n + 2) 2^-24 ~ 1.3e-6; the
    squares themselves add 1.2e-7), the count exact, PSNR = -10 log10(sum / count), and two runs bitwise equal (fixed-order
    two-stage reduction, no float atomics).  64 * 256 + 1 pixels: more than one workgroup and a ragged last one.
    Measured on an MI355X: relative error of the sum 1.4e-9 .. 4.6e-8 over the six cases."""
    from neuralrecon_w_amd import views

    pred, gt, mask = _pair(n)
    m = mask if masked else None
    s, cnt = views.sqerr(pred.cuda(), gt.cuda(), None if m is None else m.cuda())
    s2, cnt2 = views.sqerr(pred.cuda(), gt.cuda(), None if m is None else m.cuda())
    assert torch.equal(s, s2) and torch.equal(cnt, cnt2)
    sel = slice(None) if m is None else m
    ref = float(((pred.double() - gt.double()) ** 2)[sel].sum())
    want_cnt = 3 * (n if m is None else int(m.sum()))
    assert int(cnt) == want_cnt
    if want_cnt == 0:  # a single pixel that the mask drops
        assert float(s) == 0.0
        return
    err = abs(float(s) - ref) / ref
    print("sqerr n=%d masked=%s: rel err %.3g" % (n, masked, err))
    assert err <= 2e-6
    m3 = None if m is None else m[:, None].expand(-1, 3)
    p = float(views.psnr(pred.cuda(), gt.cuda(), None if m is None else m.cuda()))
    assert abs(p - float(VR.psnr(pred, gt, m3))) <= 1e-4  # 10 / ln 10 * 2e-6 relative on the mse + the float32 log10
    # the planar [3, H, W] layout of render_view's planes sums the same elements
    if n == 63:
        sp, cp = views.sqerr(pred.T.reshape(3, 7, 9).contiguous().cuda(), gt.T.reshape(3, 7, 9).contiguous().cuda(),
                             None if m is None else m.reshape(7, 9).cuda())
        assert int(cp) == want_cnt and abs(float(sp) - ref) / ref <= 2e-6


def test_sqerr_with_an_empty_mask_counts_nothing():
    from neuralrecon_w_amd import views

    pred, gt, _ = _pair(63)
    s, cnt = views.sqerr(pred.cuda(), gt.cuda(), torch.zeros(63, dtype=torch.bool).cuda())
    assert int(cnt) == 0 and float(s) == 0.0
    assert torch.isnan(views.mse(pred.cuda(), gt.cuda(), torch.zeros(63, dtype=torch.bool).cuda()))  # torch.mean of nothing


# ---------------------------------------------------------------------------------------------------
# SSIM
# ---------------------------------------------------------------------------------------------------
SSIM_SHAPES = [(2, 3, 3), (6, 6, 11), (33, 65, 3), (33, 65, 11), (17, 130, 3), (17, 130, 11)]


def _ssim_inputs(h, w, kind):
    g = torch.Generator().manual_seed(1000 * h + w)
    x = torch.rand(3, h, w, generator=g)
    if kind == "identical":
        return x, x.clone()
    if kind == "offset":
        return x * 0.8, x * 0.8 + 0.1
    if kind == "noise":
        return x, (x + 0.2 * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    # half-flat: one half of both images is constant (different constants): sigma^2 = E[x^2] - mu^2 cancels there
    y = torch.rand(3, h, w, generator=g)
    x, y = x.clone(), y.clone()
    x[:, :, : w // 2] = 0.7
    y[:, :, : w // 2] = 0.3
    return x, y


def _ssim_ref(h, w, win, kind):
    key = ("ssim", h, w, win, kind)
    if key not in _CACHE:
        x, y = _ssim_inputs(h, w, kind)
        r64 = float(VR.ssim(x, y, win, torch.float64))
        r32 = float(VR.ssim(x, y, win, torch.float32))
        _CACHE[key] = (x, y, r64, abs(r32 - r64))
    return _CACHE[key]


@pytest.mark.parametrize("h,w,win", SSIM_SHAPES)
@pytest.mark.parametrize("kind", ["identical", "offset", "noise", "halfflat"])
def test_ssim_matches_the_float64_oracle(h, w, win, kind):
    """The bound is the reference's own arithmetic: the same formula evaluated in float32 torch on the CPU deviates from the
    float64 oracle by `dev32`; the kernel is allowed 2 dev32 + 1e-6.  Identical images give exactly 1.  Image sizes cross
    both tile borders (32 x 32 output tiles) and include the smallest sides reflect padding allows.
    Measured on an MI355X (kernel deviation / float32-torch deviation): identical 0 / 0; offset and noise 1.8e-10 .. 1.5e-7 /
    1.3e-9 .. 1.2e-7; half-flat, where sigma^2 = E[x^2] - mu^2 cancels on the flat half, 7.7e-9 .. 1.3e-8 / 1.7e-5 at window 3
    and 1.8e-5 .. 1.9e-5 / 4.4e-5 .. 4.9e-5 at window 11 on the two large images (2.1e-7 / 1.4e-6 and 1.9e-7 / 2.3e-7 on the
    6 x 6 and 2 x 3 ones): the largest kernel deviation is 1.9e-5, under the float32 reference arithmetic's own 4.9e-5."""
    from neuralrecon_w_amd import views

    x, y, r64, dev32 = _ssim_ref(h, w, win, kind)
    got = float(views.ssim(x.cuda(), y.cuda(), win))
    dev = abs(got - r64)
    print("ssim %dx%d w=%d %s: oracle %.9f kernel dev %.3g float32-torch dev %.3g" % (h, w, win, kind, r64, dev, dev32))
    if kind == "identical":
        assert got == 1.0
    assert dev <= 2 * dev32 + 1e-6
    assert got == float(views.ssim(x.cuda(), y.cuda(), win))  # fixed-order reduction


def test_ssim_refuses_undersized_images_and_bad_windows():
    import ctypes as C

    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import views

    lib = L.get_lib()
    x = torch.rand(3, 5, 40).cuda()
    scratch, out = torch.empty(64, device="cuda"), torch.empty(1, device="cuda")
    st = L.stream_ptr(x.device)
    assert lib.ncw_image_ssim(L.ptr(x), L.ptr(x), 3, 5, 40, 11, L.ptr(scratch), L.ptr(out), st) == -2  # 5 <= (11 - 1) / 2
    assert lib.ncw_image_ssim(L.ptr(x), L.ptr(x), 3, 40, 1, 3, L.ptr(scratch), L.ptr(out), st) == -2
    assert lib.ncw_image_ssim(L.ptr(x), L.ptr(x), 3, 5, 40, 4, L.ptr(scratch), L.ptr(out), st) == -1
    assert lib.ncw_image_ssim(L.ptr(x), L.ptr(x), 3, 5, 40, 13, L.ptr(scratch), L.ptr(out), st) == -1
    assert lib.ncw_image_ssim(L.ptr(x), L.ptr(x), 3, 5, 40, 9, L.ptr(scratch), L.ptr(out), st) == 0   # 5 > 4
    with pytest.raises(ValueError):
        views.ssim(x, x, 11)
    assert C.sizeof(C.c_float) * int(lib.ncw_image_ssim_scratch_floats(3, 33, 65)) == 4 * 3 * 2 * 3


# ---------------------------------------------------------------------------------------------------
# depth colour map
# ---------------------------------------------------------------------------------------------------
def _depth_cases():
    g = np.random.RandomState(4)
    ramp = np.linspace(0.37, 5.21, 23 * 37, dtype=np.float32).reshape(23, 37)
    const = np.full((5, 9), 1.75, dtype=np.float32)
    mi, ma = np.float32(0.5), np.float32(3.0)
    edges = (np.arange(256, dtype=np.float32) / np.float32(255) * (ma - mi) + mi).astype(np.float32)
    edges = np.concatenate([edges, np.nextafter(edges, np.float32(-10)), np.nextafter(edges, np.float32(10))]).clip(mi, ma)
    edges = np.concatenate([edges, [mi, ma]]).astype(np.float32).reshape(11, 70)
    nasty = g.uniform(0.1, 9.0, size=(40, 33)).astype(np.float32)
    nasty[3, 4] = np.nan
    nasty[7, 1] = np.inf
    both = nasty.copy()
    both[9, 9] = -np.inf
    neg = nasty.copy()
    neg[7, 1] = -np.inf
    big = g.uniform(0, 1, size=(300, 400)).astype(np.float32)  # more than one first-stage workgroup per 256 * 1024 / ... pixels
    return {"ramp": ramp, "constant": const, "bin_edges": edges, "nan_posinf": nasty, "nan_neginf": neg, "nan_both_inf": both,
            "large": big}


@pytest.mark.parametrize("name", ["ramp", "constant", "bin_edges", "nan_posinf", "nan_neginf", "nan_both_inf", "large"])
def test_depth_colormap_index_is_numpys(name):
    """The table index of every pixel is exactly what the reference's float32 numpy expression gives (true float32
    division), on a ramp, a constant image, values on and next to the bin edges k / 255 (ma - mi) + mi, and images with NaN
    and +-inf (nan_to_num: NaN -> 0, +-inf -> +-FLT_MAX); the colour plane is the table row / 255."""
    from neuralrecon_w_amd import views

    d = _depth_cases()[name]
    want = VR.depth_index(d)
    vis, idx = views.depth_colormap(torch.from_numpy(d).cuda(), with_index=True)
    idx = idx.cpu().numpy()
    assert idx.shape == d.shape and np.array_equal(idx, want), (name, int((idx != want).sum()))
    if name in ("ramp", "bin_edges", "large"):
        assert want.min() == 0 and want.max() >= 254 and len(np.unique(want)) > 200
    rgb = (views.JET[want].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)
    assert vis.shape == (3,) + d.shape and np.array_equal(vis.cpu().numpy(), rgb)
    # another table, passed by pointer
    lut = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256], -1).astype(np.uint8)
    vis2 = views.depth_colormap(torch.from_numpy(d).cuda(), lut=lut)
    assert np.array_equal(vis2.cpu().numpy(), (lut[want].astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
