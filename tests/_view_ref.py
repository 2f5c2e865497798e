"""Float64 (or any dtype) torch restatement of what neuralrecon_w_amd.views and csrc/ncw_view.hip compute -- the yardstick of
tests/test_view_host.py and the tests/test_gpu_view_*.py files.  Each function cites the reference lines it restates;
tests/golden/view_golden.npz (tests/golden/make_golden_view.py: the reference's own datasets/ray_utils.py, metrics.py and
datasets/phototourism.py, executed) pins the restatement itself.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch
import torch.nn.functional as F


def ray_directions(H, W, K, dtype=torch.float64):
    """datasets/ray_utils.py:18-24: integer pixel coordinates (no + 0.5); dir = ((i - cx) / fx, -(j - cy) / fy, -1)."""
    K = torch.as_tensor(np.asarray(K), dtype=dtype)
    j, i = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    return torch.stack([(i - cx) / fx, -(j - cy) / fy, -torch.ones_like(i)], -1)


def rays_of(directions, c2w, dtype=torch.float64):
    """datasets/ray_utils.py:44-52: d = directions @ c2w[:, :3]^T normalised, o = c2w[:, 3]; both [H * W, 3]."""
    c2w = torch.as_tensor(np.asarray(c2w), dtype=dtype)
    d = directions.to(dtype) @ c2w[:, :3].T
    d = d / torch.norm(d, dim=-1, keepdim=True)
    o = c2w[:, 3].expand(d.shape)
    return o.reshape(-1, 3), d.reshape(-1, 3)


def view_rays(K, c2w, W, H, near, far, dtype=torch.float64):
    """datasets/phototourism.py:769-782: [H * W, 8] = o, d, near, far.  K and c2w are taken as float32 values (the dataset's
    `np.float32` K and `torch.FloatTensor(pose)`), the arithmetic runs in `dtype`."""
    K = np.asarray(K, dtype=np.float32)
    c2w = np.asarray(c2w, dtype=np.float32)
    o, d = rays_of(ray_directions(H, W, K, dtype), c2w, dtype)
    one = torch.ones_like(o[:, :1])
    return torch.cat([o, d, float(np.float32(near)) * one, float(np.float32(far)) * one], 1)


def mse(pred, gt, valid_mask=None):
    """metrics.py:5-11, reduction 'mean', in float64."""
    v = (pred.double() - gt.double()) ** 2
    if valid_mask is not None:
        v = v[valid_mask]
    return torch.mean(v)


def psnr(pred, gt, valid_mask=None):
    """metrics.py:13-14."""
    return -10 * torch.log10(mse(pred, gt, valid_mask))


def gaussian_window(w, sigma=1.5, dtype=torch.float64):
    """kornia's get_gaussian_kernel1d: exp(-(i - w // 2)^2 / (2 sigma^2)), normalised."""
    x = torch.arange(w, dtype=dtype) - w // 2
    g = torch.exp(-x ** 2 / (2 * sigma ** 2))
    return g / g.sum()


def ssim(pred, gt, window=3, dtype=torch.float64):
    """metrics.py:16-21 over kornia's ssim(pred, gt, window, 'mean') (kornia/losses/ssim.py: filter2D with the 2-D Gaussian,
    border 'reflect'; C1 = 0.01^2, C2 = 0.03^2; loss = clamp((1 - map) / 2, 0, 1)): returns 1 - 2 mean(loss).  pred / gt
    [C, H, W]; every operation in `dtype` (float32 = the reference's own arithmetic, float64 = the oracle)."""
    x, y = pred.to(dtype)[None], gt.to(dtype)[None]
    ch = x.shape[1]
    g = gaussian_window(window, 1.5, dtype)
    k2 = (g[:, None] * g[None, :])[None, None].expand(ch, 1, window, window)
    p = (window - 1) // 2

    def filt(t):
        return F.conv2d(F.pad(t, (p, p, p, p), mode="reflect"), k2, groups=ch)

    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = filt(x), filt(y)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = filt(x * x) - mu1_sq, filt(y * y) - mu2_sq, filt(x * y) - mu12
    m = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    loss = torch.clamp((1 - m) / 2, 0, 1)
    return 1 - 2 * loss.mean()


def depth_index(depth):
    """utils/visualization.py:17-22 in numpy float32, as the reference runs it: nan_to_num, global min / max,
    (x - mi) / (ma - mi + 1e-8), (255 x).astype(uint8).  The 1e-8 is added in float32 (what numpy >= 2 does with a float32 scalar
    and a Python float); a NaN left by inf / inf (an image holding +inf AND -inf) maps to 0, which is what the conversion gives
    on x86."""
    x = np.nan_to_num(np.asarray(depth, dtype=np.float32))
    mi, ma = np.min(x), np.max(x)
    with np.errstate(over="ignore", invalid="ignore"):
        den = np.float32(np.float32(ma - mi) + np.float32(1e-8))
        x = ((x - mi) / den).astype(np.float32)
        v = np.float32(255) * x
    return np.where(np.isnan(v), np.float32(0), v).astype(np.uint8)


def normal_plane(normals, H, W):
    """neuconw_system.py:459-460: n / |n| / 2 + 0.5 as [3, H, W] (float64)."""
    n = normals.double().reshape(H, W, 3)
    n = n / torch.linalg.norm(n, dim=-1)[:, :, None]
    return (n / 2 + 0.5).permute(2, 0, 1)


def scene_item(cam_params, qvec, tvec, xyz, downscale, scene_origin=None, scene_radius=None):
    """datasets/phototourism.py:363-375, 398-408, 426-444 for one image: (K float32 [3,3], c2w float64 [3,4], near, far)."""
    p = np.asarray(cam_params, dtype=np.float64)
    img_w, img_h = int(p[2] * 2), int(p[3] * 2)
    w_, h_ = img_w // downscale, img_h // downscale
    K = np.zeros((3, 3), dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[2, 2] = p[0] * w_ / img_w, p[1] * h_ / img_h, p[2] * w_ / img_w, p[3] * h_ / img_h, 1
    w, x, y, z = [float(v) for v in qvec]
    R = np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                  [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                  [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = R, np.asarray(tvec, dtype=np.float64)
    c2w = np.linalg.inv(w2c)[:3]
    c2w[..., 1:3] *= -1
    if scene_origin is not None:
        oz = (np.concatenate([np.asarray(scene_origin, dtype=np.float64), np.ones(1)])[None] @ w2c.T)[0, 2]
        return K, c2w, oz - scene_radius * 1.5, oz + scene_radius * 1.5
    zc = (np.concatenate([np.asarray(xyz, dtype=np.float64), np.ones((len(xyz), 1))], -1) @ w2c.T)[:, 2]
    zc = zc[zc > 0]
    return K, c2w, np.percentile(zc, 0.1), np.percentile(zc, 99.9)
