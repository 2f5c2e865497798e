"""Whole camera views: colour, depth, normals, PSNR / SSIM -- the image half of the reference's validation step
(lightning_modules/neuconw_system.py:404-464, 533-546), on the device.

    cam, gt, image_id = scene_view(root_dir)                        # the `val` item of datasets/phototourism.py
    out = render_view(rdr, cam, ts=image_id, gt=gt.cuda())          # colour / depth / normal / depth_vis planes, psnr, ssim
    write_panel("val.png", gt, out["color"], out["depth_vis"], out["normal"])

The rays of a pixel chunk are generated on the device (`ncw_view_rays`), rendered by the forward-only render
(renderer.NeuconWRenderer under no_grad) and scattered into planar images (`ncw_view_store`); depth colour map and metrics are
`ncw_image_*` / `ncw_depth_colormap` launches (csrc/ncw_view.hip).  Nothing is copied to the host per chunk.

    out = trace_view(rdr, cam, ts=image_id, gt=gt.cuda())           # the SURFACE instead: sphere tracing (trace.py), colour / normal at the first hit
"""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import torch

from . import colmap
from . import lib as L

DEFAULT_CHUNK = 4096  # rays per render launch (scripts/bench_view.py measures 1024 / 4096 / 16384: profiles/view/README.md)


def _jet_table():
    """MATLAB's jet(256) in closed form as 8-bit RGB rows [256, 3] (utils/visualization.py:13: cv2.COLORMAP_JET, which cv2
    applies as BGR and the reference flips to RGB).  Parity with cv2's own table is unpinned (cv2 is not a dependency)."""
    i = np.arange(256, dtype=np.float64)
    tri = lambda a, b: np.clip(np.minimum((i + a) / 64.0, (b - i) / 64.0), 0.0, 1.0)  # noqa: E731
    rgb = np.stack([tri(-95, 287), tri(-31, 223), tri(33, 159)], -1)
    return np.floor(255.0 * rgb + 0.5).astype(np.uint8)


JET = _jet_table()


class Camera:
    """One pinhole view: K [3,3] (fx, fy, cx, cy), c2w [3,4] in the renderer's "right up back" camera axes
    (datasets/phototourism.py:406-408), image size, and the near / far every ray of the view carries."""

    def __init__(self, K, c2w, width, height, near, far):
        self.K = np.asarray(K, dtype=np.float32).reshape(3, 3)
        self.c2w = np.asarray(c2w, dtype=np.float32).reshape(3, 4)  # torch.FloatTensor(poses_dict[id]) (phototourism.py:755)
        self.width, self.height = int(width), int(height)
        self.near, self.far = float(near), float(far)
        if self.width < 1 or self.height < 1:
            raise ValueError("Camera: empty image %d x %d" % (self.width, self.height))

    def struct(self):
        K = self.K
        return L.NcwViewCamera(float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]),
                               (C.c_float * 12)(*[float(v) for v in self.c2w.reshape(-1)]), self.width, self.height,
                               self.near, self.far)


def view_rays(camera, p0=0, n=None, device="cuda", out=None):
    """Rays [n, 8] = o, d, near, far of the pixels [p0, p0 + n) (row-major) of the view: one `ncw_view_rays` launch."""
    n = camera.width * camera.height - p0 if n is None else int(n)
    rays = torch.empty(n, 8, device=device, dtype=torch.float32) if out is None else out
    if not (torch.is_tensor(rays) and rays.is_cuda):
        raise L.NeuconwHipError("views.view_rays: the ray buffer is not on a GPU; there is no CPU fallback")
    if rays.dtype != torch.float32 or tuple(rays.shape) != (n, 8) or not rays.is_contiguous():
        raise ValueError("view_rays: out must be a contiguous float32 [%d, 8] tensor, got %s %s"
                         % (n, rays.dtype, tuple(rays.shape)))
    L.check(L.get_lib().ncw_view_rays(C.byref(camera.struct()), int(p0), n, L.ptr(rays), L.stream_ptr(rays.device)),
            "ncw_view_rays")
    return rays


def _scratch(device):
    return torch.empty(int(L.get_lib().ncw_image_reduce_scratch_bytes()), device=device, dtype=torch.uint8)


def sqerr(pred, gt, valid_mask=None):
    """(sum of squared differences f32 [1], element count int64 [1]) as device tensors.  pred / gt: [N, 3] or planar
    [3, H, W]; valid_mask: per pixel ([N] / [H, W], bool or uint8) or None.  Fixed-order reduction: bitwise reproducible."""
    planar = pred.dim() == 3
    if planar:
        if pred.shape[0] != 3:
            raise ValueError("sqerr: a planar image is [3, H, W], got %s" % (tuple(pred.shape),))
        n = pred.shape[1] * pred.shape[2]
    else:
        if pred.dim() != 2 or pred.shape[1] != 3:
            raise ValueError("sqerr: images are [N, 3] or [3, H, W], got %s" % (tuple(pred.shape),))
        n = pred.shape[0]
    if tuple(gt.shape) != tuple(pred.shape):
        raise ValueError("sqerr: shapes differ: %s / %s" % (tuple(pred.shape), tuple(gt.shape)))
    if not pred.is_cuda:
        raise L.NeuconwHipError("views.sqerr: the images are not on a GPU; there is no CPU fallback")
    dev = pred.device
    pred, gt = pred.detach().contiguous().float(), gt.detach().to(dev).contiguous().float()
    m = None
    if valid_mask is not None:
        if valid_mask.numel() != n:
            raise ValueError("sqerr: valid_mask holds %d entries for %d pixels" % (valid_mask.numel(), n))
        m = valid_mask.to(dev).reshape(-1).ne(0).to(torch.uint8).contiguous()
    s = torch.empty(1, device=dev, dtype=torch.float32)
    cnt = torch.empty(1, device=dev, dtype=torch.int64)
    scratch = _scratch(dev)
    L.check(L.get_lib().ncw_image_sqerr(L.ptr(pred), L.ptr(gt), L.ptr(m), n, int(planar), L.ptr(scratch), L.ptr(s), L.ptr(cnt),
                                        L.stream_ptr(dev)), "ncw_image_sqerr")
    return s, cnt


def mse(pred, gt, valid_mask=None):
    """metrics.py:5-11 (reduction 'mean') as a device scalar; NaN when the mask selects nothing, as torch.mean of nothing."""
    s, cnt = sqerr(pred, gt, valid_mask)
    return (s / cnt.float()).reshape(())


def psnr(pred, gt, valid_mask=None):
    """metrics.py:13-14: -10 log10(mse) as a device scalar."""
    return -10.0 * torch.log10(mse(pred, gt, valid_mask))


def ssim(pred, gt, window=3):
    """metrics.py:16-21 (`1 - 2 dssim` of kornia's ssim loss, reduction 'mean') as a device scalar; pred / gt [3, H, W] or
    [1, 3, H, W].  window 3 is the reference's, 11 the common SSIM's."""
    if pred.dim() == 4 and pred.shape[0] == 1:
        pred, gt = pred[0], gt[0]
    if pred.dim() != 3 or tuple(gt.shape) != tuple(pred.shape):
        raise ValueError("ssim: images are [C, H, W] of one shape, got %s / %s" % (tuple(pred.shape), tuple(gt.shape)))
    if window not in (3, 5, 7, 9, 11):
        raise ValueError("ssim: window must be one of 3, 5, 7, 9, 11 (got %r)" % (window,))
    ch, h, w = pred.shape
    if min(h, w) <= (window - 1) // 2:
        raise ValueError("ssim: a %d x %d image is too small for window %d (reflect padding of %d needs larger sides)"
                         % (h, w, window, (window - 1) // 2))
    if not pred.is_cuda:
        raise L.NeuconwHipError("views.ssim: the images are not on a GPU; there is no CPU fallback")
    dev = pred.device
    pred, gt = pred.detach().contiguous().float(), gt.detach().to(dev).contiguous().float()
    lib = L.get_lib()
    scratch = torch.empty(int(lib.ncw_image_ssim_scratch_floats(ch, h, w)), device=dev, dtype=torch.float32)
    out = torch.empty(1, device=dev, dtype=torch.float32)
    L.check(lib.ncw_image_ssim(L.ptr(pred), L.ptr(gt), ch, h, w, int(window), L.ptr(scratch), L.ptr(out), L.stream_ptr(dev)),
            "ncw_image_ssim")
    return out.reshape(())


def _lut_tensor(lut, device):
    lut = np.ascontiguousarray(np.asarray(lut, dtype=np.uint8))
    if lut.shape != (256, 3):
        raise ValueError("depth_colormap: the look-up table is [256, 3] uint8 RGB, got %s" % (lut.shape,))
    return torch.from_numpy(lut).to(device)


def depth_colormap(depth, lut=JET, with_index=False):
    """utils/visualization.py:13-25 `visualize_depth`: [3, H, W] f32 in [0, 1] of a depth map [H, W] on the device (nan_to_num,
    global min / max, 255 (x - mi) / (ma - mi + 1e-8) truncated to the table index).  with_index: also the index plane uint8."""
    if not depth.is_cuda:
        raise L.NeuconwHipError("views.depth_colormap: the depth map is not on a GPU; there is no CPU fallback")
    dev = depth.device
    d = depth.detach().contiguous().float()
    n = d.numel()
    if n < 1:
        raise ValueError("depth_colormap: empty depth map")
    lib = L.get_lib()
    mm = torch.empty(2, device=dev, dtype=torch.float32)
    scratch = _scratch(dev)
    L.check(lib.ncw_image_minmax(L.ptr(d), n, L.ptr(scratch), L.ptr(mm), L.stream_ptr(dev)), "ncw_image_minmax")
    out = torch.empty((3,) + tuple(d.shape), device=dev, dtype=torch.float32)
    idx = torch.empty(d.shape, device=dev, dtype=torch.uint8) if with_index else None
    lut_t = lut if torch.is_tensor(lut) else _lut_tensor(lut, dev)
    L.check(lib.ncw_depth_colormap(L.ptr(d), n, L.ptr(mm), L.ptr(lut_t), L.ptr(out), None, L.ptr(idx), L.stream_ptr(dev)),
            "ncw_depth_colormap")
    return (out, idx) if with_index else out


def render_view(rdr, camera, ts, chunk=DEFAULT_CHUNK, gt=None, label=None, background_rgb=None, ssim_window=3, device=None,
                nerf_far_override=None, a_code=None):
    """Renders one whole view with the forward-only render, chunk by chunk, without leaving the device
    (neuconw_system.py:404-464): per chunk `ncw_view_rays` -> renderer (perturb_overwrite = 0, no_grad) -> `ncw_view_store`.
    ts: ONE appearance index for the view (the image id for `val`, 1123 in tools/extract_mesh.py:157); label: semantic labels
    [H * W] (default zeros).  Returns device tensors color [3,H,W], depth [H,W], normal [3,H,W] (n / |n| / 2 + 0.5),
    depth_vis [3,H,W]; with gt ([3,H,W] or [H*W,3]) also psnr, mse, ssim as device scalars.  nerf_far_override: near / far from
    the SfM octree for this view (neuconw_system.py:407 sets it from NEUCONW.NEAR_FAR_OVERRIDE); None = the renderer's attribute.
    a_code [n_a]: render with this appearance code instead of the embedding row `ts` (a held-out image's fitted code, appfit.py);
    None = the embedding row.  The renderer's attributes are not touched."""
    H, W = camera.height, camera.width
    hw = H * W
    chunk = max(1, min(int(chunk), hw))
    if device is None:
        device = next(rdr.neuconw.parameters()).device
    device = torch.device(device)
    if device.type != "cuda":
        raise L.NeuconwHipError("views.render_view: the renderer is not on a GPU; the hot path has no CPU fallback")
    lib = L.get_lib()
    cam = camera.struct()
    color = torch.empty(3, H, W, device=device, dtype=torch.float32)
    depth = torch.empty(H, W, device=device, dtype=torch.float32)
    normal = torch.empty(3, H, W, device=device, dtype=torch.float32)
    rays = torch.empty(chunk, 8, device=device, dtype=torch.float32)
    ts_all = torch.full((chunk,), int(ts), device=device, dtype=torch.int64)
    if label is None:
        label_all = torch.zeros(chunk, device=device, dtype=torch.int64)
    else:
        label_all = label.to(device).reshape(-1)
        if label_all.numel() != hw:
            raise ValueError("render_view: label holds %d entries for %d pixels" % (label_all.numel(), hw))
    with torch.no_grad():
        for p0 in range(0, hw, chunk):
            n = min(chunk, hw - p0)
            r = rays[:n]
            L.check(lib.ncw_view_rays(C.byref(cam), p0, n, L.ptr(r), L.stream_ptr(device)), "ncw_view_rays")
            lab = label_all[:n] if label is None else label_all[p0:p0 + n]
            # sfm_depth_loss=False: render() reads that entry's selection back to the host (renderer.py:892-897: a
            # data-dependent shape); a view does not use it
            kw = {} if a_code is None else {"a_code": a_code}
            out, nrm = rdr._render_with_normals(r, ts_all[:n], lab, perturb_overwrite=0, background_rgb=background_rgb,
                                                sfm_depth_loss=False, far_override=nerf_far_override, **kw)
            L.check(lib.ncw_view_store(L.ptr(out["color"].contiguous()), L.ptr(out["depth"].contiguous()),
                                       L.ptr(nrm.contiguous()), p0, n, hw, L.ptr(color), L.ptr(depth), L.ptr(normal),
                                       L.stream_ptr(device)), "ncw_view_store")
    res = {"color": color, "depth": depth, "normal": normal, "depth_vis": depth_colormap(depth)}
    if gt is not None:
        g = gt.to(device).float()
        if g.dim() == 2:  # [H * W, 3], the dataset's layout (phototourism.py:766)
            g = g.reshape(H, W, 3).permute(2, 0, 1)
        g = g.reshape(3, H, W).contiguous()
        s, cnt = sqerr(color, g)
        res["mse"] = (s / cnt.float()).reshape(())
        res["psnr"] = -10.0 * torch.log10(res["mse"])
        if min(H, W) > (ssim_window - 1) // 2:
            res["ssim"] = ssim(color, g, ssim_window)
        else:  # SSIM is undefined below the window's reflect padding
            res["ssim"] = torch.full((), float("nan"), device=device)
    return res


TRACE_CHUNK = 1 << 17  # rays per trace_rays call of trace_view (scripts/bench_trace.py measures the chunk size: profiles/trace/README.md)


def trace_view(rdr, camera, ts, *, chunk=TRACE_CHUNK, background_rgb=None, a_code=None, gt=None, shade=True, ssim_window=3,
               device=None, shade_prec=None, on_hits=None, **trace_kw):
    """The surface of one whole view by sphere tracing (trace.py; not in the reference): per chunk `ncw_view_rays` ->
    trace.trace_rays -> `NeuconW.forward([p, d, a])` over the rays that HIT (ascending ray index) -> `ncw_trace_store`.
    No background NeRF and no transmittance: a pixel shows the colour network's answer AT the first surface point, or
    background_rgb (3 values, default 0) where the ray found none.  ts / a_code: the appearance as in render_view.
    Returns device tensors color [3,H,W], depth [H,W] (t at a hit, render_view's units; 0 elsewhere), normal [3,H,W]
    (g / |g| / 2 + 0.5 at a hit, 0 elsewhere), state [H,W] uint8 (trace.HIT / MISS / INSIDE / STALLED), iters [H,W] int32,
    depth_vis [3,H,W] and `stats` (host numbers: pixels per state, mean / max iters, SDF launches and evaluated points, forward
    launches); with gt also mse / psnr / ssim over the image as render_view computes them and psnr_hit over the hit pixels.
    shade=False skips the forward (colour stays background, normal 0).  shade_prec: precision of the forward (None = the
    renderer's `infer_prec` or fp32, as NeuconWRenderer.rgb); trace_kw goes to trace_rays (eps, max_iter, step, far_override,
    sdf_fn, sync_every, prec).  on_hits(p0, hit, points, dirs, rgb, grad): called once per chunk that has a hit, after its
    forward, with the chunk's first pixel, the chunk-local indices of the HIT rays [h] int64 (ascending) and, for those rays,
    the surface points [h, 3] (unit-sphere frame), ray directions [h, 3], colours [h, 3] and SDF gradients [h, 3] -- the hook
    of surfcloud.fuse_views; it needs shade=True.  The planes do not depend on it."""
    from . import trace as T
    from .neuconw import default_infer_prec

    H, W = camera.height, camera.width
    hw = H * W
    chunk = max(1, min(int(chunk), hw))
    if device is None:
        device = next(rdr.neuconw.parameters()).device
    device = torch.device(device)
    if device.type != "cuda":
        raise L.NeuconwHipError("views.trace_view: the renderer is not on a GPU; the hot path has no CPU fallback")
    if on_hits is not None and not shade:
        raise ValueError("trace_view: on_hits needs shade=True (it receives the colours and gradients of the forward)")
    bg = [0.0, 0.0, 0.0]
    if background_rgb is not None:
        if torch.as_tensor(background_rgb).numel() != 3:
            raise ValueError("trace_view: background_rgb must hold ONE colour (3 values)")
        bg = [float(v) for v in torch.as_tensor(background_rgb).reshape(3).tolist()]
    lib = L.get_lib()
    cam = camera.struct()
    planes = {"color": torch.empty(3, H, W, device=device, dtype=torch.float32),
              "depth": torch.empty(H, W, device=device, dtype=torch.float32),
              "normal": torch.empty(3, H, W, device=device, dtype=torch.float32),
              "state": torch.empty(H, W, device=device, dtype=torch.uint8),
              "iters": torch.empty(H, W, device=device, dtype=torch.int32)}
    rays = torch.empty(chunk, 8, device=device, dtype=torch.float32)
    if shade_prec is None:
        shade_prec = default_infer_prec() if rdr.infer_prec is None else rdr.infer_prec
    launches = evaluated = forwards = 0
    with torch.no_grad():
        if a_code is not None:
            if not a_code.is_cuda:
                raise L.NeuconwHipError("views.trace_view: a_code is not on a GPU; the hot path has no CPU fallback")
            a_row = a_code.detach().reshape(1, -1).float()
        else:
            a_row = rdr.embeddings["a"](torch.full((1,), int(ts), device=device, dtype=torch.int64)).detach().float()
        for p0 in range(0, hw, chunk):
            n = min(chunk, hw - p0)
            r = rays[:n]
            L.check(lib.ncw_view_rays(C.byref(cam), p0, n, L.ptr(r), L.stream_ptr(device)), "ncw_view_rays")
            tr = T.trace_rays(rdr, r, **trace_kw)
            launches += tr["launches"]
            evaluated += tr["evaluated"]
            hit = rgb = grad = None
            if shade:
                hit = torch.nonzero(tr["state"] == T.HIT).reshape(-1)  # ascending; its length reaches the host here
                if hit.numel() > 0:
                    h = hit.numel()
                    x = torch.cat([tr["points"][hit], r[hit, 3:6], a_row.expand(h, -1)], 1).unsqueeze(1)
                    rgb, _, _, grad = rdr.neuconw(x, shade_prec)
                    forwards += 1
                    if on_hits is not None:
                        on_hits(p0, hit, x[:, 0, 0:3], x[:, 0, 3:6], rgb.reshape(h, 3), grad.reshape(h, 3))
                else:
                    hit = None
            T.store_chunk(planes, p0, tr, hit, rgb, grad, bg)
    res = dict(planes)
    res["depth_vis"] = depth_colormap(planes["depth"])
    cnt = torch.bincount(planes["state"].reshape(-1).long(), minlength=5).tolist()
    it = planes["iters"]
    res["stats"] = {"rays": hw, "hit": cnt[T.HIT], "miss": cnt[T.MISS], "inside": cnt[T.INSIDE], "stalled": cnt[T.STALLED],
                    "iters_mean": float(it.float().mean()), "iters_max": int(it.max()), "sdf_launches": launches,
                    "sdf_points": evaluated, "forward_launches": forwards}
    if gt is not None:
        g = gt.to(device).float()
        if g.dim() == 2:  # [H * W, 3], the dataset's layout
            g = g.reshape(H, W, 3).permute(2, 0, 1)
        g = g.reshape(3, H, W).contiguous()
        s, c = sqerr(planes["color"], g)
        res["mse"] = (s / c.float()).reshape(())
        res["psnr"] = -10.0 * torch.log10(res["mse"])
        res["psnr_hit"] = psnr(planes["color"], g, planes["state"] == T.HIT)
        if min(H, W) > (ssim_window - 1) // 2:
            res["ssim"] = ssim(planes["color"], g, ssim_window)
        else:
            res["ssim"] = torch.full((), float("nan"), device=device)
    return res


# ---------------------------------------------------------------------------------------------------
# the dataset's view (datasets/phototourism.py `val` / `test_train` item)
# ---------------------------------------------------------------------------------------------------
def _decode_image(path, downscale):
    """The decoded pixels [h, w, 3] uint8 (RGB, LANCZOS when downscaled: phototourism.py:542-551, 761-764)."""
    try:
        from PIL import Image
    except ImportError as e:  # pragma: no cover
        raise ImportError("reading the ground-truth image %s needs Pillow (PIL), which is not installed; pass "
                          "load_image=False to scene_view for the camera alone" % path) from e
    img = Image.open(path).convert("RGB")
    w, h = img.size
    if downscale > 1:  # phototourism.py:761-764
        w, h = w // downscale, h // downscale
        img = img.resize((w, h), Image.LANCZOS)
    return np.asarray(img, dtype=np.uint8).copy()


def _load_image(path, downscale):
    arr = _decode_image(path, downscale)
    h, w = arr.shape[:2]
    return torch.from_numpy(arr).permute(2, 0, 1).float().div(255.0), w, h  # ToTensor: [3, h, w] in [0, 1]


def reference_sfm_path(root_dir):
    """The COLMAP model directory (relative to <root_dir>/dense/) the reference's dataset reads for this scene
    (datasets/phototourism.py:82-93, keyed on the directory name): '../neuralsfm' for brandenburg_gate and
    palacio_de_bellas_artes -- the model their ray caches were built from; its image ids and poses differ from dense/sparse --
    and 'sparse' for every other scene."""
    name = os.path.basename(os.path.normpath(root_dir))
    return "../neuralsfm" if name in ("brandenburg_gate", "palacio_de_bellas_artes") else "sparse"


def read_scene(root_dir, sfm_path=None, with_points=False):
    """What the reference's dataset reads ONCE per scene (datasets/phototourism.py:316-350, 360, 453-462): the COLMAP model under
    <root_dir>/dense/<sfm_path> (None = `reference_sfm_path`) and the first *.tsv.  Returns a dict: `sp` (the model directory),
    `images` / `cams` (colmap.read_images / read_cameras), `tsv`, `by_name` {file name: image id}, `ids` (the tsv's
    images that are registered in images.bin, file order) and `ids_train` (those whose split is not 'test').  with_points: the
    images carry their 2-D points (colmap.read_images), which the ray cache needs."""
    if sfm_path is None:
        sfm_path = reference_sfm_path(root_dir)
    sp = os.path.normpath(os.path.join(root_dir, "dense", sfm_path))
    if not os.path.isfile(os.path.join(sp, "images.bin")):
        raise FileNotFoundError("no COLMAP model in %s (sfm_path %r): pass sfm_path / --sfm_path for the model the ray cache "
                                "was built from" % (sp, sfm_path))
    images = colmap.read_images(os.path.join(sp, "images.bin"), with_points)
    cams = colmap.read_cameras(os.path.join(sp, "cameras.bin"))
    tsv, rows = colmap.split_rows(root_dir)
    by_name = {im["name"]: iid for iid, im in images.items()}
    ids, ids_train = [], []
    for row in rows:
        if row["filename"] not in by_name:  # "image ... not found in sfm result" (:345-347)
            continue
        ids.append(by_name[row["filename"]])
        if row.get("split") != "test":
            ids_train.append(ids[-1])
    return {"sp": sp, "sfm_path": sfm_path, "images": images, "cams": cams, "tsv": tsv, "by_name": by_name, "ids": ids,
            "ids_train": ids_train}


def image_pose(scene, image_id, downscale):
    """K [3,3] f32 rescaled by (size // downscale) / size with the reference's size int(2 cx) x int(2 cy) (phototourism.py:367-375),
    w2c [4,4] f64, c2w [3,4] f64 = inv(w2c)[:3] with columns 1, 2 negated (:406-408), and the rescaled size (w, h)."""
    im = scene["images"][image_id]
    p = scene["cams"][im["camera_id"]]["params"]
    img_w, img_h = int(p[2] * 2), int(p[3] * 2)
    w_, h_ = img_w // downscale, img_h // downscale
    K = np.zeros((3, 3), dtype=np.float32)
    K[0, 0], K[1, 1] = p[0] * w_ / img_w, p[1] * h_ / img_h
    K[0, 2], K[1, 2] = p[2] * w_ / img_w, p[3] * h_ / img_h
    K[2, 2] = 1
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = colmap.qvec2rotmat(im["qvec"]), im["tvec"]
    c2w = np.linalg.inv(w2c)[:3].copy()
    c2w[:, 1:3] *= -1
    return K, w2c, c2w, w_, h_


def image_near_far(scene, w2c, scene_origin=None, scene_radius=None):
    """phototourism.py:426-444: the 0.1 / 99.9 percentiles of the depths of the SfM points in front of the camera, or
    origin_z -+ 1.5 radius when scene_origin (SfM frame) and scene_radius are given.  points3D.bin is read once per scene."""
    if scene_origin is not None:
        if scene_radius is None:
            raise ValueError("scene_view: scene_origin needs scene_radius")
        oz = (np.concatenate([np.asarray(scene_origin, dtype=np.float64), np.ones(1)])[None] @ w2c.T)[0, 2]
        return oz - float(scene_radius) * 1.5, oz + float(scene_radius) * 1.5
    if "xyz_h" not in scene:
        _, xyz, _, _ = colmap.read_points3d(os.path.join(scene["sp"], "points3D.bin"))
        scene["xyz_h"] = np.concatenate([xyz, np.ones((len(xyz), 1))], -1)
    z = (scene["xyz_h"] @ w2c.T)[:, 2]
    z = z[z > 0]
    return np.percentile(z, 0.1), np.percentile(z, 99.9)


def scene_view(root_dir, image_id=None, img_downscale=1, sfm_path=None, split="val", image_name=None, scene_origin=None,
               scene_radius=None, load_image=True):
    """The `val` / `test_train` item of the reference's dataset (datasets/phototourism.py:316-449, 749-802) for one image:
    returns (Camera, gt [3,h,w] f32 in [0,1] or None, image_id).
      * sfm_path: the COLMAP model under <root_dir>/dense/; None = the reference's per-scene choice (`reference_sfm_path`);
      * the images of <root_dir>/*.tsv that are registered in dense/<sfm_path>/images.bin, in file order; the default id is
        the first training image (`val_id = img_ids_train[0]`); image_name selects by file name;
      * K rescaled by (size // downscale) / size with the reference's size int(2 cx) x int(2 cy) (:367-375);
      * c2w = inv(w2c)[:3] with columns 1, 2 negated ("right down front" -> "right up back", :406-408);
      * near / far: the 0.1 / 99.9 percentiles of the depths of the SfM points in front of the camera, or
        origin_z -+ 1.5 radius when scene_origin (SfM frame) and scene_radius are given (:426-444);
      * split 'val' clamps the downscale to >= 8 (:70-71);
      * the image is decoded with PIL (RGB, LANCZOS when downscaled); the view takes the decoded image's size (:760-769).
    With load_image=False nothing is decoded: gt is None and the size is the K rescale's.  The scene files are read by
    `read_scene` / `image_pose` / `image_near_far`, which cachebuild shares."""
    downscale = int(img_downscale)
    if split == "val":
        downscale = max(8, downscale)
    scene = read_scene(root_dir, sfm_path)
    images, by_name, ids_train, sp = scene["images"], scene["by_name"], scene["ids_train"], scene["sp"]
    if image_name is not None:
        if image_name not in by_name:
            raise KeyError("image %r is not in %s" % (image_name, os.path.join(sp, "images.bin")))
        image_id = by_name[image_name]
    if image_id is None:
        if not ids_train:
            raise ValueError("%s lists no training image registered in images.bin" % scene["tsv"])
        image_id = ids_train[0]
    image_id = int(image_id)
    if image_id not in images:
        raise KeyError("image id %d is not in %s" % (image_id, os.path.join(sp, "images.bin")))
    K, w2c, c2w, w_, h_ = image_pose(scene, image_id, downscale)
    near, far = image_near_far(scene, w2c, scene_origin, scene_radius)
    gt = None
    if load_image:
        gt, w_, h_ = _load_image(os.path.join(root_dir, "dense", "images", images[image_id]["name"]), downscale)
    return Camera(K, c2w, w_, h_, near, far), gt, image_id


# ---------------------------------------------------------------------------------------------------
# PNG output (stdlib only)
# ---------------------------------------------------------------------------------------------------
def to_uint8(plane):
    """[3, H, W] f32 in [0, 1] (or [H, W]) -> [H, W, 3] uint8 on the host; NaN -> 0, values clamped."""
    t = torch.as_tensor(plane).detach().float().cpu()
    if t.dim() == 2:
        t = t.unsqueeze(0).expand(3, -1, -1)
    t = torch.nan_to_num(t, nan=0.0).clamp(0.0, 1.0)
    return (t * 255.0 + 0.5).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


def write_png(path, rgb):
    """8-bit RGB PNG of an [H, W, 3] uint8 array (zlib + struct: no imaging library)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("write_png: [H, W, 3] uint8 expected, got %s" % (rgb.shape,))
    h, w = rgb.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), dtype=np.uint8), rgb.reshape(h, 3 * w)], 1).tobytes()  # filter type 0 per row

    def block(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + block(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                 + block(b"IDAT", zlib.compress(raw, 6)) + block(b"IEND", b""))


def write_panel(path, *planes):
    """The reference's validation panel (neuconw_system.py:461-464: GT | prediction | depth | normal) as ONE PNG strip: the
    planes ([3, H, W] f32 in [0, 1]; None entries are left out) side by side.  Returns (width, height) of the strip."""
    tiles = [to_uint8(p) for p in planes if p is not None]
    if not tiles:
        raise ValueError("write_panel: no plane")
    if any(t.shape != tiles[0].shape for t in tiles):
        raise ValueError("write_panel: planes of different sizes: %s" % ([t.shape for t in tiles],))
    strip = np.concatenate(tiles, 1)
    write_png(path, strip)
    return strip.shape[1], strip.shape[0]
