"""Sphere tracing of the learned surface: the first point with |sdf| <= eps along each ray (not in the reference).

    out = trace_rays(rdr, rays)            # rays [R, 8] as render() takes them -> t, state, iters, points (unit-sphere units)

The per-ray recurrence -- a sphere-tracing walk that turns into false position / bisection once the sign changes -- runs in
`ncw_trace_begin` / `ncw_trace_step` (csrc/ncw_trace.hip; stated in include/neuconw_hip.h and restated in numpy float32 by
tests/_trace_ref.py).  Between two steps the SDF is evaluated on the points of the rays still active by the value-only kernel
(`SDFNetwork.sdf` at `value_prec()`); the active list is compacted on the device, in ascending ray order, so a ray's result does
not depend on which other rays travel with it.

LIMITATION: the bracket keeps the walk convergent where |grad sdf| > 1, but a surface whose two crossings fall inside ONE step
of the walk is jumped over (possible only where |grad sdf| * step > 1): the ray then reports a later surface or MISS.  step < 1
shrinks that; nothing here guarantees the first root of such a network.
"""
import ctypes as C

import torch

from . import lib as L

HIT, MISS, INSIDE, STALLED = 1, 2, 3, 4  # NCW_TRACE_* (include/neuconw_hip.h): part of the ABI
STATE_NAMES = {HIT: "hit", MISS: "miss", INSIDE: "inside", STALLED: "stalled"}
MAX_ITER = 16383  # NCW_TRACE_MAX_ITER


def _check_params(eps, step, max_iter, sync_every):
    if not eps > 0:
        raise ValueError("trace_rays: eps must be > 0 (got %r)" % (eps,))
    if not (step > 0 and step <= 1):
        raise ValueError("trace_rays: step must lie in (0, 1] (got %r)" % (step,))
    if int(max_iter) != max_iter or not 1 <= max_iter <= MAX_ITER:
        raise ValueError("trace_rays: max_iter must be an integer in [1, %d] (got %r)" % (MAX_ITER, max_iter))
    if int(sync_every) != sync_every or sync_every < 1:
        raise ValueError("trace_rays: sync_every must be an integer >= 1 (got %r)" % (sync_every,))


@torch.no_grad()
def trace_rays(rdr, rays, *, eps=1e-3, max_iter=64, step=1.0, far_override=None, sdf_fn=None, sync_every=4, prec=None,
               _observe=None):
    """March rays [R, >= 8] (o, d, near, far, ... as render() takes them; |d| = 1) to the zero level set of the renderer's SDF.
    The rays are normalised into unit-sphere units by render()'s own `ncw_ray_prologue` launch and marched over the interval the
    sampler would place its surface samples in (NeuconWRenderer.ray_intervals: near / far, the SfM octree's under far_override /
    `nerf_far_override`, the fine octree's band when `fine_octree_data` is set).
      eps, step, max_iter: the recurrence's parameters (include/neuconw_hip.h); step < 1 shortens the walk where |grad sdf| > 1;
      sdf_fn: callable points [m, 3] -> sdf [m] (or [m, 1]) on the device; default the renderer's value path at `prec`
              (None = `rdr.infer_prec`, i.e. SDFNetwork.value_prec());
      sync_every: the host reads the number of active rays back after every sync_every-th step only; in between it evaluates the
              SDF over the last count it knows (an upper bound).  The per-ray results do not depend on it.
    Returns a dict of device tensors: t [R] f32 (the depth at a HIT, near at INSIDE, else where the recurrence stopped), state [R]
    uint8 (HIT / MISS / INSIDE / STALLED), iters [R] int32 (SDF evaluations of the ray), points [R, 3] = o + t d in unit-sphere
    units (the network's input frame), and host numbers: launches (SDF launches), evaluated (points they covered), active (the
    count known to the host at each launch)."""
    _check_params(eps, step, max_iter, sync_every)
    if not (torch.is_tensor(rays) and rays.is_cuda):
        raise L.NeuconwHipError("trace.trace_rays: rays are not on a GPU; the hot path has no CPU fallback")
    if rays.dim() != 2 or rays.shape[1] < 8:
        raise ValueError("trace_rays: rays are [R, >= 8] (o, d, near, far), got %s" % (tuple(rays.shape),))
    dev = rays.device
    R = rays.shape[0]
    t = torch.empty(R, device=dev, dtype=torch.float32)
    state = torch.empty(R, device=dev, dtype=torch.uint8)
    iters = torch.empty(R, device=dev, dtype=torch.int32)
    points = torch.empty(R, 3, device=dev, dtype=torch.float32)
    res = {"t": t, "state": state, "iters": iters, "points": points, "launches": 0, "evaluated": 0, "active": []}
    if R == 0:
        return res
    if R > 2 ** 31 - 1:
        raise ValueError("trace_rays: at most 2^31 - 1 rays per call (got %d)" % R)
    if sdf_fn is None:
        p = rdr.infer_prec if prec is None else prec
        sdf_fn = lambda x: rdr.neuconw.sdf(x, p)  # noqa: E731
    rays_o, rays_d, near, far, _, _ = rdr.ray_prologue(rays)
    _, _, s_near, s_far = rdr.ray_intervals(rays_o, rays_d, near, far, far_override)
    s_near, s_far = s_near.reshape(-1).float().contiguous(), s_far.reshape(-1).float().contiguous()
    lib = L.get_lib()
    st = L.stream_ptr(dev)
    rec = torch.empty(R, 6, device=dev, dtype=torch.float32)
    active = [torch.empty(R, device=dev, dtype=torch.int32) for _ in range(2)]
    count = [torch.zeros(1, device=dev, dtype=torch.int32) for _ in range(2)]
    pts = torch.empty(R, 3, device=dev, dtype=torch.float32)
    scratch = torch.empty(int(lib.ncw_trace_scratch_bytes(R)), device=dev, dtype=torch.uint8)
    L.check(lib.ncw_trace_begin(L.ptr(rays_o), L.ptr(rays_d), L.ptr(s_near), L.ptr(s_far), R, L.ptr(rec), L.ptr(active[0]),
                                L.ptr(count[0]), L.ptr(pts), L.ptr(scratch), st), "ncw_trace_begin")
    m = int(count[0].item())
    cur = 0
    if _observe is not None:
        _observe(0, active[0][:m])
    for k in range(1, int(max_iter) + 1):
        if m == 0:
            break
        sdf = sdf_fn(pts[:m])
        if not (torch.is_tensor(sdf) and sdf.is_cuda):
            raise L.NeuconwHipError("trace.trace_rays: sdf_fn returned something that is not on a GPU")
        if sdf.numel() != m:
            raise ValueError("trace_rays: sdf_fn returned %d values for %d points" % (sdf.numel(), m))
        sdf = sdf.reshape(-1).float().contiguous()
        res["launches"] += 1
        res["evaluated"] += m
        res["active"].append(m)
        L.check(lib.ncw_trace_step(L.ptr(sdf), L.ptr(active[cur]), L.ptr(count[cur]), m, L.ptr(rays_o), L.ptr(rays_d),
                                   L.ptr(s_far), R, float(eps), float(step), int(max_iter), L.ptr(rec), L.ptr(active[cur ^ 1]),
                                   L.ptr(count[cur ^ 1]), L.ptr(pts), L.ptr(scratch), st), "ncw_trace_step")
        cur ^= 1
        if k % int(sync_every) == 0 and k < max_iter:
            m = int(count[cur].item())
            if _observe is not None:
                _observe(k, active[cur][:m])
    L.check(lib.ncw_trace_finish(L.ptr(rec), L.ptr(rays_o), L.ptr(rays_d), R, L.ptr(t), L.ptr(state), L.ptr(iters), L.ptr(points),
                                 st), "ncw_trace_finish")
    return res


def store_chunk(planes, p0, tr, hit_idx=None, rgb=None, grad=None, background=None):
    """Scatter one chunk's trace result `tr` (trace_rays' dict of n rays = the pixels [p0, p0 + n)) into the planes of a view
    (dict color [3,H,W], depth [H,W], normal [3,H,W], state [H,W] uint8, iters [H,W] int32): one `ncw_trace_store` call.
    hit_idx [h] int64 (ascending chunk-local indices of HIT rays) with rgb [h, 3] / grad [h, 3] of those rays; every other pixel
    gets `background` (3 host floats, default 0) as colour, depth 0 and normal 0."""
    n = tr["t"].shape[0]
    hw = planes["depth"].numel()
    h = 0 if hit_idx is None else int(hit_idx.numel())
    bg = (C.c_float * 3)(*([0.0, 0.0, 0.0] if background is None else [float(v) for v in background]))
    if h:
        hit_idx, rgb, grad = hit_idx.contiguous(), rgb.reshape(h, 3).float().contiguous(), grad.reshape(h, 3).float().contiguous()
    L.check(L.get_lib().ncw_trace_store(L.ptr(tr["t"]), L.ptr(tr["state"]), L.ptr(tr["iters"]), L.ptr(hit_idx if h else None),
                                        L.ptr(rgb if h else None), L.ptr(grad if h else None), h, bg, int(p0), n, hw,
                                        L.ptr(planes["color"]), L.ptr(planes["depth"]), L.ptr(planes["normal"]),
                                        L.ptr(planes["state"]), L.ptr(planes["iters"]), L.stream_ptr(planes["depth"].device)),
            "ncw_trace_store")
