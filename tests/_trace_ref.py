"""numpy restatement of the sphere tracer's per-ray recurrence (include/neuconw_hip.h, "Surface views by sphere tracing";
csrc/ncw_trace.hip) -- the yardstick of tests/test_trace_host.py and tests/test_gpu_trace.py.  `march` runs it in any float dtype:
float32 restates the kernels bit for bit (every product, quotient and sum rounded once, in the kernels' order), float64 is the
oracle march.  Also the analytic SDFs and the small view the GPU tests share.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

HIT, MISS, INSIDE, STALLED = 1, 2, 3, 4


def points_of(o, d, t):
    """p = o + t d: the product, then the sum, per component, in the arrays' dtype."""
    return o + t[:, None] * d


def march(o, d, near, far, sdf_fn, eps=1e-3, step=1.0, max_iter=64, dtype=np.float32):
    """o, d [R, 3], near, far [R]; sdf_fn: points [m, 3] (dtype) -> sdf [m].  Returns dict t, state (uint8), iters (int32),
    points [R, 3], lists (the ascending active list in front of every evaluation, the begin list first; the last one may be
    empty), evaluated (points handed to sdf_fn)."""
    f = dtype
    o, d = np.asarray(o, dtype=f), np.asarray(d, dtype=f)
    near, far = np.asarray(near, dtype=f).reshape(-1), np.asarray(far, dtype=f).reshape(-1)
    R = o.shape[0]
    eps, step, half = f(eps), f(step), f(0.5)
    t = near.copy()
    t_lo, t_hi = near.copy(), near.copy()
    s_lo, s_hi = np.zeros(R, f), np.zeros(R, f)
    state = np.where(far > near, 0, MISS).astype(np.uint8)
    br = np.zeros(R, np.int64)
    iters = np.zeros(R, np.int32)
    lists, evaluated = [np.nonzero(state == 0)[0]], 0
    for k in range(1, int(max_iter) + 1):
        act = lists[-1]
        if act.size == 0:
            break
        with np.errstate(all="ignore"):
            s = np.asarray(sdf_fn(points_of(o[act], d[act], t[act])), dtype=f).reshape(-1)
        assert s.shape[0] == act.size
        evaluated += act.size
        iters[act] += 1
        for j, r in enumerate(act):  # per ray, as the kernel's thread does it
            sj = s[j]
            if not np.isfinite(sj):
                state[r] = STALLED
            elif abs(sj) <= eps:
                state[r] = HIT
            elif sj > 0:
                t_lo[r], s_lo[r] = t[r], sj
            elif k == 1:
                state[r] = INSIDE
            else:
                t_hi[r], s_hi[r] = t[r], sj
                br[r] = max(br[r], 1)
            if state[r] != 0:
                continue
            if br[r] == 0:
                tn = f(t[r] + f(step * sj))
                if tn > far[r]:
                    state[r] = MISS
                else:
                    t[r] = tn
            else:
                w = f(t_hi[r] - t_lo[r])
                if br[r] & 1:
                    t[r] = f(t_lo[r] + f(f(s_lo[r] * w) / f(s_lo[r] - s_hi[r])))
                else:
                    t[r] = f(t_lo[r] + f(half * w))
                br[r] += 1
            if state[r] == 0 and k == max_iter:
                state[r] = STALLED
        lists.append(act[state[act] == 0])
    return {"t": t, "state": state, "iters": iters, "points": points_of(o, d, t), "lists": lists, "evaluated": evaluated}


# ---- analytic SDFs (float32 in, float32 out, each operation rounded once) -------------------------------------------------
def sphere_sdf(radius=0.5, scale=1.0):
    """scale * (|p| - radius): gradient `scale` everywhere."""
    def fn(p):
        f = p.dtype.type
        n = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2])
        return f(scale) * (n - f(radius))
    return fn


def sphere_slab_sdf(radius=0.5, scale=3.0, z0=0.7, half=0.02):
    """A sphere scaled by `scale` united with a thin slab |z - z0| <= half (also scaled): gradient 3, a thin sheet in front."""
    sph = sphere_sdf(radius, scale)

    def fn(p):
        f = p.dtype.type
        slab = f(scale) * (np.abs(p[:, 2] - f(z0)) - f(half))
        return np.minimum(sph(p), slab)
    return fn


# ---- the small view of the GPU tests (tests/_view_ref.py's ray formula: integer pixel coordinates) --------------------------
VIEW_W, VIEW_H, VIEW_FOCAL, VIEW_NEAR, VIEW_FAR = 24, 16, 20.0, 0.2, 4.0
VIEW_EYE = (0.1, -0.05, 1.6)


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """c2w [3, 4] in the renderer's "right up back" axes: the camera looks along -z of its frame."""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    upv = np.cross(back, right)
    return np.stack([right, upv, back, eye], 1)


def view_camera_args(eye=VIEW_EYE, target=(0.0, 0.0, 0.0)):
    """(K, c2w, width, height, near, far) of the 24 x 16 view: focal 20 px, principal point at the centre."""
    K = np.array([[VIEW_FOCAL, 0, VIEW_W / 2.0], [0, VIEW_FOCAL, VIEW_H / 2.0], [0, 0, 1]], dtype=np.float32)
    return K, look_at(eye, target).astype(np.float32), VIEW_W, VIEW_H, VIEW_NEAR, VIEW_FAR


def view_rays64(eye=VIEW_EYE, target=(0.0, 0.0, 0.0)):
    """Rays [384, 8] float64 of that view by tests/_view_ref.py's formula."""
    from tests import _view_ref as VR

    K, c2w, W, H, near, far = view_camera_args(eye, target)
    return VR.view_rays(K, c2w, W, H, near, far).numpy()


# ---- the fixture networks and their fp64 oracle -------------------------------------------------------------------------------
FIXTURES = {"A": dict(W=64, n_layers=8, skip=(4,), jitter=False), "B": dict(W=64, n_layers=8, skip=(4,), jitter=True),
            "C": dict(W=64, n_layers=2, skip=(), jitter=True), "D": dict(W=256, n_layers=8, skip=(4,), jitter=True),
            # D as `_mk` builds it by default (perturbed) has NO surface in front of this camera (0 hits on the fp64 oracle), so
            # D0 -- the same width unperturbed: a sphere -- gives the split-fp16 value path hits to be measured on.  Its two
            # grazing rays creep past the silhouette for 65 and 91 evaluations on the fp64 oracle itself, so D0 marches with
            # max_iter = 128 (the recurrence's property at that cap, not the kernels').
            "D0": dict(W=256, n_layers=8, skip=(4,), jitter=False, max_iter=128)}
TOL_F32 = 1e-4     # tests/test_gpu_sdf.py test_sdf_infer_vs_oracle: max |sdf - oracle| < TOL_F32 max |oracle|, fp32 value path
TOL_SPLIT = 5e-6   # tests/test_gpu_sdf.py test_split_precision_value_path: the same measure for the split-fp16 value path


def mk_net(W, n_layers, skip, seed=0, jitter=True):
    """tests/test_gpu_sdf.py `_mk`, on the CPU (the caller moves it): same seed, same construction and perturbation order."""
    import torch

    import neuralrecon_w_amd as nw

    torch.manual_seed(seed)
    net = nw.SDFNetwork(d_in=3, d_out=W + 1, d_hidden=W, n_layers=n_layers, skip_in=skip)
    if jitter:
        with torch.no_grad():
            for n, p in net.named_parameters():
                if n.endswith("weight_g"):
                    p.mul_(1.0 + 0.1 * torch.randn_like(p))
                if n.endswith("weight_v") and not n.startswith("lin%d" % (net.n_lin - 1)):
                    p.add_(0.02 * torch.randn_like(p))
    return net


def oracle_of(net, skip):
    """(sdf64(points [m,3] float64 numpy) -> [m], grad64 -> [m,3], scale) of a network on the fp64 CPU oracle.  scale = max |sdf|
    over the cube sample of test_sdf_infer_vs_oracle (4133 points in [-1.2, 1.2]^3, seed 5): the magnitude the project's value-path
    bounds (TOL_F32, TOL_SPLIT) are relative to."""
    import torch

    from oracle import neuconw_oracle as O

    sd = {"sdf_net." + k: v.detach().cpu().double() for k, v in net.state_dict().items()}

    def sdf64(p):
        return O.sdf_net(sd, torch.from_numpy(np.ascontiguousarray(p, dtype=np.float64)), skip_in=skip, with_grad=False)[0].numpy()

    def grad64(p):
        return O.sdf_net(sd, torch.from_numpy(np.ascontiguousarray(p, dtype=np.float64)), skip_in=skip)[2].numpy()

    g = torch.Generator().manual_seed(5)
    x = (torch.rand(4133, 3, generator=g) * 2 - 1) * 1.2
    return sdf64, grad64, float(np.abs(sdf64(x.double().numpy())).max())


def fixture_stats(sdf64, grad64, rays, res, ref, eps, delta, n_depths=512):
    """What tests 3-5 of the issue measure, from one march `res` (t, state) against the fp64 march `ref` of the same rays [R, 8]
    (float64): dict with residual (max |sdf64(p_hit)| over res' HIT rays, at res' own `points` when it carries them), n_hit, left_out (hit rays with D < 0.2 or a state that
    differs), worst_dt_ratio (max |dt| / bound over the compared rays), and for the MISS rays of res: band (rays whose minimum
    over n_depths uniform depths is below 10 (eps + delta)) and crossed (the others whose minimum is <= 0)."""
    o, d = rays[:, 0:3], rays[:, 3:6]
    st, t = np.asarray(res["state"]), np.asarray(res["t"], dtype=np.float64)
    hit = st == HIT
    out = {"n_hit": int(hit.sum()), "n_miss": int((st == MISS).sum()), "n_stalled": int((st == STALLED).sum()),
           "n_inside": int((st == INSIDE).sum())}
    p_hit = np.asarray(res["points"], dtype=np.float64)[hit] if "points" in res else o[hit] + t[hit, None] * d[hit]
    out["residual"] = float(np.abs(sdf64(p_hit)).max()) if hit.any() else 0.0
    both = hit & (np.asarray(ref["state"]) == HIT)
    t_ref = np.asarray(ref["t"], dtype=np.float64)
    D = np.full(len(st), np.inf)
    if both.any():
        ga = np.abs((grad64(o[both] + t[both, None] * d[both]) * d[both]).sum(1))
        gb = np.abs((grad64(o[both] + t_ref[both, None] * d[both]) * d[both]).sum(1))
        D[both] = np.minimum(ga, gb)
    cmp_ = both & (D >= 0.2)
    out["left_out"] = int(hit.sum() - cmp_.sum())
    bound = 2.0 * (2.0 * eps + delta) / D[cmp_]
    out["worst_dt_ratio"] = float((np.abs(t - t_ref)[cmp_] / bound).max()) if cmp_.any() else 0.0
    miss = np.nonzero(st == MISS)[0]
    z = np.linspace(rays[miss, 6], rays[miss, 7], n_depths, axis=1) if miss.size else np.zeros((0, n_depths))
    pts = o[miss, None, :] + z[:, :, None] * d[miss, None, :]
    mn = sdf64(pts.reshape(-1, 3)).reshape(miss.size, n_depths).min(1) if miss.size else np.zeros(0)
    band = mn < 10.0 * (eps + delta)
    out["band"] = int(band.sum())
    out["crossed"] = int((mn[~band] <= 0).sum())
    out["crossed_any"] = int((mn <= 0).sum())
    return out
