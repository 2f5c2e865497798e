"""The inputs and calls of the per-ray fixture tests/golden/rays_parent.npz: every entry point of csrc/ncw_rays.hip that
keeps a ray in LDS or shares a formula with one that does (ncw_composite_fwd / _bwd, ncw_upsample, ncw_sort_merge,
ncw_sample_coarse, ncw_boundary, ncw_bg_select) over the seeded cases of tests/_ray_cases.py, at the smallest shapes that reach
every path: R = 5 rays (one full workgroup of four waves plus one), both LDS capacities (512 / 1088) on both sides of their
thresholds.  tests/golden/make_golden_rays_parent.py runs `compute` on the build whose outputs are the reference,
tests/test_gpu_rays_parent.py on the build under test.

Per-ray outputs are kept as arrays, per-sample outputs as the SHA-256 of their bytes (`packed`): as exact a comparison, and the
file stays small.  `inputs_digest` is stored beside the outputs and checked before anything is compared."""
import hashlib

import numpy as np
import torch

from tests import _ray_cases as C

R = 5
# compositor outputs with one value per ray (kept as arrays); every other output has one per sample (kept as a digest)
PER_RAY = ("color", "color_sphere", "color_bg", "weights_sum", "weights_max", "depth", "normals", "eik", "d_inv_s")
UPSAMPLE = [(2, 8, 512.0), (64, 65, 512.0), (65, 64, 1024.0), (511, 128, 512.0), (512, 128, 1024.0), (1087, 128, 4096.0)]
MERGE = [(448, 64, True), (509, 4, True), (1056, 32, False)]  # 512 and 513 in all with the payload, 1088 without
COARSE = [(n, 4, perturb) for n in (65, 513) for perturb in (False, True)]
BOUNDARY = (24, 5)
BG_SELECT = (70, 9, 37, 4)  # rays, seed (test_gpu_bg_select.py: _rays_crossing_the_sphere), primary samples, outside samples
EXTRA_SHAPE = (61, 4)       # the device-scalar cos_anneal and the grad_scale calls


def comp_cases():
    seen, out = set(), []
    for c in C.shape_cases() + C.option_cases():
        if c not in seen:
            seen.add(c)
            out.append(c)
    assert all(c.R == R for c in out)
    return out


def bg_select_inputs():
    """(o, d, z [70, 37], sample_dist [70]): the rays of tests/test_gpu_bg_select.py, whose interval [0.6, 3.6] leaves the unit
    sphere at both ends, with sorted uniform samples on it."""
    from tests.test_gpu_bg_select import _rays_crossing_the_sphere

    n, seed, S, _ = BG_SELECT
    rays = _rays_crossing_the_sphere(n, seed)[0]
    g = torch.Generator().manual_seed(100 + seed)
    near, far = rays[:, 6:7], rays[:, 7:8]
    z = torch.sort(near + (far - near) * torch.rand(n, S, generator=g), -1)[0]
    return rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous(), z.contiguous(), ((far - near) / S).reshape(-1).contiguous()


def _tensors(x):
    if torch.is_tensor(x):
        yield x
    elif isinstance(x, dict):
        for k in sorted(x):
            yield from _tensors(x[k])
    elif isinstance(x, (tuple, list)):
        for v in x:
            yield from _tensors(v)


def inputs_digest():
    h = hashlib.sha256()
    groups = [C.comp_case_inputs(c) for c in comp_cases()]
    groups += [{k: v for k, v in C.upsample_case(n, nn, s, R=R).items() if k in ("o", "d", "z", "sdf")} for n, nn, s in UPSAMPLE]
    groups += [{k: v for k, v in C.merge_case(na, nb, R=R).items() if k in ("a", "b", "pa", "pb")} for na, nb, _ in MERGE]
    groups += [{k: v for k, v in C.coarse_case(R, n, no, p).items() if not k.startswith("ref")} for n, no, p in COARSE]
    groups += [{k: v for k, v in C.boundary_case(*BOUNDARY, R=R).items() if not k.startswith("ref")}]
    groups += [bg_select_inputs()]
    for g in groups:
        for t in _tensors(g):
            h.update(t.detach().contiguous().numpy().tobytes())  # (comp_reference leaves requires_grad on the shared inputs)
    return h.hexdigest()


def _cu(*ts):
    return [t.detach().cuda() if t is not None else None for t in ts]


def _comp(out, tag, c, cos=None, grad_scale=1.0, grad_scale_dev=None):
    from neuralrecon_w_amd import rayops

    I = C.comp_case_inputs(c)
    ctx = rayops.CompositeCtx(*_cu(I["o"], I["d"], I["z"], I["sample_dist"], I["sdf"], I["grad"], I["rgb"], I["inv_s"]),
                              c.cos if cos is None else cos, *_cu(I["z_feed"], I["density"], I["bg_rgb"]),
                              background_rgb=I["background_rgb"].detach().cuda() if I["background_rgb"] is not None else None,
                              trim_sphere=c.trim)
    fwd = ctx.forward()
    if not c.with_bg:
        fwd.pop("color_bg")  # written as zeros without a background
    ct = I["cot"]
    adj = ctx.backward(*_cu(ct["d_color"], ct["d_weights_sum"], ct["d_depth"], ct["d_eik_num"]), grad_scale=grad_scale,
                       grad_scale_dev=grad_scale_dev)
    for k, v in list(fwd.items()) + list(adj.items()):
        if v is not None:
            out["%s.%s.%s" % (tag, C.case_id(c), k)] = v


def compute(device="cuda:0"):
    """{name: tensor on the host} of every output of the calls above, as the kernels wrote them."""
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import rayops

    assert torch.device(device) == torch.device("cuda:0")
    out = {}
    for c in comp_cases():
        _comp(out, "comp", c)
    c = C.comp_case(*EXTRA_SHAPE)
    _comp(out, "comp_cos_dev", c, cos=torch.tensor([c.cos], device="cuda"))
    _comp(out, "comp_scale8_dev", c, grad_scale=8.0, grad_scale_dev=torch.tensor([0.5], device="cuda"))
    _comp(out, "comp_scale0", c, grad_scale=0.0)  # grad_scale 0 means 1: the one field the host edits
    for n, n_new, inv_s in UPSAMPLE:
        U = C.upsample_case(n, n_new, inv_s, R=R)
        out["upsample.%d.z_new" % n] = rayops.upsample(*_cu(U["o"], U["d"], U["z"], U["sdf"]), n_new, inv_s)
    for na, nb, payload in MERGE:
        M = C.merge_case(na, nb, R=R)
        a, b, pa, pb = _cu(M["a"], M["b"], M["pa"], M["pb"])
        merged, pout = rayops.sort_merge(a, b, pa, pb) if payload else rayops.sort_merge(a, b)
        out["merge.%d.out" % (na + nb)] = merged
        if payload:
            out["merge.%d.payload" % (na + nb)] = pout
    for n, no, perturb in COARSE:
        K = C.coarse_case(R, n, no, perturb)
        got = rayops.sample_coarse(*_cu(K["near"], K["far"], K["s_near"], K["s_far"]), n, no, *_cu(K["rs"], K["ro"]))
        for name, t in zip(("z", "z_out", "sample_dist"), got):
            out["coarse.%d.%s.%s" % (n, "jitter" if perturb else "plain", name)] = t
    B = C.boundary_case(*BOUNDARY, R=R)
    out["boundary.zb"] = rayops.boundary(*_cu(B["near"], B["far"], B["z"]), BOUNDARY[1])
    o, d, z, sd = _cu(*bg_select_inputs())
    n, _, S, O_ = BG_SELECT
    idx = torch.full((n * (S + O_),), -1, dtype=torch.int32, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(L.get_lib().ncw_bg_select(L.ptr(o), L.ptr(d), L.ptr(z), L.ptr(sd), n, S, O_, L.ptr(idx), L.ptr(offs), L.ptr(cnt),
                                      L.stream_ptr(o.device)), "ncw_bg_select")
    out["bg_select.idx"], out["bg_select.offsets"] = idx[: int(cnt)], offs
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def per_ray(name):
    """Is output `name` kept as an array (one value per ray, and the bg_select list) or as a digest?"""
    return name.startswith("bg_select.") or name.endswith(".sample_dist") or name.rsplit(".", 1)[1] in PER_RAY


def packed(out):
    """The outputs as the fixture stores them."""
    sha = lambda t: torch.from_numpy(  # noqa: E731
        np.frombuffer(hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest().encode("ascii"), dtype=np.uint8).copy())
    return {k: (v if per_ray(k) else sha(v)) for k, v in out.items()}
