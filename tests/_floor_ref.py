"""References of the floor-normal loss.  No GPU in here.

  floor_*               a torch restatement of the floor contract (the reference's rendering/renderer.py:918-945 `floor_loss`), in
                        any dtype: float64 arbitrates
  comp_reference_normals_on
                        tests/_ray_cases.comp_reference_on with one more upstream cotangent: the loss gains
                        (normals * d_normals).sum(), so autograd gives what composite_bwd_kernel must add for NcwCompositeGrad.d_normals
"""
import functools

import torch

from oracle import neuconw_oracle as O
from tests import _ray_cases as C


# --------------------------------------------------------------------------------------------------------------------
# floor contract
# --------------------------------------------------------------------------------------------------------------------
def floor_n_gt(sfm_to_gt):
    """sfm_to_gt.float()[:3,:3].T @ e_z over its float32 norm (renderer.py:930-937) -> float32 [3]."""
    v = torch.as_tensor(sfm_to_gt).float()[:3, :3].T @ torch.tensor([0.0, 0.0, 1.0])
    return v / torch.linalg.norm(v)


def floor_mask(label, ids):
    m = torch.zeros(label.shape[0], dtype=torch.bool)
    for i in ids:
        m |= label == i
    return m


def floor_forward(normals, label, ids, n_gt, rays_o, rays_d, depth, scaled, dtype=torch.float64):
    """-> (floor_error [R,3] dense, n_floor, y_var) in `dtype` from inputs of any dtype."""
    t = lambda x: x.to(dtype)  # noqa: E731
    m = floor_mask(label, ids)
    n = int(m.sum())
    R = normals.shape[0]
    scale = (R / max(n, 1)) if scaled else 1.0
    fe = (t(normals) - t(n_gt)).abs() * t(m)[:, None] * scale
    xyz = t(rays_o) + t(rays_d) * t(depth).reshape(-1, 1)
    y_var = torch.var(xyz[m]) if n > 0 else torch.zeros((), dtype=dtype)
    return fe, n, y_var


def floor_backward(normals, label, ids, n_gt, d_fe, scaled, dtype=torch.float64):
    """d_normals by autograd through the restatement (torch's abs has sign(0) = 0, like its L1 loss)."""
    x = normals.to(dtype).requires_grad_(True)
    z = torch.zeros(normals.shape[0], 3, dtype=dtype)
    fe, _, _ = floor_forward(x, label, ids, n_gt, z, z, z[:, 0], scaled, dtype)
    return torch.autograd.grad((fe * d_fe.to(dtype)).sum(), x)[0]


# --------------------------------------------------------------------------------------------------------------------
# compositor with a cotangent for `normals`
# --------------------------------------------------------------------------------------------------------------------
def d_normals_of(c):
    """The seeded upstream cotangent of `normals` for a compositor case [R,3] (fp32, never modified)."""
    return torch.randn(c.R, 3, generator=torch.Generator().manual_seed(2))


def comp_reference_normals_on(I, c, dtype, d_normals, scale=1.0, only_normals=False):
    """Adjoints {name: tensor} of O.composite in `dtype` for the loss of C.comp_reference_on + (normals * d_normals).sum(), every
    cotangent times `scale`; only_normals: every other cotangent is zero."""
    t = lambda x: x.to(dtype) if x is not None else None  # noqa: E731
    leaf = {k: I[k].to(dtype).requires_grad_(True) for k in ("sdf", "grad", "rgb", "inv_s")}
    bg_alpha = None
    if c.with_bg:
        leaf["density"] = I["density"].to(dtype).requires_grad_(True)
        leaf["bg_rgb"] = I["bg_rgb"].to(dtype).requires_grad_(True)
        bg_alpha = O.bg_alpha_from_density(leaf["density"], t(I["z_feed"]), t(I["sample_dist"]))
    ref = O.composite(dict(trim_sphere=c.trim), t(I["o"]), t(I["d"]), t(I["z"]), t(I["sample_dist"]), leaf["rgb"], leaf["inv_s"],
                      leaf["sdf"], leaf["grad"], c.cos, bg_alpha, leaf.get("bg_rgb"), t(I["background_rgb"]))
    ct = I["cot"]
    loss = (ref["normals"] * (t(d_normals) * scale)).sum()
    if not only_normals:
        loss = loss + (ref["color"] * (t(ct["d_color"]) * scale)).sum()
        loss = loss + (ref["weights_sum"][:, 0] * (t(ct["d_weights_sum"]) * scale)).sum()
        if ct["d_depth"] is not None:
            loss = loss + (ref["depth"] * (t(ct["d_depth"]) * scale)).sum()
        if ct["d_eik_num"] is not None:
            loss = loss + (ref["eik_num"] * (t(ct["d_eik_num"]) * scale)).sum()
    names = list(leaf)
    adj = torch.autograd.grad(loss, [leaf[k] for k in names], allow_unused=True)
    return {k: (v if v is not None else torch.zeros_like(leaf[k])).detach() for k, v in zip(names, adj)}


@functools.lru_cache(maxsize=None)
def comp_reference_normals(c, scale=1.0, only_normals=False):
    """-> (adj64, adj32) of a case with d_normals_of(c): computed once, shared, left unchanged."""
    I = C.comp_case_inputs(c)
    dn = d_normals_of(c)
    return (comp_reference_normals_on(I, c, torch.float64, dn, scale, only_normals),
            comp_reference_normals_on(I, c, torch.float32, dn, scale, only_normals))
