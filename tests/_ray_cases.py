"""Case generators and references for the per-ray sampler / compositor kernels (csrc/ncw_rays.hip).  No GPU in here.

Every reference is oracle/neuconw_oracle.py evaluated twice on the same fp32 inputs: in float64, which arbitrates, and in
float32 on the CPU -- the "fp32 restatement", the reference's own arithmetic.  A kernel is held to
`err_kernel <= max(floor, 4 * err_fp32_restatement)`, both errors against float64 (`bound`): the floors are those of
tests/test_gpu_rays.py; the factor 4 is two bits for the kernels' chunked wave scans (another summation order than cumprod)
and for expf / log1pf a few ulp from torch's -- not margin for a wrong term, which shows at 1e-3 and above.

The conditions a case must satisfy (guard band, exclusion cap, finite references) are decided on the references alone --
tests/test_ray_cases_host.py asserts them for every case the GPU tests use; a kernel's output is never consulted."""
import collections
import functools

import torch

from oracle import neuconw_oracle as O
from tests._util import rel_err, synth_rays

FLOOR_FWD, FLOOR_EIK_DEN, FLOOR_ADJ, FLOOR_SAMPLE, FLOOR_UPSAMPLE = 2e-5, 1e-6, 1e-4, 1e-6, 2e-5
FACTOR = 4.0
GUARD_BAND = 5e-6       # no section mid-point within this of the radii 1.0 / 1.2 (the masks pn < 1.0, pn < 1.2 are discontinuous)
UPSAMPLE_EXCLUDE = 2e-5  # a ray is left out iff the fp32 restatement is off float64 by more than this (of max |z|) on it ...
UPSAMPLE_CAP = 0.05      # ... and at most this fraction of a case's rays may be


def bound(floor, err32):
    return max(floor, FACTOR * err32)


# --------------------------------------------------------------------------------------------------------------------
# compositor
# --------------------------------------------------------------------------------------------------------------------
def comp_inputs(R, S, O_, seed, with_bg=True, inv_s=20.0, dens_extreme=False, zero_grad_col=False, miss_ray=False,
                deep_ray=False):
    """The compositor inputs of tests/test_gpu_rays.py (same random stream), plus value switches applied afterwards:
      dens_extreme   density 25 on columns 1::5 and -25 on columns 3::5 (F.softplus threshold 20; exp(-25) under fp32 eps)
      zero_grad_col  grad = 0 on column S // 2 (gn == 0 in the eikonal adjoint; true_cos == 0: the relu kinks)
      miss_ray       ray 1's origin moved by +3 in x: it misses the unit sphere and the radius 1.2 (all inside = 0)
      deep_ray       ray 2 has sdf = -0.5 throughout (at inv_s = 3000 both sigmoids underflow to 0: alpha = 1e-5 / 1e-5)"""
    g = torch.Generator().manual_seed(seed)
    rays, _, _, _ = synth_rays(R, seed, 10)
    o, d = rays[:, 0:3], rays[:, 3:6]
    z = torch.sort(1.0 + 2.2 * torch.rand(R, S, generator=g), -1)[0]
    sample_dist = torch.full((R, 1), 2.0 / S)
    mid = z + torch.cat([z[:, 1:] - z[:, :-1], sample_dist], -1) * 0.5
    pts = o[:, None] + d[:, None] * mid[..., None]
    sdf = pts.norm(dim=-1) - 0.5 + 0.01 * torch.randn(R, S, generator=g)
    grad = pts / pts.norm(dim=-1, keepdim=True) * (1 + 0.1 * torch.randn(R, S, 1, generator=g)) \
        + 0.05 * torch.randn(R, S, 3, generator=g)
    rgb = torch.rand(R, S, 3, generator=g)
    z_out = 3.3 + torch.sort(torch.rand(R, O_, generator=g), -1)[0] * 5
    z_feed = torch.sort(torch.cat([z, z_out], -1), -1)[0] if with_bg else None
    density = torch.randn(R, S + O_, generator=g) * 2 if with_bg else None
    bg_rgb = torch.rand(R, S + O_, 3, generator=g) if with_bg else None
    if dens_extreme and with_bg:
        density[:, 1::5] = 25.0
        density[:, 3::5] = -25.0
    if zero_grad_col:
        grad[:, S // 2] = 0.0
    if miss_ray:
        o = o.clone()
        o[1, 0] += 3.0
    if deep_ray:
        sdf[2] = -0.5
    return dict(o=o, d=d, z=z, sample_dist=sample_dist, sdf=sdf, grad=grad, rgb=rgb, z_feed=z_feed, density=density,
                bg_rgb=bg_rgb, inv_s=torch.tensor([float(inv_s)]))


# One compositor case.  cos is a python float; brgb: a background colour is passed; values: the four value switches at once;
# cot: "all" or "no_depth_eik" (d_depth and d_eik_num handed over as None).  The seed is 7 + S like tests/test_gpu_rays.py unless
# the guard band asked for another (test_ray_cases_host.py: test_comp_case_conditions); it is fixed here, by hand.
CompCase = collections.namedtuple("CompCase", "S O with_bg R seed inv_s cos brgb trim values cot")


def comp_case(S, O_, with_bg=None, R=5, seed=None, inv_s=20.0, cos=0.3, brgb=True, trim=True, values=False, cot="all"):
    with_bg = True if with_bg is None else with_bg
    return CompCase(S, O_, with_bg, R, _SEEDS.get((S, O_, R), 7 + S) if seed is None else seed, float(inv_s), float(cos), brgb,
                    trim, values, cot)


# (S, O, R) -> seed, where 7 + S puts a mid-point inside the guard band: (1088, 0) at seed 1095 has one 3.8e-6 off radius 1.0
_SEEDS = {(1088, 0, 5): 1096}

SHAPES_STD = [(1, 0), (1, 1), (2, 0), (63, 0), (64, 0), (65, 0), (60, 4), (61, 4), (127, 2), (448, 64), (512, 0)]
SHAPES_BIG = [(509, 4), (512, 1), (1024, 32), (1056, 32), (1088, 0)]
OPTION_SHAPES = [(61, 4), (509, 4)]  # one per capacity
INDEP_SHAPES = [(61, 4), (1056, 32)]


def shape_cases():
    cs = [comp_case(S, O_) for S, O_ in SHAPES_STD + SHAPES_BIG]
    cs.append(comp_case(64, 0, with_bg=False))  # z_feed = None
    return cs


def option_cases():
    cs = []
    for S, O_ in OPTION_SHAPES:
        cs += [comp_case(S, O_, trim=t) for t in (True, False)]
        cs += [comp_case(S, O_, brgb=False)]
        cs += [comp_case(S, O_, cos=c) for c in (0.0, 1.0)]  # 0.3 is the default case above
        cs += [comp_case(S, O_, inv_s=s) for s in (403.0, 3000.0)]
        cs += [comp_case(S, O_, inv_s=s, cos=1.0) for s in (403.0,)]  # d_inv_s as a cancelling sum
        cs += [comp_case(S, O_, inv_s=s, values=True) for s in (20.0, 403.0, 3000.0)]
        cs += [comp_case(S, O_, cot="no_depth_eik")]
    return cs


def indep_cases():
    return [comp_case(S, O_, R=9, values=True) for S, O_ in INDEP_SHAPES]


def scale_cases():
    """grad_scale cases: the plain inputs.  A power-of-two scale commutes with every fp32 operation except a rounding in the
    subnormal range, so `2 x bit for bit` holds exactly where no intermediate is subnormal.  With the value switches on it does
    not hold for the fp32 restatement itself: on the sdf = -0.5 ray the transmittance runs through the subnormals to 0 at
    S = 509 (test_ray_cases_host.py: test_scale_cases_scale_exactly_in_fp32 decides this on the reference)."""
    return [comp_case(S, O_) for S, O_ in OPTION_SHAPES]


def all_comp_cases():
    seen, out = set(), []
    for c in shape_cases() + option_cases() + indep_cases() + scale_cases():
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def case_id(c):
    s = "S%d_O%d_R%d" % (c.S, c.O, c.R)
    if not c.with_bg:
        s += "_nobg"
    if c.inv_s != 20.0:
        s += "_s%d" % c.inv_s
    if c.cos != 0.3:
        s += "_cos%g" % c.cos
    if not c.brgb:
        s += "_nobrgb"
    if not c.trim:
        s += "_notrim"
    if c.values:
        s += "_values"
    if c.cot != "all":
        s += "_" + c.cot
    return s


BACKGROUND_RGB = (0.1, 0.2, 0.3)


@functools.lru_cache(maxsize=None)
def comp_case_inputs(c):
    """fp32 inputs of a case (never modified afterwards), the upstream cotangents included."""
    I = comp_inputs(c.R, c.S, c.O, c.seed, c.with_bg, c.inv_s, c.values, c.values, c.values, c.values)
    g = torch.Generator().manual_seed(1)
    I["cot"] = dict(d_color=torch.randn(c.R, 3, generator=g), d_weights_sum=torch.randn(c.R, generator=g),
                    d_depth=torch.randn(c.R, generator=g), d_eik_num=torch.randn(c.R, generator=g))
    if c.cot == "no_depth_eik":
        I["cot"]["d_depth"] = I["cot"]["d_eik_num"] = None
    I["background_rgb"] = torch.tensor([BACKGROUND_RGB]) if c.brgb else None
    return I


def guard_distance(I):
    """(min |pn - 1.0|, min |pn - 1.2|) over the section mid-points, in float64."""
    o, d, z, sd = (I[k].double() for k in ("o", "d", "z", "sample_dist"))
    mid = z + torch.cat([z[:, 1:] - z[:, :-1], sd], -1) * 0.5
    pn = (o[:, None] + d[:, None] * mid[..., None]).norm(dim=-1)
    return float((pn - 1.0).abs().min()), float((pn - 1.2).abs().min())


FWD_KEYS = ("color", "color_sphere", "color_bg", "weights", "weights_sum", "weights_max", "cdf", "inside", "depth", "normals",
            "mid_z", "dists", "eik_num", "eik_den", "bg_alpha")
ADJ_KEYS = ("sdf", "grad", "rgb", "inv_s", "density", "bg_rgb")


def fwd_floor(k):
    return FLOOR_EIK_DEN if k == "eik_den" else FLOOR_FWD


def comp_reference_on(I, c, dtype):
    """O.composite + O.bg_alpha_from_density with autograd in `dtype` -> (forward {name: tensor}, adjoints {name: tensor});
    names are the kernel's (rayops.CompositeCtx), `inv_s` adjoint summed over rays; absent outputs are absent."""
    t = lambda x: x.to(dtype) if x is not None else None  # noqa: E731
    leaf = {k: I[k].to(dtype).requires_grad_(True) for k in ("sdf", "grad", "rgb", "inv_s")}
    bg_alpha = None
    if c.with_bg:
        leaf["density"] = I["density"].to(dtype).requires_grad_(True)
        leaf["bg_rgb"] = I["bg_rgb"].to(dtype).requires_grad_(True)
        bg_alpha = O.bg_alpha_from_density(leaf["density"], t(I["z_feed"]), t(I["sample_dist"]))
    ref = O.composite(dict(trim_sphere=c.trim), t(I["o"]), t(I["d"]), t(I["z"]), t(I["sample_dist"]), leaf["rgb"], leaf["inv_s"],
                      leaf["sdf"], leaf["grad"], c.cos, bg_alpha, leaf.get("bg_rgb"), t(I["background_rgb"]))
    fwd = dict(color=ref["color"], color_sphere=ref["color_sphere"], weights=ref["weights"], weights_sum=ref["weights_sum"][:, 0],
               weights_max=ref["weights"].max(-1)[0], cdf=ref["cdf"], inside=ref["inside_sphere"], depth=ref["depth"],
               normals=ref["normals"], mid_z=ref["mid_z_vals"], dists=ref["dists"], eik_num=ref["eik_num"], eik_den=ref["eik_den"])
    if c.with_bg:
        fwd["color_bg"] = ref["color_bg"]
        fwd["bg_alpha"] = bg_alpha
    ct = I["cot"]
    loss = (ref["color"] * t(ct["d_color"])).sum() + (ref["weights_sum"][:, 0] * t(ct["d_weights_sum"])).sum()
    if ct["d_depth"] is not None:
        loss = loss + (ref["depth"] * t(ct["d_depth"])).sum()
    if ct["d_eik_num"] is not None:
        loss = loss + (ref["eik_num"] * t(ct["d_eik_num"])).sum()
    names = list(leaf)
    adj = dict(zip(names, torch.autograd.grad(loss, [leaf[k] for k in names])))
    return {k: v.detach() for k, v in fwd.items()}, adj


@functools.lru_cache(maxsize=None)
def comp_reference(c):
    """-> (fwd64, adj64, fwd32, adj32) of a case: computed once, shared, left unchanged."""
    I = comp_case_inputs(c)
    return comp_reference_on(I, c, torch.float64) + comp_reference_on(I, c, torch.float32)


def comp_restatement_adjoints_scaled(c, scale):
    """The fp32 restatement's adjoints with every upstream cotangent multiplied by `scale`."""
    I = dict(comp_case_inputs(c))
    I["cot"] = {k: (v * scale if v is not None else None) for k, v in I["cot"].items()}
    return comp_reference_on(I, c, torch.float32)[1]


def comp_restatement_errors(c):
    """{("fwd" | "adj", name): rel err of the fp32 restatement against float64}."""
    f64, a64, f32, a32 = comp_reference(c)
    e = {("fwd", k): rel_err(f32[k], f64[k]) for k in f64}
    e.update({("adj", k): rel_err(a32[k], a64[k]) for k in a64})
    return e


def slice_rays(I, r0, r1):
    """The same case restricted to rays [r0, r1) (ray independence: a ray run alone)."""
    out = {}
    for k, v in I.items():
        if k == "cot":
            out[k] = {n: (t[r0:r1] if t is not None else None) for n, t in v.items()}
        elif k in ("inv_s", "background_rgb") or v is None:
            out[k] = v
        else:
            out[k] = v[r0:r1]
    return out


# --------------------------------------------------------------------------------------------------------------------
# upsample
# --------------------------------------------------------------------------------------------------------------------
UPSAMPLE_R = 41
# (n, n_new, inv_s); n >= 512 runs on the large-ray instantiation
UPSAMPLE_SHAPES = [(3, 5, 64.0), (511, 128, 512.0), (2, 1, 512.0), (2, 8, 512.0), (64, 65, 512.0), (65, 64, 1024.0),
                   (129, 128, 2048.0), (512, 128, 1024.0), (1087, 128, 4096.0), (1024, 1, 512.0)]
UPSAMPLE_INDEP = [(65, 64, 1024.0), (1087, 128, 4096.0)]


@functools.lru_cache(maxsize=None)
def upsample_case(n, n_new, inv_s, R=UPSAMPLE_R):
    """The generator of test_upsample_vs_oracle (seed = n) -> dict(o, d, z, sdf, ref64, ref32, excluded [R] bool, zmax)."""
    rays, _, _, _ = synth_rays(R, 3, 10)
    o, d = rays[:, 0:3], rays[:, 3:6]
    g = torch.Generator().manual_seed(n)
    z = torch.sort(1.0 + 2.0 * torch.rand(R, n, generator=g), -1)[0]
    pts = o[:, None] + d[:, None] * z[..., None]
    sdf = pts.norm(dim=-1) - 0.5 + 0.02 * torch.randn(R, n, generator=g)
    ref64 = O.up_sample(o.double(), d.double(), z.double(), sdf.double(), n_new, inv_s)
    ref32 = O.up_sample(o, d, z, sdf, n_new, inv_s)
    zmax = float(ref64.abs().max())
    # sample_pdf switches its denominator at 1e-5: isolated rays are discontinuous.  Decided by the two references alone.
    excluded = (ref32.double() - ref64).abs().amax(-1) > UPSAMPLE_EXCLUDE * zmax
    return dict(o=o, d=d, z=z, sdf=sdf, ref64=ref64, ref32=ref32, excluded=excluded, zmax=zmax)


def upsample_err(got, U):
    """Worst per-ray error against float64 over the rays kept, as a fraction of max |z|."""
    keep = ~U["excluded"]
    return float((got.double() - U["ref64"]).abs().amax(-1)[keep].max() / U["zmax"])


# --------------------------------------------------------------------------------------------------------------------
# sample_coarse / boundary
# --------------------------------------------------------------------------------------------------------------------
COARSE_N = [1, 2, 63, 64, 65, 128, 512, 513, 1088]
COARSE_OUT = [0, 1, 4, 32, 65]
COARSE_R = [1, 5]


@functools.lru_cache(maxsize=None)
def coarse_case(R, n, n_out, perturb, window=False):
    """-> dict(near, far, s_near, s_far, rs, ro, ref64, ref32); ref* = (z, z_out or None, sample_dist) of O.sparse_sampler."""
    g = torch.Generator().manual_seed(1000 * n + 10 * n_out + R)
    rays, _, _, _ = synth_rays(R, 4, 10)
    near, far = rays[:, 6:7], rays[:, 7:8] + 0.3 * torch.rand(R, 1, generator=g)
    rs = torch.rand(R, 1, generator=g) if perturb else None
    ro = torch.rand(R, n_out, generator=g) if perturb else None
    s_near, s_far = near, far
    if window:  # the fine-octree case: z from the window, z_out from the ray's far
        s_near = near + 0.2 + 0.1 * torch.rand(R, 1, generator=g)
        s_far = far - 0.3 - 0.1 * torch.rand(R, 1, generator=g)
    cfg = dict(n_samples=n, n_importance=0, n_outside=n_out, up_sample_steps=1, s_val_base=0, render_bg=True)
    refs = []
    for dt in (torch.float64, torch.float32):
        t = lambda x: x.to(dt) if x is not None else None  # noqa: E731
        refs.append(O.sparse_sampler({}, cfg, rays[:, 0:3].to(dt), rays[:, 3:6].to(dt), t(near), t(far), t(rs), t(ro),
                                     window=(t(s_near), t(s_far)) if window else None))
    return dict(near=near, far=far, s_near=s_near, s_far=s_far, rs=rs, ro=ro, ref64=refs[0], ref32=refs[1])


BOUNDARY_NB = [1, 2, 5, 10, 65, 130]
BOUNDARY_N = [24, 600]


@functools.lru_cache(maxsize=None)
def boundary_case(n, nb, R=5):
    g = torch.Generator().manual_seed(100 * n + nb)
    near = 0.5 + 0.3 * torch.rand(R, 1, generator=g)
    far = 4.0 + torch.rand(R, 1, generator=g)
    z = torch.sort(1.0 + 2.0 * torch.rand(R, n, generator=g), -1)[0]
    ref64 = O.boundary_samples(near.double(), far.double(), z.double(), nb)
    ref32 = O.boundary_samples(near, far, z, nb)
    return dict(near=near, far=far, z=z, ref64=ref64, ref32=ref32)


# --------------------------------------------------------------------------------------------------------------------
# sort_merge
# --------------------------------------------------------------------------------------------------------------------
MERGE_SHAPES = [(1, 0), (0, 1), (32, 32), (64, 1), (448, 64), (509, 4), (1056, 32), (1, 1087)]
MERGE_INDEP = [(61, 4), (1056, 32)]


@functools.lru_cache(maxsize=None)
def merge_case(na, nb, R=5):
    """a sorted, b unsorted; half of all entries are quantised to 1/8, so there are ties within each operand and across them;
    values of both signs -> dict(a, b, pa, pb, ref, ref_payload) with the stable torch.sort as the reference."""
    g = torch.Generator().manual_seed(10000 * na + nb)

    def draw(n):
        v = torch.randn(R, n, generator=g)
        return torch.where(torch.rand(R, n, generator=g) < 0.5, torch.round(v * 8) / 8, v)

    a = torch.sort(draw(na), -1)[0]
    b = draw(nb)
    if na > 5 and nb > 0:
        b[:, 0] = a[:, 5]  # a tie across the operands on every ray
    pa, pb = torch.rand(R, na, generator=g), torch.rand(R, nb, generator=g)
    ref, idx = torch.sort(torch.cat([a, b], -1), dim=-1, stable=True)
    return dict(a=a, b=b, pa=pa, pb=pb, ref=ref, ref_payload=torch.gather(torch.cat([pa, pb], -1), 1, idx))
