"""The cases of tests/test_gpu_rays_edges.py, checked on the references alone (no GPU): the guard band round the discontinuous
sphere masks, the cap on rays an upsample comparison may leave out, finite float64 references, and the error of the fp32
restatement against float64 -- the figure the kernels' bound is derived from (tests/_ray_cases.py: bound).  Run with -s to see
each case's figures."""
import pytest
import torch

from tests import _ray_cases as C
from tests._util import rel_err


def test_generator_unchanged_with_switches_off():
    """The value switches are applied after the random stream is drawn: with all of them off the inputs are those
    tests/test_gpu_rays.py has always used; with them on, only the documented entries differ."""
    a = C.comp_inputs(5, 61, 4, 68)
    b = C.comp_inputs(5, 61, 4, 68, True, 403.0, True, True, True, True)
    assert float(a["inv_s"]) == 20.0 and float(b["inv_s"]) == 403.0
    for k in ("d", "z", "sample_dist", "rgb", "z_feed", "bg_rgb"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["o"][[0, 2, 3, 4]], b["o"][[0, 2, 3, 4]]) and float(b["o"][1, 0] - a["o"][1, 0]) == pytest.approx(3.0)
    assert bool((b["grad"][:, 30] == 0).all()) and torch.equal(a["grad"][:, :30], b["grad"][:, :30])
    assert bool((b["sdf"][2] == -0.5).all()) and torch.equal(a["sdf"][[0, 1, 3, 4]], b["sdf"][[0, 1, 3, 4]])
    assert bool((b["density"][:, 1::5] == 25).all()) and bool((b["density"][:, 3::5] == -25).all())
    assert torch.equal(a["density"][:, 0::5], b["density"][:, 0::5])


@pytest.mark.parametrize("c", C.all_comp_cases(), ids=C.case_id)
def test_comp_case_conditions(c):
    I = C.comp_case_inputs(c)
    d10, d12 = C.guard_distance(I)
    f64, a64, f32, a32 = C.comp_reference(c)
    errs = C.comp_restatement_errors(c)
    print("\n%s seed %d: guard band %.1e / %.1e; fp32 restatement: %s" % (
        C.case_id(c), c.seed, d10, d12, " ".join("%s.%s %.1e" % (k[0], k[1], v) for k, v in errs.items())))
    assert d10 > C.GUARD_BAND and d12 > C.GUARD_BAND, (d10, d12)
    for name, t in list(f64.items()) + list(a64.items()):
        assert bool(torch.isfinite(t).all()), name
    assert set(f64) == set(C.FWD_KEYS) - (set() if c.with_bg else {"color_bg", "bg_alpha"})
    assert set(a64) == set(C.ADJ_KEYS) - (set() if c.with_bg else {"density", "bg_rgb"})
    # the restatement is the reference's own arithmetic: it agrees with float64 on the masks exactly
    assert torch.equal(f32["inside"].double(), f64["inside"]) and torch.equal(f32["eik_den"].double(), f64["eik_den"])
    # where fp32 itself cannot resolve a quantity, 4 x its error bounds nothing: that happens in the adjoints of sdf / grad / inv_s
    # (saturated sigmoids at S <= 2 or inv_s = 3000, d_inv_s as a cancelling sum) and, at S = 1, in depth = one alpha of 1e-5 size
    loose = sorted(k for k, v in errs.items() if v > 1e-3)
    if loose:
        print("  fp32 cannot resolve:", loose)
    assert all((k[0] == "adj" and k[1] in ("sdf", "grad", "inv_s")) or (k == ("fwd", "depth") and c.S == 1) for k in loose), loose
    if c.values:  # the switches do what they are for
        assert float(f64["inside"][1].sum()) == 0 and float(f64["eik_den"][1]) == 0 and float(f64["weights_sum"][1]) == 0
        assert bool((I["density"] > 20).any()) and bool((I["density"] < -20).any())
        assert bool((I["grad"][:, c.S // 2] == 0).all())
        if c.inv_s == 3000.0:
            assert bool((f64["cdf"][2] == 0).all())  # both sigmoids underflow, float64 included
    else:
        assert float(f64["inside"].sum(-1).min()) > 0 or c.S < 8


@pytest.mark.parametrize("c", C.scale_cases(), ids=C.case_id)
def test_scale_cases_scale_exactly_in_fp32(c):
    """The grad_scale test asks for adjoints that are bit for bit 2 x the unscaled ones.  That can hold only where no fp32
    intermediate is subnormal; decided here on the fp32 restatement: its adjoints scale exactly on the cases the GPU test uses
    (smallest weight ~1e-10), and do not with the value switches on at S = 509 (weights down to 1e-45 on the sdf = -0.5 ray)."""
    a1, a2 = C.comp_reference(c)[3], C.comp_restatement_adjoints_scaled(c, 2.0)
    for k in a1:
        assert torch.equal(a2[k], 2.0 * a1[k]), k
    w = C.comp_reference(c)[2]["weights"]
    print("\n%s: smallest fp32 weight %.1e" % (C.case_id(c), float(w.min())))
    assert float(w.min()) > 1e-20
    if c.S == 509:
        cv = C.comp_case(c.S, c.O, values=True)
        b1, b2 = C.comp_reference(cv)[3], C.comp_restatement_adjoints_scaled(cv, 2.0)
        off = (b2["sdf"] != 2.0 * b1["sdf"])
        assert bool(off.any()) and bool(off[[0, 1, 3, 4]].sum() == 0) and float(b1["sdf"][off].abs().max()) < 1e-30


def test_weights_max_lies_in_an_outside_column_somewhere():
    """weights_max is taken over all M = S + O columns: only a case whose largest weight sits in an outside column can tell that
    from a maximum over the S primary ones.  One such case per object."""
    for shapes in (C.SHAPES_STD, C.SHAPES_BIG):
        hit = []
        for S, O_ in shapes:
            w = C.comp_reference(C.comp_case(S, O_))[0]["weights"]
            if O_ > 0 and bool((w[:, S:].amax(-1) > 1.01 * w[:, :S].amax(-1)).any()):
                hit.append((S, O_))
        assert hit, shapes


def test_trim_sphere_changes_only_color_bg():
    """On the reference: trim_sphere = False differs from True in color_bg and in nothing else (what the GPU test asks bit for bit)."""
    for S, O_ in C.OPTION_SHAPES:
        t, f = C.comp_reference(C.comp_case(S, O_, trim=True))[0], C.comp_reference(C.comp_case(S, O_, trim=False))[0]
        assert rel_err(f["color_bg"], t["color_bg"]) > 1e-2
        assert all(torch.equal(t[k], f[k]) for k in t if k != "color_bg")


@pytest.mark.parametrize("n,n_new,inv_s", C.UPSAMPLE_SHAPES)
def test_upsample_case_conditions(n, n_new, inv_s):
    U = C.upsample_case(n, n_new, inv_s)
    R = U["z"].shape[0]
    n_ex = int(U["excluded"].sum())
    e32 = C.upsample_err(U["ref32"], U)
    print("\nupsample (%d, %d, %g): %d of %d rays excluded; fp32 restatement on the rest %.1e" % (n, n_new, inv_s, n_ex, R, e32))
    assert R >= 41 and n_ex <= C.UPSAMPLE_CAP * R, n_ex
    assert bool(torch.isfinite(U["ref64"]).all())
    assert e32 <= C.UPSAMPLE_EXCLUDE  # by construction of the exclusion
    assert bool((U["ref64"][:, 1:] >= U["ref64"][:, :-1]).all())


def test_coarse_and_boundary_references():
    worst = 0.0
    for n in C.COARSE_N:
        for no in C.COARSE_OUT:
            for perturb in (False, True):
                for R in C.COARSE_R:
                    K = C.coarse_case(R, n, no, perturb)
                    for a, b in zip(K["ref32"], K["ref64"]):
                        assert (a is None) == (b is None)
                        if b is not None:
                            assert bool(torch.isfinite(b).all())
                            worst = max(worst, rel_err(a, b))
                    assert (K["ref64"][1] is None) == (no == 0)
    K = C.coarse_case(5, 65, 4, True, window=True)
    assert not torch.equal(K["s_near"], K["near"]) and not torch.equal(K["s_far"], K["far"])
    z, zo, sd = K["ref64"]
    assert rel_err(sd, (K["s_far"] - K["s_near"]).double() / 65) < 1e-12  # z comes from the window ...
    assert float(zo.min()) > float(K["far"].min())  # ... z_out from the ray's far
    worst_b = 0.0
    for n in C.BOUNDARY_N:
        for nb in C.BOUNDARY_NB:
            B = C.boundary_case(n, nb)
            assert B["ref64"].shape == (5, nb) and bool(torch.isfinite(B["ref64"]).all())
            worst_b = max(worst_b, rel_err(B["ref32"], B["ref64"]))
    print("\nfp32 restatement: sample_coarse %.1e, boundary %.1e" % (worst, worst_b))
    assert worst < C.FLOOR_SAMPLE and worst_b < C.FLOOR_SAMPLE


def test_sparse_sampler_window_is_the_fine_octree_path():
    """window=(s_near, s_far) with boundary_samples takes the same lines as a fine octree: the boundary samples of
    O.boundary_samples, merged and sorted; without a window nothing changes."""
    from oracle import neuconw_oracle as O

    K = C.coarse_case(5, 65, 4, False, window=True)
    cfg = dict(n_samples=65, n_importance=0, n_outside=4, up_sample_steps=1, s_val_base=0, render_bg=True, boundary_samples=10)
    o = torch.zeros(5, 3)
    z0, zo0, sd0 = O.sparse_sampler({}, dict(cfg, boundary_samples=0), o, o, K["near"], K["far"], window=(K["s_near"], K["s_far"]))
    z1, zo1, sd1 = O.sparse_sampler({}, cfg, o, o, K["near"], K["far"], window=(K["s_near"], K["s_far"]))
    assert z1.shape == (5, 75) and torch.equal(zo0, zo1) and torch.equal(sd0, sd1)
    assert torch.equal(z1, torch.sort(torch.cat([O.boundary_samples(K["near"], K["far"], z0, 10), z0], -1), -1)[0])
    z2, _, _ = O.sparse_sampler({}, cfg, o, o, K["near"], K["far"])  # no fine octree, no window: no boundary samples (:549)
    assert z2.shape == (5, 65)


def test_merge_cases_cover_ties_and_signs():
    for na, nb in C.MERGE_SHAPES + C.MERGE_INDEP:
        M = C.merge_case(na, nb)
        assert M["ref"].shape == (5, na + nb)
        if na >= 32 and nb >= 4:
            cat = torch.cat([M["a"], M["b"]], -1)
            assert bool((M["a"][:, 1:] == M["a"][:, :-1]).any()), "ties within a"
            assert bool((M["b"][:, :, None] == M["a"][:, None, :]).any()), "ties across"
            assert float(cat.min()) < 0 < float(cat.max())
            assert not bool((M["b"][:, 1:] >= M["b"][:, :-1]).all()), "b is unsorted"
