"""CPU-side checks: the C-ABI library loads and exports every symbol include/neuconw_hip.h declares,
the ctypes structs mirror the header, the drop-in modules expose the reference's state_dict keys,
and the product path refuses to run without a GPU (no CPU fallback)."""
import ctypes
import os
import re

import pytest
import torch

from tests._util import ROOT, load_golden


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "neuconw_hip.h")).read()
    return sorted(set(re.findall(r"^(?:int|int64_t|const char\*)\s+(ncw_\w+)\s*\(", src, flags=re.M)))


def test_library_exports_every_declared_symbol():
    from neuralrecon_w_amd import build, lib as L

    path = build.LIB
    if not os.path.isfile(path):
        build.build(verbose=False)
    cdll = ctypes.CDLL(path)
    declared = _header_symbols()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(cdll, name), "missing export: " + name
    assert sorted(L.exported_symbols()) == declared, "lib.py bindings out of sync with the header"
    assert cdll.ncw_abi_version() == L.ABI_VERSION


def test_library_is_built_from_this_tree(monkeypatch):
    """The shipped .so carries the sha256 of the sources it was built from; the binding recomputes it from csrc/ + include/
    and refuses a library built from anything else (a GPU box runs the PREBUILT library: this is what ties the kernels under
    test to the tree).  Also: a different hash is really refused."""
    from neuralrecon_w_amd import build, lib as L

    cdll = ctypes.CDLL(build.LIB)
    cdll.ncw_source_hash.restype = ctypes.c_char_p
    assert cdll.ncw_source_hash().decode() == build.source_hash(), "libneuconw_hip.so is stale: rebuild (__graft_entry__.build())"
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(build, "source_hash", lambda: "0" * 64)
    monkeypatch.delenv("NEUCONW_HIP_LIB", raising=False)
    with pytest.raises(L.NeuconwHipError, match="built from other sources"):
        L.get_lib()
    monkeypatch.undo()
    L.get_lib()  # the real tree loads


def test_probe_hooks_cannot_enter_the_product_build():
    """NCW_EXP_* timing hooks (scripts/probes/ncw_exp_hooks.h) compile only under NCW_BUILD_TAG (a probe library beside the
    product); csrc/ncw_common.h #errors on them otherwise and build.py refuses the flag."""
    import subprocess
    import sys

    env = dict(os.environ, NCW_EXTRA_HIPCC_FLAGS="-DNCW_EXP_NOLOAD")
    env.pop("NCW_BUILD_TAG", None)
    r = subprocess.run([sys.executable, "-c", "import neuralrecon_w_amd.build"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "NCW_BUILD_TAG" in r.stderr
    src = open(os.path.join(ROOT, "neuralrecon-w_amd", "csrc", "ncw_common.h")).read()
    assert "#error" in src and "NCW_PROBE_BUILD" in src


def test_struct_sizes_match_c_layout():
    """sizeof of every ctypes mirror equals what the C compiler lays out (checked with gcc)."""
    import subprocess
    import tempfile

    from neuralrecon_w_amd import lib as L

    names = ["NcwSeg", "NcwPackDesc", "NcwUnpackDesc", "NcwSdfNet", "NcwPoints", "NcwSdfStash", "NcwWgradDesc",
             "NcwColorNet", "NcwColorStash", "NcwNerfNet", "NcwNerfStash", "NcwCompositeIn", "NcwCompositeOut",
             "NcwCompositeGrad"]
    prog = '#include <stdio.h>\n#include "neuconw_hip.h"\nint main(){' + "".join(
        'printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in names) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe]).decode().split()
    sizes = dict(zip(out[0::2], map(int, out[1::2])))
    for n in names:
        assert ctypes.sizeof(getattr(L, n)) == sizes[n], (n, ctypes.sizeof(getattr(L, n)), sizes[n])


def test_state_dict_keys_match_reference_checkpoint_format():
    """Golden fixtures carry the real reference's state_dict: our modules must load it unchanged."""
    from tests._build import build_system, load_golden_weights

    sd, _, _, _ = load_golden("render_w64_det")
    emb, neuconw, nerf, _ = build_system(device="cpu")
    load_golden_weights(sd, emb, neuconw, nerf)
    ours = {"neuconw." + k for k in neuconw.state_dict()} | {"nerf." + k for k in nerf.state_dict()}
    theirs = {k for k in sd if not k.startswith("embedding_a")}
    assert theirs <= ours
    extra = ours - theirs
    assert all(k.startswith("neuconw.xyz_encoding_final") for k in extra), extra  # dropped from the fixtures
    # full-size checkpoint shape of the shipped config (84 tensors incl. embedding)
    import neuralrecon_w_amd as nw
    sdf_cfg = dict(d_in=3, d_out=513, d_hidden=512, n_layers=8, skip_in=(4,), multires=6, bias=0.5, scale=1,
                   geometric_init=True, weight_norm=True, inside_outside=False)
    color_cfg = dict(d_in=9, d_feature=512, mode="idr", d_out=3, d_hidden=256, n_layers=4, head_channels=128,
                     static_head_layers=2, weight_norm=True, multires_view=4)
    big = nw.NeuconW(sdf_cfg, color_cfg, dict(init_val=0.3), 48, True)
    bg = nw.NeRF(D=8, d_in=4, d_in_view=3, W=256, multires=10, multires_view=4, output_ch=4, skips=[4],
                 encode_appearance=True, in_channels_a=48, in_channels_dir=27, use_viewdirs=True)
    assert len(big.state_dict()) + len(bg.state_dict()) + 1 == 84
    assert sum(p.numel() for p in big.parameters()) == 2957627
    assert sum(p.numel() for p in bg.parameters()) == 698628
    assert big.sdf_net.lin3.weight_v.shape == (473, 512) and big.sdf_net.lin8.weight_v.shape == (513, 512)


def test_no_cpu_fallback():
    import neuralrecon_w_amd as nw
    from tests._build import build_system

    emb, neuconw, nerf, rdr = build_system(device="cpu")
    with pytest.raises(nw.NeuconwHipError):
        neuconw.sdf(torch.zeros(4, 3))
    with pytest.raises(nw.NeuconwHipError):
        rdr.render(torch.zeros(4, 10), torch.zeros(4, dtype=torch.long), torch.zeros(4, dtype=torch.long))


def _lo_pairs(net):
    """[(hi pointer, lo pointer, transposed)] of every residual field (`*_lo`) of a net struct with its hi field."""
    out = []
    for name, _ in net._fields_:
        if name.endswith("_lo"):
            hi, lo = getattr(net, name[:-3]), getattr(net, name)
            pairs = zip(hi, lo) if hasattr(lo, "__len__") else [(hi, lo)]
            out += [(h, l, name.startswith("wt")) for h, l in pairs]
    return out


def test_pack_plan_descriptors_cover_every_parameter():
    """Host logic of the pack plan, at every SDF width and precision: every Linear of the three networks is packed
    (forward + transposed) and has exactly one gradient-unpack descriptor per source row; every residual matrix a net struct
    points at (`*_lo`: the low halves of the fp16 hi + lo pairs) is packed by exactly one `residual` descriptor over the same
    rows / segments / orientation as its hi matrix, and the structs hold the residuals exactly where the split is on
    (fp16 only; SDF: W = 256 / 512, every layer forward, transposed too; colour: every layer forward; background: width 256)."""
    from neuralrecon_w_amd import lib as L
    from tests._build import build_system

    for W in (64, 256, 512):
        kw = {} if W == 64 else dict(color_hidden=256, head=128, nerf_w=256)
        emb, neuconw, nerf, _ = build_system(W=W, device="cpu", **kw)
        for prec in (L.PREC_F32, L.PREC_BF16, L.PREC_F16):
            for tag, mod in (("sdf", neuconw.sdf_net), ("color", neuconw.color_net), ("nerf", nerf)):
                plan = mod.plan(prec)
                packed = {p["weight"].data_ptr() for p in plan._pack}
                rows = {}
                for u in plan._unpack:
                    rows.setdefault(u["weight"].data_ptr(), 0)
                    rows[u["weight"].data_ptr()] += u["nrows"]
                for name, p in mod.named_parameters():
                    if p.dim() == 2 and not name.startswith("views_linears") and not name.endswith("weight_g"):
                        assert p.data_ptr() in packed, name
                        assert rows[p.data_ptr()] == p.shape[0], name
                by_ptr = {}
                for p in plan._pack:
                    by_ptr.setdefault(plan.mat_ptr(p["mat"]), []).append(p)
                pairs = _lo_pairs(plan.net)
                for hi, lo, transposed in pairs:
                    if lo:
                        assert hi and len(by_ptr[lo]) == 1 and len(by_ptr[hi]) == 1, (tag, prec)
                        d_lo, d_hi = by_ptr[lo][0], by_ptr[hi][0]
                        assert d_lo["residual"] and not d_hi["residual"] and d_lo["transpose"] == d_hi["transpose"] == transposed
                        assert d_lo["weight"] is d_hi["weight"] and d_lo["g"] is d_hi["g"] and d_lo["scale"] == d_hi["scale"]
                        assert (d_lo["row0"], d_lo["nrows"], d_lo["segs"]) == (d_hi["row0"], d_hi["nrows"], d_hi["segs"])
                        assert plan._mats[d_lo["mat"]][1:] == plan._mats[d_hi["mat"]][1:]
                n_res = sum(1 for p in plan._pack if p["residual"])
                assert n_res == sum(1 for _, lo, _ in pairs if lo), (tag, prec)  # no residual matrix that no struct field reads
                fwd = sum(1 for h, lo, t in pairs if lo and not t)
                bwd = sum(1 for h, lo, t in pairs if lo and t)
                n_mod = sum(1 for h, _, t in pairs if h and not t)  # Linears of the network (the SDF feature rows have no `_lo` field)
                split = prec == L.PREC_F16 and (tag == "color" or W in (256, 512))
                assert (fwd, bwd) == ((n_mod, n_mod if tag == "sdf" else 0) if split else (0, 0)), (tag, prec, fwd, bwd)


def test_same_seed_same_init_as_reference():
    """Constructing our modules consumes the RNG exactly like the reference: same seed -> same weights.  Against the live
    reference where its tree is present, else against the fingerprint of its weights in tests/golden/ref_checks.npz
    (per key: sum, sum of |x| and 16 values, tests/golden/make_golden_refchecks.py)."""
    import numpy as np

    import neuralrecon_w_amd as nw
    from oracle import ref_import
    from tests.golden.make_golden_refchecks import init_fingerprint

    sdf_cfg = dict(d_in=3, d_out=257, d_hidden=256, n_layers=8, skip_in=(4,), multires=6, bias=0.5, scale=1,
                   geometric_init=True, weight_norm=True, inside_outside=False)
    color_cfg = dict(d_in=9, d_feature=256, mode="idr", d_out=3, d_hidden=256, n_layers=4, head_channels=128,
                     static_head_layers=2, weight_norm=True, multires_view=4)
    live = ref_import.available()
    if live:
        ns = ref_import.load()
        torch.manual_seed(7)
        ref = ns.NeuconW(sdf_cfg, color_cfg, dict(init_val=0.3), 48, True)
        ref_bg = ns.NeRF(D=8, d_in=4, d_in_view=3, W=256, multires=10, multires_view=4, output_ch=4, skips=[4],
                         encode_appearance=True, in_channels_a=48, in_channels_dir=27, use_viewdirs=True)
    torch.manual_seed(7)
    ours = nw.NeuconW(sdf_cfg, color_cfg, dict(init_val=0.3), 48, True)
    ours_bg = nw.NeRF(D=8, d_in=4, d_in_view=3, W=256, multires=10, multires_view=4, output_ch=4, skips=[4],
                      encode_appearance=True, in_channels_a=48, in_channels_dir=27, use_viewdirs=True)
    if live:
        a, b = ref.state_dict(), ours.state_dict()
        assert list(a) == list(b)
        for k in a:
            assert torch.allclose(a[k], b[k], rtol=0, atol=1e-7), k
        a, b = ref_bg.state_dict(), ours_bg.state_dict()
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k
        return
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_checks.npz"))
    for tag, mod, atol in (("nc", ours, 1e-7), ("bg", ours_bg, 0.0)):  # the live bounds: allclose(atol 1e-7) / equal
        keys, s, a, pick = init_fingerprint(mod.state_dict())
        n = np.array([v.numel() for v in mod.state_dict().values()])
        assert list(keys) == list(g["init_%s_keys" % tag])
        assert np.abs(pick - g["init_%s_pick" % tag]).max() <= atol, tag
        # the sums carry every element: bounded by atol per element plus float64 summation order
        assert (np.abs(s - g["init_%s_sum" % tag]) <= atol * n + 1e-9 * (1 + np.abs(a))).all(), tag
        assert (np.abs(a - g["init_%s_abs" % tag]) <= atol * n + 1e-9 * (1 + np.abs(a))).all(), tag
