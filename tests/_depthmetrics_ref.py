"""numpy restatement of the contract of neuralrecon_w_amd.depthmetrics (include/neuconw_hip.h "Depth and normal maps against
ground truth", csrc/ncw_depthmetrics.hip): the per-pixel float32 terms with every operation rounded once, the classes, the two
bin rules, and the float64 sums IN THE HEADER'S ORDER (lane-sequential `cumsum`, never `np.sum`, whose pairwise order is
another contract; lane tree and fold = tests/_align_ref.py's, which the header cites word for word).  `plain` evaluates the same
per-pixel terms and adds them in plain float64 / exact integer arithmetic: the yardstick of tests/test_depthmetrics_host.py.
TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np
import torch

from tests import _view_ref as VR
from tests._align_ref import _seq, _tree

LANES, BLOCK, NSUMS, NCOUNTS, FIXED, MAX_EDGES = 256, 2048, 6, 12, 18, 2048   # NCW_DM_*
PRED_Z, PRED_T = 0, 1
SUMS = ("sum_abs", "sum_err", "sum_sq", "sum_rel", "sum_sq_rel", "sum_cos")
COUNTS = ("both", "gt_only", "pred_only", "neither", "masked", "delta1", "delta2", "delta3", "normals", "ang1", "ang2", "ang3")
f32 = np.float32


def thresholds():
    """(delta_thr [3], cos_thr [3]) float32, as depthmetrics.make_tables rounds them."""
    return (np.array([1.25, 1.25 ** 2, 1.25 ** 3], dtype=np.float32),
            np.array([math.cos(math.radians(a)) for a in (11.25, 22.5, 30.0)], dtype=np.float32))


def ray_norm(K, c2w, H, W):
    """nrm [H*W] float32 of ncw_raymath.h's view_ray_dir, every operation rounded once: the directions are tests/_view_ref.py's
    (float32 torch, elementwise), the product with c2w[:, :3] and the norm are written out in the kernel's order."""
    K = np.asarray(K, dtype=np.float32).reshape(3, 3)
    c = np.asarray(c2w, dtype=np.float32).reshape(3, 4)
    d = VR.ray_directions(H, W, K, torch.float32).numpy().reshape(-1, 3)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    w = [(dx * c[k, 0] + dy * c[k, 1]) + dz * c[k, 2] for k in range(3)]
    return np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]).astype(np.float32)


def per_pixel(gt_z, pred, gt_n=None, pred_n=None, mask=None, mode=PRED_Z, nrm=None, scale=1.0, cos_edges=None, rel_edges=None,
              delta_thr=None, cos_thr=None):
    """Rules 1-6 for n pixels (flat arrays; normals [3, n]).  Returns a dict of per-pixel arrays: the class flags, the float32 terms
    (0 where the pixel takes no part), the bins (-1 there), the flags of the threshold counts and the three planes."""
    dt, ct = thresholds()
    delta_thr = dt if delta_thr is None else np.asarray(delta_thr, dtype=f32)
    cos_thr = ct if cos_thr is None else np.asarray(cos_thr, dtype=f32)
    cos_edges, rel_edges = np.asarray(cos_edges, dtype=f32), np.asarray(rel_edges, dtype=f32)
    zg = np.asarray(gt_z, dtype=f32).reshape(-1)
    pv = np.asarray(pred, dtype=f32).reshape(-1)
    n = zg.size
    masked = np.zeros(n, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    with np.errstate(all="ignore"):
        vg = np.isfinite(zg) & (zg > 0)
        if mode == PRED_T:
            zp = ((pv * f32(scale)) / np.asarray(nrm, dtype=f32).reshape(-1)).astype(f32)
            vp = np.isfinite(pv) & (pv > 0) & np.isfinite(zp) & (zp > 0)
        else:
            zp = pv
            vp = np.isfinite(pv) & (pv > 0)
        live = ~masked
        both = live & vg & vp
        o = {"masked": masked, "both": both, "gt_only": live & vg & ~vp, "pred_only": live & ~vg & vp, "neither": live & ~vg & ~vp}
        e = (zp - zg).astype(f32)
        a = np.abs(e)
        r = (a / zg).astype(f32)
        q1, q2 = (zp / zg).astype(f32), (zg / zp).astype(f32)
        q = np.where(q1 > q2, q1, q2)
        ee = (e * e).astype(f32)
        s = (ee / zg).astype(f32)
        z0 = f32(0)
        o["terms"] = np.stack([np.where(both, t, z0) for t in (a, e, ee, r, s)], 0)          # [5, n] float32
        for k in range(3):
            o["delta%d" % (k + 1)] = both & (q < delta_thr[k])
        o["bin_rel"] = np.where(both, np.searchsorted(rel_edges, r, side="right"), -1)        # the number of edges <= r
        scored = np.zeros(n, dtype=bool)
        c = np.full(n, np.nan, dtype=f32)
        if gt_n is not None and pred_n is not None:
            g = np.asarray(gt_n, dtype=f32).reshape(3, -1)
            p = np.asarray(pred_n, dtype=f32).reshape(3, -1)
            if mode == PRED_T:
                p = (f32(2) * p - f32(1)).astype(f32)
            fin = np.isfinite(g).all(0) & np.isfinite(p).all(0)
            scored = both & fin & (g != 0).any(0) & (p != 0).any(0)
            dot = ((g[0] * p[0] + g[1] * p[1]) + g[2] * p[2]).astype(f32)
            c = np.where(dot < -1, f32(-1), np.where(dot > 1, f32(1), dot)).astype(f32)
        o["normals"] = scored
        o["cos"] = np.where(scored, c, z0)
        for k in range(3):
            o["ang%d" % (k + 1)] = scored & (c >= cos_thr[k])
        # the number of edges > c over a DESCENDING table = the number of -edges < -c over the ascending one
        o["bin_cos"] = np.where(scored, np.searchsorted(-cos_edges, -np.where(scored, c, z0), side="left"), -1)
        nan = f32(np.nan)
        o["err_rel"] = np.where(both, r, nan).astype(f32)
        o["err_cos"] = np.where(scored, c, nan).astype(f32)
        o["z_pred"] = np.where(vp, zp, z0).astype(f32)
    return o


def _hists(o, nr, na):
    hr = np.bincount(o["bin_rel"][o["bin_rel"] >= 0], minlength=nr + 1).astype(np.int64)
    hc = np.bincount(o["bin_cos"][o["bin_cos"] >= 0], minlength=na + 1).astype(np.int64)
    return hr, hc


def ordered_sums(terms, dtype=np.float64):
    """[k, n] per-pixel terms (0 where a pixel takes no part: adding +0.0 leaves a partial sum unchanged, and no partial sum is
    -0.0) -> [k] sums in rule 7's order."""
    terms = np.asarray(terms).astype(dtype)
    k, n = terms.shape
    nb = (n + BLOCK - 1) // BLOCK
    pad = np.zeros((k, nb * BLOCK), dtype=dtype)
    pad[:, :n] = terms
    lanes = _seq(pad.reshape(k, nb, BLOCK // LANES, LANES), 2)                # [k, nb, 256]: ascending j per lane
    rows = _tree(lanes)                                                        # [k, nb]
    nr = max((nb + LANES - 1) // LANES, 1)
    padr = np.zeros((k, nr * LANES), dtype=dtype)
    padr[:, :nb] = rows
    return _tree(_seq(padr.reshape(k, nr, LANES), 1))                          # lane l: rows l, l + 256, ..


def row_from(o, nr, na, sums):
    hr, hc = _hists(o, nr, na)
    d = {k: float(sums[i]) for i, k in enumerate(SUMS)}
    d.update({k: int(o[k].sum()) for k in COUNTS})
    d["hist_rel"], d["hist_cos"] = hr, hc
    return d


def compare(gt_z, pred, cos_edges, rel_edges, **kw):
    """The row the kernel writes (dict: SUMS float, COUNTS int, hist_rel, hist_cos) and the three planes, bit for bit."""
    o = per_pixel(gt_z, pred, cos_edges=cos_edges, rel_edges=rel_edges, **kw)
    terms = np.concatenate([o["terms"], o["cos"][None]], 0)
    return row_from(o, len(rel_edges), len(cos_edges), ordered_sums(terms)), {k: o[k] for k in ("err_rel", "err_cos", "z_pred")}


def plain(gt_z, pred, cos_edges, rel_edges, **kw):
    """The same float32 per-pixel terms added in plain float64 (math.fsum: the exactly rounded sum), with Σ|term| per sum."""
    o = per_pixel(gt_z, pred, cos_edges=cos_edges, rel_edges=rel_edges, **kw)
    terms = np.concatenate([o["terms"], o["cos"][None]], 0).astype(np.float64)
    sums = [math.fsum(t.tolist()) for t in terms]
    mags = [math.fsum(np.abs(t).tolist()) for t in terms]
    return row_from(o, len(rel_edges), len(cos_edges), sums), mags, int(o["both"].sum())


def words(row, nr, na):
    """The row as the int64 words of the device table."""
    w = np.zeros(FIXED + nr + 1 + na + 1, dtype=np.int64)
    w[:NSUMS] = np.array([row[k] for k in SUMS], dtype=np.float64).view(np.int64)
    w[NSUMS:FIXED] = [row[k] for k in COUNTS]
    w[FIXED:FIXED + nr + 1] = row["hist_rel"]
    w[FIXED + nr + 1:] = row["hist_cos"]
    return w
