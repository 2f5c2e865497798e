"""numpy restatement of the surface-cloud fusion contract (include/neuconw_hip.h: QUANTISE, ACCUMULATE, RESOLVE): float64, every
operation rounded on its own, np.unique + np.add.at for the table.  The yardstick of tests/test_gpu_fuse.py and
tests/test_gpu_surfcloud.py: keys, table and outputs are compared BIT FOR BIT."""
import numpy as np

ACC = 10  # count, sum qpos [3], sum qn [3], sum qc [3]


def make_grid(lo, h, dims, scale=1.0, off=(0.0, 0.0, 0.0), cos_min=None):
    return {"lo": np.asarray(lo, dtype=np.float64).reshape(3), "h": np.float64(h),
            "dims": np.asarray(dims, dtype=np.int64).reshape(3), "scale": np.float64(scale),
            "off": np.asarray(off, dtype=np.float64).reshape(3), "cos_min": None if cos_min is None else np.float64(cos_min)}


def grid_of(lo, hi, cell, scale=1.0, offset=0.0, cos_min=None):
    """The grid surfcloud.SurfaceCloud(lo, hi, cell, scale, offset, cos_min) builds: dims = max(1, ceil((hi - lo) / cell))."""
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64).reshape(-1), (3,))
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64).reshape(-1), (3,))
    off = np.broadcast_to(np.asarray(offset, dtype=np.float64).reshape(-1), (3,))
    dims = np.maximum(1, np.ceil((hi - lo) / np.float64(cell))).astype(np.int64)
    return make_grid(lo, cell, dims, scale, off, cos_min)


def quantise(p, n, d, c, grid):
    """keys [m] int64 (-1 = invalid) and payload [m, 10] int64 (rows of invalid samples are 0) of m samples (float32 arrays)."""
    p, n, d, c = (np.asarray(a, dtype=np.float32).reshape(-1, 3) for a in (p, n, d, c))
    lo, h, dims = grid["lo"], grid["h"], grid["dims"]
    with np.errstate(all="ignore"):
        x = p.astype(np.float64) * grid["scale"] + grid["off"]
        g = (x - lo) / h
        cf = np.floor(g)
        ok = np.isfinite(p).all(1) & np.isfinite(n).all(1) & np.isfinite(d).all(1)
        ok &= ((cf >= 0.0) & (cf < dims.astype(np.float64))).all(1)
        n64, d64 = n.astype(np.float64), d.astype(np.float64)
        nn = (n64[:, 0] * n64[:, 0] + n64[:, 1] * n64[:, 1]) + n64[:, 2] * n64[:, 2]
        ok &= np.isfinite(nn) & (nn > 0.0)
        ln = np.sqrt(nn)
        if grid["cos_min"] is not None:
            facing = -((n64[:, 0] * d64[:, 0] + n64[:, 1] * d64[:, 1]) + n64[:, 2] * d64[:, 2])
            ok &= facing >= grid["cos_min"] * ln
        cell = np.where(ok[:, None], cf, 0.0).astype(np.int64)
        keys = np.where(ok, (cell[:, 2] * dims[1] + cell[:, 1]) * dims[0] + cell[:, 0], -1).astype(np.int64)
        pay = np.zeros((p.shape[0], ACC), dtype=np.int64)
        pay[:, 0] = 1
        q = np.floor((g - cf) * 65536.0)
        pay[:, 1:4] = np.where(ok[:, None], np.minimum(q, 65535.0), 0.0).astype(np.int64)
        qn = np.rint(n64 / ln[:, None] * 32767.0)  # ties to even
        pay[:, 4:7] = np.where(ok[:, None], qn, 0.0).astype(np.int64)
        c64 = c.astype(np.float64)
        c64 = np.where(c64 > 0.0, c64, 0.0)  # NaN -> 0
        c64 = np.where(c64 < 1.0, c64, 1.0)
        pay[:, 7:10] = np.rint(c64 * 255.0).astype(np.int64)
        pay[~ok] = 0
    return keys, pay


def accumulate(batches, grid):
    """The table of `batches` = [(p, n, d, c, serial), ...]: keys [C] int64 ascending, acc [C, 10] int64, views [C] int32 (the
    number of distinct serials per key) and the number of valid samples."""
    ks, ps, ss = [np.zeros(0, np.int64)], [np.zeros((0, ACC), np.int64)], [np.zeros(0, np.int64)]
    for p, n, d, c, serial in batches:
        k, pay = quantise(p, n, d, c, grid)
        ks.append(k[k >= 0])
        ps.append(pay[k >= 0])
        ss.append(np.full(int((k >= 0).sum()), serial, dtype=np.int64))
    k, pay, s = np.concatenate(ks), np.concatenate(ps), np.concatenate(ss)
    keys, inv = np.unique(k, return_inverse=True)
    acc = np.zeros((keys.shape[0], ACC), dtype=np.int64)
    np.add.at(acc, inv.reshape(-1), pay)
    pairs = np.unique(np.stack([k, s], 1), axis=0) if k.size else np.zeros((0, 2), np.int64)
    views = np.zeros(keys.shape[0], dtype=np.int32)
    np.add.at(views, np.searchsorted(keys, pairs[:, 0]), 1)
    return {"keys": keys, "acc": acc, "views": views, "valid": int(k.shape[0])}


def cells_of(keys, grid):
    dims = grid["dims"]
    return np.stack([keys % dims[0], (keys // dims[0]) % dims[1], keys // dims[0] // dims[1]], 1)


def resolve(table, grid, min_views=1, min_count=1):
    """RESOLVE + the filters of SurfaceCloud.finish, in ascending key."""
    keys, acc, views = table["keys"], table["acc"], table["views"]
    cnt = acc[:, 0]
    cell = cells_of(keys, grid).astype(np.float64)
    with np.errstate(all="ignore"):
        m = (acc[:, 1:4].astype(np.float64) / cnt.astype(np.float64)[:, None] + 0.5) / 65536.0
        pos = grid["lo"] + (cell + m) * grid["h"]
        N = acc[:, 4:7].astype(np.float64)
        ln = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        deg = ~(ln > 0.0)
        normal = np.where(deg[:, None], 0.0, N / ln[:, None]).astype(np.float32)
    colour = ((2 * acc[:, 7:10] + cnt[:, None]) // (2 * cnt[:, None])).astype(np.uint8)
    keep = (views >= min_views) & (cnt >= min_count) & ~deg
    return {"positions": pos[keep], "normals": normal[keep], "colours": colour[keep], "count": cnt[keep], "views": views[keep],
            "keys": keys[keep], "cells": int(keys.shape[0]), "degenerate": int(deg.sum())}


def inside_cells(pos, keys, grid):
    """True iff every position lies strictly inside the cell of its key: lo + cell h < pos < lo + (cell + 1) h per axis."""
    cell = cells_of(keys, grid).astype(np.float64)
    a = grid["lo"] + cell * grid["h"]
    b = grid["lo"] + (cell + 1.0) * grid["h"]
    return bool(((pos > a) & (pos < b)).all())
