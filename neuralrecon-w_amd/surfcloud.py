"""One oriented, coloured surface cloud from many sphere-traced views (not in the reference).

    cloud = SurfaceCloud(lo, hi, cell, scale=radius, offset=origin, cos_min=0.1)    # the grid, in SfM coordinates
    fuse_views(rdr, [(camera, ts), ...], cloud)                                      # views.trace_view per view -> cloud.add
    out = cloud.finish(min_views=2)                                                  # positions / normals / colours / count / views / keys
    ply.write("surface_cloud.ply", out["positions"], rgb=out["colours"], normals=out["normals"])

Every HIT of a traced view lies on the zero level set to the tracer's eps, is seen by its camera by construction and carries
the SDF gradient and the colour network's answer.  The samples are quantised and accumulated per grid cell in an open-addressed
device table (`ncw_fuse_insert`, csrc/ncw_fuse.hip) -- integers only, so the table is a function of the multiset of samples,
bit for bit on every run -- and resolved to ONE point per occupied cell (`ncw_fuse_resolve`).  The table never holds the
samples: its size follows the occupied cells, not the views.  The contract is stated in include/neuconw_hip.h and restated in
numpy by tests/_fuse_ref.py.  Cell rule, filters and the appearance choice are this project's: no parity with open3d's
voxel_down_sample or any multi-view-stereo fusion is claimed.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import lib as L

DEFAULT_CAPACITY = 1 << 20  # table rows of a new cloud (96 bytes each); add() grows it
MAX_CAPACITY = 1 << 31      # rows add() refuses to grow beyond by default (192 GiB): a cell size far too small for the box


def _vec3(v, name):
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3 or not np.isfinite(a).all():
        raise ValueError("SurfaceCloud: %s must hold 1 or 3 finite values, got %r" % (name, v))
    return a


def _pow2_at_least(n):
    return 1 << max(0, int(n) - 1).bit_length()


class SurfaceCloud:
    """The accumulator of one surface cloud.  Grid: lo, hi [3] (or one value) and the cell size `cell` > 0 in the OUTPUT frame;
    dims_a = max(1, ceil((hi_a - lo_a) / cell)) cells per axis (at most 2^20), so the grid covers [lo, lo + dims cell), which
    contains [lo, hi).  A sample's point p (the network's unit-sphere frame) is taken to the output frame by x = p scale +
    offset: scale / offset = the scene's radius / origin give SfM coordinates, as scripts/extract_mesh.py writes its PLY.
    cos_min: a sample is kept iff the angle between its gradient and the direction back to the camera has cosine >= cos_min
    (None = no such test).  capacity: initial table rows (a power of two); max_capacity: the rows add() may grow to."""

    def __init__(self, lo, hi, cell, scale=1.0, offset=0, cos_min=None, device=None, capacity=DEFAULT_CAPACITY,
                 max_capacity=MAX_CAPACITY):
        self.lo, self.hi = _vec3(lo, "lo"), _vec3(hi, "hi")
        self.cell, self.scale = float(cell), float(scale)
        self.offset = _vec3(offset, "offset")
        if not (self.cell > 0 and math.isfinite(self.cell)):
            raise ValueError("SurfaceCloud: cell must be finite and > 0 (got %r)" % (cell,))
        if not math.isfinite(self.scale) or self.scale == 0:
            raise ValueError("SurfaceCloud: scale must be finite and not 0 (got %r)" % (scale,))
        if not (self.hi > self.lo).all():
            raise ValueError("SurfaceCloud: hi must exceed lo on every axis (got %r / %r)" % (lo, hi))
        if cos_min is not None and not (math.isfinite(float(cos_min)) and -1.0 <= float(cos_min) <= 1.0):
            raise ValueError("SurfaceCloud: cos_min must lie in [-1, 1] or be None (got %r)" % (cos_min,))
        self.cos_min = None if cos_min is None else float(cos_min)
        dims = np.maximum(1, np.ceil((self.hi - self.lo) / self.cell))
        if (dims > L.FUSE_MAX_DIM).any():
            raise ValueError("SurfaceCloud: %s cells per axis exceed 2^20: the cell size %g is too small for the box"
                             % (dims.astype(np.int64).tolist(), self.cell))
        self.dims = dims.astype(np.int64)
        for name, c in (("capacity", capacity), ("max_capacity", max_capacity)):
            if int(c) != c or c < 1 or c > L.FUSE_MAX_CAPACITY or (int(c) & (int(c) - 1)):
                raise ValueError("SurfaceCloud: %s must be a power of two in [1, 2^36] (got %r)" % (name, c))
        if capacity > max_capacity:
            raise ValueError("SurfaceCloud: capacity %d exceeds max_capacity %d" % (capacity, max_capacity))
        self.capacity, self.max_capacity = int(capacity), int(max_capacity)
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise L.NeuconwHipError("surfcloud.SurfaceCloud: device %s is not a GPU; the fusion has no CPU fallback" % self.device)
        self._grid = L.NcwFuseGrid((C.c_double * 3)(*self.lo), self.cell, (C.c_int64 * 3)(*[int(d) for d in self.dims]),
                                   self.scale, (C.c_double * 3)(*self.offset),
                                   0.0 if self.cos_min is None else self.cos_min, 0 if self.cos_min is None else 1, 0)
        self._table = None       # allocated by the first add(): constructing a cloud launches nothing
        self._bound = 0          # an upper bound on the occupied rows that needs no read-back
        self._last_view = -1
        self._offered = 0
        self._growths = 0
        self._launches = 0

    # -------------------------------------------------------------------------------------------
    def _alloc(self, capacity):
        dev = self.device
        return {"keys": torch.full((capacity,), L.FUSE_EMPTY, device=dev, dtype=torch.int64),
                "acc": torch.zeros(capacity, L.FUSE_ACC, device=dev, dtype=torch.int64),
                "stamp": torch.zeros(capacity, device=dev, dtype=torch.int32),
                "views": torch.zeros(capacity, device=dev, dtype=torch.int32),
                "counters": torch.zeros(L.FUSE_COUNTERS, device=dev, dtype=torch.int64),
                "capacity": capacity}

    @staticmethod
    def _struct(t):
        return L.NcwFuseTable(t["keys"].data_ptr(), t["acc"].data_ptr(), t["stamp"].data_ptr(), t["views"].data_ptr(),
                              t["counters"].data_ptr(), t["capacity"])

    def _counters(self):
        """(occupied, overflow, valid) read back from the device; a non-zero overflow counter is an error."""
        if self._table is None:
            return 0, 0, 0
        occ, over, valid, _ = self._table["counters"].tolist()
        if over != 0:
            raise L.NeuconwHipError("surfcloud: %d samples found no slot in the table (capacity %d): the cloud is incomplete"
                                    % (over, self.capacity))
        return occ, over, valid

    def _reserve(self, n):
        """Room for n more samples BEFORE they are inserted: the table stays at most half full, so the bounded probe loop of
        the kernel always ends at an EMPTY word.  The true occupied count is read back only when the bound asks for growth."""
        if self._table is None:
            self._table = self._alloc(self.capacity)
        if 2 * (self._bound + n) <= self.capacity:
            return
        self._bound = self._counters()[0]
        need = 2 * (self._bound + n)
        if need <= self.capacity:
            return
        capacity = _pow2_at_least(need)
        if capacity > self.max_capacity:
            raise L.NeuconwHipError("surfcloud: %d occupied cells + %d samples need a table of %d rows, more than max_capacity "
                                    "%d: nothing was inserted (choose a larger cell or a tighter box)"
                                    % (self._bound, n, capacity, self.max_capacity))
        new = self._alloc(capacity)
        L.check(L.get_lib().ncw_fuse_move(C.byref(self._struct(self._table)), C.byref(self._struct(new)),
                                          L.stream_ptr(self.device)), "ncw_fuse_move")
        new["counters"][2:3].copy_(self._table["counters"][2:3])  # the valid counter is carried; the move counted the rest
        self._table, self.capacity = new, capacity
        self._growths += 1
        self._launches += 1

    def add(self, points, grads, dirs, colours, view):
        """Adds n samples of the view with serial `view` (an integer that never decreases from call to call; the samples of
        one view may come in several calls): points / grads / dirs / colours [n, 3] float32 DEVICE tensors (module
        docstring).  One `ncw_fuse_insert` launch; nothing is read back unless the table has to grow."""
        names = ("points", "grads", "dirs", "colours")
        ts = (points, grads, dirs, colours)
        if int(view) != view or not 0 <= view <= L.FUSE_MAX_SERIAL:
            raise ValueError("SurfaceCloud.add: view must be an integer in [0, 2^31 - 2] (got %r)" % (view,))
        if view < self._last_view:
            raise ValueError("SurfaceCloud.add: view serials must not decrease (%d after %d): the distinct-view count "
                             "relies on it" % (view, self._last_view))
        for name, t in zip(names, ts):
            if not (torch.is_tensor(t) and t.is_cuda):
                raise L.NeuconwHipError("surfcloud.SurfaceCloud.add: %s is not a tensor on a GPU; the fusion has no CPU fallback"
                                        % name)
            if self.device.index is None:  # "cuda": the cloud lives where its first samples are
                self.device = t.device
            if t.device != self.device:
                raise ValueError("SurfaceCloud.add: %s is on %s, the cloud on %s" % (name, t.device, self.device))
        n = points.shape[0] if points.dim() == 2 else -1
        for name, t in zip(names, ts):
            if t.dim() != 2 or tuple(t.shape) != (n, 3):
                raise ValueError("SurfaceCloud.add: %s must be [n, 3], got %s" % (name, tuple(t.shape)))
        if n > 2 ** 31 - 1:
            raise ValueError("SurfaceCloud.add: at most 2^31 - 1 samples per call (got %d)" % n)
        self._last_view = int(view)
        if n == 0:
            return
        p, g, d, c = (t.detach().float().contiguous() for t in ts)
        self._reserve(n)
        L.check(L.get_lib().ncw_fuse_insert(L.ptr(p), L.ptr(g), L.ptr(d), L.ptr(c), n, int(view), C.byref(self._grid),
                                            C.byref(self._struct(self._table)), L.stream_ptr(self.device)), "ncw_fuse_insert")
        self._bound += n
        self._offered += n
        self._launches += 1

    def table(self):
        """The occupied rows in ascending key as device tensors: keys [C] int64, acc [C, 10] int64 (count, sum qpos, sum qn,
        sum qc), views [C] int32 -- what ACCUMULATE defines (WHERE a key sits in the table is not part of it)."""
        if self._table is None:
            e = torch.empty(0, device=self.device, dtype=torch.int64)
            return {"keys": e, "acc": e.reshape(0, L.FUSE_ACC), "views": e.int()}
        self._counters()
        rows = self._rows()
        return {"keys": self._table["keys"][rows], "acc": self._table["acc"][rows], "views": self._table["views"][rows]}

    def _rows(self):
        occ = torch.nonzero(self._table["keys"] >= 0).reshape(-1)
        order = torch.sort(self._table["keys"][occ], stable=True)[1]
        return occ[order].contiguous()

    def finish(self, min_views=1, min_count=1):
        """RESOLVE: a dict of device tensors over the cells with views >= min_views, count >= min_count and a non-zero
        normal sum, in ascending key: positions [C, 3] f64 (output frame), normals [C, 3] f32 (unit), colours [C, 3] uint8,
        count [C] int64, views [C] int32, keys [C] int64; and `cells` / `degenerate`: the occupied cells and how many of them
        had opposite normals cancel.  The cloud stays as it is: more views may be added and finish() called again."""
        dev = self.device
        self._counters()
        rows = self._rows() if self._table is not None else torch.empty(0, device=dev, dtype=torch.int64)
        n = rows.numel()
        out = {"positions": torch.empty(n, 3, device=dev, dtype=torch.float64),
               "normals": torch.empty(n, 3, device=dev, dtype=torch.float32),
               "colours": torch.empty(n, 3, device=dev, dtype=torch.uint8),
               "count": torch.empty(n, device=dev, dtype=torch.int64),
               "views": torch.empty(n, device=dev, dtype=torch.int32),
               "degenerate": torch.empty(n, device=dev, dtype=torch.uint8),
               "keys": torch.empty(n, device=dev, dtype=torch.int64)}
        if n:
            L.check(L.get_lib().ncw_fuse_resolve(C.byref(self._struct(self._table)), L.ptr(rows), n, C.byref(self._grid),
                                                 L.ptr(out["positions"]), L.ptr(out["normals"]), L.ptr(out["colours"]),
                                                 L.ptr(out["count"]), L.ptr(out["views"]), L.ptr(out["degenerate"]),
                                                 L.ptr(out["keys"]), L.stream_ptr(dev)), "ncw_fuse_resolve")
            self._launches += 1
        deg = out.pop("degenerate")
        keep = (out["views"] >= int(min_views)) & (out["count"] >= int(min_count)) & (deg == 0)
        res = {k: v[keep] for k, v in out.items()}
        res["cells"], res["degenerate"] = n, int(deg.sum())
        return res

    def stats(self):
        """Host numbers: samples offered / valid, occupied cells, capacity, table bytes, growths, overflow, launches."""
        occ, over, valid = self._counters()
        return {"offered": self._offered, "valid": valid, "invalid": self._offered - valid, "cells": occ,
                "capacity": self.capacity, "table_bytes": self.capacity * (8 + 8 * L.FUSE_ACC + 4 + 4), "growths": self._growths,
                "overflow": over, "launches": self._launches}


def mean_appearance(rdr):
    """The mean row of the appearance embedding [n_a] f32: the code `fuse_views(appearance="mean")` shades every view with."""
    return rdr.embeddings["a"].weight.detach().float().mean(0)


def fuse_views(rdr, cameras_and_ts, cloud, *, appearance="mean", chunk=None, on_view=None, **trace_kw):
    """Traces every view of `cameras_and_ts` (pairs (views.Camera, ts)) with views.trace_view and feeds the HIT rays of every
    chunk -- point, SDF gradient, ray direction, colour -- to cloud.add with the view's position in the list as its serial.
    appearance: "mean" = ONE code for all views, the mean embedding row (the cloud's colours then do not mix the views'
    exposures; this project's choice), "view" = each view's own row `ts`, or a tensor [n_a] = that code for all views.
    chunk: rays per trace call (None = views.TRACE_CHUNK); trace_kw goes to trace_view (eps, max_iter, step, ...).
    on_view(serial, out): called with every view's trace_view result (planes and stats) before it is dropped.
    Returns host numbers: views, rays, hit / miss / inside / stalled, samples (= hits handed to the cloud)."""
    from . import views as V

    if torch.is_tensor(appearance):
        a_code = appearance
    elif appearance == "mean":
        a_code = mean_appearance(rdr)
    elif appearance == "view":
        a_code = None
    else:
        raise ValueError("fuse_views: appearance is 'mean', 'view' or a code tensor (got %r)" % (appearance,))
    tot = {"views": 0, "rays": 0, "hit": 0, "miss": 0, "inside": 0, "stalled": 0, "samples": 0}
    kw = dict(trace_kw)
    if chunk is not None:
        kw["chunk"] = chunk
    for serial, (camera, ts) in enumerate(cameras_and_ts):
        def on_hits(p0, hit, pts, dirs, rgb, grad, serial=serial):
            cloud.add(pts, grad, dirs, rgb, serial)
            tot["samples"] += int(hit.numel())

        out = V.trace_view(rdr, camera, ts, a_code=a_code, on_hits=on_hits, **kw)
        tot["views"] += 1
        for k in ("rays", "hit", "miss", "inside", "stalled"):
            tot[k] += out["stats"][k]
        if on_view is not None:
            on_view(serial, out)
    return tot
