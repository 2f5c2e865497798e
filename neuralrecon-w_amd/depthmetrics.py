"""Depth and normal maps of one view against ground truth, on the device (not in the reference: DESIGN.md 8).

    gz, gn = gt_planes_from_mesh(RasterMesh(v, f), face_normals, K, w2c, H, W)       # the truth: rasterised mesh (SfM frame)
    t, nn, _ = pred_planes_from_trace(rdr, camera, ts)                                # the learned surface: views.trace_view
    row = compare_planes(gz, t, gt_n=gn, pred_n=nn, mode="t", camera=camera, scale=rdr.radius)
    print(summarise([row])["pooled"])                                                 # abs-rel, RMSE, delta, angles, completeness
    eval_scene(root_dir, pred="mesh", pred_mesh="mesh.ply", gt_mesh="mesh.ply")       # a whole split -> rows and the summary

One view is ONE `ncw_depthmetrics_view` call (csrc/ncw_depthmetrics.hip: a fused launch and a fold) into row v of a device table;
`ViewScorer.rows()` reads the table of a whole split back once.  The per-pixel rules, the row layout and the order of the sums
are stated in include/neuconw_hip.h and restated in numpy by tests/_depthmetrics_ref.py.  The kernel calls no cos / pow: the
thresholds and the two edge tables are made here.  `summarise` is host float64 arithmetic over the rows.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import lib as L

ROW_SUMS = ("sum_abs", "sum_err", "sum_sq", "sum_rel", "sum_sq_rel", "sum_cos")       # words 0..5 (float64)
ROW_COUNTS = ("both", "gt_only", "pred_only", "neither", "masked", "delta1", "delta2", "delta3", "normals", "ang1", "ang2",
              "ang3")                                                                 # words 6..17 (int64)
ANGLE_SHARES = (11.25, 22.5, 30.0)  # degrees
MODES = {"z": L.DM_PRED_Z, "t": L.DM_PRED_T}


# ---------------------------------------------------------------------------------------------------
# thresholds and tables (host)
# ---------------------------------------------------------------------------------------------------
def default_rel_edges():
    """1001 edges, geometric from 1e-4 to 10 (ratio 10^0.005: a bin centre is within 0.6 % of any value in its bin)."""
    return np.geomspace(1e-4, 10.0, 1001)


def make_tables(angle_step=0.1, rel_edges=None):
    """(cos_edges float32 [NA], rel_edges float32 [NR], thresholds) for compare_planes.  cos_edges[k - 1] = cos(k angle_step) for
    k = 1 .. NA with NA = ceil(180 / angle_step) - 1 (angle bin k is (k step, (k + 1) step], bin 0 holds 0 too, the last one ends at 180), in
    float64 and then rounded; both tables must stay strictly monotonic AFTER the rounding (ValueError otherwise)."""
    step = float(angle_step)
    if not (step > 0 and step <= 180):
        raise ValueError("depthmetrics: angle_step must lie in (0, 180] degrees (got %r)" % (angle_step,))
    na = max(1, int(math.ceil(180.0 / step - 1e-9)) - 1)
    if na > L.DM_MAX_EDGES:
        raise ValueError("depthmetrics: angle_step %g gives %d edges; at most %d (angle_step >= %.4g)"
                         % (step, na, L.DM_MAX_EDGES, 180.0 / (L.DM_MAX_EDGES + 1)))
    cos_e = np.cos(np.deg2rad(step * np.arange(1, na + 1, dtype=np.float64))).astype(np.float32)
    rel_e = np.asarray(default_rel_edges() if rel_edges is None else rel_edges, dtype=np.float64).reshape(-1).astype(np.float32)
    if not 1 <= rel_e.size <= L.DM_MAX_EDGES:
        raise ValueError("depthmetrics: rel_edges holds %d values; 1 .. %d" % (rel_e.size, L.DM_MAX_EDGES))
    if not (np.isfinite(rel_e).all() and (np.diff(rel_e) > 0).all()):
        raise ValueError("depthmetrics: rel_edges must be finite and strictly ascending as float32")
    if not (np.diff(cos_e) < 0).all():
        raise ValueError("depthmetrics: cos(k angle_step) is not strictly descending in float32 at angle_step %g" % step)
    thr = {"delta": [np.float32(1.25), np.float32(1.25 ** 2), np.float32(1.25 ** 3)],
           "cos": [np.float32(math.cos(math.radians(a))) for a in ANGLE_SHARES]}
    return cos_e, rel_e, thr


def _plane(t, shape, dtype, dev, what):
    if t is None:
        return None
    if not (torch.is_tensor(t) and t.is_cuda):
        raise L.NeuconwHipError("depthmetrics: %s is not on a GPU; there is no CPU fallback" % what)
    if tuple(t.shape) != tuple(shape):
        raise ValueError("depthmetrics: %s is %s, expected %s" % (what, tuple(t.shape), tuple(shape)))
    if dtype == torch.uint8:
        t = t.ne(0).to(torch.uint8) if t.dtype != torch.uint8 else t
    return t.detach().to(dev, dtype).contiguous()


class ViewScorer:
    """The device table [n_views, K] of a split and what a launch into it needs: the two edge tables, the thresholds, scratch.
    `score(v, ...)` launches view v; `rows()` reads the whole table back ONCE and returns one dict per view."""

    def __init__(self, n_views=1, angle_step=0.1, rel_edges=None, device=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise L.NeuconwHipError("depthmetrics.ViewScorer: the comparison runs on a GPU only; there is no CPU fallback")
        self.dev = dev
        self.angle_step = float(angle_step)
        self.cos_edges_host, self.rel_edges_host, thr = make_tables(angle_step, rel_edges)
        self.thr = thr
        self.cos_edges = torch.from_numpy(self.cos_edges_host).to(dev)
        self.rel_edges = torch.from_numpy(self.rel_edges_host).to(dev)
        self.na, self.nr = int(self.cos_edges_host.size), int(self.rel_edges_host.size)
        self.K = L.DM_FIXED + self.nr + 1 + self.na + 1
        self.n_views = int(n_views)
        if self.n_views < 1:
            raise ValueError("depthmetrics.ViewScorer: n_views must be >= 1")
        self.table = torch.zeros(self.n_views, self.K, dtype=torch.int64, device=dev)
        self.scratch = None

    def score(self, v, gt_z, pred, gt_n=None, pred_n=None, mask=None, mode="z", camera=None, scale=1.0, want_planes=False):
        """One view into row v.  gt_z, pred [H,W]; gt_n, pred_n [3,H,W] or None; mask [H,W] (non-zero / True = excluded) or None;
        mode 'z' (pred = eye-space z, pred_n = unit normals) or 't' (pred / pred_n = views.trace_view's depth / normal planes;
        camera = its views.Camera, scale = the renderer's radius).  want_planes: returns dict(err_rel, err_cos, z_pred) [H,W]."""
        if mode not in MODES:
            raise ValueError("depthmetrics: mode must be 'z' or 't' (got %r)" % (mode,))
        if not 0 <= int(v) < self.n_views:
            raise IndexError("depthmetrics: view %d outside the table of %d rows" % (v, self.n_views))
        if not (torch.is_tensor(gt_z) and gt_z.dim() == 2):
            raise ValueError("depthmetrics: gt_z is an [H, W] tensor")
        H, W = int(gt_z.shape[0]), int(gt_z.shape[1])
        if H < 1 or W < 1:
            raise ValueError("depthmetrics: empty image %d x %d" % (H, W))
        dev = self.dev
        gz = _plane(gt_z, (H, W), torch.float32, dev, "gt_z")
        pz = _plane(pred, (H, W), torch.float32, dev, "pred")
        gn = _plane(gt_n, (3, H, W), torch.float32, dev, "gt_n")
        pn = _plane(pred_n, (3, H, W), torch.float32, dev, "pred_n")
        mk = _plane(mask, (H, W), torch.uint8, dev, "mask")
        if not (float(scale) > 0 and math.isfinite(float(scale))):
            raise ValueError("depthmetrics: scale must be finite and > 0 (got %r)" % (scale,))
        prm = L.NcwDepthMetricsParams()
        if mode == "t":
            if camera is None:
                raise ValueError("depthmetrics: mode 't' needs the view's Camera (the t -> z conversion uses its rays)")
            if (camera.height, camera.width) != (H, W):
                raise ValueError("depthmetrics: the camera is %d x %d, the planes %d x %d" % (camera.height, camera.width, H, W))
            prm.cam = camera.struct()
        prm.scale = float(scale)
        for k in range(3):
            prm.delta_thr[k] = float(self.thr["delta"][k])
            prm.cos_thr[k] = float(self.thr["cos"][k])
        prm.n_cos_edges, prm.n_rel_edges = self.na, self.nr
        prm.cos_edges, prm.rel_edges = self.cos_edges.data_ptr(), self.rel_edges.data_ptr()
        lib = L.get_lib()
        need = int(lib.ncw_depthmetrics_scratch_bytes(H * W))
        if self.scratch is None or self.scratch.numel() * 8 < need:
            self.scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
        planes = None
        if want_planes:
            planes = {k: torch.empty(H, W, dtype=torch.float32, device=dev) for k in ("err_rel", "err_cos", "z_pred")}
        p = planes or {}
        L.check(lib.ncw_depthmetrics_view(L.ptr(gz), L.ptr(gn), L.ptr(pz), L.ptr(pn), L.ptr(mk), H, W, MODES[mode], C.byref(prm),
                                          L.ptr(self.scratch), L.ptr(self.table), int(v), self.K, L.ptr(p.get("err_rel")),
                                          L.ptr(p.get("err_cos")), L.ptr(p.get("z_pred")), L.stream_ptr(dev)),
                "ncw_depthmetrics_view")
        return planes

    def rows(self):
        """One dict per view: the float64 sums and int64 counts under ROW_SUMS / ROW_COUNTS, `hist_rel` [NR + 1] and `hist_cos`
        [NA + 1] (int64), and what `summarise` needs to read them: `rel_edges` (float64 of the float32 table), `angle_step`."""
        t = self.table.cpu().numpy()
        return [row_dict(t[v], self.nr, self.na, self.rel_edges_host, self.angle_step) for v in range(self.n_views)]


def row_dict(words, nr, na, rel_edges, angle_step):
    """A table row (int64 [K]) as the dict `summarise` takes."""
    words = np.ascontiguousarray(words, dtype=np.int64)
    sums = words[:L.DM_SUMS].view(np.float64)
    d = {k: float(sums[i]) for i, k in enumerate(ROW_SUMS)}
    d.update({k: int(words[L.DM_SUMS + i]) for i, k in enumerate(ROW_COUNTS)})
    d["hist_rel"] = words[L.DM_FIXED:L.DM_FIXED + nr + 1].copy()
    d["hist_cos"] = words[L.DM_FIXED + nr + 1:L.DM_FIXED + nr + 1 + na + 1].copy()
    d["rel_edges"] = np.asarray(rel_edges, dtype=np.float64).copy()
    d["angle_step"] = float(angle_step)
    return d


def compare_planes(gt_z, pred, *, gt_n=None, pred_n=None, mask=None, mode="z", camera=None, scale=1.0, angle_step=0.1,
                   rel_edges=None, want_planes=False):
    """Scores ONE view (see ViewScorer.score) and returns its raw row as a dict (ViewScorer.rows); with want_planes=True returns
    (row, planes) with planes = dict(err_rel, err_cos, z_pred) [H,W] f32 on the device."""
    if not (torch.is_tensor(gt_z) and gt_z.is_cuda):
        raise L.NeuconwHipError("depthmetrics.compare_planes: gt_z is not on a GPU; there is no CPU fallback")
    sc = ViewScorer(1, angle_step, rel_edges, gt_z.device)
    planes = sc.score(0, gt_z, pred, gt_n=gt_n, pred_n=pred_n, mask=mask, mode=mode, camera=camera, scale=scale,
                      want_planes=want_planes)
    row = sc.rows()[0]
    return (row, planes) if want_planes else row


# ---------------------------------------------------------------------------------------------------
# the summary (host, float64)
# ---------------------------------------------------------------------------------------------------
def _div(a, b):
    return float(a) / float(b) if b else float("nan")


def _lower_median_bin(hist):
    """The bin holding the ceil(n / 2)-th smallest value (the lower median); -1 for an empty histogram."""
    n = int(hist.sum())
    if n == 0:
        return -1
    return int(np.searchsorted(np.cumsum(hist), (n + 1) // 2, side="left"))


def rel_bin_centres(rel_edges):
    """Centres of the NR + 1 bins [0, e0), [e0, e1), .., [e_last, inf): the last bin reports its lower edge."""
    e = np.asarray(rel_edges, dtype=np.float64)
    lo = np.concatenate([[0.0], e])
    hi = np.concatenate([e, e[-1:]])
    return (lo + hi) / 2


def angle_bin_centres(n_bins, angle_step):
    """Centres in degrees of the bins (k step, (k + 1) step], the last one ending at 180."""
    lo = angle_step * np.arange(n_bins, dtype=np.float64)
    hi = np.minimum(lo + angle_step, 180.0)
    hi[-1] = 180.0
    return (lo + hi) / 2


def summarise_row(row, unit_scale=1.0):
    """The scores of one raw row (or of a pooled one).  Lengths (mae, rmse, bias, sq_rel) are multiplied by unit_scale; ratios
    are not.  Every score of an empty view is NaN (no division by zero)."""
    n, u = row["both"], float(unit_scale)
    nn = row["normals"]
    out = {k: row[k] for k in ("both", "gt_only", "pred_only", "neither", "masked", "normals")}
    out["abs_rel"] = _div(row["sum_rel"], n)
    out["sq_rel"] = _div(row["sum_sq_rel"], n) * u
    out["rmse"] = math.sqrt(_div(row["sum_sq"], n)) * u if n else float("nan")
    out["mae"] = _div(row["sum_abs"], n) * u
    out["bias"] = _div(row["sum_err"], n) * u
    for k in (1, 2, 3):
        out["delta%d" % k] = _div(row["delta%d" % k], n)
    out["completeness"] = _div(n, n + row["gt_only"])
    out["extra"] = _div(row["pred_only"], n + row["pred_only"])
    b = _lower_median_bin(row["hist_rel"])
    out["median_rel"] = float(rel_bin_centres(row["rel_edges"])[b]) if b >= 0 else float("nan")
    ac = angle_bin_centres(len(row["hist_cos"]), row["angle_step"])
    b = _lower_median_bin(row["hist_cos"])
    out["median_angle"] = float(ac[b]) if b >= 0 else float("nan")
    out["mean_angle"] = _div(float((row["hist_cos"].astype(np.float64) * ac).sum()), nn)
    out["mean_cos"] = _div(row["sum_cos"], nn)
    for k, a in enumerate(ANGLE_SHARES):
        out["angle_within_%g" % a] = _div(row["ang%d" % (k + 1)], nn)
    return out


def pool_rows(rows):
    """One row over all pixels of `rows`: sums, counts and histograms added (the tables must be the same)."""
    rows = list(rows)
    if not rows:
        raise ValueError("depthmetrics.pool_rows: no rows")
    r0 = rows[0]
    for r in rows[1:]:
        if r["angle_step"] != r0["angle_step"] or not np.array_equal(r["rel_edges"], r0["rel_edges"]):
            raise ValueError("depthmetrics.pool_rows: rows of different tables")
    out = {k: math.fsum(r[k] for r in rows) for k in ROW_SUMS}
    out.update({k: sum(r[k] for r in rows) for k in ROW_COUNTS})
    out["hist_rel"] = np.sum([r["hist_rel"] for r in rows], axis=0).astype(np.int64)
    out["hist_cos"] = np.sum([r["hist_cos"] for r in rows], axis=0).astype(np.int64)
    out["rel_edges"], out["angle_step"] = r0["rel_edges"], r0["angle_step"]
    return out


def summarise(rows, unit_scale=1.0):
    """{"views": [scores per view], "pooled": scores over all pixels of all views} from raw rows (host, float64)."""
    rows = list(rows)
    return {"views": [summarise_row(r, unit_scale) for r in rows], "pooled": summarise_row(pool_rows(rows), unit_scale)}


# ---------------------------------------------------------------------------------------------------
# planes
# ---------------------------------------------------------------------------------------------------
def raster_K(K):
    """K [3,3] of the project's rays (pixel (r, c) looks through the image point (c, r): views.Camera) as the rasterizer takes
    it: it samples (c + 0.5, r + 0.5), so cx and cy move by half a pixel (synth.raster_K at ss = 1)."""
    K = np.array(K, dtype=np.float64).reshape(3, 3)
    K[0, 2] += 0.5
    K[1, 2] += 0.5
    return K


@torch.no_grad()
def gt_planes_from_mesh(raster_mesh, face_normals, K, w2c, H, W, cull="back", znear=None, zfar=None, zbuf=None,
                        half_pixel=True, normal_view=None):
    """(z [H,W] f32, 0 = empty; normal [3,H,W] f32, 0 there) of a reproj.RasterMesh seen by K [3,3] at world -> camera w2c (3x4 /
    4x4, OpenCV axes, the mesh's frame): `rasterize` + `resolve`, then the face's normal gathered by face id.  face_normals
    [F,3] (numpy or device tensor) in the frame the normals are compared in, or None (no normal plane).  With cull='none' a
    normal is turned toward the camera (n . p_cam <= 0 in the camera frame); with 'back' the visible faces face it already.
    normal_view [3,3]: the rotation from the FRAME OF face_normals to the camera; None = the rotation of w2c, which is right when
    the normals are in the mesh's own frame.  A caller that hands over normals already turned into another frame (eval_scene with
    gt_frame='gt': a GT-frame mesh, normals in the SfM frame) gives that frame's rotation.
    half_pixel: K is the camera of the project's rays and moves by half a pixel for the rasterizer (`raster_K`)."""
    from . import reproj

    H, W = int(H), int(W)
    Kr = raster_K(K) if half_pixel else np.asarray(K, dtype=np.float64).reshape(3, 3)
    kw = {}
    if znear is not None:
        kw["znear"] = znear
    if zfar is not None:
        kw["zfar"] = zfar
    s = raster_mesh.view_struct(Kr, w2c, H, W, cull=cull, **kw)
    if zbuf is None or zbuf.numel() != H * W:
        zbuf = torch.empty(H * W, dtype=torch.int64, device=raster_mesh.dev)
    raster_mesh.rasterize(s, zbuf)
    z, face = reproj.resolve(zbuf, H, W)
    if face_normals is None:
        return z, None
    fn = face_normals if torch.is_tensor(face_normals) else torch.from_numpy(np.ascontiguousarray(face_normals, dtype=np.float32))
    fn = fn.to(raster_mesh.dev, torch.float32).reshape(-1, 3)
    if fn.shape[0] != raster_mesh.nf:
        raise ValueError("gt_planes_from_mesh: %d normals for %d faces" % (fn.shape[0], raster_mesh.nf))
    hit = face >= 0
    n = fn[face.clamp(min=0).long()] * hit.unsqueeze(-1)                       # [H,W,3]
    if cull == "none":
        V = np.asarray(w2c if normal_view is None else normal_view, dtype=np.float64)[:3, :3]
        R = torch.from_numpy(V / np.linalg.norm(V[0])).to(raster_mesh.dev, torch.float32)
        r, c = torch.meshgrid(torch.arange(H, device=z.device, dtype=torch.float32),
                              torch.arange(W, device=z.device, dtype=torch.float32), indexing="ij")
        p = torch.stack([(c + 0.5 - float(Kr[0, 2])) / float(Kr[0, 0]), (r + 0.5 - float(Kr[1, 2])) / float(Kr[1, 1]),
                         torch.ones_like(c)], -1)
        away = ((n @ R.T) * p).sum(-1) > 0
        n = torch.where(away.unsqueeze(-1), -n, n)
    return z, n.permute(2, 0, 1).contiguous()


@torch.no_grad()
def gt_planes_from_cloud(cloud, K, pose, H, W, scene_config=None, voxel_size=None, device=None):
    """(z [H,W] f32, None): reproj.render_cloud_depth's first-hit depth of a GT cloud, voxel-quantised (the entry into the first
    occupied voxel + 0.02), no normals.  cloud: a reproj.VoxelCloud, or points [N,3] in the frame of scene_config's eval_bbx
    (then scene_config and voxel_size are needed; the grid is rebuilt on every call).  pose: camera -> world of that frame."""
    from . import reproj

    if not isinstance(cloud, reproj.VoxelCloud):
        if scene_config is None or voxel_size is None:
            raise ValueError("gt_planes_from_cloud: points need scene_config and voxel_size")
        cloud = reproj.VoxelCloud(cloud, scene_config, voxel_size, device)
    depth = torch.empty(int(H) * int(W), dtype=torch.float32, device=cloud.dev)
    cloud.trace(K, pose, int(H), int(W), depth=depth)
    return depth.view(int(H), int(W)), None


def pred_planes_from_trace(rdr, camera, ts, **trace_kw):
    """(depth [H,W], normal [3,H,W] or None, out): views.trace_view's planes for compare_planes(mode='t', camera=camera,
    scale=rdr.radius).  With shade=False the tracer evaluates no gradient: the normal plane is None."""
    from . import views

    out = views.trace_view(rdr, camera, ts, **trace_kw)
    return out["depth"], (out["normal"] if trace_kw.get("shade", True) else None), out


def pred_planes_from_mesh(raster_mesh, face_normals, K, w2c, H, W, cull="back", **kw):
    """The rasteriser again, for an extracted mesh: (z, normal) as gt_planes_from_mesh, for compare_planes(mode='z')."""
    return gt_planes_from_mesh(raster_mesh, face_normals, K, w2c, H, W, cull=cull, **kw)


# ---------------------------------------------------------------------------------------------------
# a scene
# ---------------------------------------------------------------------------------------------------
def _label_mask(root_dir, name, ids, H, W, device):
    """uint8 [H,W]: 1 where semantic_maps/<stem>.npz holds one of `ids` (nearest sample when the map has another size);
    None without the file."""
    path = os.path.join(root_dir, "semantic_maps", os.path.splitext(name)[0] + ".npz")
    if not ids or not os.path.isfile(path):
        return None
    lab = np.load(path)["arr_0"]
    lh, lw = lab.shape[:2]
    if (lh, lw) != (H, W):
        lab = lab[np.minimum(np.arange(H) * lh // H, lh - 1)][:, np.minimum(np.arange(W) * lw // W, lw - 1)]
    return torch.from_numpy(np.isin(lab, list(ids)).astype(np.uint8)).to(device)


def _z_range(verts, unit_scale):
    """(znear, zfar) of the rasteriser for a mesh: 1e-4 and 1e4 of its box diagonal, in camera (SfM) units -- the rasteriser's
    own defaults are pyrender's 0.05 / 100, which fit a metric scene only."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    diag = float(np.linalg.norm(v.max(0) - v.min(0))) / float(unit_scale)
    return 1e-4 * diag, 1e4 * diag


def split_ids(scene, split):
    """Image ids of 'train' / 'test' / 'all' in the tsv's order (views.read_scene)."""
    if split == "all":
        return list(scene["ids"])
    train = set(scene["ids_train"])
    if split == "train":
        return list(scene["ids_train"])
    if split == "test":
        return [i for i in scene["ids"] if i not in train]
    raise ValueError("split must be 'train', 'test' or 'all' (got %r)" % (split,))


@torch.no_grad()
def eval_scene(root_dir, *, pred="mesh", cfg_path=None, ckpt_path=None, pred_mesh=None, gt_mesh=None, gt_cloud=None,
               gt_frame="sfm", split="test", max_views=None, img_downscale=1, mask_labels=("person",), sfm_path="sparse",
               voxel_size=None, cull="back", angle_step=0.1, rel_edges=None, prec=None, trace_kw=None, on_view=None,
               device=None, verbose=False):
    """Scores every view of a split of the scene directory `root_dir` against its ground truth.
      truth: gt_mesh (a triangle PLY: depth and normals by the rasteriser) or gt_cloud (a point PLY: voxel first-hit depth at
             voxel_size over config.yaml's eval_bbx, no normals).  gt_frame 'sfm': the file is in the SfM frame and seen with the
             image's w2c; 'gt': it is in the ground-truth frame and seen with w2c inv(sfm2gt) (config.yaml; as reproj_filter forms
             it), its normals turned into the SfM frame, and the summary's lengths are multiplied by the sfm2gt scale.  Depths
             are SfM camera units either way.  A gt_cloud with gt_frame 'sfm' is carried to the GT frame first (the voxel grid
             lives over eval_bbx).
      prediction: pred='mesh' with pred_mesh (a PLY in the SfM frame, e.g. scripts/extract_mesh.py's) or pred='trace' with
             cfg_path + ckpt_path (views.trace_view of the learned surface; trace_kw goes to it; ts = the image id).
      mask_labels: ADE20K label names excluded where semantic_maps/<stem>.npz exists.
      on_view(info): called per view with dict(index, image_id, name, gt_z, pred, planes, mode) -- planes = err_rel / err_cos /
             z_pred when the callback is given (the tool's --panels / --write_planes).
    Returns dict(rows, summary, views=[{image_id, name, width, height}], unit_scale)."""
    import yaml

    from . import evalmesh, labels, ply, reproj, synth, views

    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise L.NeuconwHipError("depthmetrics.eval_scene: device %s is not a GPU; there is no CPU fallback" % (dev,))
    if (gt_mesh is None) == (gt_cloud is None):
        raise ValueError("eval_scene: give exactly one of gt_mesh / gt_cloud")
    if gt_frame not in ("sfm", "gt"):
        raise ValueError("eval_scene: gt_frame must be 'sfm' or 'gt' (got %r)" % (gt_frame,))
    if pred not in ("mesh", "trace"):
        raise ValueError("eval_scene: pred must be 'mesh' or 'trace' (got %r)" % (pred,))
    if pred == "mesh" and pred_mesh is None:
        raise ValueError("eval_scene: pred='mesh' needs pred_mesh")
    if pred == "trace" and (cfg_path is None or ckpt_path is None):
        raise ValueError("eval_scene: pred='trace' needs cfg_path and ckpt_path")
    log = print if verbose else (lambda *a: None)
    scene = views.read_scene(root_dir, sfm_path)
    ids = split_ids(scene, split)
    if max_views is not None:
        ids = ids[:int(max_views)]
    if not ids:
        raise ValueError("eval_scene: split %r of %s holds no registered image" % (split, root_dir))
    scene_config, S, unit_scale = None, np.eye(4), 1.0
    cfg_file = os.path.join(root_dir, "config.yaml")
    if gt_frame == "gt" or gt_cloud is not None:
        with open(cfg_file) as fh:
            scene_config = yaml.safe_load(fh)
        S = np.array(scene_config["sfm2gt"], dtype=np.float64)
    if gt_frame == "gt":
        unit_scale = float(np.sqrt((S[0, :3] ** 2).sum()))
    S_inv = np.linalg.inv(S)

    gt_raster = gt_fn = gt_vox = None
    if gt_mesh is not None:
        gv, gf, _ = ply.read_mesh(gt_mesh)
        if gf.shape[0] == 0:
            raise ValueError("eval_scene: %s has no faces; pass it as gt_cloud" % gt_mesh)
        gt_raster = reproj.RasterMesh(gv, gf, dev)
        gt_range = _z_range(gv, unit_scale)
        n, _ = synth.face_normals(np.asarray(gv, dtype=np.float64), np.asarray(gf, dtype=np.int64))
        if gt_frame == "gt":
            n = n @ (S[:3, :3] / unit_scale)  # R^T n as rows: the SfM frame, where the prediction's normals live
        gt_fn = torch.from_numpy(n.astype(np.float32)).to(dev)
    else:
        if voxel_size is None:
            raise ValueError("eval_scene: gt_cloud needs voxel_size (units of eval_bbx)")
        pts, _, _ = ply.read_mesh(gt_cloud)
        if gt_frame == "sfm":
            pts = evalmesh.apply_transform(pts, S)
        gt_vox = reproj.VoxelCloud(pts, scene_config, voxel_size, dev)

    rdr = pr_raster = pr_fn = None
    if pred == "mesh":
        pv, pf, _ = ply.read_mesh(pred_mesh)
        if pf.shape[0] == 0:
            raise ValueError("eval_scene: %s has no faces" % pred_mesh)
        pr_raster = reproj.RasterMesh(pv, pf, dev)
        pr_range = _z_range(pv, 1.0)
        pr_fn = torch.from_numpy(synth.face_normals(np.asarray(pv, dtype=np.float64), np.asarray(pf, dtype=np.int64))[0]
                                 .astype(np.float32)).to(dev)
    else:
        from . import config as CFG
        from . import trainer

        cfg = CFG.load_config(cfg_path, {"DATASET": {"ROOT_DIR": root_dir}})
        emb, neuconw, nerf, rdr, _ = CFG.build_system(cfg, dev, prec)
        trainer.load_checkpoint(ckpt_path, emb, neuconw, nerf)
        for m in (emb, neuconw, nerf):
            m.eval()
    mask_ids = [labels.label_id(n) for n in (mask_labels or ())]

    sc = ViewScorer(len(ids), angle_step, rel_edges, dev)
    infos = []
    for v, iid in enumerate(ids):
        name = scene["images"][iid]["name"]
        K, w2c, c2w, W, H = views.image_pose(scene, iid, int(img_downscale))
        if gt_raster is not None:
            gz, gn = gt_planes_from_mesh(gt_raster, gt_fn, K, w2c @ S_inv if gt_frame == "gt" else w2c, H, W, cull=cull, normal_view=w2c[:3, :3],
                                         znear=gt_range[0], zfar=gt_range[1])
        else:
            gz, gn = gt_planes_from_cloud(gt_vox, K, np.linalg.inv(w2c @ S_inv), H, W)
        mask = _label_mask(root_dir, name, mask_ids, H, W, dev)
        if pred == "mesh":
            pz, pn = pred_planes_from_mesh(pr_raster, pr_fn, K, w2c, H, W, cull=cull, znear=pr_range[0], zfar=pr_range[1])
            kw = dict(mode="z")
        else:
            near, far = views.image_near_far(scene, w2c)
            cam = views.Camera(K, c2w, W, H, near, far)
            pz, pn, _ = pred_planes_from_trace(rdr, cam, iid, **(trace_kw or {}))
            kw = dict(mode="t", camera=cam, scale=float(rdr.radius))
        planes = sc.score(v, gz, pz, gt_n=gn, pred_n=pn if gn is not None else None, mask=mask, want_planes=on_view is not None,
                          **kw)
        infos.append({"image_id": int(iid), "name": name, "width": int(W), "height": int(H)})
        if on_view is not None:
            on_view(dict(infos[-1], index=v, gt_z=gz, pred=pz, planes=planes, mode=kw["mode"]))
        log("view %d / %d: %s (%d x %d)" % (v + 1, len(ids), name, W, H))
    rows = sc.rows()
    return {"rows": rows, "summary": summarise(rows, unit_scale), "views": infos, "unit_scale": unit_scale}
