"""Mesh operations on the GPU: connected components and the compaction of a face subset (csrc/ncw_meshops.hip).

The reference has no such mode: its reprojection filter writes a point cloud (utils/reproj_filter.py:293-300) and nothing in
it labels the components of a mesh.  Two users here, which do the same thing -- choose a subset of faces, then compact:
  * reproj.reproj_filter(keep_faces=True) keeps the faces of the vertices the views mark (`face_select` + `submesh`);
  * mesh.extract_mesh(min_component_faces / largest_components) drops floaters before the colour pass (`clean`).

Connectivity is by SHARED VERTEX INDEX: two faces that only share coordinates are not connected, two pieces that touch in one
welded vertex are one component.  A face takes part iff its mask is set, its corners lie in [0, V) and are distinct.  The label
of a component is the smallest vertex index in it.  Everything is exact integer work, bitwise reproducible.

`simplify` (csrc/ncw_simplify.hip) is the one operation here with floating-point work: uniform-grid vertex clustering with a
quadric-optimal vertex per cell.  Its contract (include/neuconw_hip.h) fixes every summation order, so it is bitwise
reproducible too.
"""
import ctypes as C
import math

import torch

from . import lib as L

MAX_INDEX = (1 << 31) - 1


def _check(faces, n_vertices, what):
    """ValueError for what no device could run; then the device check ("no CPU fallback")."""
    if not torch.is_tensor(faces) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError("meshops.%s: faces must be an integer (int32 / int64) tensor [F,3]" % what)
    if faces.shape[0] == 0:
        raise ValueError("meshops.%s: F == 0: there is no face to work on" % what)
    if faces.shape[0] > MAX_INDEX:
        raise ValueError("meshops.%s: at most 2^31 - 1 faces" % what)
    n_vertices = int(n_vertices)
    if n_vertices < 0 or n_vertices > MAX_INDEX:
        raise ValueError("meshops.%s: V = %d: vertex indices are int32, V < 2^31" % (what, n_vertices))
    if not faces.is_cuda:
        raise L.NeuconwHipError("meshops.%s: the faces are not on a GPU; there is no CPU fallback" % what)
    return n_vertices


def _faces32(faces):
    """int32 [F,3], contiguous.  int64 indices outside int32 become -1 (out of range for every V): never a wrapped index."""
    if faces.dtype == torch.int32:
        return faces.contiguous()
    bad = (faces < 0) | (faces > MAX_INDEX)
    return torch.where(bad, torch.full_like(faces, -1), faces).to(torch.int32).contiguous()


def _mask(m, n, dev, what, name):
    if m is None:
        return None
    if not torch.is_tensor(m) or m.numel() != n or m.dim() != 1:
        raise ValueError("meshops.%s: %s must be a tensor of %d elements" % (what, name, n))
    if m.device != dev:
        raise L.NeuconwHipError("meshops.%s: %s is not on %s; there is no CPU fallback" % (what, name, dev))
    return (m != 0).to(torch.uint8).contiguous()


@torch.no_grad()
def components(faces, n_vertices, keep=None):
    """(labels int32 [V], sizes int32 [V]) on the device.  labels[v] = the smallest vertex index of v's component over the
    participating faces (keep [F]: nonzero = takes part; None = all); a vertex of no participating face is its own label.
    sizes[l] = participating faces of the component labelled l, 0 at every other index."""
    V = _check(faces, n_vertices, "components")
    dev = faces.device
    f32 = _faces32(faces)
    F = int(f32.shape[0])
    k8 = _mask(keep, F, dev, "components", "keep")
    lib, st = L.get_lib(), L.stream_ptr(dev)
    labels = torch.arange(V, dtype=torch.int32, device=dev)
    sizes = torch.zeros(V, dtype=torch.int32, device=dev)
    L.check(lib.ncw_mesh_cc_hook(L.ptr(f32), L.ptr(k8), F, V, L.ptr(labels), st), "ncw_mesh_cc_hook")
    L.check(lib.ncw_mesh_cc_flatten(L.ptr(labels), V, st), "ncw_mesh_cc_flatten")
    L.check(lib.ncw_mesh_cc_sizes(L.ptr(f32), L.ptr(k8), F, V, L.ptr(labels), L.ptr(sizes), st), "ncw_mesh_cc_sizes")
    return labels, sizes


@torch.no_grad()
def select_components(sizes, min_faces=0, largest=None):
    """comp_ok uint8 [V]: 1 at the labels whose component has at least `min_faces` faces and, with largest = K, is among the K
    components with the most faces -- ties to the SMALLER label (one sort of the composite key (max - size) V + label, no
    reliance on topk's tie order).  Only indices with sizes > 0 are components.  min_faces = 0 and largest = None: all ones."""
    if not torch.is_tensor(sizes) or sizes.dim() != 1 or sizes.dtype != torch.int32:
        raise ValueError("meshops.select_components: sizes must be the int32 [V] tensor of `components`")
    if int(min_faces) < 0 or (largest is not None and int(largest) < 0):
        raise ValueError("meshops.select_components: min_faces and largest must not be negative")
    if not sizes.is_cuda:
        raise L.NeuconwHipError("meshops.select_components: sizes is not on a GPU; there is no CPU fallback")
    ok = sizes >= int(min_faces)
    if largest is not None:
        V = int(sizes.shape[0])
        lab = torch.nonzero(sizes > 0).reshape(-1)                     # ascending labels, int64
        s = sizes[lab].long()
        top = torch.zeros(V, dtype=torch.bool, device=sizes.device)
        if lab.numel() and int(largest) > 0:
            key = (s.max() - s) * V + lab                               # < 2^62
            top[lab[torch.sort(key).indices[: int(largest)]]] = True
        ok = ok & top
    return ok.to(torch.uint8).contiguous()


@torch.no_grad()
def face_select(faces, n_vertices, vflags=None, min_corners=1, labels=None, comp_ok=None):
    """keep uint8 [F]: 1 iff the face's corners are in range and distinct, at least `min_corners` (1..3) of them have
    vflags [V] != 0 (when given), and comp_ok[labels[corner 0]] != 0 (when labels / comp_ok are given)."""
    if int(min_corners) not in (1, 2, 3):
        raise ValueError("meshops.face_select: min_corners must be 1, 2 or 3 (got %r)" % (min_corners,))
    if (labels is None) != (comp_ok is None):
        raise ValueError("meshops.face_select: labels and comp_ok go together")
    V = _check(faces, n_vertices, "face_select")
    dev = faces.device
    f32 = _faces32(faces)
    F = int(f32.shape[0])
    v8 = _mask(vflags, V, dev, "face_select", "vflags")
    c8 = _mask(comp_ok, V, dev, "face_select", "comp_ok")
    if labels is not None:
        if labels.dtype != torch.int32 or labels.numel() != V or labels.device != dev:
            raise ValueError("meshops.face_select: labels must be the int32 [V] tensor of `components`")
        labels = labels.contiguous()
    keep = torch.empty(F, dtype=torch.uint8, device=dev)
    L.check(L.get_lib().ncw_mesh_face_select(L.ptr(f32), F, V, L.ptr(v8), int(min_corners), L.ptr(labels), L.ptr(c8), L.ptr(keep),
                                             L.stream_ptr(dev)), "ncw_mesh_face_select")
    return keep


@torch.no_grad()
def submesh(vertices, faces, keep, colors=None):
    """The mesh of the faces with keep [F] != 0 (and corners in range and distinct): (vertices' [V',...], faces' int32 [F',3],
    colors' or None, vertex_index int64 [V']).  vertex_index holds the old index of every kept vertex -- the vertices some
    kept face uses -- in ascending order; kept faces keep their order too.  Attributes are gathered with torch indexing, in
    their own dtype.  An empty result is a valid mesh with 0 vertices and 0 faces.  Two device -> host reads (the counts)."""
    V = _check(faces, vertices.shape[0], "submesh")
    dev = faces.device
    if vertices.device != dev or (colors is not None and colors.device != dev):
        raise L.NeuconwHipError("meshops.submesh: vertices / colors are not on %s; there is no CPU fallback" % dev)
    f32 = _faces32(faces)
    F = int(f32.shape[0])
    k8 = _mask(keep, F, dev, "submesh", "keep")
    if k8 is None:
        raise ValueError("meshops.submesh: keep is required")
    k8 = k8 * face_select(f32, V)                                      # never index with an invalid face
    lib, st = L.get_lib(), L.stream_ptr(dev)
    used = torch.zeros(V, dtype=torch.uint8, device=dev)
    L.check(lib.ncw_mesh_compact_mark(L.ptr(f32), L.ptr(k8), F, V, L.ptr(used), st), "ncw_mesh_compact_mark")
    f_incl = torch.cumsum(k8, 0, dtype=torch.int32)
    n_out = int(f_incl[-1])
    index = torch.nonzero(used).reshape(-1)
    faces_out = torch.empty(n_out, 3, dtype=torch.int32, device=dev)
    if n_out:
        vmap = (torch.cumsum(used, 0, dtype=torch.int32) - used).contiguous()
        offset = (f_incl - k8).contiguous()
        L.check(lib.ncw_mesh_compact_faces(L.ptr(f32), L.ptr(k8), L.ptr(offset), L.ptr(vmap), F, V, n_out, L.ptr(faces_out), st),
                "ncw_mesh_compact_faces")
    return vertices[index], faces_out, (None if colors is None else colors[index]), index


@torch.no_grad()
def clean(vertices, faces, colors=None, min_component_faces=0, largest_components=None, stats=None):
    """`submesh` of the components with at least `min_component_faces` faces that are among the `largest_components` largest
    (ties to the smaller label; None = no such limit).  stats (dict): components / faces before and after."""
    V = int(vertices.shape[0])
    labels, sizes = components(faces, V)
    ok = select_components(sizes, min_component_faces, largest_components)
    keep = face_select(faces, V, labels=labels, comp_ok=ok)
    out = submesh(vertices, faces, keep, colors)
    if stats is not None:
        comp = sizes > 0
        stats.update(components_before=int(comp.sum()), components_after=int((comp & (ok != 0)).sum()),
                     faces_before=int(faces.shape[0]), faces_after=int(out[1].shape[0]))
    return out


def _csr(cluster_of, n_clusters):
    """Stable sort of list entries by cluster: (order int64 [n], offsets int64 [C+1])."""
    order = torch.sort(cluster_of, stable=True).indices
    off = torch.zeros(n_clusters + 1, dtype=torch.int64, device=cluster_of.device)
    off[1:] = torch.cumsum(torch.bincount(cluster_of, minlength=n_clusters), 0)
    return order, off


def simplify_grid(lo, hi, cell):
    """Cells per axis of `simplify`'s grid over the box lo .. hi (lists of 3 floats): n = floor((hi - lo) / cell) + 1.
    ValueError for what the contract refuses: a cell size that is not finite and positive, a box that is not finite, 2^62 cells
    or more."""
    h = float(cell)
    if not (math.isfinite(h) and h > 0.0):
        raise ValueError("meshops.simplify: the cell size must be finite and positive (got %r)" % (cell,))
    if not all(math.isfinite(v) for v in list(lo) + list(hi)):
        raise ValueError("meshops.simplify: a used vertex has a coordinate that is not finite")
    n = []
    for a in range(3):
        q = (hi[a] - lo[a]) / h
        if not (math.isfinite(q) and q < 2.0 ** 62):
            raise ValueError("meshops.simplify: cell %r gives 2^62 cells or more" % (cell,))
        n.append(int(math.floor(q)) + 1)
    if n[0] * n[1] * n[2] >= 1 << 62:
        raise ValueError("meshops.simplify: cell %r gives %d x %d x %d cells, 2^62 or more" % (cell, n[0], n[1], n[2]))
    return n


def _stage(stats, name):
    """Stage boundary for scripts/bench_simplify.py: with stats["events"] a list, (name, device event) is appended to it."""
    if stats is not None and isinstance(stats.get("events"), list):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        stats["events"].append((name, e))


@torch.no_grad()
def simplify(vertices, faces, cell, colors=None, eps=1e-3, stats=None):
    """Vertex clustering on a uniform grid of cell size `cell` (the vertices' own units) with a quadric-optimal vertex per cell
    (Lindstrom's out-of-core simplification): (vertices' [V',3], faces' int32 [F',3], colors' or None, cluster_index int64 [V]).
    cluster_index maps every old vertex to its new vertex, or to -1 (a vertex of no participating face, or of a cell that no
    surviving face names).  Vertices come back in the input dtype; all arithmetic is float64 in a fixed order (the contract in
    include/neuconw_hip.h, restated by tests/_simplify_ref.py): the result is bitwise reproducible.

      * a face takes part iff its corners are in range and distinct; the grid spans the vertices such faces use;
      * every occupied cell becomes one vertex: the minimiser of the summed squared plane distances of the faces that touch the
        cell, regularised towards the mean of the cell's vertices by eps, and the mean itself where that solve is singular or
        leaves the cell -- creases and corners stay sharp where a plain cell mean rounds them off;
      * a face survives iff its corners fall into three different cells; duplicates (the same triple of cells in the same
        orientation) are dropped, the first one is kept; a pair of OPPOSITE orientation is not a duplicate, both stay;
      * colours (uint8 [V,3]) are averaged per cell, floor(sum / count + 0.5).

    This is this project's choice: the reference has no such mode, and no parity with open3d's simplify_vertex_clustering,
    trimesh or meshlab is claimed.  Clustering can create non-manifold edges, and it joins components that come within one cell
    of each other -- so `clean` goes first.  On a smooth convex surface the quadric vertex sits outside the surface by about as
    much as the cell mean sits inside: it is not closer there, it is closer at creases.
    stats (dict): vertices / faces before and after, clusters, clusters_at_mean, and at_mean (uint8 [V']: 1 where the output
    vertex is its cell's member mean), members / list_entries (the lengths of the two lists the placement walks).  ValueError for what no device could run (cell or eps not finite and positive / not
    negative, no participating face, non-finite coordinates, 2^62 cells or more); NeuconwHipError for CPU tensors."""
    if not torch.is_tensor(vertices) or vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype not in (torch.float32, torch.float64):
        raise ValueError("meshops.simplify: vertices must be a float32 / float64 tensor [V,3]")
    h, eps = float(cell), float(eps)
    if not (math.isfinite(h) and h > 0.0):
        raise ValueError("meshops.simplify: the cell size must be finite and positive (got %r)" % (cell,))
    if not (math.isfinite(eps) and eps >= 0.0):
        raise ValueError("meshops.simplify: eps must be finite and not negative (got %r)" % (eps,))
    V = _check(faces, vertices.shape[0], "simplify")
    dev = faces.device
    if vertices.device != dev or (colors is not None and colors.device != dev):
        raise L.NeuconwHipError("meshops.simplify: vertices / colors are not on %s; there is no CPU fallback" % dev)
    if colors is not None and (colors.dtype != torch.uint8 or tuple(colors.shape) != (V, 3)):
        raise ValueError("meshops.simplify: colors must be a uint8 tensor [V,3]")
    f32 = _faces32(faces)
    F = int(f32.shape[0])
    x = vertices.to(torch.float64).contiguous()
    lib, st = L.get_lib(), L.stream_ptr(dev)
    _stage(stats, "start")
    # 1 participation, used vertices
    part = face_select(f32, V)
    used = torch.zeros(V, dtype=torch.uint8, device=dev)
    L.check(lib.ncw_mesh_compact_mark(L.ptr(f32), L.ptr(part), F, V, L.ptr(used), st), "ncw_mesh_compact_mark")
    uidx = torch.nonzero(used).reshape(-1)
    if uidx.numel() == 0:
        raise ValueError("meshops.simplify: no face takes part (corners in range and distinct): there is nothing to simplify")
    # 2 grid
    xu = x[uidx].t().contiguous()                                      # [3, n]: a reduction along rows, not down three columns
    lo, hi = xu.amin(1).tolist(), xu.amax(1).tolist()
    n = simplify_grid(lo, hi, h)
    lo_c, n_c = (C.c_double * 3)(*lo), (C.c_int64 * 3)(*n)
    _stage(stats, "prepare")
    keys = torch.empty(V, dtype=torch.int64, device=dev)
    L.check(lib.ncw_mesh_sc_keys(L.ptr(x), L.ptr(used), V, lo_c, h, n_c, L.ptr(keys), st), "ncw_mesh_sc_keys")
    # 3 clusters: the distinct keys, ascending
    ckeys, inverse = torch.unique(keys[uidx], sorted=True, return_inverse=True)
    n_cl = int(ckeys.shape[0])
    cluster = torch.full((V,), -1, dtype=torch.int32, device=dev)
    cluster[uidx] = inverse.to(torch.int32)
    _stage(stats, "keys")
    # 7 faces; the incidences of rule 5
    tri = torch.empty(F, 3, dtype=torch.int32, device=dev)
    survive = torch.empty(F, dtype=torch.uint8, device=dev)
    inc3 = torch.empty(F, 3, dtype=torch.int32, device=dev)
    L.check(lib.ncw_mesh_sc_faces(L.ptr(f32), F, V, L.ptr(cluster), n_cl, L.ptr(tri), L.ptr(survive), L.ptr(inc3), st),
            "ncw_mesh_sc_faces")
    _stage(stats, "faces")
    # the lists: members in ascending v, incident faces in ascending f (stable sorts of ascending entries)
    order, mem_off = _csr(inverse, n_cl)
    mem = uidx[order].to(torch.int32).contiguous()
    flat = inc3.reshape(-1)
    e = torch.nonzero(flat >= 0).reshape(-1)
    order, inc_off = _csr(flat[e].long(), n_cl)
    inc = torch.div(e[order], 3, rounding_mode="floor").to(torch.int32).contiguous()
    _stage(stats, "lists")
    # 4, 5, 6, 9 placement
    cverts = torch.empty(n_cl, 3, dtype=torch.float64, device=dev)
    at_mean = torch.empty(n_cl, dtype=torch.uint8, device=dev)
    ccols = None if colors is None else torch.empty(n_cl, 3, dtype=torch.uint8, device=dev)
    L.check(lib.ncw_mesh_sc_place(L.ptr(x), L.ptr(f32), V, F, L.ptr(ckeys.contiguous()), n_cl, L.ptr(mem_off), L.ptr(mem),
                                  int(mem.shape[0]), L.ptr(inc_off), L.ptr(inc), int(inc.shape[0]), lo_c, h, n_c, eps,
                                  L.ptr(None if colors is None else colors.contiguous()), L.ptr(cverts), L.ptr(at_mean),
                                  L.ptr(ccols), st), "ncw_mesh_sc_place")
    _stage(stats, "place")
    # 7 duplicates: survivors sorted by their triple, stably, so the first of a run is the smallest input index
    sidx = torch.nonzero(survive).reshape(-1)
    keep = torch.zeros(F, dtype=torch.uint8, device=dev)
    if sidx.numel():
        t = tri[sidx].long()
        o = torch.sort(t[:, 2], stable=True).indices
        o = o[torch.sort((t[:, 0] * n_cl + t[:, 1])[o], stable=True).indices]    # < 2^62
        ts = t[o]
        first = torch.ones(o.shape[0], dtype=torch.bool, device=dev)
        first[1:] = (ts[1:] != ts[:-1]).any(1)
        keep[sidx[o[first]]] = 1
    _stage(stats, "dedup")
    # 8 output: the clusters a kept face names
    v_out, f_out, c_out, index = submesh(cverts, tri, keep, ccols)
    new_of = torch.full((n_cl + 1,), -1, dtype=torch.int64, device=dev)          # the last entry serves cluster -1
    new_of[index] = torch.arange(index.shape[0], dtype=torch.int64, device=dev)
    cluster_index = new_of[cluster.long()]
    _stage(stats, "compaction")
    if stats is not None:
        stats.update(vertices_before=V, vertices_after=int(v_out.shape[0]), faces_before=F, faces_after=int(f_out.shape[0]),
                     clusters=n_cl, clusters_at_mean=int(at_mean.sum()), at_mean=at_mean[index], list_entries=int(inc.shape[0]),
                     members=int(mem.shape[0]))
    return v_out.to(vertices.dtype), f_out, c_out, cluster_index
