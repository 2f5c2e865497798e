"""Mesh operations on the GPU: connected components and the compaction of a face subset (csrc/ncw_meshops.hip).

The reference has no such mode: its reprojection filter writes a point cloud (utils/reproj_filter.py:293-300) and nothing in
it labels the components of a mesh.  Two users here, which do the same thing -- choose a subset of faces, then compact:
  * reproj.reproj_filter(keep_faces=True) keeps the faces of the vertices the views mark (`face_select` + `submesh`);
  * mesh.extract_mesh(min_component_faces / largest_components) drops floaters before the colour pass (`clean`).

Connectivity is by SHARED VERTEX INDEX: two faces that only share coordinates are not connected, two pieces that touch in one
welded vertex are one component.  A face takes part iff its mask is set, its corners lie in [0, V) and are distinct.  The label
of a component is the smallest vertex index in it.  Everything is exact integer work, bitwise reproducible.
"""
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
