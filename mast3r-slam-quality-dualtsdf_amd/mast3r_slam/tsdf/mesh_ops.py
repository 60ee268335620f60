"""Connected components of a welded triangle mesh on the device, and the filter that drops small ones ("floaters").

No counterpart in the reference.  The kernels are csrc/mesh_components.hip (DESIGN.md "Mesh components"); the numpy
statement of the same definitions is tests/cc_numpy.py.  A component's label is its smallest vertex index, dense
component ids number the components in the order of that index, a face belongs to the component of its first vertex,
and a vertex that no face uses is a component of its own with zero faces.  Works on any welded mesh (`faces` i32[F,3]
with indices in [0, V)), not only on what TSDFVolume.extract_mesh returns.
"""
import torch

import mslam_hip as _m

from ._mesh_args import _faces_arg, _mesh_tuple_arg


def _label_and_count(faces, V, F, want_vertices=True):
    """(root i32[V], counts i32[2,V]): counts[0] faces / counts[1] vertices of each component at its root's index."""
    L, stream = _m.lib(), _m.stream_ptr()
    root = torch.empty(V, dtype=torch.int32, device=faces.device)
    counts = torch.empty((2, V), dtype=torch.int32, device=faces.device)
    _m.check(L.mslam_mesh_cc_label(_m.ptr(faces), F, V, _m.ptr(root), stream), "mesh_cc_label")
    _m.check(L.mslam_mesh_cc_count(_m.ptr(faces), F, V, _m.ptr(root), _m.ptr(counts[0]),
                                   _m.ptr(counts[1]) if want_vertices else 0, 1, stream), "mesh_cc_count")
    return root, counts


def mesh_components(faces, num_vertices):
    """Connected components of the mesh `faces` i32[F,3] (device) over `num_vertices` vertices ->
    (vertex_component i32[V], face_component i32[F], component_faces i32[C], component_vertices i32[C]) device tensors.
    Components are numbered 0..C-1 in the order of their smallest vertex index.  Exact and bit-identical across repeated
    calls.  Two host reads: the index range of `faces`, and C."""
    faces, V, F = _faces_arg(faces, num_vertices, True, "mesh_components")
    dev = faces.device
    i32 = dict(dtype=torch.int32, device=dev)
    if V == 0:
        return tuple(torch.empty(0, **i32) for _ in range(4))
    if F == 0:
        return (torch.arange(V, **i32), torch.empty(0, **i32), torch.zeros(V, **i32), torch.ones(V, **i32))
    root, counts = _label_and_count(faces, V, F)
    is_root = root == torch.arange(V, **i32)
    dense = (torch.cumsum(is_root, 0) - 1).to(torch.int32)          # component id, valid at the roots
    vertex_component = dense[root.long()]
    face_component = vertex_component[faces[:, 0].long()]
    return vertex_component, face_component, counts[0][is_root], counts[1][is_root]


def _compact(per_vertex, faces, flags, V, F):
    """The compaction tail of filter_mesh and simplify_mesh: the rows of the contiguous per-vertex tensors f32[V,3] and
    of `faces` i32[F,3] (re-indexed) whose flag in `flags` i32[V + F] (vertices, then faces) is set -> (out per-vertex
    tensors, out_faces, base i32[V + F]: the output row of each flagged row, n_v).  One host read: the output sizes."""
    incl = torch.cumsum(flags, 0)                           # one scan over both flag rows; faces carry n_v in front
    n_v, n_vf = (int(x) for x in incl[[V - 1, V + F - 1]].cpu())
    n_f = n_vf - n_v
    base = incl - flags
    base[V:] -= n_v
    out = [torch.empty((n_v, 3), dtype=torch.float32, device=flags.device) for _ in per_vertex]
    out_faces = torch.empty((n_f, 3), dtype=torch.int32, device=flags.device)
    src, dst = ([_m.ptr(t) for t in ts] + [0] for ts in (per_vertex, out))     # [0]: no colours
    _m.check(_m.lib().mslam_mesh_cc_emit(src[0], src[1], src[2], _m.ptr(faces), F, V, _m.ptr(flags),
                                         _m.ptr(flags[V:]) if F else 0, _m.ptr(base), _m.ptr(base[V:]) if F else 0,
                                         dst[0], dst[1], dst[2], _m.ptr(out_faces) if n_f else 0, n_v, n_f,
                                         _m.stream_ptr()), "mesh_cc_emit")
    return out, out_faces, base, n_v


def filter_mesh(mesh, min_faces=0, keep_largest=None, _validate=True):
    """Drops whole components of `mesh` = (vertices f32[V,3], normals f32[V,3], faces i32[F,3][, colors f32[V,3]]), the
    tuple extract_mesh returns; the result has the same arity.  Keeps the components with at least `min_faces` faces;
    `keep_largest=k` then keeps only the k of them with the most faces (ties: the lower component id).  Kept vertices
    (with their normals and colours) stay in their original order and the faces are re-indexed, so a canonical mesh
    stays canonical and every kept vertex of a mesh without unused vertices is still used.  `min_faces <= 0` with
    `keep_largest=None` returns the input tensors unchanged.  Host reads: the index range of the faces, and the output
    sizes."""
    mesh = tuple(mesh)
    _mesh_tuple_arg(mesh, "filter_mesh", check=False)
    if keep_largest is not None and int(keep_largest) < 0:
        raise ValueError("filter_mesh: keep_largest must be >= 0")
    if int(min_faces) <= 0 and keep_largest is None:
        return mesh
    verts, _, faces, _, per_vertex = _mesh_tuple_arg(mesh, "filter_mesh")
    faces, V, F = _faces_arg(faces, verts.shape[0], _validate, "filter_mesh")
    if V == 0:
        return mesh
    per_vertex = [t.contiguous() for t in per_vertex]
    dev = verts.device
    root, counts = _label_and_count(faces, V, F, want_vertices=False)
    nfaces = counts[0]                                      # zero away from the roots
    is_root = root == torch.arange(V, dtype=torch.int32, device=dev)
    keep = is_root & (nfaces >= int(min_faces))
    if keep_largest is not None:
        # stable descending sort: among equal face counts the lower root index = the lower component id comes first
        order = torch.sort(torch.where(keep, nfaces, -1), stable=True, descending=True)[1][:int(keep_largest)]
        top = torch.zeros(V, dtype=torch.bool, device=dev)
        top[order] = True
        keep = keep & top
    keep_root = keep.to(torch.uint8)
    flags = torch.empty(V + F, dtype=torch.int32, device=dev)
    _m.check(_m.lib().mslam_mesh_cc_select(_m.ptr(faces), F, V, _m.ptr(root), _m.ptr(keep_root), _m.ptr(flags),
                                           _m.ptr(flags[V:]) if F else 0, _m.stream_ptr()), "mesh_cc_select")
    out, out_faces, _, _ = _compact(per_vertex, faces, flags, V, F)
    return (out[0], out[1], out_faces, *out[2:])
