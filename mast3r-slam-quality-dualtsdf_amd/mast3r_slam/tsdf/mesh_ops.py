"""Connected components of a welded triangle mesh on the device, and the filter that drops small ones ("floaters").

No counterpart in the reference.  The kernels are csrc/mesh_components.hip (DESIGN.md "Mesh components"); the numpy
statement of the same definitions is tests/cc_numpy.py.  A component's label is its smallest vertex index, dense
component ids number the components in the order of that index, a face belongs to the component of its first vertex,
and a vertex that no face uses is a component of its own with zero faces.  Works on any welded mesh (`faces` i32[F,3]
with indices in [0, V)), not only on what TSDFVolume.extract_mesh returns.
"""
import torch

import mslam_hip as _m


def _faces_arg(faces, num_vertices, validate, what):
    """faces as a contiguous i32[F,3] device tensor; `validate`: the index range, one reduction and one host read."""
    if not torch.is_tensor(faces):
        raise TypeError(f"{what}: faces must be a device tensor")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: faces must be (F,3), got {tuple(faces.shape)}")
    _m.require_dtype(faces, torch.int32, "faces")
    faces = faces.contiguous()
    V, F = int(num_vertices), int(faces.shape[0])
    if V < 0 or V >= 1 << 31 or 3 * F >= 1 << 31:
        raise ValueError(f"{what}: {V} vertices / {F} faces are outside the int32 index range")
    if validate and F > 0:
        _m.ptr(faces)                                       # a host tensor raises here: no CPU path exists
        lo, hi = (int(x) for x in torch.stack(torch.aminmax(faces)).cpu())
        if lo < 0 or hi >= V:
            raise ValueError(f"{what}: face indices span [{lo}, {hi}], outside [0, {V})")
    return faces, V, F


def _label_and_count(faces, V, F, want_vertices=True):
    """(root i32[V], counts i32[2,V]): counts[0] faces / counts[1] vertices of each component at its root's index."""
    L = _m.lib()
    stream = _m.stream_ptr()
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


def filter_mesh(mesh, min_faces=0, keep_largest=None, _validate=True):
    """Drops whole components of `mesh` = (vertices f32[V,3], normals f32[V,3], faces i32[F,3][, colors f32[V,3]]), the
    tuple extract_mesh returns; the result has the same arity.  Keeps the components with at least `min_faces` faces;
    `keep_largest=k` then keeps only the k of them with the most faces (ties: the lower component id).  Kept vertices
    (with their normals and colours) stay in their original order and the faces are re-indexed, so a canonical mesh
    stays canonical and every kept vertex of a mesh without unused vertices is still used.  `min_faces <= 0` with
    `keep_largest=None` returns the input tensors unchanged.  Host reads: the index range of the faces, and the output
    sizes."""
    mesh = tuple(mesh)
    if len(mesh) not in (3, 4):
        raise ValueError(f"filter_mesh: mesh must hold 3 or 4 tensors, got {len(mesh)}")
    if keep_largest is not None and int(keep_largest) < 0:
        raise ValueError("filter_mesh: keep_largest must be >= 0")
    if int(min_faces) <= 0 and keep_largest is None:
        return mesh
    verts, normals, faces = mesh[:3]
    colors = mesh[3] if len(mesh) == 4 else None
    per_vertex = [verts, normals] + ([colors] if colors is not None else [])
    for name, t in zip(("vertices", "normals", "colors"), per_vertex):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3 or t.shape[0] != verts.shape[0]:
            raise ValueError(f"filter_mesh: {name} must be ({int(verts.shape[0])},3)")
        _m.require_dtype(t, torch.float32, name)
    faces, V, F = _faces_arg(faces, verts.shape[0], _validate, "filter_mesh")
    if V == 0:
        return mesh
    verts, normals = verts.contiguous(), normals.contiguous()
    colors = colors.contiguous() if colors is not None else None
    dev = verts.device
    L = _m.lib()
    stream = _m.stream_ptr()
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
    _m.check(L.mslam_mesh_cc_select(_m.ptr(faces), F, V, _m.ptr(root), _m.ptr(keep_root), _m.ptr(flags),
                                    _m.ptr(flags[V:]) if F else 0, stream), "mesh_cc_select")
    incl = torch.cumsum(flags, 0)                           # one scan over both flag rows; faces carry V' in front
    n_v, n_vf = (int(x) for x in incl[[V - 1, V + F - 1]].cpu())
    n_f = n_vf - n_v
    base = incl - flags
    base[V:] -= n_v
    out = [torch.empty((n_v, 3), dtype=torch.float32, device=dev) for _ in per_vertex]
    out_faces = torch.empty((n_f, 3), dtype=torch.int32, device=dev)
    _m.check(L.mslam_mesh_cc_emit(_m.ptr(verts), _m.ptr(normals), _m.ptr(colors), _m.ptr(faces), F, V, _m.ptr(flags),
                                  _m.ptr(flags[V:]) if F else 0, _m.ptr(base), _m.ptr(base[V:]) if F else 0,
                                  _m.ptr(out[0]), _m.ptr(out[1]), _m.ptr(out[2]) if colors is not None else 0,
                                  _m.ptr(out_faces) if n_f else 0, n_v, n_f, stream), "mesh_cc_emit")
    return (out[0], out[1], out_faces) + ((out[2],) if colors is not None else ())
