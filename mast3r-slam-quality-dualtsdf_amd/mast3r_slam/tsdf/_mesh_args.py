"""Argument checks shared by mesh_ops, mesh_simplify, mesh_smooth, mesh_holes, mesh_metrics and mesh_align; `what`, the
caller's name, is the prefix of every message.  There is no CPU path: a host tensor raises in mslam_hip.ptr.  Below them
the sampler's core: mesh_metrics and mesh_align both draw from it, and mesh_metrics imports mesh_align."""
import math

import numpy as np
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


def _mesh_arg(vertices, faces, validate, what):
    """(vertices f32[V,3], faces i32[F,3], V, F) contiguous device tensors; `validate`: the index range of the faces,
    one reduction and one host read."""
    if not torch.is_tensor(vertices):
        raise TypeError(f"{what}: vertices must be a device tensor")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{what}: vertices must be (V,3), got {tuple(vertices.shape)}")
    _m.require_dtype(vertices, torch.float32, "vertices")
    _m.ptr(vertices)                                        # a host tensor raises here: no CPU path exists
    faces, V, F = _faces_arg(faces, vertices.shape[0], validate, what)
    _m.ptr(faces)
    if faces.device != vertices.device:
        raise ValueError(f"{what}: vertices and faces are on different devices")
    return vertices.contiguous(), faces, V, F


def _mesh_tuple_arg(mesh, what, check=True, on_device=False):
    """extract_mesh's tuple -> (verts, normals, faces, colors or None, per_vertex = [verts, normals(, colors)]).
    `check` False: the arity alone, for a caller's "off" path; `on_device`: a host tensor raises here."""
    if len(mesh) not in (3, 4):
        raise ValueError(f"{what}: mesh must hold 3 or 4 tensors, got {len(mesh)}")
    verts, normals, faces, colors = (mesh + (None,))[:4]
    per_vertex = [verts, normals] + ([colors] if colors is not None else [])
    for name, t in zip(("vertices", "normals", "colors"), per_vertex if check else ()):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3 or t.shape[0] != verts.shape[0]:
            raise ValueError(f"{what}: {name} must be ({int(verts.shape[0])},3)")
        _m.require_dtype(t, torch.float32, name)
        if on_device:
            _m.ptr(t)
    return verts, normals, faces, colors, per_vertex


def _bool_arg(value, name, what):
    """A switch such as fill_holes' `bowties` / extract_mesh's `fill_bowties`: a bool (numpy's too), nothing else."""
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"{what}: {name} must be a bool, got {value!r}")
    return bool(value)


def _ranges(verts, faces, *more):
    """(lowest and highest coordinate, lowest and highest face index, all coordinates finite) of a non-empty mesh as
    Python floats: one stacked reduction, one host read.  `more`: further 0-d tensors that ride along in that read."""
    vlo, vhi = torch.aminmax(verts)
    flo, fhi = torch.aminmax(faces)
    finite = torch.isfinite(verts).all()
    return torch.stack([x.double() for x in (vlo, vhi, flo, fhi, finite) + more]).cpu().tolist()


def _check_finite(what, vlo, vhi, finite):
    if not finite or not (math.isfinite(vlo) and math.isfinite(vhi)):
        raise ValueError(f"{what}: vertex coordinates span [{vlo}, {vhi}] and are not all finite")


def _check_face_range(what, flo, fhi, V):
    if flo < 0 or fhi >= V:
        raise ValueError(f"{what}: face indices span [{int(flo)}, {int(fhi)}], outside [0, {V})")


def _points_arg(x, name, what, device=None):
    """f32[n,3] contiguous device tensor; numpy arrays and lists are moved to `device` (there is no CPU path)."""
    if not torch.is_tensor(x):
        if device is None:
            raise TypeError(f"{what}: {name} must be a device tensor")
        x = torch.as_tensor(np.asarray(x, np.float32)).to(device)
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{what}: {name} must be (n,3), got {tuple(x.shape)}")
    _m.require_dtype(x, torch.float32, name)
    _m.ptr(x)
    if x.shape[0] >= 1 << 31:
        raise ValueError(f"{what}: too many points for the int32 index range")
    return x.contiguous()


def _sim3_arg(T, what, device, dtype):
    """A Sim3 given as a tensor, array or sequence of 8 numbers (or a lietorch Sim3) -> tensor[8] on the device."""
    T = getattr(T, "data", T)
    T = T.detach().to(device=device, dtype=dtype) if torch.is_tensor(T) else torch.as_tensor(
        np.asarray(T, np.float64), dtype=dtype, device=device)
    if T.numel() != 8:
        raise ValueError(f"{what}: a Sim3 is 8 numbers [t(3), q(xyzw), s], got shape {tuple(T.shape)}")
    return T.reshape(8).contiguous()


def _pair(mesh, what):
    mesh = tuple(mesh)
    if len(mesh) == 2:
        return mesh
    if len(mesh) in (3, 4):                                  # extract_mesh: (vertices, normals, faces[, colors])
        return mesh[0], mesh[2]
    raise ValueError(f"compare_meshes: {what} must be (vertices, faces) or an extract_mesh tuple")


def _areas(vertices, faces, V, F):
    area = torch.empty(F, dtype=torch.float64, device=vertices.device)
    _m.check(_m.lib().mslam_mesh_face_areas(_m.ptr(vertices), _m.ptr(faces), F, V, _m.ptr(area), _m.stream_ptr()),
             "mesh_face_areas")
    return area


def _sample(vertices, faces, V, F, n, seed, what):
    """(points, face, total area as a Python float).  One host read: the total."""
    n = int(n)
    if n < 1 or n >= 1 << 31:
        raise ValueError(f"{what}: n must be in [1, 2^31), got {n}")
    dev = vertices.device
    cdf = torch.cumsum(_areas(vertices, faces, V, F), 0) if F else torch.zeros(0, dtype=torch.float64, device=dev)
    total = float(cdf[-1]) if F else 0.0
    if not (total > 0.0 and total < float("inf")):
        raise ValueError(f"{what}: the mesh has no area to sample (total area {total})")
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    _m.check(_m.lib().mslam_mesh_sample(_m.ptr(vertices), _m.ptr(faces), F, V, _m.ptr(cdf), total, n,
                                        int(seed) & ((1 << 64) - 1), _m.ptr(points), _m.ptr(face), _m.stream_ptr()),
             "mesh_sample")
    return points, face, total
