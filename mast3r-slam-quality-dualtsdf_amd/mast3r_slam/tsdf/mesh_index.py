"""A spatial index for the mesh tools: the faces' Morton order, the boxes of the 128-face tiles in that order and of
the groups of 32 tiles above them, so that mesh_distance, align_meshes, render_mesh and observed_points prune their
face scans whatever order the mesh's faces are in - a ground truth from a dataset, say.  Outputs never change by a bit:
ties go to the lowest original face index (DESIGN.md "Mesh index").

No counterpart in the reference.  The kernels are csrc/mesh_index.hip and the scans of csrc/mesh_tri.h and
csrc/mesh_raycast.hip; the numpy statement of the index is tests/meshindex_numpy.py."""
import torch

import mslam_hip as _m

from ._mesh_args import _mesh_arg, _pair


class _SpatialIndex:
    """What MeshIndex and CloudIndex (cloud.py) share: `device`, `bounds` f32[6] (the box the Morton keys are taken in),
    `order` i32[n] (the elements by key, from a stable sort), and `ws` / `ws_bytes`, the workspace of the boxes of the
    128-element tiles in that order and of the groups of 32 tiles.  A subclass checks its arguments, sets `device` and
    `bounds`, forms its elements' keys and calls _build; it keeps its own `check`."""

    def _build(self, keys, n, name, source):
        """`order` from the keys i64[n], then the workspace: mslam_<name>_bytes(n) and mslam_<name>_boxes(*source, order,
        workspace, bytes, stream)."""
        L = _m.lib()
        self.order = torch.sort(keys, stable=True)[1].to(torch.int32)
        self.ws_bytes = int(getattr(L, f"mslam_{name}_bytes")(n))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device) if self.ws_bytes else None
        _m.check(getattr(L, f"mslam_{name}_boxes")(*source, _m.ptr(self.order), _m.ptr(self.ws), self.ws_bytes,
                                                   _m.stream_ptr()), f"{name}_boxes")

    def point_keys(self, points):
        """keys i64[n] of the points f32[n,3] (contiguous, on the index's device): their Morton codes in `bounds`, a
        point outside it in the nearest cell.  Sorting queries by them makes neighbours of the lanes of a wave."""
        n = int(points.shape[0])
        keys = torch.empty(n, dtype=torch.int64, device=self.device)
        _m.check(_m.lib().mslam_mesh_index_point_keys(_m.ptr(points), n, _m.ptr(self.bounds), _m.ptr(keys),
                                                      _m.stream_ptr()), "mesh_index_point_keys")
        return keys

    def query_order(self, points):
        """i64[n]: the points' indices in the order of their keys (stable)."""
        return torch.sort(self.point_keys(points), stable=True)[1]


class MeshIndex(_SpatialIndex):
    """The index of the mesh (vertices f32[V,3], faces i32[F,3], device tensors), built once and passed as `index=` to
    mesh_distance, compare_meshes, align_meshes, render_mesh and observed_points for that same mesh.  It keeps the two
    tensors (they are never copied or permuted), `order` i32[F] - the faces by the Morton code of their centroids,
    invalid faces last, from a stable sort - and the workspace of boxes.  `validate`: the index range of the faces
    (one host read; the kernels skip out-of-range faces either way)."""

    def __init__(self, vertices, faces, validate=True):
        what = "MeshIndex"
        self.shapes = (tuple(vertices.shape), tuple(faces.shape)) if torch.is_tensor(vertices) and torch.is_tensor(
            faces) else None
        self.pointers = (vertices.data_ptr(), faces.data_ptr()) if self.shapes else None
        self.v, self.f, self.V, self.F = _mesh_arg(vertices, faces, validate, what)
        dev = self.device = self.v.device
        # the box of the vertices: plumbing, like the sort below
        self.bounds = torch.cat((self.v.amin(0), self.v.amax(0))).contiguous() if self.V else torch.zeros(
            6, dtype=torch.float32, device=dev)
        keys = torch.empty(self.F, dtype=torch.int64, device=dev)
        _m.check(_m.lib().mslam_mesh_index_keys(_m.ptr(self.v), self.V, _m.ptr(self.f), self.F, _m.ptr(self.bounds),
                                                _m.ptr(keys), _m.stream_ptr()), "mesh_index_keys")
        self._build(keys, self.F, "mesh_index", (_m.ptr(self.v), _m.ptr(self.f), self.F, self.V))

    def check(self, vertices, faces, what):
        """Raises ValueError unless the index was built for these very tensors: the same shapes and data pointers."""
        same = (torch.is_tensor(vertices) and torch.is_tensor(faces) and self.shapes is not None
                and (tuple(vertices.shape), tuple(faces.shape)) == self.shapes
                and ((vertices.data_ptr(), faces.data_ptr()) == self.pointers
                     or (vertices.data_ptr(), faces.data_ptr()) == (self.v.data_ptr(), self.f.data_ptr())))
        if not same:
            raise ValueError(f"{what}: the MeshIndex was built for another mesh (shapes or data pointers differ)")
        return self


def build_mesh_index(mesh, validate=True):
    """MeshIndex of `mesh`: (vertices, faces) device tensors or an extract_mesh tuple."""
    return MeshIndex(*_pair(mesh, "mesh"), validate=validate)


def _index_arg(cls, index, what, *tensors):
    """index=None / True / an index of class `cls` (MeshIndex, CloudIndex) -> None or one checked against `tensors`,
    the mesh's vertices and faces or the cloud's points."""
    if index is None or index is False:
        return None
    if index is True:
        return cls(*tensors)
    if not isinstance(index, cls):
        raise TypeError(f"{what}: index must be None, True or a {cls.__name__}, got {type(index).__name__}")
    return index.check(*tensors, what)


def _index_ops(index, levels=2):
    """The operands (order, index, index_bytes, levels) of a C entry point that takes an index; without one the plain
    scan: no order, no boxes, and levels 1, which it does not read.  An entry point without `levels` takes [:3]."""
    if index is None:
        return 0, 0, 0, 1
    return _m.ptr(index.order), _m.ptr(index.ws), index.ws_bytes, levels


_NEAREST = ((torch.float64, ()), (torch.int32, ()))     # a nearest-element scan's outputs: dist2 f64[n], nearest i32[n]


def _sorted_scan(queries, index, sort_queries, outputs, scan, extras=()):
    """The tensors of `outputs`, a (dtype, trailing shape) each - (torch.int32, (k,)) is i32[n,k] - from
    scan(q, *extras, *outs), the call that fills them for the queries q f32[n,3].  With an index, `sort_queries` and more
    than one query, q is the queries in the order of their Morton keys, `extras` (per-query tensors or None) go with
    them, and the results are scattered back."""
    n, dev = int(queries.shape[0]), queries.device
    outs = [torch.empty((n, *tail), dtype=dtype, device=dev) for dtype, tail in outputs]
    perm = index.query_order(queries) if index is not None and sort_queries and n > 1 else None
    if perm is None:
        scan(queries, *extras, *outs)
        return tuple(outs)
    scan(queries[perm].contiguous(), *(None if e is None else e[perm].contiguous() for e in extras), *outs)
    return tuple(torch.empty_like(o).index_copy_(0, perm, o) for o in outs)
