"""A spatial index for the mesh tools: the faces' Morton order, the boxes of the 128-face tiles in that order and of
the groups of 32 tiles above them, so that mesh_distance, align_meshes, render_mesh and observed_points prune their
face scans whatever order the mesh's faces are in - a ground truth from a dataset, say.  Outputs never change by a bit:
ties go to the lowest original face index (DESIGN.md "Mesh index").

No counterpart in the reference.  The kernels are csrc/mesh_index.hip and the scans of csrc/mesh_tri.h and
csrc/mesh_raycast.hip; the numpy statement of the index is tests/meshindex_numpy.py."""
import torch

import mslam_hip as _m

from ._mesh_args import _mesh_arg, _pair


class MeshIndex:
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
        L, st = _m.lib(), _m.stream_ptr()
        # the box of the vertices: plumbing, like the sort below
        self.bounds = torch.cat((self.v.amin(0), self.v.amax(0))).contiguous() if self.V else torch.zeros(
            6, dtype=torch.float32, device=dev)
        keys = torch.empty(self.F, dtype=torch.int64, device=dev)
        _m.check(L.mslam_mesh_index_keys(_m.ptr(self.v), self.V, _m.ptr(self.f), self.F, _m.ptr(self.bounds),
                                         _m.ptr(keys), st), "mesh_index_keys")
        self.order = torch.sort(keys, stable=True)[1].to(torch.int32)
        self.ws_bytes = int(L.mslam_mesh_index_bytes(self.F))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev) if self.ws_bytes else None
        _m.check(L.mslam_mesh_index_boxes(_m.ptr(self.v), _m.ptr(self.f), self.F, self.V, _m.ptr(self.order),
                                          _m.ptr(self.ws), self.ws_bytes, st), "mesh_index_boxes")

    def point_keys(self, points):
        """keys i64[n] of the points f32[n,3] (contiguous, on the index's device): their Morton codes in the mesh's box,
        a point outside it in the nearest cell.  Sorting queries by them makes neighbours of the lanes of a wave."""
        n = int(points.shape[0])
        keys = torch.empty(n, dtype=torch.int64, device=self.device)
        _m.check(_m.lib().mslam_mesh_index_point_keys(_m.ptr(points), n, _m.ptr(self.bounds), _m.ptr(keys),
                                                      _m.stream_ptr()), "mesh_index_point_keys")
        return keys

    def query_order(self, points):
        """i64[n]: the points' indices in the order of their keys (stable)."""
        return torch.sort(self.point_keys(points), stable=True)[1]

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


def _index_arg(index, vertices, faces, what):
    """index=None / True / a MeshIndex -> None or a MeshIndex checked against the mesh."""
    if index is None or index is False:
        return None
    if index is True:
        return MeshIndex(vertices, faces)
    if not isinstance(index, MeshIndex):
        raise TypeError(f"{what}: index must be None, True or a MeshIndex, got {type(index).__name__}")
    return index.check(vertices, faces, what)
