"""Ray casting against a triangle mesh on the device: depth / normal views of any mesh in the format of
TSDFVolume.render, and the observed part of a ground truth - the points some camera of a run sees, occlusion included -
which mesh_metrics.compare_meshes(observed=...) keeps when it scores completion and recall.

No counterpart in the reference.  The kernel is csrc/mesh_raycast.hip (DESIGN.md "Mesh ray casting"); the numpy
statement of the same definitions is tests/raycast_numpy.py.  Valid faces are those of mesh_metrics."""
import torch

import mslam_hip as _m

from ._mesh_args import _mesh_arg, _pair, _points_arg
from ._view_args import _eye, _hw_arg, _K_arg, _poses_arg, compose_sim3, rotate  # noqa: F401 (re-exported)
from .global_volume import _render_args
from .mesh_index import MeshIndex, _index_arg, _index_ops


class _Caster:
    """A mesh with the boxes of its 128-face tiles, computed once and reused by every view; with `index` (None, True or
    a MeshIndex of the mesh) the tiles and group boxes are the index's."""

    def __init__(self, vertices, faces, validate, skip, what, index=None):
        self.index = _index_arg(MeshIndex, index, what, vertices, faces)
        self.v, self.f, self.V, self.F = _mesh_arg(vertices, faces, validate, what)
        self.device = self.v.device
        L = _m.lib()
        own = skip and self.F and self.index is None
        self.ws_bytes = int(L.mslam_mesh_raycast_workspace_bytes(self.F)) if own else 0
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device) if self.ws_bytes else None
        if self.ws_bytes:
            _m.check(L.mslam_mesh_raycast_boxes(_m.ptr(self.v), _m.ptr(self.f), self.F, self.V, _m.ptr(self.ws),
                                                self.ws_bytes, _m.stream_ptr()), "mesh_raycast_boxes")

    def cast(self, rays, h, w, pose, near, far, face=False, t64=False):
        """rays f32[h*w,3] contiguous, pose f32[8] -> (range f32[h*w], normal f32[h*w,3], hit u8[h*w], face, t64)."""
        n, dev = h * w, self.device
        rng = torch.empty(n, dtype=torch.float32, device=dev)
        nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
        hit = torch.empty(n, dtype=torch.uint8, device=dev)
        fc = torch.empty(n, dtype=torch.int32, device=dev) if face else None
        t = torch.empty(n, dtype=torch.float64, device=dev) if t64 else None
        if self.index is not None:
            _m.check(_m.lib().mslam_mesh_raycast_indexed(_m.ptr(rays), h, w, _m.ptr(pose), _m.ptr(self.v),
                                                         _m.ptr(self.f), self.F, self.V, float(near), float(far),
                                                         *_index_ops(self.index), 0, _m.ptr(rng), _m.ptr(nrm),
                                                         _m.ptr(hit), _m.ptr(fc), _m.ptr(t), _m.stream_ptr()),
                     "mesh_raycast_indexed")
            return rng, nrm, hit, fc, t
        _m.check(_m.lib().mslam_mesh_raycast(_m.ptr(rays), h, w, _m.ptr(pose), _m.ptr(self.v), _m.ptr(self.f), self.F,
                                             self.V, float(near), float(far), 1 if self.ws_bytes else 0,
                                             _m.ptr(self.ws), self.ws_bytes, _m.ptr(rng), _m.ptr(nrm), _m.ptr(hit),
                                             _m.ptr(fc), _m.ptr(t), _m.stream_ptr()), "mesh_raycast")
        return rng, nrm, hit, fc, t


def render_mesh(mesh, pose, rays=None, K=None, hw=None, near=0.05, far=10.0, skip=True, return_face=False,
                validate=True, index=None):
    """Ray cast of a triangle mesh from a camera -> (range f32[h,w], normals f32[h,w,3], hit bool[h,w]) device tensors,
    the arguments and the tuple of TSDFVolume.render (DESIGN.md "Mesh ray casting").  `mesh`: (vertices f32[V,3], faces
    i32[F,3]) device tensors or an extract_mesh tuple.  `pose`: Sim3 (8,) [t, q, s], world from camera.  Either `rays`
    f32[h,w,3], camera frame, or a pinhole `K` (3,3) with `hw`.  `range` is the ray parameter of the first hit in
    [near, far] (world units) divided by the pose's scale, so range * rays is the camera-frame pointmap; 0 on a miss.
    normals: the hit face's geometric normal, unit, world frame, towards the camera.  `skip=False` scans every face
    (same output, for checks and timing).  `return_face`: a fourth tensor i32[h,w], the face hit, -1 on a miss.
    `validate`: the index range of the faces (one host read; the kernel skips out-of-range faces either way).
    `index`: None, True or a MeshIndex of the mesh - the cast runs over its Morton-ordered tiles and group boxes, same
    output bit for bit, for faces in any order (DESIGN.md "Mesh index"); image rays are coherent and are not sorted."""
    vertices, faces = _pair(mesh, "mesh")
    caster = _Caster(vertices, faces, validate, bool(skip), "render_mesh", index)
    pose, rays, _ = _render_args(pose, rays, K, hw, near, far, 1.0, 1.0, caster.device)
    h, w = int(rays.shape[0]), int(rays.shape[1])
    rng, nrm, hit, fc, _ = caster.cast(rays, h, w, pose, near, far, face=bool(return_face))
    out = (rng.view(h, w), nrm.view(h, w, 3), hit.view(h, w).bool())
    return out + (fc.view(h, w),) if return_face else out


def observed_points(points, mesh, poses, K, hw, near=0.05, far=10.0, tol=0.01, skip=True, compact_every=4, index=None,
                    sort_queries=True):
    """bool[n] device tensor: which of the points f32[n,3] some pinhole camera sees.  A point p is observed when, for
    one of the `poses` (Sim3s [t, q, s], world from camera, rounded to f32) with origin o, all in f64: its camera-frame
    z > 0; its pixel -0.5 <= u < w - 0.5, -0.5 <= v < h - 0.5 (K (3,3), hw = (h, w), pixel centres at integers); its
    distance near <= r = |p - o| <= far; and the ray from o along the f32 unit direction to p misses `mesh` or first
    hits it at t >= r - tol (world units).  The projection and the field-of-view test are torch ops, the occlusion test
    is the ray-cast kernel on the points in view.  Points already observed leave the working set every `compact_every`
    views (0: never); a point's answer depends on nothing but the point, so the result does not depend on it.
    `index`: None, True or a MeshIndex of the mesh (DESIGN.md "Mesh index"): the casts run over it, and with
    `sort_queries` the points are worked through in the order of their Morton keys - the rays of a wave then end at
    neighbouring points - and the answers scattered back; the same answers."""
    points = _points_arg(points, "points", "observed_points")
    vertices, faces = _pair(mesh, "mesh")
    caster = _Caster(vertices, faces, True, bool(skip), "observed_points", index)
    dev = points.device
    if caster.device != dev:
        raise ValueError("observed_points: points and mesh are on different devices")
    if caster.index is not None and sort_queries and points.shape[0] > 1:
        perm = caster.index.query_order(points)
        seen = observed_points(points[perm].contiguous(), mesh, poses, K, hw, near, far, tol, skip, compact_every,
                               caster.index, False)
        return torch.empty_like(seen).index_copy_(0, perm, seen)
    poses = _poses_arg(poses, "observed_points").to(torch.float32)
    fx, fy, cx, cy = _K_arg(K, "observed_points")
    h, w = _hw_arg(hw, "observed_points")
    near, far, tol = float(near), float(far), float(tol)
    seen = torch.zeros(points.shape[0], dtype=torch.bool, device=dev)
    alive = torch.arange(points.shape[0], device=dev)
    P = points.double()
    for k, pose in enumerate(poses):
        if compact_every and k and k % int(compact_every) == 0:
            alive = alive[~seen[alive]]
        if alive.numel() == 0:
            break
        p64 = pose.to(dev).double()
        v = P[alive] - p64[:3]
        X = rotate(torch.stack((-p64[3], -p64[4], -p64[5], p64[6])), v)
        r = torch.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        u = fx * X[:, 0] / X[:, 2] + cx
        vv = fy * X[:, 1] / X[:, 2] + cy
        in_view = ((X[:, 2] > 0.0) & (u >= -0.5) & (u < w - 0.5) & (vv >= -0.5) & (vv < h - 0.5) & (r >= near) &
                   (r <= far) & ~seen[alive])
        idx = torch.nonzero(in_view).reshape(-1)
        m = int(idx.numel())
        if m == 0:
            continue
        dirs = (v[idx] / r[idx].unsqueeze(-1)).float().contiguous()
        t64 = caster.cast(dirs, 1, m, _eye(pose).to(dev), 0.0, float("inf"), t64=True)[4]
        seen[alive[idx[t64 >= r[idx] - tol]]] = True
    return seen
