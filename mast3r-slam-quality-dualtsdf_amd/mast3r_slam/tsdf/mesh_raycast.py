"""Ray casting against a triangle mesh on the device: depth / normal views of any mesh in the format of
TSDFVolume.render, and the observed part of a ground truth - the points some camera of a run sees, occlusion included -
which mesh_metrics.compare_meshes(observed=...) keeps when it scores completion and recall.

No counterpart in the reference.  The kernel is csrc/mesh_raycast.hip (DESIGN.md "Mesh ray casting"); the numpy
statement of the same definitions is tests/raycast_numpy.py.  Valid faces are those of mesh_metrics."""
import numpy as np
import torch

import mslam_hip as _m

from ._mesh_args import _mesh_arg, _pair, _points_arg
from .global_volume import _render_args
from .mesh_index import MeshIndex, _index_arg


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
            ix = self.index
            _m.check(_m.lib().mslam_mesh_raycast_indexed(_m.ptr(rays), h, w, _m.ptr(pose), _m.ptr(self.v),
                                                         _m.ptr(self.f), self.F, self.V, float(near), float(far),
                                                         _m.ptr(ix.order), _m.ptr(ix.ws), ix.ws_bytes, 2, 0,
                                                         _m.ptr(rng), _m.ptr(nrm), _m.ptr(hit), _m.ptr(fc), _m.ptr(t),
                                                         _m.stream_ptr()), "mesh_raycast_indexed")
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


def _rotate(q, r):
    u0 = 2.0 * (q[1] * r[:, 2] - q[2] * r[:, 1])
    u1 = 2.0 * (q[2] * r[:, 0] - q[0] * r[:, 2])
    u2 = 2.0 * (q[0] * r[:, 1] - q[1] * r[:, 0])
    return torch.stack(((r[:, 0] + q[3] * u0) + (q[1] * u2 - q[2] * u1),
                        (r[:, 1] + q[3] * u1) + (q[2] * u0 - q[0] * u2),
                        (r[:, 2] + q[3] * u2) + (q[0] * u1 - q[1] * u0)), -1)


def _poses_arg(poses, what):
    """f32[n,8] on the host, from a tensor, an array or a sequence of Sim3s (lietorch Sim3s included)."""
    if not torch.is_tensor(poses) and not isinstance(poses, np.ndarray):
        poses = [p if isinstance(p, np.ndarray) else getattr(p, "data", p) for p in poses]
        poses = torch.stack([torch.as_tensor(p).detach().reshape(8).to("cpu", torch.float64) for p in poses]) \
            if len(poses) else torch.zeros((0, 8), dtype=torch.float64)
    poses = torch.as_tensor(poses).detach().to("cpu")
    if poses.numel() % 8 != 0:
        raise ValueError(f"{what}: poses must be (n,8) Sim3s [t, q, s], got shape {tuple(poses.shape)}")
    return poses.reshape(-1, 8)


def compose_sim3(T, poses):
    """T o pose for poses f64[n,8] and one Sim3 T (8 numbers), in f64 on the host: the cameras of a map moved into the
    frame an alignment leads to."""
    T = torch.as_tensor(T, dtype=torch.float64).detach().to("cpu").reshape(8)
    p = poses.to(torch.float64)
    a, b = T[3:7], p[:, 3:7]
    q = torch.stack((a[3] * b[:, 0] + a[0] * b[:, 3] + a[1] * b[:, 2] - a[2] * b[:, 1],
                     a[3] * b[:, 1] - a[0] * b[:, 2] + a[1] * b[:, 3] + a[2] * b[:, 0],
                     a[3] * b[:, 2] + a[0] * b[:, 1] - a[1] * b[:, 0] + a[2] * b[:, 3],
                     a[3] * b[:, 3] - a[0] * b[:, 0] - a[1] * b[:, 1] - a[2] * b[:, 2]), -1)
    return torch.cat((T[7] * _rotate(a, p[:, :3]) + T[:3], q, (T[7] * p[:, 7]).unsqueeze(-1)), -1)


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
    Kd = torch.as_tensor(np.asarray(torch.as_tensor(K).detach().cpu(), np.float64)).reshape(3, 3).tolist()
    h, w = (int(x) for x in hw)
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
        X = _rotate(torch.stack((-p64[3], -p64[4], -p64[5], p64[6])), v)
        r = torch.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        u = Kd[0][0] * X[:, 0] / X[:, 2] + Kd[0][2]
        vv = Kd[1][1] * X[:, 1] / X[:, 2] + Kd[1][2]
        in_view = ((X[:, 2] > 0.0) & (u >= -0.5) & (u < w - 0.5) & (vv >= -0.5) & (vv < h - 0.5) & (r >= near) &
                   (r <= far) & ~seen[alive])
        idx = torch.nonzero(in_view).reshape(-1)
        m = int(idx.numel())
        if m == 0:
            continue
        dirs = (v[idx] / r[idx].unsqueeze(-1)).float().contiguous()
        eye = torch.cat((pose[:3], pose.new_tensor([0.0, 0.0, 0.0, 1.0, 1.0]))).to(dev).contiguous()
        t64 = caster.cast(dirs, 1, m, eye, 0.0, float("inf"), t64=True)[4]
        seen[alive[idx[t64 >= r[idx] - tol]]] = True
    return seen
