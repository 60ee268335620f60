"""Cloud smoothing on the device: the moving-least-squares projection (Levin; Alexa et al.) in its plane form - every
point moves onto the weighted least-squares plane of the cloud within a radius of it - the cloud-side twin of
smooth_mesh.  The centimetre-scale noise of the pointmaps along the viewing rays goes; points neither appear nor leave.

No counterpart in the reference.  The kernel is csrc/cloud_mls.hip (DESIGN.md "Cloud smoothing"); the numpy statement of
the same definition is tests/cloud_mls_numpy.py.  A cloud is points f32[N,3]; a point is valid when its three
coordinates are finite.  Everything is f64 on the f32 inputs in one fixed order: the sums run in the order of the walk,
the index's `order` with an index and the point order without one, so the two forms differ by rounding and each gives
the same bytes on every call.
"""
import math

import torch

import mslam_hip as _m

from ._mesh_args import _points_arg
from .cloud import CloudIndex, _colors_arg, _valid
from .mesh_index import _index_arg, _index_ops, _sorted_scan

_OUTPUTS = ((torch.float32, (3,)), (torch.float32, (3,)), (torch.float32, ()), (torch.int32, ()))


def _step(queries, points, h2, min_points, strength, query_normals, point_normals, cos_gate, index):
    """One mslam_cloud_mls_step of the checked arguments -> (points, normals, curvature, count).  The outputs are fresh
    tensors: they alias neither input."""
    n, N = int(queries.shape[0]), int(points.shape[0])

    def scan(q, qn, out, normals, curvature, count):
        _m.check(_m.lib().mslam_cloud_mls_step(_m.ptr(q), n, _m.ptr(points), N, h2, min_points, strength, _m.ptr(qn),
                                               _m.ptr(point_normals), cos_gate, *_index_ops(index), 0, _m.ptr(out),
                                               _m.ptr(normals), _m.ptr(curvature), _m.ptr(count), 0, _m.stream_ptr()),
                 "cloud_mls_step")

    return _sorted_scan(queries, index, True, _OUTPUTS, scan, (query_normals,))


def _mls_args(what, radius, min_points, strength, edge_angle):
    if not (float(radius) > 0.0 and math.isfinite(float(radius))):
        raise ValueError(f"{what}: radius must be positive and finite, got {radius}")
    if isinstance(min_points, bool) or int(min_points) != min_points or int(min_points) < 1:
        raise ValueError(f"{what}: min_points must be an integer >= 1, got {min_points!r}")
    if not 0.0 <= float(strength) <= 1.0:
        raise ValueError(f"{what}: strength must be in [0, 1], got {strength}")
    cos_gate = 0.0
    if edge_angle is not None:
        if not 0.0 <= float(edge_angle) <= 90.0:
            raise ValueError(f"{what}: edge_angle must be in [0, 90] degrees, got {edge_angle}")
        cos_gate = math.cos(math.radians(float(edge_angle)))
    return float(radius) * float(radius), int(min_points), float(strength), cos_gate


def _result(out):
    points, normals, curvature, count = out
    return dict(points=points, normals=normals, curvature=curvature, count=count, moved=~torch.isnan(curvature))


def cloud_mls(queries, points, radius, min_points=6, strength=1.0, normals=None, edge_angle=None, index=True):
    """One step of the MLS plane projection of the queries f32[n,3] onto the cloud `points` f32[N,3] -> a dict of device
    tensors: points f32[n,3], normals f32[n,3], curvature f32[n], count i32[n], moved bool[n].

    A valid point q of the cloud JOINS query p when its squared distance d2 (cloud_distance's f64 sum) is
    <= float(radius)^2; its weight is (1 - d2 / radius^2)^2, so a point on the rim counts with weight 0.  The weighted
    centroid m (relative to p) and covariance of the joining points give the plane: its normal n is the unit
    eigenvector of the smallest eigenvalue (f64, cyclic Jacobi), turned so that its largest component is positive, and
    the query moves to p + strength ((n . m) n), `strength` in [0, 1].  curvature is the surface variation
    l_min / (l0 + l1 + l2) and count the joining points, not capped.  A query STAYS - the same bits, normal (0, 0, 0),
    curvature NaN, moved False - when it is invalid, when count < min_points, when count < 3 or when the neighbourhood
    is coincident or collinear (the middle eigenvalue <= 2^-40 of the largest).

    `normals` = (query_normals f32[n,3], point_normals f32[N,3]) and `edge_angle` in degrees in [0, 90] go together: a
    point then joins only when |cos| of the angle between its normal and the query's is >= cos(edge_angle), whatever
    the signs.  A query whose normal is zero or non-finite is not gated; a point whose normal is zero or non-finite
    joins no gated query (at edge_angle < 90).  `index`: None, True or a CloudIndex of the tensor.  The sums run in the
    index's order, or in the point order with index=None: the two differ by rounding, each is the same bytes on every
    call (DESIGN.md "Cloud smoothing")."""
    what = "cloud_mls"
    h2, min_points, strength, cos_gate = _mls_args(what, radius, min_points, strength, edge_angle)
    if (normals is None) != (edge_angle is None):
        raise ValueError(f"{what}: normals and edge_angle go together")
    queries = _points_arg(queries, "queries", what)
    index = _index_arg(CloudIndex, index, what, points)
    points = _points_arg(points, "points", what)
    if queries.device != points.device:
        raise ValueError(f"{what}: queries and points are on different devices")
    qn = pn = None
    if normals is not None:
        if not isinstance(normals, (tuple, list)) or len(normals) != 2:
            raise ValueError(f"{what}: normals must be the pair (query_normals, point_normals)")
        qn, pn = _points_arg(normals[0], "query_normals", what), _points_arg(normals[1], "point_normals", what)
        if qn.shape != queries.shape or pn.shape != points.shape:
            raise ValueError(f"{what}: normals must be ({int(queries.shape[0])},3) and ({int(points.shape[0])},3), got "
                             f"{tuple(qn.shape)} and {tuple(pn.shape)}")
        if qn.device != points.device or pn.device != points.device:
            raise ValueError(f"{what}: normals and points are on different devices")
    return _result(_step(queries, points, h2, min_points, strength, qn, pn, cos_gate, index))


def smooth_cloud(points, radius, iterations=1, min_points=6, strength=1.0, edge_angle=None, colors=None, index=True):
    """The cloud `points` f32[N,3] smoothed by `iterations` MLS steps -> (points f32[N,3], colors or None, info).

    The surface is that of the INPUT cloud throughout - one index, built once: q_0 = points and q_{t+1} =
    cloud_mls(q_t, points, ...)["points"], so the cloud does not shrink onto itself step after step.  With `edge_angle`
    (degrees) one ungated step of the cloud in itself first gives every point's normal at the same radius, and every
    step is then gated by it: point j pulls row i only when their normals stand within edge_angle of each other (up to
    sign), which keeps a wall from rounding the floor's edge.  Row i's own normal stays fixed across the iterations.
    Order, count, `colors` (u8[N,3], returned as they are) and invalid rows are untouched.  radius, min_points,
    strength and index as in cloud_mls.

    info: moved bool[N] (the row moved in some iteration), normals f32[N,3], curvature f32[N] and count i32[N] of the
    last step (device tensors), and n_valid, rms_displacement, max_displacement - Python numbers from one host read,
    the displacement from the input to the output over the valid rows in f64."""
    what = "smooth_cloud"
    h2, min_points, strength, cos_gate = _mls_args(what, radius, min_points, strength, edge_angle)
    if isinstance(iterations, bool) or int(iterations) != iterations or int(iterations) < 1:
        raise ValueError(f"{what}: iterations must be an integer >= 1, got {iterations!r}")
    index = _index_arg(CloudIndex, index, what, points)
    points = _points_arg(points, "points", what)
    N = int(points.shape[0])
    if colors is not None:
        colors = _colors_arg(colors, N, what)
    nrm = None
    if edge_angle is not None:
        nrm = _step(points, points, h2, min_points, strength, None, None, 0.0, index)[1]
    q, moved, last = points, torch.zeros(N, dtype=torch.bool, device=points.device), None
    for _ in range(int(iterations)):
        last = _result(_step(q, points, h2, min_points, strength, nrm, nrm, cos_gate, index))
        q, moved = last["points"], moved | last["moved"]
    ok = _valid(points)
    d = torch.where(ok[:, None], q.double() - points.double(), 0.0)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    n_valid, total, worst = torch.stack([ok.sum().double(), d2.sum(), d2.max() if N else d2.sum()]).tolist()
    info = dict(moved=moved, normals=last["normals"], curvature=last["curvature"], count=last["count"],
                n_valid=int(n_valid), rms_displacement=math.sqrt(total / n_valid) if n_valid else 0.0,
                max_displacement=math.sqrt(worst))
    return q, colors, info
