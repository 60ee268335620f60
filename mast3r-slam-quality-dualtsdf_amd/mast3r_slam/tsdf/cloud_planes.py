"""Which planes a point cloud consists of, by sequential RANSAC on the device, and the planarity figures that need no
ground truth: how flat the flat parts of a map are, how much of the map lies on them, how square they stand to each
other.

No counterpart in the reference.  The kernels are csrc/cloud_planes.hip (DESIGN.md "Cloud planes"); the numpy statement
of the same definitions is tests/cloud_planes_numpy.py.  A cloud is points f32[N,3]; a point is valid when its three
coordinates are finite.  Everything about coordinates is f64 on the f32 inputs in one fixed order, the counts are
integers, and the result is a function of the cloud, the parameters and the seed: the same bytes on every call.
"""
import math

import numpy as np
import torch

import mslam_hip as _m

from ._mesh_args import _points_arg
from .cloud import _k_arg, _valid, cloud_normals

_C = _m.header_constants()
MAX_HYPOTHESES = _C["MSLAM_CLOUD_PLANES_MAX_HYPOTHESES"]
MAX_PLANES = _C["MSLAM_CLOUD_PLANES_MAX_PLANES"]
ROW = _C["MSLAM_CLOUD_PLANES_ROW"]
STATE = _C["MSLAM_CLOUD_PLANES_STATE"]


def _int_arg(value, name, what, lo, hi=None):
    if isinstance(value, bool) or int(value) != value or int(value) < lo or (hi is not None and int(value) > hi):
        raise ValueError(f"{what}: {name} must be an integer " + (f">= {lo}" if hi is None else f"in [{lo}, {hi}]")
                         + f", got {value!r}")
    return int(value)


def _normals_arg(normals, points, viewpoint, what):
    """None, a k (cloud_normals(points, k)) or f32[N,3] on the points' device -> None or the tensor."""
    if normals is None:
        return None
    if not torch.is_tensor(normals):
        return cloud_normals(points, _k_arg(normals, what, "normals (a neighbour count)"), viewpoint=viewpoint)[0]
    if tuple(normals.shape) != tuple(points.shape):
        raise ValueError(f"{what}: normals must be ({int(points.shape[0])},3), got {tuple(normals.shape)}")
    _m.require_dtype(normals, torch.float32, "normals")
    _m.ptr(normals)
    if normals.device != points.device:
        raise ValueError(f"{what}: normals and points are on different devices")
    return normals.contiguous()


def cloud_planes(points, tol, normals=None, normal_angle=None, max_planes=16, min_points=100, hypotheses=1024,
                 refit_iterations=2, seed=0, viewpoint=None):
    """The planes of the cloud `points` f32[N,3] -> dict of device tensors and n_planes (a Python int, the one host read).

    Up to `max_planes` rounds, each of which finds one plane among the REMAINING points - the valid points without a
    label, in ascending order.  A round draws `hypotheses` planes through three remaining points each (SplitMix64 of
    seed, round, hypothesis and slot, mod the list's length), counts for each the remaining points within `tol` of it,
    takes the one with the most (the lowest hypothesis on ties), refits it `refit_iterations` times to the covariance
    of its supporters - a refit that is degenerate or supports fewer points is not taken - and labels its supporters.
    The call ends with the first round whose best count is below `min_points`, or when fewer than max(3, min_points)
    points remain.  With `normals` - f32[N,3], or a k for cloud_normals(points, k) - a point supports a plane only if
    its normal is finite, not zero and within `normal_angle` radians (in [0, pi/2], default pi/6) of the plane's, either
    way round.  Planes are numbered in discovery order; n and d are negated together so that `viewpoint` (3 numbers)
    lies on the positive side or, without one, so that n's largest component is positive.

    labels i32[N] (-1: on no plane), planes f64[P,4] (unit n, d: n . x + d = 0), counts i32[P], rmse f64[P],
    centroids f64[P,3], eigenvalues f64[P,3] (of the supporters' covariance, in the order of the Jacobi columns),
    sum_r2 f64[P], n_planes = P.  `tol` is finite and > 0, hypotheses in [1, 1024], max_planes in [1, 64],
    min_points >= 1, seed any integer (taken mod 2^64).  Not split into connected patches: cloud_clusters on a plane's
    points does that (DESIGN.md "Cloud planes")."""
    what = "cloud_planes"
    if not (float(tol) > 0.0 and math.isfinite(float(tol))):
        raise ValueError(f"{what}: tol must be positive and finite, got {tol}")
    hypotheses = _int_arg(hypotheses, "hypotheses", what, 1, MAX_HYPOTHESES)
    max_planes = _int_arg(max_planes, "max_planes", what, 1, MAX_PLANES)
    min_points = _int_arg(min_points, "min_points", what, 1)
    refit_iterations = _int_arg(refit_iterations, "refit_iterations", what, 0, 64)
    if isinstance(seed, bool) or int(seed) != seed:
        raise ValueError(f"{what}: seed must be an integer, got {seed!r}")
    if normals is None and normal_angle is not None:
        raise ValueError(f"{what}: normal_angle needs normals")
    cos_angle = 0.0
    if normals is not None:
        angle = math.pi / 6.0 if normal_angle is None else float(normal_angle)
        if not 0.0 <= angle <= math.pi / 2.0:
            raise ValueError(f"{what}: normal_angle must be in [0, pi/2], got {normal_angle}")
        cos_angle = min(1.0, max(0.0, math.cos(angle)))
    points = _points_arg(points, "points", what)
    N, dev = int(points.shape[0]), points.device
    vp = None
    if viewpoint is not None:
        vp = viewpoint if torch.is_tensor(viewpoint) else torch.as_tensor(np.asarray(viewpoint, np.float32))
        if vp.numel() != 3:
            raise ValueError(f"{what}: viewpoint must be 3 numbers, got {tuple(vp.shape)}")
        vp = vp.detach().to(device=dev, dtype=torch.float32).reshape(3).contiguous()
    normals = _normals_arg(normals, points, vp, what)
    L, st = _m.lib(), _m.stream_ptr()
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    rows = torch.zeros((max_planes, ROW), dtype=torch.float64, device=dev)
    state = torch.zeros(STATE, dtype=torch.int32, device=dev)
    nbytes = int(L.mslam_cloud_planes_workspace_bytes(N, hypotheses))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _m.check(L.mslam_cloud_planes(_m.ptr(points), _m.ptr(normals), N, float(tol), cos_angle, max_planes, min_points,
                                  hypotheses, refit_iterations, int(seed) & ((1 << 64) - 1), _m.ptr(vp), _m.ptr(ws),
                                  nbytes, _m.ptr(labels), _m.ptr(rows), _m.ptr(state), st), "cloud_planes")
    P = int(state[1])                                                         # the host read
    rows = rows[:P]
    return dict(labels=labels, planes=rows[:, :4].contiguous(), counts=rows[:, 4].to(torch.int32),
                rmse=rows[:, 12].contiguous(), centroids=rows[:, 6:9].contiguous(),
                eigenvalues=rows[:, 9:12].contiguous(), sum_r2=rows[:, 5].contiguous(), n_planes=P)


def _host(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def plane_figures(result, points=None):
    """Host floats from cloud_planes' result (at most 64 rows): plane_share, the labelled points over the valid points
    of `points` (None: every point counts as valid); plane_rmse over all labelled points, from the planes' sums of r^2;
    n_planes; manhattan_deg, the mean over pairs of planes, weighted by the product of their counts, of the distance of
    the angle between their normals to the nearer of 0 and 90 degrees - 0 for a box, and 0 without a pair."""
    n = _host(result["planes"]).astype(np.float64).reshape(-1, 4)[:, :3]
    c = _host(result["counts"]).astype(np.float64)
    if "sum_r2" in result:
        sum_r2 = _host(result["sum_r2"]).astype(np.float64)
    else:
        sum_r2 = _host(result["rows"]).astype(np.float64).reshape(-1, ROW)[:, 5]
    if points is None:
        n_valid = int(result["labels"].shape[0])
    else:
        n_valid = int(_valid(points).sum()) if torch.is_tensor(points) else int(np.isfinite(np.asarray(points)).all(1).sum())
    total = float(c.sum())
    num = den = 0.0
    for i in range(len(n)):
        for j in range(i + 1, len(n)):
            a = math.degrees(math.acos(min(1.0, abs(float(n[i] @ n[j])))))
            num += c[i] * c[j] * min(a, 90.0 - a)
            den += c[i] * c[j]
    return dict(plane_share=total / n_valid if n_valid else 0.0,
                plane_rmse=float(math.sqrt(sum_r2.sum() / total)) if total else 0.0,
                n_planes=int(len(n)), manhattan_deg=float(num / den) if den else 0.0)
