"""Views of a point cloud on the device: the z-buffer splat of a cloud into pinhole views - range, index, hit and colour
images in the format of render_mesh - and the observed part of a cloud, the points some camera of a run sees with the
cloud itself as the occluder, which cloud.compare_clouds(observed=...) keeps when it scores completion and recall
against a scan without faces.

No counterpart in the reference.  The kernels are csrc/cloud_view.hip (DESIGN.md "Cloud views"); the numpy statement of
the same definitions is tests/cloudview_numpy.py.  A splat needs a projection, so every function here takes a pinhole
`K`; the ray-image model of an uncalibrated camera has none."""
import math

import numpy as np
import torch

import mslam_hip as _m

from ._mesh_args import _points_arg
from ._view_args import _hw_arg, _K_arg, _poses_arg, _range_arg, compose_sim3

MAX_RADIUS = _m.header_constants()["MSLAM_CLOUD_VIEW_MAX_RADIUS"]


def _view_args(what, K, hw, near, far, radius, point_size, max_radius):
    """((fx, fy, cx, cy), h, w, near, far, radius, point_size (-1.0: none), max_radius), checked: the camera by
    _view_args.py, the footprint of a point here."""
    k4, (h, w), (near, far) = _K_arg(K, what), _hw_arg(hw, what), _range_arg(near, far, what, strict=False)
    for name, v in (("radius", radius), ("max_radius", max_radius)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{what}: {name} must be an integer, got {v!r}")
    radius, max_radius = int(radius), int(max_radius)
    if not 0 <= radius <= max_radius <= MAX_RADIUS:
        raise ValueError(f"{what}: need 0 <= radius <= max_radius <= {MAX_RADIUS}, got radius {radius} and max_radius "
                         f"{max_radius}")
    if point_size is not None and not (float(point_size) >= 0.0 and math.isfinite(float(point_size))):
        raise ValueError(f"{what}: point_size must be None or a finite world-unit diameter >= 0, got {point_size!r}")
    size = -1.0 if point_size is None else float(point_size)
    return k4, h, w, near, far, radius, size, max_radius


def _check_pixels(what, V, h, w):
    if V * h * w >= 1 << 31:
        raise ValueError(f"{what}: {V} views of {h} x {w} pixels are outside the int32 index range")


def _splat(points, poses, k4, h, w, near, far, radius, size, max_radius, zbuf, counters=None):
    """mslam_cloud_view_splat of the checked arguments into zbuf u64 (held as i64)[>= V h w]; poses f32[V,8] on the
    device."""
    _m.check(_m.lib().mslam_cloud_view_splat(_m.ptr(points), int(points.shape[0]), _m.ptr(poses), int(poses.shape[0]),
                                             *k4, h, w, near, far, radius, size, max_radius, _m.ptr(zbuf),
                                             _m.ptr(counters), _m.stream_ptr()), "cloud_view_splat")


def render_cloud(points, pose, K, hw, colors=None, near=0.05, far=10.0, radius=0, point_size=None, max_radius=8):
    """Z-buffer splat of the cloud `points` f32[N,3] (a device tensor) into a pinhole view -> (range f32[h,w], index
    i32[h,w], hit bool[h,w]) device tensors, and with `colors` u8[N,3] a fourth, rgb u8[h,w,3] (DESIGN.md "Cloud views").
    `pose`: Sim3 (8,) [t, q, s], world from camera, or a batch [M,8], which returns stacked [M,h,w] tensors.  `K` (3,3),
    `hw` = (h, w), pixel centres at integers.

    A point is in the view when its camera-frame z > 0, its projection lies in the image and its distance r from the
    camera centre is in [near, far] (world units).  It covers the square of half-width rho pixels around its pixel:
    rho = `radius`, or with `point_size` (a world-unit diameter) min(max_radius, max(radius, floor(point_size / 2 *
    max(fx, fy) / z))), so that a point keeps its size in the world.  Per pixel the point of the smallest f32(r) wins,
    then the lowest index: `index` is that point (-1 on a miss), `range` is f32(r) divided by the pose's scale, so that
    range * ray is the camera-frame point as for render_mesh (0 on a miss), rgb its colour (0 on a miss).  The image does
    not depend on the order of the points and is the same bytes on every call.  Holes between points are not filled."""
    what = "render_cloud"
    points = _points_arg(points, "points", what)
    dev, N = points.device, int(points.shape[0])
    if colors is not None:
        from .cloud import _colors_arg

        colors = _colors_arg(colors, N, what)
        if colors.device != dev:
            raise ValueError(f"{what}: points and colors are on different devices")
    pose = getattr(pose, "data", pose)
    if not torch.is_tensor(pose):
        pose = torch.as_tensor(np.asarray(pose, np.float64))
    single = pose.dim() <= 1                                                 # a 2-D pose is a batch, also [1,8]
    if pose.dim() > 2 or (single and pose.numel() != 8):
        raise ValueError(f"{what}: pose must be a Sim3 (8,) [t, q, s] or a batch (M,8), got shape {tuple(pose.shape)}")
    poses = _poses_arg(pose, what).to(device=dev, dtype=torch.float32).contiguous()
    k4, h, w, near, far, radius, size, max_radius = _view_args(what, K, hw, near, far, radius, point_size, max_radius)
    V = int(poses.shape[0])
    _check_pixels(what, V, h, w)
    zbuf = torch.empty((V, h, w), dtype=torch.int64, device=dev)
    _splat(points, poses, k4, h, w, near, far, radius, size, max_radius, zbuf)
    rng = torch.empty((V, h, w), dtype=torch.float32, device=dev)
    idx = torch.empty((V, h, w), dtype=torch.int32, device=dev)
    hit = torch.empty((V, h, w), dtype=torch.uint8, device=dev)
    rgb = torch.empty((V, h, w, 3), dtype=torch.uint8, device=dev) if colors is not None else None
    _m.check(_m.lib().mslam_cloud_view_resolve(_m.ptr(zbuf), _m.ptr(poses), V, h, w, _m.ptr(colors), N, _m.ptr(rng),
                                               _m.ptr(idx), _m.ptr(hit), _m.ptr(rgb), _m.stream_ptr()),
             "cloud_view_resolve")
    out = (rng, idx, hit.bool()) + ((rgb,) if rgb is not None else ())
    return tuple(t[0] for t in out) if single else out


def _tol_arg(what, tol, rel_tol, point_size):
    """tol None: 2 point_size with a point_size, else 0.01, observed_points' default."""
    tol = (2.0 * float(point_size) if point_size is not None else 0.01) if tol is None else float(tol)
    rel_tol = float(rel_tol)
    if not (tol >= 0.0 and rel_tol >= 0.0):
        raise ValueError(f"{what}: tol and rel_tol must be >= 0, got {tol} and {rel_tol}")
    return tol, rel_tol


def observed_cloud_points(points, cloud, poses, K, hw, near=0.05, far=10.0, tol=None, rel_tol=0.0, radius=0,
                          point_size=None, max_radius=8, chunk=8):
    """bool[n] device tensor: which of the points f32[n,3] some pinhole camera sees, with the cloud `cloud` f32[N,3] as
    the occluder (the points need not belong to it; both device tensors).  `poses`: Sim3s [t, q, s], world from camera,
    rounded to f32; `K` (3,3), `hw` = (h, w).  The cloud is splatted into every view (render_cloud's rule and its
    `radius`, `point_size`, `max_radius`); a point p is observed by a view when it is in the view and its own pixel is
    empty or f32(r_p) <= r_win (1 + rel_tol) + tol for the f32 range r_win that won the pixel (world units).  With
    tol = rel_tol = 0 a point that wins its pixel sees itself.

    `tol` None: 2 point_size with a point_size - a footprint of half-width point_size / 2 on a surface tilted theta from
    frontal spans (point_size / 2) tan theta in range, and 2 point_size admits theta up to atan 4, about 76 degrees -
    else 0.01, observed_points' default.  The price: anything closer than `tol` behind a surface counts as seen.  A
    fixed pixel `radius` depends on the resolution and leaks between the points of a near surface; `point_size`, about
    twice the cloud's spacing, does not (DESIGN.md "Cloud views").

    The views are worked through `chunk` at a time: one splat and one visibility launch per chunk, into one z-buffer of
    chunk h w u64 that is reused, and nothing is read back.  The result does not depend on `chunk`."""
    what = "observed_cloud_points"
    points = _points_arg(points, "points", what)
    cloud = _points_arg(cloud, "cloud", what)
    dev = points.device
    if cloud.device != dev:
        raise ValueError(f"{what}: points and cloud are on different devices")
    if isinstance(chunk, bool) or int(chunk) != chunk or int(chunk) < 1:
        raise ValueError(f"{what}: chunk must be an integer >= 1, got {chunk!r}")
    poses = _poses_arg(poses, what).to(device=dev, dtype=torch.float32).contiguous()
    k4, h, w, near, far, radius, size, max_radius = _view_args(what, K, hw, near, far, radius, point_size, max_radius)
    tol, rel_tol = _tol_arg(what, tol, rel_tol, point_size)
    V, n = int(poses.shape[0]), int(points.shape[0])
    chunk = max(1, min(int(chunk), V))
    _check_pixels(what, chunk, h, w)
    seen = torch.zeros(n, dtype=torch.uint8, device=dev)
    zbuf = torch.empty(chunk * h * w, dtype=torch.int64, device=dev)
    L, st = _m.lib(), _m.stream_ptr()
    for k in range(0, V, chunk):
        part = poses[k:k + chunk]                                            # rows of a contiguous tensor: contiguous
        _splat(cloud, part, k4, h, w, near, far, radius, size, max_radius, zbuf)
        _m.check(L.mslam_cloud_view_visible(_m.ptr(points), n, _m.ptr(zbuf), _m.ptr(part), int(part.shape[0]), *k4,
                                            h, w, near, far, tol, rel_tol, _m.ptr(seen), st), "cloud_view_visible")
    return seen.bool()


_OBSERVED_KEYS = {"poses", "K", "hw", "near", "far", "tol", "rel_tol", "radius", "point_size", "max_radius", "frame"}


def _observed_cloud(what, gt, observed, T, voxel):
    """bool[n]: the points of the (thinned) ground-truth cloud that the cameras of compare_clouds' `observed` see, the
    cloud itself the occluder; T: the alignment transform or None."""
    spec = dict(observed)
    if set(spec) - _OBSERVED_KEYS or not {"poses", "K", "hw"} <= set(spec):
        raise ValueError(f"{what}: observed needs poses, K and hw (and takes near, far, tol, rel_tol, radius, "
                         f"point_size, max_radius, frame); got {sorted(spec)}")
    frame = spec.pop("frame", "gt")
    if frame not in ("gt", "pred"):
        raise ValueError(f"{what}: observed['frame'] must be 'gt' or 'pred', got {frame!r}")
    if spec.get("point_size") is None:
        if voxel is not None:
            spec["point_size"] = 2.0 * float(voxel)
        elif spec.get("radius") is None:
            raise ValueError(f"{what}: observed needs the size of a point: give voxel (point_size is then 2 voxel), "
                             "or point_size or radius in observed")
    if spec.get("radius") is None:
        spec.pop("radius", None)
    poses = _poses_arg(spec.pop("poses"), what)
    if frame == "pred" and T is not None:
        poses = compose_sim3(T, poses)
    return observed_cloud_points(gt, gt, poses, spec.pop("K"), spec.pop("hw"), **spec)
