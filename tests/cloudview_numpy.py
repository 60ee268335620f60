"""Numpy statement of the cloud views (DESIGN.md "Cloud views"; the kernels are csrc/cloud_view.hip): the z-buffer splat
of a point cloud into pinhole views, its resolve into range / index / hit / rgb images, and the observed rule of
mast3r_slam.tsdf.observed_cloud_points.  Everything is f64 on the f32 inputs and the operation order written here is the
kernels': no sum is reassociated and a * b + c is two roundings.  The projection is raycast_numpy.view_rays', with its
grouping of sums and its rotate.

A pixel's z-buffer entry is the minimum of (bits of f32(r) as u32) << 32 | index over the points whose footprint covers
it, all ones when none does: the nearest f32 range wins, then the lowest index, whatever order the points arrive in."""
import numpy as np

from raycast_numpy import rotate

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_RADIUS = 8                       # MSLAM_CLOUD_VIEW_MAX_RADIUS


def _k4(K):
    K = np.asarray(K, np.float64).reshape(3, 3)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def project(points, pose, K, hw, near, far):
    """One view -> (in_view bool[n], px i64[n], py i64[n], r f64[n], X2 f64[n]); px, py are 0 where not in view.  A
    point with a non-finite coordinate is in no view, and every comparison with a NaN is false."""
    p = np.asarray(pose, np.float32).astype(np.float64).reshape(8)
    fx, fy, cx, cy = _k4(K)
    h, w = hw
    pts = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        v = pts - p[:3]
        X = rotate(np.array([-p[3], -p[4], -p[5], p[6]]), v)
        r = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        u = fx * X[:, 0] / X[:, 2] + cx
        vv = fy * X[:, 1] / X[:, 2] + cy
        in_view = (np.isfinite(pts).all(1) & (X[:, 2] > 0.0) & (u >= -0.5) & (u < w - 0.5) & (vv >= -0.5)
                   & (vv < h - 0.5) & (r >= near) & (r <= far))
        px = np.where(in_view, np.floor(u + 0.5), 0.0).astype(np.int64)
        py = np.where(in_view, np.floor(vv + 0.5), 0.0).astype(np.int64)
    return in_view, px, py, r, X[:, 2]


def footprint(X2, K, radius, point_size, max_radius):
    """rho i64[n] of points in view: `radius`, or with a world-unit diameter point_size
    min(max_radius, max(radius, floor(0.5 point_size max(fx, fy) / X2))), the min taken in f64."""
    if point_size is None:
        return np.full(len(X2), int(radius), np.int64)
    fx, fy, _, _ = _k4(K)
    with np.errstate(all="ignore"):
        g = np.floor(0.5 * float(point_size) * max(fx, fy) / X2)
    return np.minimum(float(max_radius), np.maximum(float(radius), g)).astype(np.int64)


def range_bits(r):
    """The u32 bit patterns of f32(r) as u64."""
    with np.errstate(all="ignore"):
        return np.asarray(r, np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)


def splat(points, poses, K, hw, near=0.05, far=10.0, radius=0, point_size=None, max_radius=MAX_RADIUS):
    """zbuf u64[V,h,w]."""
    poses = np.asarray(poses, np.float32).reshape(-1, 8)
    h, w = hw
    zbuf = np.full((len(poses), h, w), EMPTY, np.uint64)
    for k, pose in enumerate(poses):
        in_view, px, py, r, X2 = project(points, pose, K, hw, near, far)
        idx = np.flatnonzero(in_view)
        if len(idx) == 0:
            continue
        rho = footprint(X2[idx], K, radius, point_size, max_radius)
        key = (range_bits(r[idx]) << np.uint64(32)) | idx.astype(np.uint64)
        flat = zbuf[k].reshape(-1)
        R = int(rho.max())
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                x, y = px[idx] + dx, py[idx] + dy
                ok = (rho >= max(abs(dx), abs(dy))) & (x >= 0) & (x < w) & (y >= 0) & (y < h)
                np.minimum.at(flat, (y * w + x)[ok], key[ok])
    return zbuf


def resolve(zbuf, poses, colors=None):
    """(range f32[V,h,w], index i32[V,h,w], hit u8[V,h,w][, rgb u8[V,h,w,3]]) of a z-buffer: range = f32(f64(r32) / s),
    0 on a miss; index -1 on a miss; rgb the winner's colour, 0 on a miss."""
    poses = np.asarray(poses, np.float32).reshape(-1, 8)
    zbuf = np.asarray(zbuf, np.uint64)
    hit = zbuf != EMPTY
    index = np.where(hit, (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    r32 = (zbuf >> np.uint64(32)).astype(np.uint32).view(np.float32)
    s = poses[:, 7].astype(np.float64)[:, None, None]
    with np.errstate(all="ignore"):
        rng = np.where(hit, r32.astype(np.float64) / s, 0.0).astype(np.float32)
    out = (rng, index, hit.astype(np.uint8))
    if colors is not None:
        colors = np.asarray(colors, np.uint8).reshape(-1, 3)
        rgb = np.zeros(hit.shape + (3,), np.uint8)
        if len(colors):
            rgb = np.where(hit[..., None], colors[np.where(hit, index, 0)], 0).astype(np.uint8)
        out += (rgb,)
    return out


def visible(queries, zbuf, poses, K, hw, near=0.05, far=10.0, tol=0.01, rel_tol=0.0, seen=None):
    """seen u8[m]: 1 where some view observes the query - it is in the view, and its own pixel is empty or
    f64(f32(r_q)) <= f64(r32 of the pixel) (1 + rel_tol) + tol.  `seen`: the start (rows already 1 stay 1)."""
    poses = np.asarray(poses, np.float32).reshape(-1, 8)
    queries = np.asarray(queries, np.float32).reshape(-1, 3)
    seen = np.zeros(len(queries), np.uint8) if seen is None else np.array(seen, np.uint8)
    for k, pose in enumerate(poses):
        in_view, px, py, r, _ = project(queries, pose, K, hw, near, far)
        z = np.asarray(zbuf[k], np.uint64)[py, px]
        win = (z >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
        with np.errstate(all="ignore"):
            own = r.astype(np.float32).astype(np.float64)
            ok = in_view & ((z == EMPTY) | (own <= win * (1.0 + float(rel_tol)) + float(tol)))
        seen[ok] = 1
    return seen


def default_tol(tol, point_size):
    """tol None: 2 point_size with a point_size, else 0.01 (observed_points')."""
    if tol is not None:
        return float(tol)
    return 2.0 * float(point_size) if point_size is not None else 0.01


def observed(queries, cloud, poses, K, hw, near=0.05, far=10.0, tol=None, rel_tol=0.0, radius=0, point_size=None,
             max_radius=MAX_RADIUS):
    """bool[m]: the queries some view observes through the splat of `cloud`."""
    zbuf = splat(cloud, poses, K, hw, near, far, radius, point_size, max_radius)
    return visible(queries, zbuf, poses, K, hw, near, far, default_tol(tol, point_size), rel_tol).astype(bool)
