"""Numpy statement of the mesh ray caster (DESIGN.md "Mesh ray casting"; the kernel is csrc/mesh_raycast.hip) and of
the observed rule of mast3r_slam.tsdf.observed_points.  Everything is f64 on the f32 inputs, and the operation order
written here is the kernel's: no sum is reassociated and a * b - c is two roundings.

The intersection is the two-sided watertight test of Woop, Benthin and Wald (2013).  Valid faces are those of
meshdist_numpy.triangles.  Among the valid faces hit at near <= t <= far the smallest t wins, then the lowest index."""
import numpy as np

from meshdist_numpy import _cross, _dot, triangles


def rotate(q, r):
    """r + w u + q x u with u = 2 q x r (not renormalised), grouped as csrc/tsdf_render.hip groups it."""
    u0 = 2.0 * (q[1] * r[..., 2] - q[2] * r[..., 1])
    u1 = 2.0 * (q[2] * r[..., 0] - q[0] * r[..., 2])
    u2 = 2.0 * (q[0] * r[..., 1] - q[1] * r[..., 0])
    return np.stack([(r[..., 0] + q[3] * u0) + (q[1] * u2 - q[2] * u1),
                     (r[..., 1] + q[3] * u1) + (q[2] * u0 - q[0] * u2),
                     (r[..., 2] + q[3] * u2) + (q[0] * u1 - q[1] * u0)], -1)


def directions(pose, rays):
    """(o f64[3], d f64[n,3], s) of the f32 pose [t, q, s] and the f32 camera-frame rays."""
    p = np.asarray(pose, np.float32).astype(np.float64).reshape(8)
    r = np.asarray(rays, np.float32).astype(np.float64).reshape(-1, 3)
    return p[:3], rotate(p[3:7], r), p[7]


def _take(a, k):
    return np.take_along_axis(a, k[:, None], 1)[:, 0]


def cast(o, d, vertices, faces, near, far):
    """(t64 f64[n], face i32[n]) of the rays o + t d; +inf and -1 on a miss.  A ray with a zero or non-finite direction
    misses."""
    a, b, c, valid = triangles(vertices, faces)
    n = len(d)
    ad = np.abs(d)
    ok = np.isfinite(d).all(1) & (ad > 0.0).any(1)
    kz = np.where(ad[:, 1] > ad[:, 0], 1, 0)
    kz = np.where(ad[:, 2] > _take(ad, kz), 2, kz)            # the first axis of largest |d|
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    with np.errstate(all="ignore"):
        dz = _take(d, kz)
        kx, ky = np.where(dz < 0.0, ky, kx), np.where(dz < 0.0, kx, ky)
        Sx, Sy, Sz = _take(d, kx) / dz, _take(d, ky) / dz, 1.0 / dz
        best = np.full(n, np.inf)
        face = np.full(n, -1, np.int32)
        for f in np.flatnonzero(valid):
            x, y, z = [], [], []
            for v in (a[f], b[f], c[f]):
                q = v - o
                x.append(q[kx] - Sx * q[kz])
                y.append(q[ky] - Sy * q[kz])
                z.append(Sz * q[kz])
            U = x[2] * y[1] - y[2] * x[1]
            V = x[0] * y[2] - y[0] * x[2]
            W = x[1] * y[0] - y[1] * x[0]
            det = (U + V) + W
            t = ((U * z[0] + V * z[1]) + W * z[2]) / det
            one_sign = ((U >= 0.0) & (V >= 0.0) & (W >= 0.0)) | ((U <= 0.0) & (V <= 0.0) & (W <= 0.0))
            hit = ok & one_sign & (det != 0.0) & (t >= near) & (t <= far) & (t < best)
            best = np.where(hit, t, best)
            face = np.where(hit, np.int32(f), face)
    return best, face


def render(pose, rays, vertices, faces, near=0.05, far=10.0):
    """(range f32[n], normal f32[n,3], hit u8[n], face i32[n], t64 f64[n]) as mslam_mesh_raycast writes them."""
    o, d, s = directions(pose, rays)
    t64, face = cast(o, d, vertices, faces, near, far)
    hit = face >= 0
    a, b, c, _ = triangles(vertices, faces)
    g = np.where(hit, face, 0)
    if len(a) == 0:
        nrm = np.zeros((len(d), 3))
    else:
        nrm = _cross(b[g] - a[g], c[g] - a[g])
    with np.errstate(all="ignore"):
        unit = nrm / np.sqrt(_dot(nrm, nrm))[:, None]
        unit = np.where((_dot(nrm, d) > 0.0)[:, None], -unit, unit)          # towards the origin
        rng = np.where(hit, t64 / s, 0.0).astype(np.float32)
    normal = np.where(hit[:, None], unit, 0.0).astype(np.float32)
    return rng, normal, hit.astype(np.uint8), face, t64


def compose(T, pose):
    """The Sim3 T o pose in f64: s_T R_T t + t_T, q_T x q, s_T s (poses moved into another frame)."""
    T, p = np.asarray(T, np.float64).reshape(8), np.asarray(pose, np.float64).reshape(8)
    a, b = T[3:7], p[3:7]
    q = np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                  a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                  a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3],
                  a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])
    return np.concatenate([T[7] * rotate(a, p[:3]) + T[:3], q, [T[7] * p[7]]])


def view_rays(point, pose, K, hw, near, far):
    """One view of the observed rule -> (in_view bool[n], dirs f32[n,3], r f64[n]): the points in front of the camera,
    inside the image (pixel centres at integers) and at a distance r = |p - o| in [near, far]; the unit direction from o
    to p rounded to f32, the occlusion ray.  The pose's scale cancels in u, v and, being positive, keeps the sign of z."""
    p = np.asarray(pose, np.float32).astype(np.float64).reshape(8)
    K = np.asarray(K, np.float64).reshape(3, 3)
    h, w = hw
    v = np.asarray(point, np.float32).astype(np.float64).reshape(-1, 3) - p[:3]
    X = rotate(np.array([-p[3], -p[4], -p[5], p[6]]), v)
    r = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    with np.errstate(all="ignore"):
        u = K[0, 0] * X[:, 0] / X[:, 2] + K[0, 2]
        vv = K[1, 1] * X[:, 1] / X[:, 2] + K[1, 2]
        dirs = (v / r[:, None]).astype(np.float32)
    in_view = ((X[:, 2] > 0.0) & (u >= -0.5) & (u < w - 0.5) & (vv >= -0.5) & (vv < h - 0.5) & (r >= near) & (r <= far))
    return in_view, dirs, r


def observed(points, vertices, faces, poses, K, hw, near=0.05, far=10.0, tol=0.01):
    """bool[n]: the point is in some view (view_rays) and the ray from that view's origin towards it misses the mesh or
    first hits it at t64 >= r - tol."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    seen = np.zeros(len(points), bool)
    for pose in np.asarray(poses, np.float32).reshape(-1, 8):
        in_view, dirs, r = view_rays(points, pose, K, hw, near, far)
        idx = np.flatnonzero(in_view)
        o = pose[:3].astype(np.float64)
        t64, _ = cast(o, dirs[idx].astype(np.float64), vertices, faces, 0.0, np.inf)
        seen[idx[t64 >= r[idx] - tol]] = True
    return seen
