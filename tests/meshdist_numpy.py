"""Numpy statement of the mesh-quality definitions (DESIGN.md "Mesh quality"; the kernels are csrc/mesh_distance.hip):
face areas, the stratified area-weighted surface sampler with its counter hash, the exact point-to-triangle-mesh
distance by Voronoi regions (Ericson, Real-Time Collision Detection 5.1.5) and the accuracy / completion metrics.
Everything is f64 on the f32 inputs, and the operation order written here is the kernel's: no sum is reassociated and
a * b + c is two roundings.

A face is valid when its three indices lie in [0, V) and (b - a) x (c - a) is not exactly zero.  An invalid face has
area 0, is never sampled and is never the nearest face."""
import numpy as np

MASK64 = (1 << 64) - 1


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def triangles(vertices, faces):
    """(a, b, c f64[F,3], valid bool[F]); the corners of an invalid face are zeros."""
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    in_range = ((f >= 0) & (f < len(v))).all(1)
    g = np.where(in_range[:, None], f, 0)
    if len(v) == 0:
        z = np.zeros((len(f), 3))
        return z, z.copy(), z.copy(), np.zeros(len(f), bool)
    a, b, c = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    n = _cross(b - a, c - a)
    valid = in_range & (n != 0.0).any(1)
    a, b, c = (np.where(valid[:, None], x, 0.0) for x in (a, b, c))
    return a, b, c, valid


def face_areas(vertices, faces):
    a, b, c, valid = triangles(vertices, faces)
    n = _cross(b - a, c - a)
    return np.where(valid, 0.5 * np.sqrt(_dot(n, n)), 0.0)


def hash64(seed, i):
    """splitmix64 of seed + (i + 1) * 0x9E3779B97F4A7C15, all modulo 2^64.  i: uint64 array."""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & MASK64) + (np.asarray(i, np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def barycentrics(seed, i):
    """(r1, r2) f64 of sample i: the top 24 bits and bits 16..39 of the hash, times 2^-24, folded into the triangle."""
    z = hash64(seed, i)
    r1 = (z >> np.uint64(40)).astype(np.float64) * 2.0 ** -24
    r2 = ((z >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    fold = r1 + r2 > 1.0
    return np.where(fold, 1.0 - r1, r1), np.where(fold, 1.0 - r2, r2)


def sample(vertices, faces, cdf, n, seed=0):
    """n samples -> (points f32[n,3], face i32[n]).  cdf f64[F]: the inclusive cumulative face areas; the total is
    cdf[-1].  Sample i takes u = (i + 0.5) / n * total and the first face with cdf[f] > u by bisection, then steps back
    to the last valid face at or before it, so a face without area is never chosen."""
    a, b, c, valid = triangles(vertices, faces)
    cdf = np.asarray(cdf, np.float64)
    F = len(cdf)
    i = np.arange(n)
    u = (i.astype(np.float64) + 0.5) / np.float64(n) * cdf[-1]
    lo, hi = np.zeros(n, np.int64), np.full(n, F, np.int64)
    while (lo < hi).any():
        act = lo < hi
        mid = np.where(act, lo + (hi - lo) // 2, 0)
        up = cdf[mid] > u
        hi = np.where(act & up, mid, hi)
        lo = np.where(act & ~up, mid + 1, lo)
    f = np.minimum(lo, F - 1)
    prev_valid = np.maximum.accumulate(np.where(valid, np.arange(F), 0))     # last valid face at or before each face
    f = prev_valid[f]
    r1, r2 = barycentrics(seed, i.astype(np.uint64))
    p = (a[f] + r1[:, None] * (b[f] - a[f])) + r2[:, None] * (c[f] - a[f])
    return p.astype(np.float32), f.astype(np.int32)


def tri_dist2(p, a, b, c):
    """Squared distance from the points p f64[n,3] to ONE triangle a, b, c f64[3]: the region tests in Ericson's order
    (vertex A, vertex B, edge AB, vertex C, edge AC, edge BC, interior), the first that holds decides."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    e1, e2 = d4 - d3, d5 - d6
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = e1 / (e1 + e2)
        denom = 1.0 / ((va + vb) + vc)
        v, w = vb * denom, vc * denom
        q = (a + ab * v[:, None]) + ac * w[:, None]                                     # interior
        cases = [(va <= 0.0) & (e1 >= 0.0) & (e2 >= 0.0), b + w_bc[:, None] * (c - b),
                 (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), a + w_ac[:, None] * ac,
                 (d6 >= 0.0) & (d5 <= d6), np.broadcast_to(c, p.shape),
                 (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), a + v_ab[:, None] * ab,
                 (d3 >= 0.0) & (d4 <= d3), np.broadcast_to(b, p.shape),
                 (d1 <= 0.0) & (d2 <= 0.0), np.broadcast_to(a, p.shape)]
        for cond, point in zip(cases[0::2], cases[1::2]):          # lowest priority first: the last written wins
            q = np.where(cond[:, None], point, q)
        r = p - q
        return _dot(r, r)


def closest(points, vertices, faces):
    """(dist2 f64[n], nearest i32[n]): the smallest squared distance from each point (f32) to a valid face and the lowest
    index of a face that attains it: faces in ascending order, strict `<`.  No valid face: +inf and -1."""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    a, b, c, valid = triangles(vertices, faces)
    best = np.full(len(p), np.inf)
    nearest = np.full(len(p), -1, np.int32)
    for f in np.flatnonzero(valid):
        d = tri_dist2(p, a[f], b[f], c[f])
        better = d < best
        best = np.where(better, d, best)
        nearest = np.where(better, np.int32(f), nearest)
    return best, nearest


def metrics(d_pred_to_gt, d_gt_to_pred, threshold, pred_area, gt_area):
    """The dict of compare_meshes from the two distance arrays (distances, not squares)."""
    dp, dg = np.asarray(d_pred_to_gt, np.float64), np.asarray(d_gt_to_pred, np.float64)
    assert len(dp) == len(dg)
    accuracy, completion = float(dp.sum() / len(dp)), float(dg.sum() / len(dg))
    precision, recall = float((dp <= threshold).sum() / len(dp)), float((dg <= threshold).sum() / len(dg))
    fscore = 2.0 * precision * recall / (precision + recall) if precision + recall > 0.0 else 0.0
    return dict(accuracy=accuracy, accuracy_median=float(np.median(dp)), completion=completion,
                completion_median=float(np.median(dg)), precision=precision, recall=recall, fscore=fscore,
                chamfer=0.5 * (accuracy + completion), n_samples=len(dp), threshold=float(threshold),
                pred_area=float(pred_area), gt_area=float(gt_area))
