"""Numpy statement of the k nearest neighbours, the normals and the outlier rules of a point cloud (DESIGN.md "Point
clouds"; the kernels are csrc/cloud_knn.hip, the Python layer mast3r_slam/tsdf/cloud.py).  Everything is f64 on the f32
inputs, and the operation order written here is the kernel's: one multiply or add at a time, sums in list order."""
import math

import numpy as np

import cloud_numpy as C

MAX_K = 32                         # MSLAM_CLOUD_KNN_MAX_K of include/mslam_hip.h


# ----------------------------------------------------------------------------------------------------------------------
# k nearest neighbours
# ----------------------------------------------------------------------------------------------------------------------
def knn(queries, points, k, exclude=None, chunk=256):
    """(dist2 f64[n,k], neighbors i32[n,k]): row i is the k smallest valid points under the total order (dist2, index),
    ascending - np.lexsort with dist2 the primary key and the index the secondary.  exclude i32[n]: the point with that
    index is left out of the row (an entry outside [0, N): nothing).  (+inf, -1) in the slots beyond the points that
    qualify and in the row of a query with a non-finite coordinate."""
    q, p = C.f32(queries), C.f32(points)
    n, N = len(q), len(p)
    ok_p, ok_q = C.valid(p), C.valid(q)
    dist2 = np.full((n, k), np.inf)
    nb = np.full((n, k), -1, np.int32)
    if N == 0 or n == 0:
        return dist2, nb
    index = np.arange(N)
    for s in range(0, n, chunk):
        d = C.dist2_matrix(q[s:s + chunk], p)
        d[:, ~ok_p] = np.inf                                   # a real distance is finite: +inf marks "not a candidate"
        d[~ok_q[s:s + chunk]] = np.inf
        if exclude is not None:
            e = np.asarray(exclude, np.int64)[s:s + chunk]
            rows = np.flatnonzero((e >= 0) & (e < N))
            d[rows, e[rows]] = np.inf
        order = np.lexsort((np.broadcast_to(index, d.shape), d), axis=-1)[:, :k]
        got = np.take_along_axis(d, order, 1)
        m = order.shape[1]
        dist2[s:s + chunk, :m] = got
        nb[s:s + chunk, :m] = np.where(np.isinf(got), -1, order)
    return dist2, nb


# ----------------------------------------------------------------------------------------------------------------------
# normals
# ----------------------------------------------------------------------------------------------------------------------
PAIRS = ((0, 1), (0, 2), (1, 2))


def jacobi3(A, sweeps=16):
    """Cyclic Jacobi on the symmetric matrices A f64[M,3,3], ma_jacobi4 of csrc/mesh_align.hip restated for 3 x 3 ->
    (A after the sweeps, its diagonal the eigenvalues; V, its columns the eigenvectors).  Per matrix: before each sweep
    the squares of the off-diagonal and of the diagonal entries are summed in row-major order and the matrix stops for
    good unless off > 2^-104 diag; a pair whose entry is exactly zero is skipped."""
    A = np.array(A, np.float64).reshape(-1, 3, 3).copy()
    M = len(A)
    V = np.tile(np.eye(3), (M, 1, 1))
    active = np.ones(M, bool)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            off, diag = np.zeros(M), np.zeros(M)
            for a in range(3):
                for b in range(3):
                    sq = A[:, a, b] * A[:, a, b]
                    if a == b:
                        diag = diag + sq
                    else:
                        off = off + sq
            active &= off > 2.0 ** -104 * diag
            if not active.any():
                break
            for p, q in PAIRS:
                do = active & (A[:, p, q] != 0.0)
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * A[:, p, q])
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                cs = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * cs
                for r in range(3):                                           # A <- A J
                    x, y = A[:, r, p].copy(), A[:, r, q].copy()
                    A[:, r, p], A[:, r, q] = np.where(do, cs * x - sn * y, x), np.where(do, sn * x + cs * y, y)
                for r in range(3):                                           # A <- J^T A
                    x, y = A[:, p, r].copy(), A[:, q, r].copy()
                    A[:, p, r], A[:, q, r] = np.where(do, cs * x - sn * y, x), np.where(do, sn * x + cs * y, y)
                for r in range(3):                                           # V <- V J
                    x, y = V[:, r, p].copy(), V[:, r, q].copy()
                    V[:, r, p], V[:, r, q] = np.where(do, cs * x - sn * y, x), np.where(do, sn * x + cs * y, y)
    return A, V


def moments(points, neighbors):
    """(count i32[N], centroid f64[N,3], covariance f64[N,6] = xx xy xz yy yz zz) of every point's neighbour row: the
    entries in [0, N) of a valid point's row; sums in list order, one addition at a time, each divided by the count.
    Zeros without a neighbour."""
    p = C.f32(points)
    N = len(p)
    nb = np.asarray(neighbors, np.int64).reshape(N, -1)
    P = p.astype(np.float64)
    entry = (nb >= 0) & (nb < N) & C.valid(p)[:, None]
    m = entry.sum(1)
    j = np.clip(nb, 0, max(N - 1, 0))
    with np.errstate(all="ignore"):
        total = np.zeros((N, 3))
        for s in range(nb.shape[1]):
            total = total + np.where(entry[:, s, None], P[j[:, s]], 0.0)
        dm = np.maximum(m, 1).astype(np.float64)[:, None]
        c = np.where(m[:, None] > 0, total / dm, 0.0)
        cov = np.zeros((N, 6))
        for s in range(nb.shape[1]):
            r = P[j[:, s]] - c
            prod = np.stack([r[:, 0] * r[:, 0], r[:, 0] * r[:, 1], r[:, 0] * r[:, 2], r[:, 1] * r[:, 1],
                             r[:, 1] * r[:, 2], r[:, 2] * r[:, 2]], 1)
            cov = cov + np.where(entry[:, s, None], prod, 0.0)
        cov = np.where(m[:, None] > 0, cov / dm, 0.0)
    return m.astype(np.int32), c, cov


def normals(points, neighbors, viewpoint=None):
    """dict(normal f32[N,3], curvature f32[N], count i32[N], centroid, covariance, eigenvalues f64[N,3], degenerate):
    the eigenvector of the smallest diagonal entry after jacobi3 (the lowest index on ties) times 1 / sqrt(sum of
    squares); (0, 0, 0) and NaN when count < 3 or the middle eigenvalue <= 2^-40 of the largest; the curvature
    max(l_min, 0) / ((l0 + l1) + l2).  viewpoint f32[3] or f32[N,3]: flipped when (nx dx + ny dy) + nz dz < 0 for
    d = viewpoint - point; None: flipped when the component of largest magnitude (lowest axis on ties) is negative.
    Each output rounded once to f32."""
    p = C.f32(points)
    N = len(p)
    m, c, cov = moments(p, neighbors)
    A = np.stack([cov[:, [0, 1, 2]], cov[:, [1, 3, 4]], cov[:, [2, 4, 5]]], 1)
    D, V = jacobi3(A)
    lam = np.stack([D[:, 0, 0], D[:, 1, 1], D[:, 2, 2]], 1)
    with np.errstate(all="ignore"):
        lo = np.zeros(N, np.int64)
        lmin = lam[:, 0].copy()
        for a in (1, 2):
            less = lam[:, a] < lmin
            lo, lmin = np.where(less, a, lo), np.where(less, lam[:, a], lmin)
        lmax = np.maximum(np.maximum(lam[:, 0], lam[:, 1]), lam[:, 2])
        lmid = np.maximum(np.minimum(lam[:, 0], lam[:, 1]), np.minimum(np.maximum(lam[:, 0], lam[:, 1]), lam[:, 2]))
        degenerate = (m < 3) | (lmid <= 2.0 ** -40 * lmax)
        v = V[np.arange(N), :, lo]
        n2 = np.zeros(N)
        for a in range(3):
            n2 = n2 + v[:, a] * v[:, a]
        v = v * (1.0 / np.sqrt(n2))[:, None]
        if viewpoint is not None:
            d = np.broadcast_to(np.asarray(viewpoint, np.float32).astype(np.float64), (N, 3)) - p.astype(np.float64)
            flip = (v[:, 0] * d[:, 0] + v[:, 1] * d[:, 1]) + v[:, 2] * d[:, 2] < 0.0
        else:
            big = v[:, 0].copy()
            for a in (1, 2):
                big = np.where(np.abs(v[:, a]) > np.abs(big), v[:, a], big)
            flip = big < 0.0
        v = np.where(flip[:, None], -v, v)
        curv = np.maximum(lmin, 0.0) / ((lam[:, 0] + lam[:, 1]) + lam[:, 2])
        normal = np.where(degenerate[:, None], 0.0, v).astype(np.float32)
        curvature = np.where(degenerate, np.nan, curv).astype(np.float32)
    return dict(normal=normal, curvature=curvature, count=m, centroid=c, covariance=cov, eigenvalues=lam,
                degenerate=degenerate, normal64=np.where(degenerate[:, None], 0.0, v))


# ----------------------------------------------------------------------------------------------------------------------
# outliers
# ----------------------------------------------------------------------------------------------------------------------
def mean_distances(points, k):
    """(mean f64[N], scored bool[N]): the mean distance to the k nearest neighbours other than the point itself - the
    sum in list order over the m found, divided by m - for a valid point with m >= 1; NaN elsewhere."""
    p = C.f32(points)
    N = len(p)
    d2, nb = knn(p, p, k, exclude=np.arange(N))
    has = nb >= 0
    total = np.zeros(N)
    with np.errstate(all="ignore"):
        d = np.sqrt(d2)
        for s in range(k):
            total = total + np.where(has[:, s], d[:, s], 0.0)
        m = has.sum(1)
        scored = C.valid(p) & (m >= 1)
        return np.where(scored, total / np.maximum(m, 1), np.nan), scored


def statistics(mean, scored):
    """(mu, sigma): the mean and the SAMPLE standard deviation (divisor M - 1; 0 when M < 2) over the scored points,
    with exact (fsum) sums."""
    x = mean[scored]
    M = len(x)
    if M == 0:
        return math.nan, math.nan
    mu = math.fsum(x) / M
    sigma = math.sqrt(math.fsum((x - mu) * (x - mu)) / (M - 1)) if M >= 2 else 0.0
    return mu, sigma


def outliers(points, k=16, std_ratio=2.0, radius=None, min_neighbors=None, threshold=None):
    """keep bool[N].  Statistical rule (std_ratio not None): mean_i <= threshold, which is mu + std_ratio * sigma unless
    given.  Radius rule: the min_neighbors-th neighbour other than the point has dist2 <= f64(radius)^2.  Both given:
    both hold.  An invalid point is never kept."""
    p = C.f32(points)
    keep = C.valid(p)
    if std_ratio is not None:
        mean, scored = mean_distances(p, k)
        if threshold is None:
            mu, sigma = statistics(mean, scored)
            threshold = mu + std_ratio * sigma
        with np.errstate(all="ignore"):
            keep = keep & scored & (mean <= threshold)
    if radius is not None:
        d2 = knn(p, p, min_neighbors, exclude=np.arange(len(p)))[0][:, min_neighbors - 1]
        keep = keep & (d2 <= float(radius) * float(radius))
    return keep
