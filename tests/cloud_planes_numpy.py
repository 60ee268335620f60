"""Numpy statement of the RANSAC plane segmentation of a point cloud (DESIGN.md "Cloud planes"; the kernels are
csrc/cloud_planes.hip, the Python layer mast3r_slam/tsdf/cloud_planes.py).  Everything about coordinates is f64 on the
f32 inputs, one multiply or add at a time in the order written here, which is the kernel's; the hash is Python integers;
everything else is integer work.

THE ROUND.  One round finds one plane; `planes` runs up to max_planes of them and stops at the first that finds none.
  remaining  the indices of the valid points (three finite coordinates) without a label, ascending; M its length.
             M < max(3, min_points) ends the call.
  draw       hypothesis h of round r takes the points rem[draw(seed, r, h, j)], j = 0, 1, 2, with
             draw = mix(mix(mix(seed) ^ ((r << 32) | h)) ^ j) mod M, mix SplitMix64's finaliser on 64-bit unsigned
             integers.  n = (p1 - p0) x (p2 - p0), each component two products and a difference, divided by its length
             sqrt((nx nx + ny ny) + nz nz); d = -((nx p0x + ny p0y) + nz p0z).  VOID when two of the three draws are
             equal or the length is not finite and > 0: its four numbers are NaN, it counts 0 and is never chosen.
  support    a remaining point supports the plane (n, d) when |((nx px + ny py) + nz pz) + d| <= tol and, with normals,
             its normal m is finite and not zero and |(nx mx + ny my) + nz mz| >= cos_angle.
  count      count[h] = the supporters of hypothesis h among the remaining points.
  select     the largest count, the lowest h on ties; a count below min_points ends the call.
  refit      `sums` of the supporters of the current plane about the origin p0 of the chosen hypothesis, `fit` a
             candidate from them, `sums` of the candidate's supporters; the candidate replaces the plane unless the fit
             is degenerate or it has fewer supporters, in which case the refit ends.  refit_iterations times.
  label      the supporters of the final plane get the label planes_found; `row` is the plane's row.
"""
import math

import numpy as np

import cloud_knn_numpy as K
import cloud_numpy as C

MAX_HYPOTHESES = 1024              # MSLAM_CLOUD_PLANES_MAX_HYPOTHESES of include/mslam_hip.h
MAX_PLANES = 64                    # MSLAM_CLOUD_PLANES_MAX_PLANES
ROW = 13                           # MSLAM_CLOUD_PLANES_ROW: n(3) d count sum_r2 centroid(3) eigenvalues(3) rmse
SUMS = 11                          # MSLAM_CLOUD_PLANES_SUMS: count, q(3), qq^T as xx xy xz yy yz zz, r^2
BLOCK = 256                        # points per block of the sums
MASK = (1 << 64) - 1


# ----------------------------------------------------------------------------------------------------------------------
# the hash
# ----------------------------------------------------------------------------------------------------------------------
def mix(x):
    """SplitMix64's finaliser on a Python integer in [0, 2^64)."""
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def draw(seed, r, h, j, M):
    """The position in the remaining list of point j of hypothesis h of round r."""
    return mix(mix(mix(seed & MASK) ^ ((r << 32) | h)) ^ j) % M


# ----------------------------------------------------------------------------------------------------------------------
# the stages
# ----------------------------------------------------------------------------------------------------------------------
def remaining(points, labels):
    """i32[M]: the valid points with a label < 0, ascending."""
    p = C.f32(points)
    return np.flatnonzero(C.valid(p) & (np.asarray(labels).reshape(len(p)) < 0)).astype(np.int32)


def plane_from_triple(p0, p1, p2):
    """f64[..., 4] of the f64 points p0, p1, p2 f64[..., 3]; NaN where the length is not finite and > 0."""
    with np.errstate(all="ignore"):
        a, b = p1 - p0, p2 - p0
        nx = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
        ny = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
        nz = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        nx, ny, nz = nx / length, ny / length, nz / length
        d = -((nx * p0[..., 0] + ny * p0[..., 1]) + nz * p0[..., 2])
        ok = np.isfinite(length) & (length > 0.0)
        return np.where(ok[..., None], np.stack([nx, ny, nz, d], -1), np.nan)


def hypotheses(points, rem, seed, r, H):
    """(hyp f64[H,4], triples i32[H,3]): the planes of round r and the points they were drawn from (-1 without a
    remaining point)."""
    P = C.f32(points).astype(np.float64)
    M = len(rem)
    if M == 0:
        return np.full((H, 4), np.nan), np.full((H, 3), -1, np.int32)
    pos = np.array([[draw(seed, r, h, j, M) for j in range(3)] for h in range(H)], np.int64).reshape(H, 3)
    tri = np.asarray(rem, np.int64)[pos]
    hyp = plane_from_triple(P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]])
    void = (pos[:, 0] == pos[:, 1]) | (pos[:, 0] == pos[:, 2]) | (pos[:, 1] == pos[:, 2])
    return np.where(void[:, None], np.nan, hyp), tri.astype(np.int32)


def gate(normals, rem):
    """(m f64[M,3], usable bool[M]) of the remaining points' normals: finite and not zero."""
    m = C.f32(normals)[np.asarray(rem, np.int64)].astype(np.float64)
    return m, np.isfinite(m).all(1) & (m != 0.0).any(1)


def residuals(points, rem, planes):
    """f64[H,M]: ((nx px + ny py) + nz pz) + d of the remaining points for the planes f64[H,4]."""
    p = C.f32(points)[np.asarray(rem, np.int64)].astype(np.float64)
    n = np.asarray(planes, np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        return ((n[:, None, 0] * p[None, :, 0] + n[:, None, 1] * p[None, :, 1]) + n[:, None, 2] * p[None, :, 2]) \
            + n[:, None, 3]


def support(points, normals, rem, planes, tol, cos_angle=0.0):
    """bool[H,M]: which remaining points support which of the planes f64[H,4]."""
    n = np.asarray(planes, np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        s = np.abs(residuals(points, rem, n)) <= tol
        if normals is not None:
            m, usable = gate(normals, rem)
            dot = (n[:, None, 0] * m[None, :, 0] + n[:, None, 1] * m[None, :, 1]) + n[:, None, 2] * m[None, :, 2]
            s &= usable[None, :] & (np.abs(dot) >= cos_angle)
    return s


def count(points, normals, rem, hyp, tol, cos_angle=0.0, chunk=64):
    """i32[H]."""
    hyp = np.asarray(hyp, np.float64).reshape(-1, 4)
    out = np.zeros(len(hyp), np.int32)
    for s in range(0, len(hyp), chunk):
        out[s:s + chunk] = support(points, normals, rem, hyp[s:s + chunk], tol, cos_angle).sum(1)
    return out


def select(counts, min_points):
    """(h, count, accepted): the largest count, the lowest h on ties (argmax returns the first maximum)."""
    h = int(np.argmax(counts))
    return h, int(counts[h]), bool(counts[h] >= min_points)


def wave_sum(v):
    """Lane 0 of the descending shuffle tree over the 64 lanes of the last axis."""
    v = np.array(v, np.float64)
    for off in (32, 16, 8, 4, 2, 1):
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
    return v[..., 0]


def block_sum(v):
    """f64[K] of v f64[256,K]: the tree in each of the four waves, then the waves in wave order."""
    w = wave_sum(np.asarray(v, np.float64).reshape(4, 64, -1).transpose(0, 2, 1))
    return ((w[0] + w[1]) + w[2]) + w[3]


def sums(points, normals, rem, plane, origin, tol, cos_angle=0.0):
    """f64[SUMS] over the supporters of `plane` among the remaining points, q = p - origin in f64: row i of the list is
    thread i % 256 of block i // 256 (a point that does not support adds 0.0); block_sum per block; then thread t of
    one block of 256 adds the blocks t, t + 256, ... in ascending order onto 0.0, and block_sum again."""
    p = C.f32(points)[np.asarray(rem, np.int64)].astype(np.float64)
    M = len(p)
    plane = np.asarray(plane, np.float64).reshape(4)
    with np.errstate(all="ignore"):
        s = support(points, normals, rem, plane, tol, cos_angle)[0]
        r = residuals(points, rem, plane)[0]
        q = p - np.asarray(origin, np.float64).reshape(1, 3)
        v = np.stack([np.ones(M), q[:, 0], q[:, 1], q[:, 2], q[:, 0] * q[:, 0], q[:, 0] * q[:, 1], q[:, 0] * q[:, 2],
                      q[:, 1] * q[:, 1], q[:, 1] * q[:, 2], q[:, 2] * q[:, 2], r * r], 1)
        v = np.where(s[:, None], v, 0.0)
        nb = (M + BLOCK - 1) // BLOCK
        v = np.concatenate([v, np.zeros((nb * BLOCK - M, SUMS))])
        partial = np.stack([block_sum(v[b * BLOCK:(b + 1) * BLOCK]) for b in range(nb)]) if nb else np.zeros((0, SUMS))
        acc = np.zeros((BLOCK, SUMS))
        for b in range(0, nb, BLOCK):
            rows = partial[b:b + BLOCK]
            acc[:len(rows)] = acc[:len(rows)] + rows
        return block_sum(acc)


def covariance(S):
    """(mean f64[3], A f64[3,3]) of the sums: mean = sum q / c, A_ab = sum q_a q_b / c - mean_a mean_b."""
    c = S[0]
    m = S[1:4] / c
    xx, xy, xz, yy, yz, zz = (S[4 + k] / c for k in range(6))
    A = np.array([[xx - m[0] * m[0], xy - m[0] * m[1], xz - m[0] * m[2]],
                  [xy - m[0] * m[1], yy - m[1] * m[1], yz - m[1] * m[2]],
                  [xz - m[0] * m[2], yz - m[1] * m[2], zz - m[2] * m[2]]])
    return m, A


def fit(S, origin):
    """(plane f64[4], degenerate) from the sums S about `origin`: the eigenvector of the smallest eigenvalue of the
    covariance by cloud_knn_numpy.jacobi3 (the lowest column on ties) times 1 / sqrt of its squares' sum, d at the
    centroid origin + mean.  Degenerate: fewer than 3 supporters, or a middle eigenvalue <= 2^-40 of the largest."""
    if not S[0] >= 3.0:
        return np.full(4, np.nan), True
    with np.errstate(all="ignore"):
        m, A = covariance(S)
        D, V = K.jacobi3(A[None])
        lam = np.array([D[0, 0, 0], D[0, 1, 1], D[0, 2, 2]])
        lo = 0
        for a in (1, 2):
            if lam[a] < lam[lo]:
                lo = a
        lmax = max(max(lam[0], lam[1]), lam[2])
        lmid = max(min(lam[0], lam[1]), min(max(lam[0], lam[1]), lam[2]))
        if lmid <= 2.0 ** -40 * lmax:
            return np.full(4, np.nan), True
        v = V[0, :, lo]
        v = v * (1.0 / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
        c = np.asarray(origin, np.float64) + m
        d = -((v[0] * c[0] + v[1] * c[1]) + v[2] * c[2])
        return np.array([v[0], v[1], v[2], d]), False


def refit(points, normals, rem, plane, origin, tol, cos_angle=0.0, iterations=2):
    """(plane f64[4], S f64[SUMS] of its supporters, accepted: how many candidates replaced the plane)."""
    plane = np.asarray(plane, np.float64).reshape(4)
    S = sums(points, normals, rem, plane, origin, tol, cos_angle)
    accepted = 0
    for _ in range(iterations):
        cand, degenerate = fit(S, origin)
        if degenerate:
            break
        S_cand = sums(points, normals, rem, cand, origin, tol, cos_angle)
        if not S_cand[0] >= S[0]:
            break
        plane, S, accepted = cand, S_cand, accepted + 1
    return plane, S, accepted


def orient(plane, viewpoint=None):
    """The plane with n and d negated together: with a viewpoint f32[3] when ((nx vx + ny vy) + nz vz) + d < 0, without
    one when the component of n of largest magnitude (the lowest axis on ties) is negative."""
    n = np.asarray(plane, np.float64).reshape(4)
    if viewpoint is not None:
        v = np.asarray(viewpoint, np.float32).astype(np.float64).reshape(3)
        flip = ((n[0] * v[0] + n[1] * v[1]) + n[2] * v[2]) + n[3] < 0.0
    else:
        big = n[0]
        for a in (1, 2):
            if abs(n[a]) > abs(big):
                big = n[a]
        flip = big < 0.0
    return -n if flip else n.copy()


def row(plane, S, origin, viewpoint=None):
    """f64[ROW]: the oriented plane, its supporters' count and sum of r^2, their centroid origin + sum q / c and the
    eigenvalues of their covariance in the order of jacobi3's columns, and sqrt(sum r^2 / count)."""
    with np.errstate(all="ignore"):
        m, A = covariance(S)
        D, _ = K.jacobi3(A[None])
        return np.concatenate([orient(plane, viewpoint), [S[0], S[10]], np.asarray(origin, np.float64) + m,
                               [D[0, 0, 0], D[0, 1, 1], D[0, 2, 2]], [np.sqrt(S[10] / S[0])]])


def planes(points, tol, normals=None, cos_angle=0.0, max_planes=16, min_points=100, hypotheses_per_round=1024,
           refit_iterations=2, seed=0, viewpoint=None):
    """dict: labels i32[N], rows f64[P,ROW], planes f64[P,4], counts i32[P], rmse, centroids, eigenvalues, n_planes."""
    p = C.f32(points)
    P64 = p.astype(np.float64)
    labels = np.full(len(p), -1, np.int32)
    rows = []
    for r in range(max_planes):
        rem = remaining(p, labels)
        if len(rem) < max(3, min_points):
            break
        hyp, tri = hypotheses(p, rem, seed, r, hypotheses_per_round)
        h, c, ok = select(count(p, normals, rem, hyp, tol, cos_angle), min_points)
        if not ok:
            break
        origin = P64[tri[h, 0]]
        plane, S, _ = refit(p, normals, rem, hyp[h], origin, tol, cos_angle, refit_iterations)
        labels[rem[support(p, normals, rem, plane, tol, cos_angle)[0]]] = len(rows)
        rows.append(row(plane, S, origin, viewpoint))
    rows = np.array(rows, np.float64).reshape(-1, ROW)
    return dict(labels=labels, rows=rows, planes=rows[:, :4].copy(), counts=rows[:, 4].astype(np.int32),
                rmse=rows[:, 12].copy(),
                centroids=rows[:, 6:9].copy(), eigenvalues=rows[:, 9:12].copy(), n_planes=len(rows))


def figures(result, n_valid):
    """plane_figures' numbers from the statement's result: the share of the valid points that carry a label, the rmse
    over all of them, the number of planes, and the count-weighted mean over pairs of planes of the distance of the
    angle between their normals to the nearer of 0 and 90 degrees (0 without a pair)."""
    n = result["planes"][:, :3]
    c = result["counts"].astype(np.float64)
    total = float(c.sum())
    num = den = 0.0
    for i in range(len(n)):
        for j in range(i + 1, len(n)):
            a = math.degrees(math.acos(min(1.0, abs(float(n[i] @ n[j])))))
            num += c[i] * c[j] * min(a, 90.0 - a)
            den += c[i] * c[j]
    return dict(plane_share=total / n_valid if n_valid else 0.0,
                plane_rmse=float(math.sqrt(result["rows"][:, 5].sum() / total)) if total else 0.0,
                n_planes=len(n), manhattan_deg=float(num / den) if den else 0.0)
