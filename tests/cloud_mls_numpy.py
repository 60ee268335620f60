"""Numpy statement of the cloud smoothing step, the moving-least-squares projection in its plane form (DESIGN.md "Cloud
smoothing"; the kernel is csrc/cloud_mls.hip, the Python layer mast3r_slam/tsdf/cloud_smooth.py).  Everything is f64 on
the f32 inputs, one multiply or add at a time, and THE SUMS ARE SEQUENTIAL IN `order`: np.cumsum(...)[-1], never
np.sum, which adds pairwise.

THE DEFINITION.  A point of the cloud with a non-finite coordinate does not exist.  For query p and point q,
d2 = (dx dx + dy dy) + dz dz of the f64 differences (cloud_numpy.dist2_matrix).  q JOINS when d2 <= h2 and, with a gate,
fabs((ax bx + ay by) + az bz) >= cos_gate for the query's normal a and the point's normal b; a query whose normal is
(0, 0, 0) or non-finite is not gated, a point's non-finite normal counts as (0, 0, 0).  inv = 1 / h2, u = 1 - d2 inv,
w = u u: a neighbour at d2 == h2 joins with weight 0.  r = q - p.  Per joining neighbour, in the order order[0], order[1],
... (None: ascending index; entries outside [0, N) are skipped):
    S0 += w;  wx = w rx: S1x += wx, Sxx += wx rx, Sxy += wx ry, Sxz += wx rz;  wy = w ry: S1y += wy, Syy += wy ry,
    Syz += wy rz;  wz = w rz: S1z += wz, Szz += wz rz;  count += 1.
m = S1 / S0, C = S2 / S0 - m m^T entry by entry (zeros unless S0 > 0), cloud_knn_numpy.jacobi3 on C, and the eigenvector
tail of cloud_knn_numpy.normals without a viewpoint: the column of the smallest diagonal entry (the lowest index on
ties) times 1 / sqrt(sum of squares), flipped when its component of largest magnitude (lowest axis on ties) is negative;
degenerate when count < 3 or lmid <= 2^-40 lmax; curvature max(lmin, 0) / ((l0 + l1) + l2).
t = (nx mx + ny my) + nz mz, out = f32(p + (strength t) n).  A query STAYS - its input bits, normal (0, 0, 0), curvature
NaN - when it has a non-finite coordinate, when count < min_points, when count < 3 or when it is degenerate."""
import math

import numpy as np

import cloud_knn_numpy as K
import cloud_numpy as C

MOMENTS = 18                       # MSLAM_CLOUD_MLS_MOMENTS of include/mslam_hip.h


def _last(a):
    """The sequential sum of every row of a[c, M] from +0: the last entry of the running sum (0 for M = 0).  The running
    sum starts at its first term where the kernel's starts at +0, which differs only when every term is -0: the + 0.0
    turns that -0 into the +0 of 0 + (-0) and changes no other value."""
    return np.cumsum(a, 1)[:, -1] + 0.0 if a.shape[1] else np.zeros(len(a))


def sums(Q, P, h2, order=None, qn=None, pn=None, cos_gate=None, chunk=128):
    """(S f64[n,10] = S0, S1 xyz, S2 xx xy xz yy yz zz; count i32[n]) of the queries Q in the cloud P, the terms added in
    `order`.  A point that does not join enters with the weight +0, so its terms are +-0 and change no bit of a running
    sum that started at +0 (_last)."""
    q32, p32 = C.f32(Q), C.f32(P)
    n, N = len(q32), len(p32)
    o = np.arange(N, dtype=np.int64) if order is None else np.asarray(order, np.int64)
    o = o[(o >= 0) & (o < N)]
    o = o[C.valid(p32)[o]] if N else o
    px, py, pz = np.ascontiguousarray(p32[o].astype(np.float64).T) if len(o) else np.zeros((3, 0))
    ok_q = C.valid(q32)
    q64 = np.where(ok_q[:, None], q32, np.float32(0)).astype(np.float64)
    S, count = np.zeros((n, 10)), np.zeros(n, np.int32)
    gate = qn is not None
    if gate:
        a32, b32 = C.f32(qn), C.f32(pn)
        gated = np.isfinite(a32).all(1) & (a32 != 0).any(1)
        B = np.where(np.isfinite(b32).all(1)[:, None], b32, np.float32(0)).astype(np.float64)[o]
        A = a32.astype(np.float64)
    inv = 1.0 / np.float64(h2)
    with np.errstate(all="ignore"):
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            # r, point - query, is the exact negation of cloud_numpy.dist2_matrix's difference: the same squares, so d
            # is that function's value bit for bit
            rx, ry, rz = (c[None, :] - q64[s:e, k, None] for k, c in enumerate((px, py, pz)))
            d = (rx * rx + ry * ry) + rz * rz
            join = (d <= h2) & ok_q[s:e, None]
            if gate:
                a = A[s:e]
                dot = np.abs((a[:, None, 0] * B[None, :, 0] + a[:, None, 1] * B[None, :, 1]) + a[:, None, 2] * B[None, :, 2])
                join &= ~gated[s:e, None] | (dot >= cos_gate)
            cols = join.any(0)                                   # columns that join no row of the chunk add only +0
            if 2 * int(cols.sum()) < len(cols):                 # worth the copies
                d, join, rx, ry, rz = (x[:, cols] for x in (d, join, rx, ry, rz))
            u = 1.0 - d * inv
            w = np.where(join, u * u, 0.0)
            S[s:e, 0] = _last(w)
            for k, (ra, rest) in enumerate(((rx, (rx, ry, rz)), (ry, (ry, rz)), (rz, (rz,)))):
                wa = w * ra                                      # wx, then wy, then wz
                S[s:e, 1 + k] = _last(wa)
                for j, rb in enumerate(rest):
                    S[s:e, (4, 7, 9)[k] + j] = _last(wa * rb)
            count[s:e] = join.sum(1)
    return S, count


def finish(Q, S, count, min_points, strength):
    """From the sums to every output of the step: the dict of mls_step."""
    q32 = C.f32(Q)
    n = len(q32)
    p = np.where(C.valid(q32)[:, None], q32, np.float32(0)).astype(np.float64)
    with np.errstate(all="ignore"):
        live = S[:, 0] > 0.0
        s0 = np.where(live, S[:, 0], 1.0)
        m = np.where(live[:, None], S[:, 1:4] / s0[:, None], 0.0)
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        cov = np.stack([np.where(live, S[:, 4 + k] / s0 - m[:, a] * m[:, b], 0.0) for k, (a, b) in enumerate(pairs)], 1)
        A = np.stack([cov[:, [0, 1, 2]], cov[:, [1, 3, 4]], cov[:, [2, 4, 5]]], 1)
        D, V = K.jacobi3(A) if n else (np.zeros((0, 3, 3)), np.zeros((0, 3, 3)))
        lam = np.stack([D[:, 0, 0], D[:, 1, 1], D[:, 2, 2]], 1)
        # the eigenvector tail of cloud_knn_numpy.normals, viewpoint None
        lo = np.zeros(n, np.int64)
        lmin = lam[:, 0].copy()
        for a in (1, 2):
            less = lam[:, a] < lmin
            lo, lmin = np.where(less, a, lo), np.where(less, lam[:, a], lmin)
        lmax = np.maximum(np.maximum(lam[:, 0], lam[:, 1]), lam[:, 2])
        lmid = np.maximum(np.minimum(lam[:, 0], lam[:, 1]), np.minimum(np.maximum(lam[:, 0], lam[:, 1]), lam[:, 2]))
        degenerate = (count < 3) | (lmid <= 2.0 ** -40 * lmax)
        v = V[np.arange(n), :, lo]
        n2 = np.zeros(n)
        for a in range(3):
            n2 = n2 + v[:, a] * v[:, a]
        v = v * (1.0 / np.sqrt(n2))[:, None]
        big = v[:, 0].copy()
        for a in (1, 2):
            big = np.where(np.abs(v[:, a]) > np.abs(big), v[:, a], big)
        v = np.where((big < 0.0)[:, None], -v, v)
        moved = C.valid(q32) & (count >= int(min_points)) & ~degenerate
        t = (v[:, 0] * m[:, 0] + v[:, 1] * m[:, 1]) + v[:, 2] * m[:, 2]
        st = np.float64(strength) * t
        new = (p + st[:, None] * v).astype(np.float32)
        curv = np.maximum(lmin, 0.0) / ((lam[:, 0] + lam[:, 1]) + lam[:, 2])
    points = q32.copy()                                          # a query that stays keeps its bits, NaN payloads included
    points[moved] = new[moved]
    normal64 = np.where(moved[:, None], v, 0.0)
    mom = np.zeros((n, MOMENTS))
    mom[:, :10], mom[:, 10:13], mom[:, 13:16], mom[:, 16] = S, lam, normal64, np.where(moved, t, 0.0)
    return dict(points=points, normals=normal64.astype(np.float32),
                curvature=np.where(moved, curv, np.nan).astype(np.float32), count=count.astype(np.int32), moved=moved,
                moments=mom)


def mls_step(Q, P, h2, min_points, strength, order=None, qn=None, pn=None, cos_gate=None):
    """One step for the queries Q f32[n,3] on the cloud P f32[N,3] -> dict(points f32[n,3], normals f32[n,3], curvature
    f32[n], count i32[n], moved bool[n], moments f64[n,18]).  moments: S0, S1 (3), S2 (6), the three diagonal entries after
    the sweeps, the signed unit normal before its rounding (zeros when the query stays), t (0 when it stays), 0."""
    assert (qn is None) == (pn is None) and (qn is None) == (cos_gate is None)
    S, count = sums(Q, P, h2, order, qn, pn, cos_gate)
    return finish(Q, S, count, min_points, strength)


def smooth(P, radius, iterations=1, min_points=6, strength=1.0, edge_angle=None, order=None):
    """The loop of smooth_cloud -> (points f32[N,3], info).  The surface is the INPUT cloud's in every iteration:
    q_0 = P, q_{t+1} = step(q_t, P).  With edge_angle (degrees): one ungated step of the cloud in itself gives the cloud's
    normals, then every step is gated by cos(edge_angle) with those as the points' normals and row i's own as query i's.
    info: moved bool[N] (in some iteration), normals, curvature and count of the last step, n_valid, rms_displacement
    and max_displacement over the valid rows (f64, the distance between the f32 input and output)."""
    P = C.f32(P)
    h2 = float(radius) * float(radius)
    qn = pn = cos_gate = None
    if edge_angle is not None:
        qn = pn = mls_step(P, P, h2, min_points, strength, order)["normals"]
        cos_gate = math.cos(math.radians(edge_angle))
    q, moved, last = P, np.zeros(len(P), bool), None
    for _ in range(int(iterations)):
        last = mls_step(q, P, h2, min_points, strength, order, qn, pn, cos_gate)
        q, moved = last["points"], moved | last["moved"]
    ok = C.valid(P)
    d = q[ok].astype(np.float64) - P[ok].astype(np.float64)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    info = dict(moved=moved, n_valid=int(ok.sum()), normals=last["normals"], curvature=last["curvature"],
                count=last["count"], rms_displacement=math.sqrt(d2.sum() / len(d2)) if len(d2) else 0.0,
                max_displacement=math.sqrt(d2.max()) if len(d2) else 0.0)
    return q, info
