"""Numpy statement of the mesh-alignment definitions (DESIGN.md "Mesh alignment"; the kernels are csrc/mesh_align.hip):
the Sim3 transform rounded to f32 once, the closest point of a triangle (the point tests/meshdist_numpy.py `tri_dist2`
selects), the moment sums about fixed origins, Horn's quaternion solve of the weighted Umeyama problem, one trimmed ICP
step and the loop.  Everything is f64 on the f32 inputs.  The sums here are numpy's (pairwise); the kernels' fixed order
differs, and tests compare them within the bound that holds for any order.

A Sim3 is lietorch's [t(3), q(xyzw), s]; it acts as s * R(q) p + t."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshdist_numpy as D  # noqa: E402

N_SUMS = 19          # count, sum w, sum w p (3), sum w c (3), sum w p c^T (9), sum w |p|^2, sum w dist2
OK, DEGENERATE = 0, 1


def quat_to_mat(q):
    x, y, z, w = (np.float64(v) for v in q)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                     [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                     [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]])


def act(T, P):
    """s * (R p) + t in f64, the kernel's operation order; P f64[n,3] -> f64[n,3]."""
    T = np.asarray(T, np.float64)
    R = quat_to_mat(T[3:7])
    P = np.asarray(P, np.float64).reshape(-1, 3)
    return np.stack([T[7] * ((R[d, 0] * P[:, 0] + R[d, 1] * P[:, 1]) + R[d, 2] * P[:, 2]) + T[d] for d in range(3)], 1)


def init_state(T0=None):
    """The state from an f32[8] Sim3: f64, the quaternion normalised in f64; None: the identity."""
    if T0 is None:
        return np.array([0, 0, 0, 0, 0, 0, 1, 1], np.float64)
    T = np.asarray(T0, np.float32).astype(np.float64)
    T[3:7] *= 1.0 / np.sqrt((T[3] * T[3] + T[4] * T[4]) + (T[5] * T[5] + T[6] * T[6]))
    return T


def sim3_inv(T):
    T = np.asarray(T, np.float64)
    R = quat_to_mat(T[3:7])
    return np.concatenate([-(R.T @ T[:3]) / T[7], [-T[3], -T[4], -T[5], T[6]], [1.0 / T[7]]])


def sim3_from(rotvec_deg_axis, t, s):
    """Sim3 from (angle in degrees, axis), a translation and a scale."""
    angle, axis = rotvec_deg_axis
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    h = 0.5 * np.deg2rad(angle)
    return np.concatenate([np.asarray(t, np.float64), axis * np.sin(h), [np.cos(h)], [float(s)]])


def tri_closest(p, a, b, c):
    """The closest point q f64[...,3] of the triangle(s) a, b, c (f64[3], or any shape that broadcasts against p) to the
    points p f64[...,3]: the point meshdist_numpy.tri_dist2 selects, by the same region tests in the same order."""
    shape = np.broadcast_shapes(p.shape, a.shape)
    p, a, b, c = (np.broadcast_to(x, shape) for x in (p, a, b, c))
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = D._dot(ab, ap), D._dot(ac, ap)
    bp = p - b
    d3, d4 = D._dot(ab, bp), D._dot(ac, bp)
    cp = p - c
    d5, d6 = D._dot(ab, cp), D._dot(ac, cp)
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
        q = (a + ab * v[..., None]) + ac * w[..., None]
        cases = [(va <= 0.0) & (e1 >= 0.0) & (e2 >= 0.0), b + w_bc[..., None] * (c - b),
                 (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), a + w_ac[..., None] * ac,
                 (d6 >= 0.0) & (d5 <= d6), c,
                 (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), a + v_ab[..., None] * ab,
                 (d3 >= 0.0) & (d4 <= d3), b,
                 (d1 <= 0.0) & (d2 <= 0.0), a]
        for cond, point in zip(cases[0::2], cases[1::2]):
            q = np.where(cond[..., None], point, q)
    return q


def closest(points, vertices, faces):
    """meshdist_numpy.closest - (dist2, nearest): the smallest squared distance to a valid face and the lowest index of
    a face that attains it, +inf and -1 without a valid face - evaluated only on the (point, face) pairs that can hold
    the minimum: a face lies inside the sphere about its centroid through its farthest corner, and the nearest
    centroid is a point of a face, so a face whose sphere is farther than that (plus 1e-9 of the coordinates) holds
    neither the minimum nor a tie.  The pairs that remain go through the same operations on the same numbers, so the
    bits are those of the full scan (tests/test_mesh_align_cpu.py compares the two)."""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    a, b, c, valid = D.triangles(vertices, faces)
    ids = np.flatnonzero(valid)
    if len(ids) == 0 or len(p) == 0:
        return np.full(len(p), np.inf), np.full(len(p), -1, np.int32)
    a, b, c = a[ids], b[ids], c[ids]
    ctr = (a + b + c) / 3.0
    rad = np.sqrt(np.max([((x - ctr) ** 2).sum(1) for x in (a, b, c)], 0))
    dc = np.sqrt(((p[:, None, :] - ctr[None]) ** 2).sum(2))
    slack = 1e-9 * (1.0 + max(np.abs(p).max(), np.abs(a).max(), np.abs(b).max(), np.abs(c).max()))
    pi, fj = np.nonzero(dc - rad[None] <= dc.min(1)[:, None] + slack)
    r = p[pi] - tri_closest(p[pi], a[fj], b[fj], c[fj])
    d = D._dot(r, r)
    order = np.lexsort((fj, d, pi))                      # by point, then distance, then face index
    first = order[np.r_[True, pi[order][1:] != pi[order][:-1]]]
    return d[first], ids[fj[first]].astype(np.int32)


def closest_points(Q, vertices, faces, nearest):
    """c f64[n,3]: the closest point of face nearest[i] to Q[i] (f32 points); NaN where nearest[i] < 0."""
    q = np.asarray(Q, np.float32).astype(np.float64).reshape(-1, 3)
    a, b, c, _ = D.triangles(vertices, faces)
    out = np.full(q.shape, np.nan)
    m = np.asarray(nearest) >= 0
    if m.any():
        f = np.asarray(nearest)[m]
        out[m] = tri_closest(q[m], a[f], b[f], c[f])
    return out


def sum_terms(P, C, w, counts, op, oc, d2):
    """The per-pair terms f64[n, N_SUMS] about the origins op, oc (zero rows where `counts` is False)."""
    n = len(P)
    terms = np.zeros((n, N_SUMS))
    m = np.asarray(counts, bool)
    if m.any():
        a, b, ww = P[m] - op, C[m] - oc, np.asarray(w, np.float64)[m]
        terms[m, 0] = 1.0
        terms[m, 1] = ww
        terms[m, 2:5] = ww[:, None] * a
        terms[m, 5:8] = ww[:, None] * b
        terms[m, 8:17] = ww[:, None] * (a[:, :, None] * b[:, None, :]).reshape(-1, 9)
        terms[m, 17] = ww * D._dot(a, a)
        terms[m, 18] = ww * np.asarray(d2, np.float64)[m]
    return terms


def horn_solve(sums, op, oc, with_scale=True):
    """The weighted Umeyama solution from the sums: the rotation from the top eigenvector of Horn's 4x4 matrix (here by
    numpy's eigh), s = tr(R M) / sum w |p - pm|^2, t = cm - s R pm -> Sim3 f64[8] with q.w >= 0, or None when degenerate
    (fewer than 3 pairs, no source spread, no positive finite scale)."""
    sums = np.asarray(sums, np.float64)
    count, W = sums[0], sums[1]
    if not (count >= 3.0 and W > 0.0):
        return None
    pm, cm = sums[2:5] / W, sums[5:8] / W
    S = sums[8:17].reshape(3, 3) - W * np.outer(pm, cm)
    spread = sums[17] - W * (pm @ pm)
    if not (spread > 0.0 and np.isfinite(S).all()):
        return None
    k = 1.0 / np.abs(S).max() if np.abs(S).max() > 0.0 else 1.0
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = S * k
    N = np.array([[xx + yy + zz, yz - zy, zx - xz, xy - yx],
                  [yz - zy, xx - yy - zz, xy + yx, zx + xz],
                  [zx - xz, xy + yx, yy - xx - zz, yz + zy],
                  [xy - yx, zx + xz, yz + zy, zz - xx - yy]])
    e = np.linalg.eigh(N)[1][:, -1]
    if e[0] < 0.0:
        e = -e
    q = np.array([e[1], e[2], e[3], e[0]]) / np.linalg.norm(e)
    R = quat_to_mat(q)
    s = float(np.sum(R * S.T) / spread) if with_scale else 1.0
    if not (s > 0.0 and np.isfinite(s)):
        return None
    t = (np.asarray(oc) + cm) - s * (R @ (np.asarray(op) + pm))
    return np.concatenate([t, q, [s]])


def umeyama_svd(src, dst, w=None, with_scale=True):
    """An independent formulation (Umeyama 1991): centred weighted covariance, SVD, the reflection fix -> (R, t, s)."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    w = np.ones(len(src)) if w is None else np.asarray(w, np.float64)
    w = w / w.sum()
    ms, md = w @ src, w @ dst
    a, b = src - ms, dst - md
    cov = (b * w[:, None]).T @ a
    U, sv, Vt = np.linalg.svd(cov)
    d = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0.0:
        d[2] = -1.0
    R = U @ np.diag(d) @ Vt
    s = float((sv * d).sum() / (w @ (a * a).sum(1))) if with_scale else 1.0
    return R, md - s * (R @ ms), s


def fit_pairs(src, dst, weights=None, with_scale=True):
    """(T f64[8], status, sums, rmse of dst - src): the statement of mslam_mesh_align_fit_pairs.  Degenerate: the
    identity."""
    P = np.asarray(src, np.float32).astype(np.float64).reshape(-1, 3)
    C = np.asarray(dst, np.float32).astype(np.float64).reshape(-1, 3)
    ident = init_state()
    if len(P) == 0:
        return ident, DEGENERATE, np.zeros(N_SUMS), np.inf
    w = np.ones(len(P)) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    r = C - P
    sums = sum_terms(P, C, w, w > 0.0, P[0], C[0], D._dot(r, r)).sum(0)
    T = horn_solve(sums, P[0], C[0], with_scale)
    rmse = np.sqrt(sums[18] / sums[1]) if sums[1] > 0.0 else np.inf
    return (ident, DEGENERATE, sums, rmse) if T is None else (T, OK, sums, rmse)


def icp_step(T, P, vertices, faces, trim=np.inf, with_scale=True):
    """One iteration from the state T f64[8] on the source points P f32[n,3] -> dict: moved f32[n,3], dist2, nearest,
    closest, inlier, sums, T (the new state; the old one when degenerate), status, rmse, inliers."""
    P32 = np.asarray(P, np.float32).reshape(-1, 3)
    P64 = P32.astype(np.float64)
    moved = act(T, P64).astype(np.float32)
    d2, nearest = closest(moved, vertices, faces)
    c = closest_points(moved, vertices, faces, nearest)
    inlier = (nearest >= 0) & (d2 <= np.float64(trim) * np.float64(trim))
    out = dict(moved=moved, dist2=d2, nearest=nearest, closest=c, inlier=inlier)
    if len(P64) == 0:
        return dict(out, sums=np.zeros(N_SUMS), T=np.asarray(T, np.float64), status=DEGENERATE, rmse=np.inf, inliers=0)
    op = P64[0]
    oc = act(T, op[None])[0]
    terms = sum_terms(P64, c, np.ones(len(P64)), inlier, op, oc, d2)
    sums = terms.sum(0)
    Tn = horn_solve(sums, op, oc, with_scale)
    rmse = np.sqrt(sums[18] / sums[1]) if sums[1] > 0.0 else np.inf
    return dict(out, terms=terms, sums=sums, T=np.asarray(T, np.float64) if Tn is None else Tn,
                status=DEGENERATE if Tn is None else OK, rmse=rmse, inliers=int(sums[0]))


def icp(P, vertices, faces, T0=None, iters=50, trim=np.inf, with_scale=True):
    """The loop: `iters` steps from T0 (f32[8] or None) -> (T f64[8], history f64[iters,4] of inliers, rmse at T_k, scale
    after the solve, status).  `trim` may be a sequence, one value per iteration."""
    T = init_state(T0)
    trims = np.broadcast_to(np.asarray(trim, np.float64), (iters,))
    hist = np.zeros((iters, 4))
    for k in range(iters):
        st = icp_step(T, P, vertices, faces, trims[k], with_scale)
        T = st["T"]
        hist[k] = st["inliers"], st["rmse"], T[7], st["status"]
    return T, hist


# ----------------------------------------------------------------------------------------------------------------------
# the recovery cases of the CPU and GPU tests
# ----------------------------------------------------------------------------------------------------------------------
def subdivide(V, F, k):
    """Every triangle into k x k congruent ones -> (vertices f32, faces i32), unshared vertices, in face order."""
    V = np.asarray(V, np.float64)
    out = []
    for f in F:
        a, b, c = V[f[0]], V[f[1]], V[f[2]]
        pt = lambda i, j: a + (b - a) * (i / k) + (c - a) * (j / k)
        for i in range(k):
            for j in range(k - i):
                out.append((pt(i, j), pt(i + 1, j), pt(i, j + 1)))
                if i + j < k - 1:
                    out.append((pt(i + 1, j), pt(i + 1, j + 1), pt(i, j + 1)))
    tri = np.array(out)
    return tri.reshape(-1, 3).astype(np.float32), np.arange(3 * len(tri), dtype=np.int32).reshape(-1, 3)


RECOVERY = {"small": ((3.0, (1.0, 2.0, 3.0)), (0.03, -0.03, 0.0265), 0.95),       # 3 deg, 5 cm, scale 0.95
            "mid": ((8.0, (3.0, -1.0, 2.0)), (0.09, 0.09, -0.0794), 0.9)}           # 8 deg, 15 cm, scale 0.9
RECOVERY_N, RECOVERY_TRIM, RECOVERY_ITERS = 1025, 0.25, 80


@functools.lru_cache(maxsize=None)
def recovery_case(name):
    """(source mesh (V, F), target mesh (V, F), the known Sim3 A f64[8]) of an ICP recovery case: the source is the part
    of the room subdivided 6 x 6 whose face centroids have x < 1 (264 faces), moved by A^-1; the target the room
    subdivided 4 x 4 (192 faces, two tiles).  Aligning source onto target should return A."""
    from mast3r_slam import synthetic

    rv, rf = synthetic.room_mesh()
    sv, sf = subdivide(rv, rf, 6)
    keep = sv[sf].astype(np.float64).mean(1)[:, 0] < 1.0
    sv = sv.reshape(-1, 3, 3)[keep].reshape(-1, 3)
    sf = np.arange(len(sv), dtype=np.int32).reshape(-1, 3)
    tv, tf = subdivide(rv, rf, 4)
    A = sim3_from(*RECOVERY[name])
    src = act(sim3_inv(A), sv.astype(np.float64)).astype(np.float32)
    return (src, sf), (tv, tf), A


def sim3_error(T, A):
    """(rotation angle between the two in radians, for small angles; |t - t_A|; |s - s_A|)."""
    T, A = np.asarray(T, np.float64), np.asarray(A, np.float64)
    R = quat_to_mat(T[3:7]) @ quat_to_mat(A[3:7]).T
    ang = float(np.linalg.norm(R - np.eye(3)) / np.sqrt(2.0))          # |R - I|_F = 2 sqrt(2) sin(angle / 2)
    return ang, float(np.linalg.norm(T[:3] - A[:3])), float(abs(T[7] - A[7]))
