"""Numpy statement of point-to-plane ICP for clouds and meshes (DESIGN.md "Point-to-plane ICP"; the kernels are
csrc/icp_plane.hip, the Python layer align_clouds / align_meshes with metric="plane"): the pair with its normal, the
inlier rule, the plane row and the weighted point rows about the moved first sample, the 39 sums, the scaled Cholesky
solve, the Sim3 update and the log row.  Everything is f64 on the f32 inputs, and every product grouping written here is
the kernel's: one multiply or add at a time.  The sums here are numpy's (pairwise); the kernels' fixed order differs,
and tests compare them within the bound that holds for any order.  The solve and the update are written with Python
floats, operation by operation as the kernel does them, so the solve of the SAME sums differs from the device's only
where sin, cos and exp do.

A Sim3 is lietorch's [t(3), q(xyzw), s]; it acts as s * R(q) p + t.  The unknowns are xi = (tau, omega, sigma) and the
update is x -> o + e^sigma R(omega) (x - o) + tau about o, the moved first sample."""
import functools
import math

import numpy as np

import cloud_knn_numpy as K
import cloud_numpy as C
import meshalign_numpy as A
import meshdist_numpy as D

N_SUMS = 39          # count, sum w, sum r^2, sum dist2, g (7), the upper triangle of H row by row (28)
G0, H0 = 4, 11       # where g and H begin
LOG = 6 + N_SUMS     # inliers, rms, scale, status, point rmse, normal_spread, the sums
OK, DEGENERATE = A.OK, A.DEGENERATE
PIVOT = 2.0 ** -40   # the smallest pivot of the scaled matrix; cloud_normals' "collinear" constant
SMALL = 2.0 ** -26   # |omega|^2 below which the series stand in for sin and cos


def h_index(j, k):
    """Where H[j][k], j <= k, lies among the sums."""
    return H0 + 7 * j - j * (j - 1) // 2 + (k - j)


def h_matrix(sums):
    H = np.zeros((7, 7))
    for j in range(7):
        for k in range(j, 7):
            H[j, k] = H[k, j] = sums[h_index(j, k)]
    return H


# ----------------------------------------------------------------------------------------------------------------------
# the pair
# ----------------------------------------------------------------------------------------------------------------------
def face_normals(vertices, faces):
    """f64[F,3]: ((b - a) x (c - a)) divided by its length sqrt((nx nx + ny ny) + nz nz); NaN for an invalid face."""
    a, b, c, valid = D.triangles(vertices, faces)
    n = D._cross(b - a, c - a)
    with np.errstate(all="ignore"):
        return n / np.sqrt(D._dot(n, n))[:, None]


def match(moved, target):
    """(dist2, nearest, c f64[n,3], n f64[n,3]) of the f32 points `moved` against target = ("cloud", points, normals)
    or ("mesh", vertices, faces): the existing scans with their tie rules; c NaN and n zero without a neighbour."""
    kind, x, y = target
    q = C.f32(moved)
    if kind == "cloud":
        d2, nn = C.nearest(q, x)
        has = nn >= 0
        j = np.maximum(nn, 0)
        if len(C.f32(x)):
            c = np.where(has[:, None], C.f32(x)[j].astype(np.float64), np.nan)
            nrm = np.where(has[:, None], C.f32(y)[j].astype(np.float64), 0.0)
        else:
            c, nrm = np.full((len(q), 3), np.nan), np.zeros((len(q), 3))
    else:
        # a sample with a non-finite coordinate is at a NaN distance from every face, which never beats the best
        ok = np.isfinite(q).all(1)
        d2, nn = np.full(len(q), np.inf), np.full(len(q), -1, np.int32)
        d2[ok], nn[ok] = A.closest(q[ok], x, y)
        c = A.closest_points(q, x, y, nn)
        fn = face_normals(x, y)
        nrm = np.where((nn >= 0)[:, None], fn[np.maximum(nn, 0)], 0.0) if len(fn) else np.zeros((len(q), 3))
    return d2, nn.astype(np.int32), c, nrm


def usable(nrm):
    """bool[n]: the normal is finite and not zero."""
    with np.errstate(all="ignore"):
        return np.isfinite(nrm).all(1) & (nrm != 0.0).any(1)


# ----------------------------------------------------------------------------------------------------------------------
# rows and sums
# ----------------------------------------------------------------------------------------------------------------------
def rows(q, c, nrm, o):
    """(J f64[n,7], r f64[n], P f64[n,3,7], e f64[n,3]): the plane row and the three point rows of every pair about o.
    J = [n, a x n, n . a], r = n . e; P_d = [u_d, a x u_d, a_d], r_d = e_d; a = q - o, e = q - c."""
    a, e = q - o, q - c
    r = (nrm[:, 0] * e[:, 0] + nrm[:, 1] * e[:, 1]) + nrm[:, 2] * e[:, 2]
    J = np.stack([nrm[:, 0], nrm[:, 1], nrm[:, 2],
                  a[:, 1] * nrm[:, 2] - a[:, 2] * nrm[:, 1],
                  a[:, 2] * nrm[:, 0] - a[:, 0] * nrm[:, 2],
                  a[:, 0] * nrm[:, 1] - a[:, 1] * nrm[:, 0],
                  (nrm[:, 0] * a[:, 0] + nrm[:, 1] * a[:, 1]) + nrm[:, 2] * a[:, 2]], 1)
    z, u = np.zeros(len(q)), np.ones(len(q))
    P = np.stack([np.stack([u, z, z, z, a[:, 2], -a[:, 1], a[:, 0]], 1),
                  np.stack([z, u, z, -a[:, 2], z, a[:, 0], a[:, 1]], 1),
                  np.stack([z, z, u, a[:, 1], -a[:, 0], z, a[:, 2]], 1)], 1)
    return J, r, P, e


def sum_terms(q, c, nrm, o, d2, nearest, trim=np.inf, alpha=0.0):
    """(terms f64[n, N_SUMS], inlier bool[n]).  A pair is an inlier when it has a neighbour, dist2 <= trim^2 and a
    usable normal - or, with alpha > 0, no usable normal: its normal is then taken as zero and only the point rows
    remain.  g_j = J_j r + alpha ((P0_j e0 + P1_j e1) + P2_j e2), H_jk = J_j J_k + alpha ((P0_j P0_k + P1_j P1_k) +
    P2_j P2_k); zeros for a pair that does not count."""
    n = len(q)
    terms = np.zeros((n, N_SUMS))
    ok = usable(nrm)
    with np.errstate(all="ignore"):
        inlier = (np.asarray(nearest) >= 0) & (d2 <= np.float64(trim) * np.float64(trim)) & (ok | (alpha > 0.0))
    m = inlier
    if not m.any():
        return terms, inlier
    nz = np.where(ok[:, None], nrm, 0.0)[m]
    J, r, P, e = rows(q[m], c[m], nz, o)
    alpha = np.float64(alpha)
    t = np.zeros((int(m.sum()), N_SUMS))
    t[:, 0] = 1.0
    t[:, 1] = 1.0
    t[:, 2] = r * r
    t[:, 3] = d2[m]
    for j in range(7):
        t[:, G0 + j] = J[:, j] * r + alpha * ((P[:, 0, j] * e[:, 0] + P[:, 1, j] * e[:, 1]) + P[:, 2, j] * e[:, 2])
        for k in range(j, 7):
            t[:, h_index(j, k)] = J[:, j] * J[:, k] + alpha * ((P[:, 0, j] * P[:, 0, k] + P[:, 1, j] * P[:, 1, k])
                                                             + P[:, 2, j] * P[:, 2, k])
    terms[m] = t
    return terms, inlier


# ----------------------------------------------------------------------------------------------------------------------
# solve and update
# ----------------------------------------------------------------------------------------------------------------------
def solve(sums, with_scale=True):
    """(xi f64[7] or None, pivots): H scaled to unit diagonal, Cholesky, H xi = -g; sigma = 0 without scale.  None when
    degenerate: fewer inliers than unknowns, a zero or non-finite diagonal entry, a pivot <= 2^-40, a non-finite xi.
    `pivots`: the pivots met, for the tests."""
    s = [float(x) for x in sums]
    nu = 7 if with_scale else 6
    pivots = []
    if not s[0] >= float(nu):
        return None, pivots
    sc = []
    for j in range(nu):
        d = s[h_index(j, j)]
        if not (d > 0.0 and d < math.inf):
            return None, pivots
        sc.append(1.0 / math.sqrt(d))
    L = [[0.0] * nu for _ in range(nu)]
    for j in range(nu):
        pv = (s[h_index(j, j)] * sc[j]) * sc[j]
        for k in range(j):
            pv -= L[j][k] * L[j][k]
        pivots.append(pv)
        if not pv > PIVOT:
            return None, pivots
        l = math.sqrt(pv)
        L[j][j] = l
        for i in range(j + 1, nu):
            x = (s[h_index(j, i)] * sc[i]) * sc[j]
            for k in range(j):
                x -= L[i][k] * L[j][k]
            L[i][j] = x / l
    y = [0.0] * nu
    for j in range(nu):
        x = -(s[G0 + j] * sc[j])
        for k in range(j):
            x -= L[j][k] * y[k]
        y[j] = x / L[j][j]
    z = [0.0] * nu
    for j in range(nu - 1, -1, -1):
        x = y[j]
        for k in range(j + 1, nu):
            x -= L[k][j] * z[k]
        z[j] = x / L[j][j]
    xi = np.zeros(7)
    for j in range(nu):
        xi[j] = z[j] * sc[j]
    if not np.isfinite(xi).all():
        return None, pivots
    return xi, pivots


def rodrigues(w):
    """(R f64[3,3], A, B, hs, cw) of omega: R = I + A [w]x + B [w]x^2 written out entry by entry, A = sin th / th,
    B = 2 sin^2(th / 2) / th^2; hs = sin(th / 2) / th and cw = cos(th / 2) make the unit quaternion (w hs, cw).  Below
    th^2 = 2^-26 the series 1 - th^2 / 6, 1/2 - th^2 / 24, 1/2 - th^2 / 48, 1 - th^2 / 8, whose next terms are below
    2^-52 of the first."""
    wx, wy, wz = (float(x) for x in w)
    th2 = (wx * wx + wy * wy) + wz * wz
    if th2 < SMALL:
        Af, Bf, hs, cw = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 0.5 - th2 / 48.0, 1.0 - th2 / 8.0
    else:
        th = math.sqrt(th2)
        sh = math.sin(0.5 * th)
        Af, Bf, hs, cw = math.sin(th) / th, (2.0 * (sh * sh)) / th2, sh / th, math.cos(0.5 * th)
    R = np.array([[1.0 + Bf * (wx * wx - th2), Bf * (wx * wy) - Af * wz, Bf * (wx * wz) + Af * wy],
                  [Bf * (wx * wy) + Af * wz, 1.0 + Bf * (wy * wy - th2), Bf * (wy * wz) - Af * wx],
                  [Bf * (wx * wz) - Af * wy, Bf * (wy * wz) + Af * wx, 1.0 + Bf * (wz * wz - th2)]])
    return R, Af, Bf, hs, cw


def update(T, xi, o, with_scale=True):
    """D o T for D: x -> o + e^sigma R(omega) (x - o) + tau -> the new Sim3, or None without a positive finite scale:
    s' = e^sigma s, q' = q_delta * q renormalised, t' = (o + e^sigma (R (t - o))) + tau.  Without scale s is kept as it
    is."""
    T = [float(x) for x in T]
    R, _, _, hs, cw = rodrigues(xi[3:6])
    es = math.exp(float(xi[6])) if with_scale else 1.0
    sn = es * T[7]
    if not (sn > 0.0 and sn < math.inf):
        return None
    dx, dy, dz, dw = float(xi[3]) * hs, float(xi[4]) * hs, float(xi[5]) * hs, cw
    qx, qy, qz, qw = T[3:7]
    nx = ((dw * qx + dx * qw) + dy * qz) - dz * qy
    ny = ((dw * qy - dx * qz) + dy * qw) + dz * qx
    nz = ((dw * qz + dx * qy) - dy * qx) + dz * qw
    nw = ((dw * qw - dx * qx) - dy * qy) - dz * qz
    inv = 1.0 / math.sqrt((nx * nx + ny * ny) + (nz * nz + nw * nw))
    b = [T[d] - float(o[d]) for d in range(3)]
    t = [(float(o[d]) + es * ((float(R[d, 0]) * b[0] + float(R[d, 1]) * b[1]) + float(R[d, 2]) * b[2])) + float(xi[d])
         for d in range(3)]
    return np.array(t + [nx * inv, ny * inv, nz * inv, nw * inv, sn if with_scale else T[7]])


def delta_map(xi, o, X):
    """x -> o + e^sigma R(omega) (x - o) + tau on the points X f64[n,3], for the tests of the rows."""
    R = rodrigues(xi[3:6])[0]
    return o + math.exp(float(xi[6])) * ((X - o) @ R.T) + np.asarray(xi[:3])


def normal_spread(sums):
    """The smallest eigenvalue of H's translation block (K.jacobi3, clamped at 0) over sum w; 0 without a pair."""
    if not sums[1] > 0.0:
        return 0.0
    H = h_matrix(sums)[:3, :3]
    lam = K.jacobi3(H[None])[0][0]
    return max(min(lam[0, 0], lam[1, 1], lam[2, 2]), 0.0) / float(sums[1])


def log_row(sums, T_after, status, alpha):
    """The device's log row from the sums."""
    W = float(sums[1])
    with np.errstate(all="ignore"):
        rms = math.sqrt((sums[2] + alpha * sums[3]) / W) if W > 0.0 else math.inf
        prmse = math.sqrt(sums[3] / W) if W > 0.0 else math.inf
    return np.concatenate([[sums[0], rms, T_after[7], float(status), prmse, normal_spread(sums)], sums])


# ----------------------------------------------------------------------------------------------------------------------
# one iteration and the loop
# ----------------------------------------------------------------------------------------------------------------------
def origin(T, src):
    """o: T src[0] in f64, rounded once to f32."""
    return A.act(T, C.f32(src)[:1].astype(np.float64))[0].astype(np.float32).astype(np.float64)


def step(T, src, target, trim=np.inf, with_scale=True, alpha=0.0, moved=None, sums=None):
    """One iteration from the state T f64[8] on the samples src f32[n,3] -> dict: moved, dist2, nearest, closest,
    normal, inlier, terms, sums, xi, T (the old one when degenerate), status, log.  `moved`: take these f32 points as
    the moved samples; `sums`: solve these instead of the statement's own."""
    T = np.asarray(T, np.float64)
    P32 = C.f32(src)
    if moved is None:
        moved = A.act(T, P32.astype(np.float64)).astype(np.float32)
    q = C.f32(moved).astype(np.float64)
    d2, nn, c, nrm = match(moved, target)
    out = dict(moved=moved, dist2=d2, nearest=nn, closest=c, normal=nrm)
    if len(P32) == 0:
        z = np.zeros(N_SUMS)
        return dict(out, inlier=np.zeros(0, bool), terms=np.zeros((0, N_SUMS)), sums=z, xi=None, T=T,
                    status=DEGENERATE, log=log_row(z, T, DEGENERATE, alpha))
    o = origin(T, P32)
    with np.errstate(all="ignore"):
        terms, inlier = sum_terms(q, c, nrm, o, d2, nn, trim, alpha)
    own = terms.sum(0)
    use = own if sums is None else np.asarray(sums, np.float64)
    xi, pivots = solve(use, with_scale)
    Tn = None if xi is None else update(T, xi, o, with_scale)
    status = DEGENERATE if Tn is None else OK
    Tn = T if Tn is None else Tn
    return dict(out, inlier=inlier, terms=terms, sums=own, xi=xi, pivots=pivots, origin=o, T=Tn, status=status,
                log=log_row(use, Tn, status, alpha))


def icp(src, target, T0=None, iters=10, trim=np.inf, with_scale=True, alpha=0.0):
    """`iters` steps from T0 (f32[8] or None, as mslam_mesh_align_init takes it) -> (T f64[8], history f64[iters, 6]:
    inliers, rms, scale after the solve, status, point rmse, normal_spread, states f64[iters, 8])."""
    T = A.init_state(T0)
    trims = np.broadcast_to(np.asarray(trim, np.float64), (iters,))
    hist, states = np.zeros((iters, 6)), np.zeros((iters, 8))
    for k in range(iters):
        st = step(T, src, target, trims[k], with_scale, alpha)
        T = st["T"]
        hist[k], states[k] = st["log"][:6], T
    return T, hist, states


# ----------------------------------------------------------------------------------------------------------------------
# fixtures
# ----------------------------------------------------------------------------------------------------------------------
BOX_HALF = np.array([2.0, 1.5, 1.2])
TABLE_CENTRE, TABLE_HALF = np.array([0.7, -0.4, -0.8]), np.array([0.4, 0.3, 0.4])
BOX_MOVE = A.sim3_from((5.0, (1.0, 2.0, 3.0)), (0.03, -0.03, 0.0265), 0.95)       # 5 degrees, 5 cm, scale 0.95
BOX_SAMPLES, BOX_K = 500, 16


def _faces(rng, centre, half, m):
    out = []
    for ax in range(3):
        for sgn in (-1.0, 1.0):
            p = rng.uniform(-1.0, 1.0, (m, 3)) * half
            p[:, ax] = sgn * half[ax]
            out.append(p + centre)
    return out


def box_cloud(seed, n=4000):
    """The walls of a closed box with half extents (2.0, 1.5, 1.2), n // 6 points each, and a table inside it, n // 24
    points per face -> f32[., 3]."""
    rng = np.random.default_rng(seed)
    return np.concatenate(_faces(rng, np.zeros(3), BOX_HALF, n // 6)
                          + _faces(rng, TABLE_CENTRE, TABLE_HALF, n // 24)).astype(np.float32)


def knn_normals(points, k=BOX_K):
    return K.normals(points, K.knn(points, points, k)[1])["normal"]


@functools.lru_cache(maxsize=None)
def box_case(n=4000):
    """(pred, gt, gt's normals at k = 16, the 500 stride samples of pred): the target is seed 0, the source an
    independent sampling (seed 1) of the same surfaces moved by BOX_MOVE^-1, so no exact pairs exist."""
    gt = box_cloud(0, n)
    pred = A.act(A.sim3_inv(BOX_MOVE), box_cloud(1, n).astype(np.float64)).astype(np.float32)
    return pred, gt, knn_normals(gt), C.stride_sample(pred, BOX_SAMPLES)[0]


def room_cloud(n_kf=4, n_pts=1000, step=80, h=96, w=128, seed0=0):
    """tests/test_cloud_gpu.room_cloud: world points of the synthetic room seen from n_kf poses, n_pts each, picked by
    default_rng(seed0 + kf)."""
    from mast3r_slam import synthetic

    out = []
    for kf in range(n_kf):
        T_wc = synthetic.camera_pose(kf * step)
        X = synthetic.render_pointmap(T_wc, h, w).reshape(-1, 3)
        sel = np.random.default_rng(seed0 + kf).permutation(len(X))[:n_pts]
        out.append(synthetic.sim3_act(T_wc, X[sel]).astype(np.float32))
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def room_case(form, move=BOX_MOVE.tobytes()):
    """(pred, gt, gt's normals, 500 samples) of the four-view room moved by `move`^-1.  form "exact": pred is gt itself,
    moved; "resampled": a second sampling, from default_rng(100 + kf)."""
    M = np.frombuffer(move, np.float64)
    gt = room_cloud()
    base = gt if form == "exact" else room_cloud(seed0=100)
    pred = A.act(A.sim3_inv(M), base.astype(np.float64)).astype(np.float32)
    return pred, gt, knn_normals(gt), C.stride_sample(pred, BOX_SAMPLES)[0]


def point_icp_states(src, gt, iters, trim=np.inf):
    """The states after every iteration of the point metric (cloud_numpy.icp_step) -> f64[iters, 8]."""
    T = A.init_state()
    out = np.zeros((iters, 8))
    for k in range(iters):
        T = C.icp_step(T, src, gt, trim)["T"]
        out[k] = T
    return out


def mesh_icp_states(P, vertices, faces, iters, trim):
    """The same for the point-to-mesh metric (meshalign_numpy.icp_step)."""
    T = A.init_state()
    out = np.zeros((iters, 8))
    for k in range(iters):
        T = A.icp_step(T, P, vertices, faces, trim)["T"]
        out[k] = T
    return out
