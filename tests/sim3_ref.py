"""The Sim3 pose algebra (csrc/sim3.h; mslam_sim3_op, mslam_sim3_act, lietorch_hip.Sim3) in float64, the measures that
compare a float32 pose with it, a float32 restatement of the formulae the kernels evaluate, the tolerance of the
exponential's translation row by row, and the input sets of tests/test_sim3_edges_gpu.py.  numpy / scipy only; nothing
here touches the device.  Pinned on its own in tests/test_sim3_ref_cpu.py.

Poses are lietorch's [t(3), q(xyzw), s]; tangent vectors are xi = [tau(3), phi(3), sigma].  Two poses are compared as
transforms, never quaternion by quaternion: q and -q are the same pose."""
import itertools

import numpy as np
import scipy.linalg
from scipy.spatial.transform import Rotation

F32_EPS = 2.0 ** -24        # unit roundoff of float32


# ---- Sim3 in float64 --------------------------------------------------------------------------------------------------
def sim3_matrix(T):
    """4x4 similarity [[s R, t], [0, 1]] of a pose [t(3), q(xyzw), s]."""
    T = np.asarray(T, np.float64)
    M = np.eye(4)
    M[:3, :3] = T[7] * Rotation.from_quat(T[3:7]).as_matrix()
    M[:3, 3] = T[:3]
    return M


def sim3_from_matrix(M):
    s = np.cbrt(np.linalg.det(M[:3, :3]))
    q = Rotation.from_matrix(M[:3, :3] / s).as_quat()
    return np.concatenate([M[:3, 3], q, [s]])


def sim3_generator(xi):
    xi = np.asarray(xi, np.float64)
    G = np.zeros((4, 4))
    p = xi[3:6]
    G[:3, :3] = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]]) + xi[6] * np.eye(3)
    G[:3, 3] = xi[:3]
    return G


def sim3_exp(xi):
    """Pose [t, q, s] of exp(xi), xi = [tau(3), phi(3), sigma]."""
    return sim3_from_matrix(scipy.linalg.expm(sim3_generator(xi)))


def sim3_retr(xi, T):
    """exp(xi) * T."""
    return sim3_from_matrix(scipy.linalg.expm(sim3_generator(xi)) @ sim3_matrix(T))


def sim3_log(T1, T0):
    """The xi with exp(xi) * T0 = T1, in float64: matrix logarithm of M(T1) M(T0)^-1."""
    G = np.real(scipy.linalg.logm(sim3_matrix(T1) @ np.linalg.inv(sim3_matrix(T0))))
    A = G[:3, :3]
    W = 0.5 * (A - A.T)
    return np.array([G[0, 3], G[1, 3], G[2, 3], W[2, 1], W[0, 2], W[1, 0], np.trace(A) / 3.0])


# ---- batched, through 4x4 matrices ------------------------------------------------------------------------------------
def matrices(T):
    """(n,4,4) float64 similarities of poses (n,8) of any float type; the quaternion is normalised in float64."""
    T = np.asarray(T, np.float64).reshape(-1, 8)
    M = np.zeros((T.shape[0], 4, 4))
    M[:, :3, :3] = T[:, 7, None, None] * Rotation.from_quat(T[:, 3:7]).as_matrix()
    M[:, :3, 3] = T[:, :3]
    M[:, 3, 3] = 1.0
    return M


def exp_m(xi):
    """(n,4,4) exp of tangent vectors (n,7): scipy's expm of the generator, row by row."""
    xi = np.asarray(xi, np.float64).reshape(-1, 7)
    return np.stack([scipy.linalg.expm(sim3_generator(x)) for x in xi])


def exp_closed_m(xi):
    """(n,4,4) exp in closed form, float64, every term well conditioned.  With z = sigma + i theta and
    f(z) = (e^z - 1) / z = integral_0^1 e^(zu) du, the translation is V tau with
      V = integral_0^1 e^(sigma u) R(u phi) du = C I + Im f [n]x + (C - Re f) [n]x^2,  C = f(sigma),  n = phi / theta,
    (A theta = Im f and B theta^2 = C - Re f in sim3.h's letters).  f comes from expm1, so no term cancels: each is
    known to a few 2^-53 of max(1, e^sigma), the natural size of V."""
    xi = np.asarray(xi, np.float64).reshape(-1, 7)
    tau, phi, sigma = xi[:, :3], xi[:, 3:6], xi[:, 6]
    theta = np.linalg.norm(phi, axis=1)
    n = phi / np.where(theta > 0, theta, 1.0)[:, None]
    z = sigma + 1j * theta
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(z != 0, np.expm1(z) / np.where(z != 0, z, 1.0), 1.0)
        C = np.where(sigma != 0, np.expm1(sigma) / np.where(sigma != 0, sigma, 1.0), 1.0)
    n_tau = np.cross(n, tau)
    t = C[:, None] * tau + f.imag[:, None] * n_tau + (C - f.real)[:, None] * np.cross(n, n_tau)
    M = np.zeros((xi.shape[0], 4, 4))
    M[:, :3, :3] = np.exp(sigma)[:, None, None] * Rotation.from_rotvec(phi).as_matrix()
    M[:, :3, 3] = t
    M[:, 3, 3] = 1.0
    return M


def inv_m(T):
    """(n,4,4) inverses of poses (n,8): [[R^T / s, -R^T t / s], [0, 1]], written out (no LU of a matrix whose entries
    span s and t)."""
    M = matrices(T)
    s = np.cbrt(np.linalg.det(M[:, :3, :3]))
    Rt = np.swapaxes(M[:, :3, :3], 1, 2) / (s * s)[:, None, None]
    out = np.zeros_like(M)
    out[:, :3, :3] = Rt
    out[:, :3, 3] = -np.einsum("nij,nj->ni", Rt, M[:, :3, 3])
    out[:, 3, 3] = 1.0
    return out


def mul_m(A, B):
    """(n,4,4) products A * B (X -> A(B(X))) of poses (n,8) or (1,8)."""
    return matrices(A) @ matrices(B)


def retr_m(xi, T):
    """(n,4,4) exp(xi) * T."""
    return exp_m(xi) @ matrices(T)


def act(T, X):
    """s R X + t in float64: poses (n,8) or (1,8), points (n,3) -> (n,3)."""
    M = matrices(T)
    return np.einsum("nij,nj->ni", M[:, :3, :3], np.asarray(X, np.float64)) + M[:, :3, 3]


# ---- error measures ---------------------------------------------------------------------------------------------------
def split(M):
    """(s, R, t) of similarities (n,4,4)."""
    s = np.cbrt(np.linalg.det(M[:, :3, :3]))
    return s, M[:, :3, :3] / s[:, None, None], M[:, :3, 3]


def pose_errors(T, M64):
    """Per row, how far poses T (n,8) are from the similarities M64 (n,4,4):
      rot   = angle of R R64^T (rad; through scipy's quaternion of the product, so small angles keep their digits),
      scale = |s / s64 - 1|,
      trans = |t - t64|_inf, NOT yet divided by the op's natural size (size_* below)."""
    T = np.asarray(T, np.float64).reshape(-1, 8)
    s64, R64, t64 = split(M64)
    R = Rotation.from_quat(T[:, 3:7]).as_matrix()
    rot = Rotation.from_matrix(R @ np.swapaxes(R64, 1, 2)).magnitude()
    return dict(rot=rot, scale=np.abs(T[:, 7] / s64 - 1.0), trans=np.abs(T[:, :3] - t64).max(1))


def _norm(v):
    return np.linalg.norm(np.asarray(v, np.float64), axis=-1)


def size_exp(xi):
    """|tau| max(1, e^sigma): V of exp_closed_m has norm at most max(1, e^sigma)."""
    xi = np.asarray(xi, np.float64).reshape(-1, 7)
    return _norm(xi[:, :3]) * np.maximum(1.0, np.exp(xi[:, 6]))


def size_inv(T):
    """|t| / s: the size of -R^T t / s."""
    T = np.asarray(T, np.float64).reshape(-1, 8)
    return _norm(T[:, :3]) / T[:, 7]


def size_mul(A, B):
    """s_A |t_B| + |t_A|: the sizes of the two terms of s_A R_A t_B + t_A.  A and B as poses (n,8) or (1,8), or as
    similarities (n,4,4)."""
    def st(P):
        P = np.asarray(P, np.float64)
        if P.ndim == 3:
            s, _, t = split(P)
            return s, _norm(t)
        P = P.reshape(-1, 8)
        return P[:, 7], _norm(P[:, :3])
    (sa, ta), (_, tb) = st(A), st(B)
    return sa * tb + ta


def size_act(T, X):
    """s |X| + |t|."""
    T = np.asarray(T, np.float64).reshape(-1, 8)
    return T[:, 7] * _norm(X) + _norm(T[:, :3])


def scaled(err, size):
    """err / size with 0 / 0 = 0 (an identity translation has no size and must come out exact)."""
    err, size = np.asarray(err, np.float64), np.asarray(size, np.float64)
    return np.where(size > 0, err / np.where(size > 0, size, 1.0), np.where(err > 0, np.inf, 0.0))


# ---- the formulae in float32 ------------------------------------------------------------------------------------------
# A vectorised restatement of what sim3.h evaluates (the reference's formulae), one float32 rounding per operation, no
# fused multiply-add.  exp, sin and cos are taken in float64 and rounded once, so they are the correctly rounded float32
# values on every machine; what a real expf / sinf / cosf may return instead is modelled by the nudges.
f32 = np.float32


def _nudge(x, k):
    """x moved by k float32 ulps (k steps of nextafter)."""
    to = f32(np.inf if k > 0 else -np.inf)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, to)
    return x


def _fn32(fn, x, k):
    return _nudge(fn(x.astype(np.float64)).astype(f32), k)


def _cross32(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def unit32(T):
    """sim3_unit (inv, mul, retr): q / sqrt(q.q) in float32, as 1 / sqrt times q."""
    T = np.array(T, f32).reshape(-1, 8)
    q = T[:, 3:7]
    n2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]
    inv = f32(1.0) / np.sqrt(n2)
    T[:, 3:7] = q * inv[:, None]
    return T


def unit64(T):
    """sim3_unit_f64 (gn.hip), the normalisation of Sim3.exp: the norm in float64, every component rounded once."""
    T = np.array(T, f32).reshape(-1, 8)
    q = T[:, 3:7].astype(np.float64)
    inv = 1.0 / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    T[:, 3:7] = (q * inv[:, None]).astype(f32)
    return T


def exp_branches(xi):
    """(sigma_small, theta_small) of every row as the float32 code decides them: |sigma| < 1e-6, theta < 1e-6.  A row
    with both set takes C, A and B as constants; every other row computes at least one of them by a difference."""
    xi = np.asarray(xi, f32).reshape(-1, 7)
    phi = xi[:, 3:6]
    theta = np.sqrt(phi[:, 0] * phi[:, 0] + phi[:, 1] * phi[:, 1] + phi[:, 2] * phi[:, 2])
    return np.abs(xi[:, 6]) < f32(1e-6), theta < f32(1e-6)


def exp32(xi, nudge=(0, 0, 0), unit=True):
    """sim3_exp in float32 (sim3.h:119-183).  nudge = (k_exp, k_sin, k_cos) moves exp(sigma), sin(theta) and cos(theta)
    by that many ulps.  The half-angle sin and cos of the quaternion take none: the rotation is well conditioned.
    Below theta^2 = 1e-6 the quaternion is a series in theta^2: +, -, x, / and sqrt only, each correctly rounded on the
    host and in the kernels (built without contraction), so that part can be compared bit for bit.  unit=True
    normalises as the op kernel does for exp (unit64); inside retr the exponential is not normalised."""
    xi = np.asarray(xi, f32).reshape(-1, 7)
    k_exp, k_sin, k_cos = nudge
    tau, phi, sigma = xi[:, :3], xi[:, 3:6], xi[:, 6]
    one, half = f32(1.0), f32(0.5)
    with np.errstate(all="ignore"):
        scale = _fn32(np.exp, sigma, k_exp)
        theta_sq = phi[:, 0] * phi[:, 0] + phi[:, 1] * phi[:, 1] + phi[:, 2] * phi[:, 2]
        theta = np.sqrt(theta_sq)
        # so3_exp
        p4 = theta_sq * theta_sq
        imag_s = half - f32(1.0 / 48.0) * theta_sq + f32(1.0 / 3840.0) * p4
        real_s = one - f32(1.0 / 8.0) * theta_sq + f32(1.0 / 384.0) * p4
        h = half * theta
        imag_l = _fn32(np.sin, h, 0) / theta
        real_l = _fn32(np.cos, h, 0)
        small = theta_sq < f32(1e-6)
        imag, real = np.where(small, imag_s, imag_l), np.where(small, real_s, real_l)
        q = np.concatenate([imag[:, None] * phi, real[:, None]], 1)
        # the W matrix's coefficients
        sin_t, cos_t = _fn32(np.sin, theta, k_sin), _fn32(np.cos, theta, k_cos)
        s_small, t_small = np.abs(sigma) < f32(1e-6), theta < f32(1e-6)
        sigma_sq = sigma * sigma
        C = np.where(s_small, one, (scale - one) / sigma)
        A00, B00 = half, f32(1.0 / 6.0)
        A01 = (one - cos_t) / theta_sq
        B01 = (theta - sin_t) / (theta_sq * theta)
        A10 = ((sigma - one) * scale + one) / sigma_sq
        B10 = (scale * half * sigma_sq + scale - one - sigma * scale) / (sigma_sq * sigma)
        a, b, c = scale * sin_t, scale * cos_t, theta_sq + sigma_sq
        A11 = (a * sigma + (one - b) * theta) / (theta * c)
        B11 = (C - ((b - one) * sigma + a * theta) / c) / theta_sq
        A = np.where(s_small, np.where(t_small, A00, A01), np.where(t_small, A10, A11)).astype(f32)
        B = np.where(s_small, np.where(t_small, B00, B01), np.where(t_small, B10, B11)).astype(f32)
        t = C[:, None] * tau
        w = _cross32(phi, tau)
        t = t + A[:, None] * w
        w = _cross32(phi, w)
        t = t + B[:, None] * w
    T = np.concatenate([t, q, scale[:, None]], 1).astype(f32)
    return unit64(T) if unit else T


def _quat_mul32(a, b):
    return np.stack([a[:, 3] * b[:, 0] + a[:, 0] * b[:, 3] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 3] * b[:, 1] - a[:, 0] * b[:, 2] + a[:, 1] * b[:, 3] + a[:, 2] * b[:, 0],
                     a[:, 3] * b[:, 2] + a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0] + a[:, 2] * b[:, 3],
                     a[:, 3] * b[:, 3] - a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1] - a[:, 2] * b[:, 2]], 1)


def _quat_rot32(q, X):
    """X + w u + q x u, u = 2 q x X."""
    u = f32(2.0) * _cross32(q[:, :3], X)
    return X + q[:, 3:4] * u + _cross32(q[:, :3], u)


def _rows(a, b, wa=8, wb=8):
    a, b = np.asarray(a, f32).reshape(-1, wa), np.asarray(b, f32).reshape(-1, wb)
    n = max(a.shape[0], b.shape[0])
    return np.broadcast_to(a, (n, wa)), np.broadcast_to(b, (n, wb))


def inv32(T, unit=True):
    T = np.asarray(T, f32).reshape(-1, 8)
    qi = T[:, 3:7] * np.array([-1, -1, -1, 1], f32)
    si = f32(1.0) / T[:, 7]
    t = -si[:, None] * _quat_rot32(qi, T[:, :3])
    out = np.concatenate([t, qi, si[:, None]], 1).astype(f32)
    return unit32(out) if unit else out


def mul32(A, B, unit=True):
    A, B = _rows(A, B)
    t = A[:, 7:8] * _quat_rot32(A[:, 3:7], B[:, :3]) + A[:, :3]
    out = np.concatenate([t, _quat_mul32(A[:, 3:7], B[:, 3:7]), (A[:, 7] * B[:, 7])[:, None]], 1).astype(f32)
    return unit32(out) if unit else out


def retr32(xi, T, unit=True):
    """exp(xi) * T; the exponential is not normalised in between (sim3_retr)."""
    xi, T = _rows(xi, T, 7, 8)
    return mul32(exp32(xi, unit=False), T, unit=unit)


def act32(T, X):
    T, X = _rows(T, X, 8, 3)
    return (_quat_rot32(T[:, 3:7], X) * T[:, 7:8] + T[:, :3]).astype(f32)


# ---- the exponential's grid and its translation tolerance -------------------------------------------------------------
THETAS = (0.0, 5e-7, 9.9e-7, 1.01e-6, 1e-5, 1e-4, 9.9e-4, 1.01e-3, 1e-2, 0.3, 3.0, np.pi, 6.0)
SIGMAS = (0.0, 5e-7, 1.01e-6, -1.01e-6, 1e-5, 1e-4, -1e-4, 1e-3, 1e-2, -1e-2, 0.3, -0.3, 3.0, -3.0)
PER_CELL = 8
NUDGES = tuple(itertools.product((-2, 0, 2), repeat=3))
CAP_ULPS = 64.0


def exp_grid():
    """(xi float32 (n,7), theta (n,), sigma (n,)): every (theta, sigma) cell of THETAS x SIGMAS - both sides of the
    three thresholds (|sigma| = 1e-6, theta = 1e-6, theta^2 = 1e-6), rotations at and beyond pi, scales from 1/20 to
    20 - with PER_CELL random unit axes and tau ~ N(0, 1).  theta and sigma are the cell's nominal values."""
    rng = np.random.default_rng(20240607)
    rows, th, sg = [], [], []
    for theta in THETAS:
        for sigma in SIGMAS:
            ax = rng.normal(size=(PER_CELL, 3))
            ax /= np.linalg.norm(ax, axis=1, keepdims=True)
            tau = rng.normal(size=(PER_CELL, 3))
            rows.append(np.concatenate([tau, theta * ax, np.full((PER_CELL, 1), sigma)], 1))
            th += [theta] * PER_CELL
            sg += [sigma] * PER_CELL
    return np.concatenate(rows).astype(f32), np.array(th), np.array(sg)


def exp_trans_tol(xi, M64=None):
    """Per row, the absolute tolerance of exp's translation in float32:
        2 x max over the 27 nudges in {-2, 0, +2}^3 of |t32 - t64|_inf  +  4 x 2^-24 |t64|_inf.
    expf, sinf and cosf of a host or device library are each within 1 ulp of the true value, so two libraries differ by
    up to 2 ulps: the nudges span that.  The factor 2 covers the roundings of the remaining arithmetic, which the nudges
    do not move, taken in another order; the last term is the rounding of the result itself, so the tolerance is never
    zero.  Where the formula is well conditioned this is a few ulps of the translation; where C, A or B lose their
    digits to cancellation it is as wide as the formula is uncertain, and no wider."""
    xi = np.asarray(xi, f32).reshape(-1, 7)
    t64 = (exp_m(xi) if M64 is None else M64)[:, :3, 3]
    dev = np.zeros(xi.shape[0])
    for nd in NUDGES:
        dev = np.maximum(dev, np.abs(exp32(xi, nd)[:, :3].astype(np.float64) - t64).max(1))
    return 2.0 * dev + 4.0 * F32_EPS * np.abs(t64).max(1)


def exp_cap(xi):
    """64 x 2^-24 |tau| max(1, e^sigma): a row whose tolerance is below this is held to a few dozen ulps."""
    return CAP_ULPS * F32_EPS * size_exp(xi)


def well_conditioned(theta, sigma):
    """The cells every formula evaluates without a cancelling difference of nearly equal numbers."""
    theta, sigma = np.asarray(theta), np.asarray(sigma)
    return ((sigma == 0) | (np.abs(sigma) >= 0.3)) & ((theta == 0) | (theta >= 0.3))


# ---- pose, point and step inputs --------------------------------------------------------------------------------------
def poses(n, seed=0):
    """(n,8) float32 poses: scale log-uniform over [1e-3, 1e3]; |t| log-uniform over [1e-3, 1e3] in a random direction,
    every eighth row t = 0; rotations random, every fifth row the identity, every seventh within 1e-3 rad of pi; every
    other quaternion negated.  Quaternions are normalised in float64 and rounded: unit to a few 2^-24."""
    rng = np.random.default_rng([seed, n, 8])
    k = np.arange(n)
    s = 10.0 ** rng.uniform(-3, 3, n)
    d = rng.normal(size=(n, 3))
    t = d / np.linalg.norm(d, axis=1, keepdims=True) * (10.0 ** rng.uniform(-3, 3, n))[:, None]
    t[k % 8 == 3] = 0.0
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = rng.uniform(0, np.pi, n)
    ang[k % 5 == 1] = 0.0
    near = k % 7 == 2
    ang[near] = np.pi - rng.uniform(0, 1e-3, near.sum())
    q = Rotation.from_rotvec(ax * ang[:, None]).as_quat()
    q[k % 2 == 1] *= -1.0
    return np.concatenate([t, q, s[:, None]], 1).astype(f32)


def points(n, seed=0):
    """(n,3) float32 points, |X| log-uniform over [1e-2, 1e2], every ninth the origin."""
    rng = np.random.default_rng([seed, n, 3])
    d = rng.normal(size=(n, 3))
    X = d / np.linalg.norm(d, axis=1, keepdims=True) * (10.0 ** rng.uniform(-2, 2, n))[:, None]
    X[np.arange(n) % 9 == 4] = 0.0
    return X.astype(f32)


def steps(n, seed=0):
    """(n,7) float32 tangent vectors for retr, from the well-conditioned cells of the exponential only (the others have
    their own row-wise tolerance and would drown every other term of retr): tau ~ N(0, 1); theta uniform in
    [0.3, pi], every fourth row 0; |sigma| uniform in [0.3, 1] with either sign, every third row 0; row 0 is zero."""
    rng = np.random.default_rng([seed, n, 7])
    k = np.arange(n)
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    theta = rng.uniform(0.3, np.pi, n)
    theta[k % 4 == 2] = 0.0
    sigma = rng.uniform(0.3, 1.0, n) * rng.choice([-1.0, 1.0], n)
    sigma[k % 3 == 1] = 0.0
    xi = np.concatenate([rng.normal(size=(n, 3)), ax * theta[:, None], sigma[:, None]], 1)
    xi[0] = 0.0
    return xi.astype(f32)


N_BASE = 1000      # the largest batch the GPU tests run; the baselines are measured on it


# ---- float32 baselines ------------------------------------------------------------------------------------------------
# Each constant is the largest error, against float64, of the float32 formulae on the inputs the GPU tests use:
# exp on exp_grid() (rotation and scale; the translation has exp_trans_tol), inv / mul / retr / act on poses(N_BASE),
# points(N_BASE) and steps(N_BASE) with the seeds of measure_baselines().  "The float32 formulae" are the restatement
# above and, where it has the op, the C oracle (oracle.sim3_exp, sim3_retr, sim3_act, and sim3_rel = Ti^-1 Tj measured
# as a product with float64's Ti^-1 on the left); the maximum of the two is taken, as
# tests/test_sim3_ref_cpu.py::test_fp32_baselines prints it, rounded up to two digits.  That test fails when a fresh
# measurement is not within half to one and a half times a constant.  They are properties of float32 arithmetic on these
# inputs, not of the kernels; the GPU tests allow FACTOR = 4 times them for another sqrt / division schedule and fmaf.
# rot in rad, scale as |s / s64 - 1|, trans as |t - t64|_inf over the op's natural size (size_*).
BASELINES = {
    "exp": dict(rot=4.1e-7, scale=5.7e-8),                  # measured 4.06e-07 (theta = 6: the half angle's rounding), 5.63e-08
    "inv": dict(rot=6.5e-8, scale=5.9e-8, trans=2.8e-7),    # measured 6.44e-08, 5.82e-08, 2.77e-07
    "mul": dict(rot=2.2e-7, scale=9.5e-8, trans=2.8e-7),    # measured 2.16e-07, 9.40e-08 (sim3_rel: two roundings), 2.79e-07
    "retr": dict(rot=2.6e-7, scale=1.1e-7, trans=2.9e-7),   # measured 2.54e-07, 1.06e-07, 2.89e-07
    "act": dict(trans=4.4e-7),                              # measured 4.33e-07
}
FACTOR = 4.0


def measure(T32, M64, size=None):
    """{rot, scale, trans}: the maxima of pose_errors over the rows, trans divided by `size` (left out without one)."""
    e = pose_errors(T32, M64)
    out = dict(rot=float(e["rot"].max()), scale=float(e["scale"].max()))
    if size is not None:
        out["trans"] = float(scaled(e["trans"], size).max())
    return out


def base_inputs():
    """The inputs of inv / mul / retr / act: A, B poses, xi steps, X points, N_BASE rows each."""
    return dict(A=poses(N_BASE, 1), B=poses(N_BASE, 2), xi=steps(N_BASE, 3), X=points(N_BASE, 4))


def measure_baselines(oracle=None):
    """{op: {measure: value}} of the restatement, and of the C oracle too when the module is passed."""
    xi_g, _, _ = exp_grid()
    d = base_inputs()
    A, B, xi, X = d["A"], d["B"], d["xi"], d["X"]
    runs = {"exp": [measure(exp32(xi_g), exp_m(xi_g))],
            "inv": [measure(inv32(A), inv_m(A), size_inv(A))],
            "mul": [measure(mul32(A, B), mul_m(A, B), size_mul(A, B))],
            "retr": [measure(retr32(xi, B), retr_m(xi, B), size_mul(exp_m(xi), B))],
            "act": [dict(trans=float(scaled(np.abs(act32(A, X) - act(A, X)).max(1), size_act(A, X)).max()))]}
    if oracle is not None:
        runs["exp"].append(measure(oracle.sim3_exp(xi_g), exp_m(xi_g)))
        runs["retr"].append(measure(oracle.sim3_retr(xi, B), retr_m(xi, B), size_mul(exp_m(xi), B)))
        Ai = inv_m(A)
        runs["mul"].append(measure(oracle.sim3_rel(A, B), Ai @ matrices(B), size_mul(Ai, B)))
        Y = np.stack([oracle.sim3_act(A[k], X[k:k + 1])[0] for k in range(N_BASE)])
        runs["act"].append(dict(trans=float(scaled(np.abs(Y - act(A, X)).max(1), size_act(A, X)).max())))
    return {op: {k: max(r[k] for r in rs) for k in rs[0]} for op, rs in runs.items()}
