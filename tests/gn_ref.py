"""Plain float64 reference of ONE accumulation pass of the global Gauss-Newton backend (csrc/gn.hip: gn_compact,
gn_accum, gn_reduce) over directed edges, for the three residual kinds, the dense normal equations and their Cholesky
step, and the input sets of tests/test_gn_blocks_gpu.py and tests/test_gn_loop_gpu.py.  Written in the reference's form:
per point the Jacobian of the residual with respect to the point P = Ti^-1 Tj Xj, times dP/dxi = [I, -[P]x, P] in frame
i, carried to a left perturbation of the world pose Tj by the adjoint of Ti^-1 (computed from the group's generators,
Ti^-1 G Ti), Ji = -Jj, A = sqrt(w) [Ji, Jj], H = A^T A - never in the kernel's regrouped M B M^T form with its 35
accumulators.  numpy / scipy only; nothing here touches the device.  Pinned on its own in tests/test_gn_ref_cpu.py
(finite differences, the float32 oracle, populations of the input sets, float32 baselines)."""
import functools

import numpy as np
import scipy.linalg

from mast3r_slam import synthetic
from tracker_ref import HUBER, _huber, _ray_dist, _skew, sim3_generator, sim3_matrix

KINDS = ("rays", "calib", "points")
ROWS = {"rays": 4, "calib": 3, "points": 3}
# rows of the strong family (a: unit ray | pixel | point, sigma_a) and of the weak one (b: distance | log depth, sigma_b)
FAMILY_A = {"rays": (0, 1, 2), "calib": (0, 1), "points": (0, 1, 2)}
FAMILY_B = {"rays": (3,), "calib": (2,), "points": ()}

# Production values (config["local_opt"]) and the sets under which the weak family carries the blocks: rays (10, 0.01) /
# calib (100, 0.01).  On the graphs of cases() they need no further adjustment: the weak family holds > 99.8 % of every
# edge's trace and 58-76 % of its rows are Huber outliers; what is tuned instead is the pose noise of the graphs under
# the production sigmas (NOISE below).  All of it is asserted in test_gn_ref_cpu.py::test_populations.
SIGMAS = {"rays": (0.003, 10.0), "calib": (1.0, 10.0), "points": (0.05, 0.0)}
WEAK_SIGMAS = {"rays": (10.0, 0.01), "calib": (100.0, 0.01)}

BORDER_MARGIN, Z_MARGIN = 1e-3, 1e-4    # no compacted point this close to a gate: float32 and float64 agree on every gate

# float32 baselines: oracle.gn_edges (the float32 scalar restatement of the reference's edge kernels, 256 virtual threads
# and its reduction tree) on every input set of cases(), measured against edges() with block_errors(); and one iteration
# of oracle.gauss_newton on the step cases measured with backward_error().  Each constant is the maximum over the input
# sets as tests/test_gn_ref_cpu.py::test_fp32_baselines prints it, rounded up to two digits; that test fails when a fresh
# measurement is not within half to one and a half times them.  They are a property of float32 arithmetic on these
# inputs, never of the kernel.  Where each maximum occurs is noted beside it.
FP32_ERRH_BASELINE = 4.6e-6         # 4.533e-06 at chunks-rays-5 (five points: nothing averages out); up to 3.7e-6 elsewhere
FP32_ERRG_BASELINE = 8.5e-6         # 8.411e-06 at calib-weak-96x128
FP32_BACKWARD_BASELINE = 8.5e-7     # 8.442e-07 at calib-weak-24x32


# ---- the kernel's work split, restated ------------------------------------------------------------------------------------
def carve(E, HW):
    """(S, chunk_len) of gn_carve: every edge is split into S = min(ceil(1024 / E), max(HW / 4096, 1)) chunks of
    chunk_len = align256(ceil(HW / S)) points."""
    S = max(1, min(-(-1024 // E), max(HW // 4096, 1)))
    chunk_len = max(256, -(-(-(-HW // S)) // 256) * 256)
    return S, chunk_len


def chunk_counts(mask, E, HW):
    """Survivors of every chunk, (E, S), from a boolean (E, HW) mask."""
    S, L = carve(E, HW)
    return np.stack([mask[:, c * L:min(HW, (c + 1) * L)].sum(1) for c in range(S)], 1)


# ---- Sim3 -------------------------------------------------------------------------------------------------------------------
def _vee(G):
    A = G[:3, :3]
    W = 0.5 * (A - A.T)
    return np.array([G[0, 3], G[1, 3], G[2, 3], W[2, 1], W[0, 2], W[1, 0], np.trace(A) / 3.0])


def adjoint_inv(Mi):
    """7x7 Ad(Ti^-1): column k is vee(Ti^-1 G_k Ti).  Ti^-1 exp(xi) Tj = exp(Ad(Ti^-1) xi) Ti^-1 Tj."""
    Minv = np.linalg.inv(Mi)
    return np.stack([_vee(Minv @ sim3_generator(np.eye(7)[k]) @ Mi) for k in range(7)], 1)


def _as_matrix(T):
    T = np.asarray(T, np.float64)
    return T if T.ndim == 2 else sim3_matrix(T)


# ---- residual rows of one directed edge ---------------------------------------------------------------------------------------
def point_rows(kind, Ti, Tj, Xi, Xj, ind=None, K=None, width=1, z_eps=0.0):
    """Residuals e (n, rows) and Jacobians J (n, rows, 14) = [d e / d xi_i, d e / d xi_j] (left perturbations exp(xi) T
    of the world poses) of matched points Xi (in frame i, already gathered) and Xj (in frame j); P = Ti^-1 Tj Xj (n, 3).
    calib: rows whose depths are at or below z_eps are evaluated with the depth replaced by 1 (they are gated)."""
    Mi, Mj = _as_matrix(Ti), _as_matrix(Tj)
    Xi, Xj = np.asarray(Xi, np.float64), np.asarray(Xj, np.float64)
    Mij = np.linalg.inv(Mi) @ Mj
    P = Xj @ Mij[:3, :3].T + Mij[:3, 3]
    n = P.shape[0]
    dP = np.concatenate([np.broadcast_to(np.eye(3), (n, 3, 3)), -_skew(P), P[:, :, None]], -1)          # (n,3,7), frame i
    if kind == "rays":
        rd_j, drd = _ray_dist(P, jac=True)
        e = rd_j - _ray_dist(Xi)
        dres = drd                                                                                      # (n,4,3)
    elif kind == "calib":
        K = np.asarray(K, np.float64)
        ok = (P[:, 2] > z_eps) & (Xi[:, 2] > z_eps)
        z = np.where(ok, P[:, 2], 1.0)
        zi = np.where(ok, Xi[:, 2], 1.0)
        u = K[0, 0] * P[:, 0] / z + K[0, 2]
        v = K[1, 1] * P[:, 1] / z + K[1, 2]
        ind = np.asarray(ind, np.int64)
        e = np.stack([u - ind % width, v - ind // width, np.log(z) - np.log(zi)], -1)
        dres = np.zeros((n, 3, 3))
        dres[:, 0, 0] = K[0, 0] / z
        dres[:, 1, 1] = K[1, 1] / z
        dres[:, 0, 2] = -K[0, 0] * P[:, 0] / z ** 2
        dres[:, 1, 2] = -K[1, 1] * P[:, 1] / z ** 2
        dres[:, 2, 2] = 1.0 / z
    else:
        e = P - Xi
        dres = np.broadcast_to(np.eye(3), (n, 3, 3))
    Jj = (dres @ dP) @ adjoint_inv(Mi)
    return e, np.concatenate([-Jj, Jj], -1), P


def edges(kind, Twc, Xs, Cs, K, ie, je, idx, valid_match, Q, sigma_a, sigma_b, C_thresh, Q_thresh, height=0, width=1,
          pixel_border=0, z_eps=0.0, huber=HUBER):
    """One accumulation pass.  ie / je are ROW indices into Twc / Xs.  Per edge (leading axis E):
      H (E,14,14) = A^T A, g (E,14) = A^T b, cost (E) = 1/2 b^T b with A = sqrt(w) [Ji, Jj], b = sqrt(w) e,
      w = huber(sqrt_info e) sqrt_info^2, sqrt_info = sqrt(Q) / sigma on the rows that pass every gate, 0 elsewhere;
      Hfam / gfam / costfam (2,E,...): the same sums over the rows of family a and of family b alone;
      Habs / gabs: the sums with every term in absolute value;
      compact (E,HW): the pose-independent gates (valid_match, Q > Q_thresh, Ci[idx] > C_thresh, Cj > C_thresh);
      valid_zi, valid_zj, in_border (E,HW; calib): the pose-dependent gates of every point, before `compact`;
      rows (E,HW): the points that take part; ind (E,HW): the gathered index (0 where valid_match is 0);
      whitened: list of (n_e, rows) arrays, sqrt_info e of the points that take part."""
    f8 = lambda a: np.asarray(a, np.float64)
    Twc, Xs, Cs = f8(Twc), f8(Xs), f8(Cs).reshape(Xs.shape[0], -1)
    idx, vm = np.asarray(idx, np.int64), np.asarray(valid_match).reshape(idx.shape) != 0
    Q = f8(Q).reshape(idx.shape)
    E, HW = idx.shape
    nr = ROWS[kind]
    fam = np.zeros(nr, int)
    fam[list(FAMILY_B[kind])] = 1
    sig = np.where(fam == 0, sigma_a, sigma_b if kind != "points" else 1.0)
    out = dict(H=np.zeros((E, 14, 14)), g=np.zeros((E, 14)), cost=np.zeros(E), Hfam=np.zeros((2, E, 14, 14)),
               gfam=np.zeros((2, E, 14)), costfam=np.zeros((2, E)), Habs=np.zeros((E, 14, 14)), gabs=np.zeros((E, 14)),
               compact=np.zeros((E, HW), bool), rows=np.zeros((E, HW), bool), ind=np.zeros((E, HW), np.int64), whitened=[])
    if kind == "calib":
        out.update(valid_zi=np.zeros((E, HW), bool), valid_zj=np.zeros((E, HW), bool), in_border=np.zeros((E, HW), bool))
    for e in range(E):
        i, j = int(ie[e]), int(je[e])
        ind = np.where(vm[e], idx[e], 0)
        with np.errstate(invalid="ignore"):
            compact = vm[e] & (Q[e] > Q_thresh) & (Cs[i][ind] > C_thresh) & (Cs[j] > C_thresh)
        out["compact"][e], out["ind"][e] = compact, ind
        rows = compact.copy()
        if kind == "calib":          # the gates of every point, with the unreadable ones (NaN) counted as failing
            with np.errstate(invalid="ignore", divide="ignore"):
                _, _, P = point_rows("points", Twc[i], Twc[j], Xs[i][ind], Xs[j])
                Kd = f8(K)
                u, v = Kd[0, 0] * P[:, 0] / P[:, 2] + Kd[0, 2], Kd[1, 1] * P[:, 1] / P[:, 2] + Kd[1, 2]
                out["valid_zi"][e] = Xs[i][ind][:, 2] > z_eps
                out["valid_zj"][e] = P[:, 2] > z_eps
                out["in_border"][e] = ((u > pixel_border) & (u < width - 1 - pixel_border) & (v > pixel_border)
                                       & (v < height - 1 - pixel_border))
            rows &= out["valid_zi"][e] & out["valid_zj"][e] & out["in_border"][e]
        out["rows"][e] = rows
        k = np.flatnonzero(rows)
        if len(k) == 0:
            out["whitened"].append(np.zeros((0, nr)))
            continue
        res, J, _ = point_rows(kind, Twc[i], Twc[j], Xs[i][ind[k]], Xs[j][k], ind=ind[k], K=K, width=width, z_eps=z_eps)
        sqrt_info = np.sqrt(Q[e][k])[:, None] / sig[None, :]
        whitened = sqrt_info * res
        robust = sqrt_info * np.sqrt(_huber(whitened, huber))
        out["whitened"].append(whitened)
        for f in (0, 1):
            r = np.flatnonzero(fam == f)
            if len(r) == 0:
                continue
            A = (robust[:, r, None] * J[:, r]).reshape(-1, 14)
            b = (robust[:, r] * res[:, r]).reshape(-1)
            out["Hfam"][f, e] = A.T @ A
            out["gfam"][f, e] = A.T @ b
            out["costfam"][f, e] = 0.5 * float(b @ b)
            out["Habs"][e] += np.abs(A).T @ np.abs(A)
            out["gabs"][e] += np.abs(A).T @ np.abs(b)
    out["H"], out["g"], out["cost"] = out["Hfam"].sum(0), out["gfam"].sum(0), out["costfam"].sum(0)
    return out


def blocks(H, g):
    """(E,14,14), (E,14) -> the reference's layout Hs (4,E,7,7) = [ii, ij, ji, jj], gs (2,E,7) = [i, j]."""
    return np.stack([H[:, :7, :7], H[:, :7, 7:], H[:, 7:, :7], H[:, 7:, 7:]]), np.stack([g[:, :7], g[:, 7:]])


def block_errors(ref, Hs, gs):
    """Per directed edge, the maximum over the four blocks / two gradients of
      errH = max_ab |A_ab - Â_ab| / sqrt(Â_aa Â_bb),  errg = max_a |g_a - ĝ_a| / sqrt(2 ĉ Â_aa),
    each block against its own reference, with Â (the diagonal), ĉ from the float64 ii block and cost.  Both denominators
    bound every summand's magnitude (Cauchy-Schwarz).  Where Â_aa = 0 (an edge without a survivor) the entry must be
    exactly 0: asserted here.  -> (errH (E), errg (E))."""
    Hr, gr = blocks(ref["H"], ref["g"])
    Hs, gs = np.asarray(Hs, np.float64), np.asarray(gs, np.float64)
    E = Hr.shape[1]
    eH, eg = np.zeros(E), np.zeros(E)
    for e in range(E):
        d = np.sqrt(np.diagonal(Hr[0, e]))
        if not (d > 0).all():
            assert not d.any() and ref["cost"][e] == 0, e
            assert not Hs[:, e].any() and not gs[:, e].any(), f"edge {e} has no survivor but non-zero blocks"
            continue
        eH[e] = max(np.max(np.abs(Hs[b, e] - Hr[b, e]) / np.outer(d, d)) for b in range(4))
        eg[e] = max(np.max(np.abs(gs[b, e] - gr[b, e]) / (np.sqrt(2 * ref["cost"][e]) * d)) for b in range(2))
    return eH, eg


# ---- dense normal equations -------------------------------------------------------------------------------------------------
def edge_rows(ii, jj):
    """Global keyframe ids -> row indices (sorted unique ids; the first is the pinned pose)."""
    uniq = np.unique(np.concatenate([ii, jj]))
    return np.searchsorted(uniq, ii), np.searchsorted(uniq, jj)


def dense(ref, ie, je, N):
    """The (7N, 7N) system H x = b of the N unpinned poses (row index - 1; the pinned pose's rows and columns dropped)
    from the per-edge sums, and the same with every term in absolute value.  The step is dx = -x."""
    n = 7 * N
    out = dict(H=np.zeros((n, n)), b=np.zeros(n), Habs=np.zeros((n, n)), babs=np.zeros(n))
    for e in range(len(ie)):
        sl = [slice(7 * (r - 1), 7 * r) if r >= 1 else None for r in (int(ie[e]), int(je[e]))]
        for a in (0, 1):
            if sl[a] is None:
                continue
            out["b"][sl[a]] += ref["g"][e, 7 * a:7 * a + 7]
            out["babs"][sl[a]] += ref["gabs"][e, 7 * a:7 * a + 7]
            for c in (0, 1):
                if sl[c] is not None:
                    out["H"][sl[a], sl[c]] += ref["H"][e, 7 * a:7 * a + 7, 7 * c:7 * c + 7]
                    out["Habs"][sl[a], sl[c]] += ref["Habs"][e, 7 * a:7 * a + 7, 7 * c:7 * c + 7]
    return out


def solve(sys):
    """dx (N,7) = -H^-1 b by scipy's Cholesky."""
    return -scipy.linalg.cho_solve(scipy.linalg.cho_factor(sys["H"], lower=True), sys["b"]).reshape(-1, 7)


def backward_error(sys, dx):
    """max_i |(H x - b)_i| / (sum_j Habs_ij |x_j| + babs_i) with x = -dx: how far dx is from solving the reference's normal
    equations, in units of the sums' own magnitude - independent of the conditioning of H."""
    x = -np.asarray(dx, np.float64).reshape(-1)
    return float(np.max(np.abs(sys["H"] @ x - sys["b"]) / (sys["Habs"] @ np.abs(x) + sys["babs"])))


def outlier_fraction(ref, kind, family, k=HUBER):
    """Fraction of the rows of a family (0: a, 1: b) that lie in Huber's outlier branch, over all edges."""
    r = list((FAMILY_A, FAMILY_B)[family][kind])
    w = np.concatenate(ref["whitened"])[:, r]
    return float((np.abs(w) >= k).mean())


def weak_trace_share(ref):
    """Per edge, the weak family's share of the trace of the ii block."""
    tr = np.trace(ref["H"][:, :7, :7], axis1=1, axis2=2)
    return np.trace(ref["Hfam"][1][:, :7, :7], axis1=1, axis2=2) / np.where(tr > 0, tr, 1.0)


# ---- input sets ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph(n_kf, h, w, seed, pose_noise=0.01, point_noise=0.0):
    return synthetic.make_graph(n_kf=n_kf, h=h, w=w, seed=seed, pose_noise=pose_noise, point_noise=point_noise)


def _case(name, kind, g, sigmas, C_thresh=0.0, Q_thresh=1.5, pixel_border=-10, z_eps=1e-6, step=False, **extra):
    E, HW = g["idx_ii2jj"].shape
    return dict(name=name, kind=kind, g=g, sigma_a=sigmas[0], sigma_b=sigmas[1], C_thresh=C_thresh, Q_thresh=Q_thresh,
                pixel_border=pixel_border, z_eps=z_eps, h=g["h"], w=g["w"], E=E, HW=HW, P=g["Xs"].shape[0], step=step,
                split=carve(E, HW), **extra)


def _first_points(g, HW):
    """The first HW points of every keyframe of a graph: Xs / Cs / idx / valid / Q cut to HW, matches that pointed behind
    the cut re-aimed at idx mod HW (in range; mostly gross mismatches, which Huber then handles).  No image shape."""
    idx = g["idx_ii2jj"][:, :HW] % HW
    out = dict(g, Xs=np.ascontiguousarray(g["Xs"][:, :HW]), Cs=np.ascontiguousarray(g["Cs"][:, :HW]), idx_ii2jj=idx,
               valid_match=np.ascontiguousarray(g["valid_match"][:, :HW]), Q=np.ascontiguousarray(g["Q"][:, :HW]), h=0, w=0)
    if HW <= 5:
        out["valid_match"] = np.ones_like(out["valid_match"])
    return out


CHUNK_SMALL = (1, 3, 5, 255, 257, 1023, 1025)
CHUNK_S3 = 12325
CHUNK_S18 = 73729
S18_SURVIVORS = (0, 1, 2, 3, 4, 5, 1023, 1024, 1025)      # chunks 0-8; chunks 9-16 keep all of their points, 17 has none


def _prescribed(g):
    """valid_match of the S = 18 shape set so that chunk c < 9 of either edge keeps exactly S18_SURVIVORS[c] points, at
    random places, and every later chunk all of its points (the case runs with both thresholds at 0)."""
    E, HW = g["idx_ii2jj"].shape
    S, L = carve(E, HW)
    rng = np.random.default_rng(18)
    vm = np.ones((E, HW, 1), bool)
    for e in range(E):
        for c, n in enumerate(S18_SURVIVORS):
            vm[e, c * L:(c + 1) * L] = False
            vm[e, c * L + rng.choice(L, n, replace=False)] = True
    return dict(g, valid_match=vm)


def _gated(g, z_eps, pixel_border):
    """calib gates: an eighth of every keyframe's points moved to a depth at or below z_eps a
    tenth mirrored through the camera centre (behind the camera, in either role); then every match that lies within the
    margins of a gate at the initial poses is switched off, so that float32 and float64 agree on every gate."""
    rng = np.random.default_rng(5)
    Xs = g["Xs"].copy()
    P, HW = Xs.shape[:2]
    r = rng.uniform(size=(P, HW))
    low = r < 0.125
    Xs[..., 2] = np.where(low, rng.uniform(-0.05, z_eps - 2 * Z_MARGIN, (P, HW)), Xs[..., 2])
    Xs[(r > 0.9)] *= -1.0
    Xs = Xs.astype(np.float32)
    g = dict(g, Xs=Xs)
    ie, je = edge_rows(g["ii"], g["jj"])
    vm = g["valid_match"].copy()
    Kd = g["K"].astype(np.float64)
    for e in range(len(ie)):
        ind = np.where(vm[e, :, 0], g["idx_ii2jj"][e], 0)
        _, _, Pj = point_rows("points", g["Twc"][ie[e]], g["Twc"][je[e]], Xs[ie[e]][ind], Xs[je[e]])
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = Kd[0, 0] * Pj[:, 0] / Pj[:, 2] + Kd[0, 2], Kd[1, 1] * Pj[:, 1] / Pj[:, 2] + Kd[1, 2]
        near = (np.abs(Pj[:, 2] - z_eps) < Z_MARGIN)
        zi = Xs[ie[e]][ind][:, 2].astype(np.float64)
        near |= np.abs(zi - z_eps) < Z_MARGIN
        for x, hi in ((u, g["w"] - 1 - pixel_border), (v, g["h"] - 1 - pixel_border)):
            near |= (np.abs(x - pixel_border) < BORDER_MARGIN) | (np.abs(x - hi) < BORDER_MARGIN)
        vm[e, near, 0] = False
    return dict(g, valid_match=vm)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: input set} of tests/test_gn_blocks_gpu.py and tests/test_gn_loop_gpu.py, built once."""
    out = []
    # every kind x both sigma sets at 24x32 (S = 1) and at 96x128 (S = 3, HW an exact multiple): blocks and one step
    for h, w, n_kf, seed in ((24, 32, 4, 3), (96, 128, 5, 4)):
        for kind in KINDS:
            g = _graph(n_kf, h, w, seed, *NOISE[kind])
            out.append(_case(f"{kind}-production-{h}x{w}", kind, g, SIGMAS[kind], step=True))
            if kind in WEAK_SIGMAS:
                gw = _graph(n_kf, h, w, seed, *NOISE_WEAK[kind])
                out.append(_case(f"{kind}-weak-{h}x{w}", kind, gw, WEAK_SIGMAS[kind], step=True))
    # calib gates, and the confidence thresholds of test_compaction_gates for every kind
    gg = _gated(_graph(5, 48, 64, 9, *NOISE["calib"]), 0.05, 2)
    out.append(_case("gates", "calib", gg, SIGMAS["calib"], pixel_border=2, z_eps=0.05))
    out.append(_case("gates-thresholds", "calib", gg, SIGMAS["calib"], C_thresh=1.8, Q_thresh=2.4, pixel_border=2, z_eps=0.05))
    for kind in KINDS:
        out.append(_case(f"thresholds-{kind}", kind, _graph(5, 48, 64, 9, *NOISE[kind]), SIGMAS[kind], C_thresh=1.8, Q_thresh=2.4))
    # chunk shapes, two directed edges: any num_points for rays and points, 95x130 for calib
    small, big = _graph(2, 33, 32, 6, *NOISE["rays"]), _graph(2, 240, 320, 6, *NOISE["rays"])
    for HW in CHUNK_SMALL + (CHUNK_S3, CHUNK_S18):
        g = _first_points(small if HW <= 1025 else big, HW)
        for kind in ("rays", "points"):
            out.append(_case(f"chunks-{kind}-{HW}", kind, g, SIGMAS[kind], chunks=True))
    gp = _prescribed(_first_points(big, CHUNK_S18))
    for kind in ("rays", "points"):
        out.append(_case(f"chunks-{kind}-{CHUNK_S18}-prescribed", kind, gp, SIGMAS[kind], Q_thresh=0.0, chunks=True))
    out.append(_case("chunks-calib-95x130", "calib", _graph(2, 95, 130, 6, *NOISE["calib"]), SIGMAS["calib"], pixel_border=2,
                     z_eps=0.05, chunks=True))
    out = {c["name"]: c for c in out}
    # the split every chunk case is meant to hit
    for HW in CHUNK_SMALL:
        assert out[f"chunks-rays-{HW}"]["split"] == (1, max(256, -(-HW // 256) * 256))
    assert out[f"chunks-rays-{CHUNK_S3}"]["split"] == (3, 4352) and CHUNK_S3 - 2 * 4352 == 3621
    assert out[f"chunks-rays-{CHUNK_S18}"]["split"] == (18, 4352) and CHUNK_S18 - 16 * 4352 == 4097      # chunk 16
    assert 17 * 4352 > CHUNK_S18                                   # chunk 17 begins behind the end
    assert out["chunks-calib-95x130"]["split"] == (3, 4352) and 95 * 130 - 2 * 4352 == 3646
    assert out["rays-production-96x128"]["split"][0] == 3 and out["rays-production-24x32"]["split"][0] == 1
    return out


# (pose_noise, point_noise) of make_graph per kind and sigma set, tuned so that 20-80 % of the rows of the family under
# test are Huber outliers (asserted in test_gn_ref_cpu.py::test_populations).  rays: at 24x32 the nearest-pixel matches
# alone put ~75 % of the unit-ray rows outside 1.345 sigma (half a pixel is 0.016 rad against sigma = 0.003), so the
# poses add little; points: 0.01 leaves only 12-19 % outside.
NOISE = {"rays": (0.002, 0.0), "calib": (0.01, 0.0), "points": (0.03, 0.0)}
NOISE_WEAK = {"rays": (0.01, 0.0), "calib": (0.01, 0.0)}


def reference(c, Twc=None, **over):
    """edges() of an input set at its initial poses (or at Twc)."""
    g = c["g"]
    ie, je = edge_rows(g["ii"], g["jj"])
    a = dict(sigma_a=c["sigma_a"], sigma_b=c["sigma_b"], C_thresh=c["C_thresh"], Q_thresh=c["Q_thresh"], height=c["h"],
             width=max(c["w"], 1), pixel_border=c["pixel_border"], z_eps=c["z_eps"])
    a.update(over)
    return edges(c["kind"], g["Twc"] if Twc is None else Twc, g["Xs"], g["Cs"], g["K"], ie, je, g["idx_ii2jj"], g["valid_match"],
                 g["Q"], **a)
