"""Plain float64 reference of ONE Gauss-Newton step of the frame-to-keyframe Sim3 tracker (csrc/tracker.hip,
mslam_track_pose), the Sim3 logarithm that turns the pose the kernel produced back into its step, and the input sets of
tests/test_tracker_step_gpu.py.  The step is written in the reference's form - explicit (n,4,7) / (n,3,7) Jacobians
d(ray, dist)/dP or d(u, v, log z)/dP times dP/dxi = [I, -[P]x, P], A = robust J, H = A^T A - and never in the kernel's
expanded rows.  numpy / scipy only; nothing here touches the device.  Pinned on its own in tests/test_tracker_ref_cpu.py
(golden normal equations, finite differences of the cost, float32 baselines)."""
import numpy as np

# the float64 Sim3 group has one statement, tests/sim3_ref.py; this module's users keep finding it here
from sim3_ref import sim3_exp, sim3_from_matrix, sim3_generator, sim3_log, sim3_matrix, sim3_retr  # noqa: F401

CHUNK = 65536

# Production values (config["tracking"])
HUBER = 1.345
SIGMAS = {"rays": (0.003, 10.0), "calib": (1.0, 10.0)}

# float32 baselines: oracle/tracker_py.py (the float32 numpy restatement of the reference's step: act_sim3_jac,
# ray_dist / project_calib, solve, then oracle.sim3_retr) run for one iteration on every input set of cases() - all of
# them but the one above the block cap, whose (n,4,7) float32 Jacobians do not fit -, the pose it returns turned into a
# step by sim3_log and measured against step() in float64 with backward_error() and the relative error of the cost.
# Each constant is the maximum over those input sets as tests/test_tracker_ref_cpu.py::test_fp32_baselines prints it
# (2.192e-04 at rays-65, 1.607e-07 at huber-rays-production), rounded up to two digits; that test fails when a fresh
# measurement is not within half to one and a half times them.  They are a property of float32 arithmetic on these inputs, not of the
# kernel.  The backward baseline comes from the scale row of the unit-ray systems: (I - r r^T) / d times dP/dsigma = P
# is zero in exact arithmetic, in float32 it leaves ~1e-7 that the unit-ray weights (1 / 0.003^2) lift against a row fed
# by distance rows of weight 1 / 10^2 alone (the other rows of that system stay below 1e-6).  The calibrated systems
# reach 2.5e-5.
FP32_BACKWARD_BASELINE = 2.2e-4
FP32_COST_BASELINE = 1.7e-7


def roundtrip_tol(tau):
    """How closely |sim3_log(T1, T0)| returns |tau| after T1 = exp(tau) T0 went through float32 (exp, composition, eight
    rounded floats): 5e-7 max(1, |tau|) for the roundings, plus 2^-23 |tau_t| / |sigma|: the float32 exponential scales
    the translation by C = (e^sigma - 1) / sigma with e^sigma rounded near 1 (the reference's formula, sim3.h and the
    oracle alike), which loses C to 2^-24 / |sigma| for 1e-6 <= |sigma| << 1.  Checked on the CPU against the oracle's
    retraction over steps of 0.003 to 2 (tests/test_tracker_ref_cpu.py::test_sim3_log_round_trip_through_float32)."""
    tau = np.asarray(tau, np.float64)
    sigma = max(abs(tau[6]), 1e-6)
    return 5e-7 * max(1.0, np.linalg.norm(tau)) + 2.0 ** -23 * np.linalg.norm(tau[:3]) / sigma


# ---- one GN step --------------------------------------------------------------------------------------------------------
def _skew(P):
    o = np.zeros(P.shape[0])
    return np.stack([o, -P[:, 2], P[:, 1], P[:, 2], o, -P[:, 0], -P[:, 1], P[:, 0], o], -1).reshape(-1, 3, 3)


def _huber(r, k):
    a = np.abs(r)
    with np.errstate(divide="ignore"):
        return np.where(a < k, 1.0, k / a)


def _ray_dist(X, jac=False):
    d = np.linalg.norm(X, axis=-1, keepdims=True)
    r = X / d
    rd = np.concatenate([r, d], -1)
    if not jac:
        return rd
    dr = (np.eye(3) - r[:, :, None] * r[:, None, :]) / d[:, :, None]
    return rd, np.concatenate([dr, r[:, None, :]], 1)            # (n,4,3)


def step(use_calib, T, Xf, Xk, idx, Qk, valid, sigma_a, sigma_b, huber, K=None, hw=None, pixel_border=0, z_eps=0.0,
         uv=None):
    """One step at pose T (relative pose keyframe <- frame; [t, q, s] or the 4x4 similarity itself): residual r = z - h(T Xf[idx]) of every keyframe pixel,
    J = dr/dxi for the left perturbation exp(xi) T, sqrt_info = valid sqrt(Qk) / sigma (times the gates, calibrated),
    robust = sqrt_info sqrt(huber(sqrt_info r)), A = robust J, b = robust r.  Returns a dict with
      H = A^T A, g = -A^T b (H tau = g), cost = 1/2 b^T b, tau = solve(H, g) (None when H is singular),
      Habs = |A|^T |A|, gabs = |A|^T |b|: the same sums with every term in absolute value,
      whitened = sqrt_info r (n, 4 | 3), rows = the rows that take part (sqrt_info > 0),
      valid_meas, valid_z, in_border (calibrated): the three gates of every point, before `valid`."""
    f8 = lambda a: np.asarray(a, np.float64)
    T, Xf, Xk, Qk = f8(T), f8(Xf).reshape(-1, 3), f8(Xk).reshape(-1, 3), f8(Qk).reshape(-1)
    idx, valid = np.asarray(idx, np.int64).reshape(-1), np.asarray(valid).reshape(-1) != 0
    n = Xk.shape[0]
    M = T if T.ndim == 2 else sim3_matrix(T)
    nr = 3 if use_calib else 4
    if use_calib:
        K = f8(K)
        h, w = hw
        if uv is None:
            k = np.arange(n)
            uv = np.stack([k % w, k // w], -1)
        uv = f8(uv)
    out = dict(H=np.zeros((7, 7)), g=np.zeros(7), cost=0.0, Habs=np.zeros((7, 7)), gabs=np.zeros(7))
    diag = dict(whitened=[], rows=[])
    if use_calib:
        diag.update(valid_meas=[], valid_z=[], in_border=[])
    for c0 in range(0, n, CHUNK):
        sl = slice(c0, min(n, c0 + CHUNK))
        P = Xf[idx[sl]] @ M[:3, :3].T + M[:3, 3]
        m = P.shape[0]
        dP = np.concatenate([np.broadcast_to(np.eye(3), (m, 3, 3)), -_skew(P), P[:, :, None]], -1)       # (m,3,7)
        sq = valid[sl] * np.sqrt(Qk[sl])
        if not use_calib:
            rd_f, drd = _ray_dist(P, jac=True)
            r = _ray_dist(Xk[sl]) - rd_f
            J = -(drd @ dP)                                                                                  # (m,4,7)
        else:
            z = P[:, 2]
            valid_z = z > z_eps
            zs = np.where(z != 0, z, 1.0)                      # a gated point takes no part: keep its row finite
            u = K[0, 0] * P[:, 0] / zs + K[0, 2]
            v = K[1, 1] * P[:, 1] / zs + K[1, 2]
            in_border = (u > pixel_border) & (u < w - 1 - pixel_border) & (v > pixel_border) & (v < h - 1 - pixel_border)
            zk = Xk[sl, 2]
            valid_meas = zk > z_eps
            meas = np.stack([uv[sl, 0], uv[sl, 1], np.log(np.where(valid_meas, zk, 1.0))], -1)
            r = meas - np.stack([u, v, np.log(np.where(valid_z, z, 1.0))], -1)
            dpz = np.zeros((m, 3, 3))
            dpz[:, 0, 0] = K[0, 0] / zs
            dpz[:, 1, 1] = K[1, 1] / zs
            dpz[:, 0, 2] = -K[0, 0] * P[:, 0] / zs ** 2
            dpz[:, 1, 2] = -K[1, 1] * P[:, 1] / zs ** 2
            dpz[:, 2, 2] = 1.0 / zs
            J = -(dpz @ dP)                                                                                  # (m,3,7)
            sq = sq * (valid_z & in_border & valid_meas)
            diag["valid_meas"].append(valid_meas); diag["valid_z"].append(valid_z); diag["in_border"].append(in_border)
        sqrt_info = np.concatenate([np.repeat(sq[:, None] / sigma_a, nr - 1, 1), sq[:, None] / sigma_b], 1)
        whitened = sqrt_info * r
        robust = sqrt_info * np.sqrt(_huber(whitened, huber))
        A = (robust[:, :, None] * J).reshape(-1, 7)
        b = (robust * r).reshape(-1)
        out["H"] += A.T @ A
        out["g"] -= A.T @ b
        out["cost"] += 0.5 * float(b @ b)
        out["Habs"] += np.abs(A).T @ np.abs(A)
        out["gabs"] += np.abs(A).T @ np.abs(b)
        diag["whitened"].append(whitened); diag["rows"].append(sqrt_info > 0)
    out.update({k: np.concatenate(v) for k, v in diag.items()})
    try:
        out["tau"] = np.linalg.solve(out["H"], out["g"]) if np.linalg.matrix_rank(out["H"]) == 7 else None
    except np.linalg.LinAlgError:
        out["tau"] = None
    return out


def backward_error(ref, tau):
    """max_i |(H tau - g)_i| / (sum_j Habs_ij |tau_j| + gabs_i): how far `tau` is from solving the reference's normal
    equations, in units of the sums' own magnitude - independent of the conditioning of H."""
    tau = np.asarray(tau, np.float64)
    return float(np.max(np.abs(ref["H"] @ tau - ref["g"]) / (ref["Habs"] @ np.abs(tau) + ref["gabs"])))


def outlier_fraction(ref, k=HUBER):
    """Fraction of the participating rows whose whitened residual lies in Huber's outlier branch."""
    rows = ref["rows"]
    return float((np.abs(ref["whitened"][rows]) >= k).mean())


# ---- input sets ---------------------------------------------------------------------------------------------------------
RAY_SIZES = (5, 63, 64, 65, 257, 2047, 2048, 2049, 4097)
RAY_LARGE = 1024 * 2048 + 1025          # above the 1024-block cap: the grid-stride loop's ninth trip
CALIB_SIZES = ((7, 9), (17, 31), (64, 32), (45, 46))
BORDER_MARGIN, Z_MARGIN = 1e-3, 1e-4    # no point this close to a gate: float32 and float64 agree on every gate


def _intrinsics(h, w):
    return np.array([[0.9 * w, 0, 0.5 * (w - 1) + 0.3], [0, 0.95 * w, 0.5 * (h - 1) - 0.2], [0, 0, 1]], np.float32)


def make_case(kind, size, seed=0, sigmas=None, valid_frac=0.9, pose_err=0.1, noise=0.05, pixel_border=-10, z_eps=1e-6,
              gates=False):
    """One input set, float32 as the kernel reads it.  kind "rays": size = n, "calib": size = (h, w).
    T_true has a rotation of about 0.2 rad, scale 1.15 and a translation; T0 = exp(pose_err * d) T_true.  idx is random
    with collisions.  rays: Xk = T_true Xf[idx] + noise * |.| * N(0, 1).  calib: every frame point is built for ONE of the
    keyframe pixels that index it (pixel + noise px, depth z), so the other pixels that collide on it see a residual of
    many pixels; keyframe depths are the true ones times exp(noise N(0, 1)).  gates=True (calib): a tenth of the keyframe
    depths at or below z_eps, a tenth of the frame points behind the camera, frame points spread over a window wider
    than the image.  Points within BORDER_MARGIN px of a border or Z_MARGIN of z_eps (at T0, float64) are re-drawn."""
    calib = kind == "calib"
    h, w = size if calib else (0, 0)
    n = h * w if calib else int(size)
    rng = np.random.default_rng([seed, n, int(calib), int(gates)])
    sa, sb = sigmas if sigmas is not None else SIGMAS[kind]
    T_true = sim3_exp(np.array([0.25, -0.15, 0.2, 0.12, -0.1, 0.13, np.log(1.15)]))
    d = rng.normal(size=7)
    T0 = sim3_retr(pose_err * d / np.linalg.norm(d), T_true).astype(np.float32)
    Mt, Mi = sim3_matrix(T_true), np.linalg.inv(sim3_matrix(T_true))
    idx = rng.integers(0, n, n)
    Qk = rng.uniform(1.0, 4.0, n).astype(np.float32)
    valid = rng.uniform(size=n) < valid_frac
    case = dict(kind=kind, use_calib=int(calib), n=n, h=h, w=w, T0=T0, idx=idx.astype(np.int64), Qk=Qk, valid=valid,
                sigma_a=sa, sigma_b=sb, huber=HUBER, pixel_border=pixel_border, z_eps=z_eps, K=None)
    if not calib:
        dirs = rng.normal(size=(n, 3)) * [0.5, 0.5, 0.2] + [0, 0, 1]
        Xf = dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * rng.uniform(1.0, 5.0, (n, 1))
        Pk = Xf[idx] @ Mt[:3, :3].T + Mt[:3, 3]
        Xk = Pk + noise * np.linalg.norm(Pk, axis=1, keepdims=True) * rng.normal(size=(n, 3))
        case.update(Xf=Xf.astype(np.float32), Xk=Xk.astype(np.float32))
        return case
    K = _intrinsics(h, w)
    case["K"] = K
    owner = np.arange(n)                       # the keyframe pixel each frame point is built for
    owner[idx] = np.arange(n)
    spread = 0.12 * np.array([w, h]) if gates else 0.0     # std of the extra pixel scatter, per axis

    def draw(sel):
        m = len(sel)
        px = np.stack([owner[sel] % w, owner[sel] // w], -1) + rng.normal(size=(m, 2)) * (1.0 + spread)
        z = rng.uniform(1.0, 5.0, m)
        if gates:
            z = np.where(rng.uniform(size=m) < 0.1, -z, z)
        Pt = np.stack([(px[:, 0] - K[0, 2]) / K[0, 0] * z, (px[:, 1] - K[1, 2]) / K[1, 1] * z, z], -1)
        return (Pt @ Mi[:3, :3].T + Mi[:3, 3]).astype(np.float32)

    Xf = draw(np.arange(n))
    zk = np.empty(n)

    def draw_k(sel):
        z = np.abs((Xf[idx[sel]].astype(np.float64) @ Mt[:3, :3].T + Mt[:3, 3])[:, 2]) * np.exp(noise * rng.normal(size=len(sel)))
        if gates:
            z = np.where(rng.uniform(size=len(sel)) < 0.1, rng.uniform(-0.05, z_eps - 2 * Z_MARGIN, len(sel)), z)
        return z

    zk[:] = draw_k(np.arange(n))
    for _ in range(100):
        Xk = np.stack([np.zeros(n), np.zeros(n), zk], -1).astype(np.float32)
        M0 = sim3_matrix(T0)
        P = Xf.astype(np.float64) @ M0[:3, :3].T + M0[:3, 3]
        zs = np.where(np.abs(P[:, 2]) > 0, P[:, 2], 1.0)
        u, v = K[0, 0] * P[:, 0] / zs + K[0, 2], K[1, 1] * P[:, 1] / zs + K[1, 2]
        near = np.abs(P[:, 2] - z_eps) < Z_MARGIN
        for x, hi in ((u, w - 1 - pixel_border), (v, h - 1 - pixel_border)):
            near |= (np.abs(x - pixel_border) < BORDER_MARGIN) | (np.abs(x - hi) < BORDER_MARGIN)
        near_k = np.abs(Xk[:, 2].astype(np.float64) - z_eps) < Z_MARGIN
        if not near.any() and not near_k.any():
            break
        if near.any():
            Xf[near] = draw(np.flatnonzero(near))
        if near_k.any():
            zk[near_k] = draw_k(np.flatnonzero(near_k))
    else:
        raise AssertionError("make_case: could not move every point off the gates")
    case.update(Xf=Xf, Xk=Xk)
    return case


def reference(case, T=None):
    """step() of an input set at T (default: its T0), the float32 inputs cast to float64."""
    c = case
    return step(c["use_calib"], c["T0"] if T is None else T, c["Xf"], c["Xk"], c["idx"], c["Qk"], c["valid"], c["sigma_a"],
                c["sigma_b"], c["huber"], K=c["K"], hw=(c["h"], c["w"]), pixel_border=c["pixel_border"], z_eps=c["z_eps"])


def check_gates(c, ref):
    """Each gate alone removes >= 5 % of the points, >= 30 % survive all three, none sits on a gate."""
    vm, vz, ib = ref["valid_meas"], ref["valid_z"], ref["in_border"]
    assert (~vm).mean() >= 0.05 and (~vz).mean() >= 0.05 and (~ib).mean() >= 0.05, ((~vm).mean(), (~vz).mean(), (~ib).mean())
    assert (vm & vz & ib).mean() >= 0.30
    assert (c["Xk"][:, 2] <= c["z_eps"]).any()
    M = sim3_matrix(c["T0"])
    P = c["Xf"][c["idx"]].astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    assert (P[:, 2] < 0).mean() >= 0.05
    K, b = c["K"].astype(np.float64), c["pixel_border"]
    u, v = K[0, 0] * P[:, 0] / P[:, 2] + K[0, 2], K[1, 1] * P[:, 1] / P[:, 2] + K[1, 2]
    for x, hi in ((u, c["w"] - 1 - b), (v, c["h"] - 1 - b)):
        assert np.minimum(np.abs(x - b), np.abs(x - hi)).min() >= BORDER_MARGIN
    assert np.abs(P[:, 2] - c["z_eps"]).min() >= Z_MARGIN
    assert np.abs(c["Xk"][:, 2].astype(np.float64) - c["z_eps"]).min() >= Z_MARGIN


MASK_HUBER = {
    # name: (kind, size, make_case arguments).  Noise is tuned per sigma so that 20-80 % of the valid rows are outliers.
    "rays-production": ("rays", 4097, dict(valid_frac=0.5)),
    "rays-unit": ("rays", 4097, dict(valid_frac=0.5, sigmas=(1.0, 1.0), noise=0.8)),
    "calib-production": ("calib", (45, 46), dict(valid_frac=0.5)),
    "calib-unit": ("calib", (45, 46), dict(valid_frac=0.5, sigmas=(1.0, 1.0), noise=0.8)),
}
GATES = ("calib", (64, 32), dict(gates=True, pixel_border=2, z_eps=0.05))


def cases(large=False):
    """{name: input set} of every single-step test of tests/test_tracker_step_gpu.py (the loop tests reuse rays-2049 and
    calib-17x31); large=True adds the one above the block cap."""
    out = {f"rays-{n}": make_case("rays", n) for n in RAY_SIZES}
    out.update({f"calib-{h}x{w}": make_case("calib", (h, w)) for h, w in CALIB_SIZES})
    out.update({f"huber-{k}": make_case(kind, size, **kw) for k, (kind, size, kw) in MASK_HUBER.items()})
    out["gates"] = make_case(GATES[0], GATES[1], **GATES[2])
    if large:
        out["rays-large"] = make_case("rays", RAY_LARGE)
    return out
