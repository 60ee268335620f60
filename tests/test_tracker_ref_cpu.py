"""CPU tests (-m "not gpu") of tests/tracker_ref.py, the float64 reference that tests/test_tracker_step_gpu.py holds
mslam_track_pose to: the golden normal equations built from the reference's own geometry.py, finite differences of the
cost, the Sim3 logarithm, the properties the GPU tests assume of their input sets, and the float32 baselines."""
import os

import numpy as np
import pytest
import scipy.linalg

import oracle
import tracker_ref as R
from mast3r_slam import synthetic
from oracle import tracker_py


@pytest.fixture(scope="module")
def case_set():
    return R.cases()


@pytest.fixture(scope="module")
def refs(case_set):
    return {k: R.reference(c) for k, c in case_set.items()}


# ---- golden -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rays", "calib"])
def test_step_matches_reference_formulae(kind, golden_dir):
    """H and g of step() against tests/golden/tracker_formulae.npz (the reference's geometry.py composed as
    tracker.py:208-318, float64), the inputs rebuilt as make_golden.py::section_tracker builds them and mapped to
    tracker roles: Xk := Xs[0][idx], Xf := Xs[1], identity idx, T := Twc[1], the confidence gates folded into `valid`,
    the gathered pixel grid as the calibrated measurement.  The golden stores the edge kernel's g = A^T b, the negative
    of the tracker's.  Both sides are float64 evaluations of the same formulae in a different order of operations.
    Observed: max|dH| / max|H| = 2.3e-15 (rays), 1.8e-16 (calib); max|dg| / max|g| = 5.1e-16 (rays), 7.9e-16 (calib);
    asserted at 1e-13, room for another BLAS's summation order and nothing else."""
    fx = np.load(os.path.join(golden_dir, "tracker_formulae.npz"))
    h, w = 12, 16
    g = synthetic.make_graph(n_kf=2, h=h, w=w, seed=0, pose_noise=0.02, extra_edges=0)
    idx = g["idx_ii2jj"][0]
    Q = g["Q"][0].astype(np.float64)[:, 0]
    Cs = g["Cs"].astype(np.float64)
    K = g["K"].astype(np.float64)
    Xs = g["Xs"].astype(np.float64)
    uv = None
    if kind == "calib":      # constrain_points_to_ray (global_opt.py:180-182) in float64, as the golden's script does
        grid = np.stack(np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64), indexing="xy"), -1)
        grid = grid.reshape(-1, 2)
        z = Xs[:, :, 2:3]
        Xs = np.concatenate([(grid[None, :, 0:1] - K[0, 2]) / K[0, 0] * z, (grid[None, :, 1:2] - K[1, 2]) / K[1, 1] * z, z], -1)
        np.testing.assert_array_equal(Xs.astype(np.float32), fx["Xs_calib"])
        uv = grid[idx]
    valid = g["valid_match"][0][:, 0] & (Q > 1.5) & (Cs[0][idx][:, 0] > 0.0) & (Cs[1][:, 0] > 0.0)
    Tj = fx["Twc"][1].astype(np.float64)
    M = np.eye(4)            # the golden's pose acts as s (X + w uv + q x uv) + t with the float32 quaternion as stored
    M[:3, :3] = Tj[7] * synthetic.quat_rotate(Tj[3:7], np.eye(3)).T
    M[:3, 3] = Tj[:3]
    sa, sb = R.SIGMAS[kind]
    ref = R.step(kind == "calib", M, Xs[1], Xs[0][idx], np.arange(h * w), Q, valid, sa, sb, 1.345, K=K, hw=(h, w),
                 pixel_border=-10, z_eps=1e-6, uv=uv)
    H_ref, g_ref = fx[f"H_{kind}"], fx[f"g_{kind}"]
    eH = np.abs(ref["H"] - H_ref).max() / np.abs(H_ref).max()
    eg = np.abs(-ref["g"] - g_ref).max() / np.abs(g_ref).max()
    print(f"golden {kind}: dH {eH:.2e} dg {eg:.2e}")
    assert eH < 1e-13 and eg < 1e-13


# ---- finite differences ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rays-257", "calib-17x31", "gates"])
def test_gradient_is_the_finite_difference_of_the_cost(case_set, name):
    """huber = inf: cost(exp(eps e_i) T) is smooth, and g = -d cost / d eps_i.  Central differences with eps = 1e-5:
    truncation ~ eps^2 |cost'''| / 6, rounding ~ 1e-16 cost / eps; asserted at 1e-6 of gabs (observed <= 6e-8).
    Both sigmas are 1 here: at the production values the unit-ray rows weigh 1e7 times the distance rows, and the
    rounding of the cost would drown the scale component of the gradient, which only the distance rows feed.
    The gated case keeps its gates fixed: no point is within the margins of a gate, so none flips within eps."""
    c = dict(case_set[name], huber=np.inf, sigma_a=1.0, sigma_b=1.0)
    ref = R.reference(c)
    M0 = R.sim3_matrix(c["T0"])
    eps = 1e-5
    fd = np.zeros(7)
    for i in range(7):
        cost = [R.reference(c, scipy.linalg.expm(R.sim3_generator(s * eps * np.eye(7)[i])) @ M0)["cost"] for s in (1, -1)]
        fd[i] = (cost[0] - cost[1]) / (2 * eps)
    err = np.abs(ref["g"] + fd) / ref["gabs"]
    print(f"fd {name}: {err.max():.2e}")
    assert err.max() < 1e-6


def test_huber_weights_and_abs_sums(refs):
    """cost = 1/2 sum rho'-weighted squares: with every row's weight written out by hand (1 inside k, k / |r| outside) the
    cost equals sum over rows of 1/2 r^2 (inliers) or 1/2 k |r| (outliers); Habs / gabs dominate |H| / |g|."""
    for name, ref in refs.items():
        wr = np.abs(ref["whitened"][ref["rows"]])
        want = 0.5 * np.where(wr < R.HUBER, wr ** 2, R.HUBER * wr).sum()
        assert abs(ref["cost"] - want) <= 1e-12 * want, name
        assert (np.abs(ref["H"]) <= ref["Habs"] * (1 + 1e-12)).all() and (np.abs(ref["g"]) <= ref["gabs"] * (1 + 1e-12)).all()
        np.testing.assert_allclose(ref["H"] @ ref["tau"], ref["g"], atol=1e-9 * ref["gabs"].max())


# ---- Sim3 logarithm ---------------------------------------------------------------------------------------------------
def test_sim3_log_inverts_exp():
    rng = np.random.default_rng(0)
    for _ in range(20):
        T0 = R.sim3_exp(rng.normal(0, 0.4, 7))
        xi = rng.normal(0, 0.3, 7)
        np.testing.assert_allclose(R.sim3_log(R.sim3_retr(xi, T0), T0), xi, atol=1e-13)
    np.testing.assert_allclose(R.sim3_log(T0, T0), 0, atol=1e-14)
    # the float64 exponential agrees with the oracle's closed form (float32)
    xi = rng.normal(0, 0.3, 7)
    np.testing.assert_allclose(R.sim3_matrix(oracle.sim3_exp(xi)[0]), R.sim3_matrix(R.sim3_exp(xi)), atol=2e-6)


def test_sim3_log_round_trip_through_float32(case_set):
    """|sim3_log(retr_f32(tau, T0), T0)| against |tau| with the oracle's float32 retraction, steps of 0.003 to 2 in random
    directions from the poses of the input sets: within roundtrip_tol(), the tolerance the GPU test holds the kernel's
    last_delta_norm to.  Observed: up to 1.1e-4 at |tau| = 0.03 with sigma = 3.5e-6 (tolerance 4.2e-4: the float32
    (e^sigma - 1) / sigma), below 3e-7 wherever |sigma| > 1e-3."""
    rng = np.random.default_rng(1)
    T0s = [c["T0"] for c in case_set.values()]
    worst = 0.0
    for i in range(700):
        xi = rng.normal(size=7)
        xi = (xi / np.linalg.norm(xi) * (0.003, 0.01, 0.03, 0.1, 0.3, 1.0, 2.0)[i % 7]).astype(np.float32)
        tau = R.sim3_log(oracle.sim3_retr(xi, T0s[i % len(T0s)])[0], T0s[i % len(T0s)])
        err = abs(np.linalg.norm(tau) - np.linalg.norm(xi.astype(np.float64)))
        worst = max(worst, err / R.roundtrip_tol(tau))
        assert err <= R.roundtrip_tol(tau), (xi, err)
    print(f"round trip: worst error / tolerance {worst:.2f}")


# ---- what the GPU tests assume of their inputs -------------------------------------------------------------------------
def test_inputs_are_what_the_gpu_tests_assume(case_set, refs):
    for name, c in case_set.items():
        ref = refs[name]
        assert len(np.unique(c["idx"])) < c["n"] or c["n"] < 4, name                  # collisions
        rot = 2 * np.arccos(min(1.0, abs(float(c["T0"][6]))))
        assert 0.1 < rot < 0.4 and abs(c["T0"][7] - 1) > 0.05 and np.linalg.norm(c["T0"][:3]) > 0.1, name
        assert ref["tau"] is not None and np.linalg.norm(ref["tau"]) < 3.0, name
        if c["kind"] == "rays":      # typical unit-ray residual of a few percent: sigma_a * whitened / sqrt(Q)
            e = np.abs(ref["whitened"][:, :3] * c["sigma_a"] / np.sqrt(c["Qk"].astype(np.float64))[:, None])[ref["rows"][:, 0]]
            assert np.median(e) > 0.01, (name, np.median(e))
    for key in R.MASK_HUBER:
        c, ref = case_set["huber-" + key], refs["huber-" + key]
        assert 0.4 < c["valid"].mean() < 0.6
        assert 0.2 <= R.outlier_fraction(ref) <= 0.8, (key, R.outlier_fraction(ref))
    R.check_gates(case_set["gates"], refs["gates"])


def test_reference_trajectory_descends(case_set):
    """Float64 GN steps from T0 on the inputs of the GPU trajectory test: the cost falls over the four poses that test
    evaluates (undamped GN with Huber weights promises no descent in general; on these inputs it holds with a gap
    of more than 1e-3 of the cost, far above what a float32 step changes)."""
    for name in ("rays-2049", "calib-17x31"):
        c = case_set[name]
        T, costs = c["T0"].astype(np.float64), []
        for _ in range(4):
            ref = R.reference(c, T)
            costs.append(ref["cost"])
            T = R.sim3_retr(ref["tau"], T)
        assert all(b < a * (1 - 1e-3) for a, b in zip(costs, costs[1:])), (name, costs)


# ---- float32 baselines ------------------------------------------------------------------------------------------------
def fp32_step(c):
    """One iteration of oracle/tracker_py.py::track (float32) from T0 -> (T1, tau f32, cost)."""
    cfg = dict(sigma_ray=c["sigma_a"], sigma_dist=c["sigma_b"], sigma_pixel=c["sigma_a"], sigma_depth=c["sigma_b"],
               huber=c["huber"], pixel_border=c["pixel_border"], depth_eps=c["z_eps"], max_iters=1, rel_error=0.0,
               delta_norm=0.0)
    ident = np.array([0, 0, 0, 0, 0, 0, 1, 1], np.float32)
    trace = []
    _, T1, it = tracker_py.track(bool(c["use_calib"]), c["Xf"][c["idx"]], c["Xk"], c["T0"], ident, c["Qk"], c["valid"], cfg,
                                 K=c["K"], img_size=(c["h"], c["w"]), trace=trace)
    assert it == 1 and len(trace) == 1
    return T1, trace[0][0], trace[0][1]


def test_fp32_baselines(case_set, refs):
    """The float32 oracle's single step against the float64 reference, with the two measures the GPU test asserts;
    the maxima are the constants in tests/tracker_ref.py."""
    worst = dict(backward=0.0, cost=0.0)
    for name, c in case_set.items():
        ref = refs[name]
        T1, tau32, cost32 = fp32_step(c)
        tau = R.sim3_log(T1, c["T0"])
        m = dict(backward=R.backward_error(ref, tau), cost=abs(cost32 - ref["cost"]) / ref["cost"])
        print(f"fp32 {name:24s} backward {m['backward']:.2e} cost {m['cost']:.2e}")
        assert abs(np.linalg.norm(tau) - np.linalg.norm(tau32.astype(np.float64))) <= R.roundtrip_tol(tau), name
        worst = {k: max(worst[k], m[k]) for k in worst}
    print("fp32 baselines:", {k: f"{v:.3e}" for k, v in worst.items()})
    # the constants are this measurement; another BLAS sums the float32 A^T A in another order, so a fresh one may differ
    # a little - a constant that is off by more is stale
    assert 0.5 * R.FP32_BACKWARD_BASELINE < worst["backward"] < 1.5 * R.FP32_BACKWARD_BASELINE
    assert 0.5 * R.FP32_COST_BASELINE < worst["cost"] < 1.5 * R.FP32_COST_BASELINE
