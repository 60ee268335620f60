"""CPU tests (-m "not gpu") of tests/sim3_ref.py, the float64 Sim3 group, float32 restatement and tolerances that
tests/test_sim3_edges_gpu.py holds mslam_sim3_op, mslam_sim3_act and lietorch_hip.Sim3 to: the float64 group against
itself (two independent exponentials, the logarithm, the group laws), the float32 restatement and the C oracle against
the exponential's row-wise tolerance, the baseline constants against a fresh measurement, and the parts of the Sim3
class that need no device."""
import numpy as np
import pytest
import torch

import oracle
import sim3_ref as S


@pytest.fixture(scope="module")
def grid():
    xi, theta, sigma = S.exp_grid()
    M64 = S.exp_m(xi)
    return dict(xi=xi, theta=theta, sigma=sigma, M64=M64, tol=S.exp_trans_tol(xi, M64), cap=S.exp_cap(xi))


def _rel(M, M_ref):
    """Largest difference of two similarities: rotation entries, scale (relative), translation over the larger of
    1 and |t|."""
    s, R, t = S.split(M)
    s0, R0, t0 = S.split(M_ref)
    tn = np.maximum(1.0, np.linalg.norm(t0, axis=1))
    return max(np.abs(R - R0).max(), np.abs(s / s0 - 1).max(), (np.abs(t - t0).max(1) / tn).max())


# ---- float64 ----------------------------------------------------------------------------------------------------------
def test_exp_expm_matches_closed_form(grid):
    """scipy's expm of the generator against the closed form (expm1 of sigma + i theta) on the whole grid: rotation
    entries, relative scale, translation over |tau| max(1, e^sigma), all <= 1e-12.  Both are float64 and independent;
    observed 7e-14, 6e-14, 2e-14."""
    xi = grid["xi"]
    s, R, t = S.split(grid["M64"])
    sc, Rc, tc = S.split(S.exp_closed_m(xi))
    worst = (np.abs(R - Rc).max(), np.abs(s / sc - 1).max(), S.scaled(np.abs(t - tc).max(1), S.size_exp(xi)).max())
    print("expm vs closed form: rot %.1e scale %.1e trans %.1e" % worst)
    assert max(worst) <= 1e-12
    assert grid["xi"].shape[0] == 8 * len(S.THETAS) * len(S.SIGMAS)


def test_log_of_exp_is_identity():
    """sim3_log(sim3_exp(xi), identity) = xi to 1e-12 |xi| for rotations below pi, from 1e-6 to 3 rad and scales e^-1 to
    e^1 (the principal logarithm is the inverse only there)."""
    rng = np.random.default_rng(5)
    I = np.array([0, 0, 0, 0, 0, 0, 1, 1.0])
    for theta in (0.0, 1e-6, 1e-3, 0.3, 3.0):
        for sigma in (0.0, 1e-6, -0.3, 1.0):
            ax = rng.normal(size=3)
            xi = np.concatenate([rng.normal(size=3), theta * ax / np.linalg.norm(ax), [sigma]])
            back = S.sim3_log(S.sim3_exp(xi), I)
            assert np.abs(back - xi).max() <= 1e-12 * max(1.0, np.linalg.norm(xi)), (theta, sigma)


def test_group_laws():
    """inv, mul and act in float64 on the pose inputs of the GPU tests (scales 1e-3..1e3, |t| to 1e3), to 1e-12 in
    _rel's measure: A^-1 A = I, (A B)^-1 = B^-1 A^-1, (A B) C = A (B C), (A B)(X) = A(B(X)), A^-1(A(X)) = X, and
    exp(xi) exp(-xi) = I, exp(0) = I.  Translations of a product are compared over its natural size."""
    A, B, C, X = S.poses(200, 1), S.poses(200, 2), S.poses(200, 5), S.points(200, 4)
    MA, MB, MC = S.matrices(A), S.matrices(B), S.matrices(C)
    I = np.broadcast_to(np.eye(4), MA.shape)

    def close(M, M0, size):
        s, R, t = S.split(M)
        s0, R0, t0 = S.split(M0)
        e = max(np.abs(R - R0).max(), np.abs(s / s0 - 1).max(), S.scaled(np.abs(t - t0).max(1), size).max())
        assert e <= 1e-12, e

    close(S.inv_m(A) @ MA, I, 2 * S.size_inv(A))
    close(np.linalg.inv(S.mul_m(A, B)), S.inv_m(B) @ S.inv_m(A), S.size_mul(S.inv_m(B), S.inv_m(A)))
    sAB = S.size_mul(A, B)
    close(S.mul_m(A, B) @ MC, MA @ (MB @ MC), S.split(MA @ MB)[0] * np.linalg.norm(C[:, :3], axis=1) + sAB)
    Y = S.act(A, X)
    assert S.scaled(np.abs(np.einsum("nij,nj->ni", (MA @ MB)[:, :3, :3], X) + (MA @ MB)[:, :3, 3]
                           - S.act(A, S.act(B, X))).max(1),
                    S.split(MA @ MB)[0] * np.linalg.norm(X, axis=1) + sAB).max() <= 1e-12
    Mi = S.inv_m(A)
    back = np.einsum("nij,nj->ni", Mi[:, :3, :3], Y) + Mi[:, :3, 3]
    assert S.scaled(np.abs(back - X).max(1), np.linalg.norm(X, axis=1) + 2 * S.size_inv(A)).max() <= 1e-12
    xi = S.steps(50, 3)
    close(S.exp_m(xi) @ S.exp_m(-xi), I[:50], 2 * S.size_exp(xi) * np.maximum(1.0, np.exp(-xi[:, 6].astype(np.float64))))
    assert np.array_equal(S.exp_m(np.zeros((1, 7)))[0], np.eye(4))
    # the single-pose functions tests/tracker_ref.py re-exports agree with the batched ones
    assert np.abs(S.sim3_matrix(A[3]) - MA[3]).max() == 0.0
    assert _rel(S.sim3_matrix(S.sim3_retr(xi[7], B[7]))[None], S.retr_m(xi[7:8], B[7:8])) <= 1e-12


# ---- the float32 exponential ------------------------------------------------------------------------------------------
def test_restatement_matches_oracle_exp(grid):
    """exp32 with no nudge against oracle.sim3_exp (neither normalises): bit for bit on every row that takes C, A and B
    as constants (|sigma| < 1e-6 and theta < 1e-6: 8 rows in each of 3 x 2 cells); on every other row, where a host
    sinf / cosf / expf may differ from the correctly rounded one by an ulp, translation within the row's tolerance and
    rotation and scale within the baselines."""
    xi = grid["xi"]
    mine, theirs = S.exp32(xi, unit=False), oracle.sim3_exp(xi)
    s_small, t_small = S.exp_branches(xi)
    const = s_small & t_small
    assert const.sum() == 8 * 3 * 2
    assert np.array_equal(mine[const].view(np.int32), theirs[const].view(np.int32))
    print("rows equal bit for bit: %d of %d" % ((mine.view(np.int32) == theirs.view(np.int32)).all(1).sum(), len(xi)))
    t64 = grid["M64"][:, :3, 3]
    for T in (mine, theirs):
        assert (np.abs(T[:, :3] - t64).max(1) <= grid["tol"]).all()
    d = S.pose_errors(mine, S.matrices(theirs))
    assert d["rot"].max() <= S.BASELINES["exp"]["rot"] and d["scale"].max() <= S.BASELINES["exp"]["scale"]


def test_oracle_inside_row_tolerance(grid):
    """The C oracle's exponential against exp_trans_tol on every grid row, nothing left out; and the tolerance is not
    empty: at least a third of the rows are held to 64 ulps of |tau| max(1, e^sigma), among them every row of the
    well-conditioned cells (sigma = 0 or |sigma| >= 0.3, theta = 0 or theta >= 0.3)."""
    xi, tol, cap = grid["xi"], grid["tol"], grid["cap"]
    err = np.abs(oracle.sim3_exp(xi)[:, :3] - grid["M64"][:, :3, 3]).max(1)
    ratio = err / tol
    print("oracle exp translation: worst error / tolerance %.2f; rows with tolerance <= cap: %.1f %%"
          % (ratio.max(), 100 * (tol <= cap).mean()))
    assert (tol > 0).all() and np.isfinite(tol).all()
    assert (err <= tol).all(), np.flatnonzero(err > tol)
    assert (tol <= cap).mean() >= 1.0 / 3.0
    wc = S.well_conditioned(grid["theta"], grid["sigma"])
    assert wc.sum() == 8 * 5 * 5
    assert (tol[wc] <= cap[wc]).all()


def test_exp_is_ill_conditioned_where_the_issue_says(grid):
    """The two figures that motivate a row-wise tolerance, from the restatement: C = (e^sigma - 1) / sigma is off by
    more than 0.1 % just above |sigma| = 1e-6, and A = (1 - cos theta) / theta^2 is 0, not 1/2, at theta = 1e-4 with
    sigma = 0 - so the translation misses float64 by about |phi x tau| / 2."""
    xi, th, sg = grid["xi"], grid["theta"], grid["sigma"]
    e = S.scaled(np.abs(S.exp32(xi)[:, :3] - grid["M64"][:, :3, 3]).max(1), S.size_exp(xi))
    assert e[(np.abs(sg) == 1.01e-6) & (th == 0)].max() > 1e-3
    rows = (sg == 0) & (th == 1e-4)
    assert 1e-5 < e[rows].max() < 1e-4
    assert (e <= grid["tol"] / S.size_exp(xi)).all()


# ---- baselines --------------------------------------------------------------------------------------------------------
def test_fp32_baselines():
    """The float32 restatement and the C oracle against float64 with the measures the GPU tests assert; the maxima are
    the constants in tests/sim3_ref.py."""
    fresh = S.measure_baselines(oracle)
    for op, ms in fresh.items():
        print("fp32 %-5s" % op, {k: "%.3e" % v for k, v in ms.items()})
    assert {op: set(ms) for op, ms in fresh.items()} == {op: set(ms) for op, ms in S.BASELINES.items()}
    # the constants are this measurement; another libm rounds the oracle's sinf / cosf / expf differently, so a fresh
    # one may differ a little - a constant that is off by more is stale
    for op, ms in fresh.items():
        for k, v in ms.items():
            assert 0.5 * S.BASELINES[op][k] < v < 1.5 * S.BASELINES[op][k], (op, k, v)


def test_inputs_are_what_the_gpu_tests_assume():
    """Scales span 1e-3..1e3, |t| reaches 1e3 and |X| 1e2; identities, rotations within 1e-3 of pi and both signs of
    q are present in every batch size the GPU tests run but n = 1; quaternions are unit to 4 ulps."""
    for n in (63, 64, 65, 1000):
        T = S.poses(n, 1).astype(np.float64)
        assert np.abs(np.linalg.norm(T[:, 3:7], axis=1) - 1).max() <= 4 * S.F32_EPS
        ang = 2 * np.arccos(np.clip(np.abs(T[:, 6]), 0, 1))
        assert (ang == 0).any() and ((ang > np.pi - 1e-3) & (ang <= np.pi)).any()
        assert (T[:, 6] < 0).any() and (T[:, 6] > 0).any()
        assert T[:, 7].min() < 1e-2 and T[:, 7].max() > 1e2 and 1e-3 <= T[:, 7].min() and T[:, 7].max() <= 1e3
        assert 1e2 < np.linalg.norm(T[:, :3], axis=1).max() <= 1e3 * (1 + 1e-6)
    X = S.points(1000, 4)
    assert 50 < np.linalg.norm(X, axis=1).max() <= 1e2 * (1 + 1e-6)
    xi = S.steps(1000, 3)
    assert S.well_conditioned(np.linalg.norm(xi[:, 3:6], axis=1), xi[:, 6]).all()


# ---- the Sim3 class without a device ----------------------------------------------------------------------------------
def test_wrapper_refuses_host_tensors():
    from lietorch_hip import Sim3

    with pytest.raises(RuntimeError, match="device tensors only"):
        Sim3.Identity(1).inv()


def test_wrapper_matrix_on_cpu():
    from lietorch_hip import Sim3

    T = S.poses(65, 1)
    M = Sim3(torch.from_numpy(T.astype(np.float64)).reshape(5, 13, 8)).matrix()
    assert M.shape == (5, 13, 4, 4) and M.dtype == torch.float64
    want = np.stack([S.sim3_matrix(t) for t in T])
    # matrix() takes q as it is, sim3_matrix normalises it: the inputs are unit to 4 ulps of float32 (|q|^2 to 8), an
    # entry of R is quadratic in q and below 1, so it moves by at most 8 ulps; twice that is allowed, times s
    M64 = M.numpy().reshape(-1, 4, 4)
    assert (np.abs(M64 - want)[:, :3, :3].max((1, 2)) <= 16 * S.F32_EPS * T[:, 7]).all()
    assert np.array_equal(M64[:, :3, 3], T[:, :3].astype(np.float64)) and np.array_equal(M64[:, 3], want[:, 3])
    # float32 data: float32 arithmetic, a few more ulps
    M32 = Sim3(torch.from_numpy(T)).matrix().numpy().astype(np.float64)
    assert (np.abs(M32 - want)[:, :3, :3].max((1, 2)) <= 32 * S.F32_EPS * T[:, 7]).all()
    assert np.array_equal(M32[:, :3, 3], T[:, :3].astype(np.float64)) and np.array_equal(M32[:, 3], want[:, 3])
