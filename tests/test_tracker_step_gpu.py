"""GPU tests (-m gpu) of mslam_track_pose (csrc/tracker.hip) through the C ABI, one Gauss-Newton step at a time, against
the float64 reference of tests/tracker_ref.py: the step the kernel took (the Sim3 logarithm of the pose it wrote) must
solve the reference's normal equations to 4 x what the float32 oracle reaches on the same inputs, at every size where
the accumulation takes another path, with masks, Huber outliers and the calibrated gates in play; and the loop state in
the workspace must behave as documented (chunks, reset, stop flags, Cholesky failure)."""
import numpy as np
import pytest
import torch

import tracker_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 4.0     # kernel vs float32 baseline: per-thread fmaf chains, a wave tree, fp64 across blocks


@pytest.fixture(scope="module")
def case_set():
    return R.cases()


class Solver:
    """One input set on the device and a workspace; run() is one call of mslam_track_pose."""

    def __init__(self, c, device):
        import mslam_hip as m

        self.m, self.L, self.c, self.device = m, m.lib(), c, device
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.Xf, self.Xk, self.idx, self.Qk = t(c["Xf"]), t(c["Xk"]), t(c["idx"]), t(c["Qk"])
        self.valid = t(c["valid"].astype(np.uint8))
        self.K = t(c["K"]) if c["use_calib"] else None
        self.T = torch.empty(8, dtype=torch.float32, device=device)
        self.status = torch.zeros(8, dtype=torch.int32, device=device)
        self.ws = self.workspace(0)

    def workspace(self, fill):
        return torch.full((self.L.mslam_track_workspace_bytes(self.c["n"]),), fill, dtype=torch.uint8, device=self.device)

    def set_pose(self, T):
        self.T.copy_(torch.from_numpy(np.asarray(T, np.float32)))

    def run(self, first, last, rel_error=0.0, delta_norm=0.0):
        """-> (T f32[8], status i32[8], the same 32 bytes as f32[8])."""
        c, m = self.c, self.m
        rc = self.L.mslam_track_pose(c["use_calib"], m.ptr(self.T), m.ptr(self.Xf), m.ptr(self.Xk), m.ptr(self.idx), m.ptr(self.Qk),
                                     m.ptr(self.valid), c["n"], m.ptr(self.K), c["w"], c["h"], c["sigma_a"], c["sigma_b"],
                                     c["huber"], c["pixel_border"], c["z_eps"], first, last, rel_error, delta_norm,
                                     m.ptr(self.status), m.ptr(self.ws), self.ws.numel(), m.stream_ptr())
        m.check(rc, "track_pose")
        st = self.status.cpu().numpy().copy()
        return self.T.cpu().numpy().copy(), st, st.view(np.float32)


DONE, ITERS, CHOL_FAIL, OLD_COST, LAST_COST, LAST_DELTA = range(6)


def check_single_step(name, c, T0, T1, st, stf, ref):
    """The single-step assertion: backward error of the normal equations and the cost at FACTOR x the float32 baselines,
    last_delta_norm against |log(T1 T0^-1)| at the tolerance that logarithm round-trips to, the status record."""
    tau = R.sim3_log(T1, T0)
    be = R.backward_error(ref, tau)
    ce = abs(float(stf[LAST_COST]) - ref["cost"]) / ref["cost"]
    de = abs(float(stf[LAST_DELTA]) - np.linalg.norm(tau))
    print(f"step {name:24s} backward {be:.2e} ({be / R.FP32_BACKWARD_BASELINE:.3f} x baseline) cost {ce:.2e} "
          f"({ce / R.FP32_COST_BASELINE:.3f} x baseline) delta {de:.2e} (tol {R.roundtrip_tol(tau):.2e}) |tau| {np.linalg.norm(tau):.3g}")
    assert st[ITERS] == 1 and st[CHOL_FAIL] == 0 and st[DONE] == 0, (name, st[:3])
    assert be <= FACTOR * R.FP32_BACKWARD_BASELINE, (name, be)
    assert ce <= FACTOR * R.FP32_COST_BASELINE, (name, ce)
    assert de <= R.roundtrip_tol(tau), (name, de)
    return tau


def single_step(name, c, device):
    s = Solver(c, device)
    s.set_pose(c["T0"])
    T1, st, stf = s.run(0, 1)
    ref = R.reference(c)
    check_single_step(name, c, c["T0"], T1, st, stf, ref)
    return ref


@pytest.mark.parametrize("n", R.RAY_SIZES)
def test_single_step_rays(device, case_set, n):
    single_step(f"rays-{n}", case_set[f"rays-{n}"], device)


def test_single_step_rays_above_the_block_cap(device):
    """n = 1024 * 2048 + 1025: the grid is capped at 1024 blocks and the grid-stride loop takes a ninth, ragged trip."""
    single_step("rays-large", R.make_case("rays", R.RAY_LARGE), device)


@pytest.mark.parametrize("hw", R.CALIB_SIZES)
def test_single_step_calib(device, case_set, hw):
    name = f"calib-{hw[0]}x{hw[1]}"
    single_step(name, case_set[name], device)


@pytest.mark.parametrize("key", list(R.MASK_HUBER))
def test_single_step_mask_and_huber(device, case_set, key):
    """Half of the valid flags off, Qk over [1, 4], production sigmas and 1 / 1; between 20 % and 80 % of the rows that
    take part lie in Huber's outlier branch (asserted from the reference's whitened residuals)."""
    c = case_set["huber-" + key]
    ref = single_step("huber-" + key, c, device)
    assert 0.4 < c["valid"].mean() < 0.6
    assert c["Qk"].min() < 1.2 and c["Qk"].max() > 3.8
    assert 0.2 <= R.outlier_fraction(ref) <= 0.8


def test_single_step_calibrated_gates(device, case_set):
    """pixel_border = 2, z_eps = 0.05, keyframe depths at or below z_eps, frame points behind the camera: each gate alone
    removes >= 5 % of the points, >= 30 % survive all, and none lies within 1e-3 px / 1e-4 of a gate."""
    c = case_set["gates"]
    assert c["pixel_border"] == 2 and c["z_eps"] == 0.05
    ref = single_step("gates", c, device)
    R.check_gates(c, ref)


# ---- loop semantics ---------------------------------------------------------------------------------------------------
LOOP_CASES = ("rays-2049", "calib-17x31")


@pytest.mark.parametrize("name", LOOP_CASES)
@pytest.mark.parametrize("thresholds", [(0.0, 0.0), (1e-3, 1e-3)])
def test_chunked_loop_equals_uninterrupted(device, case_set, name, thresholds):
    c = case_set[name]
    a, b = Solver(c, device), Solver(c, device)
    a.set_pose(c["T0"]); b.set_pose(c["T0"])
    Ta, sta, _ = a.run(0, 12, *thresholds)
    b.run(0, 3, *thresholds)
    Tb, stb, _ = b.run(3, 12, *thresholds)
    assert Ta.tobytes() == Tb.tobytes() and sta.tobytes() == stb.tobytes(), (sta, stb)
    if thresholds == (0.0, 0.0):
        assert sta[ITERS] == 12 and sta[DONE] == 0
    else:
        assert 3 < sta[ITERS] <= 12


@pytest.mark.parametrize("name", LOOP_CASES)
def test_first_iter_zero_resets_a_dirty_workspace(device, case_set, name):
    c = case_set[name]
    a, b = Solver(c, device), Solver(c, device)
    b.ws = b.workspace(0xFF)
    a.set_pose(c["T0"]); b.set_pose(c["T0"])
    Ta, sta, _ = a.run(0, 3)
    Tb, stb, _ = b.run(0, 3)
    assert Ta.tobytes() == Tb.tobytes() and sta.tobytes() == stb.tobytes(), (sta, stb)
    assert sta[ITERS] == 3


@pytest.mark.parametrize("name", LOOP_CASES)
def test_stop_flags(device, case_set, name):
    c = case_set[name]
    s = Solver(c, device)
    s.set_pose(c["T0"])
    T_one, _, _ = s.run(0, 1)
    # |tau| < 1e9 at once: stops after iteration 1
    s.set_pose(c["T0"])
    T, st, _ = s.run(0, 12, 0.0, 1e9)
    assert st[ITERS] == 1 and st[DONE] == 1 and st[CHOL_FAIL] == 0
    assert T.tobytes() == T_one.tobytes()
    # a finished loop ignores further launches
    T2, st2, _ = s.run(1, 12, 0.0, 1e9)
    assert T2.tobytes() == T.tobytes() and st2.tobytes() == st.tobytes()
    T2, st2, _ = s.run(5, 7, 0.0, 0.0)
    assert T2.tobytes() == T.tobytes() and st2.tobytes() == st.tobytes()
    # relative decrease: iteration 1 compares against old = inf -> NaN -> no stop; iteration 2 stops
    s.set_pose(c["T0"])
    T, st, stf = s.run(0, 12, 1e9, 0.0)
    assert st[ITERS] == 2 and st[DONE] == 1 and st[CHOL_FAIL] == 0
    assert np.isfinite(stf[OLD_COST]) and stf[OLD_COST] == stf[LAST_COST]
    T2, st2, _ = s.run(2, 12, 1e9, 0.0)
    assert T2.tobytes() == T.tobytes() and st2.tobytes() == st.tobytes()


@pytest.mark.parametrize("what", ["rays-none-valid", "calib-none-valid", "rays-one-point"])
def test_cholesky_failure(device, case_set, what):
    """H = 0 (no valid point) or of rank 4 (one point): the factorisation fails, the pose stays as it was."""
    if what == "rays-one-point":
        c = R.make_case("rays", 1, valid_frac=1.0)
    else:
        c = dict(case_set["rays-2049" if what.startswith("rays") else "calib-17x31"])
        c["valid"] = np.zeros_like(c["valid"])
    s = Solver(c, device)
    s.set_pose(c["T0"])
    T, st, _ = s.run(0, 12)
    assert st[CHOL_FAIL] == 1 and st[DONE] == 1 and st[ITERS] == 1, st[:3]
    assert T.tobytes() == c["T0"].tobytes()


@pytest.mark.parametrize("name", LOOP_CASES)
def test_trajectory_of_single_steps(device, case_set, name):
    """Four single-iteration calls, each from the pose the GPU produced: every step passes the single-step assertion
    against the reference evaluated at that pose, and the reference's cost does not increase along them."""
    c = case_set[name]
    s = Solver(c, device)
    T = c["T0"]
    costs = []
    for k in range(4):
        s.set_pose(T)
        T1, st, stf = s.run(0, 1)
        ref = R.reference(c, T)
        check_single_step(f"{name} step {k}", c, T, T1, st, stf, ref)
        costs.append(ref["cost"])
        T = T1
    assert all(b <= a for a, b in zip(costs, costs[1:])), costs
