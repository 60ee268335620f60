"""CPU tests of the ICP loop that align_meshes and align_clouds share (mast3r_slam.tsdf.mesh_align._icp_run and
_icp_args): the stop rule, driven by a scripted step that writes given (inliers, rmse, scale, status) rows into a host
log tensor, and the refusals of the loop arguments.  No device is touched."""
import math

import numpy as np
import pytest
import torch

from mast3r_slam.tsdf.mesh_align import DEGENERATE, OK, _icp_args, _icp_run


def run(rows, max_iters, check_every, tol, columns=4):
    """_icp_run over the scripted rows -> (iterations, converged, history, the iterations step was called with).  The
    log is max_iters x `columns` (align_meshes' log is wider than the four figures), NaN where no step has written."""
    rows = np.asarray(rows, np.float64)
    log = torch.full((max_iters, columns), math.nan, dtype=torch.float64)
    calls = []

    def step(it):
        calls.append(it)
        log[it, :4] = torch.from_numpy(rows[it])

    iterations, converged, hist = _icp_run(step, log, max_iters, check_every, tol)
    assert calls == list(range(iterations))                    # every iteration once, in order, none after the stop
    assert isinstance(hist, np.ndarray) and hist.dtype == np.float64 and hist.shape == (iterations, 4)
    np.testing.assert_array_equal(hist, rows[:iterations])
    return iterations, converged


def rows_of(rmse, status=None):
    status = [OK] * len(rmse) if status is None else status
    return [(100.0 + i, r, 1.0, s) for i, (r, s) in enumerate(zip(rmse, status))]


@pytest.mark.parametrize("columns", [4, 9])
def test_convergence_on_a_check_boundary(columns):
    # the RMSE stops changing between iterations 5 and 6 (1-based), and 6 is a check
    rows = rows_of([8.0, 4.0, 2.0, 1.0, 0.5, 0.5, 0.25, 0.25, 0.25])
    assert run(rows, 9, 3, 1e-6, columns) == (6, True)
    # within tol relative, not only equal: |0.5 - 0.4996| = 4e-4 <= 1e-3 * 0.5, and 1e-4 is too tight for it
    rows = rows_of([8.0, 4.0, 2.0, 1.0, 0.5, 0.4996, 0.1, 0.05, 0.01])
    assert run(rows, 9, 3, 1e-3, columns) == (6, True)
    assert run(rows, 9, 3, 1e-4, columns) == (9, False)


def test_convergence_between_checks_is_reported_at_the_next_check():
    # iterations 2 and 3 agree, but the log is first read after 4, where 3 and 4 agree too
    assert run(rows_of([8.0, 0.5, 0.5, 0.5, 0.1, 0.1, 0.1, 0.1]), 8, 4, 1e-6) == (4, True)
    # only the two iterations before a read are compared: 2 and 3 agree, 3 and 4 do not, so the loop goes on to 8
    assert run(rows_of([8.0, 0.5, 0.5, 0.4, 0.3, 0.2, 0.1, 0.1]), 8, 4, 1e-6) == (8, True)
    assert run(rows_of([8.0, 0.5, 0.5, 0.4, 0.3, 0.2, 0.1, 0.05]), 8, 4, 1e-6) == (8, False)


def test_degenerate_status_is_found_at_the_next_check():
    status = [OK, OK, OK, DEGENERATE, DEGENERATE, DEGENERATE, DEGENERATE, DEGENERATE, DEGENERATE, DEGENERATE]
    rmse = [8.0, 4.0, 2.0, math.inf, math.inf, math.inf, math.inf, math.inf, math.inf, math.inf]
    # degenerate from iteration 4 on; the reads come after 5 and 10, and the one after 5 stops the loop, not converged
    # although the RMSE repeats
    assert run(rows_of(rmse, status), 10, 5, 1e-6) == (5, False)
    # a status that is OK again at the read is not seen: only the latest row's status is tested
    status = [OK, OK, DEGENERATE, OK, OK, OK]
    assert run(rows_of([8.0, 4.0, 2.0, 1.0, 0.5, 0.25], status), 6, 2, 1e-6) == (6, False)
    status = [OK, OK, OK, DEGENERATE, OK, OK]
    assert run(rows_of([8.0, 4.0, 2.0, 1.0, 0.5, 0.25], status), 6, 2, 1e-6) == (4, False)


def test_final_read_when_max_iters_is_no_multiple_of_check_every():
    rmse = [8.0, 4.0, 2.0, 1.0, 0.5, 0.25, 0.125]
    assert run(rows_of(rmse), 7, 3, 1e-6) == (7, False)                 # reads after 3, 6 and 7
    assert run(rows_of(rmse[:5] + [0.3, 0.3]), 7, 3, 1e-6) == (7, True)  # the last read is a check like any other
    assert run(rows_of(rmse[:6] + [0.1], [OK] * 6 + [DEGENERATE]), 7, 3, 1e-6) == (7, False)
    assert run(rows_of(rmse[:2]), 2, 5, 1e-6) == (2, False)             # check_every beyond max_iters: one read


def test_tol_zero_needs_an_exactly_repeated_rmse():
    x = 0.1 + 0.2
    assert run(rows_of([1.0, x, x]), 3, 1, 0.0) == (3, True)
    assert run(rows_of([1.0, x, np.nextafter(x, 1.0), 0.0]), 4, 1, 0.0) == (4, False)
    assert run(rows_of([1.0, 0.0, 0.0]), 3, 1, 0.0) == (3, True)        # 0 <= 0 * 0


def test_a_single_iteration_is_never_converged():
    assert run(rows_of([0.0]), 1, 1, 1.0) == (1, False)
    assert run(rows_of([0.5]), 1, 5, math.inf) == (1, False)
    assert run(rows_of([0.5, 0.5, 0.5]), 3, 1, 0.0) == (2, True)        # the first read after which two rows exist
    assert run(rows_of([0.5], [DEGENERATE]), 1, 1, 1.0) == (1, False)


@pytest.mark.parametrize("what", ["align_meshes", "align_clouds"])
def test_icp_args(what):
    assert _icp_args(what, 3, 2, 0.0, 0.25) == (3, 2, [0.25, 0.25, 0.25])
    assert _icp_args(what, 2.0, 7.0, 1e-6, math.inf) == (2, 7, [math.inf, math.inf])
    for seq in ([0.3, 0.2, 0.0], (0.3, 0.2, 0.0), np.array([0.3, 0.2, 0.0])):
        max_iters, check_every, trims = _icp_args(what, 3, 1, 1e-6, seq)
        assert (max_iters, check_every, trims) == (3, 1, [0.3, 0.2, 0.0]) and all(type(t) is float for t in trims)
    with pytest.raises(ValueError, match=rf"^{what}: a trim sequence needs one value per iteration \(5\), got 2$"):
        _icp_args(what, 5, 1, 1e-6, [0.1, 0.2])
    with pytest.raises(ValueError, match=rf"^{what}: a trim sequence needs one value per iteration \(2\), got 3$"):
        _icp_args(what, 2, 1, 1e-6, np.array([0.1, 0.2, 0.3]))
    with pytest.raises(ValueError, match=rf"^{what}: trim must be >= 0 \(\+inf keeps every pair\)$"):
        _icp_args(what, 3, 1, 1e-6, -0.5)
    with pytest.raises(ValueError, match=rf"^{what}: trim must be >= 0"):
        _icp_args(what, 3, 1, 1e-6, [0.1, -0.0001, 0.1])
    with pytest.raises(ValueError, match=rf"^{what}: trim must be >= 0"):
        _icp_args(what, 3, 1, 1e-6, math.nan)
    with pytest.raises(ValueError, match=rf"^{what}: max_iters and check_every must be >= 1, got 0 and 5$"):
        _icp_args(what, 0, 5, 1e-6, math.inf)
    with pytest.raises(ValueError, match=rf"^{what}: max_iters and check_every must be >= 1, got 3 and 0$"):
        _icp_args(what, 3, 0, 1e-6, math.inf)
    with pytest.raises(ValueError, match=rf"^{what}: tol must be >= 0, got nan$"):
        _icp_args(what, 3, 1, math.nan, math.inf)
    with pytest.raises(ValueError, match=rf"^{what}: tol must be >= 0, got -1.0$"):
        _icp_args(what, 3, 1, -1.0, math.inf)
