"""GPU tests (-m gpu) of the global Gauss-Newton loop state and of the opened-up loop (mslam_gn_begin / compact /
compact_at / accumulate / solve_retract / status, include/mslam_hip.h) through the C ABI: the opened loop against the
closed entry points bit for bit, compaction by slots, the documented status record {done, iterations, chol_fail,
||dx||} after a solve, after convergence and after a failed factorisation, and an edge listed twice."""
import numpy as np
import pytest
import torch

import gn_ref as G
from gn_abi import CHOL_FAIL, DONE, ITERS, LAST_NORM, Gn
from test_gn_blocks_gpu import FACTOR

pytestmark = pytest.mark.gpu

LOOP_CASES = {"rays": "rays-production-24x32", "calib": "calib-production-24x32", "points": "points-production-24x32"}


@pytest.fixture(scope="module")
def case_set():
    return G.cases()


def bits(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("k", [1, 3])
def test_opened_loop_equals_closed_entry(device, case_set, kind, k):
    c = case_set[LOOP_CASES[kind]]
    T_closed, dx_closed = Gn(c, device).closed(k)
    s = Gn(c, device)
    Twc, dx = s.poses()
    Hs, gs = s.buffers()
    s.begin()
    s.compact()
    for _ in range(k):
        s.accumulate(Twc, Hs, gs)
        s.solve(Hs, gs, Twc, dx)
    st, _ = s.status()
    assert st[ITERS] == k and st[DONE] == 0 and st[CHOL_FAIL] == 0, st
    assert dx_closed.abs().max() > 0
    assert bits(Twc) == bits(T_closed) and bits(dx) == bits(dx_closed)


@pytest.mark.parametrize("kind", G.KINDS)
def test_compaction_slots(device, case_set, kind):
    """Two compact_at calls, each with its own slices of idx / valid / Q and its edge_begin, fill the slots [0, cut) and
    [cut, E) of one accumulate range: blocks bit-identical to one compact."""
    c = case_set[LOOP_CASES[kind]]
    whole = Gn(c, device)
    Hs, gs = whole.buffers()
    whole.begin()
    whole.compact()
    whole.accumulate(whole.Twc0, Hs, gs)
    s = Gn(c, device)
    E, cut = c["E"], c["E"] // 3 + 1
    Hp, gp = s.buffers()
    s.begin()
    s.compact_at(cut, E - cut, cut, E)          # the later slots first: the order of the calls does not matter
    s.compact_at(0, cut, 0, E)
    s.accumulate(s.Twc0, Hp, gp)
    assert Hs.abs().sum() > 0
    assert bits(Hs) == bits(Hp) and bits(gs) == bits(gp)


@pytest.mark.parametrize("kind", G.KINDS)
def test_status_after_one_solve(device, case_set, kind):
    c = case_set[LOOP_CASES[kind]]
    s = Gn(c, device)
    Twc, dx = s.poses()
    Hs, gs = s.buffers()
    s.begin()
    st, _ = s.status()
    assert not st.any(), st
    s.compact()
    s.accumulate(Twc, Hs, gs)
    s.solve(Hs, gs, Twc, dx, 0.0)
    st, stf = s.status()
    assert st[ITERS] == 1 and st[DONE] == 0 and st[CHOL_FAIL] == 0, st
    nrm = np.linalg.norm(dx.cpu().numpy().astype(np.float64))
    assert nrm > 0 and abs(float(stf[LAST_NORM]) - nrm) <= 1e-6 * nrm, (stf[LAST_NORM], nrm)


def test_status_after_convergence(device, case_set):
    """delta_thresh = 1e9: done after the first solve; a further accumulate leaves sentinel-filled Hs / gs untouched, a
    further solve_retract leaves Twc, dx and the iteration count untouched."""
    c = case_set[LOOP_CASES["rays"]]
    s = Gn(c, device)
    Twc, dx = s.poses()
    Hs, gs = s.buffers()
    s.begin()
    s.compact()
    s.accumulate(Twc, Hs, gs)
    s.solve(Hs, gs, Twc, dx, 1e9)
    st, _ = s.status()
    assert st[DONE] == 1 and st[ITERS] == 1 and st[CHOL_FAIL] == 0, st
    assert bits(Twc) != bits(s.Twc0)
    T1, dx1 = bits(Twc), bits(dx)
    Hsent, gsent = s.buffers(fill=-7.5)
    s.accumulate(Twc, Hsent, gsent)
    assert (Hsent == -7.5).all() and (gsent == -7.5).all()
    s.solve(Hs, gs, Twc, dx, 1e9)
    s.solve(Hs, gs, Twc, dx, 0.0)
    st2, _ = s.status()
    assert bits(Twc) == T1 and bits(dx) == dx1 and st2.tobytes() == st.tobytes(), (st, st2)


@pytest.mark.parametrize("kind", G.KINDS)
def test_factorisation_failure_is_recorded(device, case_set, kind):
    """Every match invalid: H = 0, the factorisation fails, dx = 0, the poses stay, and status[2] says so after that solve.
    A later solve on good inputs that succeeds clears it: in the same loop, and from a fresh begin."""
    c = case_set[LOOP_CASES[kind]]
    s = Gn(c, device)
    Twc, dx = s.poses()
    dx.fill_(3.0)
    Hs, gs = s.buffers()
    s.begin()
    s.compact(vm=torch.zeros_like(s.vm))
    s.accumulate(Twc, Hs, gs)
    assert not Hs.any() and not gs.any()
    s.solve(Hs, gs, Twc, dx)
    st, stf = s.status()
    assert not dx.any() and bits(Twc) == bits(s.Twc0)
    assert st[CHOL_FAIL] != 0 and st[ITERS] == 1 and st[DONE] == 0 and stf[LAST_NORM] == 0, st
    # the same loop goes on with good inputs
    s.compact()
    s.accumulate(Twc, Hs, gs)
    s.solve(Hs, gs, Twc, dx)
    st, _ = s.status()
    assert st[CHOL_FAIL] == 0 and st[ITERS] == 2 and dx.abs().max() > 0, st
    # failure again, then a fresh begin
    Twc, dx = s.poses()
    s.compact(vm=torch.zeros_like(s.vm))
    s.accumulate(Twc, Hs, gs)
    s.solve(Hs, gs, Twc, dx)
    assert s.status()[0][CHOL_FAIL] != 0
    s.begin()
    assert s.status()[0][CHOL_FAIL] == 0
    s.compact()
    s.accumulate(Twc, Hs, gs)
    s.solve(Hs, gs, Twc, dx)
    st, _ = s.status()
    assert st[CHOL_FAIL] == 0 and st[ITERS] == 1 and dx.abs().max() > 0, st
    T_closed, dx_closed = Gn(c, device).closed(1)
    assert bits(Twc) == bits(T_closed) and bits(dx) == bits(dx_closed)


@pytest.mark.parametrize("kind", G.KINDS)
def test_duplicate_edge(device, case_set, kind):
    """The first directed edge listed twice: the step solves the reference's dense normal equations with that edge counted
    twice, at the bar of test_gn_blocks_gpu.py::test_one_step."""
    c = case_set[LOOP_CASES[kind]]
    g = c["g"]
    dup = lambda a: np.concatenate([a, a[:1]])
    g2 = dict(g, **{k: dup(g[k]) for k in ("ii", "jj", "idx_ii2jj", "valid_match", "Q")})
    c2 = dict(c, g=g2, E=c["E"] + 1)
    ref = G.reference(c2)
    assert np.array_equal(ref["H"][0], ref["H"][-1]) and ref["H"].shape[0] == c["E"] + 1
    ie, je = G.edge_rows(g2["ii"], g2["jj"])
    once = G.dense(G.reference(c), *G.edge_rows(g["ii"], g["jj"]), c["P"] - 1)
    twice = G.dense(ref, ie, je, c["P"] - 1)
    assert np.abs(twice["H"] - once["H"]).max() > 1e-3 * np.abs(once["H"]).max()
    Twc, dx = Gn(c2, device).closed(1)
    be = G.backward_error(twice, dx.cpu().numpy())
    print(f"duplicate {kind}: backward {be:.2e} ({be / G.FP32_BACKWARD_BASELINE:.3f} x baseline), counted once "
          f"{G.backward_error(once, dx.cpu().numpy()):.2e}")
    assert be <= FACTOR * G.FP32_BACKWARD_BASELINE, be
