"""GPU tests (-m gpu) of the mesh-alignment kernels (csrc/mesh_align.hip, DESIGN.md "Mesh alignment") and of
mast3r_slam.tsdf.fit_sim3 / transform_mesh / align_meshes / compare_meshes(align=...), SlamSystem.align_trajectory /
evaluate_mesh(align=...) and evaluate.trajectory_ate, against mslam_mesh_distance (bit for bit) and the numpy statement
(tests/meshalign_numpy.py).

Bounds.  The match: dist2 and nearest byte for byte those of mslam_mesh_distance(skip=0) on the step's own moved points;
the moved points within one f32 ulp of the numpy transform; the closest point within 1e-12 of the largest coordinate.
The sums: |device - exact sum of the same terms| <= n * 2^-52 * sum |term|, which holds for any order of summation.
The solve: within 1e-9 of the numpy Horn solve of the device's own sums."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

from mast3r_slam import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshalign_numpy as A  # noqa: E402
import meshdist_numpy as D  # noqa: E402
from test_mesh_align_cpu import pair_case, recovery_run  # noqa: E402
from kernel_refs import Guarded, check_guards  # noqa: E402
from mesh_support import BLOCK, VS, T as TILE, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

STEP_N = (1, BLOCK - 1, BLOCK, BLOCK + 1, 4 * BLOCK + 1)
STEP_F = (1, TILE - 1, TILE, TILE + 1, 4 * TILE + 1)
T0 = A.sim3_from((37.0, (1.0, -2.0, 0.5)), (0.3, -1.0, 2.0), 1.7).astype(np.float32)      # a non-trivial Sim3
LOG = 24
SOLVE_TOL = 1e-9


def _lib():
    import mslam_hip as _m

    return _m, _m.lib(), _m.stream_ptr()


@functools.lru_cache(maxsize=None)
def align_case(nf, n):
    """Triangles and target-frame points as tile_case of tests/test_mesh_metrics_gpu.py builds them (small random
    triangles in the unit cube in the order of their x, points in the order of theirs, far outliers among both), two
    invalid faces where there is room, and the source points: the target-frame points moved by T0^-1."""
    rng = np.random.default_rng(1000 * nf + n)
    centre = rng.uniform(0.0, 1.0, (nf, 3))
    centre = centre[np.argsort(centre[:, 0])]
    V = (centre[:, None, :] + rng.uniform(-0.06, 0.06, (nf, 3, 3))).astype(np.float32).reshape(-1, 3)
    far = rng.choice(min(nf, TILE), min(3, nf // 8), replace=False)
    V.reshape(nf, 3, 3)[far] += np.float32(40.0)
    F = np.arange(3 * nf, dtype=np.int32).reshape(nf, 3)
    if nf >= TILE - 1:
        F[5] = [0, 0, 1]                                   # no area
        F[nf - 2] = [3 * nf, 1, 2]                         # an index out of range
    Q = rng.uniform(-0.1, 1.1, (n, 3))
    Q = Q[np.argsort(Q[:, 0])]
    Q[0] -= 30.0
    Q[n // 2] += 45.0
    P = A.act(A.sim3_inv(A.init_state(T0)), Q).astype(np.float32)
    return P, V, F


def _step(device, P, V, F, init=T0, warm=None, trim=math.inf, with_scale=True, steps=1, guard=False, count=False):
    """mslam_mesh_align_init, then `steps` calls of mslam_mesh_align_step -> dict of host arrays of the LAST step, the
    state before it (T_before) and after (T, status), and the log rows of all steps."""
    _m, L, st = _lib()
    n, nf = len(P), len(F)
    p, v, f = _dev(device, P, np.float32), _dev(device, V, np.float32), _dev(device, F, np.int32)
    t0 = None if init is None else _dev(device, init, np.float32)
    wb = int(L.mslam_mesh_align_workspace_bytes(n, nf, 1 if count else 0))
    assert wb == 48 * ((nf + TILE - 1) // TILE) + (19 * 8 + (16 if count else 0)) * ((n + BLOCK - 1) // BLOCK)
    make = (lambda dt, shape: Guarded(device, dt, shape)) if guard else None
    bufs = {}
    for name, dt, shape in (("ws", torch.float64, (max(wb // 8, 1),)), ("state", torch.float64, (9,)),
                            ("nearest", torch.int32, (n,)), ("moved", torch.float32, (n, 3)),
                            ("dist2", torch.float64, (n,)), ("closest", torch.float64, (n, 3)),
                            ("log", torch.float64, (steps, LOG))):
        if guard and int(np.prod(shape)) > 0:
            bufs[name] = make(dt, shape)
            bufs[name + "_t"] = bufs[name].t
        else:
            bufs[name + "_t"] = torch.zeros(shape, dtype=dt, device=device)
    ws, state, nearest = bufs["ws_t"], bufs["state_t"], bufs["nearest_t"]
    nearest.copy_(_dev(device, np.full(n, -1) if warm is None else warm, np.int32))
    _m.check(L.mslam_mesh_align_init(_m.ptr(t0), _m.ptr(v), _m.ptr(f), nf, len(V), _m.ptr(ws), wb, _m.ptr(state), st),
             "mesh_align_init")
    T64, T32 = torch.empty(8, dtype=torch.float64, device=device), torch.empty(8, dtype=torch.float32, device=device)
    status = torch.full((1,), -5, dtype=torch.int32, device=device)
    for k in range(steps):
        _m.check(L.mslam_mesh_align_read(_m.ptr(state), _m.ptr(T64), 0, 0, st), "mesh_align_read")
        before = T64.cpu().numpy().copy()
        _m.check(L.mslam_mesh_align_step(_m.ptr(p), n, _m.ptr(v), _m.ptr(f), nf, len(V), float(trim),
                                         1 if with_scale else 0, 1 if count else 0, _m.ptr(ws), wb, _m.ptr(state),
                                         _m.ptr(nearest), _m.ptr(bufs["moved_t"]), _m.ptr(bufs["dist2_t"]),
                                         _m.ptr(bufs["closest_t"]), _m.ptr(bufs["log_t"][k]), st), "mesh_align_step")
    _m.check(L.mslam_mesh_align_read(_m.ptr(state), _m.ptr(T64), _m.ptr(T32), _m.ptr(status), st), "mesh_align_read")
    out = {k[:-2]: t.cpu().numpy() for k, t in bufs.items() if k.endswith("_t")}
    out.update(T_before=before, T=T64.cpu().numpy(), T32=T32.cpu().numpy(), status=int(status), guards=bufs, p=p, v=v,
               f=f)
    if count and n and nf:
        waves = (n + 63) // 64
        counts = ws.view(torch.int32)[-4 * ((n + BLOCK - 1) // BLOCK):].cpu().numpy()[:waves]
        out["skipped"] = float(counts.sum()) / (waves * ((nf + TILE - 1) // TILE))
    return out


def _mesh_distance(device, r, skip=0):
    """mslam_mesh_distance on the step's own moved points -> (dist2, nearest) host arrays."""
    _m, L, st = _lib()
    n, nf = r["moved"].shape[0], int(r["f"].shape[0])
    q = _dev(device, r["moved"], np.float32)
    d2 = torch.empty(n, dtype=torch.float64, device=device)
    near = torch.empty(n, dtype=torch.int32, device=device)
    wb = int(L.mslam_mesh_distance_workspace_bytes(nf)) if skip else 0
    ws = torch.zeros(max(wb, 8), dtype=torch.uint8, device=device)
    _m.check(L.mslam_mesh_distance(_m.ptr(q), n, _m.ptr(r["v"]), _m.ptr(r["f"]), nf, int(r["v"].shape[0]), skip,
                                   _m.ptr(ws), wb, _m.ptr(d2), _m.ptr(near), st), "mesh_distance")
    return d2.cpu().numpy(), near.cpu().numpy()


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _check_sums(log_row, terms, n):
    """The reduced sums of a log row against the exact sum of `terms`, within the bound that holds for any order.
    Returns the largest error as a share of the bound."""
    worst = 0.0
    for k in range(A.N_SUMS):
        exact = math.fsum(terms[:, k])
        bound = n * 2.0 ** -52 * math.fsum(np.abs(terms[:, k]))
        err = abs(log_row[4 + k] - exact)
        assert err <= bound, (k, log_row[4 + k], exact, bound)
        worst = max(worst, err / bound if bound > 0.0 else 0.0)
    return worst


def _check_solve(r, sums, op, oc, with_scale=True):
    """The state after a step against the numpy Horn solve of the device's own sums -> the largest difference."""
    want = A.horn_solve(sums, op, oc, with_scale)
    if want is None:
        assert r["status"] == A.DEGENERATE and np.array_equal(r["T"], r["T_before"])
        return 0.0
    assert r["status"] == A.OK
    diff = float(np.abs(r["T"] - want).max())
    assert diff <= SOLVE_TOL, (diff, r["T"], want)
    assert np.array_equal(r["T32"], r["T"].astype(np.float32))
    return diff


# ----------------------------------------------------------------------------------------------------------------------
# 1., 2. one step: the match is mesh_distance, the closest point, the sums and the solve
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", STEP_N)
@pytest.mark.parametrize("nf", STEP_F)
def test_step_matches_mesh_distance_and_numpy(device, nf, n):
    """Measured on MI355X over all shapes: the sums reach at most 0.006 of their bound, the solve differs from numpy's by
    at most 3.9e-14."""
    P, V, F = align_case(nf, n)
    cold = _step(device, P, V, F)
    state0 = A.init_state(T0)
    assert np.abs(cold["T_before"] - state0).max() <= 2.0 ** -52 * np.abs(state0).max()
    want_q = A.act(cold["T_before"], P.astype(np.float64))
    assert (np.abs(cold["moved"].astype(np.float64) - want_q) <= _ulp32(want_q)).all()
    d2, near = _mesh_distance(device, cold)
    assert cold["dist2"].tobytes() == d2.tobytes() and cold["nearest"].tobytes() == near.tobytes()
    culled = _mesh_distance(device, cold, skip=1)
    assert culled[0].tobytes() == d2.tobytes() and culled[1].tobytes() == near.tobytes()
    valid = D.triangles(V, F)[3]
    assert (near >= 0).all() and valid[near].all()
    # the closest point, and through it dist2 once more
    want_c = A.closest_points(cold["moved"], V, F, near)
    scale = max(np.abs(V[F[valid]]).max(), np.abs(cold["moved"]).max())
    assert np.abs(cold["closest"] - want_c).max() <= 1e-12 * scale
    r = cold["moved"].astype(np.float64) - cold["closest"]
    assert (np.abs(D._dot(r, r) - d2) <= 1e-12 * d2).all()
    # warm starts change no bit: the right faces, wrong ones, faces out of range, invalid faces
    rng = np.random.default_rng(nf + n)
    wrong = rng.integers(0, nf, n)
    wrong[::7] = [nf, nf + 5, -7, 2 ** 31 - 1, -2 ** 31][n % 5]
    if nf >= TILE - 1:
        wrong[1::5] = 5
        wrong[2::9] = nf - 2
    for warm in (near, wrong, np.where(np.arange(n) % 2 == 0, near, -1)):
        hot = _step(device, P, V, F, warm=warm)
        for key in ("moved", "dist2", "nearest", "closest", "log", "T"):
            assert hot[key].tobytes() == cold[key].tobytes(), key
    # the sums over every pair (trim = inf), and the solve of the device's own sums
    p64 = P.astype(np.float64)
    op, oc = p64[0], A.act(cold["T_before"], p64[:1])[0]
    terms = A.sum_terms(p64, cold["closest"], np.ones(n), np.ones(n, bool), op, oc, d2)
    share = _check_sums(cold["log"][0], terms, n)
    diff = _check_solve(cold, cold["log"][0][4:4 + A.N_SUMS], op, oc)
    row = cold["log"][0]
    assert row[0] == n and row[3] == cold["status"] and row[2] == cold["T"][7]
    assert abs(row[1] - np.sqrt(math.fsum(d2) / n)) <= n * 2.0 ** -52 * row[1]
    print(f"F={nf} n={n}: sums at {share:.3f} of the bound, solve within {diff:.2e}, status {cold['status']}")
    assert cold["status"] == (A.OK if n >= 3 else A.DEGENERATE)


@pytest.mark.parametrize("n", [BLOCK - 1, BLOCK + 1])
@pytest.mark.parametrize("nf", [TILE, TILE + 1, 4 * TILE + 1])
def test_cold_step_skips_the_tiles_mesh_distance_skips(device, nf, n):
    """One scan, two callers (md_scan of csrc/mesh_tri.h): a cold step takes its bound from the home tile of the
    block's first moved point, as mslam_mesh_distance does on the same points, so every wave skips the same number of
    tiles, the int32 words themselves, and returns the same bytes.  One tile is scanned plainly by both: no tile is
    skipped."""
    _m, L, st = _lib()
    P, V, F = align_case(nf, n)
    cold = _step(device, P, V, F, count=True)
    nblk, waves = (n + BLOCK - 1) // BLOCK, (n + 63) // 64
    step_counts = cold["ws"].view(np.int32)[-4 * nblk:][:waves]
    box = int(L.mslam_mesh_distance_workspace_bytes(nf))
    ws = torch.full((box + 16 * nblk,), 0xFF, dtype=torch.uint8, device=device)
    d2 = torch.empty(n, dtype=torch.float64, device=device)
    near = torch.empty(n, dtype=torch.int32, device=device)
    _m.check(L.mslam_mesh_distance(_m.ptr(_dev(device, cold["moved"], np.float32)), n, _m.ptr(cold["v"]),
                                   _m.ptr(cold["f"]), nf, int(cold["v"].shape[0]), 2, _m.ptr(ws), ws.numel(),
                                   _m.ptr(d2), _m.ptr(near), st), "mesh_distance")
    dist_counts = ws[box:].view(torch.int32).cpu().numpy()[:waves]
    print(f"F={nf} n={n}: skipped per wave, step {step_counts.tolist()}, mesh_distance {dist_counts.tolist()}")
    assert np.array_equal(step_counts, dist_counts)
    assert cold["dist2"].tobytes() == d2.cpu().numpy().tobytes()
    assert cold["nearest"].tobytes() == near.cpu().numpy().tobytes()
    if nf <= TILE:
        assert not step_counts.any() and not dist_counts.any()


@pytest.mark.parametrize("nf,n", [(4 * TILE + 1, 4 * BLOCK + 1), (TILE + 1, BLOCK - 1), (TILE - 1, 3 * 64 + 7)])
def test_trimmed_sums_and_solve(device, nf, n):
    """A trim that drops most pairs, a whole block (points 256..511) and whole waves without an inlier, n no multiple
    of 64, without scale too.  Measured on MI355X: sums at most 0.003 of the bound, solve within 6.7e-16."""
    P, V, F = align_case(nf, n)
    P = P.copy()
    P[BLOCK:2 * BLOCK] += np.float32(10.0)
    P[n - 40:] -= np.float32(20.0)
    p64 = P.astype(np.float64)
    for trim, with_scale in ((0.08, True), (0.08, False), (0.0, True)):
        r = _step(device, P, V, F, trim=trim, with_scale=with_scale)
        d2, near = _mesh_distance(device, r)
        assert r["dist2"].tobytes() == d2.tobytes() and r["nearest"].tobytes() == near.tobytes()
        inlier = (near >= 0) & (d2 <= np.float64(trim) * np.float64(trim))
        assert not inlier[BLOCK:2 * BLOCK].any() and not inlier[n - 40:].any()
        op, oc = p64[0], A.act(r["T_before"], p64[:1])[0]
        terms = A.sum_terms(p64, r["closest"], np.ones(n), inlier, op, oc, d2)
        share = _check_sums(r["log"][0], terms, n)
        diff = _check_solve(r, r["log"][0][4:4 + A.N_SUMS], op, oc, with_scale)
        assert r["log"][0][0] == inlier.sum()
        if trim > 0.0 and nf > 1:
            assert 3 <= inlier.sum() < n - 40 and r["status"] == A.OK
        if trim == 0.0:
            assert r["status"] == A.DEGENERATE and np.array_equal(r["T"], r["T_before"])
        if not with_scale and r["status"] == A.OK:
            assert r["T"][7] == 1.0
        print(f"F={nf} n={n} trim={trim} scale={with_scale}: inliers {inlier.sum()}, sums at {share:.3f} of the bound, "
              f"solve within {diff:.2e}")


def test_no_target_and_no_points(device):
    P, V, F = align_case(TILE + 1, BLOCK + 1)
    for faces in (np.zeros((0, 3), np.int32), np.array([[0, 0, 1], [3 * len(F), 1, 2], [-1, 2, 3]], np.int32)):
        r = _step(device, P, V, faces)
        assert r["status"] == A.DEGENERATE and np.array_equal(r["T"], r["T_before"])
        assert np.isposinf(r["dist2"]).all() and (r["nearest"] == -1).all() and np.isnan(r["closest"]).all()
        assert r["log"][0][0] == 0 and np.isposinf(r["log"][0][1]) and r["log"][0][3] == A.DEGENERATE
    r = _step(device, P[:0], V, F, init=None)
    assert r["status"] == A.DEGENERATE and np.array_equal(r["T"], A.init_state()) and r["log"][0][0] == 0


# ----------------------------------------------------------------------------------------------------------------------
# 3. the same bytes on every run
# ----------------------------------------------------------------------------------------------------------------------
def test_ten_steps_twice_give_the_same_bytes(device):
    P, V, F = align_case(4 * TILE + 1, 4 * BLOCK + 1)
    start = A.sim3_from((39.0, (1.0, -2.0, 0.4)), (0.32, -1.0, 1.98), 1.68).astype(np.float32)       # near T0
    runs = [_step(device, P, V, F, init=start, trim=0.2, steps=10, count=True) for _ in range(2)]
    for key in ("T", "T32", "log", "nearest", "moved", "dist2", "closest"):
        assert runs[0][key].tobytes() == runs[1][key].tobytes(), key
    log = runs[0]["log"]
    assert (log[:, 3] == A.OK).all() and (log[:, 0] >= 3).all()
    assert not np.array_equal(runs[0]["T"], A.init_state(start))    # and they are iterations of something
    print(f"ten steps: rmse {log[0, 1]:.4g} -> {log[-1, 1]:.4g}, inliers {int(log[0, 0])} -> {int(log[-1, 0])}, "
          f"(wave, tile) scans skipped in the last step {runs[0]['skipped']:.3f}")


# ----------------------------------------------------------------------------------------------------------------------
# 4. fit_sim3
# ----------------------------------------------------------------------------------------------------------------------
def _fit_raw(device, P, C, w, with_scale):
    _m, L, st = _lib()
    n = len(P)
    p, c = _dev(device, P, np.float32), _dev(device, C, np.float32)
    wt = None if w is None else _dev(device, w, np.float32)
    wb = int(L.mslam_mesh_align_workspace_bytes(n, 0, 0))
    ws = torch.zeros(max(wb, 8), dtype=torch.uint8, device=device)
    state = torch.zeros(9, dtype=torch.float64, device=device)
    log = torch.zeros(LOG, dtype=torch.float64, device=device)
    _m.check(L.mslam_mesh_align_fit_pairs(_m.ptr(p), _m.ptr(c), _m.ptr(wt), n, 1 if with_scale else 0, _m.ptr(ws), wb,
                                          _m.ptr(state), _m.ptr(log), st), "mesh_align_fit_pairs")
    T64 = torch.empty(8, dtype=torch.float64, device=device)
    T32 = torch.empty(8, dtype=torch.float32, device=device)
    status = torch.full((1,), -5, dtype=torch.int32, device=device)
    _m.check(L.mslam_mesh_align_read(_m.ptr(state), _m.ptr(T64), _m.ptr(T32), _m.ptr(status), st), "mesh_align_read")
    return dict(T=T64.cpu().numpy(), T32=T32.cpu().numpy(), status=int(status), log=log.cpu().numpy()[None],
                T_before=A.init_state())


@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("kind", ["generic", "coplanar", "weighted"])
def test_fit_sim3(device, kind, offset):
    """Measured on MI355X: sums at most 0.004 of the bound; the solve within 3.1e-12 of numpy's at 1000 m (the
    translation) and 2.8e-15 at the origin."""
    from mast3r_slam.tsdf import fit_sim3

    for n in (3, BLOCK, BLOCK + 1):
        P, C, w = pair_case(kind, seed=n, n=n, offset=offset)
        if kind == "weighted" and n == 3:
            w[:] = [0.5, 1.5, 1.0]
        for with_scale in (True, False):
            r = _fit_raw(device, P, C, w, with_scale)
            want_T, want_status, want_sums, want_rmse = A.fit_pairs(P, C, w, with_scale)
            p64, c64 = P.astype(np.float64), C.astype(np.float64)
            ww = np.ones(n) if w is None else w.astype(np.float64)
            d = c64 - p64
            terms = A.sum_terms(p64, c64, ww, ww > 0.0, p64[0], c64[0], D._dot(d, d))
            share = _check_sums(r["log"][0], terms, n)
            diff = _check_solve(r, r["log"][0][4:4 + A.N_SUMS], p64[0], c64[0], with_scale)
            assert r["status"] == want_status == A.OK
            assert np.abs(r["T"] - want_T).max() <= SOLVE_TOL          # and the statement from its own sums
            assert abs(r["log"][0][1] - want_rmse) <= n * 2.0 ** -52 * want_rmse
            got = fit_sim3(_dev(device, P, np.float32), _dev(device, C, np.float32),
                           None if w is None else _dev(device, w, np.float32), with_scale=with_scale)
            assert got[0].dtype == torch.float64 and got[1].dtype == torch.float32 and got[0].is_cuda
            assert got[0].cpu().numpy().tobytes() == r["T"].tobytes()
            assert got[1].cpu().numpy().tobytes() == r["T32"].tobytes()
            assert abs(np.linalg.det(A.quat_to_mat(r["T"][3:7])) - 1.0) <= 1e-14
            if not with_scale:
                assert r["T"][7] == 1.0
        print(f"{kind} offset={offset} n={n}: sums at {share:.3f} of the bound, solve within {diff:.2e}")
    if kind != "weighted" and offset == 0.0:
        # exact data: the known Sim3 comes back to the rounding of dst (2^-24 of coordinates below 8)
        rng = np.random.default_rng(9)
        P = rng.normal(size=(BLOCK + 1, 3)).astype(np.float32)
        if kind == "coplanar":
            P[:, 2] = np.float32(0.5)
        truth = A.sim3_from((121.0, (0.3, 1.0, -2.0)), (0.5, -0.25, 1.0), 1.3)
        C = A.act(truth, P.astype(np.float64)).astype(np.float32)
        got = fit_sim3(_dev(device, P, np.float32), _dev(device, C, np.float32))[0].cpu().numpy()
        assert max(A.sim3_error(got, truth)) <= 8.0 * 2.0 ** -24 * 4.0


def test_fit_sim3_degenerate(device):
    from mast3r_slam.tsdf import fit_sim3

    rng = np.random.default_rng(0)
    P = rng.normal(size=(5, 3)).astype(np.float32)
    C = (2.0 * P + 1.0).astype(np.float32)
    ident = A.init_state()
    cases = [(P[:n], C[:n], None, True) for n in (0, 1, 2)]
    cases += [(np.repeat(P[:1], 5, 0), C, None, True), (P, np.repeat(C[:1], 5, 0), None, True),
              (P, C, np.zeros(5, np.float32), True), (P, C, np.array([1, 1, 0, 0, 0], np.float32), True)]
    for src, dst, w, with_scale in cases:
        assert A.fit_pairs(src, dst, w, with_scale)[1] == A.DEGENERATE
        r = _fit_raw(device, src, dst, w, with_scale)
        assert r["status"] == A.DEGENERATE and np.array_equal(r["T"], ident) and r["log"][0][3] == A.DEGENERATE
        assert r["log"][0][0] == (len(src) if w is None else (w > 0).sum())
        with pytest.raises(ValueError, match="degenerate"):
            fit_sim3(_dev(device, src, np.float32).reshape(-1, 3), _dev(device, dst, np.float32).reshape(-1, 3),
                     None if w is None else _dev(device, w, np.float32))
    r = _fit_raw(device, P, np.repeat(C[:1], 5, 0), None, False)           # defined without scale
    assert r["status"] == A.OK and r["T"][7] == 1.0
    with pytest.raises(ValueError, match="differ in shape"):
        fit_sim3(_dev(device, P, np.float32), _dev(device, C[:4], np.float32))
    with pytest.raises(ValueError, match="weights must be"):
        fit_sim3(_dev(device, P, np.float32), _dev(device, C, np.float32), _dev(device, np.ones(4), np.float32))
    with pytest.raises(RuntimeError, match="dtype"):
        fit_sim3(_dev(device, P, np.float32), _dev(device, C, np.float32), _dev(device, np.ones(5), np.float64))


# ----------------------------------------------------------------------------------------------------------------------
# 5. ICP end to end
# ----------------------------------------------------------------------------------------------------------------------
def _case_on_device(device, name):
    (sv, sf), (tv, tf), truth = A.recovery_case(name)
    return ((_dev(device, sv, np.float32), _dev(device, sf, np.int32)),
            (_dev(device, tv, np.float32), _dev(device, tf, np.int32)), truth)


@pytest.mark.parametrize("name", ["small", "mid"])
def test_align_meshes_recovers_a_known_sim3(device, name):
    """Measured on MI355X: the device ends where the numpy statement ends on the same samples, to the three digits
    printed: small 2.45e-8 rad / 4.8e-7 m / 4.93e-8, mid 4.05e-8 rad / 2.12e-6 m / 2.13e-7 from the truth; without scale
    2.8e-8 rad / 3.1e-8 m and 2.2e-8 rad / 1.0e-8 m."""
    from mast3r_slam.tsdf import align_meshes, sample_mesh

    pred, gt, truth = _case_on_device(device, name)
    kw = dict(n_samples=A.RECOVERY_N, max_iters=A.RECOVERY_ITERS, trim=A.RECOVERY_TRIM, seed=0)
    res = align_meshes(pred, gt, tol=0.0, **kw)
    assert sorted(res) == ["T", "converged", "history", "inliers", "iterations", "rmse"]
    assert res["T"].dtype == torch.float64 and res["T"].is_cuda and res["history"].shape == (A.RECOVERY_ITERS, 4)
    assert res["iterations"] == A.RECOVERY_ITERS and not res["converged"]
    assert res["rmse"] == res["history"][-1, 1] and res["inliers"] == res["history"][-1, 0] == A.RECOVERY_N
    P = sample_mesh(*pred, A.RECOVERY_N, seed=0)[0].cpu().numpy()
    T_np, hist_np = recovery_run(name, P)
    err, err_np = A.sim3_error(res["T"].cpu().numpy(), truth), A.sim3_error(T_np, truth)
    print(f"{name}: device (rad, m, scale) " + " ".join(f"{e:.3g}" for e in err) + "; numpy on the same samples "
          + " ".join(f"{e:.3g}" for e in err_np) + f"; final rmse {res['rmse']:.3g} / {hist_np[-1, 1]:.3g}")
    assert all(e <= 10.0 * e_np for e, e_np in zip(err, err_np))
    assert np.array_equal(res["history"][:, 0], hist_np[:, 0])               # the same inliers all the way
    # converged / iterations against tol and check_every, from the history itself
    for check_every in (5, 7):
        tol = 0.2
        res = align_meshes(pred, gt, tol=tol, check_every=check_every, **kw)
        h, it = res["history"], res["iterations"]
        assert res["converged"] and it % check_every == 0 and it < A.RECOVERY_ITERS and len(h) == it
        change = np.abs(np.diff(h[:, 1])) / h[:-1, 1]
        assert change[it - 2] <= tol
        assert all(change[k - 2] > tol for k in range(check_every, it, check_every))
    # without scale on a scale-1 offset
    (sv, sf), (tv, tf), _ = A.recovery_case(name)
    rigid = truth.copy()
    rigid[7] = 1.0
    src = A.act(A.sim3_inv(rigid), A.act(truth, sv.astype(np.float64))).astype(np.float32)
    res = align_meshes((_dev(device, src, np.float32), pred[1]), gt, tol=0.0, with_scale=False, **kw)
    P = sample_mesh(_dev(device, src, np.float32), pred[1], A.RECOVERY_N, seed=0)[0].cpu().numpy()
    T_np = A.icp(P, tv, tf, None, A.RECOVERY_ITERS, A.RECOVERY_TRIM, False)[0]
    err, err_np = A.sim3_error(res["T"].cpu().numpy(), rigid), A.sim3_error(T_np, rigid)
    print(f"{name} without scale: device " + " ".join(f"{e:.3g}" for e in err) + "; numpy "
          + " ".join(f"{e:.3g}" for e in err_np))
    assert float(res["T"][7]) == 1.0 and (res["history"][:, 2] == 1.0).all()
    assert all(e <= 10.0 * e_np for e, e_np in zip(err[:2], err_np[:2]))


def test_align_meshes_trim_sequence_and_init(device):
    from mast3r_slam.tsdf import align_meshes

    pred, gt, truth = _case_on_device(device, "small")
    kw = dict(n_samples=A.RECOVERY_N, max_iters=10, seed=0, tol=0.0, check_every=5)
    const = align_meshes(pred, gt, trim=0.25, **kw)
    seq = align_meshes(pred, gt, trim=[0.25] * 3 + [0.1] * 2 + [1e-9] * 5, **kw)
    h, g = seq["history"], const["history"]
    assert np.array_equal(h[:3], g[:3])                                # the same trim: the same bytes
    assert h[3, 0] < g[3, 0]                                           # a tighter one: fewer pairs
    assert seq["iterations"] == 10 and not seq["converged"]
    assert (h[5:, 3] == A.DEGENERATE).all() and (h[5:, 0] < 3).all()   # none within a nanometre: the state stays
    assert (h[5:, 2] == h[4, 2]).all()
    stop = align_meshes(pred, gt, trim=[0.25] * 3 + [1e-9] * 7, **kw)
    assert stop["iterations"] == 5 and not stop["converged"] and stop["history"][4, 3] == A.DEGENERATE
    # from the truth nothing is left to do: one check and done
    res = align_meshes(pred, gt, init=truth, trim=0.25, n_samples=A.RECOVERY_N, max_iters=10, tol=1.0, check_every=2)
    assert res["iterations"] == 2 and res["rmse"] <= 1e-6 and max(A.sim3_error(res["T"].cpu().numpy(), truth)) <= 1e-6
    assert res["inliers"] == A.RECOVERY_N


# ----------------------------------------------------------------------------------------------------------------------
# 6. guarded buffers and refused arguments
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, BLOCK + 1])
def test_guarded_buffers(device, n):
    P, V, F = align_case(TILE + 1, BLOCK + 1)
    for count in (False, True):
        r = _step(device, P[:n], V, F, trim=0.5, guard=True, count=count, steps=2)
        g = {k: b for k, b in r["guards"].items() if not k.endswith("_t")}
        # all of the workspace is written; `closest` holds NaN too, so only its guards are looked at
        check_guards(g, ("state", "nearest", "moved", "dist2", "log", "ws"), f"mesh_align_step count={count}")
    _m, L, st = _lib()
    p, c = _dev(device, P[:n], np.float32), _dev(device, P[:n] * 2, np.float32)
    wb = int(L.mslam_mesh_align_workspace_bytes(n, 0, 0))
    ws, state, log = (Guarded(device, torch.float64, (k,)) for k in (wb // 8, 9, LOG))
    _m.check(L.mslam_mesh_align_fit_pairs(_m.ptr(p), _m.ptr(c), 0, n, 1, _m.ptr(ws.t), wb, _m.ptr(state.t),
                                          _m.ptr(log.t), st), "mesh_align_fit_pairs")
    T64, T32 = Guarded(device, torch.float64, (8,)), Guarded(device, torch.float32, (8,))
    status = Guarded(device, torch.int32, (1,))
    _m.check(L.mslam_mesh_align_read(_m.ptr(state.t), _m.ptr(T64.t), _m.ptr(T32.t), _m.ptr(status.t), st), "read")
    bufs = dict(ws=ws, state=state, log=log, T64=T64, T32=T32, status=status)
    check_guards(bufs, list(bufs), "mesh_align_fit_pairs, mesh_align_read")


def test_refused_arguments(device):
    _m, L, st = _lib()
    P, V, F = align_case(TILE + 1, BLOCK + 1)
    n, nf, nv = len(P), len(F), len(V)
    p, v, f = _dev(device, P, np.float32), _dev(device, V, np.float32), _dev(device, F, np.int32)
    wb = int(L.mslam_mesh_align_workspace_bytes(n, nf, 0))
    ws = torch.zeros(wb, dtype=torch.uint8, device=device)
    state = torch.zeros(9, dtype=torch.float64, device=device)
    near = torch.full((n,), -1, dtype=torch.int32, device=device)
    moved = torch.zeros((n, 3), dtype=torch.float32, device=device)
    d2 = torch.zeros(n, dtype=torch.float64, device=device)
    log = torch.zeros(LOG, dtype=torch.float64, device=device)
    P_ = _m.ptr
    assert L.mslam_mesh_align_workspace_bytes(-1, 5, 0) == 0 and L.mslam_mesh_align_workspace_bytes(5, -1, 0) == 0
    assert L.mslam_mesh_align_init(0, P_(v), P_(f), nf, nv, P_(ws), wb, P_(state), st) == 0
    step = lambda **k: L.mslam_mesh_align_step(*[k.get(a, d) for a, d in (
        ("src", P_(p)), ("n", n), ("v", P_(v)), ("f", P_(f)), ("nf", nf), ("nv", nv), ("trim", 0.5), ("scale", 1),
        ("count", 0), ("ws", P_(ws)), ("wb", wb), ("state", P_(state)), ("near", P_(near)), ("moved", P_(moved)),
        ("d2", P_(d2)), ("closest", 0), ("log", P_(log)), ("st", st))])
    assert step() == 0                                                        # closest may be NULL
    short = step(wb=wb - 1)
    assert short == -3 and f"{wb} needed" in L.mslam_last_error().decode()   # MSLAM_ENOMEM, with the size
    assert step(count=1) == -3                                                # the counters need room of their own
    for bad in (dict(n=-1), dict(nf=-1), dict(nv=-1), dict(trim=-0.1), dict(trim=float("nan")), dict(src=0),
                dict(near=0), dict(moved=0), dict(d2=0), dict(ws=0), dict(state=0), dict(log=0), dict(f=0), dict(v=0)):
        assert step(**bad) == -1, bad                                         # MSLAM_EINVAL, nothing launched
    assert L.mslam_mesh_align_init(0, P_(v), P_(f), nf, nv, P_(ws), 47, P_(state), st) == -3
    for args in ((0, P_(v), P_(f), -1, nv, P_(ws), wb, P_(state), st), (0, P_(v), P_(f), nf, nv, P_(ws), wb, 0, st),
                 (0, P_(v), 0, nf, nv, P_(ws), wb, P_(state), st), (0, 0, P_(f), nf, nv, P_(ws), wb, P_(state), st),
                 (0, P_(v), P_(f), nf, nv, 0, wb, P_(state), st)):
        assert L.mslam_mesh_align_init(*args) == -1, args
    fit = lambda **k: L.mslam_mesh_align_fit_pairs(*[k.get(a, d) for a, d in (
        ("src", P_(p)), ("dst", P_(moved)), ("w", 0), ("n", n), ("scale", 1), ("ws", P_(ws)), ("wb", wb),
        ("state", P_(state)), ("log", P_(log)), ("st", st))])
    assert fit() == 0
    assert fit(wb=8) == -3
    for bad in (dict(n=-1), dict(src=0), dict(dst=0), dict(ws=0), dict(state=0), dict(log=0)):
        assert fit(**bad) == -1, bad
    assert L.mslam_mesh_align_read(0, 0, 0, 0, st) == -1
    assert L.mslam_mesh_align_read(P_(state), 0, 0, 0, st) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# 7. compare_meshes(align=...)
# ----------------------------------------------------------------------------------------------------------------------
def test_compare_meshes_align(device):
    from mast3r_slam.tsdf import compare_meshes, transform_mesh

    pred, gt, truth = _case_on_device(device, "small")
    n, th = 4001, 0.02
    plain = compare_meshes(pred, gt, n_samples=n, threshold=th)
    assert compare_meshes(pred, gt, n_samples=n, threshold=th, align=None) == plain
    assert sorted(plain) == sorted(D.metrics([1.0], [1.0], th, 1.0, 1.0))               # the keys of before
    moved = (transform_mesh(pred[0], truth), pred[1])
    in_frame = compare_meshes(moved, gt, n_samples=n, threshold=th)
    given = compare_meshes(pred, gt, n_samples=n, threshold=th, align=truth)
    assert given.pop("alignment") == dict(T=[float(x) for x in truth], rmse=None, iterations=None)
    assert given == in_frame
    normals = torch.zeros_like(pred[0])
    assert compare_meshes((pred[0], normals, pred[1]), gt, n_samples=n, threshold=th,
                          align=torch.from_numpy(truth)).pop("accuracy") == in_frame["accuracy"]
    # the source is a part of the room itself: in frame it lies on the target to f32 rounding
    assert in_frame["accuracy"] <= 1e-6 and in_frame["precision"] == 1.0 and plain["accuracy"] > 0.01
    icp = compare_meshes(pred, gt, n_samples=n, threshold=th, align="icp",
                         align_kw=dict(n_samples=A.RECOVERY_N, max_iters=A.RECOVERY_ITERS, trim=A.RECOVERY_TRIM, tol=0.0))
    al = icp.pop("alignment")
    assert sorted(al) == ["T", "iterations", "rmse"] and al["iterations"] == A.RECOVERY_ITERS and len(al["T"]) == 8
    # Every sample moves by at most the displacement between the two transforms over the mesh, and the distance to a
    # mesh is 1-Lipschitz in both the sample and the mesh: with the CPU test's bounds on the recovery (10x what the
    # statement reaches: 2.5e-7 rad and 4.9e-7 in scale over a radius below 4 m, 4.8e-6 m) that is below 1e-5 m.
    margin = 1e-5
    err = A.sim3_error(np.array(al["T"]), truth)
    print(f"icp against the truth: {err}; accuracy {icp['accuracy']:.3g} / {in_frame['accuracy']:.3g}, completion "
          f"{icp['completion']:.6g} / {in_frame['completion']:.6g}")
    for key in ("accuracy", "accuracy_median", "completion", "completion_median"):
        assert abs(icp[key] - in_frame[key]) <= margin, key
    assert icp["precision"] == in_frame["precision"] == 1.0
    assert abs(icp["recall"] - in_frame["recall"]) <= 2.0 / n            # a sample at the threshold may change sides
    assert abs(icp["pred_area"] - in_frame["pred_area"]) <= 1e-5 * in_frame["pred_area"]


# ----------------------------------------------------------------------------------------------------------------------
# 8. the product: a run scored against a ground truth in another frame
# ----------------------------------------------------------------------------------------------------------------------
def test_trajectory_ate(device):
    from mast3r_slam import evaluate

    rng = np.random.default_rng(4)
    est = rng.normal(size=(40, 3)).astype(np.float32)
    move = A.sim3_from((50.0, (1.0, 1.0, -0.3)), (0.4, 2.0, -1.0), 2.5)
    gt = A.act(move, est.astype(np.float64))
    rmse, T = evaluate.trajectory_ate(est, gt.astype(np.float32))
    assert T.shape == (8,) and T.dtype == np.float64
    assert rmse <= 4.0 * 2.0 ** -24 * np.abs(gt).max() and max(A.sim3_error(T, move)) <= 1e-6
    rigid = move.copy()
    rigid[7] = 1.0
    rmse, T = evaluate.trajectory_ate(torch.from_numpy(est), A.act(rigid, est.astype(np.float64)), with_scale=False)
    assert rmse <= 4.0 * 2.0 ** -24 * np.abs(gt).max() and T[7] == 1.0
    # by hand: a square in the plane z = 0 whose corners are lifted by +d, +d, -d, -d.  The lift is orthogonal to every
    # translation, rotation and scaling of the square (sum sigma_k p_k = 0), so the best similarity is the identity and
    # the error is d at every corner; moved by `move`, it is scale * d.
    d = 0.125
    sq = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], np.float64)
    lifted = sq + d * np.array([1, 1, -1, -1])[:, None] * np.array([0, 0, 1.0])
    for with_scale, M, want in ((True, move, 2.5 * d), (False, rigid, d)):
        rmse, T = evaluate.trajectory_ate(sq, A.act(M, lifted), with_scale=with_scale)
        assert abs(rmse - want) <= 1e-5 * want and max(A.sim3_error(T, M)) <= 2e-6      # f32 inputs: 2.4e-7 a coordinate


def test_slam_system_evaluate_mesh_aligned(device, monkeypatch):
    """The run of test_mesh_metrics_gpu.test_slam_system_evaluate_mesh, scored against the room moved by a known Sim3
    `move`: align_trajectory recovers it from the keyframes' centres, ICP from there, and the figures in the moved frame
    are the in-frame ones times the scale.  Measured on MI355X (DESIGN.md "Mesh alignment"): 3 keyframes, align_trajectory
    2e-7 rad / 5e-8 m / 5e-8 from the truth; accuracy in frame 4.083 mm, by the trajectory's transform 4.083 mm, after
    ICP 3.230 mm, 2.1 mrad / 5.2 mm / 0.24 % from the truth; precision 1.0000 in all three."""
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from test_slam_system_gpu import RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    move = A.sim3_from((25.0, (0.2, 1.0, 0.1)), (2.0, -1.0, 0.5), 1.6)
    rv, rf = synthetic.room_mesh()
    gv = A.act(move, rv.astype(np.float64)).astype(np.float32)
    n = 20000
    try:
        system.run(_frames(list(range(0, 60, 3)), device))
        in_frame = system.evaluate_mesh(rv, rf, n_samples=n, threshold=VS)
        centres = np.stack([system.keyframes[i].T_WC.data.reshape(8)[:3].cpu().numpy()
                            for i in range(len(system.keyframes))])
        gt_pos = A.act(move, centres.astype(np.float64)).astype(np.float32)
        T_traj = system.align_trajectory(gt_pos).cpu().numpy()
        by_traj = system.evaluate_mesh(gv, rf, n_samples=n, threshold=VS * move[7], align=T_traj)
        icp = system.evaluate_mesh(gv, rf, n_samples=n, threshold=VS * move[7], align="icp", init="trajectory",
                                   gt_positions=gt_pos, align_kw=dict(trim=0.12 * move[7]))
        with pytest.raises(ValueError, match="gt_positions"):
            system.evaluate_mesh(gv, rf, align="icp", init="trajectory")
        with pytest.raises(ValueError, match="ground-truth positions"):
            system.align_trajectory(gt_pos[:-1])
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    assert len(centres) >= 3
    err = A.sim3_error(T_traj, move)
    s = move[7]
    print(f"{len(centres)} keyframes; align_trajectory against the truth (rad, m, scale): {err}")
    print(f"in frame: accuracy {in_frame['accuracy']:.6f} precision {in_frame['precision']:.4f}; by trajectory: "
          f"{by_traj['accuracy'] / s:.6f} {by_traj['precision']:.4f}; icp from there: {icp['accuracy'] / s:.6f} "
          f"{icp['precision']:.4f}, {icp['alignment']['iterations']} iterations, rmse {icp['alignment']['rmse'] / s:.6f}, "
          f"icp against the truth {A.sim3_error(np.array(icp['alignment']['T']), move)}")
    # f32 centres a few metres from the origin, rounded once more after the move: 2^-24 * 8 m = 5e-7 m each, over a
    # trajectory about 2 m across
    assert max(err) <= 5e-6
    # with the trajectory's transform the mesh is in the truth's frame to those 5e-6 m: the in-frame figures, scaled
    assert abs(by_traj["accuracy"] / s - in_frame["accuracy"]) <= 1e-5
    assert abs(by_traj["precision"] - in_frame["precision"]) <= 2.0 / n
    # ICP then minimises the distance of the mesh's own 4 mm of reconstruction error over seven parameters: it may
    # only come closer, and by no more than that error itself (margin: DESIGN.md "Mesh alignment")
    assert icp["accuracy"] / s <= in_frame["accuracy"] + 1e-4
    assert icp["accuracy"] / s >= 0.5 * in_frame["accuracy"]
    assert icp["precision"] >= in_frame["precision"] - 1e-3
    t_err, s_err = A.sim3_error(np.array(icp["alignment"]["T"]), move)[1:]
    assert t_err <= 2.0 * in_frame["accuracy"] * s and s_err * 1.0 <= 2.0 * in_frame["accuracy"] * s
