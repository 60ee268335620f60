"""GPU tests (-m gpu) of point-to-plane ICP (csrc/icp_plane.hip, align_clouds / align_meshes with metric="plane";
DESIGN.md "Point-to-plane ICP") against the numpy statement tests/icp_plane_numpy.py: every iteration's moved samples,
pairs, sums and solve; the block, tile and group edges in the plain and the two indexed forms; the traps of
tests/test_icp_plane_cpu.py; the recovery cases end to end; refusals; the product.  Every operand of the raw C entry
points lies in a guarded buffer (tests/kernel_refs.py), and the guards are checked after every run."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_numpy as C  # noqa: E402
import icp_plane_numpy as IP  # noqa: E402
import meshalign_numpy as A  # noqa: E402
from mesh_support import BLOCK, G, T, VS, Operands, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES_SAMPLES = (1, BLOCK - 1, BLOCK, BLOCK + 1)
SIZES_POINTS = (1, T - 1, T, T + 1, T * G + 1)          # 4 097: the first size with a second group of 32 tiles
SIZES_FACES = (1, T, T + 1)
MODES = ("plain", 1, 2)                                  # no index; the tile boxes alone; tiles and groups
INF = math.inf
EINVAL, ENOMEM = -1, -3                                 # MSLAM_EINVAL, MSLAM_ENOMEM of include/mslam_hip.h


def _lib():
    import mslam_hip as _m

    return _m, _m.lib(), _m.stream_ptr()


def _run(device, src, target, T0=None, trims=(INF,), alpha=0.0, with_scale=True, mode="plain", warm=None):
    """`len(trims)` iterations through the C entry points, every operand guarded -> a list of dicts per iteration:
    T_before, T, status, moved, dist2, nearest, closest, log.  target: ("cloud", points, normals) or ("mesh", vertices,
    faces); mode: "plain", or the `levels` of the indexed form (a mesh index always has both levels)."""
    from mast3r_slam.tsdf import CloudIndex, MeshIndex

    _m, L, st = _lib()
    kind, x, y = target
    ops = Operands(device)
    src = C.f32(src)
    n = len(src)
    s = ops.put(src, np.float32)
    t0 = None if T0 is None else ops.put(np.asarray(T0, np.float32), np.float32)
    state = ops.out(torch.float64, (9,))
    T64, status = ops.out(torch.float64, (8,)), ops.out(torch.int32, (1,))
    log = ops.out(torch.float64, (len(trims), IP.LOG))
    nearest = ops.put(np.full(n, -1, np.int32) if warm is None else warm, np.int32)
    moved, dist2 = ops.out(torch.float32, (n, 3)), ops.out(torch.float64, (n,))
    closest = ops.out(torch.float64, (n, 3))
    indexed = mode != "plain"
    if kind == "cloud":
        p, nrm = ops.put(C.f32(x), np.float32), ops.put(C.f32(y), np.float32)
        N = len(p)
        boxed = 0
        if indexed:
            ix = CloudIndex(p)
    else:
        v, f = ops.put(np.reshape(x, (-1, 3)), np.float32), ops.put(np.reshape(y, (-1, 3)), np.int32)
        nv, nf = len(v), len(f)
        boxed = 0 if indexed else nf
        if indexed:
            ix = MeshIndex(v, f, validate=False)                   # the traps hold faces with indices out of range
    if indexed:
        order = ops.put(ix.order.cpu().numpy(), np.int32)
        iws = ops.put(ix.ws.cpu().numpy(), np.uint8) if ix.ws is not None else None
        iws_bytes = ix.ws_bytes
    need = int(L.mslam_icp_plane_workspace_bytes(n, boxed))
    assert need == 48 * ((boxed + T - 1) // T) + 8 * IP.N_SUMS * ((n + BLOCK - 1) // BLOCK)
    ws = ops.out(torch.float64, (need // 8,))
    if kind == "mesh" and not indexed:
        _m.check(L.mslam_mesh_align_init(_m.ptr(t0), _m.ptr(v), _m.ptr(f), nf, nv, _m.ptr(ws), need, _m.ptr(state), st),
                 "mesh_align_init")
    else:
        _m.check(L.mslam_mesh_align_init_indexed(_m.ptr(t0), _m.ptr(state), st), "mesh_align_init_indexed")

    def read():
        _m.check(L.mslam_mesh_align_read(_m.ptr(state), _m.ptr(T64), 0, _m.ptr(status), st), "mesh_align_read")
        return T64.cpu().numpy(), int(status.cpu()[0])

    out = []
    tail = (_m.ptr(ws), need, _m.ptr(state), _m.ptr(nearest), _m.ptr(moved), _m.ptr(dist2), _m.ptr(closest))
    for it, trim in enumerate(trims):
        T_before = read()[0]
        head = (_m.ptr(s), n)
        mid = (float(trim), float(alpha), 1 if with_scale else 0)
        if kind == "cloud":
            rc = L.mslam_icp_plane_step_cloud(*head, _m.ptr(p), _m.ptr(nrm), N, *((_m.ptr(order), _m.ptr(iws), iws_bytes,
                                              mode) if indexed else (0, 0, 0, 1)), *mid, *tail, _m.ptr(log[it]), st)
        elif indexed:
            rc = L.mslam_icp_plane_step_mesh_indexed(*head, _m.ptr(v), _m.ptr(f), nf, nv, _m.ptr(order), _m.ptr(iws),
                                                     iws_bytes, *mid, *tail, _m.ptr(log[it]), st)
        else:
            rc = L.mslam_icp_plane_step_mesh(*head, _m.ptr(v), _m.ptr(f), nf, nv, *mid, *tail, _m.ptr(log[it]), st)
        _m.check(rc, "icp_plane_step")
        T_after, stat = read()
        out.append(dict(T_before=T_before, T=T_after, status=stat, moved=moved.cpu().numpy(),
                        dist2=dist2.cpu().numpy(), nearest=nearest.cpu().numpy(), closest=closest.cpu().numpy(),
                        log=log[it].cpu().numpy()))
    ops.check()
    return out


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _check_iteration(tr, src, target, trim=INF, alpha=0.0, with_scale=True):
    """One iteration of _run against the statement (the docstring of the module).  Returns the largest error of a sum
    as a share of its bound and of the state as a share of its bound."""
    src = C.f32(src)
    n = len(src)
    want_q = A.act(tr["T_before"], src.astype(np.float64))
    assert (np.abs(tr["moved"].astype(np.float64) - want_q) <= _ulp32(want_q))[np.isfinite(want_q)].all()
    sums = tr["log"][6:]
    st = IP.step(tr["T_before"], src, target, trim, with_scale, alpha, moved=tr["moved"], sums=sums)
    assert tr["nearest"].tobytes() == st["nearest"].tobytes() and tr["dist2"].tobytes() == st["dist2"].tobytes()
    assert np.allclose(tr["closest"], st["closest"], rtol=0.0, atol=1e-12, equal_nan=True)
    assert tr["log"][0] == int(st["inlier"].sum())
    worst_sum = 0.0
    for k in range(IP.N_SUMS):
        exact = math.fsum(st["terms"][:, k])
        bound = n * 2.0 ** -52 * math.fsum(np.abs(st["terms"][:, k]))
        err = abs(sums[k] - exact)
        assert err <= bound, (k, sums[k], exact, bound)
        worst_sum = max(worst_sum, err / bound if bound > 0.0 else 0.0)
    # the new state: the statement's solve of the device's own sums
    assert tr["status"] == st["status"]
    worst_state = 0.0
    if st["status"] == IP.DEGENERATE:
        assert np.array_equal(tr["T"], tr["T_before"])
    else:
        nu = 7 if with_scale else 6
        H = IP.h_matrix(sums)[:nu, :nu]
        d = 1.0 / np.sqrt(np.diag(H))
        kappa = np.linalg.cond(H * d[:, None] * d[None, :])
        bound = max(16.0 * kappa * 2.0 ** -52 * float(np.linalg.norm(st["xi"])), float(np.spacing(np.abs(st["T"]).max())))
        diff = float(np.abs(tr["T"] - st["T"]).max())
        assert diff <= bound, (diff, bound, kappa)
        worst_state = diff / bound
        if not with_scale:
            assert tr["T"][7] == tr["T_before"][7]
    want_log = st["log"][:6]
    assert tr["log"][0] == want_log[0] and tr["log"][2] == tr["T"][7] and tr["log"][3] == tr["status"]
    for k in (1, 4, 5):                                          # sqrt and / are correctly rounded: a few ulps at most
        assert tr["log"][k] == want_log[k] or abs(tr["log"][k] - want_log[k]) <= 4.0 * np.spacing(abs(want_log[k])), k
    return worst_sum, worst_state


def _same_runs(a, b):
    for x, y in zip(a, b):
        for k in ("T", "moved", "dist2", "nearest", "closest", "log"):
            assert x[k].tobytes() == y[k].tobytes(), k
        assert x["status"] == y["status"]


# ----------------------------------------------------------------------------------------------------------------------
# fixtures on the box and the recovery meshes
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def box_target(N):
    """(points, normals at k = 16) of N points of the box cloud (seed 0), in a shuffled order."""
    P = IP.box_cloud(0, 6000)
    P = P[np.random.default_rng(N).permutation(len(P))[:N]]
    return P, IP.knn_normals(P)


@functools.lru_cache(maxsize=None)
def box_samples():
    pred = IP.box_case()[0]
    return C.stride_sample(pred, max(SIZES_SAMPLES))[0]


T0_BOX = np.array([0.02, -0.01, 0.01, 0.0, 0.0, 0.0, 1.0, 0.97], np.float32)   # part of the way to BOX_MOVE


@functools.lru_cache(maxsize=None)
def mesh_case():
    """(1 025 samples of the "small" source, its target mesh)."""
    from test_icp_plane_cpu import recovery_samples

    _, (tv, tf), _ = A.recovery_case("small")
    return recovery_samples("small"), tv, tf


def _every(P, n):
    """n of the samples P, spread over all of them: sample_mesh orders its samples by face."""
    return P[(np.arange(n) * len(P)) // n]


# ----------------------------------------------------------------------------------------------------------------------
# every iteration against the statement
# ----------------------------------------------------------------------------------------------------------------------
def test_cloud_iterations_against_the_statement(device):
    """The box case, 500 samples, six iterations through the raw entry points, plain scan."""
    pred, gt, nrm, src = IP.box_case()
    target = ("cloud", gt, nrm)
    runs = _run(device, src, target, trims=(INF,) * 6)
    worst = [max(w) for w in zip(*(_check_iteration(tr, src, target) for tr in runs))]
    hist = IP.icp(src, target, None, 6)[1]
    assert [tr["log"][0] for tr in runs] == list(hist[:, 0])
    print(f"box: sums within {worst[0]:.2g} of their bound, states within {worst[1]:.2g}; final error "
          + " / ".join(f"{e:.2g}" for e in A.sim3_error(runs[-1]["T"], IP.BOX_MOVE)))
    for mode in (1, 2):
        _same_runs(_run(device, src, target, trims=(INF,) * 6, mode=mode), runs)
    # with a point weight
    runs = _run(device, src, target, trims=(INF,) * 3, alpha=0.05)
    for tr in runs:
        _check_iteration(tr, src, target, alpha=0.05)


def test_mesh_iterations_against_the_statement(device):
    """The "small" recovery case, 1 025 samples, five iterations, trim 0.25: plain and over a mesh index."""
    P, tv, tf = mesh_case()
    target = ("mesh", tv, tf)
    trims = (A.RECOVERY_TRIM,) * 5
    runs = _run(device, P, target, trims=trims)
    worst = [max(w) for w in zip(*(_check_iteration(tr, P, target, A.RECOVERY_TRIM) for tr in runs))]
    hist = IP.icp(P, target, None, 5, A.RECOVERY_TRIM)[1]
    assert [tr["log"][0] for tr in runs] == list(hist[:, 0])
    print(f"mesh: sums within {worst[0]:.2g} of their bound, states within {worst[1]:.2g}")
    _same_runs(_run(device, P, target, trims=trims, mode=2), runs)
    for tr in _run(device, P, target, trims=trims[:2], alpha=0.05, with_scale=False):
        _check_iteration(tr, P, target, A.RECOVERY_TRIM, 0.05, False)


# ----------------------------------------------------------------------------------------------------------------------
# size edges
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES_POINTS)
def test_cloud_size_edges(device, N):
    """Two iterations at every sample count against the statement, and the same bytes in the three forms.  One sample
    is fewer pairs than unknowns: degenerate.  One target point has no normal (fewer than 3 neighbours): no pair."""
    gt, nrm = box_target(N)
    target = ("cloud", gt, nrm)
    for n in SIZES_SAMPLES:
        src = box_samples()[:n]
        runs = _run(device, src, target, T0=T0_BOX, trims=(INF, 0.5))
        for tr, trim in zip(runs, (INF, 0.5)):
            _check_iteration(tr, src, target, trim)
        if n == 1 or N == 1:
            assert all(tr["status"] == IP.DEGENERATE for tr in runs)
        for mode in (1, 2):
            _same_runs(_run(device, src, target, T0=T0_BOX, trims=(INF, 0.5), mode=mode), runs)


@pytest.mark.parametrize("F", SIZES_FACES)
def test_mesh_size_edges(device, F):
    P, tv, tf = mesh_case()
    target = ("mesh", tv, tf[:F])
    for n in SIZES_SAMPLES:
        src = _every(P, n)
        runs = _run(device, src, target, trims=(INF, 0.5))
        for tr, trim in zip(runs, (INF, 0.5)):
            _check_iteration(tr, src, target, trim)
        if n == 1 or F == 1:
            assert all(tr["status"] == IP.DEGENERATE for tr in runs)          # one plane determines three unknowns
        _same_runs(_run(device, src, target, trims=(INF, 0.5), mode=2), runs)


@pytest.mark.parametrize("N", SIZES_POINTS)
def test_align_clouds_forms_give_the_same_bits(device, N):
    """align_clouds(metric="plane") without an index, with index=True and with a given CloudIndex, each twice."""
    from mast3r_slam.tsdf import CloudIndex, align_clouds, cloud_normals

    gt, nrm = box_target(N)
    g, nr = _dev(device, gt, np.float32), _dev(device, nrm, np.float32)
    for n in SIZES_SAMPLES:
        p = _dev(device, box_samples()[:n], np.float32)
        kw = dict(metric="plane", normals=nr, init=T0_BOX, n_samples=n, max_iters=3, tol=0.0, check_every=2)
        first = align_clouds(p, g, **kw)
        assert first["history"].shape[1] == 4 and first["iterations"] in (2, 3)
        assert (n > 1 and N > 1) or first["history"][-1, 3] == IP.DEGENERATE
        for index in (None, True, CloudIndex(g)):
            got = align_clouds(p, g, index=index, **kw)
            assert torch.equal(got["T"], first["T"]) and got["history"].tobytes() == first["history"].tobytes()
            assert got["point_rmse"] == first["point_rmse"] and got["normal_spread"] == first["normal_spread"]
    # normals=k is cloud_normals(gt, k) once before the loop
    own = cloud_normals(g, IP.BOX_K)[0]
    kw = dict(metric="plane", n_samples=BLOCK + 1, max_iters=3, tol=0.0, init=T0_BOX)
    assert torch.equal(align_clouds(p, g, normals=IP.BOX_K, **kw)["T"], align_clouds(p, g, normals=own, **kw)["T"])


@pytest.mark.parametrize("F", SIZES_FACES)
def test_align_meshes_forms_give_the_same_bits(device, F):
    from mast3r_slam.tsdf import MeshIndex, align_meshes

    (sv, sf), (tv, tf), _ = A.recovery_case("small")
    pred = (_dev(device, sv, np.float32), _dev(device, sf, np.int32))
    gt = (_dev(device, tv, np.float32), _dev(device, tf[:F], np.int32))
    for n in SIZES_SAMPLES:
        kw = dict(metric="plane", n_samples=n, max_iters=3, tol=0.0, check_every=2, trim=0.5)
        first = align_meshes(pred, gt, **kw)
        for index in (None, True, MeshIndex(*gt)):
            got = align_meshes(pred, gt, index=index, **kw)
            assert torch.equal(got["T"], first["T"]) and got["history"].tobytes() == first["history"].tobytes()
            assert got["point_rmse"] == first["point_rmse"] and got["normal_spread"] == first["normal_spread"]


# ----------------------------------------------------------------------------------------------------------------------
# traps
# ----------------------------------------------------------------------------------------------------------------------
def test_traps(device):
    pred, gt, nrm, src = IP.box_case()
    src = src[:300]
    # NaN samples and NaN target points have no pair
    holes = src.copy()
    holes[[5, 77, 299]] = np.nan
    g_nan, target = gt.copy(), None
    g_nan[::50] = np.nan
    target = ("cloud", g_nan, nrm)
    for mode in MODES:
        runs = _run(device, holes, target, T0=T0_BOX, trims=(INF, INF), mode=mode)
        for tr in runs:
            _check_iteration(tr, holes, target)
            assert (tr["nearest"][[5, 77, 299]] == -1).all() and (tr["nearest"] % 50 != 0).all()
            assert tr["log"][0] == 297 and tr["status"] == IP.OK
    # a NaN first sample has no origin: every sum is NaN and the state stays
    first = src.copy()
    first[0] = np.nan
    tr = _run(device, first, ("cloud", gt, nrm), T0=T0_BOX)[0]
    assert tr["status"] == IP.DEGENERATE and np.array_equal(tr["T"], tr["T_before"]) and np.isnan(tr["log"][6 + IP.h_index(3, 3)])
    # neighbours without a normal: out without a point weight, in with one
    bad = nrm.copy()
    bad[::3] = 0.0
    bad[1::9] = np.nan
    target = ("cloud", gt, bad)
    counts = []
    for alpha in (0.0, 0.05):
        tr = _run(device, src, target, T0=T0_BOX, alpha=alpha)[0]
        _check_iteration(tr, src, target, alpha=alpha)
        counts.append(tr["log"][0])
    assert counts[0] < counts[1] == 300
    # trim = 0: no pair here; a trim sequence; without scale
    target = ("cloud", gt, nrm)
    tr = _run(device, src, target, T0=T0_BOX, trims=(0.0,))[0]
    _check_iteration(tr, src, target, 0.0)
    assert tr["log"][0] == 0 and tr["status"] == IP.DEGENERATE and np.isposinf(tr["log"][1]) and tr["log"][5] == 0.0
    trims = (0.3, 0.1, 0.05)
    for tr, trim in zip(_run(device, src, target, T0=T0_BOX, trims=trims, with_scale=False), trims):
        _check_iteration(tr, src, target, trim, with_scale=False)
        assert tr["T"][7] == np.float64(T0_BOX[7])
    # a pair at exactly trim counts: the walls of [-1, 1]^3, two points pushed outwards by 0.25 and 0.5
    from test_icp_plane_cpu import BOX, _planes

    walls, wn = _planes(np.random.default_rng(9), 50, BOX)
    far = walls.copy()
    far[270] += np.float32([0, 0, 0.25])
    far[271] += np.float32([0, 0, 0.5])
    target = ("cloud", walls, wn)
    tr = _run(device, far, target, trims=(0.25,))[0]
    _check_iteration(tr, far, target, 0.25)
    assert tr["dist2"][270] == 0.0625 and tr["log"][0] == 299 and tr["status"] == IP.OK


def test_mesh_traps(device):
    """A degenerate face (zero area) through a sample and a face with an index out of range are never the nearest; NaN
    samples have no face; a warm start of any value changes nothing."""
    P, tv, tf = mesh_case()
    P = _every(P, 300).copy()
    P[7] = np.nan
    q = A.act(A.init_state(), P[:1].astype(np.float64))[0].astype(np.float32)
    v = np.concatenate([tv, q[None], q[None] + np.float32([1, 0, 0])])
    nv = len(tv)
    f = np.concatenate([[[nv, nv + 1, nv]], tf[:100], [[0, 1, len(v) + 5]], tf[100:]]).astype(np.int32)
    target = ("mesh", v, f)
    runs = _run(device, P, target, trims=(0.5, 0.5))
    for tr in runs:
        _check_iteration(tr, P, target, 0.5)
        assert tr["nearest"][7] == -1 and not np.isin(tr["nearest"], (0, 101)).any() and tr["status"] == IP.OK
    warm = np.random.default_rng(3).integers(-5, len(f) + 5, len(P)).astype(np.int32)
    _same_runs(_run(device, P, target, trims=(0.5, 0.5), warm=warm), runs)
    _same_runs(_run(device, P, target, trims=(0.5, 0.5), warm=warm, mode=2), runs)


def test_init_at_the_truth_moves_nothing(device):
    from mast3r_slam.tsdf import align_clouds

    pred, gt, nrm, _ = IP.room_case("exact")
    res = align_clouds(_dev(device, pred, np.float32), _dev(device, gt, np.float32), init=IP.BOX_MOVE, n_samples=500,
                       max_iters=1, metric="plane")
    assert max(A.sim3_error(res["T"].cpu().numpy(), IP.BOX_MOVE)) <= 1e-6 and res["point_rmse"] <= 1e-6
    assert sorted(res) == ["T", "converged", "history", "inliers", "iterations", "normal_spread", "point_rmse", "rmse"]


# ----------------------------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------------------------
def test_align_clouds_box_end_to_end(device):
    """Measured on MI355X: the device ends where the statement ends, 6.5e-4 rad / 8.2e-4 m / 7.2e-4 from the truth after
    8 iterations on these 500 samples (the point metric: 1.0e-2 / 4.0e-3 after 30)."""
    from mast3r_slam.tsdf import align_clouds

    pred, gt, nrm, src = IP.box_case()
    p, g = _dev(device, pred, np.float32), _dev(device, gt, np.float32)
    trace = []
    res = align_clouds(p, g, n_samples=IP.BOX_SAMPLES, max_iters=8, tol=0.0, metric="plane", normals=IP.BOX_K,
                       _trace=trace)
    assert res["iterations"] == 8 == len(trace) and res["history"].shape == (8, 4)
    T_np, hist_np, _ = IP.icp(src, ("cloud", gt, nrm), None, 8)
    err, err_np = A.sim3_error(res["T"].cpu().numpy(), IP.BOX_MOVE), A.sim3_error(T_np, IP.BOX_MOVE)
    print("box: device (rad, m, scale) " + " ".join(f"{e:.3g}" for e in err) + "; numpy " + " ".join(
        f"{e:.3g}" for e in err_np) + f"; rms {res['rmse']:.3g}, point rmse {res['point_rmse']:.3g}, normal_spread "
        f"{res['normal_spread']:.3g}")
    assert all(e <= 2.0 * e_np for e, e_np in zip(err, err_np))
    assert np.array_equal(res["history"][:, 0], hist_np[:, 0])
    assert res["rmse"] == res["history"][-1, 1] and res["inliers"] == res["history"][-1, 0]
    last = trace[-1]["log"].cpu().numpy()
    assert res["point_rmse"] == last[4] and res["normal_spread"] == last[5] and abs(last[5] - hist_np[-1, 5]) <= 1e-9
    # the trace holds the iteration's own buffers: the device's normals are the statement's, so are the pairs
    tr = {k: v.cpu().numpy() for k, v in trace[0].items()}
    st = IP.step(tr["T_before"], src, ("cloud", gt, nrm), moved=tr["moved"])
    assert tr["nearest"].tobytes() == st["nearest"].tobytes() and tr["dist2"].tobytes() == st["dist2"].tobytes()
    assert np.array_equal(tr["closest"], st["closest"]) and tr["status"][0] == IP.OK
    # the stop rule is _icp_run's
    got = align_clouds(p, g, n_samples=IP.BOX_SAMPLES, max_iters=20, tol=1e-3, check_every=3, metric="plane")
    assert got["converged"] and got["iterations"] % 3 == 0 and got["iterations"] < 20


@pytest.mark.parametrize("name", ["small", "mid"])
def test_align_meshes_end_to_end(device, name):
    """Six iterations where the point-to-mesh metric takes 80 (tests/test_mesh_align_gpu.py).  Measured on MI355X: the
    device ends where the statement ends on the same samples, to the three digits printed: small 7.69e-9 rad / 1.2e-8 m
    / 3.89e-9, mid 6.65e-9 / 2.64e-8 / 4.15e-9 from the truth (point-to-mesh after 80: 2.45e-8 / 4.8e-7 / 4.93e-8 and
    4.05e-8 / 2.12e-6 / 2.13e-7)."""
    from mast3r_slam.tsdf import align_meshes, sample_mesh

    (sv, sf), (tv, tf), truth = A.recovery_case(name)
    pred = (_dev(device, sv, np.float32), _dev(device, sf, np.int32))
    gt = (_dev(device, tv, np.float32), _dev(device, tf, np.int32))
    trace = []
    res = align_meshes(pred, gt, n_samples=A.RECOVERY_N, max_iters=6, trim=A.RECOVERY_TRIM, seed=0, tol=0.0,
                       metric="plane", _trace=trace)
    P = sample_mesh(*pred, A.RECOVERY_N, seed=0)[0].cpu().numpy()
    T_np, hist_np, _ = IP.icp(P, ("mesh", tv, tf), None, 6, A.RECOVERY_TRIM)
    err, err_np = A.sim3_error(res["T"].cpu().numpy(), truth), A.sim3_error(T_np, truth)
    print(f"{name}: device (rad, m, scale) " + " ".join(f"{e:.3g}" for e in err) + "; numpy on the same samples "
          + " ".join(f"{e:.3g}" for e in err_np) + f"; normal_spread {res['normal_spread']:.3g}")
    assert all(e <= 2.0 * e_np for e, e_np in zip(err, err_np))
    assert np.array_equal(res["history"][:, 0], hist_np[:, 0]) and len(trace) == 6
    assert sorted(res) == ["T", "converged", "history", "inliers", "iterations", "normal_spread", "point_rmse", "rmse"]


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals(device):
    from mast3r_slam.tsdf import align_clouds, align_meshes

    pred, gt, nrm, _ = IP.box_case()
    p, g, nr = _dev(device, pred, np.float32), _dev(device, gt, np.float32), _dev(device, nrm, np.float32)
    (sv, sf), (tv, tf), _ = A.recovery_case("small")
    mp, mg = (_dev(device, sv, np.float32), _dev(device, sf, np.int32)), (_dev(device, tv, np.float32),
                                                                         _dev(device, tf, np.int32))
    for call in (lambda **kw: align_clouds(p, g, **kw), lambda **kw: align_meshes(mp, mg, **kw)):
        with pytest.raises(ValueError, match="metric must be"):
            call(metric="planes")
        with pytest.raises(ValueError, match="point_weight goes with"):
            call(point_weight=0.05)
        with pytest.raises(ValueError, match="point_weight must be"):
            call(metric="plane", point_weight=-1.0)
        with pytest.raises(ValueError, match="point_weight must be"):
            call(metric="plane", point_weight=math.nan)
    with pytest.raises(ValueError, match="normals must be gt's"):
        align_clouds(p, g, metric="plane", normals=nr[:-1])
    with pytest.raises(RuntimeError, match="normals must have dtype"):
        align_clouds(p, g, metric="plane", normals=nr.to(torch.float64))
    with pytest.raises(RuntimeError, match="device tensors only"):
        align_clouds(p, g, metric="plane", normals=nr.cpu())
    for k in (0, 33, 2.5, True):
        with pytest.raises(ValueError, match="normals must be an integer"):
            align_clouds(p, g, metric="plane", normals=k)
    # the entry points themselves
    _m, L, st = _lib()
    n, N = 10, len(gt)
    ops = Operands(device)
    s = ops.put(pred[:n], np.float32)
    state, log = ops.put(np.zeros(9), np.float64), ops.put(np.zeros(IP.LOG), np.float64)
    near, moved, d2 = ops.put(np.zeros(n), np.int32), ops.put(np.zeros((n, 3)), np.float32), ops.put(np.zeros(n), np.float64)
    ws = ops.put(np.zeros(IP.N_SUMS), np.float64)
    ok = dict(src=_m.ptr(s), n=n, points=_m.ptr(g), normals=_m.ptr(nr), N=N, trim=1.0, alpha=0.0, ws=_m.ptr(ws),
              ws_bytes=8 * IP.N_SUMS, state=_m.ptr(state), near=_m.ptr(near), log=_m.ptr(log))

    def cloud(**kw):
        a = dict(ok, **kw)
        return L.mslam_icp_plane_step_cloud(a["src"], a["n"], a["points"], a["normals"], a["N"], 0, 0, 0, 1, a["trim"],
                                            a["alpha"], 1, a["ws"], a["ws_bytes"], a["state"], a["near"], _m.ptr(moved),
                                            _m.ptr(d2), 0, a["log"], st)

    for bad in (dict(n=-1), dict(N=-1), dict(trim=-0.5), dict(trim=math.nan), dict(alpha=-1.0), dict(alpha=math.inf),
                dict(alpha=math.nan), dict(src=0), dict(normals=0), dict(state=0), dict(log=0), dict(near=0), dict(ws=0)):
        assert cloud(**bad) == EINVAL, bad
    assert cloud(ws_bytes=8 * IP.N_SUMS - 1) == ENOMEM
    assert "needed" in L.mslam_last_error().decode()
    v, f = mg
    mesh = lambda **kw: L.mslam_icp_plane_step_mesh(ok["src"], n, _m.ptr(v), _m.ptr(f), kw.get("F", len(tf)), len(tv),
                                                    kw.get("trim", 1.0), kw.get("alpha", 0.0), 1, ok["ws"],
                                                    kw.get("ws_bytes", 0), ok["state"], ok["near"], _m.ptr(moved),
                                                    _m.ptr(d2), 0, ok["log"], st)
    assert mesh() == ENOMEM                  # no room for the boxes
    assert mesh(F=-1) == mesh(trim=-1.0) == mesh(alpha=-1.0) == EINVAL
    assert L.mslam_icp_plane_step_mesh_indexed(ok["src"], n, _m.ptr(v), _m.ptr(f), len(tf), len(tv), 0, 0, 0, 1.0, 0.0, 1,
                                               ok["ws"], ok["ws_bytes"], ok["state"], ok["near"], _m.ptr(moved),
                                               _m.ptr(d2), 0, ok["log"], st) == EINVAL
    assert L.mslam_icp_plane_workspace_bytes(-1, 0) == 0
    torch.cuda.synchronize()
    ops.check()
    assert not torch.count_nonzero(log) and not torch.count_nonzero(state)   # a refused call writes nothing


# ----------------------------------------------------------------------------------------------------------------------
# the figures and the product
# ----------------------------------------------------------------------------------------------------------------------
def test_compare_clouds_with_the_plane_metric(device):
    from mast3r_slam.tsdf import align_clouds, compare_clouds, compare_meshes, align_meshes, transform_cloud

    pred, gt, _, _ = IP.box_case()
    p, g = _dev(device, pred, np.float32), _dev(device, gt, np.float32)
    kw = dict(metric="plane", point_weight=0.05, n_samples=500, max_iters=8, trim=0.3)
    got = compare_clouds(p, g, threshold=0.05, align="icp", align_kw=kw, index=True)
    res = align_clouds(p, g, index=True, **kw)
    by_hand = compare_clouds(transform_cloud(p, res["T"]), g, threshold=0.05, index=True)
    assert got["alignment"] == dict(rmse=res["rmse"], iterations=res["iterations"], T=res["T"].tolist())
    assert {k: v for k, v in got.items() if k != "alignment"} == by_hand
    plain = compare_clouds(p, g, threshold=0.05, align="icp", align_kw=dict(n_samples=500, max_iters=8, trim=0.3))
    print(f"box accuracy after 8 iterations: plane {got['accuracy']:.5f}, point {plain['accuracy']:.5f}")
    assert got["accuracy"] < plain["accuracy"]
    (sv, sf), (tv, tf), truth = A.recovery_case("small")
    mp, mg = (_dev(device, sv, np.float32), _dev(device, sf, np.int32)), (_dev(device, tv, np.float32),
                                                                         _dev(device, tf, np.int32))
    mkw = dict(metric="plane", n_samples=A.RECOVERY_N, max_iters=6, trim=A.RECOVERY_TRIM)
    fig = compare_meshes(mp, mg, n_samples=2000, threshold=0.05, align="icp", align_kw=mkw)
    res = align_meshes(mp, mg, **mkw)
    assert fig["alignment"]["T"] == res["T"].tolist() and fig["accuracy"] <= 1e-5


def test_slam_system_evaluates_with_the_plane_metric(device, monkeypatch):
    """The 20-frame run of the product tests, scored against the room moved by a known Sim3, ICP from the trajectory's
    transform with align_kw=dict(metric="plane", point_weight=0.05).  The accuracy and precision bars are those of
    test_mesh_align_gpu.test_slam_system_evaluate_mesh_aligned for the mesh and of test_cloud_gpu.test_slam_system_cloud
    for the cloud.  Measured on MI355X, the file run alone: mesh accuracy in frame 4.084 mm, after plane ICP 3.136 mm
    (point-to-mesh ICP: 3.230 mm), precision 1.0000 in both; cloud 14.300 mm by the trajectory's transform, 14.116 mm
    after plane ICP (25 iterations).  Within the whole suite the threaded run gave 3.902 mm and 2.971 mm.

    What is NOT asserted, and why: that test's last bar - the ICP transform within twice the in-frame accuracy of the
    true one - does not hold for this metric on this scene.  The mesh's ICP does not converge in its 50 iterations and
    ends 69 mm and 4.9 % in scale from the truth (61 mm, 4.4 % within the suite; point-to-mesh: 5.2 mm, 0.24 %) while the accuracy keeps improving:
    three keyframes see little more than a corner, three orthogonal planes do not determine the scale (DESIGN.md
    "Point-to-plane ICP", "What a plane cannot fix"), and a point weight of 0.05 is a weak tie against the
    reconstruction's own systematic 4 mm.  The figures are printed; for a ground truth with poses the trajectory's
    transform remains the unbiased choice."""
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from mast3r_slam.tsdf import sample_mesh
    from mast3r_slam import synthetic
    from test_slam_system_gpu import RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    move = A.sim3_from((25.0, (0.2, 1.0, 0.1)), (2.0, -1.0, 0.5), 1.6)
    s = move[7]
    rv, rf = synthetic.room_mesh()
    gv = A.act(move, rv.astype(np.float64)).astype(np.float32)
    surface = sample_mesh(torch.from_numpy(rv).to(device), torch.from_numpy(rf).to(device), 200_000, seed=3)[0]
    moved = torch.from_numpy(A.act(move, surface.cpu().numpy().astype(np.float64)).astype(np.float32)).to(device)
    n, thr = 20000, 2.0
    plane = dict(metric="plane", point_weight=0.05, trim=0.12 * s)
    try:
        system.run(_frames(list(range(0, 60, 3)), device))
        in_frame = system.evaluate_mesh(rv, rf, n_samples=n, threshold=VS)
        centres = np.stack([system.keyframes[i].T_WC.data.reshape(8)[:3].cpu().numpy()
                            for i in range(len(system.keyframes))])
        gt_pos = A.act(move, centres.astype(np.float64)).astype(np.float32)
        mesh = system.evaluate_mesh(gv, rf, n_samples=n, threshold=VS * s, align="icp", init="trajectory",
                                    gt_positions=gt_pos, align_kw=plane)
        ckw = dict(threshold=VS * s, voxel=VS * s, conf_threshold=thr, index=True)
        T_traj = system.align_trajectory(gt_pos).cpu().numpy()
        by_traj = system.evaluate_cloud(moved, align=T_traj, **ckw)
        cloud = system.evaluate_cloud(moved, align="icp", init="trajectory", gt_positions=gt_pos, align_kw=plane, **ckw)
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    t_err, s_err = A.sim3_error(np.array(mesh["alignment"]["T"]), move)[1:]
    print(f"mesh: accuracy in frame {in_frame['accuracy']:.6f} precision {in_frame['precision']:.4f}; plane ICP "
          f"{mesh['accuracy'] / s:.6f} {mesh['precision']:.4f}, {mesh['alignment']['iterations']} iterations, "
          f"{t_err:.4g} m / {s_err:.3g} from the truth; cloud: by trajectory {by_traj['accuracy'] / s:.6f}, plane ICP "
          f"{cloud['accuracy'] / s:.6f}, {cloud['alignment']['iterations']} iterations")
    for fig in (mesh, cloud):
        assert fig["alignment"]["iterations"] >= 1 and len(fig["alignment"]["T"]) == 8
        assert np.isfinite(fig["alignment"]["rmse"])
    assert mesh["accuracy"] / s <= in_frame["accuracy"] + 1e-4
    assert mesh["accuracy"] / s >= 0.5 * in_frame["accuracy"]
    assert mesh["precision"] >= in_frame["precision"] - 1e-3
    assert cloud["accuracy"] / s <= by_traj["accuracy"] / s + 1e-4

