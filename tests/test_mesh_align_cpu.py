"""CPU tests of the numpy statement of the mesh-alignment definitions (tests/meshalign_numpy.py): the closest point
against tri_dist2, Horn's solve against an independent SVD formulation, trimmed ICP recovering a known Sim3 on a partial
room, the degenerate cases, and the argument checks of mast3r_slam.tsdf.mesh_align that need no device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshalign_numpy as A  # noqa: E402
import meshdist_numpy as D  # noqa: E402
from test_mesh_metrics_cpu import random_case  # noqa: E402


def pair_case(kind, seed=0, n=60, offset=1000.0):
    """(src f32[n,3], dst f32[n,3], weights f32[n] or None) `offset` metres from the origin: dst is a known Sim3 of src,
    for `weighted` with 1 cm of noise and random weights, a tenth of them zero."""
    rng = np.random.default_rng(seed)
    P = rng.normal(size=(n, 3))
    if kind == "coplanar":
        P[:, 2] = 0.25 * P[:, 0] - 0.5 * P[:, 1]
    P = (P + offset).astype(np.float32)
    T = A.sim3_from((rng.uniform(5.0, 175.0), rng.normal(size=3)), rng.normal(size=3), rng.uniform(0.5, 2.0))
    C = A.act(T, P.astype(np.float64))
    w = None
    if kind == "weighted":
        C = C + 0.01 * rng.normal(size=C.shape)
        w = rng.uniform(0.0, 2.0, n).astype(np.float32)
        w[rng.permutation(n)[:n // 10]] = 0.0
    return P, C.astype(np.float32), w


def test_closest_point_is_the_one_tri_dist2_selects():
    P, V, F = random_case(1)
    a, b, c, valid = D.triangles(V, F)
    p = P.astype(np.float64)
    for f in np.flatnonzero(valid):
        q = A.tri_closest(p, a[f], b[f], c[f])
        r = p - q
        assert np.array_equal(D._dot(r, r), D.tri_dist2(p, a[f], b[f], c[f]))
    d2, nearest = D.closest(P, V, F)
    q = A.closest_points(P, V, F, nearest)
    r = p - q
    assert np.array_equal(D._dot(r, r), d2)
    assert np.isnan(A.closest_points(P[:3], V, F, np.array([-1, 0, -1]))[[0, 2]]).all()
    # the pruned scan is the face-by-face scan
    F2 = np.concatenate([F[:7], [[0, 0, 1]], F[7:], F[:80]]).astype(np.int32)        # an invalid face, and ties
    want = D.closest(P, V, F2)
    got = A.closest(P, V, F2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[1].dtype == np.int32
    got = A.closest(P, V, F2[7:8])
    assert np.isinf(got[0]).all() and (got[1] == -1).all()


def test_transform_rounds_once_and_inverts():
    rng = np.random.default_rng(3)
    T = A.sim3_from((37.0, (1.0, -2.0, 0.5)), (0.3, -1.0, 2.0), 1.7)
    P = rng.normal(size=(100, 3))
    R = A.quat_to_mat(T[3:7])
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(R) - 1.0) <= 1e-15
    assert np.abs(A.act(T, P) - (T[7] * P @ R.T + T[:3])).max() <= 1e-14
    assert np.abs(A.act(A.sim3_inv(T), A.act(T, P)) - P).max() <= 1e-14
    T32 = T.astype(np.float32)
    st = A.init_state(T32)
    assert abs(np.linalg.norm(st[3:7]) - 1.0) <= 1e-15 and np.array_equal(st[[0, 1, 2, 7]], T32[[0, 1, 2, 7]])


@pytest.mark.parametrize("kind", ["generic", "coplanar", "weighted"])
def test_horn_against_svd_umeyama(kind):
    """Measured here: rotation and scale agree to about 1e-15, the translation (1000 m from the origin) to 2e-12."""
    P, C, w = pair_case(kind)
    for with_scale in (True, False):
        T, status, sums, _ = A.fit_pairs(P, C, w, with_scale)
        assert status == A.OK
        R, t, s = A.umeyama_svd(P.astype(np.float64), C.astype(np.float64), None if w is None else w.astype(np.float64),
                                with_scale)
        dR, dt, ds = np.abs(A.quat_to_mat(T[3:7]) - R).max(), np.abs(T[:3] - t).max(), abs(T[7] - s)
        print(f"{kind} with_scale={with_scale}: dR {dR:.2e} dt {dt:.2e} ds {ds:.2e}")
        assert dR <= 1e-9 and dt <= 1e-9 and ds <= 1e-9
        assert abs(np.linalg.det(A.quat_to_mat(T[3:7])) - 1.0) <= 1e-14 and T[6] >= 0.0
        assert sums[0] == (len(P) if w is None else (w > 0).sum())
    # the fit is the least-squares one: no nearby Sim3 does better
    T = A.fit_pairs(P, C, w)[0]
    ww = np.ones(len(P)) if w is None else w.astype(np.float64)
    cost = lambda X: float(ww @ ((A.act(X, P.astype(np.float64)) - C.astype(np.float64)) ** 2).sum(1))
    rng = np.random.default_rng(1)
    for _ in range(20):
        X = T + 1e-4 * rng.normal(size=8)
        X[3:7] /= np.linalg.norm(X[3:7])
        assert cost(X) >= cost(T)


# what the statement gives with the stratified sampler (1025 samples, seed 0, trim 0.25, 80 iterations), and the bounds:
# ten times that
RECOVERY_SEEN = {"small": (2.5e-8, 4.8e-7, 4.9e-8), "mid": (4.1e-8, 2.1e-6, 2.1e-7)}      # rad, m, scale


def recovery_run(name, P):
    """The numpy ICP of a recovery case on the samples P, computed once per sample set."""
    key = (name, P.tobytes())
    if key not in recovery_run.cache:
        _, (tv, tf), _ = A.recovery_case(name)
        recovery_run.cache[key] = A.icp(P, tv, tf, None, A.RECOVERY_ITERS, A.RECOVERY_TRIM, True)
    return recovery_run.cache[key]


recovery_run.cache = {}


def recovery_samples(name):
    (sv, sf), _, _ = A.recovery_case(name)
    return D.sample(sv, sf, np.cumsum(D.face_areas(sv, sf)), A.RECOVERY_N, seed=0)[0]


@pytest.mark.parametrize("name", ["small", "mid"])
def test_icp_recovers_a_known_sim3(name):
    """Observed: small (3 deg / 5 cm / 0.95) ends 2.5e-8 rad, 4.8e-7 m and 4.9e-8 in scale from the truth; mid (8 deg /
    15 cm / 0.9) 4.1e-8 rad, 2.1e-6 m, 2.1e-7.  After the first ten iterations every pair is an inlier and the RMSE
    falls by 4.4 to 5.7 every ten iterations."""
    (sv, sf), (tv, tf), truth = A.recovery_case(name)
    assert len(sf) == 264 and len(tf) == 192
    T, hist = recovery_run(name, recovery_samples(name))
    err = A.sim3_error(T, truth)
    print(f"{name}: rotation {err[0]:.3g} rad, translation {err[1]:.3g} m, scale {err[2]:.3g}; rmse every 10: "
          + " ".join(f"{r:.3g}" for r in hist[::10, 1]))
    assert all(e <= 10.0 * seen for e, seen in zip(err, RECOVERY_SEEN[name]))
    assert (hist[:, 3] == A.OK).all() and hist[0, 0] < A.RECOVERY_N and (hist[10:, 0] == A.RECOVERY_N).all()
    assert (hist[20::10, 1] <= hist[10:-10:10, 1] / 3.0).all()


def test_degenerate_and_trivial():
    rng = np.random.default_rng(0)
    P = rng.normal(size=(5, 3)).astype(np.float32)
    C = (2.0 * P + 1.0).astype(np.float32)
    ident = A.init_state()
    for n in (0, 1, 2):
        T, status, sums, _ = A.fit_pairs(P[:n], C[:n])
        assert status == A.DEGENERATE and np.array_equal(T, ident) and sums[0] == n
    T, status, _, _ = A.fit_pairs(np.repeat(P[:1], 5, 0), C)                  # all source points equal: no spread
    assert status == A.DEGENERATE and np.array_equal(T, ident)
    T, status, _, _ = A.fit_pairs(P, np.repeat(C[:1], 5, 0))                  # all targets equal: scale 0
    assert status == A.DEGENERATE
    T, status, _, _ = A.fit_pairs(P, np.repeat(C[:1], 5, 0), with_scale=False)
    assert status == A.OK and T[7] == 1.0                                     # defined without scale
    T, status, sums, rmse = A.fit_pairs(P, C, np.zeros(5, np.float32))        # all weights zero
    assert status == A.DEGENERATE and sums[0] == 0 and np.isinf(rmse)
    w = np.array([1, 1, 0, 0, 0], np.float32)                                 # two pairs that count
    assert A.fit_pairs(P, C, w)[1] == A.DEGENERATE
    T, status, _, _ = A.fit_pairs(P[:3], C[:3])                               # three points: exact
    assert status == A.OK and abs(T[7] - 2.0) <= 1e-6 and np.abs(T[:3] - 1.0).max() <= 1e-6
    # ICP without a face, and with every pair trimmed away: the state stays
    V = np.zeros((3, 3), np.float32)
    st = A.icp_step(ident, P, V, np.zeros((0, 3), np.int32))
    assert st["status"] == A.DEGENERATE and st["inliers"] == 0 and np.array_equal(st["T"], ident)
    tri = np.array([[0, 0, 50], [1, 0, 50], [0, 1, 50]], np.float32)
    st = A.icp_step(ident, P, tri, np.array([[0, 1, 2]], np.int32), trim=1.0)
    assert st["status"] == A.DEGENERATE and (st["nearest"] == 0).all() and not st["inlier"].any()
    assert A.icp_step(ident, P[:0], tri, np.array([[0, 1, 2]], np.int32))["status"] == A.DEGENERATE


def test_transform_mesh_matches_the_statement():
    from mast3r_slam.tsdf import transform_mesh

    rng = np.random.default_rng(5)
    V = rng.normal(size=(50, 3)).astype(np.float32)
    N = rng.normal(size=(50, 3)).astype(np.float32)
    T = A.sim3_from((64.0, (0.2, 1.0, -0.4)), (1.0, 2.0, -3.0), 0.6)
    moved, normals = transform_mesh(torch.from_numpy(V), T, torch.from_numpy(N))
    assert moved.dtype == torch.float32 and normals.dtype == torch.float32
    want = A.act(T, V.astype(np.float64))
    assert np.abs(moved.numpy() - want).max() <= 2.0 ** -23 * np.abs(want).max()
    want_n = N.astype(np.float64) @ A.quat_to_mat(T[3:7]).T
    assert np.abs(normals.numpy() - want_n).max() <= 2.0 ** -23 * np.abs(want_n).max()
    assert torch.equal(transform_mesh(torch.from_numpy(V), torch.from_numpy(T)), moved)
    assert torch.equal(transform_mesh(torch.from_numpy(V), [0, 0, 0, 0, 0, 0, 1, 1]), torch.from_numpy(V))


def test_argument_errors():
    from mast3r_slam.tsdf import align_meshes, compare_meshes, fit_sim3, transform_mesh

    P = torch.zeros(4, 3)
    mesh = (torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(TypeError, match="device tensor"):
        fit_sim3(np.zeros((4, 3), np.float32), P)
    with pytest.raises(ValueError, match=r"\(n,3\)"):
        fit_sim3(torch.zeros(4, 2), P)
    with pytest.raises(RuntimeError, match="dtype"):
        fit_sim3(P.double(), P)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_sim3(P, P)
    with pytest.raises(ValueError, match="8 numbers"):
        transform_mesh(P, [0.0] * 7)
    with pytest.raises(ValueError, match=r"\(V,3\)"):
        transform_mesh(torch.zeros(4), [0, 0, 0, 0, 0, 0, 1, 1])
    with pytest.raises(TypeError, match="tensor"):
        transform_mesh(np.zeros((4, 3)), [0, 0, 0, 0, 0, 0, 1, 1])
    with pytest.raises(ValueError, match="max_iters"):
        align_meshes(mesh, mesh, max_iters=0)
    with pytest.raises(ValueError, match="check_every"):
        align_meshes(mesh, mesh, check_every=0)
    with pytest.raises(ValueError, match="tol"):
        align_meshes(mesh, mesh, tol=-1.0)
    with pytest.raises(ValueError, match="one value per iteration"):
        align_meshes(mesh, mesh, max_iters=5, trim=[0.1, 0.2])
    with pytest.raises(ValueError, match="trim must be"):
        align_meshes(mesh, mesh, trim=-0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        align_meshes(mesh, mesh)
    with pytest.raises(ValueError, match="'icp'"):
        compare_meshes(mesh, mesh, align="svd")
    with pytest.raises(ValueError, match="align_kw"):
        compare_meshes(mesh, mesh, align_kw=dict(max_iters=3))
    with pytest.raises(ValueError, match="align_kw"):
        compare_meshes(mesh, mesh, align=[0, 0, 0, 0, 0, 0, 1, 1], align_kw=dict(max_iters=3))
