"""CPU tests of the numpy statement of the k nearest neighbours, the normals and the outlier rules of a point cloud
(tests/cloud_knn_numpy.py; DESIGN.md "Point clouds") on hand-computed cases, and of evaluate.save_cloud.
tests/test_cloud_knn_gpu.py runs the same traps on the device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_knn_numpy as K  # noqa: E402
import cloud_numpy as C  # noqa: E402
from test_cloud_cpu import duplicate_trap, f32_trap, lattice_trap  # noqa: E402


# ----------------------------------------------------------------------------------------------------------------------
# the traps, shared with the GPU tests
# ----------------------------------------------------------------------------------------------------------------------
def kth_tie_trap():
    """(queries, cloud, k, row): the lattice trap of test_cloud_cpu with a point ON the query put in front.  At k = 2
    the second place is a tie at distance 4 between point 1 = (8, 0, 0), whose Morton tile comes later, and point 129 =
    (0, 0, 0): the lower index wins, and at k = 3 both are listed, 1 first."""
    q, P, _ = lattice_trap()
    P = np.concatenate([q, P]).astype(np.float32)
    return q, P, 2, [0, 1]


def duplicates_trap():
    """(cloud, rows at k = 2 without exclusion, rows with every point excluded from its own row): points 0 and 2
    coincide, so each is the other's neighbour at distance 0 whether or not the point itself is left out."""
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [5, 0, 0]], np.float32)
    return P, [[0, 2], [1, 0], [0, 2], [3, 1]], [[2, 1], [0, 2], [0, 1], [1, 0]]


def test_total_order_and_kth_tie():
    q, P, k, row = kth_tie_trap()
    order = C.order_of(C.point_keys(P))
    pos = {int(j): s for s, j in enumerate(order)}
    assert pos[1] // C.TILE > pos[129] // C.TILE                        # the lower index lies in the later tile
    d2, nb = K.knn(q, P, k)
    assert nb[0].tolist() == row and d2[0].tolist() == [0.0, 16.0]
    d2, nb = K.knn(q, P, 3)
    assert nb[0].tolist() == [0, 1, 129] and d2[0].tolist() == [0.0, 16.0, 16.0]
    assert (np.delete(C.dist2_matrix(q, P)[0], [0, 1, 129]) >= 17.0).all()
    # k = 1 is the nearest neighbour of cloud_numpy, on every trap of test_cloud_cpu
    for qq, PP in (f32_trap()[:2], lattice_trap()[:2], duplicate_trap()[:2]):
        one, ref = K.knn(qq, PP, 1), C.nearest(qq, PP)
        assert one[0][:, 0].tobytes() == ref[0].tobytes() and one[1][:, 0].tobytes() == ref[1].tobytes()


def test_duplicates_and_exclusion():
    P, plain, excluded = duplicates_trap()
    d2, nb = K.knn(P, P, 2)
    assert nb.tolist() == plain and d2[:, 0].tolist() == [0, 0, 0, 0] and d2[:, 1].tolist() == [0, 1, 0, 16]
    d2, nb = K.knn(P, P, 2, exclude=np.arange(4))
    assert nb.tolist() == excluded and d2.tolist() == [[0, 1], [1, 1], [0, 1], [16, 25]]
    # an entry outside [0, N) excludes nothing
    d2, nb = K.knn(P, P, 2, exclude=[-1, 4, 2 ** 31 - 1, -2 ** 31])
    assert nb.tolist() == plain


def test_fewer_than_k_and_validity():
    P = np.array([[0, 0, 0], [np.nan, 0, 0], [2, 0, 0], [1, np.inf, 0]], np.float32)
    q = np.array([[0.5, 0, 0], [np.nan, 0, 0], [3, 0, 0]], np.float32)
    d2, nb = K.knn(q, P, 4)
    assert nb.tolist() == [[0, 2, -1, -1], [-1] * 4, [2, 0, -1, -1]]
    assert d2[0].tolist() == [0.25, 2.25, np.inf, np.inf] and np.isposinf(d2[1]).all()
    d2, nb = K.knn(q, P, 2, exclude=[0, 0, 2])
    assert nb.tolist() == [[2, -1], [-1, -1], [0, -1]]
    for empty in (P[[1, 3]], np.zeros((0, 3), np.float32)):
        d2, nb = K.knn(q, empty, 3)
        assert (nb == -1).all() and np.isposinf(d2).all() and nb.shape == (3, 3) and nb.dtype == np.int32
    assert K.knn(q[:0], P, 3)[0].shape == (0, 3)


def test_f32_and_contraction_traps_at_k2():
    q, P, want = f32_trap()
    d2, nb = K.knn(q, P, 2)
    assert nb[0].tolist() == [want, 1 - want] and d2[0].tolist() == [16781312.0, 16781312.25]
    cases = C.contraction_cases()
    assert cases
    for q, p in cases[:8]:
        cloud = np.stack([p + np.float32(100.0), p])
        d2, nb = K.knn(q[None], cloud, 2)
        assert nb[0].tolist() == [1, 0] and d2[0, 0] == C.dist2_matrix(q[None], p[None])[0, 0] != C.dist2_fused(q, p)


# ----------------------------------------------------------------------------------------------------------------------
# normals
# ----------------------------------------------------------------------------------------------------------------------
def test_jacobi_against_eigh():
    rng = np.random.default_rng(0)
    B = rng.normal(size=(1000, 3, 3))
    A = B + B.transpose(0, 2, 1)
    A[:100] = np.einsum("nij,nkj->nik", B[:100], B[:100])              # positive semi-definite ones, as a covariance is
    A[100:110, 0, 1] = A[100:110, 1, 0] = 0.0                           # a zero pair is skipped
    D, V = K.jacobi3(A)
    lam = np.sort(np.stack([D[:, 0, 0], D[:, 1, 1], D[:, 2, 2]], 1), 1)
    want = np.linalg.eigh(A)[0]
    scale = np.abs(want).max(1, keepdims=True)
    assert (np.abs(lam - want) <= 1e-13 * scale).all()
    # the columns are the eigenvectors: A V = V diag(lam), and V is orthonormal
    lam_cols = np.stack([D[:, 0, 0], D[:, 1, 1], D[:, 2, 2]], 1)
    assert np.abs(A @ V - V * lam_cols[:, None, :]).max() <= 1e-12 * scale.max()
    assert np.abs(V.transpose(0, 2, 1) @ V - np.eye(3)).max() <= 1e-13
    # a diagonal matrix is left alone
    D, V = K.jacobi3(np.diag([3.0, 1.0, 2.0]))
    assert np.array_equal(D[0], np.diag([3.0, 1.0, 2.0])) and np.array_equal(V[0], np.eye(3))


def _self_rows(P, k):
    return K.knn(P, P, k)[1]


def test_normals_plane_line_coincident():
    rng = np.random.default_rng(1)
    plane = np.c_[rng.uniform(-1, 1, (40, 2)), np.zeros(40)].astype(np.float32)        # z = 0 exactly
    out = K.normals(plane, _self_rows(plane, 8))
    assert (out["count"] == 8).all() and not out["degenerate"].any()
    assert np.array_equal(out["normal"], np.tile(np.float32([0, 0, 1]), (40, 1)))
    assert (out["curvature"] == 0.0).all() and (out["covariance"][:, [2, 4, 5]] == 0.0).all()
    # towards a viewpoint below the plane; exactly in the plane: s == 0, no flip
    assert np.array_equal(K.normals(plane, _self_rows(plane, 8), viewpoint=[0, 0, -2])["normal"][:, 2], -np.ones(40))
    assert np.array_equal(K.normals(plane, _self_rows(plane, 8), viewpoint=[9, 9, 0])["normal"][:, 2], np.ones(40))
    # the largest component positive, the lowest axis on ties
    tilted = plane[:, [2, 0, 1]].copy()                                                  # x = 0: the normal is +-x
    assert np.array_equal(K.normals(tilted, _self_rows(tilted, 8))["normal"], np.tile(np.float32([1, 0, 0]), (40, 1)))
    line = (np.arange(12, dtype=np.float32)[:, None] * np.float32([1, 2, -1])).astype(np.float32)
    out = K.normals(line, _self_rows(line, 5))
    assert out["degenerate"].all() and not out["normal"].any() and np.isnan(out["curvature"]).all()
    same = np.tile(np.float32([[0.3, -0.2, 0.9]]), (6, 1))
    out = K.normals(same, _self_rows(same, 4))
    assert out["degenerate"].all() and (out["count"] == 4).all() and not out["normal"].any()
    # m < 3; an invalid point has no neighbours at all
    few = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0]], np.float32)
    out = K.normals(few, _self_rows(few, 4))
    assert out["count"].tolist() == [2, 2, 0] and out["degenerate"].all() and not out["centroid"][2].any()
    assert out["centroid"][0].tolist() == [0.5, 0, 0] and out["covariance"][0].tolist() == [0.25, 0, 0, 0, 0, 0]


def test_normals_by_hand():
    """Four points: three on z = 0 and one at z = 1 over the origin, every point's row the whole cloud in the order
    0, 1, 2, 3.  Centroid (0.25, 0.25, 0.25); covariance 3/16 on the diagonal and -1/16 off it, whose eigenvalues are
    1/16 (the direction (1, 1, 1) / sqrt 3) and 1/4 twice: the curvature is (1/16) / (9/16) = 1/9."""
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    rows = np.tile(np.arange(4), (4, 1))
    out = K.normals(P, rows)
    assert (out["centroid"] == 0.25).all() and out["covariance"][0].tolist() == [3 / 16, -1 / 16, -1 / 16, 3 / 16,
                                                                                 -1 / 16, 3 / 16]
    assert np.abs(out["normal"] - np.float32(1 / np.sqrt(3))).max() <= 2.0 ** -23
    assert np.abs(out["curvature"] - np.float32(1 / 9)).max() <= 2.0 ** -24
    assert np.abs(np.sort(out["eigenvalues"], 1) - [1 / 16, 1 / 4, 1 / 4]).max() <= 1e-15


# ----------------------------------------------------------------------------------------------------------------------
# outliers
# ----------------------------------------------------------------------------------------------------------------------
def test_sample_std_rule_by_hand():
    """Points at x = 0, 1, 2, 3, 10, k = 1: the mean distances are 1, 1, 1, 1, 7, mu = 2.2, the squared deviations sum
    to 4 * 1.44 + 23.04 = 28.8: the sample sigma is sqrt(7.2) = 2.683, the population's sqrt(5.76) = 2.4.  At std_ratio
    1.9 the threshold is 7.298 and the last point stays; with the population sigma it would be 6.76 and the point gone."""
    P = np.zeros((5, 3), np.float32)
    P[:, 0] = [0, 1, 2, 3, 10]
    mean, scored = K.mean_distances(P, 1)
    assert mean.tolist() == [1, 1, 1, 1, 7] and scored.all()
    mu, sigma = K.statistics(mean, scored)
    assert abs(mu - 2.2) <= 1e-15 and abs(sigma - np.sqrt(7.2)) <= 1e-15
    assert K.outliers(P, 1, 1.9).all() and 2.2 + 1.9 * 2.4 < 7.0
    assert K.outliers(P, 1, 1.0).tolist() == [True] * 4 + [False]
    assert K.outliers(P, 1, 1.9, threshold=6.9).tolist() == [True] * 4 + [False]
    # k = 2: the sum in list order over the two found, halved
    assert K.mean_distances(P, 2)[0].tolist() == [1.5, 1, 1, 1.5, 7.5]
    # an invalid point is never kept and enters no statistic; a lone point has no neighbour and is not kept
    Q = np.concatenate([P, np.float32([[np.nan, 0, 0]])])
    mean, scored = K.mean_distances(Q, 1)
    assert scored.tolist() == [True] * 5 + [False] and K.statistics(mean, scored) == (mu, sigma)
    assert K.outliers(Q, 1, 1.9).tolist() == [True] * 5 + [False]
    assert K.outliers(P[:1], 1, 2.0).tolist() == [False]
    assert K.statistics(*K.mean_distances(P[:2], 1)) == (1.0, 0.0)
    # the radius rule: the second neighbour exactly at the radius is within it
    assert K.outliers(P, std_ratio=None, radius=2.0, min_neighbors=2).tolist() == [True, True, True, True, False]
    assert K.outliers(P, std_ratio=None, radius=1.0, min_neighbors=2).tolist() == [False, True, True, False, False]
    assert K.outliers(P, 1, 1.9, radius=2.0, min_neighbors=2).tolist() == [True, True, True, True, False]


# ----------------------------------------------------------------------------------------------------------------------
# save_cloud
# ----------------------------------------------------------------------------------------------------------------------
def test_save_cloud_read_back(tmp_path):
    from mast3r_slam import evaluate as ev

    rng = np.random.default_rng(0)
    P = rng.normal(size=(9, 3)).astype(np.float32)
    nrm = rng.normal(size=(9, 3)).astype(np.float32)
    col = rng.integers(0, 256, (9, 3)).astype(np.uint8)
    ev.save_cloud(tmp_path / "full.ply", P, col, nrm)
    data = (tmp_path / "full.ply").read_bytes()
    head, body = data.split(b"end_header\n", 1)
    names = [ln.split()[-1] for ln in head.decode().split("\n") if ln.startswith("property")]
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"] and b"element vertex 9" in head
    rec = np.frombuffer(body, np.dtype([(n, "<f4") for n in names[:6]] + [(n, "u1") for n in names[6:]]))
    assert len(rec) == 9
    assert np.stack([rec["nx"], rec["ny"], rec["nz"]], 1).tobytes() == nrm.tobytes()
    got, gc = ev.load_ply_points(tmp_path / "full.ply")                   # the loader skips the normals
    assert got.tobytes() == P.tobytes() and np.array_equal(gc, col)
    ev.save_cloud(tmp_path / "plain.ply", P)
    got, gc = ev.load_ply_points(tmp_path / "plain.ply")
    assert got.tobytes() == P.tobytes() and gc is None
    ev.save_cloud(tmp_path / "normals.ply", P, normals=nrm)
    assert ev.load_ply_points(tmp_path / "normals.ply")[0].tobytes() == P.tobytes()
    ev.save_cloud(tmp_path / "colors.ply", P, col)                        # the bytes save_ply writes
    ev.save_ply(tmp_path / "ref.ply", P, col)
    assert (tmp_path / "colors.ply").read_bytes() == (tmp_path / "ref.ply").read_bytes()
    with pytest.raises(ValueError, match="normals must be"):
        ev.save_cloud(tmp_path / "bad.ply", P, normals=nrm[:-1])
