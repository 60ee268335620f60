"""CPU tests of the numpy statement of the point-cloud tools (tests/cloud_numpy.py; DESIGN.md "Point clouds") on
hand-computed cases.  Each trap is shown to separate the right answer from a named wrong one: f32 arithmetic, a fused
multiply-add, the first point met on a tie, np.rint for colours.  tests/test_cloud_gpu.py runs the same traps on the
device.  Also evaluate.load_ply_points against the two writers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_numpy as C  # noqa: E402
import meshalign_numpy as A  # noqa: E402

B = C.KEY_BIAS


# ----------------------------------------------------------------------------------------------------------------------
# the traps, shared with the GPU tests
# ----------------------------------------------------------------------------------------------------------------------
def f32_trap():
    """(queries, cloud, nearest): 4096.5^2 = 16781312.25 and 4096^2 + 64^2 = 16781312 tie in f32."""
    return np.zeros((1, 3), np.float32), np.array([[4096.5, 0, 0], [4096, 64, 0]], np.float32), 1


def lattice_trap():
    """(queries, cloud, nearest): two lattice clusters of 128 points; the cluster with the HIGH indices lies at the low
    coordinates, so it is Morton tile 0.  The query (4, 0, 0) is 4 away from point 0 = (8, 0, 0) and from point 128 =
    (0, 0, 0), every other point is farther: the answer is 0, and a scan in Morton order meets 128 first."""
    grid = np.array([(a, b, c) for a in range(8) for b in range(4) for c in range(4)], np.float32)
    high = grid + np.float32([8, 0, 0])
    low = grid * np.float32([-1, 1, 1])
    return np.array([[4, 0, 0]], np.float32), np.concatenate([high, low]), 0


def duplicate_trap():
    """(queries, cloud, order, nearest): the lattice cloud with point 200 moved onto point 3.  A stable sort keeps 3
    before 200 (equal keys), so the order is the cloud's own Morton order with 200 exchanged with the first entry: a
    permutation the entry points accept like any other, in which 200 is visited a tile earlier than 3."""
    _, P, _ = lattice_trap()
    P = P.copy()
    P[200] = P[3]
    order = C.order_of(C.point_keys(P)).copy()
    k = int(np.flatnonzero(order == 200)[0])
    assert k >= C.TILE and int(np.flatnonzero(order == 3)[0]) == k - 1 >= C.TILE
    order[0], order[k] = order[k], order[0]
    pos = {int(j): k for k, j in enumerate(order)}
    assert sorted(pos) == list(range(len(P))) and pos[200] // C.TILE < pos[3] // C.TILE
    return (P[3:4] + np.float32([0.25, 0, 0])).astype(np.float32), P, order, 3


def test_f32_arithmetic_trap():
    q, P, want = f32_trap()
    d2, nn = C.nearest(q, P)
    assert d2[0] == 16781312.0 and nn[0] == want
    assert C.dist2_matrix(q, P).tolist() == [[16781312.25, 16781312.0]]
    w2, wn = C.nearest_f32(q, P)
    assert wn[0] == 0 and w2[0] == np.float32(16781312.0)         # the named wrong form answers the other point


def test_contraction_trap():
    cases = C.contraction_cases()
    assert len(cases) >= 1
    q, p = cases[0]
    got = float(C.dist2_matrix(q[None], p[None])[0, 0])
    d = q.astype(np.float64) - p.astype(np.float64)
    assert got == (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] != C.dist2_fused(q, p)
    assert abs(got - C.dist2_fused(q, p)) <= 2.0 ** -51 * got       # one rounding apart, and still other bits


def test_tie_direction_traps():
    q, P, want = lattice_trap()
    order = C.order_of(C.point_keys(P))
    assert (order[:C.TILE] >= 128).all() and (order[C.TILE:] < 128).all()      # the high indices are tile 0
    d2, nn = C.nearest(q, P)
    assert d2[0] == 16.0 and nn[0] == want
    assert C.dist2_matrix(q, P)[0, 128] == 16.0 and (np.delete(C.dist2_matrix(q, P)[0], [0, 128]) >= 17.0).all()
    assert C.nearest_in_order(q, P, order)[1][0] == want
    assert C.nearest_in_order(q, P, order, tie="first")[1][0] == 128          # the named wrong form
    q, P, order, want = duplicate_trap()
    assert C.nearest(q, P)[1][0] == want and C.nearest(q, P)[0][0] == 0.0625
    assert C.nearest_in_order(q, P, order)[1][0] == want
    assert C.nearest_in_order(q, P, order, tie="first")[1][0] == 200


def test_validity_rules():
    P = np.array([[0, 0, 0], [np.nan, 0, 0], [1, np.inf, 0], [2, 0, 0]], np.float32)
    q = np.array([[1.9, 0, 0], [0.1, 0, 0], [np.nan, 0, 0], [0, -np.inf, 0], [1, 0, 0]], np.float32)
    d2, nn = C.nearest(q, P)
    assert nn.tolist() == [3, 0, -1, -1, 0] and np.isposinf(d2[2:4]).all() and d2[4] == 1.0
    d2, nn = C.nearest(q, P[1:3])
    assert (nn == -1).all() and np.isposinf(d2).all()
    d2, nn = C.nearest(q, np.zeros((0, 3), np.float32))
    assert (nn == -1).all() and np.isposinf(d2).all()
    assert C.nearest(np.repeat(P[:1], 300, 0)[:2], np.repeat(P[3:], 300, 0))[1].tolist() == [0, 0]
    # the index: bounds over the valid points only, the invalid points last
    assert C.bounds(P).tolist() == [0, 0, 0, 2, 0, 0]
    keys = C.point_keys(P)
    assert (keys[[1, 2]] == C.NONE).all() and C.order_of(keys).tolist() == [0, 3, 1, 2]
    tile, group = C.boxes(P, C.order_of(keys))
    assert tile.tolist() == group.tolist() == [[0, 0, 0, 2, 0, 0]]
    tile, _ = C.boxes(P, [1, 2, -1, 7])
    assert np.isposinf(tile[0, :3]).all() and np.isneginf(tile[0, 3:]).all()
    one = C.boxes(P[3:], [0])[0]
    assert one.tolist() == [[2, 0, 0, 2, 0, 0]]                                  # a zero-extent box


def _key(ix, iy, iz):
    return ((ix + B) << 42) | ((iy + B) << 21) | (iz + B)


def test_voxel_keys():
    vs = 0.25
    below = np.nextafter(np.float32(0), np.float32(-1))
    top, past = np.float32((B - 1) * vs), np.float32(B * vs)
    bottom = np.float32(-B * vs)
    P = np.array([[0.5, 0.25, 0.0], [-0.0, below, 0.24999], [top, bottom, 0], [past, 0, 0],
                  [0, np.nextafter(bottom, np.float32(-np.inf)), 0], [np.nan, 0, 0], [0, 0, np.inf], [0, 0, 3e30]],
                 np.float32)
    assert float(top) == (B - 1) * vs and float(past) == B * vs
    keys = C.voxel_keys(P, vs)
    assert keys[:3].tolist() == [_key(2, 1, 0), _key(0, -1, 0), _key(B - 1, -B, 0)]
    assert (keys[3:] == C.NONE).all()
    # the arithmetic is f32: 0.3 / 0.1 is 3 in f32 and 2.9999999999999996 in f64
    assert C.voxel_keys([[0.3, 0, 0]], 0.1)[0] == _key(3, 0, 0)
    assert np.floor(np.float64(np.float32(0.3)) / np.float64(0.1)) == 3.0 and np.floor(0.3 / 0.1) == 2.0


def test_voxel_reduce_and_colour_rounding():
    vs = 1.0
    P = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.25, 0.5, 0.5], [np.nan, 0, 0], [0.75, 0.75, 0.5],
                  [1.25, 0.5, 0.5], [0.5, 0.5, 0.25]], np.float32)
    col = np.array([[0, 1, 254], [1, 10, 0], [1, 2, 255], [9, 9, 9], [0, 0, 1], [2, 11, 1], [1, 0, 0]], np.uint8)
    cen, cnt, first, color, keys = C.voxel_reduce(P, vs, col)
    assert keys.tolist() == [_key(0, 0, 0), _key(1, 0, 0)] and cnt.tolist() == [4, 2] and first.tolist() == [0, 1]
    assert cen.tolist() == [[0.5, 0.5625, 0.4375], [1.375, 0.5, 0.5]]
    # sums (2, 3, 510) over 4 and (3, 21, 1) over 2: 0.5 -> 1, 0.75 -> 1, 127.5 -> 128; 1.5 -> 2, 10.5 -> 11, 0.5 -> 1
    assert color.tolist() == [[1, 1, 128], [2, 11, 1]]
    assert np.rint(np.array([0.5, 127.5, 1.5, 10.5])).tolist() == [0, 128, 2, 10]   # the named wrong form: ties to even
    assert C.voxel_reduce(P, vs)[3] is None
    # the order of summation is the definition: one addition at a time, in original index order
    big = np.float32([[1e8, 0, 0]] + [[1.0, 0, 0]] * 64)
    small_first = big[::-1]
    a, b = C.voxel_reduce(big, 1e9)[0], C.voxel_reduce(small_first, 1e9)[0]
    s = np.float64(1e8)
    for _ in range(64):
        s = s + 1.0
    assert a[0, 0] == np.float32(s / 65.0) and C.voxel_reduce(big, 1e9)[1].tolist() == [65]
    assert b.shape == (1, 3)
    empty = C.voxel_reduce(np.zeros((0, 3), np.float32), 1.0, np.zeros((0, 3), np.uint8))
    assert empty[0].shape == (0, 3) and empty[3].shape == (0, 3)


def test_figures_by_hand():
    pred = np.array([[0, 0, 0], [1, 0, 0], [5, 0, 0], [np.nan, 0, 0]], np.float32)
    gt = np.array([[0, 0.5, 0], [1, 0, 0], [1, 2, 0]], np.float32)
    f = C.figures(pred, gt, threshold=0.75)
    assert (f["n_pred"], f["n_gt"]) == (3, 3)
    assert f["accuracy"] == (0.5 + 0.0 + 4.0) / 3 and f["accuracy_median"] == 0.5
    assert f["completion"] == (0.5 + 0.0 + 2.0) / 3 and f["completion_median"] == 0.5
    assert f["accuracy_rmse"] == np.sqrt((0.25 + 16.0) / 3)
    assert f["precision"] == 2 / 3 and f["recall"] == 2 / 3 and abs(f["fscore"] - 2 / 3) < 1e-15
    assert f["chamfer"] == 0.5 * (f["accuracy"] + f["completion"])
    g = C.figures(pred, gt, threshold=0.75, max_dist=3.0)
    assert g["accuracy"] == 0.25 and g["accuracy_outliers"] == 1 and g["completion_outliers"] == 0
    assert g["precision"] == f["precision"] and g["completion"] == f["completion"]
    same = C.figures(gt, gt)
    assert same["accuracy"] == 0.0 and same["fscore"] == 1.0


def test_icp_step_recovers_exact_pairs():
    rng = np.random.default_rng(3)
    gt = rng.uniform(-1, 1, (200, 3)).astype(np.float32)
    move = A.sim3_from((2.0, (1.0, 2.0, 3.0)), (0.01, -0.01, 0.005), 0.98)
    src = A.act(A.sim3_inv(move), gt.astype(np.float64)).astype(np.float32)
    sample, idx = C.stride_sample(src, 50)
    assert idx.tolist() == [(i * 200) // 50 for i in range(50)]
    st = C.icp_step(A.init_state(), sample, gt)
    assert st["status"] == C.OK and (st["nearest"] == idx).all() and st["inliers"] == 50
    assert max(A.sim3_error(st["T"], move)) <= 1e-6
    none = C.icp_step(A.init_state(), sample, gt, trim=0.0)
    assert none["status"] == C.DEGENERATE and none["inliers"] == 0 and np.array_equal(none["T"], A.init_state())
    T, hist = C.icp(sample, gt, iters=3)
    assert hist[-1, 1] <= 1e-6 and hist[0, 1] > 1e-3


# ----------------------------------------------------------------------------------------------------------------------
# load_ply_points
# ----------------------------------------------------------------------------------------------------------------------
def test_load_ply_points(tmp_path):
    from mast3r_slam import evaluate as ev

    rng = np.random.default_rng(0)
    P = rng.normal(size=(7, 3)).astype(np.float32)
    col = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    ev.save_ply(tmp_path / "cloud.ply", P, col)
    got, gc = ev.load_ply_points(tmp_path / "cloud.ply")
    assert got.dtype == np.float32 and got.tobytes() == P.tobytes() and gc.dtype == np.uint8 and np.array_equal(gc, col)
    F = np.array([[0, 1, 2], [2, 3, 4]], np.int32)
    ev.save_mesh(tmp_path / "mesh.ply", P, F, normals=P)
    got, gc = ev.load_ply_points(tmp_path / "mesh.ply")
    assert got.tobytes() == P.tobytes() and gc is None
    ev.save_mesh(tmp_path / "mesh_c.ply", P, F, colors=col / 255.0)
    got, gc = ev.load_ply_points(tmp_path / "mesh_c.ply")
    assert got.tobytes() == P.tobytes() and np.array_equal(gc, col)
    ev.save_ply(tmp_path / "none.ply", P[:0], col[:0])
    assert ev.load_ply_points(tmp_path / "none.ply")[0].shape == (0, 3)
    data = (tmp_path / "cloud.ply").read_bytes()
    (tmp_path / "short.ply").write_bytes(data[:-1])
    with pytest.raises(ValueError, match="ends inside the vertex element"):
        ev.load_ply_points(tmp_path / "short.ply")
    (tmp_path / "ascii.ply").write_bytes(data.replace(b"binary_little_endian", b"ascii"))
    with pytest.raises(ValueError, match="ASCII"):
        ev.load_ply_points(tmp_path / "ascii.ply")
    (tmp_path / "no.ply").write_bytes(b"not a ply at all")
    with pytest.raises(ValueError, match="not a PLY"):
        ev.load_ply_points(tmp_path / "no.ply")
    (tmp_path / "double.ply").write_bytes(data.replace(b"property float x", b"property double x"))
    with pytest.raises(ValueError, match="must be float"):
        ev.load_ply_points(tmp_path / "double.ply")
    (tmp_path / "list.ply").write_bytes(data.replace(b"property uchar red", b"property list uchar int red"))
    with pytest.raises(ValueError, match="unsupported vertex property"):
        ev.load_ply_points(tmp_path / "list.ply")
    path = ev.save_cloud_metrics(tmp_path, "m.json", dict(b=1.0, a=2))
    assert path.read_text().index('"a"') < path.read_text().index('"b"')
