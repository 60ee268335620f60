"""CPU tests of the mesh index's numpy statement (tests/meshindex_numpy.py, DESIGN.md "Mesh index"): the order is a
permutation with the invalid faces last, boxes contain their faces, a scan over the permuted tiles with the tie rule
by ORIGINAL face index equals the plain ascending scans of meshdist_numpy / raycast_numpy on the caller's mesh, and each
tie trap separates that answer from "the first face met in scan order".  The builders of the meshes and traps are shared
with tests/test_mesh_index_gpu.py."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshdist_numpy as D  # noqa: E402
import meshindex_numpy as X  # noqa: E402
import raycast_numpy as R  # noqa: E402

T = 128            # kMdTile of csrc/mesh_tri.h: faces per tile and per box
G = 32             # kMdGroup: tiles per group box
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1, 1], np.float32)


def shuffled(F, seed=5):
    """The faces in a fixed shuffled order."""
    return np.ascontiguousarray(np.asarray(F, np.int32)[np.random.default_rng(seed).permutation(len(F))])


def reverse_morton(V, F):
    """The faces renumbered so that their Morton order is the reverse of their index order: face 0 has the largest key.
    A scan in Morton order then meets the highest index first."""
    keys = X.face_keys(V, F)
    F = np.ascontiguousarray(np.asarray(F, np.int32)[np.argsort(-keys.astype(np.float64), kind="stable")])
    k2 = X.face_keys(V, F)
    assert (np.diff(k2) <= 0).all() and k2[0] > k2[-1]
    return F


@functools.lru_cache(maxsize=None)
def random_mesh(nf, seed=0):
    """Small random f32 triangles in the unit cube in a random order (every tile's box is the whole cube without an
    index), one of them degenerate and one out of range from 8 faces on, and from 130 faces on the last valid face a
    copy of face 1: a tie across tiles."""
    rng = np.random.default_rng(9000 + 7 * nf + seed)
    centre = rng.uniform(0.0, 1.0, (nf, 3))
    V = (centre[:, None, :] + rng.uniform(-0.05, 0.05, (nf, 3, 3))).astype(np.float32)
    F = np.arange(3 * nf, dtype=np.int32).reshape(nf, 3)
    if nf >= 8:
        V[nf // 2, 2] = V[nf // 2, 0]                   # degenerate: two corners coincide
        F[nf // 3] = (0, 1, 3 * nf)                     # out of range
    if nf >= T + 2:
        V[nf - 1] = V[1]
    return V.reshape(-1, 3), F


@functools.lru_cache(maxsize=None)
def fan_trap(n=300):
    """A cone of n faces round one shared apex, more than two tiles of them, renumbered so that their Morton order is the
    reverse of their index order, and a query above the apex: the apex is the closest point of every face (its vertex
    region, strictly), so every face ties exactly and face 0, the LAST one met, must win.  The apex takes each of the
    three corner slots in turn.  -> (V, F, P)"""
    ang = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([0.5 + 0.4 * np.cos(ang), 0.5 + 0.4 * np.sin(ang), np.full(n, 0.2)], 1)
    V = np.concatenate([[[0.5, 0.5, 0.6]], ring]).astype(np.float32)
    F = np.array([np.roll((0, 1 + i, 1 + (i + 1) % n), i % 3) for i in range(n)], np.int32)
    P = np.array([[0.5, 0.5, 0.9], [0.5, 0.5, 0.7], [0.53125, 0.5, 1.0]], np.float32)
    return V, reverse_morton(V, F), P


@functools.lru_cache(maxsize=None)
def ray_trap():
    """Two faces of a square in the plane z = 1 that share its diagonal, among 300 faces far behind them, renumbered so
    that their Morton order is the reverse of their index order; from the origin one ray runs through the shared edge
    and one through a shared corner.  t is (U + V + W) / det = 1 exactly for each face hit, so they tie, and the lowest
    original index must win.  -> (V, F, rays f32[2,3], pose)"""
    sq = np.array([[-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], np.float32)
    Vb, Fb = random_mesh(300, seed=1)
    V = np.concatenate([sq, Vb * np.float32(2.0) + np.float32([-1.0, -1.0, 5.0])]).astype(np.float32)
    F = np.concatenate([[[0, 1, 2], [0, 2, 3]], Fb + 4]).astype(np.int32)
    F[F >= len(V)] = len(V)                                                  # the out-of-range face stays out of range
    rays = np.array([[0, 0, 1], [-1, -1, 1]], np.float32)
    return V, reverse_morton(V, F), rays, IDENTITY


def subdivide(V, F, times):
    """Every face split into four at its edge midpoints, `times` times; the midpoints are not shared (a soup)."""
    V, F = np.asarray(V, np.float32), np.asarray(F, np.int32)
    for _ in range(times):
        a, b, c = (V[F[:, k]].astype(np.float64) for k in range(3))
        ab, bc, ca = ((a + b) / 2, (b + c) / 2, (c + a) / 2)
        tri = np.stack([np.stack(t, 1) for t in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))], 1)
        V = tri.reshape(-1, 3).astype(np.float32)
        F = np.arange(len(V), dtype=np.int32).reshape(-1, 3)
    return V, F


def test_order_is_a_permutation_with_invalid_faces_last():
    for nf in (1, 7, T, T + 1, 300):
        V, F = random_mesh(nf)
        keys = X.face_keys(V, F)
        order = X.order_of(keys)
        valid = D.triangles(V, F)[3]
        assert sorted(order.tolist()) == list(range(nf))
        assert (keys[~valid] == X.NONE).all() and (keys[valid] >= 0).all() and (keys[valid] < X.NONE).all()
        nv = int(valid.sum())
        assert valid[order[:nv]].all() and not valid[order[nv:]].any()
        assert (np.diff(keys[order]) >= 0).all()
        # stable: equal keys keep their index order
        same = np.diff(keys[order]) == 0
        assert (np.diff(order)[same] > 0).all()
    # the key's bits: x highest, 21 bits per axis, the box's far corner in the last cell
    bnd = np.array([0, 0, 0, 1, 2, 4], np.float32)
    k = X.morton(np.array([[1.0, 0, 0], [0, 2.0, 0], [0, 0, 4.0], [0.5, 0, 0], [-3.0, 9.0, np.nan]]), bnd)
    full = sum(1 << (3 * i) for i in range(21))
    assert k.tolist() == [full << 2, full << 1, full, 1 << 62, full << 1]
    assert X.point_keys(np.float32([[1, 2, 4]]), bnd)[0] == X.NONE          # all ones: the one key an invalid face shares


def test_boxes_contain_their_faces():
    for nf in (1, T - 1, T, T + 1, 300):
        V, F = random_mesh(nf)
        order = X.order_of(X.face_keys(V, F))
        tile, group = X.boxes(V, F, order)
        a, b, c, valid = D.triangles(V, F)
        assert tile.shape == ((nf + T - 1) // T, 6) and group.shape == ((len(tile) + G - 1) // G, 6)
        for slot, f in enumerate(order):
            if valid[f]:
                for box in (tile[slot // T], group[slot // (T * G)]):
                    for p in (a[f], b[f], c[f]):
                        assert (box[:3] <= p).all() and (p <= box[3:]).all()
        # Morton tiles of shuffled faces are compact: far smaller than the tiles of the faces' own order
        if nf >= 300:
            plain = X.boxes(V, F, np.arange(nf))[0]
            vol = lambda bx: np.prod(bx[:, 3:] - bx[:, :3], 1).sum()
            assert vol(tile) < 0.6 * vol(plain)
    # an order with entries out of range: they are skipped; an all-invalid mesh: empty boxes
    V, F = random_mesh(T + 1)
    tile, group = X.boxes(V, F, np.array([5, -1, T + 1, 6] + [-7] * (T - 3), np.int32))
    assert np.isfinite(tile[0]).all() and np.isposinf(tile[1, :3]).all() and np.isneginf(tile[1, 3:]).all()
    want = np.concatenate([V[F[[5, 6]].reshape(-1)].min(0), V[F[[5, 6]].reshape(-1)].max(0)])
    assert np.array_equal(tile[0], want.astype(np.float64)) and np.array_equal(group[0], tile[0])
    tile, group = X.boxes(V, np.zeros((3, 3), np.int32), np.arange(3))
    assert np.isposinf(tile[:, :3]).all() and np.isneginf(group[:, 3:]).all()


def test_permuted_scans_equal_the_plain_ones():
    rng = np.random.default_rng(3)
    for nf in (T + 2, 300):
        V, F = random_mesh(nf)
        order = X.order_of(X.face_keys(V, F))
        P = rng.uniform(-0.1, 1.1, (40, 3)).astype(np.float32)
        P[:3] = V[F[1]]                                    # on the duplicated face: an exact tie at distance 0
        want = D.closest(P, V, F)
        got = X.closest_in_order(P, V, F, order)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert (want[1][:3] != nf - 1).all()
        d = rng.normal(size=(40, 3))
        o = np.array([0.5, 0.5, 0.5])
        d[:3] = V[F[1]].astype(np.float64).mean(0) - o + 1e-3 * rng.normal(size=(3, 3))      # towards the duplicate
        want = R.cast(o, d, V, F, 0.0, 10.0)
        got = X.cast_in_order(o, d, V, F, order, 0.0, 10.0)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert (want[1][:3] == 1).all()


def test_tie_traps_separate_the_rule_from_scan_order():
    V, F, P = fan_trap()
    order = X.order_of(X.face_keys(V, F))
    assert (order == np.arange(len(F))[::-1]).all() and len(F) > 2 * T
    want = D.closest(P, V, F)
    a, b, c, _ = D.triangles(V, F)
    for i in (0, 1):                                       # straight above the apex: every face at the same distance
        d = np.array([D.tri_dist2(P[i:i + 1].astype(np.float64), a[f], b[f], c[f])[0] for f in range(len(F))])
        assert (d == d[0]).all() and want[1][i] == 0
    right = X.closest_in_order(P, V, F, order)
    wrong = X.closest_in_order(P, V, F, order, tie="first")
    assert right[0].tobytes() == want[0].tobytes() and right[1].tobytes() == want[1].tobytes()
    assert wrong[0].tobytes() == want[0].tobytes() and (wrong[1][:2] == len(F) - 1).all()

    V, F, rays, pose = ray_trap()
    order = X.order_of(X.face_keys(V, F))
    o, d, _ = R.directions(pose, rays)
    want = R.cast(o, d, V, F, 0.0, 10.0)
    pair = [f for f in range(len(F)) if set(F[f]) <= {0, 1, 2, 3}]
    assert len(pair) == 2 and (want[0] == 1.0).all() and (want[1] == pair[0]).all()
    assert list(order).index(pair[1]) < list(order).index(pair[0])              # Morton order meets the higher one first
    right = X.cast_in_order(o, d, V, F, order, 0.0, 10.0)
    wrong = X.cast_in_order(o, d, V, F, order, 0.0, 10.0, tie="first")
    assert right[0].tobytes() == want[0].tobytes() and right[1].tobytes() == want[1].tobytes()
    assert (wrong[0] == 1.0).all() and (wrong[1] == pair[1]).all()


def test_subdivide_keeps_the_surface():
    from mast3r_slam import synthetic

    V, F = synthetic.room_mesh()
    V2, F2 = subdivide(V, F, 3)
    assert len(F2) == 64 * len(F) and abs(D.face_areas(V2, F2).sum() - D.face_areas(V, F).sum()) < 1e-4
