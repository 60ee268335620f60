"""CPU tests of the numpy statement of the mesh-quality definitions (tests/meshdist_numpy.py) against answers derived by
hand and against an independent formulation of the point-to-triangle distance, and of the host-side pieces: the room's
ground-truth mesh, the PLY reader and the metrics writer."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M  # noqa: E402
import meshdist_numpy as D  # noqa: E402

REL = 1e-12


def independent_dist2(p, a, b, c):
    """Another route to the same distance: the foot of the perpendicular when it lies inside the triangle (by the signs
    of three edge functions), else the least of the three point-to-segment distances.  p f64[n,3] -> dist2 f64[n]."""
    def segment(p, u, v):
        e = v - u
        t = np.clip(((p - u) @ e) / (e @ e), 0.0, 1.0)
        r = p - (u + t[:, None] * e)
        return (r * r).sum(1)

    n = np.cross(b - a, c - a)
    h = (p - a) @ n / (n @ n)
    foot = p - h[:, None] * n
    inside = np.ones(len(p), bool)
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= np.cross(v - u, foot - u) @ n >= 0.0
    edges = np.minimum(np.minimum(segment(p, a, b), segment(p, b, c)), segment(p, c, a))
    return np.where(inside, h * h * (n @ n), edges)


def independent_closest(points, vertices, faces):
    """(per-face dist2 f64[F,n]) over every face, no validity rule: the caller passes valid faces only."""
    p = np.asarray(points, np.float32).astype(np.float64)
    v = np.asarray(vertices, np.float32).astype(np.float64)
    return np.stack([independent_dist2(p, v[f[0]], v[f[1]], v[f[2]]) for f in faces])


def random_case(seed, n_points=200, n_faces=50):
    """Random triangles in the unit cube, the last ten on the 2^-10 grid, and random points, of which the first forty
    sit exactly on a vertex or on the midpoint of an edge of a grid triangle (exact in f32 and in every f64 step)."""
    rng = np.random.default_rng(seed)
    V = rng.uniform(0.0, 1.0, (3 * n_faces, 3)).astype(np.float32)
    V[-30:] = np.round(V[-30:] * 1024.0) / 1024.0
    F = np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)
    P = rng.uniform(-0.25, 1.25, (n_points, 3)).astype(np.float32)
    for i in range(40):
        f = F[n_faces - 10 + i % 10]
        k = (i // 10) % 3
        P[i] = V[f[k]] if i < 20 else (V[f[k]] + V[f[(k + 1) % 3]]) / np.float32(2.0)
    return P, V, F


def tie_share(P, V, F, d2, nearest):
    """Checks d2 / nearest against the independent formulation as the issue states it and returns the share of points
    whose face differs from the independent argmin (allowed when its distance is within REL of the minimum)."""
    ref = np.sqrt(independent_closest(P, V, F))
    want = ref.min(0)
    got = np.sqrt(d2)
    assert (np.abs(got - want) <= REL * np.maximum(got, want)).all(), np.abs(got - want).max()
    other = nearest != ref.argmin(0)
    at_got = ref[nearest, np.arange(len(P))]
    assert (np.abs(at_got - want) <= REL * want)[other].all()
    return other.mean()


def test_seven_regions_by_hand():
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    F = np.array([[0, 1, 2]], np.int32)
    cases = [((0.25, 0.25, 2.0), 2.0),               # interior: straight up
             ((-3.0, -4.0, 0.0), 5.0),               # vertex A
             ((2.0, -1.0, 0.0), np.sqrt(2.0)),       # vertex B
             ((-1.0, 2.0, 0.0), np.sqrt(2.0)),       # vertex C
             ((0.5, -2.0, 0.0), 2.0),                # edge AB
             ((-2.0, 0.5, 0.0), 2.0),                # edge AC
             ((2.0, 2.0, 0.0), np.sqrt(4.5))]        # edge BC: the midpoint (0.5, 0.5) is 1.5 sqrt(2) away
    P = np.array([c[0] for c in cases], np.float32)
    d2, nearest = D.closest(P, V, F)
    want = np.array([c[1] for c in cases])
    assert (nearest == 0).all()
    assert (np.abs(np.sqrt(d2) - want) <= 1e-15 * want).all(), np.sqrt(d2) - want


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_closest_against_independent_formulation(seed):
    """Both formulations carry an absolute error of about 1e-16 times the coordinates (of order 1 here), so their
    distances can agree to 1e-12 relative only for points farther than 1e-4 from the surface.  The seeds are the first
    three without a random point nearer than that: seed 0 has one at 1.6e-5, where the two differ by 9e-17 = 5.6e-12
    relative."""
    P, V, F = random_case(seed)
    d2, nearest = D.closest(P, V, F)
    assert (d2[:40] == 0.0).all()                    # on a vertex or an edge midpoint: exactly zero
    assert tie_share(P, V, F, d2, nearest) <= 0.01


def test_invalid_faces_are_never_chosen():
    P, V, F = random_case(5, 60, 12)
    line = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32)                       # collinear: exact zero cross
    V2 = np.concatenate([V, line])
    bad = np.array([[0, 0, 1], [3, 3, 3], [0, 1, len(V2)], [-1, 2, 3]], np.int32)       # zero area, out of range
    bad = np.concatenate([bad, [[len(V), len(V) + 1, len(V) + 2]]]).astype(np.int32)
    mixed = np.concatenate([bad[:2], F[:5], bad[2:4], F[5:], bad[4:]])
    keep = np.array([2, 3, 4, 5, 6] + list(range(9, 9 + len(F) - 5)))
    d2, nearest = D.closest(P, V2, mixed)
    r2, rn = D.closest(P, V, F)
    assert np.array_equal(d2, r2) and np.array_equal(nearest, keep[rn])
    assert (D.face_areas(V2, mixed)[np.setdiff1d(np.arange(len(mixed)), keep)] == 0.0).all()
    d2, nearest = D.closest(P, V2, bad)
    assert np.isinf(d2).all() and (nearest == -1).all()
    d2, nearest = D.closest(P, V2, np.zeros((0, 3), np.int32))
    assert np.isinf(d2).all() and (nearest == -1).all()


def test_sampler_is_stratified_and_reproducible():
    rng = np.random.default_rng(7)
    V = rng.uniform(-1.0, 2.0, (40, 3)).astype(np.float32)
    F = np.stack([rng.permutation(40)[:3] for _ in range(64)]).astype(np.int32)
    F[[0, 9, 33, 63]] = [[1, 1, 2], [4, 4, 4], [7, 8, 7], [5, 6, 6]]                     # zero area, first and last too
    area = D.face_areas(V, F)
    assert (area[[0, 9, 33, 63]] == 0.0).all() and (np.delete(area, [0, 9, 33, 63]) > 0.0).all()
    cdf = np.cumsum(area)
    for n in (1, 63, 1000, 4097):
        pts, face = D.sample(V, F, cdf, n, seed=3)
        assert pts.dtype == np.float32 and face.dtype == np.int32
        assert (np.diff(face) >= 0).all() and (area[face] > 0.0).all()
        counts = np.bincount(face, minlength=len(F))
        assert (np.abs(counts - n * area / cdf[-1]) <= 1.0 + 1e-9).all()
        # every point from its face and the hash
        r1, r2 = D.barycentrics(3, np.arange(n, dtype=np.uint64))
        assert (r1 >= 0).all() and (r2 >= 0).all() and (r1 + r2 <= 1.0).all()
        a, b, c = (V[F[face, k]].astype(np.float64) for k in range(3))
        want = (a + r1[:, None] * (b - a)) + r2[:, None] * (c - a)
        assert np.array_equal(pts, want.astype(np.float32))
        again, face2 = D.sample(V, F, cdf, n, seed=3)
        assert np.array_equal(pts, again) and np.array_equal(face, face2)
    other = D.sample(V, F, cdf, 1000, seed=4)[0]
    assert not np.array_equal(other, D.sample(V, F, cdf, 1000, seed=3)[0])
    # the hash, spelled out once with Python integers
    z = (3 + 6 * 0x9E3779B97F4A7C15) & D.MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & D.MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & D.MASK64
    assert int(D.hash64(3, np.array([5], np.uint64))[0]) == z ^ (z >> 31)


def test_room_mesh_is_closed_and_faces_inward():
    from mast3r_slam import synthetic

    V, F = synthetic.room_mesh()
    assert V.dtype == np.float32 and V.shape == (8, 3) and F.dtype == np.int32 and F.shape == (12, 3)
    assert np.array_equal(np.abs(V), np.broadcast_to(synthetic.ROOM_HALF, (8, 3)))
    cnt, consistent = M.edge_use(F)
    assert (cnt == 2).all() and consistent
    assert D.face_areas(V, F).sum() == 2.0 * (6 * 4 + 6 * 3 + 4 * 3)
    n = M.face_normals(V, F)
    centre = V[F].astype(np.float64).mean(1)
    assert (np.einsum("ij,ij->i", n, -centre) > 0).all()


def test_load_mesh_round_trips_save_mesh(tmp_path):
    from mast3r_slam import evaluate

    rng = np.random.default_rng(2)
    V = rng.normal(size=(37, 3)).astype(np.float32)
    N = rng.normal(size=(37, 3)).astype(np.float32)
    C = rng.uniform(size=(37, 3)).astype(np.float32)
    F = rng.integers(0, 37, (55, 3)).astype(np.int32)
    for name, kw in (("plain", {}), ("normals", dict(normals=N)), ("colors", dict(colors=C)),
                     ("both", dict(normals=N, colors=C))):
        path = tmp_path / f"{name}.ply"
        evaluate.save_mesh(path, V, F, **kw)
        v, f = evaluate.load_mesh(path)
        assert v.dtype == np.float32 and f.dtype == np.int32
        assert v.tobytes() == V.tobytes() and f.tobytes() == F.tobytes()
    evaluate.save_mesh(tmp_path / "empty.ply", V[:0], F[:0])
    v, f = evaluate.load_mesh(tmp_path / "empty.ply")
    assert v.shape == (0, 3) and f.shape == (0, 3)
    raw = (tmp_path / "plain.ply").read_bytes()
    (tmp_path / "uint.ply").write_bytes(raw.replace(b"uchar int vertex", b"uchar uint vertex"))
    assert np.array_equal(evaluate.load_mesh(tmp_path / "uint.ply")[1], F)
    (tmp_path / "ascii.ply").write_bytes(raw.replace(b"binary_little_endian", b"ascii"))
    with pytest.raises(ValueError, match="ASCII"):
        evaluate.load_mesh(tmp_path / "ascii.ply")
    quad = bytearray(raw)
    quad[len(raw) - 13 * len(F)] = 4                                                   # the first face's count
    (tmp_path / "quad.ply").write_bytes(bytes(quad))
    with pytest.raises(ValueError, match="triangle"):
        evaluate.load_mesh(tmp_path / "quad.ply")


def test_save_mesh_metrics_round_trips(tmp_path):
    from mast3r_slam import evaluate

    rng = np.random.default_rng(0)
    m = D.metrics(rng.uniform(0, 0.1, 101), rng.uniform(0, 0.2, 101), 0.05, 12.5, 108.0)
    assert m["chamfer"] == 0.5 * (m["accuracy"] + m["completion"]) and m["n_samples"] == 101
    assert m["fscore"] == 2 * m["precision"] * m["recall"] / (m["precision"] + m["recall"])
    assert D.metrics([1.0], [1.0], 0.5, 1.0, 1.0)["fscore"] == 0.0
    path = evaluate.save_mesh_metrics(tmp_path / "sub", "metrics.json", m)
    text = open(path).read()
    assert json.loads(text) == m
    keys = [ln.split('"')[1] for ln in text.splitlines() if '":' in ln]
    assert keys == sorted(m)
