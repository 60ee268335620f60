"""The definition of mesh smoothing (tests/smooth_numpy.py, DESIGN.md "Mesh smoothing") judged on its own, without a
device: what it does to a noisy sphere, to an open cap and to hand meshes whose results can be worked out by hand, its
invariances, and the vertex normals it recomputes.  tests/test_mesh_smooth_gpu.py then holds the kernels to it bit for
bit."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_numpy as S  # noqa: E402
import smooth_numpy as T  # noqa: E402


def _radial(V, c, r):
    d = np.linalg.norm(V.astype(np.float64) - c, axis=1)
    return float(np.sqrt(np.mean((d - r) ** 2))), float(d.mean())


@functools.lru_cache(maxsize=None)
def _sphere():
    return T.noisy_sphere()


def test_noisy_sphere():
    clean, noisy, c, r = _sphere()
    rms0, mean0 = _radial(noisy[0], c, r)
    out = T.smooth_positions(noisy[0], noisy[2], 10)
    rms1, mean1 = _radial(out, c, r)
    lap = T.smooth_positions(noisy[0], noisy[2], 20, lam=0.5, mu=0.0)
    _, mean_lap = _radial(lap, c, r)
    print(f"noisy sphere: rms {rms0:.3e} -> {rms1:.3e} ({rms1 / rms0:.3f}), mean radius {mean0:.5f} -> {mean1:.5f} "
          f"({(mean1 / mean0 - 1) * 100:+.3f} %), 20 Laplacian steps -> {mean_lap:.5f} "
          f"({(mean_lap / mean0 - 1) * 100:+.2f} %)")
    assert (len(noisy[0]), len(noisy[2])) == (2006, 4008)
    assert rms1 < 0.5 * rms0
    assert abs(mean1 / mean0 - 1.0) < 0.002
    assert mean_lap / mean0 - 1.0 < -0.03


def test_clean_sphere():
    clean, _, c, r = _sphere()
    rms0, _ = _radial(clean[0], c, r)
    out = T.smooth_positions(clean[0], clean[2], 10)
    rms1, _ = _radial(out, c, r)
    slide = float(np.linalg.norm(out.astype(np.float64) - clean[0], axis=1).max())
    print(f"clean sphere: rms {rms0:.3e} -> {rms1:.3e}, largest move {slide / S.VS:.3f} voxels")
    assert rms1 < 1e-3


def test_open_cap():
    V, N, F = T.sphere_cap()
    vclass, degree, _ = T.classify(F, len(V))
    rim, inner, unused = vclass == T.BOUNDARY, vclass == T.INTERIOR, vclass == T.ISOLATED
    assert int(rim.sum()) == 88 and inner.any() and unused.any()
    assert np.array_equal(~unused, np.isin(np.arange(len(V)), F))
    out = {m: T.smooth_positions(V, F, 10, boundary=m) for m in T.MODES}
    for m in T.MODES:
        assert np.array_equal(out[m][unused].view(np.uint32), V[unused].view(np.uint32)), m
        assert (out[m][inner] != V[inner]).any(1).all(), m
    assert np.array_equal(out["fixed"][rim].view(np.uint32), V[rim].view(np.uint32))
    for m in ("curve", "free"):
        assert (out[m][rim] != V[rim]).any(1).all(), m
    assert not np.array_equal(out["curve"][rim], out["free"][rim])
    # the rim of "curve" is a function of the rim alone
    moved = V.copy()
    moved[inner] += 0.01
    again = T.smooth_positions(moved, F, 1, mu=0.0, boundary="curve")
    once = T.smooth_positions(V, F, 1, mu=0.0, boundary="curve")
    assert np.array_equal(again[rim], once[rim])


def _classes(name):
    V, _, F = T.hand_mesh(name)
    return T.classify(F, len(V))


def test_triangle():
    V, _, F = T.hand_mesh("triangle")
    vclass, degree, n_edges = _classes("triangle")
    assert vclass.tolist() == [T.BOUNDARY] * 3 and degree.tolist() == [2, 2, 2] and n_edges == 3
    assert np.array_equal(T.smooth_positions(V, F, 3, boundary="fixed"), V)
    # free, one step of 0.5: every vertex goes half way to the midpoint of the other two; exact in binary here
    want = [[0.25, 0.25, 0.125], [0.5, 0.25, 0.125], [0.25, 0.5, 0.25]]
    assert T.smooth_positions(V, F, 1, lam=0.5, mu=0.0, boundary="free").tolist() == want
    assert T.smooth_positions(V, F, 1, lam=0.5, mu=0.0, boundary="curve").tolist() == want      # all edges are rim


def test_two_triangles():
    V, _, F = T.hand_mesh("two_triangles")
    vclass, degree, n_edges = _classes("two_triangles")
    assert vclass.tolist() == [T.BOUNDARY] * 4 and degree.tolist() == [2, 3, 3, 2] and n_edges == 5
    row_start, nbr, mult = T.adjacency(F, 4)
    assert nbr.tolist() == [1, 2, 0, 2, 3, 0, 1, 3, 1, 2] and mult.tolist() == [1, 1, 1, 2, 1, 1, 2, 1, 1, 1]
    free = T.smooth_positions(V, F, 1, lam=0.5, mu=0.0, boundary="free").astype(np.float64)
    curve = T.smooth_positions(V, F, 1, lam=0.5, mu=0.0, boundary="curve").astype(np.float64)
    # vertex 1: free averages 0, 2, 3; curve skips 2, which lies behind the shared (interior) edge
    p = V.astype(np.float64)
    assert np.allclose(free[1], p[1] + 0.5 * ((p[0] + p[2] + p[3]) / 3 - p[1]), rtol=0, atol=1e-7)
    assert np.array_equal(curve[1], p[1] + 0.5 * ((p[0] + p[3]) / 2 - p[1]))
    assert np.array_equal(curve[0], free[0])


def test_tetrahedron():
    V, _, F = T.hand_mesh("tetrahedron")
    vclass, degree, n_edges = _classes("tetrahedron")
    assert vclass.tolist() == [T.INTERIOR] * 4 and degree.tolist() == [3] * 4 and n_edges == 6
    g = V.astype(np.float64).mean(0)
    out = T.smooth_positions(V, F, 1, lam=0.5, mu=0.0).astype(np.float64)
    # x' - g = x - g + 0.5 (mean of the others - x) = (1 - 0.5 4/3) (x - g): a third of the way out
    assert np.allclose(out - g, (V - g) / 3.0, rtol=0, atol=1e-7)
    for m in T.MODES:
        assert np.array_equal(T.smooth_positions(V, F, 1, lam=0.5, mu=0.0, boundary=m), out.astype(np.float32))


def test_bow_tie_three_on_an_edge_duplicate():
    vclass, degree, n_edges = _classes("bow_tie")
    assert vclass.tolist() == [T.BOUNDARY] * 5 and degree.tolist() == [2, 2, 4, 2, 2] and n_edges == 6
    V, _, F = T.hand_mesh("three_on_an_edge")
    row_start, nbr, mult = T.adjacency(F, 5)
    assert mult[row_start[0]:row_start[1]].tolist() == [3, 1, 1, 1] and nbr[:4].tolist() == [1, 2, 3, 4]
    assert T.classify(F, 5)[0].tolist() == [T.BOUNDARY] * 5
    curve = T.smooth_positions(V, F, 1, lam=0.5, mu=0.0, boundary="curve").astype(np.float64)
    p = V.astype(np.float64)
    assert np.allclose(curve[0], p[0] + 0.5 * ((p[2] + p[3] + p[4]) / 3 - p[0]), rtol=0, atol=1e-7)     # not over 1
    V, _, F = T.hand_mesh("duplicated_face")
    assert T.adjacency(F, 3)[2].tolist() == [2] * 6
    assert T.classify(F, 3)[0].tolist() == [T.INTERIOR] * 3
    assert (T.smooth_positions(V, F, 1, boundary="fixed") != V).any(1).all()      # nothing is held: no boundary


def test_repeated_index_and_isolated_vertex():
    V, _, F = T.hand_mesh("repeated_index")
    assert T.counting(F, 4).tolist() == [True, False]
    vclass, degree, n_edges = T.classify(F, 4)
    assert vclass.tolist() == [T.BOUNDARY] * 3 + [T.ISOLATED] and degree.tolist() == [2, 2, 2, 0] and n_edges == 3
    one = T.hand_mesh("triangle")
    for m in T.MODES:
        out = T.smooth_positions(V, F, 2, boundary=m)
        assert np.array_equal(out[:3], T.smooth_positions(one[0], one[2], 2, boundary=m)) and np.array_equal(out[3], V[3])
    V, _, F = T.hand_mesh("isolated_vertex")
    assert T.classify(F, 5)[0].tolist() == [T.INTERIOR] * 4 + [T.ISOLATED]
    assert np.array_equal(T.smooth_positions(V, F, 5, boundary="free")[4], V[4])
    # indices out of range do not count either
    bad = np.array([[0, 1, 2], [0, 1, 7], [-1, 1, 2]], np.int32)
    assert T.counting(bad, 4).tolist() == [True, False, False]
    assert np.array_equal(T.smooth_positions(V[:4], bad, 2, boundary="free"),
                          T.smooth_positions(V[:4], bad[:1], 2, boundary="free"))


def test_fan():
    V, _, F = T.hand_mesh("fan")
    n = T.FAN_VALENCE
    vclass, degree, n_edges = T.classify(F, len(V))
    assert degree[0] == n and (degree[1:] == 3).all() and n_edges == 2 * n
    assert vclass.tolist() == [T.INTERIOR] + [T.BOUNDARY] * n
    out = T.smooth_positions(V, F, 1, lam=0.5, mu=0.0).astype(np.float64)
    p = V.astype(np.float64)
    assert np.allclose(out[0], p[0] + 0.5 * (p[1:].mean(0) - p[0]), rtol=0, atol=1e-7)
    assert np.array_equal(out[1:].astype(np.float32), V[1:])
    # the statement's own sum is the plain sequential one
    s = np.zeros(3)
    for u in range(1, n + 1):
        s = s + p[u]
    assert np.array_equal(out[0].astype(np.float32), (p[0] + 0.5 * (s / n - p[0])).astype(np.float32))


def test_mu_zero_and_no_iterations():
    _, noisy, _, _ = _sphere()
    V, N, F = noisy
    adj = T.adjacency(F, len(V))
    x = V.astype(np.float64)
    for _ in range(3):
        x = T.step(x, 0.5, adj, "fixed")
    assert np.array_equal(T.smooth_positions(V, F, 3, lam=0.5, mu=0.0), x.astype(np.float32))
    assert not np.array_equal(T.smooth_positions(V, F, 3, lam=0.5, mu=-0.53), x.astype(np.float32))
    for off in (0, None, -2):
        assert all(a is b for a, b in zip(T.smooth(noisy, off), noisy))
    kept = T.smooth(noisy, 2, normals="keep")
    assert kept[1] is N and kept[2] is F and not np.array_equal(kept[0], V)


def test_face_order_is_immaterial_and_vertex_order_is_not():
    _, noisy, _, _ = _sphere()
    rng = np.random.default_rng(3)
    first = T.smooth(noisy, 10)
    shuffled = noisy[:2] + (noisy[2][rng.permutation(len(noisy[2]))],)
    again = T.smooth(shuffled, 10)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
    # a renumbering reorders the neighbour sums: within the derived bound before the final rounding, so within one f32
    # spacing after it, and not bit for bit
    perm = rng.permutation(len(noisy[0]))
    moved = T.smooth(S.renumber(noisy, perm), 10)
    bound = T.renumber_bound(10, int(T.classify(noisy[2], len(noisy[0]))[1].max()), float(np.abs(noisy[0]).max()) * 2)
    assert bound < 1e-10
    diff = np.abs(moved[0][perm].astype(np.float64) - first[0].astype(np.float64))
    assert (diff <= np.spacing(np.abs(first[0])) + bound).all()
    print(f"renumbered sphere: {int((diff > 0).sum())} of {diff.size} coordinates differ, bound {bound:.2e}")
    # an input where the order shows: the spacing of f64 at 2^30 is 2^-22, so (2^30 + 2^-23) + 2^-23 loses both small
    # terms (ties to even) while (2^-23 + 2^-23) + 2^30 keeps their sum
    big, tiny = np.float32(2.0 ** 30), np.float32(2.0 ** -23)
    V = np.array([[0.0, 0.0, 0.0], [big, 0.0, 0.0], [tiny, 1.0, 0.0], [tiny, 0.0, 1.0]], np.float32)
    F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    adj = T.adjacency(F, 4)
    s_fwd = T.step(V.astype(np.float64), 1.0, adj, "free")[0, 0]     # (big + tiny) + tiny: each tiny is lost
    perm = np.array([0, 3, 1, 2])                                    # big is summed last
    Vp, _, Fp = S.renumber((V, V, F), perm)
    s_rev = T.step(Vp.astype(np.float64), 1.0, T.adjacency(Fp, 4), "free")[0, 0]
    assert s_fwd != s_rev and abs(s_fwd - s_rev) <= T.renumber_bound(1, 3, 2.0 ** 30, lam=1.0, mu=0.0)


@pytest.mark.parametrize("name", ["sphere2", "torus", "box"])
def test_normals_follow_the_winding(name):
    V, N, F = S.shape_mesh(name)
    got = T.vertex_normals(V, F)
    dots = (got.astype(np.float64) * N).sum(1)
    assert got.dtype == np.float32 and (dots > 0).all()
    assert np.allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, atol=1e-6)
    line = f"{name}: smallest dot product with the extracted normals {dots.min():.4f}"
    if name == "sphere2":
        d = V.astype(np.float64) - np.array([0.3, -0.2, 0.1])
        cos = (got * d).sum(1) / np.linalg.norm(d, axis=1)
        ang = np.degrees(np.arccos(np.clip(cos, -1, 1)))
        line += f"; angle to the radial direction: mean {ang.mean():.2f} deg, max {ang.max():.2f} deg"
        assert (cos > 0).all()
    print(line)


def test_normals_edge_cases():
    V, N, F = T.hand_mesh("repeated_index")
    got = T.vertex_normals(V, F, N)
    n = np.cross(V[1].astype(np.float64) - V[0], V[2].astype(np.float64) - V[0])
    assert np.array_equal(got[:3], np.tile((n / np.sqrt((n * n).sum())).astype(np.float32), (3, 1)))
    assert np.array_equal(got[3], N[3]) and np.array_equal(T.vertex_normals(V, F)[3], np.zeros(3, np.float32))
    flipped = T.vertex_normals(V, F[:, [0, 2, 1]], N)
    assert np.array_equal(flipped[:3], -got[:3])
    # opposite faces cancel: the zero vector, not NaN
    both = np.array([[0, 1, 2], [0, 2, 1]], np.int32)
    assert np.array_equal(T.vertex_normals(V, both, N)[:3], np.zeros((3, 3), np.float32))
    # a zero-area face counts for connectivity and adds nothing to the normal
    line = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]], np.float32)
    assert np.array_equal(T.vertex_normals(line, F[:1]), np.zeros((3, 3), np.float32))
    assert T.classify(F[:1], 3)[1].tolist() == [2, 2, 2]


def test_entry_points_exist_without_a_device():
    import torch

    import mslam_hip
    from mast3r_slam import tsdf
    from mast3r_slam.config import config

    assert callable(tsdf.smooth_mesh) and callable(tsdf.vertex_normals)
    # smooth_iterations / smooth_lambda / smooth_mu / smooth_boundary of the five export functions: test_mesh_chain_cpu.py
    assert config["tsdf_global"]["mesh_smooth_iterations"] == 0
    declared = mslam_hip.exported_symbols()
    for s in ("mslam_mesh_smooth_edges", "mslam_mesh_smooth_step", "mslam_mesh_vertex_faces",
              "mslam_mesh_vertex_normals"):
        assert s in declared and hasattr(mslam_hip.lib(), s), s
    c = mslam_hip.header_constants()
    assert [c["MSLAM_MESH_SMOOTH_" + k] for k in ("INTERIOR", "BOUNDARY", "ISOLATED")] == [T.INTERIOR, T.BOUNDARY,
                                                                                           T.ISOLATED]
    mesh = (torch.zeros(3, 3), torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32))
    for off in (None, 0, -1):
        assert tsdf.smooth_mesh(mesh, off) is mesh
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsdf.smooth_mesh(mesh, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsdf.vertex_normals(mesh[0], mesh[2])
    for bad in (1.5, "2", 2.0):
        with pytest.raises(ValueError, match="iterations must be an integer"):
            tsdf.smooth_mesh(mesh, bad)
    for kw in (dict(lam=float("nan")), dict(mu=float("inf"))):
        with pytest.raises(ValueError, match="lam and mu must be finite"):
            tsdf.smooth_mesh(mesh, 1, **kw)
    with pytest.raises(ValueError, match="boundary must be"):
        tsdf.smooth_mesh(mesh, 1, boundary="pinned")
    with pytest.raises(ValueError, match="normals must be"):
        tsdf.smooth_mesh(mesh, 1, normals="flat")
