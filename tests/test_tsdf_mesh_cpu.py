"""CPU tests (-m "not gpu") of the global-TSDF mesh extraction: the generated marching-cubes tables
(tools/gen_mc_tables.py -> csrc/mc_tables.h), the numpy statement of the extractor (tests/mc_numpy.py) on analytic SDFs
and on the oracle's fused room, and the mesh PLY writer.  Tolerances measured here:
* sphere / torus vertices lie within 0.05 voxel of the analytic surface (observed max 0.039 voxel);
* room vertices lie within 0.5 voxel of the box walls (observed max 0.46 voxel), every normal points into the room."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M  # noqa: E402
import gen_mc_tables as G  # noqa: E402  (tools/, put on the path by mc_numpy)

VS = 0.03


def test_committed_header_is_the_generator_output():
    assert open(G.HEADER).read() == G.render_header()


def test_every_case_triangulates_exactly_its_crossing_edges():
    edge_table, tri_table, tri_count = G.build_tables()
    assert max(tri_count) == 5
    for case in range(256):
        crossing = {e for e in range(12) if edge_table[case] >> e & 1}
        inside = {c for c in range(8) if case >> c & 1}
        expect = {e for e, (c, a) in enumerate(G.EDGES) if (c in inside) != ((c | (1 << a)) in inside)}
        assert crossing == expect, case
        used = {e for t in tri_table[case] for e in t}
        assert used == crossing, case
        for t in tri_table[case]:
            assert len(set(t)) == 3, (case, t)
        assert tri_count[case] == len(tri_table[case])
    assert tri_count[0] == tri_count[255] == 0


def test_ambiguous_faces_resolve_from_the_face_signs_alone():
    """The segments a face contributes (undirected) are a function of that face's four corner signs: two cubes that
    share the face draw the same segments, so the mesh has no cracks.  The loops are exactly the face segments."""
    seen = {}
    n_ambiguous = 0
    for case in range(256):
        loops = G.case_loops(case)
        loop_pairs = {(lp[i], lp[(i + 1) % len(lp)]) for lp in loops for i in range(len(lp))}
        face_pairs = set()
        for fi, (n, cyc) in enumerate(G.FACES):
            segs, amb = G.face_segments(case, (n, cyc))
            n_ambiguous += amb
            signs = tuple(case >> c & 1 for c in cyc)
            und = frozenset(frozenset(s) for s in segs)
            assert seen.setdefault((fi, signs), und) == und, (case, fi)
            face_pairs |= set(segs)
        assert loop_pairs == face_pairs, case
    assert n_ambiguous > 0
    # the same sign pattern on opposite faces (one cube's +axis face is its neighbour's -axis face) gives the same
    # segments, edge for edge, once the edges are mapped across
    for axis in range(3):
        lo, hi = G.FACES[2 * axis], G.FACES[2 * axis + 1]
        shift = {G.edge_between(a, b): G.edge_between(a | (1 << axis), b | (1 << axis))
                 for a, b in [(lo[1][i], lo[1][(i + 1) % 4]) for i in range(4)]}
        for signs in range(16):
            s_lo = seen[(2 * axis, tuple(signs >> i & 1 for i in range(4)))]
            s_hi = seen[(2 * axis + 1, tuple(signs >> i & 1 for i in range(4)))]
            assert frozenset(frozenset(shift[e] for e in s) for s in s_lo) == s_hi


def _check_closed(V, N, F, euler, degenerate_ok=False):
    assert len(F) > 0
    cnt, consistent = M.edge_use(F)
    assert (cnt == 2).all(), "not a closed 2-manifold"
    assert consistent, "neighbouring faces wind inconsistently"
    assert M.euler(V, F) == euler
    assert np.array_equal(np.unique(F), np.arange(len(V))), "unreferenced vertex"
    fn = M.face_normals(V, F)
    dots = np.einsum("ij,ij->i", fn, N[F].mean(1))
    if degenerate_ok:   # a corner exactly at the level puts several vertices on it: zero-area faces
        dots = dots[np.linalg.norm(fn, axis=1) > 0]
    assert (dots > 0).all(), "winding disagrees with the normals"


@pytest.mark.parametrize("center,radius", [((0.0, 0.0, 0.0), 0.2), ((0.011, 0.004, -0.007), 0.13),
                                           ((0.3, -0.2, 0.1), 0.31), ((0.005, 0.005, 0.005), 0.0801)])
def test_sphere_is_closed_outward_and_accurate(center, radius):
    c = np.asarray(center)
    k, v, w = M.sample_sdf(M.sphere_sdf(c, radius), c - radius, c + radius, VS, 3 * VS)
    V, N, F = M.extract(k, v, w, VS, 0.5)
    _check_closed(V, N, F, 2)
    ctr = M.face_normals(V, F)
    assert (np.einsum("ij,ij->i", ctr, V[F].mean(1) - c) > 0).all(), "faces must wind outward"
    radial = V - c
    err = np.abs(np.linalg.norm(radial, axis=1) - radius)
    assert err.max() < 0.05 * VS
    cosang = np.einsum("ij,ij->i", N, radial / np.linalg.norm(radial, axis=1, keepdims=True))
    assert cosang.min() > 0.95
    assert np.allclose(np.linalg.norm(N, axis=1), 1.0, atol=1e-6)


def test_torus_is_closed_genus_one():
    k, v, w = M.sample_sdf(M.torus_sdf((0.01, 0.0, 0.0), 0.3, 0.1), (-0.45, -0.45, -0.15), (0.45, 0.45, 0.15), VS, 3 * VS)
    V, N, F = M.extract(k, v, w, VS, 0.5)
    _check_closed(V, N, F, 0)
    q = V.astype(np.float64) - (0.01, 0.0, 0.0)
    err = np.abs(np.sqrt((np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2) - 0.3) ** 2 + q[:, 2] ** 2) - 0.1)
    assert err.max() < 0.05 * VS


def test_validity_level_and_order_rules():
    c = np.array([0.0, 0.0, 0.0])
    k, v, w = M.sample_sdf(M.sphere_sdf(c, 0.2), c - 0.2, c + 0.2, VS, 3 * VS)
    V, N, F = M.extract(k, v, w, VS, 0.5)
    # input order does not matter
    p = np.random.default_rng(0).permutation(len(k))
    V2, N2, F2 = M.extract(k[p], v[p], w[p], VS, 0.5)
    assert np.array_equal(V, V2) and np.array_equal(N, N2) and np.array_equal(F, F2)
    # a corner below min_weight is no corner: nothing survives a threshold above every weight
    assert all(a.shape == (0, 3) for a in M.extract(k, v, w, VS, 2.0))
    # a value equal to the level counts as outside: the shell moves but stays closed
    Vl, Nl, Fl = M.extract(k, v, w, VS, 0.5, level=float(v[np.argmin(np.abs(v - 0.01))]))
    _check_closed(Vl, Nl, Fl, 2, degenerate_ok=True)


def test_room_mesh_from_the_oracle_lies_on_the_walls():
    import oracle
    from mast3r_slam import synthetic

    ref = oracle.TSDFVolume(VS, 0.12)
    for kf in range(3):
        T = synthetic.camera_pose(kf * 10)
        X = synthetic.render_pointmap(T, 96, 128).reshape(-1, 3)
        rng = np.random.default_rng(kf)
        ref.integrate(synthetic.sim3_act(T, X).astype(np.float32), rng.uniform(0.5, 2.0, len(X)),
                      T[:3].astype(np.float32))
    k, t, w = ref.voxels()
    V, N, F = M.extract(k, t, w, VS, 1.0e-3)
    assert len(F) > 1000
    H = synthetic.ROOM_HALF
    gap = np.abs(H[None] - np.abs(V.astype(np.float64)))
    assert gap.min(1).max() < 0.5 * VS
    a = np.argmin(gap, 1)
    inward = -np.sign(V[np.arange(len(V)), a])
    assert (N[np.arange(len(V)), a] * inward > 0).mean() >= 0.99
    cnt, consistent = M.edge_use(F)
    assert consistent and cnt.max() == 2


def test_mesh_ply_round_trip(tmp_path):
    from mast3r_slam import evaluate

    rng = np.random.default_rng(1)
    v = rng.normal(size=(7, 3)).astype(np.float32)
    n = rng.normal(size=(7, 3)).astype(np.float32)
    f = rng.integers(0, 7, size=(5, 3)).astype(np.int32)
    evaluate.save_mesh(tmp_path / "m.ply", v, f, normals=n)
    lines, vert, faces = M.parse_ply(tmp_path / "m.ply")
    assert lines[2:] == ["element vertex 7", "property float x", "property float y", "property float z",
                         "property float nx", "property float ny", "property float nz", "element face 5",
                         "property list uchar int vertex_indices", "end_header"]
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), v)
    assert np.array_equal(np.stack([vert["nx"], vert["ny"], vert["nz"]], 1), n)
    assert np.array_equal(faces, f)
    evaluate.save_mesh(tmp_path / "p.ply", v, f)
    lines, vert, faces = M.parse_ply(tmp_path / "p.ply")
    assert vert.dtype.names == ("x", "y", "z") and np.array_equal(faces, f)
    evaluate.save_mesh(tmp_path / "e.ply", np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    lines, vert, faces = M.parse_ply(tmp_path / "e.ply")
    assert len(vert) == 0 and faces.shape == (0, 3)


def test_mesh_entry_points_exist_without_a_device():
    import mslam_hip
    from mast3r_slam import evaluate
    from mast3r_slam.slam_system import SlamSystem
    from mast3r_slam.tsdf import TSDFGlobalManager, TSDFVolume, mesh_from_voxels

    assert callable(mesh_from_voxels) and callable(evaluate.save_tsdf_mesh)
    for cls, name in [(TSDFVolume, "extract_mesh"), (TSDFVolume, "load_voxels"), (TSDFGlobalManager, "extract_mesh"),
                      (SlamSystem, "extract_mesh")]:
        assert callable(getattr(cls, name)), name
    L = mslam_hip.lib()
    assert L.mslam_tsdf_mesh_workspace_bytes(1 << 20) >= 8 * (1 << 20)
    assert L.mslam_tsdf_mesh_workspace_bytes(1000) == 0
