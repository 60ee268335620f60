"""The definition of the boundary loops and of the hole filling (tests/holes_numpy.py, DESIGN.md "Mesh holes") judged on
its own, without a device: hand meshes whose boundary can be read off, a planar grid with one cell missing, a folded
loop, the edge cap, the face order, and marching-cubes spheres with voxels knocked out.  tests/test_mesh_holes_gpu.py
then holds the kernels to it bit for bit."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import holes_numpy as H  # noqa: E402
import mc_numpy as M  # noqa: E402

SPHERE_C, SPHERE_R, VS = np.array([0.3, -0.2, 0.1]), 0.31, 0.03


def _b(name):
    V, _, F = H.hand_mesh(name)
    return H.boundaries(F, len(V), V), H.fill(H.hand_mesh(name, True), 16, return_info=True)


def test_tetrahedron_is_watertight():
    b, out = _b("tetrahedron")
    assert b["n_boundary_edges"] == 0 and b["n_open"] == 0 and len(b["loop_id"]) == 0 and len(b["dart"]) == 0
    assert len(out[0]) == 4 and len(out[2]) == 4 and out[-1]["loop_filled"].shape == (0,)


def test_triangle_and_two_triangles_are_rims():
    b, out = _b("triangle")
    assert b["dart"].tolist() == [0, 1, 2] and b["dart_tail"].tolist() == [0, 1, 2] and b["dart_head"].tolist() == [1, 2, 0]
    assert b["loop_id"].tolist() == [0] and b["loop_length"].tolist() == [3] and b["dart_loop"].tolist() == [0, 0, 0]
    V = H.hand_mesh("triangle")[0].astype(np.float64)
    want = 0.0
    for a, c in ((0, 1), (1, 2), (2, 0)):
        d = V[c] - V[a]
        want = want + np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    assert b["loop_perimeter"].tolist() == [want]
    assert out[-1]["loop_filled"].tolist() == [False] and len(out[0]) == 3 and len(out[2]) == 1
    # the rim's fan is the triangle's flipped double cover: every product is negative
    tr = H.trace(H.hand_mesh("triangle")[2], 3)
    assert (H.fan_products(V, H.hand_mesh("triangle")[2], tr, tr["walks"][0]) < 0).all()
    b, out = _b("two_triangles")
    # faces (0, 1, 2), (1, 3, 2): the edge {1, 2} is shared, darts 1 and 5 are not boundary darts
    assert b["dart"].tolist() == [0, 2, 3, 4] and b["dart_tail"].tolist() == [0, 2, 1, 3]
    assert b["loop_id"].tolist() == [0] and b["loop_length"].tolist() == [4] and b["n_open"] == 0
    assert out[-1]["loop_filled"].tolist() == [False] and len(out[2]) == 2


def test_bow_tie_is_open():
    b, out = _b("bow_tie")
    assert b["n_boundary_edges"] == 6 and b["n_open"] == 6 and len(b["loop_id"]) == 0
    assert b["dart_loop"].tolist() == [-1] * 6
    assert len(out[0]) == 5 and len(out[2]) == 2
    # vertex 2 has two darts in and two out: the two that enter it have no successor, the other four do
    tr = H.trace(H.hand_mesh("bow_tie")[2], 5)
    assert sorted(tr["head"][tr["nxt"] < 0].tolist()) == [2, 2] and int((tr["nxt"] >= 0).sum()) == 4


def test_three_on_an_edge_duplicate_and_repeated_index():
    b, _ = _b("three_on_an_edge")
    assert b["n_boundary_edges"] == 6 and 0 not in b["dart"].tolist()          # dart 0 is 0 -> 1, m = 3
    assert {(min(a, c), max(a, c)) for a, c in zip(b["dart_tail"].tolist(), b["dart_head"].tolist())} == {
        (1, 2), (0, 2), (1, 3), (0, 3), (1, 4), (0, 4)}
    assert b["n_open"] == 6 and len(b["loop_id"]) == 0                         # vertices 0 and 1 are not simple
    b, _ = _b("duplicated_face")
    assert b["n_boundary_edges"] == 0 and b["n_open"] == 0 and len(b["loop_id"]) == 0
    b, out = _b("repeated_index")
    one, _ = _b("triangle")
    assert sorted(b) == sorted(one) and all(np.array_equal(b[k], one[k]) for k in b)
    assert len(out[0]) == 4 and len(out[2]) == 2


def test_grid_with_one_cell_removed():
    mesh = H.grid(5, 5, [(2, 2)])                                              # 6 x 6 vertices
    V, N, F, C = mesh
    out = H.fill(mesh, 16, return_info=True)
    info = out[-1]
    hole = 2 * 6 + 2
    assert info["loop_id"].tolist() == [0, hole] and info["loop_length"].tolist() == [20, 4]
    assert info["loop_filled"].tolist() == [False, True] and info["n_open"] == 0 and info["n_boundary_edges"] == 24
    assert info["loop_perimeter"].tolist() == [20.0, 4.0]
    assert out[0].dtype == np.float32 and out[2].dtype == np.int32
    assert out[0][:36].tobytes() == V.tobytes() and out[1][:36].tobytes() == N.tobytes()
    assert out[2][:len(F)].tobytes() == F.tobytes() and out[3][:36].tobytes() == C.tobytes()
    assert out[0].shape == (37, 3) and out[2].shape == (len(F) + 4, 3) and out[0][36].tolist() == [2.5, 2.5, 0.0]
    new = out[2][len(F):]
    # walk order from the loop id along the winding of the faces around the hole; fan face = (head, tail, centre)
    assert new[:, 2].tolist() == [36] * 4 and new[0, 1] == hole and new[:, 1].tolist() == np.roll(new[:, 0], 1).tolist()
    fn = M.face_normals(out[0], new)
    assert np.array_equal(fn, np.tile([0.0, 0.0, 0.5], (4, 1)))
    assert out[1][36].tolist() == [0.0, 0.0, 1.0]
    ring = [hole, hole + 1, hole + 7, hole + 6]
    assert sorted(new[:, 0].tolist()) == sorted(ring)
    assert np.allclose(out[3][36], C[ring].astype(np.float64).mean(0), rtol=0, atol=1e-7)
    cnt, consistent = M.edge_use(out[2])
    assert consistent and int((cnt == 1).sum()) == 20
    again = H.boundaries(out[2], 37)
    assert again["loop_id"].tolist() == [0] and again["loop_length"].tolist() == [20]
    # the rim is refused by the test, not by the cap
    assert H.fill(mesh, 100, return_info=True)[-1]["loop_filled"].tolist() == [False, True]


def test_one_folded_dart_refuses_the_loop():
    V, N, F, C = H.folded_ring()
    tr = H.trace(F, len(V))
    prod = H.fan_products(V.astype(np.float64), F, tr, tr["walks"][0])
    assert tr["loop_id"].tolist() == [0, 8] and len(prod) == 8 and int((prod <= 0).sum()) == 1
    out = H.fill((V, N, F, C), 16, return_info=True)
    assert out[-1]["loop_filled"].tolist() == [False, False] and len(out[0]) == len(V)
    flat = H.fill(H.ring(8), 16, return_info=True)
    assert flat[-1]["loop_filled"].tolist() == [True, False] and len(flat[0]) == 17 and len(flat[2]) == 16 + 8
    # a product of exactly zero (a degenerate fan face) does not pass: the centre lies on the line of the dart 1 -> 0
    V, N, F, C = H.ring(5)
    V = V.copy()
    V[:5] = [[1, 0, 0], [-1, 0, 0], [-2, -1, 0], [0, 3, 0], [2, -2, 0]]
    tr = H.trace(F, 10)
    prod = H.fan_products(V.astype(np.float64), F, tr, tr["walks"][0])
    assert H.centre(V.astype(np.float64), tr, tr["walks"][0]).tolist() == [0.0, 0.0, 0.0]
    assert (tr["tail"][tr["walks"][0][-1]], tr["head"][tr["walks"][0][-1]]) == (1, 0) and prod[-1] == 0.0
    assert int((prod == 0).sum()) == 1
    assert H.fill((V, N, F, C), 16, return_info=True)[-1]["loop_filled"].tolist() == [False, False]


@pytest.mark.parametrize("n", [3, 4, 9])
def test_max_edges_is_inclusive(n):
    mesh = H.ring(n)
    at = H.fill(mesh, n, return_info=True)
    below = H.fill(mesh, n - 1, return_info=True)
    assert at[-1]["loop_length"].tolist() == [n, n] and at[-1]["loop_filled"].tolist() == [True, False]
    assert below[-1]["loop_filled"].tolist() == [False, False] and len(below[0]) == 2 * n
    assert len(at[0]) == 2 * n + 1 and len(at[2]) == 3 * n
    for off in (None, 0, -1):
        assert all(a is b for a, b in zip(H.fill(mesh, off), mesh))


def test_face_order_is_immaterial():
    removed = [(1, 1), (3, 2), (5, 5), (6, 1)]
    mesh = H.grid(8, 7, removed, jitter=0.2, seed=4)
    first = H.fill(mesh, 16, return_info=True)
    assert first[-1]["loop_filled"].tolist() == [False] + [True] * 4
    perm = np.random.default_rng(5).permutation(len(mesh[2]))
    shuffled = mesh[:2] + (np.ascontiguousarray(mesh[2][perm]),) + mesh[3:]
    again = H.fill(shuffled, 16, return_info=True)
    nf = len(mesh[2])
    for k in (0, 1, 3):
        assert again[k].tobytes() == first[k].tobytes()
    assert again[2][nf:].tobytes() == first[2][nf:].tobytes() and again[2][:nf].tobytes() == shuffled[2].tobytes()
    for k in ("loop_id", "loop_length", "loop_filled", "loop_perimeter"):
        assert again[-1][k].tobytes() == first[-1][k].tobytes(), k
    # the darts are named by their faces, so they move with them
    assert np.array_equal(np.sort(first[-1]["dart_tail"]), np.sort(again[-1]["dart_tail"]))


@functools.lru_cache(maxsize=None)
def _sphere(seed):
    mesh = H.sphere_mesh(seed)
    return mesh, H.fill(mesh, 16, return_info=True)


def test_sphere_with_missing_voxels_is_closed():
    assert len(H.sphere_voxels(2)[0]) == 8282 and int((H.sphere_voxels(2)[2] == 0).sum()) == 40
    mesh, out = _sphere(2)
    info = out[-1]
    assert len(info["loop_id"]) == 16 and int(info["loop_length"].max()) == 11 and info["n_open"] == 0
    assert info["loop_filled"].all()
    assert len(out[0]) == len(mesh[0]) + 16 and len(out[2]) == len(mesh[2]) + int(info["loop_length"].sum())
    cnt, consistent = M.edge_use(out[2])
    assert consistent and (cnt == 2).all() and M.euler(out[0], out[2]) == 2
    after = H.boundaries(out[2], len(out[0]))
    assert after["n_boundary_edges"] == 0 and after["n_open"] == 0 and len(after["loop_id"]) == 0
    r = np.linalg.norm(out[0][len(mesh[0]):].astype(np.float64) - SPHERE_C, axis=1)
    print(f"sphere, seed 2: 16 loops of {sorted(info['loop_length'].tolist())} edges, centres at radius "
          f"{r.min():.4f} to {r.max():.4f}")
    assert (np.abs(r - SPHERE_R) < 0.5 * VS).all()
    nn = out[1][len(mesh[0]):].astype(np.float64)
    d = (out[0][len(mesh[0]):].astype(np.float64) - SPHERE_C) / r[:, None]
    assert ((nn * d).sum(1) > 0.9).all()                                       # the new normals point outwards
    # with a cap below the longest loop that one stays open
    capped = H.fill(mesh, 10, return_info=True)
    assert int(capped[-1]["loop_filled"].sum()) == 13
    assert H.boundaries(capped[2], len(capped[0]))["loop_length"].tolist() == [11, 11, 11]


@pytest.mark.parametrize("seed,n_open", [(0, 6), (3, 14)])
def test_open_darts_are_reported_and_left_alone(seed, n_open):
    mesh, out = _sphere(seed)
    info = out[-1]
    assert info["n_open"] == n_open and int((info["dart_loop"] < 0).sum()) == n_open
    assert info["n_boundary_edges"] == n_open + int(info["loop_length"].sum())
    after = H.boundaries(out[2], len(out[0]))
    left = int(info["loop_length"][~info["loop_filled"]].sum())
    assert after["n_open"] == n_open and after["n_boundary_edges"] == n_open + left
    open_edges = lambda b: sorted(zip(b["dart_tail"][b["dart_loop"] < 0].tolist(), b["dart_head"][b["dart_loop"] < 0].tolist()))
    assert open_edges(after) == open_edges(info)


def test_entry_points_exist_without_a_device():
    import torch

    import mslam_hip
    from mast3r_slam import tsdf
    from mast3r_slam.config import config

    assert callable(tsdf.fill_holes) and callable(tsdf.mesh_boundaries)
    # fill_holes of the five export functions, and the shape of their signatures: test_mesh_chain_cpu.py
    assert config["tsdf_global"]["mesh_fill_holes"] == 0
    declared = mslam_hip.exported_symbols()
    for s in ("keys", "mark", "darts", "link", "double", "loop_labels", "loop_assign", "measure", "emit"):
        assert "mslam_mesh_holes_" + s in declared and hasattr(mslam_hip.lib(), "mslam_mesh_holes_" + s), s
    for s in ("labels", "assign"):                                  # one loop finder serves both modes
        assert "mslam_mesh_holes_" + s not in declared and not hasattr(mslam_hip.lib(), "mslam_mesh_holes_" + s), s
    mesh = (torch.zeros(3, 3), torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32))
    for off in (None, 0, -1):
        assert tsdf.fill_holes(mesh, off) is mesh
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsdf.fill_holes(mesh, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsdf.mesh_boundaries(mesh[2], 3)
    for bad in (1.5, "2", 2.0):
        with pytest.raises(ValueError, match="fill_holes: max_edges must be an integer"):
            tsdf.fill_holes(mesh, bad)
