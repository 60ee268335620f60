"""CPU tests of the numpy statement of the bow-tie mode of the mesh holes (tests/bowtie_numpy.py, DESIGN.md "Mesh
holes"): the figures of the design's table, agreement with holes_numpy where no vertex is non-simple, and an independent
cut of the closed walks."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bowtie_numpy as BT  # noqa: E402
import holes_numpy as H  # noqa: E402

GRIDS = {
    "two diagonal": (lambda: H.grid(4, 4, [(1, 1), (2, 2)]), 24, [4, 4, 16], 16, 8),
    "three diagonal": (lambda: H.grid(5, 5, [(1, 1), (2, 2), (3, 3)], jitter=0.05), 32, [4, 4, 4, 20], 20, 12),
    "four around one": (lambda: H.grid(5, 5, [(1, 2), (2, 1), (2, 3), (3, 2)]), 36, [4, 12, 20], 24, 12),
    "corner": (lambda: H.grid(3, 3, [(0, 0), (1, 1)]), 16, [4, 12], None, None),
}
# seed: (B, loops, boundary darts after fill at cap 64, new faces)
SPHERES = {0: (598, 52, 289, 309), 1: (613, 58, 235, 378), 2: (598, 53, 218, 380)}


@functools.lru_cache(maxsize=None)
def _sphere(seed, n_removed=200):
    return H.sphere_mesh(seed, n_removed)


def _left(mesh):
    return len(H.boundary_darts(mesh[2], len(mesh[0]))[0])


def _edge_manifold(F):
    f = np.asarray(F, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    return int(np.unique(e, axis=0, return_counts=True)[1].max()) <= 2


@pytest.mark.parametrize("name", list(GRIDS))
def test_grids(name):
    make, B, lengths, left, new_faces = GRIDS[name]
    mesh = make()
    b = BT.boundaries(mesh[2], len(mesh[0]))
    assert b["n_boundary_edges"] == B and b["n_open"] == 0
    assert sorted(b["loop_length"].tolist()) == lengths
    assert int(H.boundaries(mesh[2], len(mesh[0]))["n_open"]) > 0
    if left is not None:
        out = BT.fill(mesh, 16)
        assert len(out[2]) - len(mesh[2]) == new_faces and _left(out) == left and _edge_manifold(out[2])
        assert _left(H.fill(mesh, 16)) == B


def test_two_diagonal_holes_leave_the_outer_rim():
    mesh = H.grid(4, 4, [(1, 1), (2, 2)])
    out = BT.fill(mesh, 16, return_info=True)
    assert out[-1]["loop_filled"].tolist() == [False, True, True] and out[-1]["loop_length"].tolist() == [16, 4, 4]
    b = BT.boundaries(out[2], len(out[0]))
    assert b["loop_length"].tolist() == [16] and b["n_open"] == 0 and b["loop_id"].tolist() == [0]
    rim = {v for v in range(25) if v // 5 in (0, 4) or v % 5 in (0, 4)}
    assert set(b["dart_tail"].tolist()) == rim


def test_hand_meshes():
    mesh = H.hand_mesh("bow_tie", True)
    b = BT.boundaries(mesh[2], len(mesh[0]))
    assert b["n_boundary_edges"] == 6 and b["n_open"] == 0 and b["loop_length"].tolist() == [3, 3]
    assert b["loop_id"].tolist() == [0, 2] and b["loop_head"].tolist() == [1, 4]
    assert H.boundaries(mesh[2], len(mesh[0]))["n_open"] == 6
    out = BT.fill(mesh, 16)
    assert len(out[2]) == len(mesh[2]) and _left(out) == 6                  # rims of patches, not holes
    mirrored = H.with_attributes(mesh[0][[2, 1, 0, 3, 4]], [[2, 1, 0], [0, 4, 3]])      # they share the smallest vertex
    b = BT.boundaries(mirrored[2], 5)
    assert b["loop_id"].tolist() == [0, 0] and b["loop_head"].tolist() == [2, 4] and b["n_open"] == 0
    mesh = H.hand_mesh("three_on_an_edge", True)
    b = BT.boundaries(mesh[2], len(mesh[0]))
    assert b["n_boundary_edges"] == 6 and b["n_open"] == 6 and b["loop_length"].shape == (0,)
    assert _left(BT.fill(mesh, 16)) == 6
    for name in H.HAND:
        mesh = H.hand_mesh(name, True)
        out = BT.fill(mesh, 16, return_info=True)
        assert out[-1]["n_open"] <= H.boundaries(mesh[2], len(mesh[0]))["n_open"], name


@pytest.mark.parametrize("seed", list(SPHERES))
def test_spheres(seed):
    B, loops, left, new_faces = SPHERES[seed]
    mesh = _sphere(seed)
    b = BT.boundaries(mesh[2], len(mesh[0]))
    assert b["n_boundary_edges"] == B and b["n_open"] == 0 and len(b["loop_id"]) == loops
    out = BT.fill(mesh, 64)
    assert len(out[2]) - len(mesh[2]) == new_faces and _left(out) == left and _edge_manifold(out[2])


def test_small_sphere():
    mesh = _sphere(0, 40)
    b = BT.boundaries(mesh[2], len(mesh[0]))
    assert b["n_boundary_edges"] == 173 and b["n_open"] == 0 and len(b["loop_id"]) == 20
    out = BT.fill(mesh, 64)
    assert len(out[2]) - len(mesh[2]) == 157 and _left(out) == 16 and _edge_manifold(out[2])


@pytest.mark.parametrize("name", ["ring", "strip", "grid", "sphere 1", "sphere 2"])
def test_equal_to_the_plain_statement_without_non_simple_vertices(name):
    mesh = {"ring": lambda: H.ring(7), "strip": lambda: H.strip(11), "grid": lambda: H.grid(4, 3),
            "sphere 1": lambda: _sphere(1, 40), "sphere 2": lambda: _sphere(2, 40)}[name]()
    nv = len(mesh[0])
    a, b = H.trace(mesh[2], nv), BT.trace(mesh[2], nv)
    assert (a["dart_loop"] >= 0).all()                                # no non-simple vertex: nothing is open
    assert a["walks"] == b["walks"] and np.array_equal(a["dart_loop"], b["dart_loop"])
    assert np.array_equal(a["loop_id"], b["loop_id"]) and np.array_equal(a["nxt"], b["nxt"])
    want, got = H.fill(mesh, 16, return_info=True), BT.fill(mesh, 16, return_info=True)
    for x, y in zip(want[:-1], got[:-1]):
        assert x.tobytes() == y.tobytes()
    assert set(got[-1]) == set(want[-1]) | {"loop_head"}
    for k in want[-1]:
        assert np.array_equal(want[-1][k], got[-1][k]), k


def test_re_pairing_against_a_stack_walk():
    meshes = [make() for make, *_ in GRIDS.values()] + [_sphere(s) for s in SPHERES] + [_sphere(0, 40)]
    for mesh in meshes:
        tr = BT.trace(mesh[2], len(mesh[0]))
        assert sum(len(w) for w in tr["closed"]) == len(tr["dart"])  # fan is a permutation
        assert BT.stack_cycles(tr) == {frozenset(w) for w in tr["walks"]}
        names = [(int(tr["loop_id"][l]), int(tr["loop_head"][l])) for l in range(len(tr["walks"]))]
        assert names == sorted(names) and len(set(names)) == len(names)
        for w in tr["walks"]:
            assert int(tr["tail"][w[0]]) == min(int(tr["tail"][d]) for d in w)
            assert all(int(tr["head"][a]) == int(tr["tail"][b]) for a, b in zip(w, w[1:] + w[:1]))


def test_bad_winding_and_the_other_fixtures():
    mesh = BT.bad_winding()
    b = BT.boundaries(mesh[2], len(mesh[0]))
    assert b["loop_length"].tolist() == [4, 4] and b["n_open"] == 16 and b["n_boundary_edges"] == 24
    for mesh, lengths in ((BT.gapped_fan(6, [0, 2, 4]), [3, 3, 3, 6]), (BT.two_sheets(), [8, 8]),
                          (BT.welded_rings(5), [5] * 4), (BT.diagonal_squares(3), [12, 12, 32]),
                          (BT.gapped_fan(40, [0, 20]), [3, 3, 40])):
        tr = BT.trace(mesh[2], len(mesh[0]))
        assert sorted(len(w) for w in tr["walks"]) == lengths and (tr["dart_loop"] >= 0).all()
        assert BT.stack_cycles(tr) == {frozenset(w) for w in tr["walks"]}
    tr = BT.trace(BT.gapped_fan(6, [0, 2, 4])[2], 13)
    assert sorted(len(w) for w in tr["closed"]) == [6, 9]             # the three gaps are one closed walk about vertex 0
    tr = BT.trace(BT.two_sheets()[2], 18)
    assert sorted(len(w) for w in tr["closed"]) == [8, 8] and np.array_equal(tr["nxt"], tr["fan"])


def test_face_order_and_corner_rotation():
    for mesh in (H.grid(5, 5, [(1, 2), (2, 1), (2, 3), (3, 2)]), _sphere(1)):
        a, b = BT.fill(mesh, 64, return_info=True), BT.fill(BT.reordered(mesh, 3), 64, return_info=True)
        nf = len(mesh[2])
        assert len(a[2]) > nf and a[2][nf:].tobytes() == b[2][nf:].tobytes()
        assert all(a[k].tobytes() == b[k].tobytes() for k in (0, 1))
        for k in ("loop_id", "loop_head", "loop_length", "loop_perimeter", "loop_filled"):
            assert a[-1][k].tobytes() == b[-1][k].tobytes(), k


def test_keywords_exist_without_a_device(tmp_path):
    import inspect

    import torch

    import mslam_hip
    from mast3r_slam import evaluate, tsdf
    from mast3r_slam.config import config

    assert config["tsdf_global"]["mesh_fill_bowties"] is False
    for fn in (tsdf.fill_holes, tsdf.mesh_boundaries):
        assert inspect.signature(fn).parameters["bowties"].default is False
    declared = mslam_hip.exported_symbols()
    for s in ("dkeys", "fan", "claim", "rank_init", "rank_double", "walk_keys", "pair_keys", "repair", "tail_keys",
              "tail_flag", "loop_labels", "loop_assign"):
        assert "mslam_mesh_holes_" + s in declared and hasattr(mslam_hip.lib(), "mslam_mesh_holes_" + s), s
    mesh = (torch.zeros(3, 3), torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32))
    for off in (None, 0, -1):
        assert tsdf.fill_holes(mesh, off, bowties=True) is mesh
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="fill_holes: bowties must be a bool"):
            tsdf.fill_holes(mesh, 16, bowties=bad)
        with pytest.raises(ValueError, match="mesh_boundaries: bowties must be a bool"):
            tsdf.mesh_boundaries(mesh[2], 3, bowties=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsdf.fill_holes(mesh, 16, bowties=True)

    class Source:
        def extract_mesh(self, **kw):
            self.kw = kw
            raise LookupError

    src = Source()
    for given, passed in ((dict(fill_holes=8), dict(fill_holes=8)),
                          (dict(fill_holes=8, fill_bowties=False), dict(fill_holes=8)),
                          (dict(fill_holes=8, fill_bowties=True), dict(fill_holes=8, fill_bowties=True)),
                          (dict(fill_bowties=True), {})):
        with pytest.raises(LookupError):
            evaluate.save_tsdf_mesh(tmp_path, "mesh.ply", src, **given)
        assert src.kw == dict(min_weight=None, level=0.0, **passed), given
    with pytest.raises(ValueError, match="save_tsdf_mesh: fill_bowties must be a bool"):
        evaluate.save_tsdf_mesh(tmp_path, "mesh.ply", src, fill_holes=8, fill_bowties="on")
    with pytest.raises(TypeError, match="unexpected keyword argument 'fill_bow_ties'"):
        evaluate.save_tsdf_mesh(tmp_path, "mesh.ply", src, fill_holes=8, fill_bow_ties=True)


def test_manager_and_system_pass_the_switch_on():
    """TSDFGlobalManager and SlamSystem hand fill_bowties on as they hand fill_holes on: only when it changes something,
    the system's default from tsdf_global.mesh_fill_bowties."""
    import types

    from mast3r_slam import tsdf
    from mast3r_slam.slam_system import SlamSystem

    calls = []
    volume = types.SimpleNamespace(voxel_size=0.03, extract_mesh=lambda **kw: calls.append(kw) or "mesh")
    manager = types.SimpleNamespace(volume=volume, cfg={})
    manager.extract_mesh = lambda **kw: tsdf.TSDFGlobalManager.extract_mesh(manager, **kw)
    base = dict(min_weight=None, level=0.0)
    for given, passed in ((dict(fill_holes=8), dict(colors=False, fill_holes=8)),
                          (dict(fill_holes=8, fill_bowties=False), dict(colors=False, fill_holes=8)),
                          (dict(fill_holes=8, fill_bowties=True), dict(colors=False, fill_holes=8, fill_bowties=True)),
                          (dict(fill_bowties=True), {}), ({}, {})):
        assert manager.extract_mesh(**given) == "mesh" and calls.pop() == dict(base, **passed), given
    with pytest.raises(ValueError, match="TSDFGlobalManager.extract_mesh: fill_bowties must be a bool"):
        manager.extract_mesh(fill_holes=8, fill_bowties="on")
    system = types.SimpleNamespace(tsdf_manager=manager, drain=lambda: None)
    for cfg, given, passed in (({}, {}, {}),
                               (dict(mesh_fill_holes=8), {}, dict(colors=False, fill_holes=8)),
                               (dict(mesh_fill_holes=8, mesh_fill_bowties=True), {},
                                dict(colors=False, fill_holes=8, fill_bowties=True)),
                               (dict(mesh_fill_holes=8, mesh_fill_bowties=True), dict(fill_bowties=False),
                                dict(colors=False, fill_holes=8)),
                               (dict(mesh_fill_holes=8), dict(fill_bowties=True),
                                dict(colors=False, fill_holes=8, fill_bowties=True)),
                               (dict(mesh_fill_bowties=True), {}, {}),
                               (dict(mesh_fill_bowties=True), dict(fill_holes=4),
                                dict(colors=False, fill_holes=4, fill_bowties=True))):
        manager.cfg = cfg
        assert SlamSystem.extract_mesh(system, **given) == "mesh" and calls.pop() == dict(base, **passed), (cfg, given)
