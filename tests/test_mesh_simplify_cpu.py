"""CPU checks of the yardstick itself: tests/simplify_numpy.py (the numpy statement of simplify_mesh, DESIGN.md "Mesh
simplification") against answers written out by hand and against the figures measured with the numpy prototype on
marching-cubes meshes of a sphere, a torus and a box, and the entry points that exist without a device.

Out -> in distances: 2000 area-weighted samples of the simplified mesh (meshdist_numpy.sample, seed 1) against the input
mesh.  At c = 2 voxels the prototype gave, mean / quadric: sphere2 0.0049 / 0.0022, torus 0.0130 / 0.0072, box 0.0188 /
0.0067, all far below sqrt(3) c = 0.104."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M  # noqa: E402
import simplify_numpy as S  # noqa: E402


def _ulp_close(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and bool((np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))).all())


@pytest.mark.parametrize("name", sorted(S.HAND))
@pytest.mark.parametrize("colors", [False, True])
def test_hand_built_meshes(name, colors):
    h = S.HAND[name]
    mesh = S.hand_mesh(name, colors)
    mean = S.simplify(mesh, h["cell"], "mean", return_map=True)
    quad = S.simplify(mesh, h["cell"], "quadric", return_map=True, return_info=True)
    for out in (mean, quad[:-1]):
        assert len(out) == len(mesh) + 1
        assert out[2].dtype == np.int32 and out[2].tolist() == h["out_faces"]
        assert out[-1].dtype == np.int32 and out[-1].tolist() == h["vertex_map"]
        assert all(a.dtype == np.float32 and a.shape == (max(h["vertex_map"]) + 1, 3) for a in out[:2] + out[3:-1])
    want = h.get("positions", h.get("mean_positions"))
    if want is not None:
        assert np.array_equal(mean[0], np.array(want, np.float32))
    if "positions" in h:
        assert _ulp_close(quad[0], h["positions"])
    fb = quad[-1]["fallback"]
    if "fallback" in h:
        assert fb.tolist() == h["fallback"]
    assert np.array_equal(quad[0][fb], mean[0][fb])                 # the fallback is the mean, bit for bit
    assert np.array_equal(quad[1], mean[1])                         # normals and colours do not depend on the mode
    if colors:
        assert np.array_equal(quad[3], mean[3])
        vm = np.array(h["vertex_map"])
        for o in range(vm.max() + 1):                               # a mean of values in [0, 1]
            src = mesh[3][vm == o].astype(np.float64)
            assert np.abs(mean[3][o] - src.mean(0)).max() <= 1e-6


def test_face_order_and_vertex_numbering_do_not_matter():
    mesh = S.grid_patch(9, 11, seed=4)
    rng = np.random.default_rng(0)
    ref = S.simplify(mesh, 2.5, return_map=True)
    assert 0 < len(ref[2]) < len(mesh[2])
    shuffled = S.simplify(mesh[:2] + (mesh[2][rng.permutation(len(mesh[2]))],) + mesh[3:], 2.5, return_map=True)
    for a, b in zip(ref, shuffled):
        assert np.array_equal(a, b)
    perm = rng.permutation(len(mesh[0]))
    moved = S.simplify(S.renumber(mesh, perm), 2.5, return_map=True)
    assert np.array_equal(moved[2], ref[2]) and np.array_equal(moved[-1][perm], ref[-1])
    assert _ulp_close(moved[0], ref[0])


@pytest.mark.parametrize("name", sorted(S.SHAPES))
def test_analytic_shapes_reproduce_the_measured_table(name):
    n_v, n_f, out_v, out_f, euler = S.SHAPES[name][3:]
    mesh = S.shape_mesh(name)
    assert (len(mesh[0]), len(mesh[2])) == (n_v, n_f)
    c = 2 * S.VS
    worst = {}
    for position in ("mean", "quadric"):
        V, N, F, vmap, info = S.shape_reference(name, 2, position)
        assert (len(V), len(F)) == (out_v, out_f)
        cnt, consistent = M.edge_use(F)
        assert (cnt == 2).all() and consistent and M.euler(V, F) == euler
        assert np.array_equal(np.unique(F), np.arange(len(V))) and (vmap >= 0).all()
        assert len(np.unique(F, axis=0)) == len(F)
        # inside the cell's closed box, up to the f32 rounding of the output
        assert (np.abs(V.astype(np.float64) - info["x0"]) <= 0.5 * c + np.spacing(np.abs(V))).all()
        d = S.out_to_in((V, N, F), mesh, np.sqrt(3.0) * c)
        worst[position] = float(d.max())
        assert worst[position] <= np.sqrt(3.0) * c
    print(f"{name}: out->in max, mean {worst['mean']:.4f} / quadric {worst['quadric']:.4f}")
    info = S.shape_reference(name, 2, "quadric")[-1]
    if name == "torus":
        assert info["fallback"].sum() >= 1
    else:
        assert worst["quadric"] < worst["mean"]


@pytest.mark.parametrize("name,voxels", [(n, 2) for n in sorted(S.SHAPES)] + [("sphere2", 3)])
def test_no_eigenvalue_sits_on_the_threshold(name, voxels):
    """What makes the comparison of a Jacobi solver with eigh meaningful: no lambda_i / lambda_max within a relative 1e-6
    of the 1e-3 threshold, so both sides take the same directions."""
    lam = S.shape_reference(name, voxels, "quadric")[-1]["eig"]
    assert (lam[:, 2] > 0).all()
    ratio = lam / lam[:, 2:3]
    assert np.abs(ratio / S.EIG_REL - 1.0).min() > 1e-6


def test_sphere_at_three_voxels():
    V, N, F, vmap, info = S.shape_reference("sphere2", 3, "quadric")
    cnt, consistent = M.edge_use(F)
    assert (len(V), len(F)) == (192, 380) and (cnt == 2).all() and consistent and M.euler(V, F) == 2


def test_simplify_entry_points_exist_without_a_device():
    import torch

    import mslam_hip
    from mast3r_slam import tsdf
    from mast3r_slam.config import config

    assert callable(tsdf.simplify_mesh)
    # simplify_cell / simplify_position of the five export functions: test_mesh_chain_cpu.py
    assert config["tsdf_global"]["mesh_simplify_voxels"] == 0.0
    declared = mslam_hip.exported_symbols()
    for s in ("mslam_mesh_simplify_keys", "mslam_mesh_simplify_faces", "mslam_mesh_simplify_solve",
              "mslam_mesh_simplify_mark"):
        assert s in declared and hasattr(mslam_hip.lib(), s), s
    mesh = (torch.zeros(3, 3), torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32))
    for off in (None, 0, 0.0, -1.0):                                # off: the input tensors themselves
        assert all(a is b for a, b in zip(tsdf.simplify_mesh(mesh, off), mesh))
    out = tsdf.simplify_mesh(mesh, 0.0, return_map=True)
    assert all(a is b for a, b in zip(out, mesh)) and out[3].tolist() == [0, 1, 2]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsdf.simplify_mesh(mesh, 0.1)
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="cell_size must be finite"):
            tsdf.simplify_mesh(mesh, bad)
    with pytest.raises(ValueError, match="position must be"):
        tsdf.simplify_mesh(mesh, 0.1, position="median")
