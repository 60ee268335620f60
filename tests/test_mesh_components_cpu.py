"""CPU checks of the yardstick itself: tests/cc_numpy.py (the numpy statement of mesh_components / filter_mesh) against
answers written out by hand, and the entry points that exist without a device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cc_numpy as C  # noqa: E402


@pytest.mark.parametrize("name", sorted(C.HAND))
def test_hand_built_meshes(name):
    faces, V, root, cfaces, cverts = C.HAND[name]
    assert C.labels(faces, V).tolist() == root
    vc, fc, cf, cv = C.components(faces, V)
    assert cf.tolist() == cfaces and cv.tolist() == cverts
    assert vc.dtype == fc.dtype == cf.dtype == cv.dtype == np.int32
    roots = sorted(set(root))
    assert vc.tolist() == [roots.index(r) for r in root]            # dense ids in the order of the smallest index
    assert fc.tolist() == [roots.index(root[f[0]]) for f in faces.tolist()]
    assert cf.sum() == len(faces) and cv.sum() == V


def test_strips_are_one_component_in_any_numbering():
    s = C.strip(5000)
    n = 5002
    rng = np.random.default_rng(0)
    for relabel in (np.arange(n), np.arange(n)[::-1], rng.permutation(n)):
        f = relabel[s].astype(np.int32)
        assert (C.labels(f, n) == 0).all()
        assert np.array_equal(C.labels(f[rng.permutation(len(f))], n), C.labels(f, n))
    two = np.concatenate([s[:100], s[102:]])                        # cutting faces 100 and 101 splits the strip
    root = C.labels(two, n)
    assert (root[:102] == 0).all() and (root[102:] == 102).all()
    assert C.components(two, n)[2].tolist() == [100, 4898]


def test_filter_by_hand():
    V = np.arange(21, dtype=np.float32).reshape(7, 3)
    N = -V
    col = V + 0.5
    faces = C.HAND["unreferenced"][0]
    for mesh in ((V, N, faces), (V, N, faces, col)):
        out = C.filter_mesh(mesh)                                   # off: the input itself
        assert all(a is b for a, b in zip(out, mesh))
        out = C.filter_mesh(mesh, min_faces=1)                      # drops vertex 2, the zero-face component
        kv = [0, 1, 3, 4, 5, 6]
        assert len(out) == len(mesh)
        assert np.array_equal(out[0], V[kv]) and np.array_equal(out[1], N[kv])
        assert out[2].dtype == np.int32 and out[2].tolist() == [[0, 1, 2], [3, 4, 5]]
        assert len(mesh) == 3 or np.array_equal(out[3], col[kv])
        out = C.filter_mesh(mesh, keep_largest=1)                   # a tie of one face each: the lower id stays
        assert np.array_equal(out[0], V[[0, 1, 3]]) and out[2].tolist() == [[0, 1, 2]]
        out = C.filter_mesh(mesh, min_faces=2)
        assert out[0].shape == (0, 3) and out[2].shape == (0, 3)
    f2 = np.array([[0, 1, 2], [3, 4, 5], [4, 5, 6], [7, 8, 9], [8, 9, 10], [9, 10, 11]], np.int32)
    assert C.components(f2, 12)[2].tolist() == [1, 2, 3]
    assert C.keep_mask([1, 2, 3], 2).tolist() == [False, True, True]
    assert C.keep_mask([1, 2, 3], 0, 1).tolist() == [False, False, True]
    assert C.keep_mask([3, 1, 3], 2, 1).tolist() == [True, False, False]
    assert C.keep_mask([3, 1, 3], 0, 5).tolist() == [True, True, True]
    assert C.keep_mask([3, 1, 3], 0, 0).tolist() == [False, False, False]


def test_component_entry_points_exist_without_a_device():
    import torch

    import mslam_hip
    from mast3r_slam import tsdf
    from mast3r_slam.config import config

    assert callable(tsdf.mesh_components) and callable(tsdf.filter_mesh)
    # min_component_faces / keep_largest of the five export functions: test_mesh_chain_cpu.py
    assert config["tsdf_global"]["mesh_min_component_faces"] == 0
    declared = mslam_hip.exported_symbols()
    for s in ("mslam_mesh_cc_label", "mslam_mesh_cc_count", "mslam_mesh_cc_select", "mslam_mesh_cc_emit"):
        assert s in declared and hasattr(mslam_hip.lib(), s), s
    # off: the input tensors themselves, before anything touches a device
    mesh = (torch.zeros(3, 3), torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32))
    assert all(a is b for a, b in zip(tsdf.filter_mesh(mesh), mesh))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsdf.filter_mesh(mesh, min_faces=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsdf.mesh_components(mesh[2], 3)
    with pytest.raises(ValueError, match=r"faces must be \(F,3\)"):
        tsdf.mesh_components(torch.zeros(4, dtype=torch.int32), 3)
