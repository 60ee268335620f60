"""GPU tests (-m gpu) of TSDFVolume.extract_mesh (csrc/tsdf_mesh.hip): parity with the numpy statement of the
algorithm (tests/mc_numpy.py) on volumes fused by the device integrate, analytic shapes loaded with load_voxels,
invariance (capacity, growth, repeated calls, voxel shards), edge cases, and the product path through SlamSystem.
Parity: V, F and faces exact; vertices / normals to 1e-6 absolute (both sides round the same f64 values to f32)."""
import os
import sys

import numpy as np
import pytest
import torch

from mast3r_slam import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M  # noqa: E402
from mesh_support import VS, _host, _room, _same, _vol  # noqa: E402

pytestmark = pytest.mark.gpu


def _match_numpy(mesh, keys, t, w, min_weight, level=0.0):
    V, N, F = _host(mesh)
    Vr, Nr, Fr = M.extract(keys, t, w, VS, min_weight, level)
    assert V.shape == Vr.shape and F.shape == Fr.shape
    assert np.array_equal(F, Fr)
    dv = float(np.abs(V - Vr).max()) if len(V) else 0.0
    dn = float(np.abs(N - Nr).max()) if len(N) else 0.0
    assert dv <= 1e-6 and dn <= 1e-6, (dv, dn)
    return dv, dn


def test_room_mesh_matches_numpy(device):
    vol = _vol(device)
    for pw, conf, org in _room():
        vol.integrate(pw, conf, org)
    keys, t, w = vol.voxels()
    mesh = vol.extract_mesh()
    assert mesh[0].is_cuda and mesh[0].dtype == torch.float32 and mesh[2].dtype == torch.int32
    assert mesh[2].shape[0] > 1000
    dv, dn = _match_numpy(mesh, keys, t, w, vol.min_weight)
    print(f"room parity: V={mesh[0].shape[0]} F={mesh[2].shape[0]} max|dv|={dv:.3g} max|dn|={dn:.3g}")
    # a higher weight threshold and another level follow the same rules
    _match_numpy(vol.extract_mesh(min_weight=0.5, level=0.1), keys, t, w, 0.5, 0.1)
    V, N, F = _host(mesh)
    assert np.array_equal(np.unique(F), np.arange(len(V)))


def _loaded(device, keys, t, w):
    from mast3r_slam.tsdf import mesh_from_voxels

    return mesh_from_voxels(keys, t, w, VS, 0.5, device=device)


@pytest.mark.parametrize("shape", ["sphere0", "sphere1", "sphere2", "torus"])
def test_analytic_shapes_are_closed(device, shape):
    if shape == "torus":
        k, v, w = M.sample_sdf(M.torus_sdf((0.01, 0.0, 0.0), 0.3, 0.1), (-0.45, -0.45, -0.15), (0.45, 0.45, 0.15), VS,
                               3 * VS)
        euler = 0
    else:
        c, r = [((0.0, 0.0, 0.0), 0.2), ((0.011, 0.004, -0.007), 0.13), ((0.3, -0.2, 0.1), 0.31)][int(shape[-1])]
        k, v, w = M.sample_sdf(M.sphere_sdf(c, r), np.array(c) - r, np.array(c) + r, VS, 3 * VS)
        euler = 2
    mesh = _loaded(device, k, v, w)
    _match_numpy(mesh, k, v, w, 0.5)
    V, N, F = _host(mesh)
    cnt, consistent = M.edge_use(F)
    assert (cnt == 2).all() and consistent
    assert M.euler(V, F) == euler
    assert (np.einsum("ij,ij->i", M.face_normals(V, F), N[F].mean(1)) > 0).all()


def test_invariant_to_capacity_growth_repeats_and_shards(device):
    from mast3r_slam.tsdf import mesh_from_voxels

    data = _room()
    big = _vol(device, 1 << 22)
    small = _vol(device, 1 << 14)
    shards = [_vol(device, 1 << 19, shard_id=r, num_shards=2) for r in range(2)]
    for pw, conf, org in data:
        small.maintain(reserve=len(pw) * 10)
        big.integrate(pw, conf, org)
        small.integrate(pw, conf, org)
        for s in shards:
            s.integrate(pw, conf, org, return_fused=False)
    assert 1 << 14 < small.capacity < big.capacity   # grown and rehashed; slots differ from the big table's
    ref = big.extract_mesh()
    before = big.voxels()
    _same(ref, small.extract_mesh())
    _same(ref, big.extract_mesh())                    # repeated call
    after = big.voxels()
    for x, y in zip(before, after):                   # extraction never writes the table
        assert np.array_equal(x, y)
    parts = [s.voxels() for s in shards]
    keys = np.concatenate([p[0] for p in parts])
    t = np.concatenate([p[1] for p in parts])
    w = np.concatenate([p[2] for p in parts])
    _same(ref, mesh_from_voxels(keys, t, w, VS, big.min_weight, device=device))


def test_edge_cases(device):
    empty = _vol(device, 1 << 10)
    for a in empty.extract_mesh():
        assert a.shape == (0, 3) and a.is_cuda
    one = _vol(device, 1 << 10)
    one.load_voxels(np.array([[1, 2, 3]]), np.array([-0.5]), np.array([1.0]))
    for a in one.extract_mesh():
        assert a.shape == (0, 3)
    c = np.zeros(3)
    k, v, w = M.sample_sdf(M.sphere_sdf(c, 0.2), c - 0.2, c + 0.2, VS, 3 * VS)
    vol = _vol(device, 1 << 16)
    vol.load_voxels(k, v, w)
    for a in vol.extract_mesh(min_weight=2.0):       # above every weight
        assert a.shape == (0, 3)
    # a slab whose middle layer sits exactly at the level: deterministic, and that layer counts as outside
    g = np.stack(np.meshgrid(np.arange(-4, 5), np.arange(-4, 5), np.arange(-3, 4), indexing="ij"), -1).reshape(-1, 3)
    sv = g[:, 2].astype(np.float64) * 0.25
    slab = _vol(device, 1 << 12)
    slab.load_voxels(g, sv, np.ones(len(g)))
    m1, m2 = slab.extract_mesh(), slab.extract_mesh()
    _same(m1, m2)
    _match_numpy(m1, g, sv, np.ones(len(g)), 1.0e-3)
    # t = 1 on every crossing edge: the vertices sit on the centres of the layer at the level (outside, inside below)
    assert np.allclose(m1[0].cpu().numpy()[:, 2], 0.5 * VS, rtol=0, atol=1e-7)
    # sizes that are not a multiple of the 256-thread block, on both outputs
    for r in (0.05, 0.07, 0.11):
        k, v, w = M.sample_sdf(M.sphere_sdf(c, r), c - r, c + r, VS, 3 * VS)
        mesh = _loaded(device, k, v, w)
        _match_numpy(mesh, k, v, w, 0.5)
        assert mesh[0].shape[0] % 256 or mesh[2].shape[0] % 256


def test_slam_system_mesh_and_ply(device, tmp_path, monkeypatch):
    from mast3r_slam import evaluate
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from test_slam_system_gpu import RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    try:
        system.run(_frames(list(range(0, 60, 3)), device))
        V, N, F = system.extract_mesh()
        n_v, n_f = evaluate.save_tsdf_mesh(tmp_path, "mesh.ply", system)
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    V, N, F = _host((V, N, F))
    assert len(F) > 100 and (n_v, n_f) == (len(V), len(F))
    H = synthetic.ROOM_HALF
    gap = np.abs(H[None] - np.abs(V.astype(np.float64)))
    near = gap.min(1) <= VS
    assert near.mean() >= 0.95, near.mean()
    a = np.argmin(gap, 1)
    inward = (N[np.arange(len(V)), a] * -np.sign(V[np.arange(len(V)), a])) > 0
    assert inward.mean() >= 0.95, inward.mean()
    print(f"slam mesh: V={len(V)} F={len(F)} within one voxel {near.mean():.4f} normals inward {inward.mean():.4f}")
    lines, vert, faces = M.parse_ply(tmp_path / "mesh.ply")
    assert np.array_equal(faces, F)
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), V)
    off = SlamSystem(RoomModel(device), device, tsdf_global_cfg=None)
    with pytest.raises(RuntimeError, match="global TSDF is disabled"):
        off.extract_mesh()
