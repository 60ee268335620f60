"""The camera argument layer (mast3r_slam/tsdf/_view_args.py) on the CPU: what it accepts and refuses, and its f64 camera
arithmetic against numpy statements with exact equality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import color_numpy as C  # noqa: E402
import raycast_numpy as RC  # noqa: E402

from mast3r_slam.tsdf import _view_args as VA  # noqa: E402

POSE = [0.3, -0.2, 1.5, 0.1825742, 0.3651484, 0.5477226, 0.7302967, 1.25]
K = np.array([[9.6, 0.0, 7.5], [0.0, 9.1, 4.25], [0.0, 0.0, 1.0]])


class _Sim3:
    def __init__(self, data):
        self.data = data


def _poses(n, seed=0):
    g = np.random.default_rng(seed)
    p = g.normal(size=(n, 8))
    p[:, 3:7] /= np.linalg.norm(p[:, 3:7], axis=1, keepdims=True)
    p[:, 7] = g.uniform(0.5, 2.0, n)
    return p


def test_pose_arg_forms():
    want = torch.tensor(POSE, dtype=torch.float32)
    forms = [POSE, np.array(POSE), np.array(POSE, np.float32), torch.tensor(POSE, dtype=torch.float64),
             torch.tensor(POSE).reshape(1, 8), _Sim3(torch.tensor(POSE).reshape(1, 8))]
    for pose in forms:
        got = VA._pose_arg(pose, "t", "cpu")
        assert got.dtype == torch.float32 and tuple(got.shape) == (8,) and got.is_contiguous()
        assert torch.equal(got, want)
    for bad in (POSE[:7], np.zeros((2, 8)), torch.zeros(0)):
        with pytest.raises(ValueError, match="8 values"):
            VA._pose_arg(bad, "t", "cpu")


def test_poses_arg_forms():
    p = _poses(3)
    want = torch.from_numpy(p)
    for poses in (p, want, want.reshape(-1), [row for row in p], [torch.from_numpy(row) for row in p],
                  [_Sim3(torch.from_numpy(row).reshape(1, 8)) for row in p]):
        got = VA._poses_arg(poses, "t")
        assert tuple(got.shape) == (3, 8) and got.device.type == "cpu" and torch.equal(got.double(), want)
    # Python numbers become tensors of torch's default dtype, f32, as everywhere in torch
    assert torch.equal(VA._poses_arg(p.tolist(), "t").double(), want.float().double())
    assert torch.equal(VA._poses_arg(p.astype(np.float32), "t"), torch.from_numpy(p.astype(np.float32)))   # dtype kept
    empty = VA._poses_arg([], "t")
    assert tuple(empty.shape) == (0, 8)
    assert tuple(VA._poses_arg(np.zeros((0, 8)), "t").shape) == (0, 8)
    with pytest.raises(ValueError, match="poses"):
        VA._poses_arg(np.zeros((3, 7)), "t")


def test_K_arg():
    for k in (K, torch.from_numpy(K)):
        got = VA._K_arg(k, "t")
        assert all(type(x) is float for x in got) and got == (9.6, 9.1, 7.5, 4.25)
    for k in (torch.from_numpy(K).float(), K.tolist()):                   # Python numbers: torch's default dtype, f32
        assert VA._K_arg(k, "t") == (float(np.float32(9.6)), float(np.float32(9.1)), 7.5, 4.25)
    for bad in (K[:2], K.reshape(-1), np.zeros((3, 4)), np.zeros((1, 3, 3))):
        with pytest.raises(ValueError, match="K must be"):
            VA._K_arg(bad, "t")
    for v in (np.nan, np.inf, -np.inf):
        bad = K.copy()
        bad[1, 2] = v
        with pytest.raises(ValueError, match="finite"):
            VA._K_arg(bad, "t")


def test_hw_arg():
    assert VA._hw_arg((3, 5), "t") == (3, 5) and VA._hw_arg([1, 1], "t") == (1, 1)
    assert VA._hw_arg(torch.Size((4, 6)), "t") == (4, 6) and VA._hw_arg(np.array([4, 6]), "t") == (4, 6)
    for bad in (None, (0, 5), (5, 0), (-1, 5), (3, 5, 3), (3,)):
        with pytest.raises(ValueError, match="hw"):
            VA._hw_arg(bad, "t")


def test_range_arg():
    for strict in (False, True):
        assert VA._range_arg(0.05, 10, "t", strict) == (0.05, 10.0)
        for near, far in ((2.0, 1.0), (np.nan, 1.0), (0.0, np.nan)):
            with pytest.raises(ValueError, match="near"):
                VA._range_arg(near, far, "t", strict)
    assert VA._range_arg(1.0, 1.0, "t", False) == (1.0, 1.0)              # near == far: a legal shell of one distance
    assert VA._range_arg(0.0, np.inf, "t", False) == (0.0, np.inf)
    with pytest.raises(ValueError, match="far must be greater"):          # a march divides by the span
        VA._range_arg(1.0, 1.0, "t", True)
    with pytest.raises(ValueError, match="far must be greater"):
        VA._range_arg(0.0, np.inf, "t", True)


def test_eye():
    pose = torch.tensor(POSE, dtype=torch.float32)
    eye = VA._eye(pose)
    assert eye.dtype == torch.float32 and eye.is_contiguous()
    assert eye.tolist() == pose[:3].tolist() + [0.0, 0.0, 0.0, 1.0, 1.0]


def test_rotate_and_compose_exact():
    g = np.random.default_rng(1)
    p = _poses(5, seed=2)
    r = g.normal(size=(4, 7, 3))
    for q in p[:, 3:7]:
        got = VA.rotate(torch.from_numpy(q), torch.from_numpy(r))
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), RC.rotate(q, r))
        flat = VA.rotate(torch.from_numpy(q), torch.from_numpy(r.reshape(-1, 3)))
        assert np.array_equal(flat.numpy(), RC.rotate(q, r.reshape(-1, 3)))
        conj = q * np.array([-1.0, -1.0, -1.0, 1.0])                     # the negation is exact
        assert np.array_equal(VA.rotate(torch.from_numpy(conj), torch.from_numpy(r)).numpy(), RC.rotate(conj, r))
    T = _poses(1, seed=3)[0]
    got = VA.compose_sim3(T, torch.from_numpy(p))
    want = np.stack([RC.compose(T, row) for row in p])
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want)
    assert np.array_equal(VA.compose_sim3(torch.from_numpy(T).float(), torch.from_numpy(p).float()).numpy(),
                          np.stack([RC.compose(T.astype(np.float32), row.astype(np.float32)) for row in p]))
    assert tuple(VA.compose_sim3(T, torch.zeros((0, 8))).shape) == (0, 8)


def _pinhole_rays_numpy(K, hw):
    """((u - cx) / fx, (v - cy) / fy, 1) / its length, in f64, rounded to f32 once; pixel centres at integers."""
    h, w = hw
    K = np.asarray(K, np.float64)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    r = np.stack(((u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones((h, w))), -1)
    return (r / np.linalg.norm(r, axis=-1, keepdims=True)).astype(np.float32)


def test_pinhole_rays_and_hit_points_exact():
    for hw in ((9, 17), (1, 153), (16, 16), (3, 1)):
        rays = VA.pinhole_rays(K, hw, "cpu")
        assert rays.dtype == torch.float32 and tuple(rays.shape) == hw + (3,) and rays.is_contiguous()
        assert np.array_equal(rays.numpy(), _pinhole_rays_numpy(K, hw))
    rays = VA.pinhole_rays(K, (9, 17), "cpu")
    pose = torch.tensor(POSE, dtype=torch.float32)
    rng = torch.from_numpy(np.random.default_rng(4).uniform(0.0, 5.0, (9, 17)).astype(np.float32))
    rng[2, 3] = 0.0                                                       # a miss stays at the origin
    got = VA.hit_points(pose, rays, rng)
    assert got.dtype == torch.float32 and got.is_contiguous()
    assert np.array_equal(got.numpy(), C.hit_points(pose.numpy(), rays.numpy(), rng.numpy()))
    assert np.array_equal(got[2, 3].numpy(), pose[:3].numpy())


def test_public_names_stay_where_they_were():
    from mast3r_slam.tsdf import global_volume, mesh_raycast

    assert global_volume.pinhole_rays is VA.pinhole_rays and global_volume.hit_points is VA.hit_points
    assert mesh_raycast.compose_sim3 is VA.compose_sim3 and mesh_raycast._poses_arg is VA._poses_arg
