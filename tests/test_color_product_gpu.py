"""GPU test (-m gpu) of the colour product path: a SlamSystem session on the procedural room (thread backend, stand-in
model, frames range(0, 60, 3)) whose frames carry the room texture as `uimg`, once with tsdf_global.color on and once
off.  The TSDF and the poses must not depend on the switch; the colour view at the newest keyframe must show the
texture; the writers must store the colours they were given."""
import os
import sys

import numpy as np
import pytest
import torch

from mast3r_slam import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import color_numpy as C  # noqa: E402
import render_numpy as R  # noqa: E402
from test_color_writers_cpu import read_ply  # noqa: E402
from test_slam_system_gpu import H, W, RoomModel  # noqa: E402
from mesh_support import color_checks  # noqa: E402

pytestmark = pytest.mark.gpu

KS = list(range(0, 60, 3))


def _texture_image(k):
    return 0.5 * (synthetic.render_rgb(synthetic.camera_pose(k), H, W).astype(np.float64).transpose(1, 2, 0) + 1.0)


def _frames(device):
    from mast3r_slam.frame import Frame

    return [Frame(i, torch.full((1, 3, H, W), k / 1000.0, device=device), torch.tensor([[H, W]]), torch.tensor([[H, W]]),
                  torch.from_numpy(_texture_image(k).astype(np.float32))) for i, k in enumerate(KS)]


def _session(device, color):
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem

    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18, color=color)
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    system.run(_frames(device))
    return system


def test_session_with_and_without_color(device, tmp_path, monkeypatch):
    from PIL import Image

    from mast3r_slam import evaluate
    from mast3r_slam.config import config

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    off = _session(device, False)
    try:
        off.drain()
        vox_off = off.tsdf_manager.volume.voxels()
        poses_off = [off.keyframes[i].T_WC.data.clone() for i in range(len(off.keyframes))]
        assert off.tsdf_manager.volume._color is None
        with pytest.raises(ValueError):
            off.render_view(colors=True)
    finally:
        off.shutdown()
    on = _session(device, True)
    try:
        view = on.render_view(colors=True)
        plain = on.render_view()
        vox_on = on.tsdf_manager.volume.voxels()
        poses_on = [on.keyframes[i].T_WC.data.clone() for i in range(len(on.keyframes))]
        kf = on.keyframes.last_keyframe()
        X = kf.X_canon.detach().reshape(H, W, 3).float()
        rays = (X / X.norm(dim=-1, keepdim=True).clamp_min(1.0e-12)).cpu().numpy()
        pose = kf.T_WC.data.reshape(8).cpu().numpy().astype(np.float32)
        k_last = KS[int(kf.frame_id)]
        V, F = evaluate.save_tsdf_mesh(tmp_path, "mesh.ply", on, colors=True)
        mesh = on.extract_mesh(colors=True)
        png = evaluate.save_color_view(tmp_path, "view.png", view[3], view[2])
    finally:
        on.shutdown()
    torch.cuda.synchronize()
    # the switch moves neither the TSDF nor the trajectory (the fusion draws the same random subsets)
    assert len(poses_on) == len(poses_off) > 1
    for a, b in zip(poses_on, poses_off):
        assert torch.equal(a, b)
    for a, b in zip(vox_on, vox_off):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert len(view) == 4 and len(plain) == 3
    for a, b in zip(view[:3], plain):
        assert torch.equal(a, b)
    rng, hit, rgb = view[0].cpu().numpy(), view[2].cpu().numpy(), view[3].cpu().numpy()
    assert rgb.shape == (H, W, 3) and hit.mean() > 0.5 and not rgb[~hit].any()
    # hit points in the session's world (the first camera's frame), then in the room's
    p64 = pose.astype(np.float64)
    pts = p64[:3] + (p64[7] * rng.astype(np.float64))[..., None] * R.ray_dirs(pose, rays).reshape(H, W, 3)
    room = synthetic.sim3_act(synthetic.camera_pose(KS[0]), pts)
    mx, mean = color_checks(rgb.astype(np.float64), hit, C.texture(room), _texture_image(k_last),
                            f"session view at keyframe of frame {k_last}")
    print(f"session colour view: max error {mx:.4f}, mean error {mean:.5f} (poses are estimates: the maximum is not bounded)")
    # writers
    vert, faces, _ = read_ply(tmp_path / "mesh.ply")
    assert (len(vert), len(faces)) == (V, F) == (mesh[0].shape[0], mesh[2].shape[0]) and V > 1000
    assert list(vert.dtype.names) == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    want = np.rint(255.0 * mesh[3].cpu().numpy().astype(np.float64)).astype(np.uint8)
    assert np.array_equal(np.stack([vert[c] for c in ("red", "green", "blue")], 1), want)
    assert np.array_equal(np.stack([vert[c] for c in "xyz"], 1), mesh[0].cpu().numpy())
    assert len(np.unique(want, axis=0)) > 100                    # a texture, not one grey
    img = np.asarray(Image.open(png))
    assert img.dtype == np.uint8 and np.array_equal(img, np.where(hit[..., None], np.rint(255.0 * rgb.astype(np.float64)), 0).astype(np.uint8))
