"""GPU test (-m gpu) of SlamSystem.evaluate_render on the session of tests/test_color_product_gpu.py (20 frames of the
procedural room, colour on): the figures equal the float64 definition (tests/imgmetrics_numpy.py) applied to the very
colour views and keyframe images, the held-out-view path gives the same bits, and the figures fall when the images are
replaced by their complements.  The session's figures are printed; no threshold is set on them (the poses are
estimates)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imgmetrics_numpy as M  # noqa: E402
from test_color_product_gpu import _session  # noqa: E402
from test_slam_system_gpu import H, W, RoomModel  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def session(device):
    from mast3r_slam.config import config

    mp = pytest.MonkeyPatch()
    mp.setitem(config["tracking"], "match_frac_thresh", 0.72)
    try:
        system = _session(device, True)
    finally:
        mp.undo()
    try:
        system.drain()
        yield system
    finally:
        system.shutdown()


def _views(system):
    """(poses f32[M,8], rays f32[M,H,W,3], images f32[M,H,W,3]) of the keyframes, device tensors."""
    poses, rays, images = [], [], []
    for i in range(len(system.keyframes)):
        kf = system.keyframes[i]
        X = kf.X_canon.detach().reshape(H, W, 3).float()
        rays.append(X / X.norm(dim=-1, keepdim=True).clamp_min(1.0e-12))
        poses.append(kf.T_WC.data.detach().reshape(8).clone())
        images.append(kf.uimg.detach().to(device=X.device, dtype=torch.float32))
    return torch.stack(poses), torch.stack(rays), torch.stack(images)


def _same(a, b):
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)       # NaN-safe, bit-exact for floats


def test_against_definition(session):
    got = session.evaluate_render()
    poses, rays, images = _views(session)
    n = len(session.keyframes)
    assert got["n_views"] == n > 1 and all(len(got["per_view"][k]) == n for k in ("psnr", "ssim", "n_pixels", "n_windows"))
    hits = 0
    for i in range(n):
        view = session.render_view(pose=poses[i], rays=rays[i], colors=True)
        hit, rgb = view[2].cpu().numpy(), view[3].cpu().numpy()
        ref = M.image_metrics(rgb[None], images[i].cpu().numpy()[None], hit[None])
        fb = M.figure_bounds(ref, 3)
        assert got["per_view"]["n_pixels"][i] == ref["n_pixels"][0] == hit.sum()
        assert got["per_view"]["n_windows"][i] == ref["n_windows"][0] > 0
        # psnr = -10 log10 mse: d psnr = 10 / ln 10 * d mse / mse
        tol = 10.0 / np.log(10.0) * fb["mse"][0] / ref["mse"][0] * 1.001 + 1e-12
        assert abs(got["per_view"]["psnr"][i] - ref["psnr"][0]) <= tol
        assert abs(got["per_view"]["ssim"][i] - ref["ssim"][0]) <= fb["ssim"][0]
        hits += int(hit.sum())
    pv = got["per_view"]
    assert got["hit_share"] == hits / (n * H * W) and got["window_share"] == sum(pv["n_windows"]) / (n * H * W)
    assert 0 < got["window_share"] <= got["hit_share"] <= 1      # a valid centre is itself a hit pixel
    assert got["psnr"] == sum(pv["psnr"]) / n and got["ssim"] == sum(pv["ssim"]) / n
    assert got["psnr_min"] == min(pv["psnr"]) and got["ssim_min"] == min(pv["ssim"])
    assert all(isinstance(got[k], float) for k in ("psnr", "ssim", "psnr_min", "ssim_min", "hit_share", "window_share"))
    print(f"session render quality over {n} keyframe views of {H}x{W}: psnr {got['psnr']:.3f} dB (min {got['psnr_min']:.3f}), "
          f"ssim {got['ssim']:.4f} (min {got['ssim_min']:.4f}), hit_share {got['hit_share']:.4f}, "
          f"window_share {got['window_share']:.4f}")
    # the figures do not depend on how the views are batched
    assert _same(got, session.evaluate_render(chunk=3)) and _same(got, session.evaluate_render(chunk=1))


def test_novel_view_path_and_complement(session):
    got = session.evaluate_render()
    poses, rays, images = _views(session)
    assert _same(got, session.evaluate_render(images=images, poses=poses, rays=rays))
    assert _same(got, session.evaluate_render(images=images.cpu().numpy(), poses=poses.cpu(), rays=rays))
    neg = session.evaluate_render(images=1.0 - images, poses=poses, rays=rays)
    assert neg["per_view"]["n_pixels"] == got["per_view"]["n_pixels"] and neg["n_views"] == got["n_views"]
    for a, b in zip(got["per_view"]["psnr"] + got["per_view"]["ssim"], neg["per_view"]["psnr"] + neg["per_view"]["ssim"]):
        assert a > b
    assert got["psnr"] > neg["psnr"] and got["ssim"] > neg["ssim"]
    with pytest.raises(ValueError, match="images need poses"):
        session.evaluate_render(images=images)
    with pytest.raises(ValueError, match="images need poses"):
        session.evaluate_render(images=images, poses=poses)
    with pytest.raises(ValueError, match="poses"):
        session.evaluate_render(images=images, poses=poses[:1], rays=rays)
    with pytest.raises(ValueError, match="go with images"):
        session.evaluate_render(poses=poses)


def test_writer(session, tmp_path):
    from mast3r_slam import evaluate

    got = session.evaluate_render()
    path = evaluate.save_render_metrics(tmp_path, "render.json", got)
    with open(path) as f:
        assert _same(json.load(f), got)


def test_disabled_configurations(device):
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem

    for tcfg, word in ((dict(config["tsdf_global"], enabled=True, hash_capacity=1 << 16, color=False), "colour"),
                       (dict(config["tsdf_global"], enabled=False), "disabled")):
        system = SlamSystem(RoomModel(device), device, tsdf_global_cfg=tcfg)
        try:
            with pytest.raises(RuntimeError, match=word):
                system.evaluate_render()
        finally:
            system.shutdown()
    system = SlamSystem(RoomModel(device), device,
                        tsdf_global_cfg=dict(config["tsdf_global"], enabled=True, hash_capacity=1 << 16, color=True))
    try:
        with pytest.raises(RuntimeError, match="no keyframe"):
            system.evaluate_render()
    finally:
        system.shutdown()
