"""What the mesh and render timing tools share: the room volume of profiles/mesh_time.log and the event timer.

The volume is fused the way the product fuses it: keyframes along the synthetic trajectory, `points` points each
(tsdf_global.max_points_per_kf is 40 000), the config's voxel size and truncation, the manager's maintain() before every
fusion.  One loop here, so that "the room of profiles/mesh_time.log" means one thing in every tool's log."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam-quality-dualtsdf_amd")]
import numpy as np
import torch

from mast3r_slam import synthetic
from mast3r_slam.config import config
from mast3r_slam.tsdf import TSDFVolume


def band(cfg):
    """Voxels a point may touch along its ray: what maintain() reserves per point."""
    return int(2.0 * float(cfg["trunc_dist"]) / (0.5 * float(cfg["voxel_size"]))) + 4


def build_room(n_kf, points, device):
    """The volume after n_kf keyframes; the caller's vol.maintain() returns (voxels, capacity)."""
    cfg = config["tsdf_global"]
    vol = TSDFVolume(float(cfg["voxel_size"]), float(cfg["trunc_dist"]), cfg["max_weight"], cfg["min_tsdf_weight"],
                     capacity=1 << 22, device=device)
    for i in range(n_kf):
        T = synthetic.camera_pose(i * (1000 // n_kf))
        X = synthetic.render_pointmap(T, 192, 256).reshape(-1, 3)
        rng = np.random.default_rng(i)
        sel = rng.permutation(X.shape[0])[:points]
        vol.maintain(reserve=points * band(cfg))
        vol.integrate(synthetic.sim3_act(T, X[sel]).astype(np.float32), rng.uniform(0.5, 2.0, len(sel)),
                      T[:3].astype(np.float32), return_fused=False)
    return vol


def timed_ms(fn, reps, prep=None):
    """HIP-event times in ms of `reps` calls of fn() after three warm-up calls; prep(), when given, runs before every
    call, outside the events."""
    ms = []
    for k in range(3 + reps):
        if prep is not None:
            prep()
        if k < 3:
            fn()
            continue
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def timed(fn, reps, prep=None):
    ms = timed_ms(fn, reps, prep)
    return f"median={float(np.median(ms)):.3f} min={min(ms):.3f} max={max(ms):.3f}"
