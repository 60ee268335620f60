#!/usr/bin/env python3
"""Event timing of the colour of the global TSDF (csrc/tsdf_color.hip) on a volume fused the way the product fuses it:
room keyframes along the synthetic trajectory, 40 000 points each (tsdf_global.max_points_per_kf), the config's voxel
size and truncation, maintain() before every fusion, colours = the room texture at the points.  Times, with HIP events
after warm-up, medians of repeated calls, for one further keyframe's points: (a) TSDFVolume.integrate without colour,
(b) the colour fusion alone, and their ratio; (c) sample_color for the hit points of a 384x512 view and for the
vertices of the volume's mesh.  Repeated calls fuse the same keyframe again (the voxels exist after the warm-up: the
state of a re-fusion).  Not part of bench.py.
    python tools/color_time.py 20 [--reps 20]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam-quality-dualtsdf_amd")]
import numpy as np
import torch

import mslam_hip as _m
from mast3r_slam import synthetic
from mast3r_slam.config import config
from mast3r_slam.tsdf import TSDFVolume
from mast3r_slam.tsdf.global_volume import hit_points, pinhole_rays

ap = argparse.ArgumentParser()
ap.add_argument("keyframes", type=int, nargs="+")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--points", type=int, default=40000)
ap.add_argument("--hw", type=int, nargs=2, default=(384, 512))
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = config["tsdf_global"]
vs, trunc = float(cfg["voxel_size"]), float(cfg["trunc_dist"])
band = int(2.0 * trunc / (0.5 * vs)) + 4
h, w = args.hw
print(f"voxel_size={vs} trunc={trunc} points/kf={args.points} view={h}x{w} device={torch.cuda.get_device_name(dev)}",
      flush=True)
L = _m.lib()


def texture(p):
    return np.stack((0.5 * (np.sin(3.1 * p[:, 0] + 1.7 * p[:, 1]) + 1.0), 0.5 * (np.sin(2.3 * p[:, 1] + 2.9 * p[:, 2]) + 1.0),
                     0.5 * (np.sin(4.1 * p[:, 2] + 1.3 * p[:, 0]) + 1.0)), 1).astype(np.float32)


def keyframe(i, step):
    T = synthetic.camera_pose(i * step)
    X = synthetic.render_pointmap(T, 192, 256).reshape(-1, 3)
    rng = np.random.default_rng(i)
    sel = rng.permutation(X.shape[0])[:args.points]
    pw = synthetic.sim3_act(T, X[sel]).astype(np.float32)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    return (t(pw, torch.float32), t(rng.uniform(0.5, 2.0, len(sel)), torch.float64), t(T[:3], torch.float32),
            t(texture(pw), torch.float32))


def timed(fn, reps):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


for n_kf in args.keyframes:
    vol = TSDFVolume(vs, trunc, cfg["max_weight"], cfg["min_tsdf_weight"], capacity=1 << 22, device=dev, color=True)
    step = 1000 // (n_kf + 1)
    for i in range(n_kf):
        pw, conf, org, rgb = keyframe(i, step)
        vol.maintain(reserve=args.points * band)
        vol.integrate(pw, conf, org, return_fused=False, colors=rgb)
    vol.maintain(reserve=args.points * band)
    pw, conf, org, rgb = keyframe(n_kf, step)
    n = pw.shape[0]

    def fuse_color():
        _m.check(L.mslam_tsdf_integrate_color(_m.ptr(vol._table), vol.capacity, _m.ptr(vol._color), _m.ptr(pw), _m.ptr(conf),
                                              _m.ptr(rgb), _m.ptr(org), n, vs, trunc, 0.5, _m.stream_ptr()),
                 "tsdf_integrate_color")

    a_med, a_min, a_max = timed(lambda: vol.integrate(pw, conf, org, return_fused=False), args.reps)
    b_med, b_min, b_max = timed(fuse_color, args.reps)
    voxels, cap = vol.maintain()
    print(f"keyframes={n_kf} voxels={voxels} capacity={cap} points={n}", flush=True)
    print(f"  (a) integrate_ms median={a_med:.3f} min={a_min:.3f} max={a_max:.3f}", flush=True)
    print(f"  (b) color_fuse_ms median={b_med:.3f} min={b_min:.3f} max={b_max:.3f}  ratio (b)/(a)={b_med / a_med:.3f}",
          flush=True)
    rays = pinhole_rays(synthetic.intrinsics(h, w), (h, w), dev)
    pose = torch.from_numpy(synthetic.camera_pose(5).astype(np.float32)).to(dev)
    rng_, _, hit = vol.render(pose, rays=rays)
    pts = hit_points(pose, rays, rng_)
    v_med, v_min, v_max = timed(lambda: vol.sample_color(pts), args.reps)
    print(f"  (c) sample_color view {h}x{w} hit_share={float(hit.float().mean()):.4f} ms median={v_med:.3f} min={v_min:.3f} "
          f"max={v_max:.3f}", flush=True)
    verts = vol.extract_mesh()[0]
    m_med, m_min, m_max = timed(lambda: vol.sample_color(verts), args.reps)
    print(f"  (c) sample_color mesh vertices={verts.shape[0]} ms median={m_med:.3f} min={m_min:.3f} max={m_max:.3f}",
          flush=True)
