#!/usr/bin/env python3
"""Event timing of TSDFVolume.extract_mesh (csrc/tsdf_mesh.hip) on volumes fused the way the product fuses them: room
keyframes along the synthetic trajectory, 40 000 points each (tsdf_global.max_points_per_kf), the config's voxel size
and truncation, the manager's maintain() before every fusion.  Prints voxels, V, F, the median time of an extraction
(the sort, the kernels and the one host read of the output sizes) and the occupied-slot bytes (key, tsdf, weight, state:
25 B per voxel) read per ms.  Not part of bench.py.
    python tools/mesh_time.py 60 400 [--reps 10]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam-quality-dualtsdf_amd")]
import numpy as np
import torch

from mast3r_slam import synthetic
from mast3r_slam.config import config
from mast3r_slam.tsdf import TSDFVolume

ap = argparse.ArgumentParser()
ap.add_argument("keyframes", type=int, nargs="+")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--points", type=int, default=40000)
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = config["tsdf_global"]
vs, trunc = float(cfg["voxel_size"]), float(cfg["trunc_dist"])
band = int(2.0 * trunc / (0.5 * vs)) + 4
print(f"voxel_size={vs} trunc={trunc} points/kf={args.points} device={torch.cuda.get_device_name(dev)}", flush=True)
for n_kf in args.keyframes:
    vol = TSDFVolume(vs, trunc, cfg["max_weight"], cfg["min_tsdf_weight"], capacity=1 << 22, device=dev)
    t0 = time.time()
    for i in range(n_kf):
        T = synthetic.camera_pose(i * (1000 // n_kf))
        X = synthetic.render_pointmap(T, 192, 256).reshape(-1, 3)
        rng = np.random.default_rng(i)
        sel = rng.permutation(X.shape[0])[:args.points]
        vol.maintain(reserve=args.points * band)
        vol.integrate(synthetic.sim3_act(T, X[sel]).astype(np.float32), rng.uniform(0.5, 2.0, len(sel)),
                      T[:3].astype(np.float32), return_fused=False)
    voxels, cap = vol.maintain()
    torch.cuda.synchronize()
    t_fuse = time.time() - t0
    for _ in range(2):
        vol.extract_mesh()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        v, n, f = vol.extract_mesh()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    med = float(np.median(ms))
    print(f"keyframes={n_kf} voxels={voxels} capacity={cap} V={v.shape[0]} F={f.shape[0]} "
          f"extract_ms median={med:.3f} min={min(ms):.3f} max={max(ms):.3f} "
          f"occupied_bytes_per_ms={voxels * 25 / med:.3e} (fusion {t_fuse:.1f} s)", flush=True)
