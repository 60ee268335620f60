#!/usr/bin/env python3
"""Event timing of TSDFVolume.extract_mesh (csrc/tsdf_mesh.hip) on volumes fused the way the product fuses them: room
keyframes along the synthetic trajectory, 40 000 points each (tsdf_global.max_points_per_kf), the config's voxel size
and truncation, the manager's maintain() before every fusion.  Prints voxels, V, F, the median time of an extraction
(the sort, the kernels and the one host read of the output sizes) and the occupied-slot bytes (key, tsdf, weight, state:
25 B per voxel) read per ms.  Not part of bench.py.
    python tools/mesh_time.py 60 400 [--reps 10]"""
import argparse
import time

import numpy as np
import torch

from _room import build_room, timed_ms   # first: it puts the package on sys.path
from mast3r_slam.config import config

ap = argparse.ArgumentParser()
ap.add_argument("keyframes", type=int, nargs="+")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--points", type=int, default=40000)
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = config["tsdf_global"]
vs, trunc = float(cfg["voxel_size"]), float(cfg["trunc_dist"])
print(f"voxel_size={vs} trunc={trunc} points/kf={args.points} device={torch.cuda.get_device_name(dev)}", flush=True)
for n_kf in args.keyframes:
    t0 = time.time()
    vol = build_room(n_kf, args.points, dev)
    voxels, cap = vol.maintain()
    torch.cuda.synchronize()
    t_fuse = time.time() - t0
    v, _, f = vol.extract_mesh()
    ms = timed_ms(vol.extract_mesh, args.reps)
    med = float(np.median(ms))
    print(f"keyframes={n_kf} voxels={voxels} capacity={cap} V={v.shape[0]} F={f.shape[0]} "
          f"extract_ms median={med:.3f} min={min(ms):.3f} max={max(ms):.3f} "
          f"occupied_bytes_per_ms={voxels * 25 / med:.3e} (fusion {t_fuse:.1f} s)", flush=True)
