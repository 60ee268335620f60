#!/usr/bin/env python3
"""Event timing of TSDFVolume.render (csrc/tsdf_render.hip) on a volume fused the way the product fuses it: room
keyframes along the synthetic trajectory, 40 000 points each (tsdf_global.max_points_per_kf), the config's voxel size
and truncation, the manager's maintain() before every fusion (the volume of tools/mesh_time.py).  Times, with HIP
events after warm-up, medians of repeated calls: the block pre-pass alone, the march with empty-space skipping and the
brute-force march (both without the pre-pass), for 384x512 views from poses of the trajectory.  Not part of bench.py.
    python tools/render_time.py 60 [--reps 20] [--far 10.0]"""
import argparse

import numpy as np
import torch

from _room import build_room, timed   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam import synthetic
from mast3r_slam.config import config
from mast3r_slam.tsdf.global_volume import pinhole_rays

ap = argparse.ArgumentParser()
ap.add_argument("keyframes", type=int, nargs="+")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--points", type=int, default=40000)
ap.add_argument("--far", type=float, default=10.0)
ap.add_argument("--hw", type=int, nargs=2, default=(384, 512))
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = config["tsdf_global"]
vs, trunc = float(cfg["voxel_size"]), float(cfg["trunc_dist"])
h, w = args.hw
print(f"voxel_size={vs} trunc={trunc} points/kf={args.points} view={h}x{w} near=0.05 far={args.far} step={0.5 * vs} "
      f"device={torch.cuda.get_device_name(dev)}", flush=True)
L = _m.lib()


for n_kf in args.keyframes:
    vol = build_room(n_kf, args.points, dev)
    voxels, cap = vol.maintain()
    rays = pinhole_rays(synthetic.intrinsics(h, w), (h, w), dev)
    wsb = L.mslam_tsdf_render_workspace_bytes(cap)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = (torch.empty((h, w), dtype=torch.float32, device=dev), torch.empty((h, w, 3), dtype=torch.float32, device=dev),
           torch.empty((h, w), dtype=torch.uint8, device=dev))

    def blocks():
        _m.check(L.mslam_tsdf_render_blocks(_m.ptr(vol._table), cap, vol.min_weight, _m.ptr(ws), wsb, _m.stream_ptr()),
                 "tsdf_render_blocks")

    def march(pose, skip):
        _m.check(L.mslam_tsdf_render(_m.ptr(vol._table), cap, _m.ptr(rays), h, w, _m.ptr(pose), vs, vol.min_weight, 0.0,
                                     0.05, args.far, 0.5 * vs, skip, _m.ptr(ws), wsb, _m.ptr(out[0]), _m.ptr(out[1]),
                                     _m.ptr(out[2]), _m.stream_ptr()), "tsdf_render")

    print(f"keyframes={n_kf} voxels={voxels} capacity={cap} workspace_bytes={wsb} "
          f"blocks_ms {timed(blocks, args.reps)}", flush=True)
    for frame in (5, 505):
        pose = torch.from_numpy(synthetic.camera_pose(frame).astype(np.float32)).to(dev)
        skip_ms = timed(lambda: march(pose, 1), args.reps)
        hits = float(out[2].float().mean())
        keep = [o.clone() for o in out]
        brute_ms = timed(lambda: march(pose, 0), args.reps)
        same = all(torch.equal(x, y) for x, y in zip(keep, out))
        print(f"  pose={frame} hit_share={hits:.4f} skip_ms {skip_ms} brute_ms {brute_ms} identical={same}", flush=True)
