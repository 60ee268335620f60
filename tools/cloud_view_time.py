#!/usr/bin/env python3
"""Event timing of the cloud views (csrc/cloud_view.hip, DESIGN.md "Cloud views") on the room cloud of
tools/cloud_time.py - world points of pointmaps rendered along the trajectory - thinned at the config's voxel size, seen
from --keyframes cameras along the trajectory at 384x512 with point_size = 2 voxel.  In one process, HIP events, the
median of --reps launches after three warm-up launches:
    splat      one launch over a chunk of 8 views, and over one view; beside it the memset that empties the z-buffer
               (part of the same call) on its own
    resolve    the 8 z-buffers into range / index / hit / rgb
    visible    the thinned cloud's own points against the 8 z-buffers, `seen` cleared before every launch
    the share of footprint pixels whose plain load did not settle them, so that an atomic was issued (the counters of
    a measurement launch), for the chunk as it comes and for the same points in a shuffled order
    observed_cloud_points over all cameras, and beside it observed_points of the same points against room_mesh() with
    an index, with the share of points on which the two disagree
The lines go to stdout and to --log.  Not part of bench.py.
    python tools/cloud_view_time.py [--cloud 2000000] [--keyframes 32] [--reps 20] [--log profiles/cloud_view_time.log]"""
import argparse
import os

import numpy as np
import torch

from _room import ROOT, timed   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam import synthetic
from mast3r_slam.config import config
from mast3r_slam.tsdf import downsample_cloud, observed_cloud_points, observed_points

ap = argparse.ArgumentParser()
ap.add_argument("--cloud", type=int, default=2_000_000)
ap.add_argument("--keyframes", type=int, default=32)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "cloud_view_time.log"))
args = ap.parse_args()
dev = torch.device("cuda:0")
L, st = _m.lib(), _m.stream_ptr()
H, W = 384, 512
log = open(args.log, "w")


def say(line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def room_points(n):
    """tools/cloud_time.py's cloud: whole pointmaps of H x W pixels from poses along the trajectory, in keyframe order,
    with the pixel noise of the synthetic pairs, cut to n."""
    n_kf = (n + H * W - 1) // (H * W)
    out = []
    for kf in range(n_kf):
        T = synthetic.camera_pose(kf * max(1, 1000 // n_kf))
        X = synthetic.render_pointmap(T, H, W).reshape(-1, 3)
        X = X + np.random.default_rng(kf).normal(0.0, 0.002, X.shape)
        out.append(torch.from_numpy(synthetic.sim3_act(T, X).astype(np.float32)))
    return torch.cat(out)[:n].to(dev).contiguous()


voxel = float(config["tsdf_global"]["voxel_size"])
raw = room_points(args.cloud)
cloud = downsample_cloud(raw, voxel)[0]
n = int(cloud.shape[0])
colors = torch.randint(0, 256, (n, 3), dtype=torch.uint8, device=dev)
n_kf = args.keyframes
cams = torch.from_numpy(np.stack([synthetic.camera_pose(i * (1000 // n_kf)) for i in range(n_kf)]).astype(np.float32))
cams = cams.to(dev).contiguous()
K = synthetic.intrinsics(H, W)
k4 = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
size, near, far = 2.0 * voxel, 0.05, 10.0
say(f"cloud={int(raw.shape[0])} thinned at {voxel} -> n={n}; {n_kf} cameras at {H}x{W}, point_size={size}, "
    f"device={torch.cuda.get_device_name(dev)}")
del raw

V = min(8, n_kf)
zbuf = torch.empty((V, H, W), dtype=torch.int64, device=dev)
counters = torch.zeros(2, dtype=torch.int64, device=dev)


def splat(points, views, count=False):
    _m.check(L.mslam_cloud_view_splat(_m.ptr(points), int(points.shape[0]), _m.ptr(views), int(views.shape[0]), *k4, H,
                                      W, near, far, 0, size, 8, _m.ptr(zbuf), _m.ptr(counters) if count else 0, st),
             "cloud_view_splat")


rng_ = torch.empty((V, H, W), dtype=torch.float32, device=dev)
idx = torch.empty((V, H, W), dtype=torch.int32, device=dev)
hit = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
rgb = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev)
seen = torch.zeros(n, dtype=torch.uint8, device=dev)


def resolve():
    _m.check(L.mslam_cloud_view_resolve(_m.ptr(zbuf), _m.ptr(cams), V, H, W, _m.ptr(colors), n, _m.ptr(rng_),
                                        _m.ptr(idx), _m.ptr(hit), _m.ptr(rgb), st), "cloud_view_resolve")


def visible():
    _m.check(L.mslam_cloud_view_visible(_m.ptr(cloud), n, _m.ptr(zbuf), _m.ptr(cams), V, *k4, H, W, near, far,
                                        2.0 * size, 0.0, _m.ptr(seen), st), "cloud_view_visible")


say(f"splat, {V} views, n={n}: ms {timed(lambda: splat(cloud, cams[:V]), args.reps)}")
say(f"splat, 1 view, n={n}: ms {timed(lambda: splat(cloud, cams[:1]), args.reps)}")
say(f"  the memset of {V} z-buffers alone: ms {timed(lambda: zbuf.fill_(-1), args.reps)}")
splat(cloud, cams[:V])
say(f"resolve with colours, {V} views: ms {timed(resolve, args.reps)}")
resolve()
say(f"  hit share of the pixels {float(hit.double().mean()):.4f}")
say(f"visible, n={n} queries, {V} views: ms {timed(visible, args.reps, prep=lambda: seen.zero_())}")
shuffled = cloud[torch.randperm(n, device=dev)].contiguous()
for label, pts in (("in key order", cloud), ("shuffled", shuffled)):
    counters.zero_()
    splat(pts, cams[:V], count=True)
    visited, issued = (int(x) for x in counters.tolist())
    say(f"footprint pixels visited, {label}: {visited} ({visited / max(n * V, 1):.2f} per point and view), atomics "
        f"issued {issued}: share {issued / max(visited, 1):.4f}")
    say(f"  splat, {V} views, {label}: ms {timed(lambda: splat(pts, cams[:V]), args.reps)}")

own = observed_cloud_points(cloud, cloud, cams, K, (H, W), point_size=size)
say(f"observed_cloud_points, n={n}, {n_kf} cameras, chunk 8: ms "
    f"{timed(lambda: observed_cloud_points(cloud, cloud, cams, K, (H, W), point_size=size), 3)}  observed share "
    f"{float(own.double().mean()):.4f}")
Vr, Fr = synthetic.room_mesh()
mesh = (torch.from_numpy(Vr).to(dev), torch.from_numpy(Fr).to(dev))
by_mesh = observed_points(cloud, mesh, cams.cpu(), K, (H, W), index=True)
say(f"observed_points against room_mesh() with an index, the same points and cameras: ms "
    f"{timed(lambda: observed_points(cloud, mesh, cams.cpu(), K, (H, W), index=True), 3)}  observed share "
    f"{float(by_mesh.double().mean()):.4f}; the two disagree on {float((own != by_mesh).double().mean()):.5f} of the "
    f"points (the cloud carries 2 mm of noise and its thinning, the mesh is the ideal room)")
log.close()
