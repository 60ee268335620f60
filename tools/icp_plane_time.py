#!/usr/bin/env python3
"""Event timing of point-to-plane ICP (csrc/icp_plane.hip; DESIGN.md "Point-to-plane ICP") against the point metrics of
the same library in the same run, on the room of tools/mesh_align_time.py (60 keyframes: 136 000 faces) and the room
cloud of tools/cloud_time.py (2 M points).  The source is the target moved by the inverse of a small Sim3 (2 degrees,
3 cm, scale 0.98) - the mesh itself, sampled; for the cloud a second, independent set of points of the same room.
For each metric and a ladder of iteration counts, with tol=0 so that every iteration runs: the error of the returned
Sim3 against the truth (rotation in rad, translation, scale) and the HIP-event time of the whole call, medians of
repeated calls; from the longest run the time per iteration.  The lines of the two metrics that reach the same error
give the iterations and the total time to it.  Not part of bench.py.
    python tools/icp_plane_time.py [--keyframes 60] [--cloud 2000000] [--samples 20000] [--reps 5]"""
import argparse
import math

import numpy as np
import torch

from _room import build_room, timed_ms   # first: it puts the package on sys.path
from mast3r_slam import synthetic
from mast3r_slam.config import config
from mast3r_slam.tsdf import CloudIndex, MeshIndex, align_clouds, align_meshes, cloud_normals, transform_mesh

ap = argparse.ArgumentParser()
ap.add_argument("--keyframes", type=int, default=60)
ap.add_argument("--points", type=int, default=40000)
ap.add_argument("--cloud", type=int, default=2_000_000)
ap.add_argument("--samples", type=int, default=20000)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
vs = float(config["tsdf_global"]["voxel_size"])
H, W = 384, 512
LADDER = dict(point=(10, 20, 40, 80), plane=(2, 4, 6, 8, 10))
print(f"keyframes={args.keyframes} cloud={args.cloud} samples={args.samples} voxel={vs} "
      f"device={torch.cuda.get_device_name(dev)}", flush=True)


def sim3(angle_deg, axis, t, s):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    h = 0.5 * math.radians(angle_deg)
    return np.concatenate([np.asarray(t, np.float64), axis * math.sin(h), [math.cos(h)], [s]])


def error(T, truth):
    """(rotation angle in rad, |t - t_truth|, |s - s_truth|) of the Sim3 T against the truth."""
    dq =abs(float(np.dot(T[3:7] / np.linalg.norm(T[3:7]), truth[3:7])))
    return 2.0 * math.acos(min(dq, 1.0)), float(np.linalg.norm(T[:3] - truth[:3])), abs(float(T[7] - truth[7]))


def room_points(n, seed0):
    """n world points of the room, whole pointmaps along the trajectory with the pixel noise of the synthetic pairs
    (tools/cloud_time.py), from the random streams seed0 + keyframe."""
    n_kf = (n + H * W - 1) // (H * W)
    out = []
    for kf in range(n_kf):
        T = synthetic.camera_pose(kf * max(1, 1000 // n_kf))
        X = synthetic.render_pointmap(T, H, W).reshape(-1, 3)
        X = X + np.random.default_rng(seed0 + kf).normal(0.0, 0.002, X.shape)
        out.append(torch.from_numpy(synthetic.sim3_act(T, X).astype(np.float32)))
    return torch.cat(out)[:n].to(dev).contiguous()


def ladder(name, call, truth):
    for metric, counts in LADDER.items():
        for iters in counts:
            res = call(metric, iters)
            ms = timed_ms(lambda: call(metric, iters), args.reps)
            e = error(res["T"].cpu().numpy(), truth)
            extra = f" normal_spread {res['normal_spread']:.3g}" if metric == "plane" else ""
            print(f"  {name} {metric} iterations={res['iterations']} error {e[0]:.3g} rad / {e[1]:.3g} / {e[2]:.3g} "
                  f"rmse {res['rmse']:.6f} total_ms median={float(np.median(ms)):.3f} min={min(ms):.3f} "
                  f"per_iteration_ms {float(np.median(ms)) / res['iterations']:.3f}{extra}", flush=True)


truth = sim3(2.0, (1.0, 2.0, 3.0), (0.02, -0.02, 0.01), 0.98)
trim = 4.0 * vs

vol = build_room(args.keyframes, args.points, dev)
vol.maintain()
verts, _, faces = vol.extract_mesh()
print(f"mesh: V={int(verts.shape[0])} F={int(faces.shape[0])}", flush=True)
pred, gt = (transform_mesh(verts, synthetic.sim3_inv(truth)), faces), (verts, faces)
mesh_index = MeshIndex(*gt)
ladder("mesh", lambda metric, iters: align_meshes(pred, gt, n_samples=args.samples, max_iters=iters, trim=trim, tol=0.0,
                                                  check_every=iters, index=mesh_index, metric=metric), truth)
del vol

cloud = room_points(args.cloud, 0)
other = room_points(min(args.cloud, 4 * H * W), 1000)
moved = transform_mesh(other, synthetic.sim3_inv(truth)).contiguous()
cloud_index = CloudIndex(cloud)
normals = cloud_normals(cloud, 16, index=cloud_index)[0]
print(f"cloud: N={int(cloud.shape[0])}, source {int(moved.shape[0])} points of a second sampling; "
      f"normals_ms {timed_ms(lambda: cloud_normals(cloud, 16, index=cloud_index), 3)}", flush=True)


def cloud_call(metric, iters):
    kw = dict(normals=normals) if metric == "plane" else {}
    return align_clouds(moved, cloud, n_samples=args.samples, max_iters=iters, trim=trim, tol=0.0, check_every=iters,
                        index=cloud_index, metric=metric, **kw)


ladder("cloud", cloud_call, truth)
