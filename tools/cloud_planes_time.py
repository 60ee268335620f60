#!/usr/bin/env python3
"""Event timing of the plane segmentation of a point cloud (csrc/cloud_planes.hip, DESIGN.md "Cloud planes") on the room
cloud of tools/cloud_cluster_time.py: world points of pointmaps rendered along the trajectory.  In one process, HIP
events after warm-up, medians, on two inputs:
    room      the --cloud points as they are
    thinned   the same cloud after downsample_cloud on the TSDF's voxel
and per input, with tol one voxel and --hypotheses hypotheses drawn from the whole cloud:
    count          mslam_cloud_planes_count alone: every valid point remains, the first round's hypotheses
    torch f32      the comparator: the same count as a chunked f32 matmul of [p, 1] with the hypotheses, abs, compare
                   and sum on the device (f32 products and sums: its counts may differ at the edge of tol)
    cloud_planes   the whole call at its defaults (16 rounds enqueued, one host read), and what it found
The lines are appended to --out as well as printed.  Not part of bench.py.
    python tools/cloud_planes_time.py [--cloud 2000000] [--hypotheses 1024] [--reps 5] [--out profiles/cloud_planes_time.log]"""
import argparse
import os

import numpy as np
import torch

from _room import ROOT, timed   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam import synthetic
from mast3r_slam.config import config
from mast3r_slam.tsdf import cloud_planes, downsample_cloud, plane_figures

ap = argparse.ArgumentParser()
ap.add_argument("--cloud", type=int, default=2_000_000)
ap.add_argument("--hypotheses", type=int, default=1024)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_planes_time.log"))
args = ap.parse_args()
dev = torch.device("cuda:0")
L = _m.lib()
H, W = 384, 512
voxel = float(config["tsdf_global"]["voxel_size"])
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
log = open(args.out, "a")


def say(line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


say(f"cloud={args.cloud} hypotheses={args.hypotheses} tol={voxel} device={torch.cuda.get_device_name(dev)}")


def room_points(n):
    """n world points of the room: whole pointmaps of H x W pixels from poses along the trajectory, in keyframe order,
    with the pixel noise of the synthetic pairs, cut to n (tools/cloud_cluster_time.py's cloud)."""
    n_kf = (n + H * W - 1) // (H * W)
    out = []
    for kf in range(n_kf):
        T = synthetic.camera_pose(kf * max(1, 1000 // n_kf))
        X = synthetic.render_pointmap(T, H, W).reshape(-1, 3)
        X = X + np.random.default_rng(kf).normal(0.0, 0.002, X.shape)
        out.append(torch.from_numpy(synthetic.sim3_act(T, X).astype(np.float32)))
    return torch.cat(out)[:n].to(dev).contiguous()


def run(label, cloud):
    N, nh = int(cloud.shape[0]), args.hypotheses
    st = _m.stream_ptr()
    labels = torch.full((N,), -1, dtype=torch.int32, device=dev)
    offsets = torch.empty((N + 255) // 256, dtype=torch.int32, device=dev)
    rem = torch.empty(N, dtype=torch.int32, device=dev)
    state = torch.zeros(8, dtype=torch.int32, device=dev)
    hyp = torch.empty((nh, 4), dtype=torch.float64, device=dev)
    triples = torch.empty((nh, 3), dtype=torch.int32, device=dev)
    count = torch.empty(nh, dtype=torch.int32, device=dev)
    _m.check(L.mslam_cloud_planes_remaining(_m.ptr(cloud), N, _m.ptr(labels), 100, _m.ptr(offsets), _m.ptr(rem),
                                            _m.ptr(state), st), "cloud_planes_remaining")
    _m.check(L.mslam_cloud_planes_draw(_m.ptr(cloud), N, _m.ptr(rem), N, _m.ptr(state), 0, 0, nh, _m.ptr(hyp),
                                       _m.ptr(triples), st), "cloud_planes_draw")
    M = int(state[0])
    say(f"{label}: N={N} remaining={M} H={nh} ({M * nh / 1e9:.2f} G plane tests)")

    def kernel():
        _m.check(L.mslam_cloud_planes_count(_m.ptr(cloud), 0, N, _m.ptr(rem), N, _m.ptr(state), _m.ptr(hyp), nh, voxel,
                                            0.0, _m.ptr(count), st), "cloud_planes_count")

    p4 = torch.cat([cloud[rem[:M].long()], torch.ones((M, 1), dtype=torch.float32, device=dev)], 1).contiguous()
    h32 = torch.nan_to_num(hyp.float(), nan=1.0e30).t().contiguous()           # a void hypothesis counts nothing
    other = torch.zeros(nh, dtype=torch.int64, device=dev)
    chunk = 1 << 18

    def matmul():
        other.zero_()
        for s in range(0, M, chunk):
            other.add_((torch.abs(p4[s:s + chunk] @ h32) <= voxel).sum(0))

    kernel()
    matmul()
    diff = (count.long() - other).abs()
    say(f"  best count {int(count.max())}, void hypotheses {int(torch.isnan(hyp[:, 0]).sum())}; the f32 comparator "
        f"differs in {int((diff > 0).sum())} of {nh} counts, by at most {int(diff.max())}")
    say(f"  count kernel: ms {timed(kernel, args.reps)}")
    say(f"  torch f32 matmul + compare + sum, chunks of {chunk}: ms {timed(matmul, args.reps)}")
    say(f"  cloud_planes, whole call: ms {timed(lambda: cloud_planes(cloud, voxel, hypotheses=nh), args.reps)}")
    res = cloud_planes(cloud, voxel, hypotheses=nh)
    again = cloud_planes(cloud, voxel, hypotheses=nh)
    assert torch.equal(res["labels"], again["labels"]) and torch.equal(res["planes"], again["planes"]), "two calls differ"
    fig = plane_figures(res, cloud)
    say(f"  {res['n_planes']} planes, counts {res['counts'].tolist()}")
    say(f"  plane_share {fig['plane_share']:.4f} plane_rmse {fig['plane_rmse']:.5f} manhattan_deg {fig['manhattan_deg']:.4f}")


room = room_points(args.cloud)
run("room", room)
run("thinned", downsample_cloud(room, voxel)[0])
log.close()
