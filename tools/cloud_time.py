#!/usr/bin/env python3
"""Event timing of the point-cloud tools (csrc/cloud.hip, DESIGN.md "Point clouds") on clouds of the synthetic room:
world points of pointmaps rendered along the trajectory, as evaluate.save_reconstruction gathers them.  In one process,
HIP events after warm-up, medians:
    index build         keys, stable sort, boxes of a --cloud point cloud
    cloud_distance      --queries queries (room points moved by a centimetre) against that cloud: indexed with sorted
                        queries, indexed with the queries as they come, indexed with the group level off, and the plain
                        scan; beside them a chunked torch.cdist + argmin in f32 (the baseline: not exact, no tie rule)
    downsample_cloud    --raw points on the TSDF's grid, beside a torch.unique + index_add baseline (f32 sums in any
                        order: not the same bits from call to call)
Every indexed form is compared byte for byte with the plain scan first, and the skipped share of (wave, tile) scans is
printed beside each time.  Not part of bench.py.
    python tools/cloud_time.py [--cloud 2000000] [--queries 200000] [--raw 24000000] [--reps 5]"""
import argparse

import numpy as np
import torch

from _room import timed   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam import synthetic
from mast3r_slam.config import config
from mast3r_slam.tsdf import CloudIndex, downsample_cloud

ap = argparse.ArgumentParser()
ap.add_argument("--cloud", type=int, default=2_000_000)
ap.add_argument("--queries", type=int, default=200_000)
ap.add_argument("--raw", type=int, default=24_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--plain-reps", type=int, default=1)
args = ap.parse_args()
dev = torch.device("cuda:0")
L = _m.lib()
H, W = 384, 512
VS = float(config["tsdf_global"]["voxel_size"])
print(f"cloud={args.cloud} queries={args.queries} raw={args.raw} voxel={VS} device={torch.cuda.get_device_name(dev)}",
      flush=True)


def room_points(n):
    """n world points of the room: whole pointmaps of H x W pixels from poses along the trajectory, in keyframe order,
    with the pixel noise of the synthetic pairs, cut to n."""
    n_kf = (n + H * W - 1) // (H * W)
    out = []
    for kf in range(n_kf):
        T = synthetic.camera_pose(kf * max(1, 1000 // n_kf))
        X = synthetic.render_pointmap(T, H, W).reshape(-1, 3)
        X = X + np.random.default_rng(kf).normal(0.0, 0.002, X.shape)
        out.append(torch.from_numpy(synthetic.sim3_act(T, X).astype(np.float32)))
    return torch.cat(out)[:n].to(dev).contiguous()


def distance(q, p, ix, levels, counts):
    n, N = int(q.shape[0]), int(p.shape[0])
    d2 = torch.empty(n, dtype=torch.float64, device=dev)
    near = torch.empty(n, dtype=torch.int32, device=dev)
    if ix is None:
        _m.check(L.mslam_cloud_distance(_m.ptr(q), n, _m.ptr(p), N, 0, 0, 0, 1, 0, _m.ptr(d2), _m.ptr(near),
                                        _m.stream_ptr()), "cloud_distance")
    else:
        _m.check(L.mslam_cloud_distance(_m.ptr(q), n, _m.ptr(p), N, _m.ptr(ix.order), _m.ptr(ix.ws), ix.ws_bytes, levels,
                                        _m.ptr(counts), _m.ptr(d2), _m.ptr(near), _m.stream_ptr()), "cloud_distance")
    return d2, near


def cdist_argmin(q, p, chunk=2048):
    """The baseline: torch.cdist in f32 over chunks of queries, min and argmin per row."""
    d, j = [], []
    for s in range(0, int(q.shape[0]), chunk):
        m = torch.cdist(q[s:s + chunk], p).min(1)
        d.append(m[0])
        j.append(m[1])
    return torch.cat(d), torch.cat(j)


def unique_downsample(p, vs):
    """The baseline: integer cell coordinates, torch.unique over the keys, index_add_ sums in f32, a division.  The cell
    size is a tensor: torch divides by a Python number through its reciprocal, which moves points on a cell face."""
    cell = torch.floor(p / torch.tensor(vs, dtype=torch.float32, device=p.device)).to(torch.int64)
    key = ((cell[:, 0] + (1 << 20)) << 42) | ((cell[:, 1] + (1 << 20)) << 21) | (cell[:, 2] + (1 << 20))
    uniq, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    total = torch.zeros((int(uniq.shape[0]), 3), dtype=torch.float32, device=p.device).index_add_(0, inv, p)
    return total / cnt[:, None], cnt


cloud = room_points(args.cloud)
N = int(cloud.shape[0])
pick = (torch.arange(args.queries, device=dev, dtype=torch.int64) * N) // args.queries
queries = (cloud[pick] + 0.01).contiguous()
n = int(queries.shape[0])
ntiles, waves = (N + 127) // 128, (n + 63) // 64
print(f"cloud N={N} ({ntiles} tiles, {(ntiles + 31) // 32} groups), n={n} queries", flush=True)
print(f"index build (keys, sort, boxes) ms {timed(lambda: CloudIndex(cloud), max(3, args.reps))}", flush=True)
ix = CloudIndex(cloud)
perm = ix.query_order(queries)
sorted_q = queries[perm].contiguous()
counts = torch.zeros(4 * ((n + 255) // 256), dtype=torch.int32, device=dev)
plain = distance(queries, cloud, None, 1, None)
for label, q, back, levels in (("indexed, sorted queries", sorted_q, perm, 2), ("indexed, queries as they come", queries,
                                                                               None, 2),
                               ("indexed, sorted queries, tiles alone", sorted_q, perm, 1)):
    d2, near = distance(q, cloud, ix, levels, counts)
    if back is not None:
        d2, near = torch.empty_like(d2).index_copy_(0, back, d2), torch.empty_like(near).index_copy_(0, back, near)
    assert torch.equal(d2.view(torch.int64), plain[0].view(torch.int64)) and torch.equal(near, plain[1]), label
    share = float(counts[:waves].sum()) / (waves * ntiles)
    print(f"  {label}: distance_ms {timed(lambda: distance(q, cloud, ix, levels, counts), args.reps)}  skipped share "
          f"{share:.5f}", flush=True)
print(f"  query sort (keys, sort, gather, two scatters) ms "
      f"{timed(lambda: (queries[ix.query_order(queries)].contiguous(), torch.empty_like(plain[0]).index_copy_(0, perm, plain[0]), torch.empty_like(plain[1]).index_copy_(0, perm, plain[1])), args.reps)}",
      flush=True)
print(f"  plain scan: distance_ms {timed(lambda: distance(queries, cloud, None, 1, None), args.plain_reps)}", flush=True)
base = cdist_argmin(queries, cloud)
agree = float((base[1] == plain[1].long()).double().mean())
print(f"  torch.cdist + argmin, f32, chunks of 2048: ms {timed(lambda: cdist_argmin(queries, cloud), args.plain_reps)}  "
      f"(same neighbour as the exact scan for {agree:.5f} of the queries)", flush=True)
del base, plain, sorted_q, counts

raw = room_points(args.raw)
colors = torch.randint(0, 256, (int(raw.shape[0]), 3), dtype=torch.uint8, device=dev)
out = downsample_cloud(raw, VS, colors)
again = downsample_cloud(raw, VS, colors)
assert all(torch.equal(a, b) for a, b in zip(out, again))
print(f"downsample N={int(raw.shape[0])} -> M={int(out[0].shape[0])} voxels, largest {int(out[2].max())} points", flush=True)
print(f"  downsample_cloud with colours ms {timed(lambda: downsample_cloud(raw, VS, colors), args.reps)}", flush=True)
print(f"  downsample_cloud without colours ms {timed(lambda: downsample_cloud(raw, VS), args.reps)}", flush=True)
b = unique_downsample(raw, VS)
same = int(b[0].shape[0]) == int(out[0].shape[0]) and torch.equal(b[1].to(torch.int32), out[2])
print(f"  torch.unique + index_add_ (no colours, f32 sums) ms {timed(lambda: unique_downsample(raw, VS), args.reps)}  "
      f"same voxels and counts: {same}"
      + (f", largest centroid difference {float((b[0] - out[0]).abs().max()):.3g}" if same else ""), flush=True)
