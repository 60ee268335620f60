#!/usr/bin/env python3
"""Event timing of the radius count and the density clusters of a point cloud (csrc/cloud_cluster.hip, DESIGN.md "Cloud
clusters") on the room cloud of tools/cloud_knn_time.py: world points of pointmaps rendered along the trajectory.  In
one process, HIP events after warm-up, medians, on three inputs:
    room      the --cloud points as they are, eps --eps, min_points --min-points
    thinned   the same cloud after downsample_cloud on the TSDF's voxel, eps 2.5 voxels, min_points 4
    dense     the --cloud points again with eps --dense-eps, at which a point has hundreds of neighbours
and per input:
    cloud_radius_count  the cloud in itself, indexed, the rows in the index's order; the share of (wave, tile) scans
                        skipped; compared byte for byte with the plain scan on --queries of its rows first
    link                mslam_cloud_cluster_link alone, `parent` initialised before every call outside the events
    cloud_clusters      the whole call with the index given: count, core, link, flatten, labels, ranking, sizes
    cloud_knn k = 16    the yardstick: the same cloud in itself, indexed, the rows in the index's order
MSLAM_LIB names another build of the library (one without the cached root, say).  Not part of bench.py.
    python tools/cloud_cluster_time.py [--cloud 2000000] [--queries 100000] [--reps 3]"""
import argparse
import os

import numpy as np
import torch

from _room import timed   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam import synthetic
from mast3r_slam.config import config
from mast3r_slam.tsdf import CloudIndex, cloud_clusters, downsample_cloud
from mast3r_slam.tsdf.mesh_index import _index_ops

ap = argparse.ArgumentParser()
ap.add_argument("--cloud", type=int, default=2_000_000)
ap.add_argument("--queries", type=int, default=100_000)
ap.add_argument("--eps", type=float, default=0.02)
ap.add_argument("--min-points", type=int, default=10)
ap.add_argument("--dense-eps", type=float, default=0.05)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda:0")
L = _m.lib()
H, W = 384, 512
voxel = float(config["tsdf_global"]["voxel_size"])
print(f"cloud={args.cloud} queries={args.queries} voxel={voxel} device={torch.cuda.get_device_name(dev)}"
      + (f" MSLAM_LIB={os.path.basename(os.environ['MSLAM_LIB'])}" if os.environ.get("MSLAM_LIB") else ""), flush=True)


def room_points(n):
    """n world points of the room: whole pointmaps of H x W pixels from poses along the trajectory, in keyframe order,
    with the pixel noise of the synthetic pairs, cut to n (tools/cloud_knn_time.py's cloud)."""
    n_kf = (n + H * W - 1) // (H * W)
    out = []
    for kf in range(n_kf):
        T = synthetic.camera_pose(kf * max(1, 1000 // n_kf))
        X = synthetic.render_pointmap(T, H, W).reshape(-1, 3)
        X = X + np.random.default_rng(kf).normal(0.0, 0.002, X.shape)
        out.append(torch.from_numpy(synthetic.sim3_act(T, X).astype(np.float32)))
    return torch.cat(out)[:n].to(dev).contiguous()


def run(label, cloud, eps, min_points):
    N = int(cloud.shape[0])
    eps2 = float(eps) * float(eps)
    ix = CloudIndex(cloud)
    order = ix.order
    rows = cloud[order.long()].contiguous()                    # the cloud's points in the index's order
    ntiles, waves = (N + 127) // 128, (N + 63) // 64
    skips = torch.zeros(4 * ((N + 255) // 256), dtype=torch.int32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    st = _m.stream_ptr()
    print(f"{label}: N={N} ({ntiles} tiles, {(ntiles + 31) // 32} groups) eps={eps} min_points={min_points}", flush=True)

    def radius_count(q, out, ix_, sk):
        _m.check(L.mslam_cloud_radius_count(_m.ptr(q), int(q.shape[0]), _m.ptr(cloud), N, eps2, *_index_ops(ix_),
                                            _m.ptr(sk), _m.ptr(out), st), "cloud_radius_count")

    radius_count(rows, count, ix, skips)
    share = float(skips[:waves].sum()) / (waves * ntiles)
    n = min(args.queries, N)
    pick = (torch.arange(n, device=dev, dtype=torch.int64) * N) // n
    some, plain = rows[pick].contiguous(), torch.empty(n, dtype=torch.int32, device=dev)
    radius_count(some, plain, None, None)
    assert torch.equal(count[pick], plain), "the indexed count differs from the plain scan"
    c = count.double()
    print(f"  neighbours within eps: mean {float(c.mean()):.1f} median {float(c.median()):.0f} max {int(c.max())}",
          flush=True)
    print(f"  cloud_radius_count, indexed, n={N}: ms {timed(lambda: radius_count(rows, count, ix, skips), args.reps)}  "
          f"skipped share {share:.5f}", flush=True)
    print(f"  cloud_radius_count, plain scan, n={n}: ms {timed(lambda: radius_count(some, plain, None, None), 1)}",
          flush=True)

    by_point = torch.empty_like(count).index_copy_(0, order.long(), count)
    core = (torch.isfinite(cloud).all(1) & (by_point >= min_points)).to(torch.uint8)
    parent = torch.empty(N, dtype=torch.int32, device=dev)
    anchor = torch.empty(N, dtype=torch.int32, device=dev)
    dist2 = torch.empty(N, dtype=torch.float64, device=dev)

    def init():
        _m.check(L.mslam_cloud_cluster_init(N, _m.ptr(parent), st), "cloud_cluster_init")

    def link():
        _m.check(L.mslam_cloud_cluster_link(_m.ptr(cloud), N, _m.ptr(order), N, eps2, _m.ptr(core), *_index_ops(ix),
                                            _m.ptr(skips), _m.ptr(parent), _m.ptr(anchor), _m.ptr(dist2), st),
                 "cloud_cluster_link")

    init()
    link()
    share = float(skips[:waves].sum()) / (waves * ntiles)
    print(f"  link, indexed, n={N}, core share {float(core.double().mean()):.4f}: ms {timed(link, args.reps, init)}  "
          f"skipped share {share:.5f}", flush=True)
    print(f"  cloud_clusters, index given: ms {timed(lambda: cloud_clusters(cloud, eps, min_points, index=ix), args.reps)}",
          flush=True)
    labels, info = cloud_clusters(cloud, eps, min_points, index=ix)
    sizes = info["sizes"]
    print(f"  {info['n_clusters']} clusters, largest {int(sizes.max()) if info['n_clusters'] else 0}, "
          f"{info['n_core']} core, {info['n_noise']} noise points", flush=True)
    assert torch.equal(info["count"], by_point)
    again = cloud_clusters(cloud, eps, min_points, index=ix)[0]
    assert torch.equal(again, labels), "two calls differ"

    k = 16
    d2 = torch.empty((N, k), dtype=torch.float64, device=dev)
    nb = torch.empty((N, k), dtype=torch.int32, device=dev)

    def knn():
        _m.check(L.mslam_cloud_knn(_m.ptr(rows), N, _m.ptr(cloud), N, k, 0, *_index_ops(ix), _m.ptr(skips), _m.ptr(d2),
                                   _m.ptr(nb), st), "cloud_knn")

    knn()
    share = float(skips[:waves].sum()) / (waves * ntiles)
    print(f"  cloud_knn k={k}, indexed, n={N}: ms {timed(knn, args.reps)}  skipped share {share:.5f}", flush=True)


room = room_points(args.cloud)
run("room", room, args.eps, args.min_points)
thin = downsample_cloud(room, voxel)[0]
run("thinned", thin, 2.5 * voxel, 4)
run("dense", room, args.dense_eps, args.min_points)
