#!/usr/bin/env python3
"""Event timing of the k nearest neighbours, the normals and the outlier filter of a point cloud (csrc/cloud_knn.hip,
DESIGN.md "Point clouds") on the room cloud of tools/cloud_time.py: world points of pointmaps rendered along the
trajectory.  In one process, HIP events after warm-up, medians:
    cloud_knn           the --cloud points in themselves at k = 8, 16, 32: indexed with sorted queries, indexed with the
                        queries as they come, and the plain scan over --queries of them; beside them a chunked
                        torch.cdist + topk over --baseline of them, which is f32 and has no tie rule: not the same
                        function, and the share of rows where its neighbours differ is printed
    cloud_normals       k = 16, the k-NN and the eigenvectors, with the index given
    cloud_outliers      k = 16, std_ratio 2: the k-NN, the statistics, the mask
Every indexed form is compared byte for byte with the plain scan on the --queries rows first, and the skipped share of
(wave, tile) scans is printed beside each time.  Not part of bench.py.
    python tools/cloud_knn_time.py [--cloud 2000000] [--queries 200000] [--baseline 20000] [--reps 3]"""
import argparse

import numpy as np
import torch

from _room import timed   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam import synthetic
from mast3r_slam.tsdf import CloudIndex, cloud_normals, cloud_outliers

ap = argparse.ArgumentParser()
ap.add_argument("--cloud", type=int, default=2_000_000)
ap.add_argument("--queries", type=int, default=200_000)
ap.add_argument("--baseline", type=int, default=20_000)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda:0")
L = _m.lib()
H, W = 384, 512
print(f"cloud={args.cloud} queries={args.queries} baseline={args.baseline} device={torch.cuda.get_device_name(dev)}",
      flush=True)


def room_points(n):
    """n world points of the room: whole pointmaps of H x W pixels from poses along the trajectory, in keyframe order,
    with the pixel noise of the synthetic pairs, cut to n (tools/cloud_time.py's cloud)."""
    n_kf = (n + H * W - 1) // (H * W)
    out = []
    for kf in range(n_kf):
        T = synthetic.camera_pose(kf * max(1, 1000 // n_kf))
        X = synthetic.render_pointmap(T, H, W).reshape(-1, 3)
        X = X + np.random.default_rng(kf).normal(0.0, 0.002, X.shape)
        out.append(torch.from_numpy(synthetic.sim3_act(T, X).astype(np.float32)))
    return torch.cat(out)[:n].to(dev).contiguous()


def knn(q, p, k, ix, counts, out=None):
    n, N = int(q.shape[0]), int(p.shape[0])
    d2, nb = out if out is not None else (torch.empty((n, k), dtype=torch.float64, device=dev),
                                          torch.empty((n, k), dtype=torch.int32, device=dev))
    index = (0, 0, 0, 1) if ix is None else (_m.ptr(ix.order), _m.ptr(ix.ws), ix.ws_bytes, 2)
    _m.check(L.mslam_cloud_knn(_m.ptr(q), n, _m.ptr(p), N, k, 0, *index, _m.ptr(counts), _m.ptr(d2), _m.ptr(nb),
                               _m.stream_ptr()), "cloud_knn")
    return d2, nb


def cdist_topk(q, p, k, chunk=1024):
    """The baseline: torch.cdist in f32 over chunks of queries, the k smallest per row."""
    d, j = [], []
    for s in range(0, int(q.shape[0]), chunk):
        m = torch.topk(torch.cdist(q[s:s + chunk], p), k, dim=1, largest=False, sorted=True)
        d.append(m[0])
        j.append(m[1])
    return torch.cat(d), torch.cat(j)


cloud = room_points(args.cloud)
N = int(cloud.shape[0])
ix = CloudIndex(cloud)
perm = ix.query_order(cloud)
sorted_cloud = cloud[perm].contiguous()
pick = (torch.arange(args.queries, device=dev, dtype=torch.int64) * N) // args.queries
some = cloud[pick].contiguous()
n = int(some.shape[0])
ntiles = (N + 127) // 128
print(f"cloud N={N} ({ntiles} tiles, {(ntiles + 31) // 32} groups); plain scan over n={n} of its points", flush=True)
counts = torch.zeros(4 * ((N + 255) // 256), dtype=torch.int32, device=dev)
for k in (8, 16, 32):
    print(f"k = {k}", flush=True)
    plain = knn(some, cloud, k, None, None)
    out = (torch.empty((N, k), dtype=torch.float64, device=dev), torch.empty((N, k), dtype=torch.int32, device=dev))
    for label, q, back in (("indexed, sorted queries", sorted_cloud, perm), ("indexed, queries as they come", cloud,
                                                                             None)):
        d2, nb = knn(q, cloud, k, ix, counts, out)
        share = float(counts[:(N + 63) // 64].sum()) / (((N + 63) // 64) * ntiles)
        if back is not None:
            d2, nb = torch.empty_like(d2).index_copy_(0, back, d2), torch.empty_like(nb).index_copy_(0, back, nb)
        assert torch.equal(d2[pick].view(torch.int64), plain[0].view(torch.int64)) and torch.equal(nb[pick], plain[1]), label
        del d2, nb
        print(f"  {label}, n={N}: knn_ms {timed(lambda: knn(q, cloud, k, ix, counts, out), args.reps)}  skipped share "
              f"{share:.5f}", flush=True)
    del out
    print(f"  plain scan, n={n}: knn_ms {timed(lambda: knn(some, cloud, k, None, None, plain), 1)}", flush=True)
    few = some[:args.baseline].contiguous()
    base = cdist_topk(few, cloud, k)
    differ = float((base[1] != plain[1][:args.baseline].long()).any(1).double().mean())
    print(f"  torch.cdist + topk, f32, chunks of 1024, n={int(few.shape[0])}: ms "
          f"{timed(lambda: cdist_topk(few, cloud, k), 1)}  (rows whose neighbours differ from the exact ones: "
          f"{differ:.5f})", flush=True)
    del base, plain
print(f"cloud_normals k=16, index given, n={N}: ms {timed(lambda: cloud_normals(cloud, 16, index=ix), args.reps)}",
      flush=True)
nrm, curv, cnt = cloud_normals(cloud, 16, index=ix)
print(f"  non-zero normals {float(nrm.any(1).double().mean()):.5f}, median curvature "
      f"{float(curv[~curv.isnan()].median()):.5f}", flush=True)
print(f"cloud_outliers k=16 std_ratio=2, index given, n={N}: ms "
      f"{timed(lambda: cloud_outliers(cloud, 16, 2.0, index=ix), args.reps)}", flush=True)
keep, info = cloud_outliers(cloud, 16, 2.0, index=ix)
print(f"  kept {info['kept']} of {info['n_valid']}, mu {info['mu']:.6f} sigma {info['sigma']:.6f} threshold "
      f"{info['threshold']:.6f}", flush=True)
