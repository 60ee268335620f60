#!/usr/bin/env python3
"""Event timing of the cloud smoothing step (csrc/cloud_mls.hip, DESIGN.md "Cloud smoothing") on the room cloud of
tools/cloud_knn_time.py: world points of pointmaps rendered along the trajectory.  In one process, HIP events after
warm-up, medians, on three inputs:
    room 2 cm, room 5 cm   the --cloud points as they are in themselves, radius 0.02 and 0.05
    thinned 6 cm           the same cloud after downsample_cloud on the TSDF's voxel, radius two voxels
and per input, indexed, the rows in the index's order:
    step, ungated       mslam_cloud_mls_step of the cloud in itself; the share of (wave, tile) scans skipped
    step, gated         the same with the normals of the ungated step on both sides and cos 30 degrees
    smooth_cloud        the whole call with edge_angle=30 and the index given: the normals step, the gated step, the
                        sorting of the queries and the figures
    cloud_radius_count  the floor: the same walk at the same radius with an integer in the place of the ten sums
    torch f32           the comparator on --queries rows: chunks of cdist, weights, three einsums and
                        torch.linalg.eigh in f32 against the whole cloud; its speed per row and how far its points land
                        from the kernel's
Not part of bench.py.
    python tools/cloud_mls_time.py [--cloud 2000000] [--queries 4096] [--reps 3]"""
import argparse
import math

import numpy as np
import torch

from _room import timed, timed_ms   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam import synthetic
from mast3r_slam.config import config
from mast3r_slam.tsdf import CloudIndex, downsample_cloud, smooth_cloud
from mast3r_slam.tsdf.mesh_index import _index_ops

ap = argparse.ArgumentParser()
ap.add_argument("--cloud", type=int, default=2_000_000)
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--chunk", type=int, default=128)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda:0")
L = _m.lib()
H, W = 384, 512
voxel = float(config["tsdf_global"]["voxel_size"])
COS30 = math.cos(math.radians(30.0))
print(f"cloud={args.cloud} queries={args.queries} voxel={voxel} device={torch.cuda.get_device_name(dev)}", flush=True)


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


def torch_mls(q, cloud, h2):
    """The comparator, f32 throughout: one chunk of queries against the whole cloud -> (points, moved).  The moments are
    taken about the chunk's first query, so that f32 holds them."""
    c = q[:1]
    P, Q = cloud - c, q - c
    w = (1.0 - torch.cdist(Q, P).square() / h2).clamp_min(0.0).square()
    PP = torch.cat([P * P[:, :1], P[:, 1:] * P[:, 1:2], P[:, 2:] * P[:, 2:]], 1)          # xx xy xz yy yz zz
    s0 = torch.einsum("qn->q", w)
    m = torch.einsum("qn,nk->qk", w, P) / s0[:, None]
    s2 = torch.einsum("qn,nk->qk", w, PP) / s0[:, None]
    C = s2[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3) - m[:, :, None] * m[:, None, :]
    n = torch.linalg.eigh(C)[1][:, :, 0]
    t = ((m - Q) * n).sum(1, keepdim=True)
    return Q + t * n + c


def run(label, cloud, radius):
    N = int(cloud.shape[0])
    h2 = float(radius) * float(radius)
    ix = CloudIndex(cloud)
    order = ix.order.long()
    rows = cloud[order].contiguous()                           # the cloud's points in the index's order
    ntiles, waves = (N + 127) // 128, (N + 63) // 64
    skips = torch.zeros(4 * ((N + 255) // 256), dtype=torch.int32, device=dev)
    out, nrm = torch.empty((N, 3), dtype=torch.float32, device=dev), torch.empty((N, 3), dtype=torch.float32, device=dev)
    curv, count = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    st = _m.stream_ptr()
    print(f"{label}: N={N} ({ntiles} tiles, {(ntiles + 31) // 32} groups) radius={radius}", flush=True)

    def step(qn=None, pn=None):
        _m.check(L.mslam_cloud_mls_step(_m.ptr(rows), N, _m.ptr(cloud), N, h2, 6, 1.0, _m.ptr(qn), _m.ptr(pn), COS30,
                                        *_index_ops(ix), _m.ptr(skips), _m.ptr(out), _m.ptr(nrm), _m.ptr(curv),
                                        _m.ptr(count), 0, st), "cloud_mls_step")

    step()
    share = float(skips[:waves].sum()) / (waves * ntiles)
    c = count.double()
    moved = ~torch.isnan(curv)
    print(f"  neighbours within the radius: mean {float(c.mean()):.1f} median {float(c.median()):.0f} max {int(c.max())}"
          f"; moved share {float(moved.double().mean()):.4f}", flush=True)
    print(f"  step, ungated, n={N}: ms {timed(step, args.reps)}  skipped share {share:.5f}", flush=True)
    ungated, row_normals = out.clone(), nrm.clone()
    point_normals = torch.empty_like(row_normals).index_copy_(0, order, row_normals)
    step(row_normals, point_normals)
    share = float(skips[:waves].sum()) / (waves * ntiles)
    print(f"  step, gated at 30 degrees: ms {timed(lambda: step(row_normals, point_normals), args.reps)}  skipped share "
          f"{share:.5f}; joining neighbours mean {float(count.double().mean()):.1f}", flush=True)
    print(f"  smooth_cloud(edge_angle=30), index given: ms "
          f"{timed(lambda: smooth_cloud(cloud, radius, edge_angle=30.0, index=ix), args.reps)}", flush=True)
    info = smooth_cloud(cloud, radius, edge_angle=30.0, index=ix)[2]
    print(f"  displacement: rms {1e3 * info['rms_displacement']:.3f} mm, max {1e3 * info['max_displacement']:.3f} mm",
          flush=True)

    def radius_count():
        _m.check(L.mslam_cloud_radius_count(_m.ptr(rows), N, _m.ptr(cloud), N, h2, *_index_ops(ix), _m.ptr(skips),
                                            _m.ptr(count), st), "cloud_radius_count")

    print(f"  cloud_radius_count, the same radius and index: ms {timed(radius_count, args.reps)}", flush=True)

    # the comparator on rows spread over the index's order, one chunk of consecutive rows at a time
    n = min(args.queries, N) // args.chunk * args.chunk
    starts = [(k * (N - args.chunk)) // max(n // args.chunk - 1, 1) for k in range(n // args.chunk)]
    got = []

    def torch_rows():
        got.clear()
        for s in starts:
            got.append(torch_mls(rows[s:s + args.chunk], cloud, h2))

    ms = float(np.median(timed_ms(torch_rows, 1)))
    pick = torch.cat([torch.arange(s, s + args.chunk, device=dev) for s in starts])
    far = (torch.cat(got).double() - ungated[pick].double()).norm(dim=1)[moved[pick]]
    print(f"  torch f32 (cdist, einsum, eigh), {n} rows in chunks of {args.chunk}: ms {ms:.3f}, {1e3 * ms / n:.2f} us per "
          f"row, {ms / n * N / 1e3:.1f} s for the whole cloud; its points from the kernel's: rms "
          f"{1e3 * float(far.square().mean().sqrt()):.5f} mm, max {1e3 * float(far.max()):.5f} mm", flush=True)


room = room_points(args.cloud)
run("room 2 cm", room, 0.02)
run("room 5 cm", room, 0.05)
run("thinned 6 cm", downsample_cloud(room, voxel)[0], 2.0 * voxel)
