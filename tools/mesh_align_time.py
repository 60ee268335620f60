#!/usr/bin/env python3
"""Event timing of the mesh-alignment kernels (csrc/mesh_align.hip) on the room volume of tools/mesh_time.py: keyframes
along the synthetic trajectory, 40 000 points each, the config's voxel size and truncation, maintain() before every
fusion (~0.5 M voxels, 136 000 faces at 60 keyframes).  The source is --samples points of the extracted mesh moved by the
inverse of a small Sim3 (2 degrees, 3 cm, scale 0.98); the target is the extracted mesh itself.  Timed, with HIP events
after warm-up, medians of repeated calls:
  * one ICP step (mslam_mesh_align_step: transform, match, closest points, moments, solve) from the identity, cold
    (no warm start) and warm (the faces of the step before), the state and the warm start restored before every call;
  * the un-fused composition on the same points: a torch transform, mslam_mesh_distance(skip=1) with its box pre-pass,
    and a torch reduction of the inlier count and the squared distances.  It yields no closest points, so no moments
    and no solve: it is what an un-fused step costs at least;
  * the box pre-pass with the state initialiser (mslam_mesh_align_init), once per alignment;
  * the share of (wave, tile) scans skipped by the fused step, cold and warm, and by mslam_mesh_distance(skip=2);
  * a whole align_meshes call, and what it returns against the known Sim3.
The fused step's dist2 / nearest are checked against mslam_mesh_distance bit for bit before anything is timed.  Not part
of bench.py.
    python tools/mesh_align_time.py 60 [--reps 20] [--samples 20000]"""
import argparse
import math

import numpy as np
import torch

from _room import build_room, timed   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam import synthetic
from mast3r_slam.config import config
from mast3r_slam.tsdf import align_meshes, sample_mesh, transform_mesh

ap = argparse.ArgumentParser()
ap.add_argument("keyframes", type=int, nargs="+")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--points", type=int, default=40000)
ap.add_argument("--samples", type=int, default=20000)
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = config["tsdf_global"]
vs, trunc = float(cfg["voxel_size"]), float(cfg["trunc_dist"])
print(f"voxel_size={vs} trunc={trunc} points/kf={args.points} samples={args.samples} "
      f"device={torch.cuda.get_device_name(dev)}", flush=True)
L = _m.lib()
TILE, BLOCK, LOG = 128, 256, 24


def sim3(angle_deg, axis, t, s):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    h = 0.5 * math.radians(angle_deg)
    return np.concatenate([np.asarray(t, np.float64), axis * math.sin(h), [math.cos(h)], [s]])


for n_kf in args.keyframes:
    vol = build_room(n_kf, args.points, dev)
    voxels, cap = vol.maintain()
    verts, _, faces = vol.extract_mesh()
    F, V = int(faces.shape[0]), int(verts.shape[0])
    tiles = (F + TILE - 1) // TILE
    print(f"keyframes={n_kf} voxels={voxels} capacity={cap} V={V} F={F} ({tiles} tiles)", flush=True)
    truth = sim3(2.0, (1.0, 2.0, 3.0), (0.02, -0.02, 0.01), 0.98)
    pred = (transform_mesh(verts, synthetic.sim3_inv(truth)), faces)
    n = args.samples
    src = sample_mesh(*pred, n, seed=0)[0]
    nblk = (n + BLOCK - 1) // BLOCK
    waves = (n + 63) // 64
    st = _m.stream_ptr()
    wb = int(L.mslam_mesh_align_workspace_bytes(n, F, 1))
    ws = torch.zeros(wb, dtype=torch.uint8, device=dev)
    state = torch.zeros(72, dtype=torch.uint8, device=dev)
    nearest = torch.full((n,), -1, dtype=torch.int32, device=dev)
    moved = torch.empty((n, 3), dtype=torch.float32, device=dev)
    d2 = torch.empty(n, dtype=torch.float64, device=dev)
    log = torch.zeros(LOG, dtype=torch.float64, device=dev)
    trim = 4.0 * vs

    def init():
        _m.check(L.mslam_mesh_align_init(0, _m.ptr(verts), _m.ptr(faces), F, V, _m.ptr(ws), wb, _m.ptr(state), st),
                 "mesh_align_init")

    def step(count=0):
        _m.check(L.mslam_mesh_align_step(_m.ptr(src), n, _m.ptr(verts), _m.ptr(faces), F, V, trim, 1, count, _m.ptr(ws),
                                         wb, _m.ptr(state), _m.ptr(nearest), _m.ptr(moved), _m.ptr(d2), 0, _m.ptr(log),
                                         st), "mesh_align_step")

    def skipped_share():
        counts = ws.view(torch.int32)[-4 * nblk:].cpu().numpy()[:waves]
        return counts.sum() / (waves * tiles)

    # the un-fused composition
    dws = torch.zeros(int(L.mslam_mesh_distance_workspace_bytes(F)) + 16 * nblk, dtype=torch.uint8, device=dev)
    bd2 = torch.empty(n, dtype=torch.float64, device=dev)
    bnear = torch.empty(n, dtype=torch.int32, device=dev)

    def unfused(skip=1):
        q = src                                                        # the identity, as a transform
        q = (1.0 * (q.double() @ torch.eye(3, dtype=torch.float64, device=dev).T)).float()
        _m.check(L.mslam_mesh_distance(_m.ptr(q), n, _m.ptr(verts), _m.ptr(faces), F, V, skip, _m.ptr(dws),
                                       dws.numel(), _m.ptr(bd2), _m.ptr(bnear), st), "mesh_distance")
        inl = bd2 <= trim * trim
        return inl.sum(), torch.where(inl, bd2, torch.zeros_like(bd2)).sum()

    # the same bits first
    init()
    nearest.fill_(-1)
    step(1)
    cold_share = skipped_share()
    first = nearest.clone()
    unfused(2)
    base_share = dws[-16 * nblk:].view(torch.int32).cpu().numpy()[:waves].sum() / (waves * tiles)
    assert torch.equal(bd2, d2) and torch.equal(bnear, first), "the fused match and mesh_distance differ"
    init()
    nearest.copy_(first)
    step(1)
    warm_share = skipped_share()
    assert torch.equal(bd2, d2) and torch.equal(bnear, nearest), "the warm-started match and mesh_distance differ"
    row = log.cpu().numpy()
    print(f"  one step from the identity: {int(row[0])} of {n} pairs within {trim:.3f}, rmse {row[1]:.6f}", flush=True)
    print(f"  (wave, tile) scans skipped: fused cold {cold_share:.4f}, fused warm {warm_share:.4f}, "
          f"mesh_distance {base_share:.4f}", flush=True)

    def cold_prep():
        init()
        nearest.fill_(-1)

    def warm_prep():
        init()
        nearest.copy_(first)

    for _ in range(2):                                                 # alternating: the spread shows
        print(f"  step_cold_ms {timed(step, args.reps, cold_prep)}", flush=True)
        print(f"  step_warm_ms {timed(step, args.reps, warm_prep)}", flush=True)
        print(f"  unfused_ms {timed(unfused, args.reps)}", flush=True)
    print(f"  init_ms (state and {tiles} boxes) {timed(init, args.reps)}", flush=True)
    kw = dict(n_samples=n, max_iters=50, trim=trim, seed=0)
    res = align_meshes(pred, (verts, faces), **kw)
    T = res["T"].cpu().numpy()
    print(f"  align_meshes: {res['iterations']} iterations, converged {res['converged']}, rmse {res['rmse']:.6f}, "
          f"inliers {res['inliers']}; |t - truth| {np.linalg.norm(T[:3] - truth[:3]):.2e} |q - truth| "
          f"{np.linalg.norm(T[3:7] - truth[3:7]):.2e} |s - truth| {abs(T[7] - truth[7]):.2e}", flush=True)
    print(f"  align_meshes_ms {timed(lambda: align_meshes(pred, (verts, faces), **kw), max(args.reps // 4, 3))}",
          flush=True)
