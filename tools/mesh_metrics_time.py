#!/usr/bin/env python3
"""Event timing of the mesh-quality kernels (csrc/mesh_distance.hip) on the room volume of tools/mesh_time.py: keyframes
along the synthetic trajectory, 40 000 points each, the config's voxel size and truncation, maintain() before every
fusion (~0.5 M voxels, 136 000 faces at 60 keyframes).  Three queries at --samples points each: (a) samples of the
extracted mesh against synthetic.room_mesh() (12 faces), (b) samples of the room mesh against the extracted mesh,
(c) samples of the extracted mesh against itself.  For each: the sampling (areas, cumulative sum, host read, samples),
the distance with culling (skip = 1, boxes included) and without (skip = 0), HIP events after warm-up, medians of
repeated calls, the share of (wave, tile) scans the culled form skipped, and a check that both forms return the same
bits.  Not part of bench.py.
    python tools/mesh_metrics_time.py 60 [--reps 20] [--samples 200000]"""
import argparse

import torch

from _room import build_room, timed   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam import synthetic
from mast3r_slam.config import config
from mast3r_slam.tsdf import compare_meshes, sample_mesh

ap = argparse.ArgumentParser()
ap.add_argument("keyframes", type=int, nargs="+")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--points", type=int, default=40000)
ap.add_argument("--samples", type=int, default=200000)
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = config["tsdf_global"]
vs, trunc = float(cfg["voxel_size"]), float(cfg["trunc_dist"])
print(f"voxel_size={vs} trunc={trunc} points/kf={args.points} samples={args.samples} "
      f"device={torch.cuda.get_device_name(dev)}", flush=True)
L = _m.lib()
TILE, BLOCK = 128, 256


def distance(points, verts, faces, skip, ws):
    n, F, V = int(points.shape[0]), int(faces.shape[0]), int(verts.shape[0])
    d2 = torch.empty(n, dtype=torch.float64, device=dev)
    near = torch.empty(n, dtype=torch.int32, device=dev)
    _m.check(L.mslam_mesh_distance(_m.ptr(points), n, _m.ptr(verts), _m.ptr(faces), F, V, skip, _m.ptr(ws),
                                   ws.numel(), _m.ptr(d2), _m.ptr(near), _m.stream_ptr()), "mesh_distance")
    return d2, near


rv, rf = synthetic.room_mesh()
room = (torch.from_numpy(rv).to(dev), torch.from_numpy(rf).to(dev))
for n_kf in args.keyframes:
    vol = build_room(n_kf, args.points, dev)
    voxels, cap = vol.maintain()
    verts, _, faces = vol.extract_mesh()
    mesh = (verts, faces)
    print(f"keyframes={n_kf} voxels={voxels} capacity={cap} V={verts.shape[0]} F={faces.shape[0]}", flush=True)
    n = args.samples
    nblk = (n + BLOCK - 1) // BLOCK
    for name, src, dst in (("(a) mesh samples -> room mesh", mesh, room), ("(b) room samples -> mesh", room, mesh),
                           ("(c) mesh samples -> mesh", mesh, mesh)):
        F = int(dst[1].shape[0])
        tiles = (F + TILE - 1) // TILE
        box = int(L.mslam_mesh_distance_workspace_bytes(F))
        ws = torch.zeros(box + 16 * nblk, dtype=torch.uint8, device=dev)
        print(f"  {name}: {n} points x {F} faces ({tiles} tiles)", flush=True)
        print(f"    sample_ms {timed(lambda: sample_mesh(*src, n, seed=0, _validate=False), args.reps)}", flush=True)
        pts = sample_mesh(*src, n, seed=0)[0]
        ref = distance(pts, *dst, 0, ws)
        got = distance(pts, *dst, 2, ws)
        assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1]), "culled and plain scans differ"
        counts = ws[box:].view(torch.int32).cpu().numpy()[:(n + 63) // 64]
        share = counts.sum() / (len(counts) * tiles)
        for label, skip in (("skip", 1), ("plain", 0)) * 2:            # alternating: the spread shows
            print(f"    distance_{label}_ms {timed(lambda: distance(pts, *dst, skip, ws), args.reps)}", flush=True)
        print(f"    tile share skipped {share:.4f}; mean distance {float(torch.sqrt(ref[0]).mean()):.6f}", flush=True)
    m = compare_meshes(mesh, room, n_samples=n, threshold=vs)
    print(f"  compare_meshes(mesh, room, threshold={vs}): " + " ".join(
        f"{k}={m[k]:.5f}" for k in ("accuracy", "completion", "precision", "recall", "fscore", "chamfer")), flush=True)
    print(f"  compare_meshes_ms {timed(lambda: compare_meshes(mesh, room, n_samples=n, threshold=vs), args.reps)}",
          flush=True)
