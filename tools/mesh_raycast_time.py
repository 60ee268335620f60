#!/usr/bin/env python3
"""Event timing of the mesh ray caster (csrc/mesh_raycast.hip) on the room volume of tools/mesh_time.py: keyframes along
the synthetic trajectory, 40 000 points each, the config's voxel size and truncation, maintain() before every fusion.
(1) One 384x512 pinhole view (the camera of the middle keyframe) of the extracted mesh and of synthetic.room_mesh()
(12 faces): the tile boxes, the cast with culling (skip = 1) and without (skip = 0) in one process, HIP events after
warm-up, medians of repeated calls; both forms are compared byte for byte before anything is timed.  (2)
observed_points for --samples surface samples over the keyframes' cameras at 384x512: samples of the room mesh against
the room mesh (what compare_meshes(observed=...) runs on a ground truth) and samples of the extracted mesh against the
extracted mesh, culled and plain.  Not part of bench.py.
    python tools/mesh_raycast_time.py 60 [--reps 20] [--samples 200000]"""
import argparse

import numpy as np
import torch

from _room import build_room, timed   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam import synthetic
from mast3r_slam.config import config
from mast3r_slam.tsdf import observed_points, sample_mesh
from mast3r_slam.tsdf.global_volume import pinhole_rays

ap = argparse.ArgumentParser()
ap.add_argument("keyframes", type=int, nargs="+")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--points", type=int, default=40000)
ap.add_argument("--samples", type=int, default=200000)
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = config["tsdf_global"]
H, W = 384, 512
print(f"voxel_size={float(cfg['voxel_size'])} trunc={float(cfg['trunc_dist'])} points/kf={args.points} "
      f"samples={args.samples} view={H}x{W} device={torch.cuda.get_device_name(dev)}", flush=True)
L = _m.lib()
K = synthetic.intrinsics(H, W)
rays = pinhole_rays(K, (H, W), dev).reshape(-1, 3).contiguous()


def boxes(verts, faces, ws):
    _m.check(L.mslam_mesh_raycast_boxes(_m.ptr(verts), _m.ptr(faces), int(faces.shape[0]), int(verts.shape[0]),
                                        _m.ptr(ws), ws.numel(), _m.stream_ptr()), "mesh_raycast_boxes")


def cast(pose, verts, faces, skip, ws):
    n = H * W
    out = (torch.empty(n, dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev),
           torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
           torch.empty(n, dtype=torch.float64, device=dev))
    _m.check(L.mslam_mesh_raycast(_m.ptr(rays), H, W, _m.ptr(pose), _m.ptr(verts), _m.ptr(faces), int(faces.shape[0]),
                                  int(verts.shape[0]), 0.05, 10.0, skip, _m.ptr(ws), ws.numel(), *(_m.ptr(t) for t in out),
                                  _m.stream_ptr()), "mesh_raycast")
    return out


rv, rf = synthetic.room_mesh()
room = (torch.from_numpy(rv).to(dev), torch.from_numpy(rf).to(dev))
for n_kf in args.keyframes:
    vol = build_room(n_kf, args.points, dev)
    voxels, cap = vol.maintain()
    verts, _, faces = vol.extract_mesh()
    mesh = (verts, faces)
    cams = np.stack([synthetic.camera_pose(i * (1000 // n_kf)) for i in range(n_kf)]).astype(np.float32)
    pose = torch.from_numpy(cams[n_kf // 2]).to(dev)
    print(f"keyframes={n_kf} voxels={voxels} capacity={cap} V={verts.shape[0]} F={faces.shape[0]}", flush=True)
    for name, (v, f) in (("extracted mesh", mesh), ("room mesh", room)):
        F = int(f.shape[0])
        ws = torch.empty(int(L.mslam_mesh_raycast_workspace_bytes(F)), dtype=torch.uint8, device=dev)
        boxes(v, f, ws)
        ref, got = cast(pose, v, f, 0, ws), cast(pose, v, f, 1, ws)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(ref, got)), \
            "culled and plain casts differ"
        print(f"  (1) {H}x{W} view of the {name}: {H * W} rays x {F} faces ({(F + 127) // 128} tiles), hit share "
              f"{float(ref[2].float().mean()):.4f}, mean range {float(ref[0][ref[2] > 0].mean()):.4f}", flush=True)
        print(f"    boxes_ms {timed(lambda: boxes(v, f, ws), args.reps)}", flush=True)
        for label, skip in (("skip", 1), ("plain", 0)) * 2:            # alternating: the spread shows
            print(f"    cast_{label}_ms {timed(lambda: cast(pose, v, f, skip, ws), args.reps)}", flush=True)
    for name, m in (("room mesh", room), ("extracted mesh", mesh)):
        pts = sample_mesh(*m, args.samples, seed=1)[0]
        seen = observed_points(pts, m, cams, K, (H, W))
        same = observed_points(pts, m, cams, K, (H, W), skip=False, compact_every=0)
        assert torch.equal(seen, same), "observed_points depends on culling or compaction"
        print(f"  (2) observed_points, {args.samples} samples of the {name} against it, {n_kf} cameras: observed share "
              f"{float(seen.float().mean()):.4f}", flush=True)
        reps = max(1, args.reps // 10)
        print(f"    observed_skip_ms {timed(lambda: observed_points(pts, m, cams, K, (H, W)), reps)}", flush=True)
        print(f"    observed_plain_ms {timed(lambda: observed_points(pts, m, cams, K, (H, W), skip=False), reps)}",
              flush=True)
        print(f"    observed_skip_nocompact_ms "
              f"{timed(lambda: observed_points(pts, m, cams, K, (H, W), compact_every=0), reps)}", flush=True)
