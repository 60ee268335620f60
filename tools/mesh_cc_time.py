#!/usr/bin/env python3
"""Event timing of the mesh clean-up (csrc/mesh_components.hip) on the room volume of tools/mesh_time.py: keyframes
along the synthetic trajectory, 40 000 points each, the config's voxel size and truncation, maintain() before every
fusion (~0.5 M voxels at 60 keyframes).  Times, with HIP events after warm-up, medians of repeated calls: (a) the
extraction alone, (b) labelling plus counting on its faces, with the wave-aggregated and with the one-atomic-per-element
count, and the label and the two counts on their own, (c) the whole filtered extraction, extract_mesh(
min_component_faces=n).  The mesh is timed at the volume's min_weight and at a higher threshold that breaks it into
many components.  Not part of bench.py.
    python tools/mesh_cc_time.py 60 [--reps 20] [--min-faces 50] [--weights 0 40]"""
import argparse

import torch

from _room import build_room, timed   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam.config import config
from mast3r_slam.tsdf import mesh_components

ap = argparse.ArgumentParser()
ap.add_argument("keyframes", type=int, nargs="+")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--points", type=int, default=40000)
ap.add_argument("--min-faces", type=int, default=50)
ap.add_argument("--weights", type=float, nargs="+", default=(0.0, 40.0), help="min_weight of the mesh; 0 = the volume's")
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = config["tsdf_global"]
vs, trunc = float(cfg["voxel_size"]), float(cfg["trunc_dist"])
print(f"voxel_size={vs} trunc={trunc} points/kf={args.points} device={torch.cuda.get_device_name(dev)}", flush=True)
L = _m.lib()


for n_kf in args.keyframes:
    vol = build_room(n_kf, args.points, dev)
    voxels, cap = vol.maintain()
    for mw in args.weights:
        mw = vol.min_weight if mw <= 0 else mw
        verts, _, faces = vol.extract_mesh(min_weight=mw)
        V, F = int(verts.shape[0]), int(faces.shape[0])
        cf = mesh_components(faces, V)[2]
        kept = int((cf >= args.min_faces).sum())
        print(f"keyframes={n_kf} voxels={voxels} capacity={cap} min_weight={mw:g} V={V} F={F} components={cf.numel()} "
              f"largest={int(cf.max())} faces, {kept} with >= {args.min_faces} faces", flush=True)
        root = torch.empty(V, dtype=torch.int32, device=dev)
        counts = torch.empty((2, V), dtype=torch.int32, device=dev)
        fp, rp, c0, c1, st = _m.ptr(faces), _m.ptr(root), _m.ptr(counts[0]), _m.ptr(counts[1]), _m.stream_ptr()

        def label():
            _m.check(L.mslam_mesh_cc_label(fp, F, V, rp, st), "mesh_cc_label")

        def count(aggregate):
            _m.check(L.mslam_mesh_cc_count(fp, F, V, rp, c0, c1, aggregate, st), "mesh_cc_count")

        print(f"  (a) extract_ms {timed(lambda: vol.extract_mesh(min_weight=mw), args.reps)}", flush=True)
        print(f"  (b) label_ms {timed(label, args.reps)}", flush=True)
        ref = None
        for name, aggregate in (("aggregated", 1), ("naive", 0)) * 2:        # alternating: the spread shows
            print(f"  (b) count_{name}_ms {timed(lambda: count(aggregate), args.reps)}", flush=True)
            print(f"  (b) label+count_{name}_ms {timed(lambda: (label(), count(aggregate)), args.reps)}", flush=True)
            ref = counts.clone() if ref is None else ref
            assert torch.equal(ref, counts), "the two count forms differ"
        print(f"  (c) filtered_extract_ms {timed(lambda: vol.extract_mesh(min_weight=mw, min_component_faces=args.min_faces), args.reps)}",
              flush=True)
