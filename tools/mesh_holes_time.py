#!/usr/bin/env python3
"""Event timing of the mesh holes (csrc/mesh_holes.hip) on the room volume of tools/mesh_time.py: keyframes along the
synthetic trajectory, 40 000 points each, the config's voxel size and truncation, maintain() before every fusion.  The
mesh is timed as extracted and split 1 -> 4 (welded: one midpoint per edge) `--splits` times, which doubles the length of
every boundary loop each time.  Times, with HIP events after warm-up, medians of repeated calls: (a) the dart table (edge
keys, stable sort, mark, compaction with its host read, tails and heads); (b) the link (two sorts and the kernel) and the
doubling rounds alone; (c) the loops (label keys, sort, unique_consecutive with its host read, assign); (d) measure, with
the cap and with every perimeter; (e) fill_holes(16) and mesh_boundaries as a whole, host reads included.  Then the room
figures: the loops found and compare_meshes of the mesh against synthetic.room_mesh() before and after fill_holes, at the
volume's min_weight and at `--min-weight`, where the surface is thinner and has more holes.  (f) the bow-tie mode in
the same run, on the room and on the `--min-weight` mesh: fill_holes(16) against fill_holes(16, bowties=True), the pairing
(directed keys and their sort alone, then the whole of it) and the named loops; the room figures carry a bow-tie row.
Not part of bench.py.
    python tools/mesh_holes_time.py 60 [--reps 20] [--splits 2]"""
import argparse

import torch

from _room import build_room, timed   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam import synthetic
from mast3r_slam.config import config
from mast3r_slam.tsdf import compare_meshes, fill_holes, mesh_boundaries, smooth_mesh
from mast3r_slam.tsdf import mesh_holes as MH

ap = argparse.ArgumentParser()
ap.add_argument("keyframes", type=int, nargs="+")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--points", type=int, default=40000)
ap.add_argument("--splits", type=int, default=2, help="how often the mesh is split 1 -> 4 for the larger sizes")
ap.add_argument("--samples", type=int, default=200000, help="compare_meshes samples per mesh")
ap.add_argument("--max-edges", type=int, default=16)
ap.add_argument("--min-weight", type=float, default=40.0, help="a second extraction with this min_weight")
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = config["tsdf_global"]
vs, trunc = float(cfg["voxel_size"]), float(cfg["trunc_dist"])
print(f"voxel_size={vs} trunc={trunc} points/kf={args.points} device={torch.cuda.get_device_name(dev)}", flush=True)


def split(v, f):
    """Every face into four at its edge midpoints, one midpoint per undirected edge: the mesh stays welded."""
    V = v.shape[0]
    fl = f.long()
    e = torch.cat([fl[:, [0, 1]], fl[:, [1, 2]], fl[:, [2, 0]]])
    key = e.min(1)[0] * V + e.max(1)[0]
    ukey, inv = torch.unique(key, return_inverse=True)
    mid = ((v[ukey // V].double() + v[ukey % V].double()) / 2).float()
    ab, bc, ca = (V + inv[k * len(fl):(k + 1) * len(fl)] for k in range(3))
    a, b, c = fl[:, 0], fl[:, 1], fl[:, 2]
    faces = torch.stack([torch.stack(t, 1) for t in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))], 1)
    return torch.cat([v, mid]).contiguous(), faces.reshape(-1, 3).to(torch.int32).contiguous()


def measure(verts, faces, label):
    V, F = int(verts.shape[0]), int(faces.shape[0])
    dart, tail, head = MH._darts(faces, V, F)
    B = int(dart.shape[0])
    if B == 0:
        print(f"{label}: V={V} F={F} watertight", flush=True)
        return
    state = MH._link(tail, head, V)
    rounds = MH._rounds(B)
    labelled = MH._double(state, rounds)
    tr = MH._trace(faces, V, F)
    nl = int(tr["loop_id"].shape[0])
    longest = int(tr["length"].max()) if nl else 0
    small = int((tr["length"] <= args.max_edges).sum()) if nl else 0
    print(f"{label}: V={V} F={F} boundary_darts={B} loops={nl} longest={longest} loops_within_cap={small} "
          f"open_darts={int(tr['n_open'])} doubling_rounds={rounds}", flush=True)
    print(f"  (a) dart_table_ms {timed(lambda: MH._darts(faces, V, F), args.reps)}", flush=True)
    print(f"  (b) link_ms {timed(lambda: MH._link(tail, head, V), args.reps)}", flush=True)
    print(f"  (b) doubling_{rounds}_rounds_ms {timed(lambda: MH._double(state, rounds), args.reps)}", flush=True)
    print(f"  (c) loops_ms {timed(lambda: MH._loops(state, labelled), args.reps)}", flush=True)
    print(f"  (d) measure_capped_ms "
          f"{timed(lambda: MH._measure(verts, faces, V, F, tr, args.max_edges, False), args.reps)}", flush=True)
    print(f"  (d) measure_every_perimeter_ms "
          f"{timed(lambda: MH._measure(verts, faces, V, F, tr, args.max_edges, True), args.reps)}", flush=True)
    mesh = (verts, torch.zeros_like(verts), faces)
    out = fill_holes(mesh, args.max_edges, return_info=True)
    print(f"  (e) fill_holes_{args.max_edges}_ms {timed(lambda: fill_holes(mesh, args.max_edges), args.reps)} "
          f"(filled {int(out[-1]['loop_filled'].sum())} loops, {int(out[2].shape[0]) - F} new faces)", flush=True)
    print(f"  (e) fill_holes_{args.max_edges}_unvalidated_ms "
          f"{timed(lambda: fill_holes(mesh, args.max_edges, _validate=False), args.reps)}", flush=True)
    print(f"  (e) mesh_boundaries_ms {timed(lambda: mesh_boundaries(faces, V, _validate=False), args.reps)}", flush=True)


def bowties(verts, faces, label):
    """(f): the plain call against the bow-tie mode on one mesh, and where the bow-tie mode's time goes."""
    V, F = int(verts.shape[0]), int(faces.shape[0])
    mesh = (verts, torch.zeros_like(verts), faces)
    dart, tail, head = MH._darts(faces, V, F)
    B = int(dart.shape[0])
    if B == 0:
        return
    out = fill_holes(mesh, args.max_edges, return_info=True, bowties=True)
    info = out[-1]
    print(f"  (f) {label} bowties: loops={int(info['loop_id'].shape[0])} longest={int(info['loop_length'].max())} "
          f"filled={int(info['loop_filled'].sum())} new_faces={int(out[2].shape[0]) - F} "
          f"open_darts={int(info['n_open'])} of {B}", flush=True)
    print(f"  (f) {label} fill_holes_{args.max_edges}_ms {timed(lambda: fill_holes(mesh, args.max_edges), args.reps)}",
          flush=True)
    print(f"  (f) {label} fill_holes_{args.max_edges}_bowties_ms "
          f"{timed(lambda: fill_holes(mesh, args.max_edges, bowties=True), args.reps)}", flush=True)
    print(f"  (f) {label} mesh_boundaries_bowties_ms "
          f"{timed(lambda: mesh_boundaries(faces, V, bowties=True, _validate=False), args.reps)}", flush=True)

    def directed():
        keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
        _m.check(_m.lib().mslam_mesh_holes_dkeys(_m.ptr(faces), F, V, _m.ptr(keys), _m.stream_ptr()), "dkeys")
        return torch.sort(keys, stable=True)

    paired = MH._pair(faces, V, F, dart, tail, head)

    def named_loops():
        labelled = MH._double(paired, MH._rounds(B))
        return MH._loops(paired, labelled, MH._tail_flag(labelled, tail, V), tail, head)

    print(f"  (f) {label} directed_keys_sort_ms {timed(directed, args.reps)}", flush=True)
    print(f"  (f) {label} pair_ms {timed(lambda: MH._pair(faces, V, F, dart, tail, head), args.reps)}", flush=True)
    print(f"  (f) {label} named_loops_ms {timed(named_loops, args.reps)}", flush=True)


def quality(mesh, gt, label):
    m = compare_meshes(mesh, gt, n_samples=args.samples, threshold=float(cfg["mesh_eval_threshold"]))
    print(f"  {label}: V={int(mesh[0].shape[0])} F={int(mesh[2].shape[0])} accuracy={m['accuracy']:.5f} "
          f"completion={m['completion']:.5f} precision={m['precision']:.4f} recall={m['recall']:.4f} "
          f"fscore={m['fscore']:.4f}", flush=True)


for n_kf in args.keyframes:
    vol = build_room(n_kf, args.points, dev)
    voxels, cap = vol.maintain()
    mesh = vol.extract_mesh()
    print(f"keyframes={n_kf} voxels={voxels} capacity={cap}", flush=True)
    v, f = mesh[0], mesh[2]
    measure(v, f, "room")
    bowties(v, f, "room")
    for k in range(args.splits):
        v, f = split(v, f)
        measure(v, f, f"room split {k + 1}x")
    gt = tuple(torch.from_numpy(a).to(dev) for a in synthetic.room_mesh())
    print(f"room figures against synthetic.room_mesh() ({args.samples} samples, threshold "
          f"{cfg['mesh_eval_threshold']}):", flush=True)
    for mw in (None, args.min_weight):
        mesh = vol.extract_mesh(min_weight=mw)
        out = fill_holes(mesh, args.max_edges, return_info=True)
        info = out[-1]
        hist = torch.bincount(info["loop_length"].long().clamp(max=args.max_edges + 1)).tolist()
        print(f" min_weight={vol.min_weight if mw is None else mw}: boundary_darts={int(info['n_boundary_edges'])} "
              f"loops={int(info['loop_id'].shape[0])} filled={int(info['loop_filled'].sum())} "
              f"open_darts={int(info['n_open'])} loops by length 0..{args.max_edges}, longer: {hist}", flush=True)
        quality(mesh, gt, "as extracted")
        quality(out[:3], gt, f"fill_holes={args.max_edges}")
        quality(smooth_mesh(out[:3], 5), gt, f"fill_holes={args.max_edges} + 5 iterations")
        both = fill_holes(mesh, args.max_edges, return_info=True, bowties=True)
        info = both[-1]
        print(f"  bowties: loops={int(info['loop_id'].shape[0])} filled={int(info['loop_filled'].sum())} "
              f"open_darts={int(info['n_open'])} of {int(info['n_boundary_edges'])}", flush=True)
        quality(both[:3], gt, f"fill_holes={args.max_edges}, bowties")
        quality(smooth_mesh(both[:3], 5), gt, f"fill_holes={args.max_edges}, bowties + 5 iterations")
        if mw is not None:
            bowties(mesh[0], mesh[2], f"min_weight={mw}")
