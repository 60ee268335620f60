#!/usr/bin/env python3
"""Event timing of the mesh decimation (csrc/mesh_decimate.hip) on the room volume of tools/mesh_time.py: keyframes along
the synthetic trajectory, 40 000 points each, the config's voxel size and truncation, maintain() before every fusion.
Times, with HIP events after warm-up, medians of repeated calls: (a) the extraction and simplify_mesh at two voxels of
the same run, for scale; (b) the pieces of one round on the full mesh (the tables keep their size over the rounds, the
working faces are not compacted): the two table builds (edge keys, sort, unique_consecutive with its host read; pair keys,
sort), the candidates kernel, the two rank sorts, the two spreads, the apply launches; the one-off state kernel and the
finish with its emit; (c) decimate_mesh as a whole at each ratio, host reads included, with its rounds and collapses, and
what is left of the total per round.  Not part of bench.py.
    python tools/mesh_decimate_time.py 60 [--reps 10] [--ratios 0.5 0.2 0.05]"""
import argparse

import numpy as np
import torch

from _room import build_room, timed, timed_ms   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam.config import config
from mast3r_slam.tsdf import decimate_mesh, simplify_mesh
from mast3r_slam.tsdf import mesh_decimate as MD
from mast3r_slam.tsdf import mesh_smooth as MS

ap = argparse.ArgumentParser()
ap.add_argument("keyframes", type=int, nargs="+")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--points", type=int, default=40000)
ap.add_argument("--ratios", type=float, nargs="+", default=[0.5, 0.2, 0.05])
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = config["tsdf_global"]
vs = float(cfg["voxel_size"])
print(f"voxel_size={vs} points/kf={args.points} device={torch.cuda.get_device_name(dev)}", flush=True)
L = _m.lib()


def median(fn, prep=None):
    return float(np.median(timed_ms(fn, args.reps, prep)))


def one_round(verts, faces):
    """The pieces of round 0, each timed on its own -> their medians in ms."""
    V, F = int(verts.shape[0]), int(faces.shape[0])
    st = _m.stream_ptr()
    cur = faces.clone()
    pairs, pstart = MS._face_table(cur, V, F)
    state = torch.empty((V, MD._STATE), dtype=torch.float64, device=dev)

    def state_kernel():
        _m.check(L.mslam_mesh_decimate_state(_m.ptr(verts), _m.ptr(cur), F, V, _m.ptr(pairs), _m.ptr(pstart),
                                             _m.ptr(state), st), "state")

    state_kernel()
    tab = MD._Round(verts, cur, V, F, state, -1.0, 0, False)
    out = dict(state_kernel=median(state_kernel),
               sort_edge_table=median(lambda: MS._neighbour_table(cur, V, F)),
               sort_face_table=median(lambda: MS._face_table(cur, V, F)))

    def candidates():
        _m.check(L.mslam_mesh_decimate_candidates(_m.ptr(verts), _m.ptr(cur), F, V, _m.ptr(tab.row_start),
                                                  _m.ptr(tab.nbr), _m.ptr(tab.mult), tab.E, _m.ptr(pairs),
                                                  _m.ptr(pstart), _m.ptr(state), -1.0, 0, _m.ptr(tab.best),
                                                  _m.ptr(tab.cost), _m.ptr(tab.key), 0, st), "candidates")

    out["kernel_candidates"] = median(candidates)

    def rank_sorts():
        by_key = torch.sort(tab.key)[1]
        return by_key[torch.sort(tab.cost[by_key], stable=True)[1]]

    out["sort_rank"] = median(rank_sorts)
    out["kernel_select_with_rank_sorts"] = median(lambda: tab.select(V))
    selected, _ = tab.select(V)
    sel8 = selected.to(torch.uint8)
    work, wstate = cur.clone(), state.clone()
    parent = torch.arange(V, dtype=torch.int32, device=dev)

    def fresh():
        work.copy_(cur), wstate.copy_(state)

    def apply():
        _m.check(L.mslam_mesh_decimate_apply(_m.ptr(work), F, V, _m.ptr(sel8), _m.ptr(tab.best), _m.ptr(wstate),
                                             _m.ptr(parent), st), "apply")

    out["kernel_apply"] = median(apply, fresh)
    out["candidates"] = int((tab.best >= 0).sum())
    out["selected"] = int(selected.sum())
    return out


for n_kf in args.keyframes:
    vol = build_room(n_kf, args.points, dev)
    voxels, cap = vol.maintain()
    mesh = vol.extract_mesh()
    V, F = int(mesh[0].shape[0]), int(mesh[2].shape[0])
    print(f"keyframes={n_kf} voxels={voxels} capacity={cap} V={V} F={F}", flush=True)
    print(f"  (a) extract_mesh_ms {timed(lambda: vol.extract_mesh(), args.reps)}", flush=True)
    print(f"  (a) simplify_mesh_2_voxels_ms {timed(lambda: simplify_mesh(mesh, 2 * vs), args.reps)} "
          f"-> F={int(simplify_mesh(mesh, 2 * vs)[2].shape[0])}", flush=True)
    r = one_round(mesh[0], mesh[2])
    sorts = r["sort_edge_table"] + r["sort_face_table"] + r["sort_rank"]
    kernels = r["kernel_candidates"] + (r["kernel_select_with_rank_sorts"] - r["sort_rank"]) + r["kernel_apply"]
    print(f"  (b) round 0: candidates={r['candidates']} selected={r['selected']} "
          f"({100.0 * r['selected'] / max(V, 1):.2f} % of the vertices)", flush=True)
    for k in ("state_kernel", "sort_edge_table", "sort_face_table", "kernel_candidates", "sort_rank",
              "kernel_select_with_rank_sorts", "kernel_apply"):
        print(f"  (b) {k}_ms median={r[k]:.3f}", flush=True)
    print(f"  (b) per round: sorts_and_scans_ms {sorts:.3f} kernels_ms {kernels:.3f}", flush=True)
    for ratio in args.ratios:
        out = decimate_mesh(mesh, ratio=ratio, return_info=True)
        info = out[-1]
        ms = timed_ms(lambda: decimate_mesh(mesh, ratio=ratio), args.reps)
        total = float(np.median(ms))
        rounds = max(info["rounds"], 1)
        print(f"  (c) ratio={ratio}: F={int(out[2].shape[0])} V={int(out[0].shape[0])} rounds={info['rounds']} "
              f"collapses_first_last={info['collapses'][:1].tolist()}{info['collapses'][-1:].tolist()} "
              f"max_cost={info['max_cost']:.3e} decimate_mesh_ms median={total:.3f} min={min(ms):.3f} max={max(ms):.3f} "
              f"per_round_ms {total / rounds:.3f} (sorts and scans {sorts:.3f}, kernels {kernels:.3f}, the rest: host "
              f"reads, launches and torch glue)", flush=True)
