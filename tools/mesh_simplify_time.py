#!/usr/bin/env python3
"""Event timing of the mesh simplification (csrc/mesh_simplify.hip) on the room volume of tools/mesh_time.py: keyframes
along the synthetic trajectory, 40 000 points each, the config's voxel size and truncation, maintain() before every
fusion (~0.5 M voxels at 60 keyframes).  Times, with HIP events after warm-up, medians of repeated calls: (a) the
extraction alone, the yardstick; (b) the stages of simplify_mesh on its mesh, each on its own line, launched as
simplify_mesh launches them but without its host reads: key sort (cell keys, stable sort, cluster numbering), face sort
(triples, their keys, the sort), pair sort ((cluster, face) keys and their run starts), solve (the per-cluster kernel),
emit (mark, scan, gather); (c) simplify_mesh as a whole and extract_mesh(simplify_cell=c), host reads included.  Cells of
2 and 4 voxels, both positions; V / F in and out, the clusters that fell back to their mean, and compare_meshes of every
result against the unsimplified mesh.  Not part of bench.py.
    python tools/mesh_simplify_time.py 60 [--reps 20] [--cells 2 4]"""
import argparse

import torch

from _room import build_room, timed   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam.config import config
from mast3r_slam.tsdf import compare_meshes, simplify_mesh

ap = argparse.ArgumentParser()
ap.add_argument("keyframes", type=int, nargs="+")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--points", type=int, default=40000)
ap.add_argument("--cells", type=float, nargs="+", default=(2.0, 4.0), help="cell sizes in voxels")
ap.add_argument("--samples", type=int, default=200000, help="compare_meshes samples per mesh")
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = config["tsdf_global"]
vs, trunc = float(cfg["voxel_size"]), float(cfg["trunc_dist"])
print(f"voxel_size={vs} trunc={trunc} points/kf={args.points} device={torch.cuda.get_device_name(dev)}", flush=True)
L = _m.lib()
i32, i64, f32 = (dict(dtype=d, device=dev) for d in (torch.int32, torch.int64, torch.float32))


class Stages:
    """simplify_mesh's launches, stage by stage, on buffers that persist between the stages."""

    def __init__(self, mesh, c, quadric):
        self.verts, self.normals, self.faces = mesh
        self.V, self.F, self.c, self.quadric = int(mesh[0].shape[0]), int(mesh[2].shape[0]), float(c), int(quadric)
        self.st = _m.stream_ptr()
        self.key_sort()
        self.C = int(self.cid[-1]) + 1
        self.ids = torch.arange(self.C + 1, **i64)
        for stage in (self.key_sort, self.face_sort, self.pair_sort, self.solve, self.emit):
            stage()

    def key_sort(self):
        keys = torch.empty(self.V, **i64)
        _m.check(L.mslam_mesh_simplify_keys(_m.ptr(self.verts), self.V, self.c, _m.ptr(keys), self.st), "keys")
        self.sorted_keys, self.vorder = torch.sort(keys, stable=True)
        head = torch.ones(self.V, dtype=torch.bool, device=dev)
        head[1:] = self.sorted_keys[1:] != self.sorted_keys[:-1]
        self.cid = torch.cumsum(head, 0) - 1
        self.cluster = torch.empty(self.V, **i32)
        self.cluster[self.vorder] = self.cid.to(torch.int32)
        if hasattr(self, "ids"):
            self.vstart = torch.searchsorted(self.cid, self.ids)

    def face_sort(self):
        self.tri, key = torch.empty((self.F, 3), **i32), torch.empty(self.F, **i64)
        self.pairs = torch.empty(3 * self.F, **i64)
        _m.check(L.mslam_mesh_simplify_faces(_m.ptr(self.faces), self.F, self.V, _m.ptr(self.cluster), self.C, 1,
                                             _m.ptr(self.tri), 0, _m.ptr(key), _m.ptr(self.pairs), self.st), "faces")
        self.forder = torch.sort(key, stable=True)[1]

    def pair_sort(self):
        self.sorted_pairs = torch.sort(self.pairs)[0]
        self.pstart = torch.searchsorted(self.sorted_pairs, self.ids * self.F)

    def solve(self):
        self.out = [torch.empty((self.C, 3), **f32) for _ in range(2)]
        self.fallback = torch.empty(self.C, **i32)
        _m.check(L.mslam_mesh_simplify_solve(_m.ptr(self.verts), _m.ptr(self.normals), 0, _m.ptr(self.faces), self.F,
                                             self.V, self.c, _m.ptr(self.sorted_keys), _m.ptr(self.vorder),
                                             _m.ptr(self.vstart), _m.ptr(self.sorted_pairs), _m.ptr(self.pstart), self.C,
                                             self.quadric, _m.ptr(self.out[0]), _m.ptr(self.out[1]), 0,
                                             _m.ptr(self.fallback), self.st), "solve")

    def emit(self):
        C, F = self.C, self.F
        flags = torch.zeros(C + F, **i32)
        sorted_tri = torch.empty((F, 3), **i32)
        _m.check(L.mslam_mesh_simplify_mark(_m.ptr(self.tri), _m.ptr(self.forder), F, C, _m.ptr(sorted_tri),
                                            _m.ptr(flags[C:]), _m.ptr(flags), self.st), "mark")
        incl = torch.cumsum(flags, 0)
        if not hasattr(self, "sizes"):                                   # the one host read, outside the timed calls
            n_v, n_vf = (int(x) for x in incl[[C - 1, C + F - 1]].cpu())
            self.sizes = (n_v, n_vf - n_v)
        n_v, n_f = self.sizes
        base = incl - flags
        base[C:] -= n_v
        res = [torch.empty((n_v, 3), **f32) for _ in range(2)]
        out_faces = torch.empty((n_f, 3), **i32)
        _m.check(L.mslam_mesh_cc_emit(_m.ptr(self.out[0]), _m.ptr(self.out[1]), 0, _m.ptr(sorted_tri), F, C,
                                      _m.ptr(flags), _m.ptr(flags[C:]), _m.ptr(base), _m.ptr(base[C:]), _m.ptr(res[0]),
                                      _m.ptr(res[1]), 0, _m.ptr(out_faces), n_v, n_f, self.st), "emit")
        self.flags = flags
        self.result = (res[0], res[1], out_faces)


for n_kf in args.keyframes:
    vol = build_room(n_kf, args.points, dev)
    voxels, cap = vol.maintain()
    mesh = vol.extract_mesh()
    V, F = int(mesh[0].shape[0]), int(mesh[2].shape[0])
    print(f"keyframes={n_kf} voxels={voxels} capacity={cap} V={V} F={F}", flush=True)
    print(f"  (a) extract_ms {timed(lambda: vol.extract_mesh(), args.reps)}", flush=True)
    for cells in args.cells:
        c = cells * vs
        for position in ("quadric", "mean"):
            s = Stages(mesh, c, position == "quadric")
            ref = simplify_mesh(mesh, c, position=position)
            assert all(torch.equal(a, b) for a, b in zip(s.result, ref)), "the staged launches differ from simplify_mesh"
            used = s.flags[:s.C] > 0
            print(f"  cell={cells:g} voxels position={position}: clusters={s.C} V'={s.sizes[0]} F'={s.sizes[1]} "
                  f"(V/V'={V / max(s.sizes[0], 1):.1f} F/F'={F / max(s.sizes[1], 1):.1f}) fell_back="
                  f"{int((s.fallback[used] > 0).sum()) if position == 'quadric' else 'all'}", flush=True)
            stages = [("key_sort", s.key_sort), ("face_sort", s.face_sort), ("solve", s.solve), ("emit", s.emit)]
            if position == "quadric":
                stages.insert(2, ("pair_sort", s.pair_sort))
            for name, fn in stages:
                print(f"    (b) {name}_ms {timed(fn, args.reps)}", flush=True)
            print(f"    (c) simplify_mesh_ms {timed(lambda: simplify_mesh(mesh, c, position=position), args.reps)}", flush=True)
            print(f"    (c) simplify_mesh_unvalidated_ms "
                  f"{timed(lambda: simplify_mesh(mesh, c, position=position, _validate=False), args.reps)}", flush=True)
            print(f"    (c) simplified_extract_ms "
                  f"{timed(lambda: vol.extract_mesh(simplify_cell=c, simplify_position=position), args.reps)}", flush=True)
            m = compare_meshes(ref, mesh, n_samples=args.samples, threshold=vs)
            print(f"    vs input ({args.samples} samples, threshold one voxel): out->in mean={m['accuracy']:.5f} "
                  f"median={m['accuracy_median']:.5f} within={m['precision']:.4f}; in->out mean={m['completion']:.5f} "
                  f"median={m['completion_median']:.5f} within={m['recall']:.4f}; area {m['pred_area']:.3f} / "
                  f"{m['gt_area']:.3f}", flush=True)
