#!/usr/bin/env python3
"""Event timing of the mesh index (csrc/mesh_index.hip, DESIGN.md "Mesh index") on the room volume of tools/mesh_time.py.
Mesh A is the extracted mesh; mesh B is mesh A with every face split at its edge midpoints --split times (children stay
neighbours, so its order is as coherent as A's).  For each: the distance of --samples samples of the mesh's own surface
(in face order) and one 384x512 view from the middle keyframe, in four forms timed in one process, alternated, HIP events
after warm-up, medians:
    (i)   faces in extraction order, the existing culled path (the yardstick)
    (ii)  faces shuffled, the existing culled path
    (iii) faces shuffled, indexed
    (iv)  faces in extraction order, indexed
and for the indexed forms also with the group level off (levels = 1).  Every form is compared byte for byte with the
plain scan (skip = 0) of its mesh first, and the skipped share of (wave, tile) scans is printed beside each time.  The
build time of the index (keys, sort, boxes) is reported separately.  Not part of bench.py.
    python tools/mesh_index_time.py 60 [--reps 10] [--samples 200000] [--split 2]"""
import argparse

import torch

from _room import build_room, timed   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam import synthetic
from mast3r_slam.tsdf import MeshIndex, sample_mesh
from mast3r_slam.tsdf.global_volume import pinhole_rays

ap = argparse.ArgumentParser()
ap.add_argument("keyframes", type=int)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--points", type=int, default=40000)
ap.add_argument("--samples", type=int, default=200000)
ap.add_argument("--split", type=int, default=2)
args = ap.parse_args()
dev = torch.device("cuda:0")
H, W = 384, 512
L = _m.lib()
K = synthetic.intrinsics(H, W)
rays = pinhole_rays(K, (H, W), dev).reshape(-1, 3).contiguous()
print(f"points/kf={args.points} samples={args.samples} view={H}x{W} device={torch.cuda.get_device_name(dev)}", flush=True)


def split(v, f):
    """Every face into four at its edge midpoints (f64 midpoints rounded to f32; a soup)."""
    a, b, c = (v[f[:, k].long()].double() for k in range(3))
    ab, bc, ca = (a + b) / 2, (b + c) / 2, (c + a) / 2
    tri = torch.stack([torch.stack(t, 1) for t in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))], 1)
    v = tri.reshape(-1, 3).float().contiguous()
    return v, torch.arange(v.shape[0], dtype=torch.int32, device=v.device).reshape(-1, 3)


class Form:
    """One mesh in one face order: the existing culled path and the indexed one."""

    def __init__(self, v, f):
        self.v, self.f, self.V, self.F = v, f, int(v.shape[0]), int(f.shape[0])
        self.ix = MeshIndex(v, f, validate=False)
        self.ws = torch.empty(int(L.mslam_mesh_raycast_workspace_bytes(self.F)), dtype=torch.uint8, device=dev)
        _m.check(L.mslam_mesh_raycast_boxes(_m.ptr(v), _m.ptr(f), self.F, self.V, _m.ptr(self.ws), self.ws.numel(),
                                            _m.stream_ptr()), "mesh_raycast_boxes")

    def existing_ray_share(self, pose, waves):
        """The existing cast keeps no counts: its skipped share is the indexed entry's over the identity order with the
        tiles alone, which is the existing scan over the existing tiles."""
        order = torch.arange(self.F, dtype=torch.int32, device=dev)
        ws = torch.empty(int(L.mslam_mesh_index_bytes(self.F)), dtype=torch.uint8, device=dev)
        _m.check(L.mslam_mesh_index_boxes(_m.ptr(self.v), _m.ptr(self.f), self.F, self.V, _m.ptr(order), _m.ptr(ws),
                                          ws.numel(), _m.stream_ptr()), "mesh_index_boxes")
        keep = self.ix.order, self.ix.ws
        self.ix.order, self.ix.ws = order, ws
        try:
            return share(self.cast(pose, ("index", 1))[5], waves, self.F)
        finally:
            self.ix.order, self.ix.ws = keep

    def distance(self, pts, how):
        """how: 0 plain, 1 the existing culled path (with counts), ("index", levels)"""
        n = int(pts.shape[0])
        d2 = torch.empty(n, dtype=torch.float64, device=dev)
        near = torch.empty(n, dtype=torch.int32, device=dev)
        nblk = (n + 255) // 256
        if isinstance(how, tuple):
            counts = torch.zeros(4 * nblk, dtype=torch.int32, device=dev)
            _m.check(L.mslam_mesh_distance_indexed(_m.ptr(pts), n, _m.ptr(self.v), _m.ptr(self.f), self.F, self.V,
                                                   _m.ptr(self.ix.order), _m.ptr(self.ix.ws), self.ix.ws_bytes, how[1],
                                                   _m.ptr(counts), _m.ptr(d2), _m.ptr(near), _m.stream_ptr()),
                     "mesh_distance_indexed")
        else:
            box = int(L.mslam_mesh_distance_workspace_bytes(self.F))
            ws = torch.zeros(box + 16 * nblk, dtype=torch.uint8, device=dev)
            _m.check(L.mslam_mesh_distance(_m.ptr(pts), n, _m.ptr(self.v), _m.ptr(self.f), self.F, self.V,
                                           2 if how else 0, _m.ptr(ws), ws.numel(), _m.ptr(d2), _m.ptr(near),
                                           _m.stream_ptr()), "mesh_distance")
            counts = ws[box:].view(torch.int32)
        return d2, near, counts

    def cast(self, pose, how):
        """how: 0 plain, 1 the existing culled path, ("index", levels)"""
        n = H * W
        out = (torch.empty(n, dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev),
               torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty(n, dtype=torch.float64, device=dev))
        counts = torch.zeros(4 * int(L.mslam_mesh_raycast_blocks(H, W)), dtype=torch.int32, device=dev)
        if isinstance(how, tuple):
            _m.check(L.mslam_mesh_raycast_indexed(_m.ptr(rays), H, W, _m.ptr(pose), _m.ptr(self.v), _m.ptr(self.f),
                                                  self.F, self.V, 0.05, 10.0, _m.ptr(self.ix.order), _m.ptr(self.ix.ws),
                                                  self.ix.ws_bytes, how[1], _m.ptr(counts), *(_m.ptr(t) for t in out),
                                                  _m.stream_ptr()), "mesh_raycast_indexed")
        else:
            _m.check(L.mslam_mesh_raycast(_m.ptr(rays), H, W, _m.ptr(pose), _m.ptr(self.v), _m.ptr(self.f), self.F,
                                          self.V, 0.05, 10.0, how, _m.ptr(self.ws), self.ws.numel(),
                                          *(_m.ptr(t) for t in out), _m.stream_ptr()), "mesh_raycast")
        return out + (counts,)


def share(counts, waves, F):
    return float(counts[:waves].sum()) / (waves * ((F + 127) // 128))


def same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def measure(name, v, f, reps):
    F = int(f.shape[0])
    t = timed(lambda: MeshIndex(v, f, validate=False), max(3, reps))
    print(f"{name}: V={v.shape[0]} F={F} ({(F + 127) // 128} tiles, {(F + 4095) // 4096} groups); index build "
          f"(keys, sort, boxes) ms {t}", flush=True)
    perm = torch.randperm(F, generator=torch.Generator().manual_seed(5)).to(dev)
    forms = dict(extraction=Form(v, f), shuffled=Form(v, f[perm].contiguous()))
    pts = sample_mesh(v, f, args.samples, seed=1)[0]
    pose = torch.from_numpy(synthetic.camera_pose((args.keyframes // 2) * (1000 // args.keyframes))).float().to(dev)
    waves_p, waves_r = (args.samples + 63) // 64, 4 * int(L.mslam_mesh_raycast_blocks(H, W))
    runs = [("(i)   extraction order, existing", "extraction", 1), ("(ii)  shuffled, existing", "shuffled", 1),
            ("(iii) shuffled, indexed", "shuffled", ("index", 2)), ("(iv)  extraction order, indexed", "extraction",
                                                                    ("index", 2)),
            ("(iii') shuffled, indexed, tiles alone", "shuffled", ("index", 1)),
            ("(iv')  extraction order, indexed, tiles alone", "extraction", ("index", 1))]
    ref = {k: (fm.distance(pts, 0)[:2], fm.cast(pose, 0)[:5]) for k, fm in forms.items()}
    for label, key, how in runs:
        fm = forms[key]
        d = fm.distance(pts, how)
        c = fm.cast(pose, how)
        assert same(d[:2], ref[key][0]) and same(c[:5], ref[key][1]), f"{label}: differs from the plain scan"
        ray_share = share(c[5], waves_r, F) if isinstance(how, tuple) else fm.existing_ray_share(pose, waves_r)
        print(f"  {label}: skipped share, points {share(d[2], waves_p, F):.4f}, rays {ray_share:.4f}", flush=True)
    for rnd in range(2):                                                       # alternated: the spread shows
        for label, key, how in runs:
            fm = forms[key]
            print(f"  {label}: distance_ms {timed(lambda: fm.distance(pts, how), reps)}  cast_ms "
                  f"{timed(lambda: fm.cast(pose, how), reps)}", flush=True)
    print(f"  plain (skip = 0), extraction order: distance_ms {timed(lambda: forms['extraction'].distance(pts, 0), 2)}  "
          f"cast_ms {timed(lambda: forms['extraction'].cast(pose, 0), 2)}", flush=True)


vol = build_room(args.keyframes, args.points, dev)
vol.maintain()
verts, _, faces = vol.extract_mesh()
measure("mesh A", verts, faces, args.reps)
for _ in range(args.split):
    verts, faces = split(verts, faces)
measure(f"mesh B (A split {args.split} times)", verts, faces, max(2, args.reps // 4))
