#!/usr/bin/env python3
"""Event timing of the mesh smoothing (csrc/mesh_smooth.hip) on the room volume of tools/mesh_time.py: keyframes along
the synthetic trajectory, 40 000 points each, the config's voxel size and truncation, maintain() before every fusion.
The mesh is timed as extracted and split 1 -> 4 (welded: one midpoint per edge) `--splits` times, for a size in the
millions of faces.  Times, with HIP events after warm-up, medians of repeated calls: (a) the table build (edge keys,
sort, unique_consecutive with its host read, searchsorted); (b) one step and ten iterations (twenty launches) in both
layouts of the f64 state, three doubles per vertex and four; (c) the normals (pair keys, sort, searchsorted, kernel);
(d) smooth_mesh as a whole, host reads included; (e) for context, not as a pass mark, the same ten iterations written
with torch.index_add_ in f64, what one would write without the kernel, after showing that it agrees with the kernel to
the printed bound.  Then the room figures: compare_meshes of the mesh against synthetic.room_mesh() before and after 5
and 10 iterations, alone and followed by simplify_mesh at 2 voxels.  Not part of bench.py.
    python tools/mesh_smooth_time.py 60 [--reps 20] [--splits 2]"""
import argparse

import torch

from _room import build_room, timed   # first: it puts the package on sys.path
import mslam_hip as _m
from mast3r_slam import synthetic
from mast3r_slam.config import config
from mast3r_slam.tsdf import compare_meshes, simplify_mesh, smooth_mesh
from mast3r_slam.tsdf import mesh_smooth as MS

ap = argparse.ArgumentParser()
ap.add_argument("keyframes", type=int, nargs="+")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--points", type=int, default=40000)
ap.add_argument("--splits", type=int, default=2, help="how often the mesh is split 1 -> 4 for the larger sizes")
ap.add_argument("--samples", type=int, default=200000, help="compare_meshes samples per mesh")
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = config["tsdf_global"]
vs, trunc = float(cfg["voxel_size"]), float(cfg["trunc_dist"])
print(f"voxel_size={vs} trunc={trunc} points/kf={args.points} device={torch.cuda.get_device_name(dev)}", flush=True)
L = _m.lib()
LAM, MU, FIXED = 0.5, -0.53, MS._MODES["fixed"]


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


def steps(x0, spare, table, stride, launches):
    """`launches` steps from x0, which is only read, through the two spare states -> the last state written."""
    row_start, nbr, mult, E = table
    V = x0.shape[0]
    src, k = x0, 0
    for i in range(launches):
        _m.check(L.mslam_mesh_smooth_step(_m.ptr(src), _m.ptr(spare[k]), stride, _m.ptr(row_start), _m.ptr(nbr),
                                          _m.ptr(mult), V, E, LAM if i % 2 == 0 else MU, FIXED, 0, _m.stream_ptr()),
                 "step")
        src, k = spare[k], 1 - k
    return src


def difference_bound(iterations, max_valence, radius):
    """Two orders of the neighbour sums, both f64: each step adds at most 2 (n + 3) 2^-53 R max(1, |f|) and multiplies
    what is there by at most |1 - f| + |f| (tests/smooth_numpy.py derives it)."""
    total = 0.0
    for _ in range(iterations):
        for f in (LAM, MU):
            total = total * (abs(1.0 - f) + abs(f)) + 2.0 * (max_valence + 3) * 2.0 ** -53 * radius * max(1.0, abs(f))
    return total


def torch_iterations(x0, rows, cols, deg, fixed, iterations):
    """The same filter with index_add_: the sum's order is whatever the scatter does, so the last bits differ."""
    x = x0
    for _ in range(iterations):
        for f in (LAM, MU):
            s = torch.zeros_like(x).index_add_(0, rows, x[cols])
            x = torch.where(fixed[:, None], x, x + f * (s / deg[:, None] - x))
    return x


def measure(verts, faces, label):
    V, F = int(verts.shape[0]), int(faces.shape[0])
    table = MS._neighbour_table(faces, V, F)
    row_start, nbr, mult, E = table
    n_dir = int(row_start[V])
    deg = (row_start[1:] - row_start[:-1])
    print(f"{label}: V={V} F={F} directed_edges={n_dir} max_valence={int(deg.max())}", flush=True)
    print(f"  (a) table_ms {timed(lambda: MS._neighbour_table(faces, V, F), args.reps)}", flush=True)
    results = {}
    for stride in (3, 4):
        x0, *spare = (torch.zeros((V, stride), dtype=torch.float64, device=dev) for _ in range(3))
        x0[:, :3] = verts
        print(f"  (b) stride={stride} one_step_ms {timed(lambda: steps(x0, spare, table, stride, 1), args.reps)}",
              flush=True)
        print(f"  (b) stride={stride} ten_iterations_ms {timed(lambda: steps(x0, spare, table, stride, 20), args.reps)}",
              flush=True)
        results[stride] = steps(x0, spare, table, stride, 20)[:, :3].clone()
    assert torch.equal(results[3], results[4]), "the two layouts differ"
    normals = torch.zeros_like(verts)
    print(f"  (c) normals_ms {timed(lambda: MS._normals(verts, faces, V, F, normals, 'time'), args.reps)}", flush=True)
    mesh = (verts, normals, faces)
    out = smooth_mesh(mesh, 10)
    assert torch.equal(out[0], results[MS._STRIDE].float()), "the staged launches differ from smooth_mesh"
    print(f"  (d) smooth_mesh_10_ms {timed(lambda: smooth_mesh(mesh, 10), args.reps)}", flush=True)
    print(f"  (d) smooth_mesh_10_unvalidated_keep_normals_ms "
          f"{timed(lambda: smooth_mesh(mesh, 10, normals='keep', _validate=False), args.reps)}", flush=True)
    rows = torch.repeat_interleave(torch.arange(V, device=dev), deg)
    cols = nbr[:n_dir].long()
    rim = torch.zeros(V, dtype=torch.float64, device=dev).index_add_(0, rows, (mult[:n_dir] == 1).double())
    fixed = (rim > 0) | (deg == 0)
    x0 = verts.double()
    ref = torch_iterations(x0, rows, cols, deg.double().clamp(min=1), fixed, 10)
    err = float((ref - results[4]).abs().max())
    scale = float(x0.abs().max())
    bound = difference_bound(10, int(deg.max()), 2.0 * scale)
    print(f"  (e) index_add_ form against the kernel: max |difference| {err:.3e} on coordinates up to {scale:.2f}, "
          f"bound {bound:.1e} (both f64; only the order of the sums differs)", flush=True)
    assert err <= bound
    print(f"  (e) index_add_ten_iterations_ms "
          f"{timed(lambda: torch_iterations(x0, rows, cols, deg.double().clamp(min=1), fixed, 10), args.reps)}",
          flush=True)


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
    for k in range(args.splits):
        v, f = split(v, f)
        measure(v, f, f"room split {k + 1}x")
    gt = tuple(torch.from_numpy(a).to(dev) for a in synthetic.room_mesh())
    print(f"room figures against synthetic.room_mesh() ({args.samples} samples, threshold "
          f"{cfg['mesh_eval_threshold']}):", flush=True)
    for it in (0, 5, 10):
        sm = smooth_mesh(mesh, it)
        quality(sm, gt, f"iterations={it}")
        quality(simplify_mesh(sm, 2 * vs), gt, f"iterations={it} + simplify 2 voxels")
