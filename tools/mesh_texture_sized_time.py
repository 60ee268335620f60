#!/usr/bin/env python3
"""Event timing of the sized atlas of the mesh textures (csrc/mesh_texture.hip, DESIGN.md "Mesh textures: sized atlas")
on the mesh of tools/mesh_texture_time.py: the room volume, keyframes along the synthetic trajectory, 40 000 points each,
the mesh extracted and decimated to a fifth of its faces.  It bakes once with the uniform atlas at texels=8 and once with
the density, found by bisection, whose sized atlas owns about as many texels (floor class 4), both over a mesh index, and
prints the class histogram, the atlas size and fill, the times of the class, rank and layout launches, of the host read
and of the whole bake beside the uniform bake's, and the PSNR / SSIM of the training views for both.  HIP events after
warm-up, medians of repeated calls; two sized bakes are compared byte for byte before anything is timed.  Not part of
bench.py.
    python tools/mesh_texture_sized_time.py 60 [--reps 20] [--texels 8]"""
import argparse

import numpy as np
import torch

from _room import build_room, timed   # first: it puts the package on sys.path
from mast3r_slam import synthetic
from mast3r_slam.tsdf import (atlas_classes, bake_texture, build_mesh_index, decimate_mesh, image_metrics,
                              render_mesh_color)
from mast3r_slam.tsdf.mesh_raycast import _Caster
from mast3r_slam.tsdf.mesh_texture import _SizedBaker

ap = argparse.ArgumentParser()
ap.add_argument("keyframes", type=int, nargs="+")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--points", type=int, default=40000)
ap.add_argument("--texels", type=int, default=8)
args = ap.parse_args()
dev = torch.device("cuda:0")
h, w = 192, 256
print(f"points/kf={args.points} uniform texels={args.texels} images={h}x{w} device={torch.cuda.get_device_name(dev)}",
      flush=True)
for n_kf in args.keyframes:
    vol = build_room(n_kf, args.points, dev)
    vol.maintain()
    small = decimate_mesh(vol.extract_mesh(), ratio=0.2)
    mesh = (small[0].contiguous(), small[2].contiguous())
    ks = [i * (1000 // n_kf) for i in range(n_kf)]
    cams = np.stack([synthetic.camera_pose(k) for k in ks]).astype(np.float32)
    images = torch.from_numpy(np.stack([0.5 * (synthetic.render_rgb(synthetic.camera_pose(k), h, w).transpose(1, 2, 0)
                                               + 1.0) for k in ks]).astype(np.float32)).to(dev)
    K = synthetic.intrinsics(h, w)
    index = build_mesh_index(mesh)
    uni = bake_texture(mesh, images, cams, K, texels=args.texels, index=index)
    budget = int((uni.owner >= 0).sum())
    caster = _Caster(mesh[0], mesh[1], True, True, "mesh_texture_sized_time")

    def owned_at(density):
        bk = _SizedBaker(caster, density, 4, 256)
        bk.classes(), bk.ranks()
        counts = bk.counts14.cpu().tolist()[:-1]
        return sum(c * R * (R + 1) // 2 for c, R in zip(counts, atlas_classes))

    lo, hi = 1.0, 4096.0
    for _ in range(40):                                 # the largest density whose atlas owns no more than the uniform one
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if owned_at(mid) <= budget else (lo, mid)
    density = lo
    kw = dict(texels=4, density=density, index=index)
    tex = bake_texture(mesh, images, cams, K, **kw)
    again = bake_texture(mesh, images, cams, K, **kw)
    assert torch.equal(tex.atlas.view(torch.int32), again.atlas.view(torch.int32)) and torch.equal(tex.views, again.views)
    assert torch.equal(tex.owner, again.owner) and torch.equal(tex.face_cell, again.face_cell)
    for name, t in (("uniform", uni), ("sized", tex)):
        own = t.owner >= 0
        print(f"keyframes={n_kf} V={mesh[0].shape[0]} F={mesh[1].shape[0]} {name}: atlas={tuple(t.atlas.shape[:2])} owned="
              f"{int(own.sum())} fill={float(own.sum()) / max(own.numel(), 1):.4f} seen_share="
              f"{float(((t.views > 0) & own).sum()) / float(own.sum()):.4f}", flush=True)
    print(f"  density={density:.3f} texels per metre, classes "
          f"{ {R: c for R, c in zip(atlas_classes, tex.counts) if c} }, clamped={tex.clamped}", flush=True)
    reps = max(1, args.reps // 4)
    print(f"  bake_uniform_indexed_ms {timed(lambda: bake_texture(mesh, images, cams, K, texels=args.texels, index=index), reps)}",
          flush=True)
    print(f"  bake_sized_indexed_ms {timed(lambda: bake_texture(mesh, images, cams, K, **kw), reps)}", flush=True)
    bk = _SizedBaker(caster, density, 4, 256)
    bk.classes(), bk.ranks(), bk.read_counts(), bk.layout()
    for name, fn in (("classes", bk.classes), ("rank_3_launches", bk.ranks), ("host_read_and_buffers", bk.read_counts),
                     ("layout_2_launches", bk.layout)):
        print(f"    {name}_ms {timed(fn, args.reps)}", flush=True)
    for name, t in (("uniform", uni), ("sized", tex)):
        views = [render_mesh_color(mesh, cams[k], texture=t, K=K, hw=(h, w), index=index) for k in range(n_kf)]
        m = image_metrics(torch.stack([v[3] for v in views]), images, mask=torch.stack([v[2] for v in views]))
        print(f"  training views, {name}: PSNR {float(m['psnr'].mean()):.3f} dB SSIM {float(m['ssim'].mean()):.4f}",
              flush=True)
