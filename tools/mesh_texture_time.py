#!/usr/bin/env python3
"""Event timing of the mesh textures (csrc/mesh_texture.hip) on the room volume of tools/mesh_time.py: keyframes along
the synthetic trajectory, 40 000 points each, the mesh extracted and decimated to a fifth of its faces.  (1) The bake at
texels=8 from the keyframes' cameras and their 192x256 images of the room's texture: the whole call, plain and with a
mesh index, and its per-view steps over all views - the rays kernel, the rays kernel with the cast of its rays, the
accumulate kernel.  (2) One 384x512 pinhole view from the middle keyframe: render_mesh beside render_mesh_color from
vertex colours and from the texture.  HIP events after warm-up, medians of repeated calls; two bakes, and the indexed
bake, are compared byte for byte before anything is timed.  Not part of bench.py.
    python tools/mesh_texture_time.py 60 [--reps 20] [--texels 8]"""
import argparse

import numpy as np
import torch

from _room import build_room, timed   # first: it puts the package on sys.path
from mast3r_slam import synthetic
from mast3r_slam.tsdf import bake_texture, build_mesh_index, decimate_mesh, render_mesh, render_mesh_color
from mast3r_slam.tsdf.mesh_raycast import _Caster
from mast3r_slam.tsdf.mesh_texture import _Baker

ap = argparse.ArgumentParser()
ap.add_argument("keyframes", type=int, nargs="+")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--points", type=int, default=40000)
ap.add_argument("--texels", type=int, default=8)
args = ap.parse_args()
dev = torch.device("cuda:0")
H, W, h, w = 384, 512, 192, 256
print(f"points/kf={args.points} texels={args.texels} images={h}x{w} view={H}x{W} "
      f"device={torch.cuda.get_device_name(dev)}", flush=True)
for n_kf in args.keyframes:
    vol = build_room(n_kf, args.points, dev)
    vol.maintain()
    full = vol.extract_mesh()
    small = decimate_mesh(full, ratio=0.2)
    mesh = (small[0].contiguous(), small[2].contiguous())
    ks = [i * (1000 // n_kf) for i in range(n_kf)]
    cams = np.stack([synthetic.camera_pose(k) for k in ks]).astype(np.float32)
    images = torch.from_numpy(np.stack([0.5 * (synthetic.render_rgb(synthetic.camera_pose(k), h, w).transpose(1, 2, 0)
                                               + 1.0) for k in ks]).astype(np.float32)).to(dev)
    K = synthetic.intrinsics(h, w)
    tex = bake_texture(mesh, images, cams, K, texels=args.texels)
    again = bake_texture(mesh, images, cams, K, texels=args.texels)
    assert torch.equal(tex.atlas.view(torch.int32), again.atlas.view(torch.int32)) and torch.equal(tex.views, again.views)
    owned = tex.owner >= 0
    print(f"keyframes={n_kf} F_full={full[2].shape[0]} V={mesh[0].shape[0]} F={mesh[1].shape[0]} atlas="
          f"{tuple(tex.atlas.shape[:2])} owned={int(owned.sum())} seen_share="
          f"{float(((tex.views > 0) & owned).sum()) / float(owned.sum()):.4f}", flush=True)
    reps = max(1, args.reps // 4)
    print(f"  (1) bake_ms {timed(lambda: bake_texture(mesh, images, cams, K, texels=args.texels), reps)}", flush=True)
    index = build_mesh_index(mesh)
    assert torch.equal(bake_texture(mesh, images, cams, K, texels=args.texels, index=index).atlas, tex.atlas)
    print(f"  (1) bake_indexed_ms {timed(lambda: bake_texture(mesh, images, cams, K, texels=args.texels, index=index), reps)}",
          flush=True)
    bk = _Baker(_Caster(mesh[0], mesh[1], True, True, "mesh_texture_time"), args.texels)
    K4 = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    pd = torch.from_numpy(cams).to(dev)
    t64 = [None]

    def all_rays():
        for k in range(n_kf):
            bk.rays(pd[k], K4, (h, w), 0.05, 10.0, 0.1)

    def all_casts():                                   # every view's own rays: the rays kernel again, then the cast
        for k in range(n_kf):
            bk.rays(pd[k], K4, (h, w), 0.05, 10.0, 0.1)
            t64[0] = bk.cast(pd[k])

    def all_accumulates():
        for k in range(n_kf):
            bk.accumulate(t64[0], images[n_kf - 1], pd[n_kf - 1], 0.01)

    for name, fn in (("rays", all_rays), ("rays_and_casts", all_casts), ("accumulate", all_accumulates)):
        print(f"    {name}_{n_kf}_views_ms {timed(fn, reps)}", flush=True)
    print(f"    resolve_ms {timed(lambda: bk.resolve(None, 0.5), args.reps)}", flush=True)
    pose = cams[n_kf // 2]
    KV = synthetic.intrinsics(H, W)
    colors = torch.rand((mesh[0].shape[0], 3), device=dev)
    view = dict(K=KV, hw=(H, W))
    for label, fn in (("render_mesh", lambda: render_mesh(mesh, pose, **view)),
                      ("render_mesh_color_colors", lambda: render_mesh_color(mesh, pose, colors=colors, **view)),
                      ("render_mesh_color_texture", lambda: render_mesh_color(mesh, pose, texture=tex, **view))) * 2:
        print(f"  (2) {label}_ms {timed(fn, args.reps)}", flush=True)
