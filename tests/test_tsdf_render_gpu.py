"""GPU tests (-m gpu) of TSDFVolume.render (csrc/tsdf_render.hip): parity with the numpy statement of the march
(tests/render_numpy.py) on a room fused by the device integrate, empty-space skipping against the brute-force march,
invariance (capacity, growth, repeated calls, voxel shards), agreement with query_batch, edge cases, and the product
path through SlamSystem.  Parity: hit exact; range / normals to 1e-6 absolute (both sides round the same f64 values to
f32, the mesh tests' rule)."""
import os
import sys

import numpy as np
import pytest
import torch

from mast3r_slam import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_numpy as R  # noqa: E402
from mesh_support import POSES, VS, _host, _pose, _rays, _room, _same, _vol  # noqa: E402

pytestmark = pytest.mark.gpu


def _fused(device, capacity=1 << 20):
    vol = _vol(device, capacity)
    for pw, conf, org in _room():
        vol.integrate(pw, conf, org)
    return vol


def _match_numpy(view, voxels, min_weight, pose, rays, **kw):
    rng, nrm, hit = _host(view)
    rr, nr, hr = R.render(*voxels, VS, min_weight, pose, rays, **kw)
    assert rng.dtype == np.float32 and nrm.dtype == np.float32 and hit.dtype == bool
    assert rng.shape == rr.shape and nrm.shape == nr.shape
    assert np.array_equal(hit, hr), (int(hit.sum()), int(hr.sum()))
    dr, dn = float(np.abs(rng - rr).max()), float(np.abs(nrm - nr).max())
    print(f"parity: hits={int(hit.sum())}/{hit.size} max|drange|={dr:.3g} max|dnormal|={dn:.3g}")
    assert dr <= 1e-6 and dn <= 1e-6, (dr, dn)
    return hit


def test_room_view_matches_numpy(device):
    vol = _fused(device)
    voxels = vol.voxels()
    rays = _rays(48, 64)
    for name, pose in POSES.items():
        view = vol.render(pose, rays=rays, far=8.0)
        assert view[0].is_cuda and view[0].shape == (48, 64) and view[1].shape == (48, 64, 3)
        hit = _match_numpy(view, voxels, vol.min_weight, pose, rays, far=8.0)
        if name == "outside":
            assert not hit.any()
        else:
            assert hit.mean() > 0.5, (name, hit.mean())
        _same(view, vol.render(pose, rays=rays, far=8.0, skip=False))
    # another weight threshold, level and step follow the same rules
    kw = dict(far=8.0, level=0.1, step=0.011)
    view = vol.render(POSES["generic"], rays=rays, min_weight=0.5, **kw)
    _match_numpy(view, voxels, 0.5, POSES["generic"], rays, **kw)
    # K + hw builds the same rays
    _same(vol.render(POSES["unfused"], K=synthetic.intrinsics(48, 64), hw=(48, 64), far=8.0),
          vol.render(POSES["unfused"], rays=rays, far=8.0))


def _islands():
    """Three small spheres metres apart: almost every block a ray meets is empty."""
    ks, vs_, ws = [], [], []
    for c, r in [((0.0, 0.0, 2.0), 0.25), ((1.5, -0.8, 4.0), 0.3), ((-2.0, 1.0, 6.5), 0.4)]:
        c = np.array(c)
        k, v, w = R.sample_sdf(lambda p, c=c, r=r: np.linalg.norm(p - c, axis=-1) - r, c - r, c + r, VS, 4 * VS)
        ks.append(k), vs_.append(v), ws.append(w)
    return np.concatenate(ks), np.concatenate(vs_), np.concatenate(ws)


def test_skipping_equals_brute_force(device):
    rays = _rays(384, 512)
    vol = _fused(device)
    for name, pose in POSES.items():
        a, b = vol.render(pose, rays=rays), vol.render(pose, rays=rays, skip=False)
        _same(a, b)
        print(f"room {name}: hits {int(a[2].sum())}/{a[2].numel()}")
    k, v, w = _islands()
    isl = _vol(device, 1 << 18)
    isl.load_voxels(k, v, w)
    for pose in (_pose([0.0, 0.0, 0.0], [0.0, 0.0, 0.0]), _pose([0.3, 0.2, -1.0], [0.1, -0.2, 0.3], 0.8)):
        a, b = isl.render(pose, rays=rays, far=9.0), isl.render(pose, rays=rays, far=9.0, skip=False)
        _same(a, b)
        assert 0.005 < float(a[2].float().mean()) < 0.5


def test_invariant_to_capacity_growth_repeats_and_shards(device):
    from mast3r_slam.tsdf import render_from_voxels

    data = _room()
    big = _vol(device, 1 << 21)
    mid = _vol(device, 1 << 18)
    small = _vol(device, 1 << 14)
    for pw, conf, org in data:
        small.maintain(reserve=len(pw) * 10)
        for v in (big, mid, small):
            v.integrate(pw, conf, org)
    assert 1 << 14 < small.capacity and mid.capacity == 1 << 18 and big.capacity == 1 << 21
    rays, pose = _rays(96, 128), POSES["generic"]
    ref = big.render(pose, rays=rays)
    assert ref[2].float().mean() > 0.5
    before = big.voxels()
    _same(ref, mid.render(pose, rays=rays))
    _same(ref, small.render(pose, rays=rays))            # grown and rehashed
    _same(ref, big.render(pose, rays=rays))              # repeated call
    for x, y in zip(before, big.voxels()):               # a render never writes the table
        assert np.array_equal(x, y)
    for n in (1, 2, 3):
        shards = [_vol(device, 1 << 19, shard_id=r, num_shards=n) for r in range(n)]
        for pw, conf, org in data:
            for s in shards:
                s.integrate(pw, conf, org, return_fused=False)
        parts = [s.voxels() for s in shards]
        keys = np.concatenate([p[0] for p in parts])
        t = np.concatenate([p[1] for p in parts])
        w = np.concatenate([p[2] for p in parts])
        _same(ref, render_from_voxels(keys, t, w, VS, big.min_weight, pose, torch.from_numpy(rays), device=device))


def test_hits_agree_with_query(device):
    """query reads the nearest voxel, the render interpolates the 8 around the point: at a hit the two differ by at most
    the field's change over half a voxel diagonal, g * sqrt(3)/2 * voxel_size with g the steepest difference between
    6-neighbour valid voxels of this volume."""
    vol = _fused(device)
    keys, t, w = vol.voxels()
    ok = w >= vol.min_weight
    keys, t = keys[ok], t[ok]
    pk = R.pack(keys)
    o = np.argsort(pk)
    pk, t, keys = pk[o], t[o], keys[o]
    g = 0.0
    for a in range(3):
        q = R.pack(keys + np.eye(3, dtype=np.int64)[a])
        p = np.minimum(np.searchsorted(pk, q), len(pk) - 1)
        m = pk[p] == q
        g = max(g, float(np.abs(t[p[m]] - t[m]).max()) / VS)
    rays = _rays(96, 128)
    for level in (0.0, 0.1):
        pose = POSES["generic"]
        rng, nrm, hit = _host(vol.render(pose, rays=rays, level=level))
        d = R.ray_dirs(pose, rays).reshape(96, 128, 3)
        pw = pose[:3].astype(np.float64) + (float(pose[7]) * rng.astype(np.float64))[..., None] * d
        val, _, st = vol.query_batch(pw[hit].astype(np.float32))
        val, st = val.cpu().numpy(), st.cpu().numpy()
        assert (st > 0).mean() > 0.9
        err = np.abs(val[st > 0] - level)
        bound = g * np.sqrt(3.0) / 2.0 * VS
        print(f"level {level}: g={g:.4f} bound={bound:.5f} max|query - level|={err.max():.5f} over {len(err)} hits")
        assert err.max() <= bound


def _plane_volume(device, z0=1.0):
    """Slab z in [z0 - 4, z0 + 4] voxels around the plane z = z0 (free space below), 40 x 40 voxels wide."""
    lo, hi = np.array([-0.6, -0.6, z0 - 4 * VS]), np.array([0.6, 0.6, z0 + 4 * VS])
    k, v, w = R.sample_sdf(lambda p: z0 - p[:, 2], lo, hi, VS, 4 * VS)
    vol = _vol(device, 1 << 16)
    vol.load_voxels(k, v, w)
    return vol, (k, v, w)


def test_edge_cases(device):
    eye = _pose([0.0, 0.0, 0.0], [0.0, 0.0, 0.0])
    rays = _rays(24, 32)
    empty = _vol(device, 1 << 10)
    for skip in (True, False):
        rng, nrm, hit = _host(empty.render(eye, rays=rays, skip=skip))
        assert not hit.any() and not rng.any() and not nrm.any()
    vol, voxels = _plane_volume(device)
    # far in front of the surface: all miss
    rng, nrm, hit = _host(vol.render(eye, rays=rays, far=0.8))
    assert not hit.any() and not rng.any() and not nrm.any()
    # the plane from the origin, and a camera inside the band
    for pose in (eye, _pose([0.0, 0.0, 1.0 - 2.5 * VS], [0.05, -0.03, 0.0])):
        view = vol.render(pose, rays=rays, far=3.0)
        hit = _match_numpy(view, voxels, 1.0e-3, pose, rays, far=3.0)
        assert hit.mean() > 0.5
        _same(view, vol.render(pose, rays=rays, far=3.0, skip=False))
    # 1x1 image with a ray along the z axis, from a voxel centre column: range is the distance to the plane
    one = np.array([[[0.0, 0.0, 1.0]]], np.float32)
    p = _pose([0.5 * VS, 0.5 * VS, 0.0], [0.0, 0.0, 0.0])
    view = vol.render(p, rays=one, far=3.0)
    rng, nrm, hit = _host(view)
    assert hit.shape == (1, 1) and hit.all() and abs(float(rng[0, 0]) - 1.0) < 1e-6
    assert np.allclose(nrm[0, 0], [0.0, 0.0, -1.0], atol=1e-6)
    _match_numpy(view, voxels, 1.0e-3, p, one, far=3.0)
    # rays parallel to the other axes, started inside the band on its free side, run along the plane and leave the slab
    # without a crossing: miss, with and without skipping; from the solid side along -z the only crossing is inside-out
    inside = _pose([0.5 * VS, 0.5 * VS, 1.0 - 2.0 * VS], [0.0, 0.0, 0.0])
    for ax in ([1.0, 0.0, 0.0], [0.0, -1.0, 0.0]):
        r1 = np.array([[ax]], np.float32)
        for skip in (True, False):
            assert not _host(vol.render(inside, rays=r1, near=0.0, far=3.0, skip=skip))[2].any()
    behind = _pose([0.5 * VS, 0.5 * VS, 1.0 + 3.0 * VS], [0.0, 0.0, 0.0])
    assert not _host(vol.render(behind, rays=-one, near=0.0, far=3.0))[2].any()
    # image sizes that are not multiples of the 8x8 / 16x16 tiles
    for h, w in ((1, 7), (9, 17), (23, 5), (37, 41)):
        r = _rays(h, w)
        view = vol.render(eye, rays=r, far=3.0)
        assert view[0].shape == (h, w)
        _match_numpy(view, voxels, 1.0e-3, eye, r, far=3.0)
    # a weight threshold above every weight
    assert not _host(vol.render(eye, rays=rays, far=3.0, min_weight=2.0))[2].any()
    with pytest.raises(ValueError):
        vol.render(eye, rays=rays.reshape(-1, 3))
    with pytest.raises(ValueError):
        vol.render(eye, rays=rays, step=0.0)
    with pytest.raises(ValueError):
        vol.render(eye, rays=rays, near=1.0, far=1.0)
    with pytest.raises(ValueError):
        vol.render(eye)
    with pytest.raises(ValueError):
        vol.render(eye[:7], rays=rays)


def test_slam_system_view_and_pngs(device, tmp_path, monkeypatch):
    from PIL import Image

    from mast3r_slam import evaluate
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from test_slam_system_gpu import RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    try:
        system.run(_frames(list(range(0, 60, 3)), device))
        rng, nrm, hit = system.render_view()
        kf = system.keyframes.last_keyframe()
        X = kf.X_canon.detach().float().reshape(rng.shape + (3,)).clone()
        pose = kf.T_WC.data.reshape(8).clone()
        paths = evaluate.save_depth_view(tmp_path, "view.png", rng, nrm, hit, pose=pose)
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    rng, nrm, hit = _host((rng, nrm, hit))
    own = np.linalg.norm(X.cpu().numpy().astype(np.float64), axis=-1)
    assert hit.mean() > 0.5, hit.mean()
    both = hit & (own > 0)
    vs_cam = VS / float(pose[7])                       # one voxel in the keyframe's own units
    med = float(np.median(np.abs(rng[both] - own[both])))
    print(f"slam view: {hit.mean():.4f} of the rays hit, median |range - pointmap range| = {med / vs_cam:.4f} voxel")
    assert med < vs_cam
    depth, normal = Image.open(paths[0]), Image.open(paths[1])
    assert depth.mode in ("I;16", "I;16L", "I;16B") and normal.mode == "RGB"
    d = np.asarray(depth).astype(np.int64)
    assert d.shape == rng.shape
    assert np.array_equal(d, np.where(hit, np.clip(np.rint(rng.astype(np.float64) * 1000.0), 0, 65535), 0).astype(np.int64))
    n = np.asarray(normal)
    assert n.shape == nrm.shape and n.dtype == np.uint8
    q = pose.cpu().numpy().astype(np.float64)[3:7]
    n_cam = synthetic.quat_rotate(q * np.array([-1.0, -1.0, -1.0, 1.0]), nrm.astype(np.float64).reshape(-1, 3)).reshape(nrm.shape)
    want = np.where(hit[..., None], np.rint(0.5 * (n_cam + 1.0) * 255.0), 0)
    assert np.abs(n.astype(np.int64) - want.astype(np.int64)).max() <= 1     # the writer's own f64 rounding at .5 ties
    assert (n_cam[hit][:, 2] < 0).mean() > 0.95                               # seen surfaces face the camera
    off = SlamSystem(RoomModel(device), device, tsdf_global_cfg=None)
    with pytest.raises(RuntimeError, match="global TSDF is disabled"):
        off.render_view()
