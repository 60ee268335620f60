"""GPU tests (-m gpu) of the colour of the global TSDF (csrc/tsdf_color.hip, DESIGN.md "Colour") on the three-keyframe
room of tests/test_tsdf_render_gpu.py, coloured with the room texture (synthetic.render_rgb's formula, in [0, 1]) at the
fused world points: fusion against the numpy statement (tests/color_numpy.py), order independence bit for bit, the TSDF
left untouched, sample_color / coloured mesh / coloured view against numpy, and the colours themselves against the
analytic texture."""
import os
import sys

import numpy as np
import pytest
import torch

from mast3r_slam import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import color_numpy as C  # noqa: E402
import render_numpy as R  # noqa: E402
import tsdf_global_refs as G  # noqa: E402
from mesh_support import POSES, VS, _rays, _room, _vol, color_checks  # noqa: E402

pytestmark = pytest.mark.gpu

TRUNC = 0.12


def _colored_room():
    return [(pw, conf, org, C.texture(pw).astype(np.float32)) for pw, conf, org in _room()]


def _fused(device, capacity=1 << 20, data=None, **kw):
    vol = _vol(device, capacity, color=True, **kw)
    for pw, conf, org, rgb in (_colored_room() if data is None else data):
        vol.integrate(pw, conf, org, colors=rgb, return_fused=kw.get("num_shards", 1) == 1)
    return vol


def _host(a):
    return a.cpu().numpy()


def test_fusion_matches_numpy(device):
    """The bounds are the issue's: every in-band weight is >= 0.1 / e * 2^20 = 38 575 units and device exp may move a
    rint(w * 2^20) by one unit, so |d sum_w| <= 1e-4 sum_w and |d c| <= 0.02 / 255."""
    data = _colored_room()
    vol = _fused(device, data=data)
    keys, sums = vol.voxel_color_sums()
    vk = vol.voxels()[0]
    assert sums.dtype == np.uint64 and sums.shape == (len(vk), 4)
    assert np.array_equal(keys, vk)
    assert (sums[:, 0] > 0).all()                     # every voxel the integrate made has colour
    ref = {}
    for pw, conf, org, rgb in data:
        C.fuse(ref, pw, conf, rgb, org, VS, TRUNC)
    assert set(ref) == set(C.pack(keys).tolist())     # ... and nothing else has
    want = C.sums_for(ref, keys)
    sw, rw = sums[:, 0].astype(np.float64), want[:, 0].astype(np.float64)
    dw = float((np.abs(sw - rw) / rw).max())
    col = sums[:, 1:].astype(np.float64) / (255.0 * sw[:, None])
    colr = want[:, 1:].astype(np.float64) / (255.0 * rw[:, None])
    dc = float(np.abs(col - colr).max())
    exact = float((sums == want).all(1).mean())
    print(f"colour fusion vs numpy: {len(keys)} voxels, max rel |d sum_w| = {dw:.3g}, max |d c| = {dc * 255:.3g} / 255, "
          f"{100 * exact:.2f} % of the voxels equal in all four sums")
    assert dw <= 1e-4 and dc <= 0.02 / 255.0, (dw, dc)
    k2, rgb, w2 = vol.voxel_colors()
    assert np.array_equal(k2, keys) and np.array_equal(w2, sums[:, 0]) and np.array_equal(rgb, col)


def test_order_independent_bit_for_bit(device):
    data = _colored_room()
    ref_keys, ref_sums = _fused(device, 1 << 21, data).voxel_color_sums()

    def same(vol_or_pair, what):
        k, s = vol_or_pair.voxel_color_sums() if hasattr(vol_or_pair, "voxel_color_sums") else vol_or_pair
        assert np.array_equal(k, ref_keys), what
        assert np.array_equal(s, ref_sums), (what, int((s != ref_sums).any(1).sum()))

    rng = np.random.default_rng(5)
    perm = []
    for pw, conf, org, rgb in data:
        o = rng.permutation(len(pw))
        perm.append((pw[o], conf[o], org, rgb[o]))
    same(_fused(device, 1 << 21, perm), "permuted points")
    split = []
    for pw, conf, org, rgb in data:
        h = len(pw) // 3
        split += [(pw[:h], conf[:h], org, rgb[:h]), (pw[h:], conf[h:], org, rgb[h:])]
    same(_fused(device, 1 << 21, split), "two calls")
    same(_fused(device, 1 << 18, data), "capacity 2^18")
    small = _vol(device, 1 << 14, color=True)
    for pw, conf, org, rgb in data:
        small.maintain(reserve=len(pw) * 10)
        small.integrate(pw, conf, org, colors=rgb)
    assert small.capacity > 1 << 14
    same(small, "grown from 2^14")
    for n in (1, 2, 3):
        shards = [_fused(device, 1 << 19, data, shard_id=r, num_shards=n) for r in range(n)]
        parts = [s.voxel_color_sums() for s in shards]
        if n > 1:
            assert all(0 < len(p[0]) < len(ref_keys) for p in parts)
        keys = np.concatenate([p[0] for p in parts])
        sums = np.concatenate([p[1] for p in parts])
        o = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
        same((keys[o], sums[o]), f"{n} shards")


BAND_CASES = sorted(name for name in G.CASES if name.startswith("band_"))


@pytest.mark.parametrize("name", BAND_CASES)
def test_color_walk_visits_the_emit_walks_voxels(device, name):
    """The colour fuse finds its voxels by the keys the emit pass made them with (csrc/tsdf_walk.h): on the band-edge
    sweeps (coarse step, the clamped 1e-4 step, a band thinner than a voxel, negative and corner origins) every voxel of
    the volume must have colour, unsharded and as two shards, and the shards' union must be the unsharded volume.
    Set equality is the right assertion because no in-band weight rounds to zero units: the smallest confidence is
    above 5e-5 and exp(-|sdf| / trunc) >= 1 / e in band, so a sample adds at least 5e-5 / e * 2^20 = 19 units; checked
    below from ray_samples before the GPU is asked."""
    from mast3r_slam.tsdf import TSDFVolume

    p, c, o, vs, tr, mw, ss = G.CASES[name]()
    units = []
    for point, conf in zip(p, c):
        rs = G.ray_samples(point, o, vs, tr, ss)
        if rs is not None and len(rs[2]):
            units.append(float((conf * np.exp(rs[2].astype(np.float64))).min()) * 2.0 ** 20)
    print(f"{name}: {len(p)} rays, {len(units)} with in-band samples, smallest weight {min(units):.0f} units")
    assert len(units) > len(p) // 2 and min(units) >= 19.0
    rgb = np.random.default_rng(len(p)).uniform(0.0, 1.0, (len(p), 3)).astype(np.float32)

    def fused(**kw):
        vol = TSDFVolume(vs, tr, mw, 1.0e-3, capacity=1 << 16, device=device, color=True, **kw)
        vol.integrate(p, c, o, step_scale=ss, colors=rgb, return_fused=False)
        assert vol.maintain()[0] > 0            # raises if a sample was dropped
        keys, sums = vol.voxel_color_sums()
        assert np.array_equal(keys, vol.voxels()[0])
        dark = int((sums[:, 0] == 0).sum())
        assert dark == 0, f"{name} {kw}: {dark} of {len(keys)} voxels have no colour"
        return keys, sums

    keys, sums = fused()
    parts = [fused(shard_id=r, num_shards=2) for r in range(2)]
    assert all(0 < len(k) < len(keys) for k, _ in parts)
    uk, us = np.concatenate([k for k, _ in parts]), np.concatenate([s for _, s in parts])
    order = np.lexsort((uk[:, 2], uk[:, 1], uk[:, 0]))
    assert np.array_equal(uk[order], keys) and np.array_equal(us[order], sums)


def test_tsdf_untouched(device):
    data = _colored_room()
    with_c = _fused(device, data=data)
    plain = _vol(device, 1 << 20)
    for pw, conf, org, _ in data:
        plain.integrate(pw, conf, org)
    assert plain._color is None and not plain.color
    for x, y in zip(with_c.voxels(), plain.voxels()):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    # colour=True without colours: the same volume again, and no colour anywhere
    quiet = _vol(device, 1 << 20, color=True)
    for pw, conf, org, _ in data:
        quiet.integrate(pw, conf, org)
    for x, y in zip(quiet.voxels(), plain.voxels()):
        assert np.array_equal(x, y)
    assert not quiet.voxel_color_sums()[1].any()


def _sample_points(keys, rng):
    vox = keys[rng.integers(0, len(keys), 3000)].astype(np.float64)
    near = (vox + 0.5 + rng.uniform(-2.5, 2.5, vox.shape)) * VS           # around the band: all, some or no corners
    room = rng.uniform(-1.0, 1.0, (1500, 3)) * (np.asarray(synthetic.ROOM_HALF) + 0.3)
    k = keys[rng.integers(0, len(keys), 600)].astype(np.float64)
    plane = (k + 0.5) * VS                                                 # on lattice planes: fractions 0 (or next to it)
    plane[200:400, 1] += rng.uniform(0, VS, 200)
    plane[400:, 2] += rng.uniform(0, VS, 200)
    far = np.array([[1.0e7, 0.0, 0.0], [0.0, -3.0e6, 1.0], [np.inf, 0.0, 0.0], [np.nan, 1.0, 1.0]])
    return np.concatenate((near, room, plane, far)).astype(np.float32)


def test_sample_color_matches_numpy(device):
    vol = _fused(device)
    keys, sums = vol.voxel_color_sums()
    pts = _sample_points(keys, np.random.default_rng(11))
    assert len(pts) % 64 != 0
    dflt = (0.25, 0.5, 0.75)
    rgb, cnt = vol.sample_color(pts, default_color=dflt)
    assert rgb.is_cuda and rgb.dtype == torch.float32 and rgb.shape == (len(pts), 3)
    assert cnt.dtype == torch.uint8 and cnt.shape == (len(pts),)
    rgb, cnt = _host(rgb), _host(cnt)
    want, wcnt = C.sample(keys, sums, VS, pts, dflt)
    assert np.array_equal(cnt.astype(np.int64), wcnt)
    hist = np.bincount(wcnt, minlength=9)
    print("sample_color: coloured corners 0..8:", hist.tolist())
    assert hist[0] > 100 and hist[8] > 100 and hist[1:8].sum() > 100
    d = float(np.abs(rgb.astype(np.float64) - want).max())
    print(f"sample_color vs numpy: max |d| = {d:.3g} over {len(pts)} points")
    assert d <= 1e-6
    assert np.array_equal(rgb[wcnt == 0], np.broadcast_to(np.asarray(dflt, np.float32), (int((wcnt == 0).sum()), 3)))
    # an image-shaped list goes through the 8x8 tiles and gives the same values; sizes off the tile grid
    for h, w in ((37, 41), (1, 7), (16, 16)):
        img = pts[: h * w].reshape(h, w, 3)
        a, b = vol.sample_color(img, default_color=dflt)
        assert a.shape == (h, w, 3) and b.shape == (h, w)
        assert np.array_equal(_host(a).reshape(-1, 3), rgb[: h * w]) and np.array_equal(_host(b).reshape(-1), cnt[: h * w])
    for n in (0, 1, 63, 65):
        a, b = vol.sample_color(pts[:n], default_color=dflt)
        assert a.shape == (n, 3) and np.array_equal(_host(a), rgb[:n]) and np.array_equal(_host(b), cnt[:n])


def test_mesh_and_view_colors(device):
    from mast3r_slam.tsdf import mesh_from_voxels, render_from_voxels

    vol = _fused(device)
    keys, sums = vol.voxel_color_sums()
    mesh = vol.extract_mesh()
    cmesh = vol.extract_mesh(colors=True)
    assert len(mesh) == 3 and len(cmesh) == 4
    for x, y in zip(mesh, cmesh[:3]):
        assert x.dtype == y.dtype and torch.equal(x, y)
    v, vc = _host(cmesh[0]), _host(cmesh[3])
    assert vc.dtype == np.float32 and vc.shape == v.shape and len(v) > 0
    want, cnt = C.sample(keys, sums, VS, v)
    d = float(np.abs(vc.astype(np.float64) - want).max())
    print(f"mesh colours vs numpy: max |d| = {d:.3g} over {len(v)} vertices, {100 * (cnt == 8).mean():.1f} % with 8 corners")
    assert d <= 1e-6 and vc.min() >= 0.0 and vc.max() <= 1.0
    rays = _rays(48, 64)
    for name, pose in POSES.items():
        view = vol.render(pose, rays=rays, far=8.0)
        cview = vol.render(pose, rays=rays, far=8.0, colors=True)
        assert len(view) == 3 and len(cview) == 4
        for x, y in zip(view, cview[:3]):
            assert x.dtype == y.dtype and torch.equal(x, y)
        rng, hit, rgb = _host(cview[0]), _host(cview[2]), _host(cview[3])
        assert rgb.dtype == np.float32 and rgb.shape == (48, 64, 3)
        assert not rgb[~hit].any()
        want, _ = C.sample(keys, sums, VS, C.hit_points(pose, rays, rng).reshape(-1, 3))
        d = float(np.abs(rgb.astype(np.float64) - want.reshape(48, 64, 3))[hit].max()) if hit.any() else 0.0
        print(f"view colours vs numpy ({name}): max |d| = {d:.3g} over {int(hit.sum())} hits")
        assert d <= 1e-6
    # the union path carries the sums: same mesh colours and view colours from the voxel arrays
    k, t, w = vol.voxels()
    um = mesh_from_voxels(k, t, w, VS, vol.min_weight, device=device, colors=sums)
    for x, y in zip(cmesh, um):
        assert torch.equal(x, y)
    uv = render_from_voxels(k, t, w, VS, vol.min_weight, POSES["generic"], torch.from_numpy(rays), far=8.0, device=device,
                            colors=sums)
    for x, y in zip(vol.render(POSES["generic"], rays=rays, far=8.0, colors=True), uv):
        assert torch.equal(x, y)
    # voxels loaded without colours: the default colour everywhere
    grey = _vol(device, 1 << 20, color=True)
    grey.load_voxels(k, t, w)
    gm = grey.extract_mesh(colors=True, default_color=(0.1, 0.2, 0.3))
    assert torch.equal(gm[0], mesh[0])
    assert np.array_equal(_host(gm[3]), np.broadcast_to(np.array([0.1, 0.2, 0.3], np.float32), tuple(gm[3].shape)))
    gv = grey.render(POSES["generic"], rays=rays, far=8.0, colors=True)
    ghit = _host(gv[2])
    assert ghit.any() and np.array_equal(_host(gv[3])[ghit], np.full((int(ghit.sum()), 3), 0.5, np.float32))
    assert not _host(gv[3])[~ghit].any()


def test_colors_are_the_right_ones(device):
    """The fused points carry the texture at their exact world points, so the error of a hit pixel's colour against the
    texture at its hit point is bounded by the texture's change over the distance between the points a voxel averages
    and the sample: L * (trunc + 1.5 sqrt(3) vs), plus half an 8-bit level."""
    vol = _fused(device)
    bound = C.lipschitz() * (TRUNC + 1.5 * np.sqrt(3.0) * VS) + 0.5 / 255.0
    h, w = 96, 128
    rays = _rays(h, w)
    for k in (12, 15, 20, 57):
        T = synthetic.camera_pose(k)
        pose = T.astype(np.float32)
        rng, _, hit, rgb = (_host(x) for x in vol.render(pose, rays=rays, colors=True))
        assert hit.any(), k
        p64 = pose.astype(np.float64)
        pts = p64[:3] + (p64[7] * rng.astype(np.float64))[..., None] * R.ray_dirs(pose, rays).reshape(h, w, 3)
        full = 0.5 * (synthetic.render_rgb(T, h, w).astype(np.float64).transpose(1, 2, 0) + 1.0)
        mx, mean = color_checks(rgb.astype(np.float64), hit, C.texture(pts), full, f"camera_pose({k})")
        print(f"camera_pose({k}): bound {bound:.4f}")
        assert mx <= bound, (k, mx, bound)


def test_errors(device):
    from mast3r_slam.tsdf import TSDFGlobalManager, TSDFVolume

    pw, conf, org, rgb = _colored_room()[0]
    plain = _vol(device, 1 << 16)
    with pytest.raises(ValueError):
        plain.integrate(pw[:100], conf[:100], org, colors=rgb[:100])
    with pytest.raises(ValueError):
        plain.extract_mesh(colors=True)
    with pytest.raises(ValueError):
        plain.render(POSES["generic"], rays=_rays(8, 8), colors=True)
    with pytest.raises(ValueError):
        plain.sample_color(pw[:10])
    with pytest.raises(ValueError):
        plain.voxel_colors()
    with pytest.raises(ValueError):
        plain.load_voxels(np.zeros((1, 3), np.int64), np.zeros(1), np.ones(1), colors=np.zeros((1, 4), np.uint64))
    vol = _vol(device, 1 << 16, color=True)
    with pytest.raises(ValueError):
        vol.integrate(pw[:100], conf[:100], org, colors=rgb[:99])
    with pytest.raises(ValueError):
        vol.integrate(pw[:100], conf[:100], org, colors=rgb[:100, :2])
    with pytest.raises(ValueError):
        vol.sample_color(pw[:10, :2])
    with pytest.raises(ValueError):
        vol.load_voxels(np.zeros((2, 3), np.int64), np.zeros(2), np.ones(2), colors=np.zeros((1, 4), np.uint64))

    class Channel:                      # what the constructors read of mast3r_slam.shard's channel
        rank, world, group, is_driver = 0, 2, None, True

    with pytest.raises(ValueError):
        TSDFVolume(VS, TRUNC, capacity=1 << 10, device=device, shard_id=0, num_shards=2, channel=Channel(), color=True)
    from mast3r_slam.config import config
    from mast3r_slam.frame import KeyframeStore

    with pytest.raises(ValueError):
        TSDFGlobalManager(KeyframeStore(), dict(config["tsdf_global"], enabled=True, color=True, hash_capacity=1 << 10),
                          False, device, channel=Channel())
