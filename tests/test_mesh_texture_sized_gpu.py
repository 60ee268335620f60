"""GPU tests (-m gpu) of the sized atlas of the mesh textures (csrc/mesh_texture.hip, DESIGN.md "Mesh textures: sized
atlas") and of bake_texture(density=...) / render_mesh_color / MeshTexture / SlamSystem.bake_texture: byte for byte
against the numpy statement (tests/texture_sized_numpy.py) - classes, ranks, order, counts, owner, face_cell, atlas,
views and, through the raw entries behind guarded buffers, dir, r, cos, uv, t64 and sums after every view - on strips
whose faces alternate between the classes 4, 6 and 8 across a wave and a block, a class-64 face among class-4 faces,
culled, plain and indexed, the cross-check against the uniform atlas on a one-class mesh, both shading modes, refused
arguments, the mixed checker room whose sized atlas must beat the uniform one, and the product path."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from mast3r_slam import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imgmetrics_numpy as IM  # noqa: E402
import raycast_numpy as RC  # noqa: E402
import texture_numpy as TX  # noqa: E402
import texture_sized_numpy as TS  # noqa: E402
from mesh_support import FAR, NEAR, Operands, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

# Half the gap between the sized and the uniform PSNR of the CPU statement on the mixed checker room (19.038 dB and
# 11.242 dB: tests/test_mesh_texture_sized_cpu.py asserts both), rounded down.
MIXED_MARGIN_DB = 3.8
DENSITY = 10.0                       # the strips: need = ceil(10 L + 3.5)
EDGES = {4: (0.02, 0.045), 6: (0.1, 0.2), 8: (0.3, 0.4), 64: (5.0, 6.0)}     # longest edges well inside each class
POSE = np.concatenate([[0.1, -0.2, 0.05], synthetic.quat_from_rotvec(np.array([0.3, 0.5, -0.2])), [1.7]]).astype(np.float32)


def _same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()))


@functools.lru_cache(maxsize=None)
def strip_scene(nf, n_views, hw, big=False):
    """nf random triangles about z = 2, each scaled about its centroid so that its longest edge falls in class 4, 6 or 8
    at DENSITY, the classes interleaved at random (`big`: face 3 in class 64 and the rest in class 4); n_views cameras
    near the origin with scales 1 and 1.7, random images, vertex colours."""
    rng = np.random.default_rng(2000 * nf + 10 * n_views + hw[0] + big)
    centre = np.concatenate([rng.uniform(-0.8, 0.8, (nf, 2)), rng.uniform(1.5, 2.5, (nf, 1))], 1)
    tri = rng.uniform(-0.6, 0.6, (nf, 3, 3))
    want = rng.choice([4, 6, 8], nf) if not big else np.where(np.arange(nf) == 3, 64, 4)
    e = np.stack([np.linalg.norm(tri[:, (k + 1) % 3] - tri[:, k], axis=1) for k in range(3)], 1).max(1)
    target = np.array([rng.uniform(*EDGES[int(c)]) for c in want])
    tri = (centre[:, None, :] + (tri - tri.mean(1, keepdims=True)) * (target / e)[:, None, None]).astype(np.float32)
    V, F = tri.reshape(-1, 3), np.arange(3 * nf, dtype=np.int32).reshape(nf, 3)
    h, w = hw
    K = np.array([[0.6 * w, 0, 0.5 * w - 0.5], [0, 0.6 * w, 0.5 * h - 0.5], [0, 0, 1.0]])
    poses = []
    for k in range(n_views):
        t = rng.uniform(-0.2, 0.2, 3)
        poses.append(np.concatenate([t, synthetic.quat_from_rotvec(rng.uniform(-0.15, 0.15, 3)), [1.0 if k % 2 == 0 else 1.7]]))
    poses = np.array(poses, np.float32).reshape(-1, 8)
    images = rng.uniform(0, 1, (n_views, h, w, 3)).astype(np.float32)
    colors = rng.uniform(0, 1, (len(V), 3)).astype(np.float32)
    got = np.array(TS.CLASSES)[TS.face_classes(V, F, DENSITY, texels=4)[0]]
    assert np.array_equal(got, want), "the scene's faces must land in the classes they were built for"
    return V, F, poses, K, images, colors


def _raw_layout(ops, device, V, F, density, texels, max_texels):
    """classes, rank, the host read, layout through the C entries, every operand guarded -> dict of device tensors and
    numpy copies."""
    import mslam_hip as _m

    L, st = _m.lib(), _m.stream_ptr()
    nv, nf = len(V), len(F)
    lo, cap = TS.floor_and_cap(texels, max_texels)
    v, f = ops.put(V, np.float32), ops.put(F, np.int32)
    cls, over = ops.out(torch.int32, (nf,)), ops.out(torch.int32, (nf,))
    _m.check(L.mslam_mesh_texture_classes(_m.ptr(v), _m.ptr(f), nf, nv, density, lo, cap, _m.ptr(cls), _m.ptr(over), st),
             "classes")
    ints = int(L.mslam_mesh_texture_rank_table_ints(nf))
    assert ints == 14 * ((nf + 255) // 256 + 1)
    table = ops.out(torch.int32, (ints,))
    rank, order, counts = ops.out(torch.int32, (nf,)), ops.out(torch.int32, (nf,)), ops.out(torch.int32, (14,))
    _m.check(L.mslam_mesh_texture_rank(_m.ptr(cls), _m.ptr(over), nf, _m.ptr(table), ints, _m.ptr(rank), _m.ptr(order),
                                       _m.ptr(counts), st), "rank")
    c14 = counts.cpu().numpy()
    H, W, bands = TS.sized_layout(c14[:13])
    owner, cell = ops.out(torch.int32, (H * W,)), ops.out(torch.int32, (nf, 4))
    host = (ctypes.c_int32 * 78)(*[int(x) for x in bands.reshape(-1)])
    _m.check(L.mslam_mesh_texture_layout_sized(ctypes.addressof(host), nf, H, W, _m.ptr(cls), _m.ptr(rank),
                                               _m.ptr(order), _m.ptr(owner), _m.ptr(cell), st), "layout_sized")
    return dict(v=v, f=f, owner_d=owner, cell_d=cell, H=H, W=W, cls=cls.cpu().numpy(), clamped=over.cpu().numpy(),
                rank=rank.cpu().numpy(), order=order.cpu().numpy(), counts14=c14)


def _raw_bake(device, V, F, images, poses, K, density, texels=4, max_texels=256, near=NEAR, far=FAR, tol=0.01,
              cos_min=0.1, colors=None, default_color=0.5, skip=1):
    """The sized bake through the C entry points, every operand in a guarded allocation -> dict as
    texture_sized_numpy.bake(trace=True)."""
    import mslam_hip as _m

    L, st = _m.lib(), _m.stream_ptr()
    ops = Operands(device)
    V, F = np.reshape(V, (-1, 3)), np.reshape(F, (-1, 3))
    nv, nf = len(V), len(F)
    lay = _raw_layout(ops, device, V, F, density, texels, max_texels)
    v, f, owner, cell, H, W = (lay[k] for k in ("v", "f", "owner_d", "cell_d", "H", "W"))
    n = H * W
    col = ops.put(colors, np.float32) if colors is not None else None
    sums, views = ops.put(np.zeros((n, 4)), np.float64), ops.put(np.zeros(n), np.int32)
    wb = int(L.mslam_mesh_raycast_workspace_bytes(nf))
    ws = torch.empty(max(wb, 1), dtype=torch.uint8, device=device)
    if skip and nf:
        _m.check(L.mslam_mesh_raycast_boxes(_m.ptr(v), _m.ptr(f), nf, nv, _m.ptr(ws), wb, st), "boxes")
    tr = dict(dir=[], r=[], cos=[], uv=[], t64=[], sums_after=[])
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    for k in range(len(poses)):
        h, w = images.shape[1:3]
        p8, img = ops.put(poses[k], np.float32), ops.put(images[k], np.float32)
        d, r = ops.out(torch.float32, (n, 3)), ops.out(torch.float64, (n,))
        c, uv = ops.out(torch.float64, (n,)), ops.out(torch.float64, (n, 2))
        _m.check(L.mslam_mesh_texture_rays_sized(_m.ptr(v), _m.ptr(f), nf, nv, _m.ptr(owner), _m.ptr(cell), H, W,
                                                 _m.ptr(p8), fx, fy, cx, cy, h, w, near, far, cos_min, _m.ptr(d),
                                                 _m.ptr(r), _m.ptr(c), _m.ptr(uv), st), "rays_sized")
        eye = ops.put(np.concatenate([poses[k][:3], [0, 0, 0, 1, 1]]), np.float32)
        t64 = ops.out(torch.float64, (n,))
        rng_, nrm, hit = ops.out(torch.float32, (n,)), ops.out(torch.float32, (n, 3)), ops.out(torch.uint8, (n,))
        _m.check(L.mslam_mesh_raycast(_m.ptr(d), 1, n, _m.ptr(eye), _m.ptr(v), _m.ptr(f), nf, nv, 0.0, float("inf"),
                                      1 if skip and nf else 0, _m.ptr(ws), wb, _m.ptr(rng_), _m.ptr(nrm), _m.ptr(hit), 0,
                                      _m.ptr(t64), st), "raycast")
        _m.check(L.mslam_mesh_texture_accumulate(_m.ptr(t64), _m.ptr(r), _m.ptr(c), _m.ptr(uv), _m.ptr(img), h, w,
                                                 _m.ptr(p8), tol, n, _m.ptr(sums), _m.ptr(views), st), "accumulate")
        for key, val in zip(("dir", "r", "cos", "uv", "t64", "sums_after"), (d, r, c, uv, t64, sums)):
            tr[key].append(val.cpu().numpy().copy())
    atlas = ops.out(torch.float32, (n, 3))
    _m.check(L.mslam_mesh_texture_resolve_sized(_m.ptr(f), nf, nv, _m.ptr(owner), _m.ptr(cell), H, W, _m.ptr(sums),
                                                _m.ptr(col), default_color, _m.ptr(atlas), st), "resolve_sized")
    ops.check()
    return dict(tr, atlas=atlas.cpu().numpy().reshape(H, W, 3), views=views.cpu().numpy().reshape(H, W),
                owner=owner.cpu().numpy().reshape(H, W), face_cell=cell.cpu().numpy(), sums=sums.cpu().numpy(),
                **{k: lay[k] for k in ("cls", "clamped", "rank", "order", "counts14", "H", "W")})


def _check_bake(got, want, what):
    assert (got["H"], got["W"]) == (want["H"], want["W"]), what
    _same(got["clamped"], want["clamped"].astype(np.int32), f"{what} clamped")
    _same(got["counts14"], np.append(want["counts"], want["clamped"].sum()).astype(np.int32), f"{what} counts")
    for key in ("cls", "rank", "order", "owner", "face_cell", "atlas", "views", "sums"):
        _same(got[key], want[key], f"{what} {key}")
    for key in ("dir", "r", "cos", "uv", "t64", "sums_after"):
        assert len(got[key]) == len(want[key])
        for k, (g, w) in enumerate(zip(got[key], want[key])):
            _same(g, w, f"{what} {key} of view {k}")


def _api_bake(device, V, F, images, poses, K, density, texels=4, colors=None, **kw):
    from mast3r_slam.tsdf import bake_texture

    mesh = (_dev(device, V, np.float32), _dev(device, F, np.int32))
    fb = None if colors is None else _dev(device, colors, np.float32)
    tex = bake_texture(mesh, torch.from_numpy(images).to(device), poses, K, texels=texels, fallback=fb, density=density,
                       **kw)
    return tex, mesh


def _check_api(tex, want, what):
    from mast3r_slam.tsdf import atlas_classes

    for key in ("owner", "atlas", "views", "face_cell", "face_texels"):
        _same(getattr(tex, key), want[key], f"{what} {key}")
    assert tex.sized and tex.num_faces == want["num_faces"] and tex.density == want["density"]
    assert tuple(tex.counts) == tuple(int(c) for c in want["counts"]) and tex.clamped == int(want["clamped"].sum())
    assert tex.texels in atlas_classes and (tex.cols, tex.rows) == (0, 0)
    _same(tex.uv(), TS.face_uv(want["face_cell"]).astype(np.float32), f"{what} uv")
    R = want["face_texels"].astype(np.int64)
    own = want["owner"]
    assert np.array_equal(np.bincount(own[own >= 0], minlength=len(R)), R * (R + 1) // 2)


@pytest.mark.parametrize("nf", [1, 2, 3, 7])
def test_bake_bytes_small(device, nf):
    seen = 0
    for n_views in (0, 1, 3):
        for hw in ((16, 16), (17, 9)):
            V, F, poses, K, images, colors = strip_scene(nf, n_views, hw)
            fb = colors if (n_views + hw[0]) % 2 else None
            want = TS.bake(V, F, images, poses, K, DENSITY, texels=4, fallback=fb, trace=True)
            what = f"F={nf} K={n_views} {hw}"
            _check_bake(_raw_bake(device, V, F, images, poses, K, DENSITY, colors=fb), want, what)
            tex, _ = _api_bake(device, V, F, images, poses, K, DENSITY, colors=fb)
            _check_api(tex, want, what)
            seen += int((want["views"] > 0).sum())
            assert want["owner"].size < 20000
    assert seen > 0, "the scene must exercise the accumulation"


@pytest.mark.parametrize("nf", [65, 257, 513])
def test_bake_bytes_across_a_wave_and_a_block(device, nf):
    """Interleaved classes: the stable rank crosses a wave at 65, a block at 257 and two rows of the count table at 513.
    Culled, plain and indexed bakes, and two runs, are the same bytes."""
    V, F, poses, K, images, colors = strip_scene(nf, 3, (17, 9))
    want = TS.bake(V, F, images, poses, K, DENSITY, texels=4, fallback=colors, trace=True)
    assert (want["counts"][:3] > nf // 6).all() and want["owner"].size < 20000 and (want["views"] > 0).any()
    assert len({int(c) for c in want["cls"][:64]}) == 3                # interleaved within the first wave
    _check_bake(_raw_bake(device, V, F, images, poses, K, DENSITY, colors=colors), want, f"F={nf}")
    _check_bake(_raw_bake(device, V, F, images, poses, K, DENSITY, colors=colors, skip=0), want, f"F={nf} plain")
    for kw in (dict(), dict(skip=False), dict(index=True), dict()):
        tex, _ = _api_bake(device, V, F, images, poses, K, DENSITY, colors=colors, **kw)
        _check_api(tex, want, f"F={nf} {kw}")


def test_one_large_face_among_small_ones_and_clamping(device):
    """A class-64 face among class-4 faces: a band boundary and a right margin (W = 66 = 13 cells of 5 and one texel).
    With max_texels=16 the large face is clamped."""
    V, F, poses, K, images, colors = strip_scene(8, 3, (16, 16), big=True)
    for cap, n_clamped in ((256, 0), (16, 1)):
        want = TS.bake(V, F, images, poses, K, DENSITY, texels=4, max_texels=cap, fallback=colors, trace=True)
        assert int(want["clamped"].sum()) == n_clamped and want["face_texels"][3] == min(64, cap)
        if cap == 256:
            assert want["W"] == 66 and (want["owner"][64:, 65] == -1).all() and (want["owner"][64:, :65] >= 0).any()
        _check_bake(_raw_bake(device, V, F, images, poses, K, DENSITY, max_texels=cap, colors=colors), want, f"cap {cap}")
        tex, _ = _api_bake(device, V, F, images, poses, K, DENSITY, colors=colors, max_texels=cap)
        _check_api(tex, want, f"cap {cap}")
    assert (want["views"] > 0).any()


def test_degenerate_and_out_of_range_faces(device):
    V, F, poses, K, images, colors = strip_scene(7, 3, (17, 9))
    V2 =np.concatenate([V, np.array([[0, 0, 2], [0.5, 0.5, 2], [1, 1, 2]], np.float32)])      # three points on a line
    nv = len(V2)
    bad = np.array([[nv - 3, nv - 2, nv - 1], [0, 0, 1], [0, 1, nv], [-1, 2, 3]], np.int32)
    F2 = np.concatenate([F[:3], bad, F[3:]]).astype(np.int32)
    col2 = np.concatenate([colors, colors[:3]])
    for fb in (col2, None):
        want = TS.bake(V2, F2, images, poses, K, DENSITY, texels=6, fallback=fb, default_color=0.25, trace=True)
        got = _raw_bake(device, V2, F2, images, poses, K, DENSITY, texels=6, colors=fb, default_color=0.25)
        _check_bake(got, want, "invalid faces")
        assert list(want["face_texels"][5:7]) == [6, 6] and want["face_texels"][3] == 24      # the line is 1.41 long
        for f in range(3, 7):
            assert not want["views"][want["owner"] == f].any()
        with pytest.raises(ValueError, match=r"outside \[0, "):
            _api_bake(device, V2, F2, images, poses, K, DENSITY, texels=6, colors=fb)
        tex, _ = _api_bake(device, V2, F2, images, poses, K, DENSITY, texels=6, colors=fb, default_color=0.25,
                           validate=False)
        _check_api(tex, want, "invalid faces, api")
    assert (want["views"] > 0).any()
    tex, _ =_api_bake(device, V, F[:0], images, poses, K, DENSITY)
    assert tuple(tex.atlas.shape) == (0, 0, 3) and tex.num_faces == 0 and tuple(tex.uv().shape) == (0, 3, 2)
    assert tex.counts == (0,) * 13 and tuple(tex.face_cell.shape) == (0, 4)


@pytest.mark.parametrize("R", [6, 8])
def test_one_class_mesh_equals_the_uniform_bake(device, R):
    """The cross-check against the existing path: every face in class R, baked with texels=R and with density; the
    per-face (li, lj) blocks of atlas and views, gathered from both atlases, are the same bytes."""
    from mast3r_slam.tsdf import bake_texture

    V, F, poses, K, images, colors = strip_scene(7, 3, (17, 9))
    e, _ = TS.edge_lengths(V, F)
    scale = (np.array(EDGES[R]).mean() / e.max(1))                    # every longest edge to the middle of class R
    tri = V.reshape(-1, 3, 3).astype(np.float64)
    V = (tri.mean(1, keepdims=True) + (tri - tri.mean(1, keepdims=True)) * scale[:, None, None]).astype(np.float32).reshape(-1, 3)
    mesh = (_dev(device, V, np.float32), _dev(device, F, np.int32))
    img, col = torch.from_numpy(images).to(device), _dev(device, colors, np.float32)
    uni = bake_texture(mesh, img, poses, K, texels=R, fallback=col)
    siz = bake_texture(mesh, img, poses, K, texels=4, fallback=col, density=DENSITY)
    assert (siz.face_texels == R).all() and tuple(siz.atlas.shape) != tuple(uni.atlas.shape)
    o_u, li_u, lj_u = TX.texel_owner(7, R)
    o_s = siz.owner.cpu().numpy()
    li_s, lj_s, _ = TS.texel_local(o_s, siz.face_cell.cpu().numpy())
    blocks = []
    for tex, o, li, lj in ((uni, o_u, li_u, lj_u), (siz, o_s, li_s, lj_s)):
        a, v = np.zeros((7, R, R, 3), np.float32), np.full((7, R, R), -1, np.int32)
        m = o >= 0
        a[o[m], li[m], lj[m]] = tex.atlas.cpu().numpy()[m]
        v[o[m], li[m], lj[m]] = tex.views.cpu().numpy()[m]
        assert (v >= 0).sum() == 7 * R * (R + 1) // 2
        blocks.append((a, v))
    _same(blocks[1][0], blocks[0][0], "atlas blocks")
    _same(blocks[1][1], blocks[0][1], "views blocks")
    assert (blocks[0][1] > 0).any()


@functools.lru_cache(maxsize=None)
def _shade_case():
    from test_mesh_raycast_gpu import tile_mesh

    V, F = tile_mesh(129)
    h, w = 17, 9
    K = np.array([[0.6 * w, 0, 0.5 * w], [0, 0.6 * w, 0.5 * h], [0, 0, 1.0]])
    d = synthetic.pixel_rays(h, w, K)
    rays = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    lay = TS.layout(V, F, 3.0, texels=4)
    assert len(np.unique(lay["cls"])) >= 3
    rng = np.random.default_rng(11)
    atlas = rng.uniform(0, 1, (lay["H"], lay["W"], 3)).astype(np.float32)
    colors = rng.uniform(0, 1, (len(V), 3)).astype(np.float32)
    return V, F, rays, lay, atlas, colors, RC.render(POSE, rays, V, F, NEAR, FAR)


def test_shade_both_modes_on_a_17x9_image(device):
    import mslam_hip as _m
    from mast3r_slam.tsdf import MeshTexture, render_mesh, render_mesh_color

    V, F, rays, lay, atlas, colors, want = _shade_case()
    h, w = rays.shape[:2]
    assert 0 < want[2].sum() < h * w
    mesh = (_dev(device, V, np.float32), _dev(device, F, np.int32))
    z = torch.zeros(atlas.shape[:2], dtype=torch.int32, device=device)
    tex = MeshTexture(_dev(device, atlas, np.float32), z, z, 4, 0, 0, len(F), face_cell=_dev(device, lay["face_cell"], np.int32),
                      face_texels=_dev(device, lay["face_texels"], np.int32), counts=tuple(int(c) for c in lay["counts"]),
                      density=3.0)
    plain = render_mesh(mesh, POSE, rays=rays, near=NEAR, far=FAR)
    ref_t = TS.shade_texture(POSE, rays, V, F, want[3], atlas, lay["face_cell"])
    ref_c = TX.shade_colors(POSE, rays, V, F, want[3], colors)
    assert ref_t[want[2] > 0].any()
    for kw, ref in ((dict(colors=_dev(device, colors, np.float32)), ref_c), (dict(texture=tex), ref_t)):
        for more in (dict(), dict(skip=False), dict(index=True)):
            out = render_mesh_color(mesh, POSE, rays=rays, near=NEAR, far=FAR, **kw, **more)
            for a, b in zip(out[:3], plain):
                assert a.dtype == b.dtype and torch.equal(a, b)
            _same(out[3].reshape(-1, 3), ref, f"render_mesh_color {list(kw)} {more}")
    # the raw entry behind guards, and a cell outside the atlas shades as a miss
    for cells, ref in ((lay["face_cell"], ref_t), (lay["face_cell"] + np.int32([lay["W"], 0, 0, 0]), np.zeros_like(ref_t))):
        ops = Operands(device)
        fc, r, p = ops.put(want[3], np.int32), ops.put(rays.reshape(-1, 3), np.float32), ops.put(POSE, np.float32)
        v, f, a, c = ops.put(V, np.float32), ops.put(F, np.int32), ops.put(atlas, np.float32), ops.put(cells, np.int32)
        rgb = ops.out(torch.float32, (h * w, 3))
        _m.check(_m.lib().mslam_mesh_shade_sized(_m.ptr(fc), _m.ptr(r), h, w, _m.ptr(p), _m.ptr(v), _m.ptr(f), len(F),
                                                 len(V), _m.ptr(a), _m.ptr(c), lay["H"], lay["W"], _m.ptr(rgb),
                                                 _m.stream_ptr()), "mesh_shade_sized")
        ops.check()
        _same(rgb, ref, "raw shade")


def test_refused_arguments(device):
    import mslam_hip as _m
    from mast3r_slam.tsdf import MeshTexture, bake_texture, render_mesh_color

    V, F, poses, K, images, colors = strip_scene(7, 1, (16, 16))
    mesh = (_dev(device, V, np.float32), _dev(device, F, np.int32))
    img = torch.from_numpy(images).to(device)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="density"):
            bake_texture(mesh, img, poses, K, density=bad)
    for kw in (dict(texels=8, max_texels=7), dict(texels=9, max_texels=8), dict(texels=4, max_texels=3)):
        with pytest.raises(ValueError, match="max_texels"):
            bake_texture(mesh, img, poses, K, density=DENSITY, **kw)
    for bad in (3, 257, 4.5):
        with pytest.raises(ValueError, match="texels"):
            bake_texture(mesh, img, poses, K, density=DENSITY, texels=bad)
    tex = bake_texture(mesh, img, poses, K, density=DENSITY, texels=4)
    rays = np.zeros((3, 3, 3), np.float32) + np.float32([0, 0, 1])
    with pytest.raises(ValueError, match="faces"):
        render_mesh_color((mesh[0], mesh[1][:5].contiguous()), POSE, texture=tex, rays=rays)
    args = (tex.views, tex.owner, tex.texels, 0, 0, 7)
    more = dict(face_texels=tex.face_texels, counts=tex.counts)
    with pytest.raises(ValueError, match="sized layout"):
        render_mesh_color(mesh, POSE, texture=MeshTexture(tex.atlas[:-1], *args, face_cell=tex.face_cell, **more), rays=rays)
    with pytest.raises(ValueError, match="face_cell"):
        render_mesh_color(mesh, POSE, texture=MeshTexture(tex.atlas, *args, face_cell=tex.face_cell[:-1], **more), rays=rays)
    with pytest.raises(ValueError, match="face_cell"):
        render_mesh_color(mesh, POSE, texture=MeshTexture(tex.atlas, *args, face_cell=tex.face_cell.cpu(), **more), rays=rays)
    assert render_mesh_color(mesh, POSE, texture=tex, rays=rays)[3].shape == (3, 3, 3)
    # the C entries
    L = _m.lib()
    nf, nv = 7, len(V)
    cls, over = (torch.zeros(nf, dtype=torch.int32, device=device) for _ in range(2))
    classes = lambda d=DENSITY, lo=0, cap=12, c=_m.ptr(cls): L.mslam_mesh_texture_classes(
        _m.ptr(mesh[0]), _m.ptr(mesh[1]), nf, nv, d, lo, cap, c, _m.ptr(over), 0)
    assert classes(d=0.0) != 0 and classes(d=float("nan")) != 0 and classes(lo=5, cap=4) != 0 and classes(cap=13) != 0
    assert classes(lo=-1) != 0 and classes(c=0) != 0 and classes() == 0
    table = torch.zeros(28, dtype=torch.int32, device=device)
    rank, order = (torch.zeros(nf, dtype=torch.int32, device=device) for _ in range(2))
    counts = torch.zeros(14, dtype=torch.int32, device=device)
    ranks = lambda ints=28, t=_m.ptr(table), n_=nf, r=_m.ptr(rank): L.mslam_mesh_texture_rank(
        _m.ptr(cls), _m.ptr(over), n_, t, ints, r, _m.ptr(order), _m.ptr(counts), 0)
    assert ranks(ints=27) != 0 and ranks(t=0) != 0 and ranks(n_=-1) != 0 and ranks(r=0) != 0 and ranks() == 0
    got = counts.cpu().numpy()
    H, W, bands = TS.sized_layout(got[:13])
    owner = torch.zeros(H * W, dtype=torch.int32, device=device)
    cell = torch.zeros((nf, 4), dtype=torch.int32, device=device)

    def lay(b=bands, n_=nf, H_=H, W_=W, o=_m.ptr(owner)):
        host = (ctypes.c_int32 * 78)(*[int(x) for x in np.asarray(b).reshape(-1)])
        return L.mslam_mesh_texture_layout_sized(ctypes.addressof(host), n_, H_, W_, _m.ptr(cls), _m.ptr(rank),
                                                 _m.ptr(order), o, _m.ptr(cell), 0)

    used = int(np.flatnonzero(got[:13])[0])
    wrong = []
    for col_, delta in ((0, 1), (1, 1), (2, -1), (3, 1), (4, 1), (5, 1), (5, -1)):     # every column of a band in use
        b = bands.copy()
        b[used, col_] += delta
        wrong.append(b)
    assert all(lay(b=b) != 0 for b in wrong), [lay(b=b) for b in wrong]
    assert lay(n_=nf + 1) != 0 and lay(H_=H + 1) != 0 and lay(W_=-1) != 0 and lay(o=0) != 0
    assert L.mslam_mesh_texture_layout_sized(0, nf, H, W, _m.ptr(cls), _m.ptr(rank), _m.ptr(order), _m.ptr(owner),
                                             _m.ptr(cell), 0) != 0
    assert lay() == 0
    n = H * W
    d = torch.empty((n, 3), dtype=torch.float32, device=device)
    r, c, uv = (torch.empty(n * k, dtype=torch.float64, device=device) for k in (1, 1, 2))
    p8 = _dev(device, poses[0], np.float32)
    call = lambda h=16, w=16, near=NEAR, far=FAR, H_=H, o=_m.ptr(owner): L.mslam_mesh_texture_rays_sized(
        _m.ptr(mesh[0]), _m.ptr(mesh[1]), nf, nv, o, _m.ptr(cell), H_, W, _m.ptr(p8), 9.6, 9.6, 7.5, 7.5, h, w, near,
        far, 0.1, _m.ptr(d), _m.ptr(r), _m.ptr(c), _m.ptr(uv), 0)
    assert call(h=1) != 0 and call(w=1) != 0 and call(near=2.0, far=1.0) != 0 and call(H_=-1) != 0 and call(o=0) != 0
    assert call(H_=1 << 30) != 0 and "int32" in L.mslam_last_error().decode()
    assert call() == 0
    sums, atlas = torch.zeros((n, 4), dtype=torch.float64, device=device), torch.empty((n, 3), dtype=torch.float32, device=device)
    res = lambda s=_m.ptr(sums), W_=W: L.mslam_mesh_texture_resolve_sized(
        _m.ptr(mesh[1]), nf, nv, _m.ptr(owner), _m.ptr(cell), H, W_, s, 0, 0.5, _m.ptr(atlas), 0)
    assert res(s=0) != 0 and res(W_=-1) != 0 and res() == 0
    rgb = torch.empty((9, 3), dtype=torch.float32, device=device)
    fc = torch.full((9,), -1, dtype=torch.int32, device=device)
    rd = _dev(device, rays, np.float32)
    sh = lambda a=_m.ptr(atlas), cl=_m.ptr(cell), H_=H: L.mslam_mesh_shade_sized(
        _m.ptr(fc), _m.ptr(rd), 3, 3, _m.ptr(p8), _m.ptr(mesh[0]), _m.ptr(mesh[1]), nf, nv, a, cl, H_, W, _m.ptr(rgb), 0)
    assert sh(a=0) != 0 and sh(cl=0) != 0 and sh(H_=-1) != 0 and sh() == 0
    torch.cuda.synchronize()
    assert not rgb.any()                                               # every pixel a miss


@functools.lru_cache(maxsize=None)
def _mixed():
    return TS.mixed_statement()


def test_mixed_checker_room_sized_beats_uniform(device):
    """The test that cannot pass without the feature.  The checker room with its +x wall cut into 16 x 12 squares (394
    faces), density 9 over a floor of 8, against the uniform atlas at the smallest texels with no fewer owned texels
    (15).  CPU statement (asserted in tests/test_mesh_texture_sized_cpu.py): sized 19.038 dB, uniform 11.242 dB; the
    margin is half the gap.  The six images equal the statement's byte for byte."""
    from mast3r_slam.tsdf import bake_texture, image_metrics, render_mesh_color

    scene, want_s, (ref_s, hit_s), want_u, (ref_u, hit_u) = _mixed()
    mesh = (_dev(device, scene["V"], np.float32), _dev(device, scene["F"], np.int32))
    images = torch.from_numpy(scene["images"]).to(device)
    sized = bake_texture(mesh, images, scene["poses"], scene["K"], texels=TS.MIXED_TEXELS, density=TS.MIXED_DENSITY)
    _check_api(sized, want_s, "mixed room")
    uni = bake_texture(mesh, images, scene["poses"], scene["K"], texels=want_u["texels"])
    _same(uni.atlas, want_u["atlas"], "mixed room, uniform atlas")
    assert int((uni.owner >= 0).sum()) >= int((sized.owner >= 0).sum()) == 44928
    psnr = {}
    for name, tex, ref, hit in (("sized", sized, ref_s, hit_s), ("uniform", uni, ref_u, hit_u)):
        views = [render_mesh_color(mesh, p, texture=tex, rays=scene["rays"]) for p in scene["poses"]]
        rgb, mask = torch.stack([v[3] for v in views]), torch.stack([v[2] for v in views])
        _same(rgb, ref, f"mixed room {name} rgb")
        assert np.array_equal(mask.cpu().numpy(), hit)
        psnr[name] = float(image_metrics(rgb, images, mask=mask)["psnr"].cpu().numpy().mean())
        st = IM.image_metrics(ref, scene["images"], hit)["psnr"].mean()
        assert abs(psnr[name] - st) <= 1e-6, (name, psnr[name], st)
    print(f"mixed checker room: PSNR sized {psnr['sized']:.3f} dB on {tuple(sized.atlas.shape[:2])}, uniform texels="
          f"{uni.texels} {psnr['uniform']:.3f} dB on {tuple(uni.atlas.shape[:2])}; margin asserted {MIXED_MARGIN_DB} dB")
    assert psnr["sized"] > psnr["uniform"] + MIXED_MARGIN_DB


def test_product_session(device, tmp_path, monkeypatch):
    """The 20-frame colour session of test_mesh_texture_gpu.py::test_product_session with a sized atlas: every face owns
    its R_f (R_f + 1) / 2 texels, the mesh is scored and written.  Prints; no threshold on quality."""
    from mast3r_slam import evaluate
    from mast3r_slam.config import config
    from test_color_product_gpu import _session
    from test_slam_system_gpu import H, W

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    K = synthetic.intrinsics(H, W)
    system = _session(device, True)
    try:
        mesh = system.extract_mesh(colors=True, decimate_ratio=0.2)
        vs = system.tsdf_manager.volume.voxel_size
        sized = system.bake_texture(mesh, K=K, fallback=True, density=2.0 / vs, texels=4)
        monkeypatch.setitem(system.tsdf_manager.cfg, "mesh_texture_density", 2.0)
        by_config = system.bake_texture(mesh, K=K, fallback=True, texels=4)              # the configured density
        monkeypatch.setitem(system.tsdf_manager.cfg, "mesh_texture_density", 0.0)
        uniform = system.bake_texture(mesh, K=K, fallback=True)
        R_same = TS.uniform_texels_for(sized.num_faces, int((sized.owner >= 0).sum()))  # no fewer owned texels
        same = system.bake_texture(mesh, K=K, fallback=True, texels=R_same)
        figs = {name: system.evaluate_mesh_render(mesh, texture=t)
                for name, t in (("sized", sized), ("uniform", uniform), ("same", same))}
        paths = evaluate.save_textured_mesh(tmp_path, "map", mesh[0], mesh[2], sized, normals=mesh[1])
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    assert sized.sized and by_config.sized and not uniform.sized and by_config.density == sized.density
    assert torch.equal(by_config.atlas, sized.atlas) and torch.equal(by_config.face_cell, sized.face_cell)
    R = sized.face_texels.cpu().numpy().astype(np.int64)
    own = sized.owner.cpu().numpy()
    assert sized.num_faces == mesh[2].shape[0] == len(R) and sum(sized.counts) == len(R)
    assert np.array_equal(np.bincount(own[own >= 0], minlength=len(R)), R * (R + 1) // 2)
    for d in figs.values():
        assert np.isfinite([d[k] for k in ("psnr", "ssim", "psnr_min", "ssim_min", "hit_share", "window_share")]).all()
    v, vt, vn, fc, lib, use = TX.parse_obj(paths[0].read_text())
    assert len(vt) == 3 * sized.num_faces and np.array_equal(fc[:, :, 0], mesh[2].cpu().numpy())
    hist = {r: int(c) for r, c in zip(TS.CLASSES, sized.counts) if c}
    n_s, n_u = int((own >= 0).sum()), int((uniform.owner >= 0).sum())
    print(f"20-frame colour session, mesh decimated to {sized.num_faces} faces: sized atlas at {2.0:.1f} texels per voxel "
          f"{tuple(sized.atlas.shape[:2])}, classes {hist}, {sized.clamped} clamped, {n_s} owned texels (fill "
          f"{n_s / max(own.size, 1):.3f}): PSNR / SSIM {figs['sized']['psnr']:.3f} / {figs['sized']['ssim']:.4f}; uniform "
          f"texels=8 {tuple(uniform.atlas.shape[:2])}, {n_u} owned texels: {figs['uniform']['psnr']:.3f} / "
          f"{figs['uniform']['ssim']:.4f}; uniform texels={R_same} {tuple(same.atlas.shape[:2])}, "
          f"{int((same.owner >= 0).sum())} owned texels: {figs['same']['psnr']:.3f} / {figs['same']['ssim']:.4f}")
