"""GPU tests (-m gpu) of the mesh textures (csrc/mesh_texture.hip, DESIGN.md "Mesh textures") and of
mast3r_slam.tsdf.bake_texture / render_mesh_color / MeshTexture, evaluate.save_textured_mesh and
SlamSystem.bake_texture / evaluate_mesh_render: byte for byte against the numpy statement (tests/texture_numpy.py) -
owner, atlas, views and, through the raw entries, dir, r, cos, uv and sums after every view - at the block edge and the
ray cast's tile edge, culled, plain and indexed, degenerate and out-of-range faces behind guarded buffers, refused
arguments, run-to-run identity, both shading modes at the cast's tile edges, the checker room whose texture must beat
its vertex colours, and the product path."""
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
from mesh_support import FAR, NEAR, Operands, _dev  # noqa: E402
from test_mesh_raycast_cpu import occluder_scene  # noqa: E402
from test_mesh_raycast_gpu import POSE, tile_case  # noqa: E402

pytestmark = pytest.mark.gpu

# Half the gap between the textured and the vertex-colour PSNR of the CPU statement on the checker room (17.272 dB and
# 6.411 dB: tests/test_mesh_texture_cpu.py asserts both, DESIGN.md "Mesh textures" quotes them), rounded down.
CHECKER_MARGIN_DB = 5.4


def _same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()))


@functools.lru_cache(maxsize=None)
def bake_scene(nf, n_views, hw):
    """nf random triangles about z = 2 that face the origin or not, one of them seen edge-on from far off, n_views
    cameras near the origin looking along +z with scales 1 and 1.7, random images, vertex colours."""
    rng = np.random.default_rng(1000 * nf + 10 * n_views + hw[0])
    centre = np.concatenate([rng.uniform(-0.8, 0.8, (nf, 2)), rng.uniform(1.5, 2.5, (nf, 1))], 1)
    tri = (centre[:, None, :] + rng.uniform(-0.6, 0.6, (nf, 3, 3))).astype(np.float32)
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
    return V, F, poses, K, images, colors


def _raw_bake(device, V, F, images, poses, K, R, near=NEAR, far=FAR, tol=0.01, cos_min=0.1, colors=None,
              default_color=0.5, skip=1):
    """The bake through the C entry points, every operand in a guarded allocation -> dict as texture_numpy.bake(trace)."""
    import mslam_hip as _m

    L, st = _m.lib(), _m.stream_ptr()
    ops = Operands(device)
    V, F = np.reshape(V, (-1, 3)), np.reshape(F, (-1, 3))
    nv, nf = len(V), len(F)
    cols, rows, H, W = TX.layout(nf, R)
    n = H * W
    v, f = ops.put(V, np.float32), ops.put(F, np.int32)
    col = ops.put(colors, np.float32) if colors is not None else None
    owner = ops.out(torch.int32, (n,))
    _m.check(L.mslam_mesh_texture_layout(nf, R, cols, rows, _m.ptr(owner), st), "layout")
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
        _m.check(L.mslam_mesh_texture_rays(_m.ptr(v), _m.ptr(f), nf, nv, R, cols, rows, _m.ptr(p8), fx, fy, cx, cy, h, w,
                                           near, far, cos_min, _m.ptr(d), _m.ptr(r), _m.ptr(c), _m.ptr(uv), st), "rays")
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
    _m.check(L.mslam_mesh_texture_resolve(_m.ptr(f), nf, nv, R, cols, rows, _m.ptr(sums), _m.ptr(col), default_color,
                                          _m.ptr(atlas), st), "resolve")
    ops.check()
    return dict(tr, atlas=atlas.cpu().numpy().reshape(H, W, 3), views=views.cpu().numpy().reshape(H, W),
                owner=owner.cpu().numpy().reshape(H, W), sums=sums.cpu().numpy())


def _statement_with_sums(V, F, images, poses, K, R, **kw):
    """texture_numpy.bake(trace=True) plus sums_after: the sums after each view, from the bakes of the first k views."""
    want = TX.bake(V, F, images, poses, K, R=R, trace=True, **kw)
    want["sums_after"] = [TX.bake(V, F, images[:k + 1], poses[:k + 1], K, R=R, **kw)["sums"] for k in range(len(poses))]
    return want


def _check_bake(got, want, what):
    for key in ("owner", "atlas", "views", "sums"):
        _same(got[key], want[key], f"{what} {key}")
    for key in ("dir", "r", "cos", "uv", "t64", "sums_after"):
        assert len(got[key]) == len(want[key])
        for k, (g, w) in enumerate(zip(got[key], want[key])):
            _same(g, w, f"{what} {key} of view {k}")


def _api_bake(device, V, F, images, poses, K, R, colors=None, **kw):
    from mast3r_slam.tsdf import bake_texture

    mesh = (_dev(device, V, np.float32), _dev(device, F, np.int32))
    fb = None if colors is None else _dev(device, colors, np.float32)
    return bake_texture(mesh, torch.from_numpy(images).to(device), poses, K, texels=R, fallback=fb, **kw), mesh


def _check_api(tex, want, what):
    _same(tex.owner, want["owner"], f"{what} owner")
    _same(tex.atlas, want["atlas"], f"{what} atlas")
    _same(tex.views, want["views"], f"{what} views")
    assert (tex.texels, tex.cols, tex.rows, tex.num_faces) == (want["texels"], want["cols"], want["rows"], want["num_faces"])


@pytest.mark.parametrize("R", [4, 5, 8])
@pytest.mark.parametrize("nf", [1, 2, 3, 7])
def test_bake_bytes(device, nf, R):
    """F = 7 with R = 8 is 288 texels, one past a block."""
    seen = 0
    for n_views in (0, 1, 3):
        for hw in ((16, 16), (17, 9)):
            V, F, poses, K, images, colors = bake_scene(nf, n_views, hw)
            fb = colors if (n_views + hw[0]) % 2 else None
            want = _statement_with_sums(V, F, images, poses, K, R, fallback=fb)
            what = f"F={nf} R={R} K={n_views} {hw}"
            _check_bake(_raw_bake(device, V, F, images, poses, K, R, colors=fb), want, what)
            tex, _ = _api_bake(device, V, F, images, poses, K, R, colors=fb)
            _check_api(tex, want, what)
            _same(tex.uv(), TX.face_uv(nf, R).astype(np.float32), f"{what} uv")
            seen += int((want["views"] > 0).sum())
            if n_views == 0:
                assert not want["views"].any()
    assert seen > 0, "the scene must exercise the accumulation"
    if (nf, R) == (7, 8):
        assert want["owner"].size == 288
    print(f"F={nf} R={R}: {seen} (texel, view-set) pairs seen over the six cases")


def test_bake_at_the_cast_tile_edge_and_run_to_run(device):
    """F = 129 with R = 4: the second tile of the ray cast holds one face.  Culled, plain and indexed bakes are the same
    bytes, and so are two runs."""
    V, F, poses, K, images, colors = bake_scene(129, 3, (17, 9))
    want = _statement_with_sums(V, F, images, poses, K, 4, fallback=colors)
    got = _raw_bake(device, V, F, images, poses, K, 4, colors=colors)
    _check_bake(got, want, "F=129 R=4")
    _check_bake(_raw_bake(device, V, F, images, poses, K, 4, colors=colors, skip=0), want, "F=129 R=4 plain")
    assert (want["views"] > 0).sum() > 0 and (want["owner"] == 128).sum() == 10
    for kw in (dict(), dict(skip=False), dict(index=True), dict()):
        tex, _ = _api_bake(device, V, F, images, poses, K, 4, colors=colors, **kw)
        _check_api(tex, want, f"F=129 R=4 {kw}")


def test_occluder_scene_culled_plain_indexed(device):
    V, F, poses, K, hw, _, _ = occluder_scene()
    rng = np.random.default_rng(5)
    two = np.stack([poses[0], np.array([0.5, 0.2, -0.3, 0, 0, 0, 1, 1.7], np.float32)])
    images = rng.uniform(0, 1, (2,) + hw + (3,)).astype(np.float32)
    want = TX.bake(V, F, images, two, K, R=16)
    assert (want["views"] == 2).any() and (want["views"] == 1).any()
    p = TX.texel_points(V, F, 16)
    shadow = np.isin(p["owner"], (10, 11)) & (np.abs(p["p"][:, 0]) < 0.49) & (np.abs(p["p"][:, 1]) < 0.49)
    for kw in (dict(), dict(skip=False), dict(index=True)):
        tex, _ = _api_bake(device, V, F, images, two, K, 16, **kw)
        _check_api(tex, want, f"occluder {kw}")
    first = TX.bake(V, F, images[:1], two[:1], K, R=16)["views"].reshape(-1)
    assert shadow.sum() > 0 and (first[shadow] == 0).all()             # the quad's shadow, seen by the first camera


def test_degenerate_and_out_of_range_faces(device):
    """No view takes part in them, the fallback (or the default colour) is used, nothing outside the outputs is written
    (the guards of _raw_bake)."""
    V, F, poses, K, images, colors = bake_scene(7, 3, (16, 16))
    V2 = np.concatenate([V, np.array([[0, 0, 2], [0.5, 0.5, 2], [1, 1, 2]], np.float32)])      # three points on a line
    nv = len(V2)
    bad = np.array([[nv - 3, nv - 2, nv - 1], [0, 0, 1], [0, 1, nv], [-1, 2, 3]], np.int32)
    F2 = np.concatenate([F[:3], bad, F[3:]]).astype(np.int32)
    col2 = np.concatenate([colors, colors[:3]])
    for fb in (col2, None):
        want = _statement_with_sums(V2, F2, images, poses, K, 5, fallback=fb, default_color=0.25)
        got = _raw_bake(device, V2, F2, images, poses, K, 5, colors=fb, default_color=0.25)
        _check_bake(got, want, "invalid faces")
        for f in range(3, 7):
            mine = want["owner"] == f
            assert mine.sum() == 15 and not want["views"][mine].any()
            if f >= 5 or fb is None:                                   # out of range: the default colour
                assert (got["atlas"][mine] == np.float32(0.25)).all()
        with pytest.raises(ValueError, match=r"outside \[0, "):
            _api_bake(device, V2, F2, images, poses, K, 5, colors=fb, default_color=0.25)
        tex, _ = _api_bake(device, V2, F2, images, poses, K, 5, colors=fb, default_color=0.25, validate=False)
        _check_api(tex, want, "invalid faces, api")
    assert (want["views"] > 0).any()
    # no faces at all
    tex, _ = _api_bake(device, V, F[:0], images, poses, K, 8)
    assert tuple(tex.atlas.shape) == (0, 0, 3) and tex.num_faces == 0 and tuple(tex.uv().shape) == (0, 3, 2)


def test_refused_arguments(device):
    import mslam_hip as _m
    from mast3r_slam.tsdf import MeshTexture, bake_texture, render_mesh_color

    V, F, poses, K, images, colors = bake_scene(7, 1, (16, 16))
    mesh = (_dev(device, V, np.float32), _dev(device, F, np.int32))
    img, col = torch.from_numpy(images).to(device), _dev(device, colors, np.float32)
    for R in (3, 0, -2):
        with pytest.raises(ValueError, match="texels"):
            bake_texture(mesh, img, poses, K, texels=R)
    for shape in ((1, 1, 16, 3), (1, 16, 1, 3)):
        with pytest.raises(ValueError, match="2x2"):
            bake_texture(mesh, torch.zeros(shape, device=device), poses, K)
    with pytest.raises(ValueError, match="poses"):
        bake_texture(mesh, img, poses[:0], K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bake_texture(mesh, img, poses, K, fallback=col.cpu())          # mismatched devices
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bake_texture((mesh[0].cpu(), mesh[1]), img, poses, K)
    with pytest.raises(ValueError, match="fallback"):
        bake_texture(mesh, img, poses, K, fallback=col[:-1])
    with pytest.raises(ValueError, match="fallback=True"):
        bake_texture(mesh, img, poses, K, fallback=True)
    tex = bake_texture(mesh, img, poses, K, texels=4)
    rays = np.zeros((3, 3, 3), np.float32) + np.float32([0, 0, 1])
    for kw in (dict(), dict(colors=col, texture=tex)):
        with pytest.raises(ValueError, match="exactly one"):
            render_mesh_color(mesh, POSE, rays=rays, **kw)
    with pytest.raises(ValueError, match="faces"):
        render_mesh_color((mesh[0], mesh[1][:5].contiguous()), POSE, texture=tex, rays=rays)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render_mesh_color(mesh, POSE, colors=col.cpu(), rays=rays)
    with pytest.raises(ValueError, match="colors"):
        render_mesh_color(mesh, POSE, colors=col[:-1], rays=rays)
    with pytest.raises(TypeError, match="MeshTexture"):
        render_mesh_color(mesh, POSE, texture=tex.atlas, rays=rays)
    assert isinstance(tex, MeshTexture)
    # the C entries
    L = _m.lib()
    n = tex.atlas.shape[0] * tex.atlas.shape[1]
    own = torch.empty(n, dtype=torch.int32, device=device)
    assert L.mslam_mesh_texture_layout(7, 3, 2, 2, _m.ptr(own), 0) != 0           # R <= 3
    assert L.mslam_mesh_texture_layout(7, 4, 1, 3, _m.ptr(own), 0) != 0           # too few cells
    assert L.mslam_mesh_texture_layout(7, 4, 2, 2, 0, 0) != 0                     # null
    assert L.mslam_mesh_texture_layout(1 << 29, 64, 1 << 14, 1 << 14, _m.ptr(own), 0) != 0
    assert "int32" in L.mslam_last_error().decode()
    assert L.mslam_mesh_texture_layout(7, 4, 2, 2, _m.ptr(own), 0) == 0
    d = torch.empty((n, 3), dtype=torch.float32, device=device)
    r, c, uv = (torch.empty(n * k, dtype=torch.float64, device=device) for k in (1, 1, 2))
    p8 = _dev(device, poses[0], np.float32)
    call = lambda h=16, w=16, near=NEAR, far=FAR, R=4: L.mslam_mesh_texture_rays(
        _m.ptr(mesh[0]), _m.ptr(mesh[1]), 7, len(V), R, 2, 2, _m.ptr(p8), 9.6, 9.6, 7.5, 7.5, h, w, near, far, 0.1,
        _m.ptr(d), _m.ptr(r), _m.ptr(c), _m.ptr(uv), 0)
    assert call(h=1) != 0 and call(w=1) != 0 and call(near=2.0, far=1.0) != 0 and call(R=3) != 0 and call() == 0
    sums, views = torch.zeros((n, 4), dtype=torch.float64, device=device), torch.zeros(n, dtype=torch.int32, device=device)
    acc = lambda h=16, w=16, n_=n, t=_m.ptr(r): L.mslam_mesh_texture_accumulate(
        t, _m.ptr(r), _m.ptr(c), _m.ptr(uv), _m.ptr(img), h, w, _m.ptr(p8), 0.01, n_, _m.ptr(sums), _m.ptr(views), 0)
    assert acc(h=1) != 0 and acc(n_=-1) != 0 and acc(t=0) != 0 and acc() == 0
    rgb = torch.empty((9, 3), dtype=torch.float32, device=device)
    fc = torch.full((9,), -1, dtype=torch.int32, device=device)
    rd = _dev(device, rays, np.float32)
    sh = lambda colors, atlas, R=4: L.mslam_mesh_shade(_m.ptr(fc), _m.ptr(rd), 3, 3, _m.ptr(p8), _m.ptr(mesh[0]),
                                                       _m.ptr(mesh[1]), 7, len(V), colors, atlas, R, 2, 2, _m.ptr(rgb), 0)
    assert sh(0, 0) != 0 and sh(_m.ptr(col), _m.ptr(tex.atlas)) != 0 and sh(0, _m.ptr(tex.atlas), R=3) != 0
    assert sh(_m.ptr(col), 0) == 0 and sh(0, _m.ptr(tex.atlas)) == 0
    torch.cuda.synchronize()
    assert not rgb.any()                                               # every pixel a miss


def _raw_shade(device, face, rays, h, w, pose, V, F, colors=None, atlas=None, layout=(0, 0, 0)):
    import mslam_hip as _m

    ops = Operands(device)
    fc, r, p = ops.put(face, np.int32), ops.put(np.reshape(rays, (-1, 3)), np.float32), ops.put(pose, np.float32)
    v, f = ops.put(V, np.float32), ops.put(F, np.int32)
    c = ops.put(colors, np.float32) if colors is not None else None
    a = ops.put(atlas, np.float32) if atlas is not None else None
    rgb = ops.out(torch.float32, (h * w, 3))
    _m.check(_m.lib().mslam_mesh_shade(_m.ptr(fc), _m.ptr(r), h, w, _m.ptr(p), _m.ptr(v), _m.ptr(f), len(F), len(V),
                                       _m.ptr(c), _m.ptr(a), *layout, _m.ptr(rgb), _m.stream_ptr()), "mesh_shade")
    ops.check()
    return rgb.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _paint(nf, R):
    """Vertex colours and an atlas with a different random colour in every texel, for a mesh of nf faces."""
    rng = np.random.default_rng(nf + R)
    cols, rows, H, W = TX.layout(nf, R)
    return rng.uniform(0, 1, (3 * nf, 3)).astype(np.float32), rng.uniform(0, 1, (H, W, 3)).astype(np.float32), cols, rows


@pytest.mark.parametrize("n", [1, 64, 65, 257])
@pytest.mark.parametrize("nf", [1, 128, 129])
def test_shade_tile_cases(device, nf, n):
    rays, V, F, want = tile_case(nf, n)
    face = want[3]
    colors, atlas, cols, rows = _paint(nf, 5)
    got = _raw_shade(device, face, rays, 1, n, POSE, V, F, colors=colors)
    _same(got, TX.shade_colors(POSE, rays, V, F, face, colors), f"colours F={nf} n={n}")
    got_t = _raw_shade(device, face, rays, 1, n, POSE, V, F, atlas=atlas, layout=(5, cols, rows))
    _same(got_t, TX.shade_texture(POSE, rays, V, F, face, atlas, 5, cols), f"texture F={nf} n={n}")
    miss = face < 0
    assert not got[miss].any() and not got_t[miss].any()
    if (~miss).any():
        assert got[~miss].min() >= colors.min() - 1e-6 and got[~miss].max() <= colors.max() + 1e-6
        assert got_t[~miss].min() >= atlas.min() - 1e-6 and got_t[~miss].max() <= atlas.max() + 1e-6
    # a face index outside [0, F) shades as a miss
    odd = np.where(np.arange(n) % 2 == 0, nf + 3, face).astype(np.int32)
    got_o = _raw_shade(device, odd, rays, 1, n, POSE, V, F, colors=colors)
    assert not got_o[::2].any() and np.array_equal(got_o[1::2], got[1::2])


def test_shade_image_and_render_mesh_color(device):
    """A 17x9 image (partial 8x8 wave tiles) through render_mesh_color in both modes; its first three tensors are
    render_mesh's bytes."""
    from mast3r_slam.tsdf import MeshTexture, render_mesh, render_mesh_color

    _, V, F, _ = tile_case(129, 257)
    h, w = 17, 9
    K = np.array([[0.6 * w, 0, 0.5 * w], [0, 0.6 * w, 0.5 * h], [0, 0, 1.0]])
    d = synthetic.pixel_rays(h, w, K)
    rays = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    want = RC.render(POSE, rays, V, F, NEAR, FAR)
    assert 0 < want[2].sum() < h * w
    colors, atlas, cols, rows = _paint(129, 8)
    mesh = (_dev(device, V, np.float32), _dev(device, F, np.int32))
    z = torch.zeros(atlas.shape[0], atlas.shape[1], dtype=torch.int32, device=device)
    tex = MeshTexture(_dev(device, atlas, np.float32), z, z, 8, cols, rows, 129)
    plain = render_mesh(mesh, POSE, rays=rays, near=NEAR, far=FAR)
    for kw, ref in ((dict(colors=_dev(device, colors, np.float32)), TX.shade_colors(POSE, rays, V, F, want[3], colors)),
                    (dict(texture=tex), TX.shade_texture(POSE, rays, V, F, want[3], atlas, 8, cols))):
        for more in (dict(), dict(skip=False), dict(index=True)):
            out = render_mesh_color(mesh, POSE, rays=rays, near=NEAR, far=FAR, **kw, **more)
            assert len(out) == 4 and out[3].shape == (h, w, 3) and out[2].dtype == torch.bool
            for a, b in zip(out[:3], plain):
                assert a.dtype == b.dtype and torch.equal(a, b)
            _same(out[3].reshape(-1, 3), ref, f"render_mesh_color {list(kw)} {more}")
    four = (mesh[0], torch.zeros_like(mesh[0]), mesh[1], _dev(device, colors, np.float32))
    out = render_mesh_color(four, POSE, colors=True, rays=rays, near=NEAR, far=FAR)
    _same(out[3].reshape(-1, 3), TX.shade_colors(POSE, rays, V, F, want[3], colors), "colors=True")


@functools.lru_cache(maxsize=None)
def _checker():
    return TX.checker_statement()


def test_checker_room_texture_beats_vertex_colours(device):
    """The test that cannot pass without the feature.  room_mesh() carries a world-space checker of period 0.5 m; six
    analytic views at 96x128 are baked at texels=64 and the mesh is shaded from the six poses.  CPU statement (asserted
    in tests/test_mesh_texture_cpu.py): textured 17.272 dB, vertex colours 6.411 dB; the margin is half the gap."""
    from mast3r_slam.tsdf import bake_texture, image_metrics, render_mesh_color

    scene, want_tex, (ref_t, hit_t), (ref_c, hit_c) = _checker()
    mesh = (_dev(device, scene["V"], np.float32), _dev(device, scene["F"], np.int32))
    images = torch.from_numpy(scene["images"]).to(device)
    tex = bake_texture(mesh, images, scene["poses"], scene["K"], texels=TX.CHECKER_TEXELS)
    _check_api(tex, want_tex, "checker room")
    colors = _dev(device, scene["colors"], np.float32)
    views_t = [render_mesh_color(mesh, p, texture=tex, rays=scene["rays"]) for p in scene["poses"]]
    views_c = [render_mesh_color(mesh, p, colors=colors, rays=scene["rays"]) for p in scene["poses"]]
    figs = {}
    for name, views, ref, hit in (("texture", views_t, ref_t, hit_t), ("colors", views_c, ref_c, hit_c)):
        rgb, mask = torch.stack([v[3] for v in views]), torch.stack([v[2] for v in views])
        _same(rgb, ref, f"checker {name} rgb")
        assert np.array_equal(mask.cpu().numpy(), hit)
        m = image_metrics(rgb, images, mask=mask)
        figs[name] = {k: m[k].cpu().numpy() for k in ("psnr", "ssim", "mse")}
        # the GPU figures against the statement's, within image_metrics' own bound
        st = IM.image_metrics(ref, scene["images"], hit)
        fb = IM.figure_bounds(st, 3)
        for k in ("mse", "ssim"):
            assert (np.abs(figs[name][k] - st[k]) <= fb[k]).all(), (name, k, figs[name][k], st[k])
        assert np.allclose(figs[name]["psnr"], st["psnr"], rtol=0, atol=1e-9)
    pt, pc = figs["texture"]["psnr"].mean(), figs["colors"]["psnr"].mean()
    print(f"checker room: PSNR textured {pt:.3f} dB (SSIM {figs['texture']['ssim'].mean():.4f}), vertex colours "
          f"{pc:.3f} dB (SSIM {figs['colors']['ssim'].mean():.4f}); margin asserted {CHECKER_MARGIN_DB} dB")
    assert pt > pc + CHECKER_MARGIN_DB


def test_product_session(device, tmp_path, monkeypatch):
    """The 20-frame colour session of test_color_product_gpu: extract, decimate to a fifth, bake, score the mesh with its
    vertex colours and with its texture beside the TSDF's colour views, write OBJ + MTL + PNG.  Prints; no threshold on
    quality."""
    from PIL import Image

    from mast3r_slam import evaluate
    from mast3r_slam.config import config
    from test_color_product_gpu import _session
    from test_slam_system_gpu import H, W

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    K = synthetic.intrinsics(H, W)
    system = _session(device, True)
    try:
        mesh = system.extract_mesh(colors=True, decimate_ratio=0.2)
        with pytest.raises(ValueError, match="no projection"):
            system.bake_texture(mesh)
        tex = system.bake_texture(mesh, K=K, fallback=True)
        by_color = system.evaluate_mesh_render(mesh, colors=True)
        by_texture = system.evaluate_mesh_render(mesh, texture=tex)
        tsdf = system.evaluate_render()
        with pytest.raises(ValueError, match="exactly one"):
            system.evaluate_mesh_render(mesh)
        paths = evaluate.save_textured_mesh(tmp_path, "map", mesh[0], mesh[2], tex, normals=mesh[1])
        n_kf = len(system.keyframes)
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    for d in (by_color, by_texture):
        assert sorted(d) == sorted(tsdf) and sorted(d["per_view"]) == sorted(tsdf["per_view"])
        assert d["n_views"] == n_kf == len(d["per_view"]["psnr"])
        assert np.isfinite([d[k] for k in ("psnr", "ssim", "psnr_min", "ssim_min", "hit_share", "window_share")]).all()
        assert 0.0 < d["hit_share"] <= 1.0
    owned = tex.owner >= 0
    share = float(((tex.views > 0) & owned).sum()) / float(owned.sum())
    assert share > 0.0 and tex.num_faces == mesh[2].shape[0]
    v, vt, vn, fc, lib, use = TX.parse_obj(paths[0].read_text())
    assert np.array_equal(v.astype(np.float32), mesh[0].cpu().numpy()) and np.array_equal(fc[:, :, 0], mesh[2].cpu().numpy())
    assert len(vt) == 3 * tex.num_faces and len(vn) == len(v) and lib == "map.mtl"
    assert "map_Kd map.png" in paths[1].read_text()
    img = np.asarray(Image.open(paths[2]))
    assert img.shape == tuple(tex.atlas.shape) and img.dtype == np.uint8
    print(f"20-frame colour session, {n_kf} keyframes at {H}x{W}, mesh decimated to {tex.num_faces} faces, atlas "
          f"{tuple(tex.atlas.shape[:2])} at texels=8, {share:.4f} of the owned texels seen: PSNR / SSIM of the training "
          f"views  TSDF {tsdf['psnr']:.3f} / {tsdf['ssim']:.4f} (hit {tsdf['hit_share']:.4f}), mesh with vertex colours "
          f"{by_color['psnr']:.3f} / {by_color['ssim']:.4f} (hit {by_color['hit_share']:.4f}), mesh with texture "
          f"{by_texture['psnr']:.3f} / {by_texture['ssim']:.4f}")
