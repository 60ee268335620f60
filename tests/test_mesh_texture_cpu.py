"""CPU tests of the numpy statement of the mesh textures (tests/texture_numpy.py, DESIGN.md "Mesh textures"): the atlas
layout and its ownership rule, the footprint argument, hand cases of the view rule on the occluder scene of
test_mesh_raycast_cpu, a constant image, the checker room's two PSNR figures, and the OBJ + MTL + PNG writer."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imgmetrics_numpy as IM  # noqa: E402
import texture_numpy as TX  # noqa: E402
from test_mesh_raycast_cpu import IDENT, occluder_scene  # noqa: E402

RS = list(range(4, 17))
FS = [1, 2, 3, 7, 8, 9]


@pytest.mark.parametrize("R", RS)
def test_layout_every_texel_of_a_full_cell_has_one_owner(R):
    for F in FS:
        cols, rows, H, W = TX.layout(F, R)
        cells = (F + 1) >> 1
        assert cols == int(np.ceil(np.sqrt(cells))) and rows == -(-cells // cols) and (H, W) == (rows * R, cols * (R + 1))
        assert (cols - 1) * rows < cells <= cols * rows or rows == 1
        owner, li, lj = TX.texel_owner(F, R)
        assert owner.shape == (H, W) and owner.dtype == np.int32
        # each face owns R (R + 1) / 2 texels, all inside its own cell
        assert np.array_equal(np.bincount(owner[owner >= 0], minlength=F), np.full(F, R * (R + 1) // 2))
        for f in range(F):
            c = f >> 1
            cell = owner[(c // cols) * R:(c // cols + 1) * R, (c % cols) * (R + 1):(c % cols + 1) * (R + 1)]
            assert (cell == f).sum() == R * (R + 1) // 2
            if f + 1 < F or f & 1:                                   # a full cell: no texel without an owner
                assert np.isin(cell, (2 * c, 2 * c + 1)).all()
        # padding cells and the odd face's missing half have none
        assert (owner == -1).sum() == H * W - F * R * (R + 1) // 2
        if F & 1:
            c = F >> 1
            cell = owner[(c // cols) * R:(c // cols + 1) * R, (c % cols) * (R + 1):(c % cols + 1) * (R + 1)]
            i, j = np.meshgrid(np.arange(R + 1), np.arange(R), indexing="xy")
            assert ((cell == -1) == (i + j > R - 1)).all() and ((cell == F - 1) == (i + j <= R - 1)).all()
        # the mirror lands in half 0's ownership
        own = owner >= 0
        assert (li[own] >= 0).all() and (lj[own] >= 0).all() and ((li + lj)[own] <= R - 1).all()


@pytest.mark.parametrize("R", RS)
def test_inverse_and_forward_maps_agree_at_texel_centres(R):
    F = 9
    cols = TX.layout(F, R)[0]
    owner, li, lj = TX.texel_owner(F, R)
    y, x = np.nonzero(owner >= 0)
    f, i, j = owner[y, x], li[y, x], lj[y, x]
    s = TX.span(R)
    beta, gamma = (i - TX.M) / s, (j - TX.M) / s
    inside = (beta >= 0) & (gamma >= 0) & (1.0 - beta - gamma >= 0)
    assert (inside.sum() > 0) == (R >= 5) and (~inside).sum() > 0     # interior texels (i, j >= 1, i + j <= R - 2.5), gutter
    # unclamped: the forward map of the texel's own barycentrics is its centre, exactly (half-integers)
    fx, fy = TX.atlas_xy(f, beta, gamma, R, cols)
    assert np.abs(fx - x).max() <= 1e-12 and np.abs(fy - y).max() <= 1e-12
    # clamped: barycentrics of a point of the face, the interior ones unchanged to a rounding
    al, be, ga = TX.texel_bary(i, j, R)
    assert (al >= 0).all() and (be >= 0).all() and (ga >= 0).all() and np.abs(al + be + ga - 1.0).max() <= 1e-15
    cx, cy = TX.atlas_xy(f, be, ga, R, cols)
    if inside.any():
        assert np.abs(be[inside] - beta[inside]).max() <= 1e-15 and np.abs(ga[inside] - gamma[inside]).max() <= 1e-15
        assert np.abs(cx - x)[inside].max() <= 1e-12 and np.abs(cy - y)[inside].max() <= 1e-12
    # a gutter texel stands for a point of its own face within the gutter's width of it
    assert np.hypot(cx - x, cy - y).max() <= 1.5 * np.sqrt(2.0) + 1e-12


@pytest.mark.parametrize("R", RS)
def test_bilinear_footprint_stays_inside_the_face(R):
    """On a barycentric grid of the closed triangle - corners, edges and the hypotenuse included - each of the four
    texels of the bilinear footprint is owned by the face, for both halves."""
    F = 8
    cols = TX.layout(F, R)[0]
    owner = TX.texel_owner(F, R)[0]
    n = 48
    b, g = (a.reshape(-1) for a in np.meshgrid(np.arange(n + 1) / n, np.arange(n + 1) / n, indexing="ij"))
    keep = b + g <= 1.0 + 1e-15
    b, g = b[keep], g[keep]
    g = np.where(b + g > 1.0, 1.0 - b, g)
    assert ((b == 0) & (g == 0)).any() and ((b == 1) & (g == 0)).any() and ((b == 0) & (g == 1)).any()
    assert (b + g == 1.0).sum() >= n                                   # the hypotenuse
    for f in (0, 1, 4, 7):
        x, y = TX.atlas_xy(np.full(len(b), f), b, g, R, cols)
        x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
        for dx in (0, 1):
            for dy in (0, 1):
                assert (owner[y0 + dy, x0 + dx] == f).all(), (R, f, dx, dy)
        # and sample_atlas's clamp never acts: the face's own index is read back from an atlas that holds the owners
        at = np.repeat(owner[..., None].astype(np.float32), 3, 2)
        assert (TX.sample_atlas(at, np.full(len(b), f), b, g, R, cols) == f).all()


def _wall_scene():
    """The occluder scene reduced to what a hand case needs: the +z wall's two faces (10, 11 of the room) and the quad."""
    V, F, poses, K, hw, _, _ = occluder_scene()
    return V, F, poses, K, hw


def _texel_world(V, F, R):
    tp = TX.texel_points(V, F, R)
    return tp, tp["p"], tp["owner"]


def test_view_rule_on_the_occluder_scene():
    V, F, poses, K, hw = _wall_scene()
    R = 16
    h, w = hw
    img = np.full((1, h, w, 3), 0.25, np.float32)
    out = TX.bake(V, F, img, poses, K, R=R, trace=True)
    tp, p, owner = _texel_world(V, F, R)
    views = out["views"].reshape(-1)
    wall = np.isin(owner, (10, 11))                                  # z = +1.5
    assert wall.sum() == R * (R + 1)
    x, y = p[:, 0], p[:, 1]
    in_view = (x / 1.5 >= -0.8125) & (x / 1.5 < 0.7875) & (y / 1.5 >= -0.6125) & (y / 1.5 < 0.5875)
    shadow = (np.abs(x) < 0.5) & (np.abs(y) < 0.5)
    edge = (np.abs(np.abs(x) - 0.5) < 1e-9) | (np.abs(np.abs(y) - 0.5) < 1e-9)
    sel = wall & ~edge
    # the quad's shadow: texels of the wall behind it take no view, those beside it in the frustum take one
    assert np.array_equal(views[sel] == 1, (in_view & ~shadow)[sel])
    assert (views[sel & shadow] == 0).all() and (sel & shadow).sum() > 0 and (views[sel] == 1).sum() > 0
    # the quad itself (faces 12, 13; its normal (0, 0, 1) points away from the camera at the origin): a back face
    quad = np.isin(owner, (12, 13))
    assert (views[quad] == 0).all() and (out["cos"][0][quad] == 0).all()
    # the wall z = -1.5 lies behind the camera
    assert (views[np.isin(owner, (8, 9))] == 0).all()
    # a back-facing view of the wall: a camera outside the room looking back at it
    behind = np.array([0, 0, 4.0, 0, 1, 0, 0, 1], np.float32)
    back = TX.bake(V, F, img, behind[None], K, R=R, trace=True)
    assert (back["views"].reshape(-1)[wall] == 0).all() and (back["cos"][0][wall] == 0).all()
    # cos_min: the wall's cos is 1.5 / r
    r = np.sqrt((p * p).sum(1))
    for cm in (0.1, 0.9, 0.97):
        got = TX.bake(V, F, img, poses, K, R=R, cos_min=cm)["views"].reshape(-1)
        assert np.array_equal(got[sel] == 1, (in_view & ~shadow & (1.5 / r >= cm))[sel])
    assert (TX.bake(V, F, img, poses, K, R=R, cos_min=0.9)["views"].reshape(-1)[sel] == 1).sum() < (views[sel] == 1).sum()
    # near / far inclusive: r of one seen texel exactly, and one unit in the last place inside it
    k = np.flatnonzero(sel & (views == 1))[0]
    rk = out["r"][0][k]
    assert rk > 0
    for kw, want in ((dict(near=rk), 1), (dict(far=rk), 1), (dict(near=np.nextafter(rk, 9.0)), 0),
                     (dict(far=np.nextafter(rk, 0.0)), 0)):
        assert TX.bake(V, F, img, poses, K, R=R, **kw)["views"].reshape(-1)[k] == want, kw
    # tol: a plane 5 mm in front of the wall's texels hides them at tol < 5 mm only
    V2 = np.concatenate([V, np.array([[-3, -2, 1.495], [3, -2, 1.495], [3, 2, 1.495], [-3, 2, 1.495]], np.float32)])
    F2 = np.concatenate([F[:12], np.array([[12, 14, 13], [12, 15, 14]], np.int32)])    # vertices 12..15: the plane
    for tol, seen in ((0.01, True), (0.001, False)):
        got = TX.bake(V2, F2, img, poses, K, R=R, tol=tol)["views"].reshape(-1)
        far_from_rim = sel & in_view & (np.abs(x) < 2.9)
        assert (got[far_from_rim] == 1).all() == seen and (got[far_from_rim] == 0).all() == (not seen)


def test_image_border_is_half_open():
    """u = -0.5 exactly is in, u = w - 0.5 exactly is out: one triangle whose texel points project there."""
    K = np.array([[32.0, 0, 32.0], [0, 32.0, 24.0], [0, 0, 1.0]])
    hw = (48, 64)
    R = 4                                                             # s = 0.5: texel (0, 0) is corner a itself
    for u_edge, want in ((-0.5, 1), (63.5, 0)):
        xa = (u_edge - 32.0) / 32.0                                   # at z = 1: a multiple of 2^-6, exact in f32
        V = np.array([[xa, 0, 1], [xa, 0.25, 1], [xa + (0.25 if want else -0.25), 0, 1]], np.float32)
        assert float(V[0, 0]) == xa
        F = np.array([[0, 1, 2] if want else [0, 2, 1]], np.int32)
        tp = TX.texel_points(V, F, R)
        k = np.flatnonzero((tp["owner"] == 0) & (tp["alpha"] == 1.0))
        assert len(k) >= 1 and (tp["p"][k] == V[0].astype(np.float64)).all()
        n = tp["n"][k[0]]
        assert n[2] < 0                                               # faces the camera at the origin
        out = TX.bake(V, F, np.zeros((1,) + hw + (3,), np.float32), IDENT[None], K, R=R, trace=True)
        assert out["uv"][0][k[0], 0] == (u_edge if want else 0.0)
        assert (out["views"].reshape(-1)[k] == want).all()


def test_constant_image_gives_the_constant():
    V, F, poses, K, hw = _wall_scene()
    two = np.stack([poses[0], np.array([0.5, 0.2, -0.3, 0, 0, 0, 1, 1.7], np.float32)])
    for c in (0.25, 0.1, 0.7):
        img = np.full((2,) + hw + (3,), c, np.float32)
        out = TX.bake(V, F, img, two, K, R=16, default_color=0.0)
        seen = out["views"] > 0
        assert seen.sum() > 20 and (out["views"] == 2).any()
        err = np.abs(out["atlas"][seen].astype(np.float64) - np.float64(np.float32(c)))
        assert err.max() <= np.spacing(np.float32(c))                 # 1 ulp of f32
        assert (out["atlas"][(out["owner"] >= 0) & ~seen] == 0.0).all() and (out["atlas"][out["owner"] < 0] == 0).all()
    # no view: everything comes from the fallback
    col = np.random.default_rng(0).uniform(0, 1, (len(V), 3)).astype(np.float32)
    out = TX.bake(V, F, np.zeros((0, 2, 2, 3), np.float32), np.zeros((0, 8), np.float32), K, R=5, fallback=col)
    assert not out["views"].any()
    tp = TX.texel_points(V, F, 5)
    k = np.flatnonzero((tp["owner"] == 3) & (tp["beta"] == 1.0))[0]
    assert np.array_equal(out["atlas"].reshape(-1, 3)[k], col[F[3, 1]])
    own = out["owner"] >= 0
    assert out["atlas"][own].min() >= col.min() and out["atlas"][own].max() <= col.max()


@functools.lru_cache(maxsize=None)
def _checker():
    return TX.checker_statement()


def test_checker_room_texture_beats_vertex_colours():
    """The two figures DESIGN.md "Mesh textures" quotes, and the margin of the GPU test: half their gap."""
    scene, tex, (rgb_t, hit_t), (rgb_c, hit_c) = _checker()
    assert hit_t.all() and hit_c.all()
    pt = IM.image_metrics(rgb_t, scene["images"], hit_t)["psnr"].mean()
    pc = IM.image_metrics(rgb_c, scene["images"], hit_c)["psnr"].mean()
    print(f"checker room, 6 views at 96x128, texels=64: PSNR textured {pt:.3f} dB, vertex colours {pc:.3f} dB, gap "
          f"{pt - pc:.3f} dB; seen texels {(tex['views'] > 0).sum()} of {(tex['owner'] >= 0).sum()}")
    assert abs(pt - 17.272) < 0.01 and abs(pc - 6.411) < 0.01
    assert pt - pc > 2 * 5.4


class _HostTexture:
    """What save_textured_mesh reads of a MeshTexture, from the statement's dict."""

    def __init__(self, tex):
        self.atlas, self.texels, self.num_faces = tex["atlas"], tex["texels"], tex["num_faces"]

    def uv(self):
        return TX.face_uv(self.num_faces, self.texels).astype(np.float32)


@pytest.mark.parametrize("with_normals", [False, True])
def test_writer_round_trip(tmp_path, with_normals):
    from PIL import Image

    from mast3r_slam import evaluate

    scene, tex, _, _ = _checker()
    V, F = scene["V"], scene["F"]
    nrm = (V / np.linalg.norm(V, axis=1, keepdims=True)).astype(np.float32) if with_normals else None
    obj, mtl, png = evaluate.save_textured_mesh(tmp_path / "out", "room", V, F, _HostTexture(tex), normals=nrm)
    assert [p.name for p in (obj, mtl, png)] == ["room.obj", "room.mtl", "room.png"]
    v, vt, vn, fc, lib, use = TX.parse_obj(obj.read_text())
    assert np.array_equal(v.astype(np.float32), V)                      # %.9g round-trips f32
    assert np.array_equal(fc[:, :, 0], F) and np.array_equal(fc[:, :, 1], np.arange(3 * len(F)).reshape(-1, 3))
    assert fc.shape[2] == (3 if with_normals else 2) and len(vn) == (len(V) if with_normals else 0)
    if with_normals:
        assert np.array_equal(fc[:, :, 2], F) and np.array_equal(vn.astype(np.float32), nrm)
    H, W = tex["atlas"].shape[:2]
    uv = TX.face_uv(len(F), tex["texels"]).reshape(-1, 2)
    assert np.abs(vt[:, 0] * W - 0.5 - uv[:, 0]).max() <= 1e-6 and np.abs((1.0 - vt[:, 1]) * H - 0.5 - uv[:, 1]).max() <= 1e-6
    assert lib == "room.mtl" and use == "atlas"
    text = mtl.read_text()
    assert "newmtl atlas" in text and "map_Kd room.png" in text.splitlines()
    img = np.asarray(Image.open(png))
    assert img.dtype == np.uint8 and np.array_equal(img, np.rint(255.0 * tex["atlas"].astype(np.float64)).astype(np.uint8))
    with pytest.raises(ValueError, match="faces"):
        evaluate.save_textured_mesh(tmp_path, "bad", V, F[:5], _HostTexture(tex))


def test_mesh_texture_uv_matches_the_statement():
    """MeshTexture.uv() on host tensors (torch alone, no kernel) against face_uv, for even and odd F."""
    import torch

    from mast3r_slam.tsdf.mesh_texture import MeshTexture, atlas_layout

    for F, R in ((1, 4), (7, 8), (12, 64), (9, 5)):
        cols, rows, H, W = atlas_layout(F, R)
        assert (cols, rows, H, W) == TX.layout(F, R)
        t = MeshTexture(torch.zeros(H, W, 3), torch.zeros(H, W, dtype=torch.int32), torch.zeros(H, W, dtype=torch.int32),
                        R, cols, rows, F)
        assert np.array_equal(t.uv().numpy(), TX.face_uv(F, R).astype(np.float32))
    for bad in (3, 0, -1, 4.5):
        with pytest.raises(ValueError, match="texels"):
            atlas_layout(4, bad)
    with pytest.raises(ValueError, match="int32"):
        atlas_layout(1 << 29, 64)
