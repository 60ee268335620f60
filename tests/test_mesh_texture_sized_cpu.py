"""CPU tests of the numpy statement of the sized atlas (tests/texture_sized_numpy.py, DESIGN.md "Mesh textures: sized
atlas"): ownership on every class alone and on mixes, the footprint argument per face of a mixed layout, the class of a
face at and beside a class boundary, clamping, degenerate and out-of-range faces, the stable rank, the packing's figures,
MeshTexture.uv() and the writer's round trip, and the mixed checker room's two PSNR figures."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imgmetrics_numpy as IM  # noqa: E402
import texture_numpy as TX  # noqa: E402
import texture_sized_numpy as TS  # noqa: E402

# Half the gap between the sized and the uniform PSNR of the CPU statement on the mixed checker room (19.038 dB and
# 11.242 dB, asserted below; DESIGN.md "Mesh textures: sized atlas" quotes them), rounded down.
MIXED_MARGIN_DB = 3.8


def layout_of_classes(cls):
    """The statement's layout of faces whose classes are given."""
    cls = np.asarray(cls, np.int32)
    rank, order, counts = TS.stable_rank(cls)
    H, W, bands = TS.sized_layout(counts)
    fc = TS.face_cells(cls, rank, bands)
    return dict(cls=cls, rank=rank, order=order, counts=counts, H=H, W=W, bands=bands, face_cell=fc,
                owner=TS.texel_owner(H, W, bands, order))


def painted_owner(lay):
    """owner built the other way round: every face paints its half of its cell from face_cell; a texel painted twice, or
    outside the atlas, fails."""
    owner = np.full((lay["H"], lay["W"]), -1, np.int32)
    for f, (x0, y0, R, half) in enumerate(lay["face_cell"]):
        i, j = np.meshgrid(np.arange(R + 1), np.arange(R), indexing="xy")
        mine = (i + j > R - 1) == bool(half)
        assert x0 >= 0 and y0 >= 0 and x0 + R + 1 <= lay["W"] and y0 + R <= lay["H"], (f, x0, y0, R)
        cell = owner[y0:y0 + R, x0:x0 + R + 1]
        assert (cell[mine] == -1).all(), f"face {f} paints an owned texel"
        assert mine.sum() == R * (R + 1) // 2
        cell[mine] = f
    return owner


def check_ownership(lay):
    cls, owner = lay["cls"], lay["owner"]
    R = np.array(TS.CLASSES)[cls]
    assert owner.shape == (lay["H"], lay["W"]) and owner.dtype == np.int32
    assert np.array_equal(np.bincount(owner[owner >= 0], minlength=len(cls)), R * (R + 1) // 2)
    assert np.array_equal(owner, painted_owner(lay))                 # one owner each, and none where none is defined
    assert (owner == -1).sum() == owner.size - int((R * (R + 1) // 2).sum())
    li, lj, Rt = TS.texel_local(owner, lay["face_cell"])
    own = owner >= 0
    assert (li[own] >= 0).all() and (lj[own] >= 0).all() and ((li + lj)[own] <= Rt[own] - 1).all()
    assert np.array_equal(Rt[own], R[owner[own]])


@pytest.mark.parametrize("c", range(TS.NC))
@pytest.mark.parametrize("count", [1, 2, 3])
def test_each_class_alone(c, count):
    lay = layout_of_classes([c] * count)
    R = TS.CLASSES[c]
    check_ownership(lay)
    cells = (count + 1) >> 1
    A = cells * R * (R + 1)
    W = max(int(np.ceil(np.sqrt(A))), R + 1)
    assert lay["W"] == W and lay["H"] == -(-cells // (W // (R + 1))) * R
    assert np.array_equal(lay["order"], np.arange(count)) and np.array_equal(lay["rank"], np.arange(count))
    if count == 1:                                                    # a single face: one cell, half of it owned
        assert (lay["H"], lay["W"]) == (R, R + 1)


def test_mixes_with_partial_rows_margins_and_odd_cells():
    rng = np.random.default_rng(3)
    seen = dict(partial_row=0, margin=0, odd=0, bands=0)
    mixes = [[0] * 7 + [2] * 5 + [4] * 3, [8] + [0] * 30, [0, 1, 2, 3, 4, 5, 6], [3] * 9 + [1] * 2,
             list(rng.integers(0, 6, 257)), list(rng.integers(0, 3, 64)), [5, 0, 5, 0, 5]]
    for mix in mixes:
        mix = list(rng.permutation(mix))
        lay = layout_of_classes(mix)
        check_ownership(lay)
        used = 0
        for R, cols, rows, y0, base, count in lay["bands"]:
            if not count:
                assert rows == 0
                continue
            used += 1
            cells = (count + 1) >> 1
            assert cols == lay["W"] // (R + 1) >= 1 and rows == -(-cells // cols)
            seen["partial_row"] += cells % cols != 0
            seen["margin"] += lay["W"] % (R + 1) != 0
            seen["odd"] += count & 1
            band = lay["owner"][y0:y0 + rows * R]
            assert (band[:, cols * (R + 1):] == -1).all()             # the right margin
            assert set(np.unique(band[band >= 0])) == set(np.flatnonzero(np.array(mix) == TS.CLASSES.index(R)))
        seen["bands"] += used > 1
        # bands from the largest class down, order the same
        ys = [b[3] for b in lay["bands"][::-1] if b[5]]
        assert ys == sorted(ys) and ys[0] == 0
        assert np.array_equal(np.array(mix)[lay["order"]], np.sort(mix)[::-1])
    assert all(v > 0 for v in seen.values()), seen


def test_width_from_the_largest_cell():
    """One class-256 face beside a few small ones: ceil(sqrt(A)) = 182 < 257 = R_top + 1."""
    lay = layout_of_classes([0, 0, 12, 0])
    assert lay["W"] == 257 and lay["H"] == 256 + 4
    check_ownership(lay)
    assert (lay["face_cell"][2] == (0, 0, 256, 0)).all() and (lay["face_cell"][3] == (5, 256, 4, 0)).all()


def test_stable_rank_is_the_count_of_earlier_faces_of_the_class():
    rng = np.random.default_rng(0)
    for n in (0, 1, 65, 257, 513):
        cls = rng.integers(0, TS.NC, n).astype(np.int32)
        rank, order, counts = TS.stable_rank(cls)
        assert rank.dtype == order.dtype == counts.dtype == np.int32
        assert np.array_equal(rank, [int((cls[:f] == cls[f]).sum()) for f in range(n)])
        assert np.array_equal(counts, [(cls == c).sum() for c in range(TS.NC)])
        assert np.array_equal(order, np.argsort(-cls.astype(np.int64), kind="stable"))


def test_packing_figures():
    """The figures DESIGN.md quotes, and the Python sized_layout against the statement's."""
    from mast3r_slam.tsdf import atlas_classes, sized_layout

    assert tuple(atlas_classes) == TS.CLASSES and all(b <= 1.5 * a for a, b in zip(TS.CLASSES, TS.CLASSES[1:]))
    rng = np.random.default_rng(1)
    tail = np.bincount(np.minimum(rng.geometric(0.45, 27200) - 1, 7), minlength=TS.NC)
    cases = {"mixed room": [0, 0, 384, 0, 0, 0, 0, 0, 6, 4, 0, 0, 0], "one class": [27200] + [0] * 12,
             "long tail": list(tail), "single": [0, 0, 1] + [0] * 10, "empty": [0] * 13}
    for name, counts in cases.items():
        H, W, bands = TS.sized_layout(counts)
        h, w, b = sized_layout(counts)
        assert (h, w) == (H, W) and np.array_equal(np.array(b, np.int32), bands), name
        own = sum(c * R * (R + 1) // 2 for c, R in zip(counts, TS.CLASSES))
        print(f"{name}: counts {[int(c) for c in counts]} -> {H} x {W}, fill {own / max(H * W, 1):.3f}")
        if name == "mixed room":
            assert (H, W) == (232, 212) and own == 44928
        if name == "one class":
            assert (H, W) == (524, 522) and own / (H * W) > 0.99
        if name == "long tail":
            assert own / (H * W) > 0.85
        if name == "single":
            assert (H, W) == (8, 9)
        if name == "empty":
            assert (H, W) == (0, 0)
    for bad in ([1] * 12, [0] * 12 + [-1]):
        with pytest.raises(ValueError, match="counts"):
            sized_layout(bad)
    with pytest.raises(ValueError, match="int32"):
        sized_layout([0] * 12 + [70000])


@pytest.mark.parametrize("half_first", [False, True])
def test_bilinear_footprint_stays_inside_each_face_of_a_mixed_layout(half_first):
    """texture_numpy's footprint argument with R_f for R: on a barycentric grid of the closed triangle every texel of
    the bilinear footprint is owned by the face, for every face of a layout that mixes seven classes."""
    mix = [0, 3, 1, 1, 6, 2, 0, 4, 2, 2, 5, 0, 3] if not half_first else [2, 2, 2, 0, 0, 1, 1, 1, 4]
    lay = layout_of_classes(mix)
    n = 48
    b, g = (a.reshape(-1) for a in np.meshgrid(np.arange(n + 1) / n, np.arange(n + 1) / n, indexing="ij"))
    keep = b + g <= 1.0 + 1e-15
    b, g = b[keep], g[keep]
    g = np.where(b + g > 1.0, 1.0 - b, g)
    at = np.repeat(lay["owner"][..., None].astype(np.float32), 3, 2)
    for f in range(len(mix)):
        x, y, _ = TS.atlas_xy(lay["face_cell"], np.full(len(b), f), b, g)
        x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
        for dx in (0, 1):
            for dy in (0, 1):
                assert (lay["owner"][y0 + dy, x0 + dx] == f).all(), (f, dx, dy)
        assert (TS.sample_atlas(at, lay["face_cell"], np.full(len(b), f), b, g) == f).all()
    # a texel centre maps back to itself: the forward map of an interior texel's own barycentrics
    li, lj, R = TS.texel_local(lay["owner"], lay["face_cell"])
    yy, xx = np.nonzero(lay["owner"] >= 0)
    s = TX.span(R[yy, xx])
    fx, fy, _ = TS.atlas_xy(lay["face_cell"], lay["owner"][yy, xx], (li[yy, xx] - TX.M) / s, (lj[yy, xx] - TX.M) / s)
    assert np.abs(fx - xx).max() <= 1e-11 and np.abs(fy - yy).max() <= 1e-11


def _edge_face(L):
    """A valid triangle whose longest edge is exactly the f32 L, along x."""
    L = np.float32(L)
    return np.array([[0, 0, 0], [L, 0, 0], [L / 2, min(0.25, float(L) / 4), 0]], np.float32), np.array([[0, 1, 2]], np.int32)


def test_need_at_a_class_boundary_and_one_ulp_either_side():
    for c, R in enumerate(TS.CLASSES):
        L = np.float32(R - 3.5)                                       # density 1: need = ceil(L + 3.5) = R exactly
        up, down = np.nextafter(L, np.float32(1e9)), np.nextafter(L, np.float32(0))
        for edge, want in ((L, c), (down, c), (up, min(c + 1, TS.NC - 1))):
            V, F = _edge_face(edge)
            e, ok = TS.edge_lengths(V, F)
            assert ok.all() and e.max() == np.float64(edge)
            cls, clamped = TS.face_classes(V, F, 1.0, texels=4)
            assert cls[0] == want, (R, edge, cls)
            assert bool(clamped[0]) == (edge == up and c == TS.NC - 1)
        # the same in the doubles: need = R is in, the next double is the next class
        r = np.float64(R)
        got = TS.class_of_need(np.array([r, np.nextafter(r, 1e9), np.nextafter(r, 0.0)]), 0, TS.NC - 1)[0]
        assert list(got) == [c, min(c + 1, TS.NC - 1), c]
    # need, not L, is what is compared: density 2.5, L = 1.8 -> ceil(8.0) = 8; f32(1.8) lies just below, the next f32
    # just above -> 9
    lo32 = np.float32(1.8)
    assert TS.need_of(2.5, 1.8) == 8.0 and TS.need_of(2.5, np.float64(lo32)) == 8.0
    assert TS.need_of(2.5, np.float64(np.nextafter(lo32, np.float32(2)))) == 9.0
    # the floor: the smallest class >= texels
    V, F = _edge_face(0.5)
    for texels, want in ((4, 4), (5, 6), (8, 8), (9, 12), (200, 256), (256, 256)):
        assert TS.CLASSES[TS.face_classes(V, F, 1.0, texels=texels)[0][0]] == want
    for bad in (3, 4.5, 257):
        with pytest.raises(ValueError, match="texels"):
            TS.face_classes(V, F, 1.0, texels=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="density"):
            TS.face_classes(V, F, bad)


def test_clamping_at_max_texels():
    V = np.concatenate([_edge_face(L)[0] for L in (28.5, 28.75, 40.0, 1.0)])
    F = np.arange(12, dtype=np.int32).reshape(4, 3)
    for cap, want_R, want_cl in ((32, [32, 32, 32, 8], [0, 1, 1, 0]), (33, [32, 32, 32, 8], [0, 1, 1, 0]),
                                 (47, [32, 32, 32, 8], [0, 1, 1, 0]), (48, [32, 48, 48, 8], [0, 0, 0, 0]),
                                 (8, [8, 8, 8, 8], [1, 1, 1, 0]), (256, [32, 48, 48, 8], [0, 0, 0, 0])):
        cls, clamped = TS.face_classes(V, F, 1.0, texels=8, max_texels=cap)
        assert [TS.CLASSES[c] for c in cls] == want_R and list(clamped.astype(int)) == want_cl, cap
    for cap in (7, 0, 3.9):
        with pytest.raises(ValueError, match="max_texels"):
            TS.face_classes(V, F, 1.0, texels=8, max_texels=cap)
    with pytest.raises(ValueError, match="max_texels"):
        TS.face_classes(V, F, 1.0, texels=9, max_texels=8)            # the floor class is 12
    # a density that overflows: clamped to the cap
    cls, clamped = TS.face_classes(V, F, 1e308, texels=8)
    assert (cls == TS.NC - 1).all() and clamped.all()


def test_degenerate_and_out_of_range_faces_get_the_floor_class():
    V = np.array([[0, 0, 0], [30, 0, 0], [0, 30, 0], [1, 1, 1], [np.inf, 0, 0], [np.nan, 0, 0]], np.float32)
    F = np.array([[0, 1, 2], [3, 3, 3], [0, 1, 6], [-1, 1, 2], [0, 1, 4], [0, 5, 2], [0, 0, 1]], np.int32)
    cls, clamped = TS.face_classes(V, F, 1.0, texels=6)
    assert [TS.CLASSES[c] for c in cls] == [48, 6, 6, 6, 6, 6, 48] and not clamped.any()
    lay = TS.layout(V, F, 1.0, texels=6)
    check_ownership(dict(lay))
    tp = TS.texel_points(V, F, lay)
    assert not tp["ok"][np.isin(tp["owner"], (2, 3))].any() and tp["ok"][np.isin(tp["owner"], (0, 1, 4, 5, 6))].all()
    out = TS.bake(V, F, np.zeros((0, 2, 2, 3), np.float32), np.zeros((0, 8), np.float32), np.eye(3), 1.0, texels=6,
                  default_color=0.25)
    assert (out["atlas"][out["owner"] >= 0] == 0.25).all() and (out["atlas"][out["owner"] < 0] == 0).all()
    # no faces at all
    lay = TS.layout(V, F[:0], 1.0)
    assert (lay["H"], lay["W"]) == (0, 0) and lay["face_cell"].shape == (0, 4) and not lay["counts"].any()


@functools.lru_cache(maxsize=None)
def _mixed():
    return TS.mixed_statement()


def test_mixed_checker_room_sized_beats_uniform():
    """The test that cannot pass without the feature, on the statement: the checker room with its +x wall cut into
    16 x 12 squares (394 faces), density 9 texels per metre over a floor of 8.  The uniform atlas at the smallest texels
    with no fewer owned texels is the yardstick; the margin is half the gap between the two figures."""
    scene, sized, (rgb_s, hit_s), uni, (rgb_u, hit_u) = _mixed()
    assert len(scene["F"]) == 394 and hit_s.all() and hit_u.all()
    assert list(sized["counts"]) == [0, 0, 384, 0, 0, 0, 0, 0, 6, 4, 0, 0, 0] and not sized["clamped"].any()
    assert (sized["H"], sized["W"]) == (232, 212) and TS.owned(sized) == 44928
    assert uni["texels"] == 15 and TS.owned(uni) == 47280 >= TS.owned(sized) > 394 * 14 * 15 // 2
    check_ownership(dict(sized))
    ps = IM.image_metrics(rgb_s, scene["images"], hit_s)["psnr"].mean()
    pu = IM.image_metrics(rgb_u, scene["images"], hit_u)["psnr"].mean()
    print(f"mixed checker room, 394 faces, 6 views at 96x128: sized atlas {sized['H']}x{sized['W']} with "
          f"{TS.owned(sized)} owned texels PSNR {ps:.3f} dB; uniform atlas at texels={uni['texels']} with "
          f"{TS.owned(uni)} owned texels PSNR {pu:.3f} dB; gap {ps - pu:.3f} dB")
    assert abs(ps - 19.038) < 0.01 and abs(pu - 11.242) < 0.01
    assert ps > pu + MIXED_MARGIN_DB and ps - pu > 2 * MIXED_MARGIN_DB


def _host_texture(tex):
    """A MeshTexture on host tensors from the statement's dict: uv() is torch alone, no kernel."""
    import torch

    from mast3r_slam.tsdf import MeshTexture

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return MeshTexture(t(tex["atlas"]), t(tex["views"]), t(tex["owner"]), 8, 0, 0, tex["num_faces"],
                       face_cell=t(tex["face_cell"]), face_texels=t(tex["face_texels"]),
                       counts=tuple(int(c) for c in tex["counts"]), clamped=int(tex["clamped"].sum()),
                       density=tex["density"])


def test_uv_and_writer_round_trip(tmp_path):
    from PIL import Image

    from mast3r_slam import evaluate

    scene, tex, _, _, _ = _mixed()
    V, F = scene["V"], scene["F"]
    mt = _host_texture(tex)
    assert mt.sized and mt.clamped == 0 and mt.density == 9.0
    want = TS.face_uv(tex["face_cell"])
    got = mt.uv().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    # the corners lie inside the face's own cell, in its own half
    x0, y0, R, half = (tex["face_cell"][:, k][:, None] for k in range(4))
    lx, ly = want[:, :, 0] - x0, want[:, :, 1] - y0
    assert ((lx >= 0.5) & (lx <= R - 0.5) & (ly >= 0.5) & (ly <= R - 1.5)).all()
    assert ((lx + ly <= R - 2.5) == (half == 0)).all()
    obj, mtl, png = evaluate.save_textured_mesh(tmp_path / "out", "room", V, F, mt)
    v, vt, vn, fc, lib, use = TX.parse_obj(obj.read_text())
    assert np.array_equal(v.astype(np.float32), V) and np.array_equal(fc[:, :, 0], F)
    assert np.array_equal(fc[:, :, 1], np.arange(3 * len(F)).reshape(-1, 3)) and lib == "room.mtl"
    H, W = tex["atlas"].shape[:2]
    uv = want.reshape(-1, 2)
    assert np.abs(vt[:, 0] * W - 0.5 - uv[:, 0]).max() <= 1e-5 and np.abs((1.0 - vt[:, 1]) * H - 0.5 - uv[:, 1]).max() <= 1e-5
    img = np.asarray(Image.open(png))
    assert img.shape == (H, W, 3) and np.array_equal(img, np.rint(255.0 * tex["atlas"].astype(np.float64)).astype(np.uint8))
    # the texture read back through the file's vt shows each face its own texels: the centroid lands on an owned texel
    cen = vt.reshape(-1, 3, 2).mean(1)
    cx, cy = np.rint(cen[:, 0] * W - 0.5).astype(int), np.rint((1.0 - cen[:, 1]) * H - 0.5).astype(int)
    assert np.array_equal(tex["owner"][cy, cx], np.arange(len(F)))
    # an empty sized texture
    empty = TS.bake(V, F[:0], scene["images"], scene["poses"], scene["K"], 9.0)
    assert tuple(_host_texture(empty).uv().shape) == (0, 3, 2)
