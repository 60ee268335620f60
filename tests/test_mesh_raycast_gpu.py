"""GPU tests (-m gpu) of the mesh ray caster (csrc/mesh_raycast.hip, DESIGN.md "Mesh ray casting") and of
mast3r_slam.tsdf.render_mesh / observed_points / compare_meshes(observed=...) and SlamSystem.evaluate_mesh(observed=True)
/ evaluate_depth: parity with the numpy statement (tests/raycast_numpy.py) at the kernel's tile edges - face, hit and t64
exactly, range and normal as its f32 roundings - culled against plain scan byte for byte, the room against
synthetic.ray_box_depth, guarded buffers, waves without a casting ray, invalid faces, refused arguments, the observed
mask, and the product path."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from mast3r_slam import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M  # noqa: E402
import meshdist_numpy as D  # noqa: E402
import raycast_numpy as R  # noqa: E402
from test_mesh_raycast_cpu import occluder_scene, t_bound  # noqa: E402
from mesh_support import (CAST_KEYS, FAR, NEAR, G, T, VS, _build, _dev, _host, _indexed_cast,  # noqa: E402
                          _raw_cast, _same_bytes)

pytestmark = pytest.mark.gpu

POSE = np.concatenate([[0.1, -0.2, 0.05], synthetic.quat_from_rotvec(np.array([0.3, 0.5, -0.2])),
                       [1.7]]).astype(np.float32)
BACK = np.array([0.2, 0.1, -0.1, 0, 1, 0, 0, 1], np.float32)       # a half turn about y: the camera looks along -z


def _parity(got, want):
    """face, hit and t64 exactly; range and normal equal the statement's f32 roundings."""
    for k, w in zip(CAST_KEYS, want):
        if k in got:
            assert got[k].dtype == w.dtype and got[k].shape == w.shape, k
            assert got[k].tobytes() == w.tobytes(), (k, int((got[k] != w).sum()))


@functools.lru_cache(maxsize=None)
def tile_mesh(nf):
    """Random f32 triangles about the camera in the order of their x, so that the tiles' boxes differ; from 129 faces on
    the last face coincides with the first (a tie across tiles: the lowest index wins)."""
    rng = np.random.default_rng(7000 + nf)
    centre = rng.uniform(-2.0, 2.0, (nf, 3))
    centre = centre[np.argsort(centre[:, 0])]
    tri = (centre[:, None, :] + rng.uniform(-0.7, 0.7, (nf, 3, 3))).astype(np.float32)
    if nf > T:
        tri[nf - 1] = tri[0]
    return tri.reshape(-1, 3), np.arange(3 * nf, dtype=np.int32).reshape(nf, 3)


@functools.lru_cache(maxsize=None)
def tile_case(nf, n):
    """Rays in every direction (the lanes of a wave differ in their depth axis), one of them zero, and the numpy answer.
    Computed once per shape."""
    V, F = tile_mesh(nf)
    rng = np.random.default_rng(100 * nf + n)
    rays = rng.normal(size=(n, 3))
    rays = (rays / np.linalg.norm(rays, axis=1, keepdims=True)).astype(np.float32)
    if n > 2:
        rays[n // 2] = 0.0
    return rays, V, F, R.render(POSE, rays, V, F, NEAR, FAR)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("nf", [1, 127, 128, 129, 257])
def test_tile_edges(device, nf, n):
    rays, V, F, want = tile_case(nf, n)
    plain = _raw_cast(device, rays, 1, n, POSE, V, F, 0)
    culled = _raw_cast(device, rays, 1, n, POSE, V, F, 1)
    _parity(plain, want)
    _same_bytes(plain, culled)
    _same_bytes(culled, _raw_cast(device, rays, 1, n, POSE, V, F, 1))           # run to run
    if n > 2:
        assert plain["hit"][n // 2] == 0 and plain["face"][n // 2] == -1          # the zero direction
    if nf >= T and n >= 63:
        assert 0 < plain["hit"].sum()
    if nf > T:
        assert (plain["face"] != nf - 1).all() and (want[3] != nf - 1).all()     # the coincident pair: the first wins
    print(f"F={nf} n={n}: {int(plain['hit'].sum())} hits")


@pytest.mark.parametrize("hw,pose", [((16, 16), POSE), ((17, 9), BACK)])
def test_image_tiles(device, hw, pose):
    """Partial 8x8 wave tiles, pinhole rays (one depth axis per wave: the kernel's constant-permutation path), through
    the C entry point and through render_mesh with K and with rays."""
    from mast3r_slam.tsdf import render_mesh

    h, w = hw
    V, F = tile_mesh(257)
    K = np.array([[0.6 * w, 0, 0.5 * w], [0, 0.6 * w, 0.5 * h], [0, 0, 1.0]])
    d = synthetic.pixel_rays(h, w, K)
    rays = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    want = R.render(pose, rays, V, F, NEAR, FAR)
    plain = _raw_cast(device, rays, h, w, pose, V, F, 0)
    _parity(plain, want)
    _same_bytes(plain, _raw_cast(device, rays, h, w, pose, V, F, 1))
    assert 0 < plain["hit"].sum() < h * w
    mesh = (_dev(device, V, np.float32), _dev(device, F, np.int32))
    for kw in (dict(K=K, hw=hw), dict(rays=rays), dict(rays=_dev(device, rays, np.float32), skip=False)):
        rng, nrm, hit, face = render_mesh(mesh, pose, near=NEAR, far=FAR, return_face=True, **kw)
        assert rng.shape == (h, w) and nrm.shape == (h, w, 3) and hit.dtype == torch.bool and face.dtype == torch.int32
        _parity(dict(range=rng.cpu().numpy().reshape(-1), normal=nrm.cpu().numpy().reshape(-1, 3),
                     face=face.cpu().numpy().reshape(-1)), want)
        assert np.array_equal(hit.cpu().numpy().reshape(-1), want[2].astype(bool))
    z = torch.zeros_like(mesh[0])
    view = render_mesh((mesh[0], z, mesh[1], z), pose, rays=rays, near=NEAR, far=FAR)      # an extract_mesh tuple
    assert len(view) == 3 and np.array_equal(view[0].cpu().numpy().reshape(-1), want[0])


def test_image_and_list_share_one_pixel_map(device):
    """The pixel-to-thread map has two forms (16x16 tiles; h = 1: a list of 256 per block) and the cast and the shade
    each use it: a 17x9 view - two blocks of tiles, partial waves - of 130 faces - two face tiles - cast as an image and
    as the list of the same 153 rays gives the same bytes, and so does the colour view."""
    from mast3r_slam.tsdf import render_mesh_color

    h, w = 17, 9
    V, F = tile_mesh(130)
    K = np.array([[0.6 * w, 0, 0.5 * w], [0, 0.6 * w, 0.5 * h], [0, 0, 1.0]])
    d = synthetic.pixel_rays(h, w, K)
    rays = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    for skip in (0, 1):
        image = _raw_cast(device, rays, h, w, BACK, V, F, skip)
        _same_bytes(image, _raw_cast(device, rays, 1, h * w, BACK, V, F, skip))
    assert 0 < image["hit"].sum() < h * w
    _parity(image, R.render(BACK, rays, V, F, NEAR, FAR))
    mesh = (_dev(device, V, np.float32), _dev(device, F, np.int32))
    colors = _dev(device, np.random.default_rng(5).uniform(0.0, 1.0, (len(V), 3)), np.float32)
    as_image = render_mesh_color(mesh, BACK, colors=colors, rays=rays, near=NEAR, far=FAR)
    as_list = render_mesh_color(mesh, BACK, colors=colors, rays=rays.reshape(1, h * w, 3), near=NEAR, far=FAR)
    for a, b in zip(_host(as_image), _host(as_list)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert np.array_equal(as_image[2].cpu().numpy().reshape(-1), image["hit"].astype(bool))
    assert (as_image[3][as_image[2]] > 0.0).any() and not as_image[3][~as_image[2]].any()


def _both(device, rays, h, w, pose, V, F, **kw):
    plain = _raw_cast(device, rays, h, w, pose, V, F, 0, **kw)
    _same_bytes(plain, _raw_cast(device, rays, h, w, pose, V, F, 1, **kw))
    return plain


def test_sphere_culled_equals_plain(device):
    """A marching-cubes sphere (faces in cube-key order) seen from its centre and from outside."""
    from mast3r_slam.tsdf import mesh_from_voxels

    c = np.zeros(3)
    k, v, w = M.sample_sdf(M.sphere_sdf(c, 0.2), c - 0.2, c + 0.2, VS, 3 * VS)
    V, _, F = _host(mesh_from_voxels(k, v, w, VS, 0.5, device=device))
    assert len(F) > 4 * T
    h, wd = 40, 40
    K = np.array([[40.0, 0, 20.0], [0, 40.0, 20.0], [0, 0, 1.0]])
    d = synthetic.pixel_rays(h, wd, K)
    rays = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    inside = np.array([0.01, -0.02, 0.015, 0, 0, 0, 1, 1], np.float32)
    outside = np.concatenate([[0.05, 0.03, -0.9], synthetic.quat_from_rotvec(np.array([0.02, -0.05, 0.3])),
                              [1.0]]).astype(np.float32)
    a = _both(device, rays, h, wd, inside, V, F, near=0.0)
    assert a["hit"].all()                                                 # watertight: no ray leaves the sphere
    assert (np.abs(a["t64"] - 0.2) <= 0.03 + VS).all()
    b = _both(device, rays, h, wd, outside, V, F, near=0.0)
    assert 0.05 * h * wd < b["hit"].sum() < 0.5 * h * wd
    assert (np.abs(b["t64"][b["hit"] == 1] - 0.8) <= 0.2).all()
    sel = np.r_[0:32, 800:832]                                            # the statement on 64 of the rays
    _parity({k: x[sel] for k, x in a.items()}, R.render(inside, rays.reshape(-1, 3)[sel], V, F, 0.0, FAR))
    _parity({k: x[sel] for k, x in b.items()}, R.render(outside, rays.reshape(-1, 3)[sel], V, F, 0.0, FAR))


def test_slivers_and_one_tile(device):
    """Needle triangles (the third corner within 1e-7 of the line through the other two), and a mesh of one tile."""
    rays, V, F, _ = tile_case(257, 257)
    rng = np.random.default_rng(77)
    tri = V.reshape(-1, 3, 3).astype(np.float64)
    t = rng.uniform(-0.5, 1.5, (len(tri), 1))
    tri[:, 2] = tri[:, 0] + t * (tri[:, 1] - tri[:, 0]) + rng.uniform(-1e-7, 1e-7, (len(tri), 3))
    needles = tri.reshape(-1, 3).astype(np.float32)
    assert D.triangles(needles, F)[3].sum() > 0.9 * len(F)
    # slivers among ordinary faces: the ordinary ones are hit, the needles almost never
    mixed = np.concatenate([V, needles])
    Fm = np.concatenate([F[:100], F + len(V), F[100:]]).astype(np.int32)
    _parity(_both(device, rays, 1, len(rays), POSE, mixed, Fm), R.render(POSE, rays, mixed, Fm, NEAR, FAR))
    _parity(_both(device, rays, 1, len(rays), POSE, needles, F), R.render(POSE, rays, needles, F, NEAR, FAR))
    V1, F1 = tile_mesh(100)
    got = _both(device, rays, 1, len(rays), POSE, V1, F1)
    _parity(got, R.render(POSE, rays, V1, F1, NEAR, FAR))
    assert got["hit"].sum() > 0


def test_room_against_ray_box_depth(device):
    """range against synthetic.ray_box_depth in f64 on the same f32 pose and unit rays.  The bound: half an f32 unit of
    the range, 2^-24 t, plus the f64 term t_bound derived in test_mesh_raycast_cpu.py (its L = 4.5 m covers the unit
    rays' |d| >= 1 - 2^-23).  Every pixel hits."""
    from mast3r_slam.tsdf import render_mesh

    V, F = synthetic.room_mesh()
    mesh = (_dev(device, V, np.float32), _dev(device, F, np.int32))
    h, w = 48, 64
    K = synthetic.intrinsics(h, w)
    d = synthetic.pixel_rays(h, w, K.astype(np.float64))
    rays = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    worst = 0.0
    for k in (0, 100, 333, 999):
        pose = synthetic.camera_pose(k).astype(np.float32)
        rng, nrm, hit = render_mesh(mesh, pose, K=K, hw=(h, w), near=NEAR, far=FAR)
        o, dw, _ = R.directions(pose, rays)
        want = synthetic.ray_box_depth(o, dw)
        got = rng.cpu().numpy().reshape(-1).astype(np.float64)
        assert hit.all()
        err = np.abs(got - want)
        assert (err <= 2.0 ** -24 * want + t_bound(o, dw, want)).all()
        worst = max(worst, float((err / want).max()))
        assert ((nrm.cpu().numpy().reshape(-1, 3).astype(np.float64) * dw).sum(1) < 0.0).all()
        _parity(dict(range=rng.cpu().numpy().reshape(-1)), R.render(pose, rays, V, F, NEAR, FAR))
    print(f"room 48x64: largest relative difference of range to ray_box_depth {worst:.3g}")


def test_guards_null_outputs_invalid_faces_and_arguments(device):
    import mslam_hip as _m
    from mast3r_slam.tsdf import observed_points, render_mesh

    rays, V, F, want = tile_case(129, 257)
    for n in (1, 257):
        for skip in (0, 1):
            got = _raw_cast(device, rays[:n], 1, n, POSE, V, F, skip, guarded=True)
            _parity(got, [w[:n] for w in want])
            part = _raw_cast(device, rays[:n], 1, n, POSE, V, F, skip, face=False, t64=False, guarded=True)
            assert sorted(part) == ["hit", "normal", "range"]
            _parity(part, [w[:n] for w in want])
    img = _raw_cast(device, np.tile(rays[:153], (1, 1)), 17, 9, POSE, V, F, 1, guarded=True)
    _parity(img, R.render(POSE, rays[:153], V, F, NEAR, FAR))
    # invalid faces are skipped by the kernel itself
    line = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32)
    V2 = np.concatenate([V, line])
    nv = len(V2)
    bad = np.array([[0, 0, 1], [3, 3, 3], [nv - 3, nv - 2, nv - 1], [0, 1, nv], [-1, 2, 3]], np.int32)
    mixed = np.concatenate([bad[:2], F[:T - 3], bad[2:], F[T - 3:], bad[:1]]).astype(np.int32)
    w2 = R.render(POSE, rays, V2, mixed, NEAR, FAR)
    valid = D.triangles(V2, mixed)[3]
    for skip in (0, 1):
        got = _raw_cast(device, rays, 1, len(rays), POSE, V2, mixed, skip)
        _parity(got, w2)
        assert valid[got["face"][got["hit"] == 1]].all()
        for faces in (bad, np.zeros((0, 3), np.int32)):
            got = _raw_cast(device, rays, 1, len(rays), POSE, V2, faces, skip)
            assert not got["hit"].any() and (got["face"] == -1).all() and np.isposinf(got["t64"]).all()
            assert not got["range"].any() and not got["normal"].any()
    # refused arguments
    r, p = _dev(device, rays, np.float32), _dev(device, POSE, np.float32)
    v, f = _dev(device, V2, np.float32), _dev(device, mixed, np.int32)
    ok_f = _dev(device, F, np.int32)
    with pytest.raises(ValueError, match=r"outside \[0, "):
        render_mesh((v, f), POSE, rays=rays[None])
    assert render_mesh((v, f), POSE, rays=rays[None], validate=False)[2].any()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render_mesh((v.cpu(), ok_f), POSE, rays=rays[None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render_mesh((v, ok_f.cpu()), POSE, rays=rays[None])
    with pytest.raises(RuntimeError, match="dtype"):
        render_mesh((v.double(), ok_f), POSE, rays=rays[None])
    with pytest.raises(RuntimeError, match="dtype"):
        render_mesh((v, ok_f.long()), POSE, rays=rays[None])
    with pytest.raises(ValueError, match="give either rays"):
        render_mesh((v, ok_f), POSE)
    with pytest.raises(ValueError, match="8 values"):
        render_mesh((v, ok_f), POSE[:7], rays=rays[None])
    with pytest.raises(ValueError, match="far must be greater"):
        render_mesh((v, ok_f), POSE, rays=rays[None], near=1.0, far=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        observed_points(r.cpu(), (v, ok_f), POSE[None], np.eye(3), (4, 4))
    with pytest.raises(RuntimeError, match="dtype"):
        observed_points(r.double(), (v, ok_f), POSE[None], np.eye(3), (4, 4))
    L = _m.lib()
    n, nf = len(rays), len(mixed)
    out = [torch.empty(n * k, dtype=dt, device=device)
           for k, dt in ((1, torch.float32), (3, torch.float32), (1, torch.uint8))]
    wb = int(L.mslam_mesh_raycast_workspace_bytes(nf))
    ws = torch.empty(wb, dtype=torch.uint8, device=device)
    call = lambda skip, ws_ptr, ws_bytes, near=NEAR, far=FAR, h=1: L.mslam_mesh_raycast(
        _m.ptr(r), h, n, _m.ptr(p), _m.ptr(v), _m.ptr(f), nf, nv, near, far, skip, ws_ptr, ws_bytes, _m.ptr(out[0]),
        _m.ptr(out[1]), _m.ptr(out[2]), 0, 0, 0)
    assert L.mslam_mesh_raycast_boxes(_m.ptr(v), _m.ptr(f), nf, nv, _m.ptr(ws), wb - 1, 0) != 0     # a short workspace
    assert L.mslam_mesh_raycast_boxes(_m.ptr(v), _m.ptr(f), nf, nv, _m.ptr(ws), wb, 0) == 0
    assert call(1, 0, 0) != 0 and call(1, _m.ptr(ws), wb - 1) != 0
    assert "needed" in L.mslam_last_error().decode()
    assert call(1, _m.ptr(ws), wb, near=2.0, far=1.0) != 0 and call(1, _m.ptr(ws), wb, near=float("nan")) != 0
    assert call(1, _m.ptr(ws), wb, h=-1) != 0
    assert call(1, _m.ptr(ws), wb) == 0 and call(0, 0, 0) == 0
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def dead_wave_case(nf, dead):
    """257 rays in every direction whose first `dead` (a wave, or the whole first block) have a zero or a non-finite
    direction, the same list with copies of its casting rays in their place, and the numpy answer for the first."""
    V, F = tile_mesh(nf)
    rng = np.random.default_rng(300 * nf + dead)
    filled = rng.normal(size=(257, 3))
    filled = (filled / np.linalg.norm(filled, axis=1, keepdims=True)).astype(np.float32)
    filled[:dead] = filled[dead + np.arange(dead) % (257 - dead)]
    rays = filled.copy()
    rays[:dead] = np.array([[0, 0, 0], [np.inf, 0, 0], [np.nan, 1, 0], [0, -np.inf, 0]], np.float32)[np.arange(dead) % 4]
    with np.errstate(invalid="ignore"):
        want = R.render(POSE, rays, V, F, NEAR, FAR)
    return rays, filled, V, F, want


_INDEXES = {}


@pytest.mark.parametrize("dead", [64, 256])
@pytest.mark.parametrize("nf", [T + 1, T * G + T + 1])
def test_waves_without_a_casting_ray(device, nf, dead):
    """The one place where the tile loops of rc_kernel and md_scan (csrc/mesh_tri.h) vote differently: rc_kernel lets a
    wave none of whose rays casts skip every tile, culled or not.  Whatever the vote, its rays miss, the others'
    answers are the statement's, a wholly dead wave counts every tile, and - a wave's count depends on its own rays
    alone - the waves behind count what they count when casting rays stand in front of them."""
    rays, filled, V, F, want = dead_wave_case(nf, dead)
    n, first, waves, ntiles = len(rays), dead // 64, (len(rays) + 63) // 64, (nf + T - 1) // T

    def check(got):
        _parity(got, want)
        assert not got["hit"][:dead].any() and (got["face"][:dead] == -1).all() and np.isposinf(got["t64"][:dead]).all()
        assert not got["range"][:dead].any() and not got["normal"][:dead].any()

    for skip in (0, 1):
        check(_raw_cast(device, rays, 1, n, POSE, V, F, skip, guarded=True))
    if nf not in _INDEXES:
        _INDEXES[nf] = _build(device, V, F)
    for levels in (1, 2):
        got, counts = _indexed_cast(device, _INDEXES[nf], rays, 1, n, POSE, levels, NEAR, FAR)       # guards checked
        check(got)
        other, behind = _indexed_cast(device, _INDEXES[nf], filled, 1, n, POSE, levels, NEAR, FAR)
        assert counts.dtype == torch.int32 and torch.equal(counts[first:waves], behind[first:waves])
        assert (counts[:first] == ntiles).all()
        _same_bytes({k: x[dead:] for k, x in got.items()}, {k: x[dead:] for k, x in other.items()})
        print(f"F={nf} dead={dead} levels={levels}: tiles skipped per wave {counts[:waves].tolist()} of {ntiles}")


# ----------------------------------------------------------------------------------------------------------------------
# observed points and the metrics over them
# ----------------------------------------------------------------------------------------------------------------------
def test_observed_points_match_numpy(device):
    from mast3r_slam.tsdf import observed_points, sample_mesh

    V, F, poses, K, hw, pts, want = occluder_scene()
    mesh = (_dev(device, V, np.float32), _dev(device, F, np.int32))
    two = np.stack([poses[0], np.array([0, 0, 1.4, 0, 1, 0, 0, 1], np.float32)])
    for ps in (poses, two):
        got = observed_points(_dev(device, pts, np.float32), mesh, ps, K, hw)
        assert got.dtype == torch.bool and got.shape == (len(pts),) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), R.observed(pts, V, F, ps, K, hw))
    assert np.array_equal(observed_points(_dev(device, pts, np.float32), mesh, poses, K, hw).cpu().numpy(), want)
    # the room with three poses, samples of its surface; scaled poses among them
    Vr, Fr = synthetic.room_mesh()
    room = (_dev(device, Vr, np.float32), _dev(device, Fr, np.int32))
    P = sample_mesh(*room, 6000, seed=3)[0]
    cams = np.stack([synthetic.camera_pose(k) for k in (0, 160, 480, 700, 905)]).astype(np.float32)
    cams[1, 7] = 2.5
    K2, hw2 = synthetic.intrinsics(48, 64), (48, 64)
    w3 = R.observed(P.cpu().numpy(), Vr, Fr, cams[:3], K2, hw2)
    got = observed_points(P, room, cams[:3], K2, hw2)
    assert np.array_equal(got.cpu().numpy(), w3) and 0.05 < w3.mean() < 0.9
    # independent of compaction, of culling and of the order of the points
    w5 = R.observed(P.cpu().numpy(), Vr, Fr, cams, K2, hw2, tol=0.02, far=4.0)
    perm = torch.randperm(len(P), generator=torch.Generator().manual_seed(1)).to(device)
    for kw in (dict(), dict(compact_every=0), dict(compact_every=1), dict(compact_every=2, skip=False)):
        assert np.array_equal(observed_points(P, room, cams, K2, hw2, tol=0.02, far=4.0, **kw).cpu().numpy(), w5)
    assert np.array_equal(observed_points(P[perm], room, list(torch.from_numpy(cams)), K2, hw2, tol=0.02,
                                          far=4.0).cpu().numpy(), w5[perm.cpu().numpy()])
    assert w5.sum() >= 1 and not observed_points(P, room, cams[:0], K2, hw2).any()
    print(f"room, 3 poses at 48x64: observed share {w3.mean():.4f}; 5 poses, far 4 m: {w5.mean():.4f}")


def _metrics_over(dp, dg, n, threshold, p_area, g_area):
    """The dict of compare_meshes(observed=...) from the distances of all pred samples and of the observed gt samples."""
    a, c = D.metrics(dp, dp, threshold, p_area, g_area), D.metrics(dg, dg, threshold, p_area, g_area)
    pr = a["precision"] + c["recall"]
    return dict(a, completion=c["completion"], completion_median=c["completion_median"], recall=c["recall"],
                fscore=2.0 * a["precision"] * c["recall"] / pr if pr > 0.0 else 0.0,
                chamfer=0.5 * (a["accuracy"] + c["completion"]), gt_observed_share=len(dg) / n, n_gt_observed=len(dg))


def test_compare_meshes_over_the_observed_part(device):
    from mast3r_slam.tsdf import (compare_meshes, face_areas, mesh_distance, observed_points, sample_mesh,
                                  transform_mesh)

    V, F, _, K, hw, _, _ = occluder_scene()
    gt = (_dev(device, V, np.float32), _dev(device, F, np.int32))
    Vr, Fr = synthetic.room_mesh()
    pred = (_dev(device, (Vr * np.float32(0.99)), np.float32), _dev(device, Fr[:8], np.int32))    # four walls, shrunk
    poses = np.stack([synthetic.camera_pose(k) for k in (0, 250, 600)]).astype(np.float32)
    n, th = 5000, 0.03
    spec = dict(poses=poses, K=K, hw=hw, tol=0.02, far=6.0)
    plain = compare_meshes(pred, gt, n_samples=n, threshold=th)
    got = compare_meshes(pred, gt, n_samples=n, threshold=th, observed=spec)
    g_pts = sample_mesh(*gt, n, seed=1)[0]
    seen = observed_points(g_pts, gt, poses, K, hw, tol=0.02, far=6.0)
    assert np.array_equal(seen.cpu().numpy(), R.observed(g_pts.cpu().numpy(), V, F, poses, K, hw, tol=0.02, far=6.0))
    dp = mesh_distance(sample_mesh(*pred, n, seed=0)[0], *gt)[0].cpu().numpy()
    dg = mesh_distance(g_pts[seen], *pred)[0].cpu().numpy()
    want = _metrics_over(dp, dg, n, th, float(face_areas(*pred).sum()), float(face_areas(*gt).sum()))
    assert sorted(got) == sorted(want) and 0 < got["n_gt_observed"] < n
    for k, w in want.items():
        assert abs(got[k] - w) <= 1e-12 * abs(w), (k, got[k], w)
    for k in ("accuracy", "accuracy_median", "precision", "n_samples", "pred_area", "gt_area", "threshold"):
        assert got[k] == plain[k], k
    assert sorted(set(got) - set(plain)) == ["gt_observed_share", "n_gt_observed"]
    # without `observed`: today's dict, key for key (the figures from the distances, as test_mesh_metrics_gpu does)
    dg_all = mesh_distance(g_pts, *pred)[0].cpu().numpy()
    want_plain = D.metrics(dp, dg_all, th, float(face_areas(*pred).sum()), float(face_areas(*gt).sum()))
    assert sorted(plain) == sorted(want_plain)
    for k, w in want_plain.items():
        assert abs(plain[k] - w) <= 1e-12 * abs(w), (k, plain[k], w)
    assert compare_meshes(pred, gt, n_samples=n, threshold=th, observed=None) == plain
    # frame = "pred": a map in another frame with its alignment gives the same observed part, up to the samples within
    # the f32 rounding of the moved poses (1e-6 m) of a border: none or one of 5000
    Tm = np.concatenate([[0.3, -0.1, 0.2], synthetic.quat_from_rotvec(np.array([0.1, -0.2, 0.15])), [1.25]])
    Ti = synthetic.sim3_inv(Tm)
    moved = (transform_mesh(pred[0], Ti), pred[1])
    back = np.stack([R.compose(Ti, p) for p in poses])
    other = compare_meshes(moved, gt, n_samples=n, threshold=th, align=Tm,
                           observed=dict(spec, poses=back, frame="pred"))
    assert abs(other["n_gt_observed"] - got["n_gt_observed"]) <= 1 and "alignment" in other
    assert abs(other["recall"] - got["recall"]) <= 5.0 / got["n_gt_observed"]
    with pytest.raises(ValueError, match="no ground-truth sample is observed"):
        compare_meshes(pred, gt, n_samples=n, threshold=th, observed=dict(spec, far=0.06))
    with pytest.raises(ValueError, match="observed needs poses, K and hw"):
        compare_meshes(pred, gt, n_samples=n, threshold=th, observed=dict(poses=poses, K=K))
    with pytest.raises(ValueError, match="'gt' or 'pred'"):
        compare_meshes(pred, gt, n_samples=n, threshold=th, observed=dict(spec, frame="map"))


# ----------------------------------------------------------------------------------------------------------------------
# product path: the 20-frame run of test_mesh_metrics_gpu.test_slam_system_evaluate_mesh
# ----------------------------------------------------------------------------------------------------------------------
def test_slam_system_observed_metrics_and_depth(device, monkeypatch):
    """Measured on the MI355X (nothing below is asserted against these numbers): see DESIGN.md "Mesh ray casting"."""
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from mast3r_slam.tsdf import render_mesh, sample_mesh
    from test_slam_system_gpu import H, W, RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    n = 20000
    Vr, Fr = synthetic.room_mesh()
    K = synthetic.intrinsics(H, W)
    try:
        system.run(_frames(list(range(0, 60, 3)), device))
        every = system.evaluate_mesh(Vr, Fr, n_samples=n, threshold=VS)
        seen = system.evaluate_mesh(Vr, Fr, n_samples=n, threshold=VS, observed=True, gt_K=K)
        depth = system.evaluate_depth(Vr, Fr)
        with pytest.raises(ValueError, match="no projection"):
            system.evaluate_mesh(Vr, Fr, n_samples=n, observed=True)
        poses = np.stack([system.keyframes[i].T_WC.data.reshape(8).cpu().numpy() for i in range(len(system.keyframes))])
        mesh = system.extract_mesh()
        pose = system.keyframes[len(system.keyframes) - 1].T_WC.data
        tsdf_view = system.render_view(pose=pose, K=K, hw=(H, W))
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    room = (_dev(device, Vr, np.float32), _dev(device, Fr, np.int32))
    g_pts = sample_mesh(*room, n, seed=1)[0].cpu().numpy()
    want = R.observed(g_pts, Vr, Fr, poses, K, (H, W))
    assert seen["n_gt_observed"] == int(want.sum()) and seen["gt_observed_share"] == want.sum() / n
    assert seen["recall"] > every["recall"]
    for k in ("precision", "accuracy", "accuracy_median"):
        assert seen[k] == every[k], k
    assert sorted(set(seen) - set(every)) == ["gt_observed_share", "n_gt_observed"]
    assert all(np.isfinite(depth[k]) for k in depth) and depth["both_hit_share"] > 0.0
    assert depth["n_pixels"] == len(poses) * H * W and 0.0 <= depth["depth_l1_median"]
    # the extracted mesh seen through the mesh caster against the volume seen through the TSDF caster: measured
    mesh_view = render_mesh(mesh, pose, K=K, hw=(H, W))
    both = (tsdf_view[2] & mesh_view[2])
    diff = (tsdf_view[0] - mesh_view[0]).abs()[both]
    cosn = (tsdf_view[1] * mesh_view[1]).sum(-1)[both]
    print(f"20-frame run, {len(poses)} keyframes: observed share {seen['gt_observed_share']:.4f}; recall@{VS} "
          f"{every['recall']:.4f} -> {seen['recall']:.4f}, completion {every['completion']:.4f} -> "
          f"{seen['completion']:.4f} (median {every['completion_median']:.4f} -> {seen['completion_median']:.4f}), "
          f"fscore {every['fscore']:.4f} -> {seen['fscore']:.4f}, precision {seen['precision']:.4f}; depth L1 "
          f"{depth['depth_l1']:.5f} (median {depth['depth_l1_median']:.5f}) over {depth['both_hit_share']:.4f} of "
          f"{depth['n_pixels']} pixels; render_mesh(extract_mesh) against TSDFVolume.render: hit in both "
          f"{float(both.float().mean()):.4f}, in one only {float((tsdf_view[2] ^ mesh_view[2]).float().mean()):.4f}, "
          f"range difference mean {float(diff.mean()):.5f} max {float(diff.max()):.5f}, normals' cosine mean "
          f"{float(cosn.mean()):.4f}")
