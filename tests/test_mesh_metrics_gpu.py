"""GPU tests (-m gpu) of the mesh-quality kernels (csrc/mesh_distance.hip, DESIGN.md "Mesh quality") and of
mast3r_slam.tsdf.face_areas / sample_mesh / mesh_distance / compare_meshes and SlamSystem.evaluate_mesh: parity with
the numpy statement (tests/meshdist_numpy.py) at the kernel's tile edges, culled against plain scan bit for bit,
guarded buffers, invalid faces, the sampler, metrics that can be derived by hand, and the product path.

Parity bounds: dist2 to 1e-12 relative (the same f64 operations in the same order on both sides); the nearest face
equal, or - for at most 1 % of the points - a face whose numpy distance is within 1e-12 relative of the minimum."""
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
from test_mesh_metrics_cpu import tie_share  # noqa: E402
from kernel_refs import Guarded, check_guards  # noqa: E402
from mesh_support import BLOCK, T, VS, _dev, _host, _raw_distance, _room, _vol  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 1e-12
TILE_F = (1, T - 1, T, T + 1, 4 * T + 1)
TILE_N = (1, BLOCK - 1, BLOCK, BLOCK + 1)


@functools.lru_cache(maxsize=None)
def tile_case(nf, n):
    """Small random f32 triangles in the unit cube in the order of their x, so that the tiles' boxes differ, and points in
    the order of theirs, with a few far outliers among both, and the numpy answer.  Computed once per shape."""
    rng = np.random.default_rng(1000 * nf + n)
    centre = rng.uniform(0.0, 1.0, (nf, 3))
    centre = centre[np.argsort(centre[:, 0])]
    V = (centre[:, None, :] + rng.uniform(-0.06, 0.06, (nf, 3, 3))).astype(np.float32).reshape(-1, 3)
    far = rng.choice(min(nf, T), min(3, nf // 8), replace=False)          # all in the first tile: its box is huge
    V.reshape(nf, 3, 3)[far] += np.float32(40.0)
    F = np.arange(3 * nf, dtype=np.int32).reshape(nf, 3)
    P = rng.uniform(-0.1, 1.1, (n, 3))
    P = P[np.argsort(P[:, 0])].astype(np.float32)                          # coherent waves, as samples in face order are
    P[0] -= np.float32(30.0)                                               # far points in the first and the third wave
    P[n // 2] += np.float32(45.0)
    d2, nearest = D.closest(P, V, F)
    return P, V, F, d2, nearest


def _parity(P, V, F, d2, nearest, want_d2, want_nearest):
    assert d2.dtype == np.float64 and nearest.dtype == np.int32
    assert (np.abs(d2 - want_d2) <= REL * want_d2).all(), np.abs(d2 - want_d2).max()
    other = np.flatnonzero(nearest != want_nearest)
    if len(other):
        assert len(other) <= 0.01 * len(P)
        a, b, c, valid = D.triangles(V, F)
        for i in other:
            f = nearest[i]
            assert 0 <= f < len(F) and valid[f]
            d = D.tri_dist2(P[i:i + 1].astype(np.float64), a[f], b[f], c[f])[0]
            assert abs(np.sqrt(d) - np.sqrt(want_d2[i])) <= REL * np.sqrt(want_d2[i])
    return len(other)


@pytest.mark.parametrize("n", TILE_N)
@pytest.mark.parametrize("nf", TILE_F)
def test_tile_edges(device, nf, n):
    P, V, F, want_d2, want_nearest = tile_case(nf, n)
    # the numpy statement itself against the independent formulation, on this case's seed (CPU)
    assert tie_share(P, V, F, want_d2, want_nearest) <= 0.01
    plain = _raw_distance(device, P, V, F, 0)
    culled = _raw_distance(device, P, V, F, 1)
    differ = _parity(P, V, F, plain[0], plain[1], want_d2, want_nearest)
    assert plain[0].tobytes() == culled[0].tobytes() and plain[1].tobytes() == culled[1].tobytes()
    again = _raw_distance(device, P, V, F, 1)
    assert again[0].tobytes() == culled[0].tobytes() and again[1].tobytes() == culled[1].tobytes()
    print(f"F={nf} n={n}: max dist {np.sqrt(want_d2.max()):.3g}, faces that differ {differ}, skipped {culled[2]:.3f}")
    if nf > 2 * T and n >= BLOCK - 1:
        assert 0.0 < culled[2] < 1.0                     # some tiles are culled and some are not
    # the Python entry point: the same numbers, as distances
    from mast3r_slam.tsdf import mesh_distance

    args = (_dev(device, P, np.float32), _dev(device, V, np.float32), _dev(device, F, np.int32))
    for skip in (True, False):
        dist, near = mesh_distance(*args, skip=skip)
        assert dist.dtype == torch.float64 and near.dtype == torch.int32 and dist.is_cuda
        assert (np.abs(dist.cpu().numpy() - np.sqrt(plain[0])) <= 1e-15 * np.sqrt(plain[0])).all()
        assert np.array_equal(near.cpu().numpy(), plain[1])


def test_slivers_culled_equals_plain(device):
    """Needle triangles (the third corner within 1e-7 of the line through the other two), which marching cubes makes
    when a vertex nears a cube corner: the interior region's barycentrics lose most of their digits there, which is what
    the absolute slack of the skip test is for.  Culled, plain and numpy agree as everywhere else."""
    P, V, F, _, _ = tile_case(4 * T + 1, BLOCK + 1)
    rng = np.random.default_rng(77)
    tri = V.reshape(-1, 3, 3).astype(np.float64)
    t = rng.uniform(-0.5, 1.5, (len(tri), 1))
    tri[:, 2] = tri[:, 0] + t * (tri[:, 1] - tri[:, 0]) + rng.uniform(-1e-7, 1e-7, (len(tri), 3))
    V = tri.reshape(-1, 3).astype(np.float32)
    assert D.triangles(V, F)[3].sum() > 0.9 * len(F)
    want_d2, want_nearest = D.closest(P, V, F)
    plain = _raw_distance(device, P, V, F, 0)
    culled = _raw_distance(device, P, V, F, 1)
    _parity(P, V, F, plain[0], plain[1], want_d2, want_nearest)
    assert plain[0].tobytes() == culled[0].tobytes() and plain[1].tobytes() == culled[1].tobytes()
    assert 0.0 < culled[2] < 1.0


def test_sphere_culled_equals_plain(device):
    """A marching-cubes sphere (faces in cube-key order) queried with its own samples (in face order) and with samples of
    a sphere of twice the radius: culled and plain scans agree bit for bit, and the first is where culling bites."""
    from mast3r_slam.tsdf import mesh_from_voxels, sample_mesh

    meshes = []
    for r in (0.2, 0.4):
        c = np.zeros(3)
        k, v, w = M.sample_sdf(M.sphere_sdf(c, r), c - r, c + r, VS, 3 * VS)
        meshes.append(mesh_from_voxels(k, v, w, VS, 0.5, device=device))
    V, _, F = _host(meshes[0])
    assert len(F) > 4 * T
    shares, farthest = [], []
    for mesh in meshes:
        P = sample_mesh(mesh[0], mesh[2], 5000, seed=2)[0].cpu().numpy()
        plain = _raw_distance(device, P, V, F, 0)
        culled = _raw_distance(device, P, V, F, 1)
        assert plain[0].tobytes() == culled[0].tobytes() and plain[1].tobytes() == culled[1].tobytes()
        assert np.isfinite(plain[0]).all() and (plain[1] >= 0).all()
        w2, wn = D.closest(P[:64], V, F)
        _parity(P[:64], V, F, plain[0][:64], plain[1][:64], w2, wn)
        shares.append(culled[2])
        farthest.append(np.sqrt(plain[0].max()))
    assert farthest[0] <= 4 * 2.0 ** -24 * np.abs(V).max()        # its own samples lie on it, up to their f32 rounding
    assert 0.2 - 2 * VS <= farthest[1] <= 0.2 + 2 * VS            # and the larger sphere's lie a radius away
    print(f"sphere F={len(F)}: tile share skipped {shares[0]:.3f} (own samples), {shares[1]:.3f} (radius x 2)")
    assert shares[0] > 0.0


# ----------------------------------------------------------------------------------------------------------------------
# guarded buffers: nothing is written in front of or behind dist2, nearest, points and face
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, BLOCK + 1])
def test_guarded_buffers(device, n):
    import mslam_hip as _m

    L, st = _m.lib(), _m.stream_ptr()
    _, V, F, _, _ = tile_case(T + 1, BLOCK + 1)
    v, f = _dev(device, V, np.float32), _dev(device, F, np.int32)
    area = Guarded(device, torch.float64, (len(F),))
    _m.check(L.mslam_mesh_face_areas(_m.ptr(v), _m.ptr(f), len(F), len(V), _m.ptr(area.t), st), "mesh_face_areas")
    cdf = torch.cumsum(area.t, 0)
    pts, face = Guarded(device, torch.float32, (n, 3)), Guarded(device, torch.int32, (n,))
    _m.check(L.mslam_mesh_sample(_m.ptr(v), _m.ptr(f), len(F), len(V), _m.ptr(cdf), float(cdf[-1]), n, 7,
                                 _m.ptr(pts.t), _m.ptr(face.t), st), "mesh_sample")
    inputs = dict(area=area, pts=pts, face=face)
    check_guards(inputs, list(inputs), "mesh_face_areas, mesh_sample")
    wb = int(L.mslam_mesh_distance_workspace_bytes(len(F)))
    for skip in (0, 1):
        d2, near = Guarded(device, torch.float64, (n,)), Guarded(device, torch.int32, (n,))
        ws = Guarded(device, torch.float64, (wb // 8,))
        _m.check(L.mslam_mesh_distance(_m.ptr(pts.t), n, _m.ptr(v), _m.ptr(f), len(F), len(V), skip, _m.ptr(ws.t), wb,
                                       _m.ptr(d2.t), _m.ptr(near.t), st), "mesh_distance")
        check_guards(dict(d2=d2, near=near, pts=pts, face=face, ws=ws), ("d2", "near", "pts", "face"), f"skip={skip}")
        assert bool(ws.all_written()) == bool(skip)                      # skip = 0 leaves the workspace alone


# ----------------------------------------------------------------------------------------------------------------------
# invalid faces and bad arguments
# ----------------------------------------------------------------------------------------------------------------------
def test_invalid_faces_and_arguments(device):
    import mslam_hip as _m
    from mast3r_slam.tsdf import compare_meshes, face_areas, mesh_distance, sample_mesh

    P, V, F, _, _ = tile_case(T + 1, BLOCK - 1)
    line = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32)
    V2 = np.concatenate([V, line])
    nv = len(V2)
    bad = np.array([[0, 0, 1], [3, 3, 3], [nv - 3, nv - 2, nv - 1], [0, 1, nv], [-1, 2, 3]], np.int32)
    mixed = np.concatenate([bad[:2], F[:T - 3], bad[2:], F[T - 3:], bad[:1]]).astype(np.int32)
    want_d2, want_nearest = D.closest(P, V2, mixed)
    a, b, c, valid = D.triangles(V2, mixed)
    assert valid.sum() == len(F)
    for skip in (0, 1):                         # the C entry point checks every index itself
        d2, nearest, _ = _raw_distance(device, P, V2, mixed, skip)
        _parity(P, V2, mixed, d2, nearest, want_d2, want_nearest)
        assert valid[nearest].all()
        d2, nearest, _ = _raw_distance(device, P, V2, bad, skip)
        assert np.isposinf(d2).all() and (nearest == -1).all()
        d2, nearest, _ = _raw_distance(device, P, V2, np.zeros((0, 3), np.int32), skip)
        assert np.isposinf(d2).all() and (nearest == -1).all()
    p, v, f = _dev(device, P, np.float32), _dev(device, V2, np.float32), _dev(device, mixed, np.int32)
    in_range = _dev(device, mixed[(mixed >= 0).all(1) & (mixed < nv).all(1)], np.int32)
    areas = face_areas(v, in_range).cpu().numpy()
    assert np.array_equal(areas == 0.0, ~D.triangles(V2, in_range.cpu().numpy())[3])
    pts, face = sample_mesh(v, in_range, 3000, seed=1)
    assert (areas[face.cpu().numpy()] > 0.0).all()
    dist, near = mesh_distance(p, v, _dev(device, bad[:3], np.int32))
    assert torch.isinf(dist).all() and (near == -1).all()
    with pytest.raises(ValueError, match=r"outside \[0, "):
        mesh_distance(p, v, f)
    with pytest.raises(ValueError, match=r"outside \[0, "):
        sample_mesh(v, f, 10)
    with pytest.raises(ValueError, match="no area"):
        sample_mesh(v, _dev(device, bad[:3], np.int32), 10)
    with pytest.raises(ValueError, match="no area"):
        compare_meshes((v, in_range), (v, _dev(device, bad[:3], np.int32)), n_samples=10)
    with pytest.raises(ValueError, match="n must be"):
        sample_mesh(v, in_range, 0)
    with pytest.raises(RuntimeError, match="dtype"):
        mesh_distance(p.double(), v, in_range)
    with pytest.raises(RuntimeError, match="dtype"):
        face_areas(v.double(), in_range)
    with pytest.raises(RuntimeError, match="dtype"):
        face_areas(v, in_range.long())
    with pytest.raises(ValueError, match=r"\(n,3\)"):
        mesh_distance(p.reshape(-1), v, in_range)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_distance(p.cpu(), v, in_range)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        face_areas(v.cpu(), in_range)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sample_mesh(v, in_range.cpu(), 10)
    rc = _m.lib().mslam_mesh_distance(_m.ptr(p), len(P), _m.ptr(v), _m.ptr(f), len(mixed), nv, 1, 0, 0, 0, 0, 0)
    assert rc != 0                              # a culled scan without a workspace is refused, not run


# ----------------------------------------------------------------------------------------------------------------------
# sampler
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, BLOCK + 1, 5000])
def test_sampler_matches_numpy(device, n):
    import mslam_hip as _m
    from mast3r_slam.tsdf import face_areas, sample_mesh

    rng = np.random.default_rng(4)
    V = rng.uniform(-1.0, 2.0, (300, 3)).astype(np.float32)
    F = np.stack([rng.permutation(300)[:3] for _ in range(2 * BLOCK + 3)]).astype(np.int32)
    F[[0, 100, 101, len(F) - 1]] = [[1, 1, 2], [4, 4, 4], [7, 8, 7], [5, 6, 6]]
    v, f = _dev(device, V, np.float32), _dev(device, F, np.int32)
    area = face_areas(v, f)
    want = D.face_areas(V, F)
    got = area.cpu().numpy()
    assert (np.abs(got - want) <= REL * want).all() and np.array_equal(got == 0.0, want == 0.0)
    cdf = torch.cumsum(area, 0)
    pts, face = sample_mesh(v, f, n, seed=9)
    assert pts.dtype == torch.float32 and pts.shape == (n, 3) and face.dtype == torch.int32 and face.shape == (n,)
    want_pts, want_face = D.sample(V, F, cdf.cpu().numpy(), n, seed=9)
    assert np.array_equal(face.cpu().numpy(), want_face)
    assert np.abs(pts.cpu().numpy() - want_pts).max() <= 1e-6
    assert (want[want_face] > 0.0).all()
    counts = np.bincount(want_face, minlength=len(F))
    assert (np.abs(counts - n * got / float(cdf[-1])) <= 1.0 + 1e-9).all()
    again = sample_mesh(v, f, n, seed=9)
    assert torch.equal(again[0], pts) and torch.equal(again[1], face)
    if n > 1:
        assert not torch.equal(sample_mesh(v, f, n, seed=10)[0], pts)
    # a seed beyond 63 bits goes through as its low 64 bits
    big = sample_mesh(v, f, n, seed=(1 << 64) + 9)
    assert torch.equal(big[0], pts)
    assert _m.lib().mslam_mesh_sample(_m.ptr(v), _m.ptr(f), len(F), len(V), _m.ptr(cdf), 0.0, n, 0, _m.ptr(pts),
                                      _m.ptr(face), 0) != 0          # a zero total is refused by the entry point too


# ----------------------------------------------------------------------------------------------------------------------
# metrics that follow from the geometry: flat 8 x 8-quad grids with dyadic coordinates
# ----------------------------------------------------------------------------------------------------------------------
def _grid(lo, hi, z):
    t = np.linspace(lo, hi, 9)
    x, y = np.meshgrid(t, t, indexing="ij")
    V = np.stack([x, y, np.full_like(x, z)], -1).reshape(-1, 3).astype(np.float32)
    q = (np.arange(8)[:, None] * 9 + np.arange(8)[None]).reshape(-1)
    F = np.concatenate([np.stack([q, q + 9, q + 10], 1), np.stack([q, q + 10, q + 1], 1)]).astype(np.int32)
    return V, F


def test_derivable_metrics(device):
    from mast3r_slam.tsdf import compare_meshes, mesh_distance, sample_mesh

    d = 0.125
    V, F = _grid(0.0, 1.0, 0.5)
    W, G = _grid(-0.5, 1.5, 0.5 + d)                  # shifted along the normal, twice the extent, the same centre
    pred = (_dev(device, V, np.float32), _dev(device, F, np.int32))
    gt = (_dev(device, W, np.float32), _dev(device, G, np.int32))
    n = 4001
    same = compare_meshes(pred, pred, n_samples=n, threshold=0.01)
    bound = 4 * 2.0 ** -24 * np.abs(V).max()
    assert 0.0 <= same["accuracy"] <= bound and 0.0 <= same["completion"] <= bound
    assert same["precision"] == 1.0 and same["recall"] == 1.0 and same["fscore"] == 1.0
    assert same["pred_area"] == 1.0 and same["gt_area"] == 1.0 and same["n_samples"] == n
    out = {th: compare_meshes(pred, gt, n_samples=n, threshold=th) for th in (0.2, 0.1)}
    for th, m in out.items():
        assert abs(m["accuracy"] - d) <= REL * d and abs(m["accuracy_median"] - d) <= REL * d
        assert m["gt_area"] == 4.0 and m["threshold"] == th
        assert m["chamfer"] == 0.5 * (m["accuracy"] + m["completion"])
        pr = m["precision"] + m["recall"]
        assert m["fscore"] == (2.0 * m["precision"] * m["recall"] / pr if pr > 0.0 else 0.0)
        assert m["completion"] > d                     # three quarters of gt lie beside pred, not above it
    assert out[0.2]["precision"] == 1.0 and out[0.1]["precision"] == 0.0
    assert 0.25 <= out[0.2]["recall"] < 1.0 and out[0.1]["recall"] == 0.0 and out[0.1]["fscore"] == 0.0
    # the whole dict against the numpy statement, from the device's own samples
    dp = D.closest(sample_mesh(*pred, n, seed=0)[0].cpu().numpy(), W, G)[0]
    dg = D.closest(sample_mesh(*gt, n, seed=1)[0].cpu().numpy(), V, F)[0]
    want = D.metrics(np.sqrt(dp), np.sqrt(dg), 0.2, 1.0, 4.0)
    assert sorted(want) == sorted(out[0.2])
    for k, w in want.items():
        assert abs(out[0.2][k] - w) <= REL * abs(w), (k, out[0.2][k], w)
    # an extract_mesh tuple: normals and colours are ignored
    z = torch.zeros_like(pred[0])
    assert compare_meshes((pred[0], z, pred[1]), (gt[0], z, gt[1], z), n_samples=n, threshold=0.2) == out[0.2]
    assert compare_meshes(pred, gt, n_samples=n, threshold=0.2, skip=False) == out[0.2]
    dist, _ = mesh_distance(sample_mesh(*pred, n, seed=0)[0], *gt)
    assert (np.abs(dist.cpu().numpy() - np.sqrt(dp)) <= REL * np.sqrt(dp)).all()


# ----------------------------------------------------------------------------------------------------------------------
# product path
# ----------------------------------------------------------------------------------------------------------------------
def _recomputed(device, mesh, gt, n, threshold, prefix=512):
    """The dict of compare_meshes again: distances from the device, checked against the numpy statement on a prefix of
    the samples, means and shares in numpy."""
    from mast3r_slam.tsdf import face_areas, mesh_distance, sample_mesh

    gv, gf = (_dev(device, gt[0], np.float32), _dev(device, gt[1], np.int32))
    V, F = mesh[0].cpu().numpy(), mesh[2].cpu().numpy()
    dist = []
    for (sv, sf), (tv, tf), host, seed in (((mesh[0], mesh[2]), (gv, gf), gt, 0), ((gv, gf), (mesh[0], mesh[2]), (V, F), 1)):
        pts = sample_mesh(sv, sf, n, seed=seed)[0]
        d, near = mesh_distance(pts, tv, tf)
        d, near = d.cpu().numpy(), near.cpu().numpy()
        P = pts.cpu().numpy()[:prefix]
        w2, wn = D.closest(P, *host)
        _parity(P, host[0], host[1], d[:prefix] ** 2, near[:prefix], w2, wn)
        assert (np.abs(d[:prefix] - np.sqrt(w2)) <= REL * np.sqrt(w2)).all()
        dist.append(d)
    return D.metrics(dist[0], dist[1], threshold, float(face_areas(mesh[0], mesh[2]).sum()),
                     float(face_areas(gv, gf).sum()))


def _assert_same_metrics(got, want):
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        assert abs(got[k] - w) <= REL * abs(w), (k, got[k], w)


def test_slam_system_evaluate_mesh(device, monkeypatch):
    """The run of test_tsdf_mesh_gpu.test_slam_system_mesh_and_ply, scored against the room it was rendered from."""
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from test_slam_system_gpu import RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    assert tcfg["mesh_eval_threshold"] == 0.05
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    n = 20000
    try:
        system.run(_frames(list(range(0, 60, 3)), device))
        m = system.evaluate_mesh(*synthetic.room_mesh(), n_samples=n, threshold=VS)
        default = system.evaluate_mesh(*synthetic.room_mesh(), n_samples=n)
        mesh = system.extract_mesh()
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    _assert_same_metrics(m, _recomputed(device, mesh, synthetic.room_mesh(), n, VS))
    assert default["threshold"] == 0.05 and default["accuracy"] == m["accuracy"]
    assert default["precision"] >= m["precision"]
    Vh = mesh[0].cpu().numpy().astype(np.float64)
    near = (np.abs(synthetic.ROOM_HALF[None] - np.abs(Vh)).min(1) <= VS).mean()
    print(f"slam mesh against the room: F={mesh[2].shape[0]} accuracy {m['accuracy']:.5f} (median "
          f"{m['accuracy_median']:.5f}) completion {m['completion']:.5f} precision@{VS} {m['precision']:.4f} "
          f"recall@{VS} {m['recall']:.4f} fscore {m['fscore']:.4f}; vertices within one voxel of a wall {near:.4f}")
    assert np.isfinite(m["accuracy"]) and 0.0 <= m["accuracy"] < 0.12          # below the truncation distance
    assert 0.0 < m["recall"] <= 1.0                                            # only part of the room is seen
    off = SlamSystem(RoomModel(device), device, tsdf_global_cfg=None)
    with pytest.raises(RuntimeError, match="global TSDF is disabled"):
        off.evaluate_mesh(*synthetic.room_mesh())


def test_two_shards_score_as_one(device):
    from mast3r_slam.tsdf import compare_meshes, mesh_from_voxels

    big = _vol(device, 1 << 22)
    shards = [_vol(device, 1 << 19, shard_id=r, num_shards=2) for r in range(2)]
    for pw, conf, org in _room():
        big.integrate(pw, conf, org)
        for s in shards:
            s.integrate(pw, conf, org, return_fused=False)
    parts = [s.voxels() for s in shards]
    keys, t, w = (np.concatenate([p[j] for p in parts]) for j in range(3))
    rv, rf = synthetic.room_mesh()
    gt = (_dev(device, rv, np.float32), _dev(device, rf, np.int32))
    one = compare_meshes(big.extract_mesh(), gt, n_samples=20000, threshold=VS)
    two = compare_meshes(mesh_from_voxels(keys, t, w, VS, big.min_weight, device=device), gt, n_samples=20000,
                         threshold=VS)
    assert one == two
    assert np.isfinite(one["accuracy"]) and one["accuracy"] < 0.12 and 0.0 < one["recall"] <= 1.0
    _assert_same_metrics(one, _recomputed(device, big.extract_mesh(), (rv, rf), 20000, VS, prefix=256))
