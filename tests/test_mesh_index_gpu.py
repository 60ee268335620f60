"""GPU tests (-m gpu) of the mesh index (csrc/mesh_index.hip, the indexed scans of csrc/mesh_tri.h and
csrc/mesh_raycast.hip, mast3r_slam.tsdf.MeshIndex and the `index=` keyword; DESIGN.md "Mesh index"): keys, order and
boxes equal the numpy statement (tests/meshindex_numpy.py) byte for byte; the indexed distance and cast equal the plain
ascending scans (skip = 0) of the caller's mesh byte for byte at the tile and group edges, on a shuffled sphere, on
slivers and on the tie traps of tests/test_mesh_index_cpu.py; robustness; query sorting; that the index prunes a
shuffled mesh; and the Python and SlamSystem paths.  Every operand of the C entry points lies in a guarded buffer."""
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
import meshindex_numpy as X  # noqa: E402
from test_mesh_index_cpu import fan_trap, random_mesh, ray_trap, shuffled, subdivide  # noqa: E402
from mesh_support import (BLOCK, G, T, VS, Operands, _build, _host, _indexed_cast, _raw_cast,  # noqa: E402
                          _raw_distance, _same_bytes)

pytestmark = pytest.mark.gpu

# one face; one short of a tile, a tile, one more; one short of a group of 32 tiles, a group, one face more; a group and
# a tile and a face
SIZES_F = (1, T - 1, T, T + 1, T * G - 1, T * G, T * G + 1, T * G + T + 1)
SIZES_N = (1, 63, 64, 65, 257)
NEAR, FAR = 0.0, 10.0
POSE = np.concatenate([[0.45, 0.55, 0.5], synthetic.quat_from_rotvec(np.array([0.3, 0.5, -0.2])),
                       [1.3]]).astype(np.float32)


def _share(counts, waves, nf):
    if not nf or not waves:
        return 0.0
    return float(counts.cpu().numpy().reshape(-1)[:waves].sum()) / (waves * ((nf + T - 1) // T))


def _distance(device, ix, P, levels=2):
    """mslam_mesh_distance_indexed -> (dist2, nearest, share of (wave, tile) scans skipped); guards checked."""
    import mslam_hip as _m

    ops = Operands(device)
    n = len(P)
    p = ops.put(np.reshape(P, (-1, 3)), np.float32)
    d2, nearest = ops.out(torch.float64, (n,)), ops.out(torch.int32, (n,))
    counts = ops.out(torch.int32, (4 * ((n + BLOCK - 1) // BLOCK),))
    before = ix["ws"].clone()
    _m.check(_m.lib().mslam_mesh_distance_indexed(_m.ptr(p), n, _m.ptr(ix["v"]), _m.ptr(ix["f"]), ix["nf"], ix["nv"],
                                                  _m.ptr(ix["o"]), _m.ptr(ix["ws"]), ix["ws"].numel(), levels,
                                                  _m.ptr(counts), _m.ptr(d2), _m.ptr(nearest), _m.stream_ptr()),
             "mesh_distance_indexed")
    ops.check()
    ix["ops"].check()
    assert torch.equal(before, ix["ws"])                                   # the scan only reads the index
    return d2.cpu().numpy(), nearest.cpu().numpy(), _share(counts, (n + 63) // 64, ix["nf"])


def _cast(device, ix, rays, h, w, pose, levels=2, near=NEAR, far=FAR):
    """mslam_mesh_raycast_indexed -> (dict of numpy arrays as _raw_cast, share skipped); guards checked."""
    out, counts = _indexed_cast(device, ix, rays, h, w, pose, levels, near, far)
    return out, _share(counts, len(counts) if h > 1 else (h * w + 63) // 64, ix["nf"])


def _same_distance(a, b):
    assert a[0].dtype == b[0].dtype and a[1].dtype == b[1].dtype
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


_CASES = {}


def _case(device, nf):
    """The shuffled random mesh of nf faces with its index, built once per size."""
    if nf not in _CASES:
        V, F = random_mesh(nf)
        F = shuffled(F)
        _CASES[nf] = (V, F, _build(device, V, F))
    return _CASES[nf]


@functools.lru_cache(maxsize=None)
def queries(n):
    """Points about the unit cube, two of them far away, and rays in every direction, one of them zero."""
    rng = np.random.default_rng(40 + n)
    P = rng.uniform(-0.2, 1.2, (n, 3)).astype(np.float32)
    P[0] += np.float32(30.0)
    P[n // 2] -= np.float32(45.0)
    rays = rng.normal(size=(n, 3))
    rays = (rays / np.linalg.norm(rays, axis=1, keepdims=True)).astype(np.float32)
    if n > 2:
        rays[n // 2] = 0.0
    return P, rays


# ----------------------------------------------------------------------------------------------------------------------
# the index against its statement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", SIZES_F)
def test_statement_parity(device, nf):
    V, F, ix = _case(device, nf)
    keys = X.face_keys(V, F)
    order = X.order_of(keys)
    tile, group = X.boxes(V, F, order)
    assert ix["keys"].dtype == np.int64 and ix["keys"].tobytes() == keys.tobytes()
    assert ix["order"].dtype == np.int32 and ix["order"].tobytes() == order.tobytes()
    assert ix["tile"].tobytes() == tile.tobytes() and ix["group"].tobytes() == group.tobytes()
    again = _build(device, V, F)                                           # run to run
    for k in ("keys", "order", "tile", "group"):
        assert again[k].tobytes() == ix[k].tobytes(), k
    # the keys of query points: the same kernel, without faces
    import mslam_hip as _m

    P = queries(257)[0]
    ops = Operands(device)
    p, pk = ops.put(P, np.float32), ops.out(torch.int64, (len(P),))
    _m.check(_m.lib().mslam_mesh_index_point_keys(_m.ptr(p), len(P), _m.ptr(ix["bnd"]), _m.ptr(pk), _m.stream_ptr()),
             "mesh_index_point_keys")
    ops.check()
    assert pk.cpu().numpy().tobytes() == X.point_keys(P, X.bounds(V)).tobytes()


# ----------------------------------------------------------------------------------------------------------------------
# the indexed scans against the plain ascending scans of the caller's mesh
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES_N)
@pytest.mark.parametrize("nf", SIZES_F)
def test_scan_parity(device, nf, n):
    V, F, ix = _case(device, nf)
    P, rays = queries(n)
    plain = _raw_distance(device, P, V, F, 0)
    for levels in (2, 1):
        got = _distance(device, ix, P, levels)
        _same_distance(got, plain)
    _same_distance(_distance(device, ix, P), plain)                        # run to run
    plain_cast = _raw_cast(device, rays, 1, n, POSE, V, F, 0, near=NEAR, far=FAR)
    for levels in (2, 1):
        cast, share = _cast(device, ix, rays, 1, n, POSE, levels)
        _same_bytes(cast, plain_cast)
    if n > 2:
        assert cast["hit"][n // 2] == 0                                    # the zero direction
    print(f"F={nf} n={n}: skipped share, points {got[2]:.3f}, rays {share:.3f}; hits {int(cast['hit'].sum())}")


@functools.lru_cache(maxsize=None)
def _sphere(device, r):
    """The marching-cubes sphere of the sphere tests of test_mesh_metrics_gpu / test_mesh_raycast_gpu, radius r: the
    device mesh tuple (faces in cube-key order) and host copies of its vertices and faces."""
    from mast3r_slam.tsdf import mesh_from_voxels

    c = np.zeros(3)
    k, v, w = M.sample_sdf(M.sphere_sdf(c, r), c - r, c + r, VS, 3 * VS)
    mesh = mesh_from_voxels(k, v, w, VS, 0.5, device=device)
    V, _, F = _host(mesh)
    return mesh, V, F


def _view(h, w):
    K = np.array([[float(w), 0, 0.5 * w], [0, float(w), 0.5 * h], [0, 0, 1.0]])
    d = synthetic.pixel_rays(h, w, K)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)


INSIDE = np.array([0.01, -0.02, 0.015, 0, 0, 0, 1, 1], np.float32)
OUTSIDE = np.concatenate([[0.05, 0.03, -0.9], synthetic.quat_from_rotvec(np.array([0.02, -0.05, 0.3])),
                          [1.0]]).astype(np.float32)


def test_shuffled_sphere_and_slivers(device):
    from mast3r_slam.tsdf import sample_mesh

    mesh, V, F0 = _sphere(device, 0.2)
    F = shuffled(F0)
    assert len(F) > 4 * T
    ix = _build(device, V, F)
    near_pts = sample_mesh(mesh[0], mesh[2], 3000, seed=2)[0].cpu().numpy()
    far_pts = (near_pts * np.float32(2.0)).astype(np.float32)
    for P in (near_pts, far_pts, np.random.default_rng(1).permutation(near_pts)):
        plain = _raw_distance(device, P, V, F, 0)
        _same_distance(_distance(device, ix, P), plain)
        assert np.isfinite(plain[0]).all() and (plain[1] >= 0).all()
    rays = _view(40, 40)
    for pose in (INSIDE, OUTSIDE):
        plain = _raw_cast(device, rays, 40, 40, pose, V, F, 0, near=0.0)
        _same_bytes(_cast(device, ix, rays, 40, 40, pose)[0], plain)
        _same_bytes(_cast(device, ix, rays, 40, 40, pose, levels=1)[0], plain)
    assert _raw_cast(device, rays, 40, 40, INSIDE, V, F, 0, near=0.0)["hit"].all()
    # needle triangles (the third corner within 1e-7 of the line through the other two), alone and among ordinary faces
    Vr, Fr = random_mesh(4 * T + 1)
    rng = np.random.default_rng(77)
    tri = Vr.reshape(-1, 3, 3).astype(np.float64)
    t = rng.uniform(-0.5, 1.5, (len(tri), 1))
    tri[:, 2] = tri[:, 0] + t * (tri[:, 1] - tri[:, 0]) + rng.uniform(-1e-7, 1e-7, (len(tri), 3))
    needles = tri.reshape(-1, 3).astype(np.float32)
    assert D.triangles(needles, Fr)[3].sum() > 0.9 * len(Fr)
    P, rays = queries(257)
    mixed, Fm = np.concatenate([Vr, needles]), shuffled(np.concatenate([Fr, Fr + len(Vr)]), seed=8)
    for Vs, Fs in ((needles, shuffled(Fr)), (mixed, Fm)):
        ixs = _build(device, Vs, Fs)
        _same_distance(_distance(device, ixs, P), _raw_distance(device, P, Vs, Fs, 0))
        _same_bytes(_cast(device, ixs, rays, 1, len(rays), POSE)[0],
                    _raw_cast(device, rays, 1, len(rays), POSE, Vs, Fs, 0, near=NEAR, far=FAR))


def test_tie_traps(device):
    """The traps of test_mesh_index_cpu: every face ties exactly, the Morton order meets the highest index first, and
    the lowest original index must win, as in the plain scan."""
    V, F, P = fan_trap()
    ix = _build(device, V, F)
    assert (ix["order"] == np.arange(len(F))[::-1]).all()
    plain = _raw_distance(device, P, V, F, 0)
    assert (plain[1][:2] == 0).all()
    for levels in (2, 1):
        _same_distance(_distance(device, ix, P, levels), plain)
    V, F, rays, pose = ray_trap()
    ix = _build(device, V, F)
    pair = [f for f in range(len(F)) if set(F[f]) <= {0, 1, 2, 3}]
    plain = _raw_cast(device, rays, 1, 2, pose, V, F, 0, near=NEAR, far=FAR)
    assert (plain["t64"] == 1.0).all() and (plain["face"] == pair[0]).all()
    assert list(ix["order"]).index(pair[1]) < list(ix["order"]).index(pair[0])
    for levels in (2, 1):
        _same_bytes(_cast(device, ix, rays, 1, 2, pose, levels)[0], plain)


# ----------------------------------------------------------------------------------------------------------------------
# robustness
# ----------------------------------------------------------------------------------------------------------------------
def test_robustness(device):
    import mslam_hip as _m

    L = _m.lib()
    P, rays = queries(257)
    V, F = random_mesh(3 * T + 5)                       # holds a degenerate and an out-of-range face
    F = shuffled(F)
    valid = D.triangles(V, F)[3]
    assert not valid.all()
    ix = _build(device, V, F)
    nv = int(valid.sum())
    assert valid[ix["order"][:nv]].all() and not valid[ix["order"][nv:]].any()       # the invalid faces last
    got = _distance(device, ix, P)
    _same_distance(got, _raw_distance(device, P, V, F, 0))
    assert valid[got[1]].all()
    # all faces invalid, no faces, no queries
    bad = np.array([[0, 0, 1], [3, 3, 3], [0, 1, len(V)], [-1, 2, 3]], np.int32)
    for Fb in (bad, np.zeros((0, 3), np.int32)):
        ib = _build(device, V, Fb)
        assert (ib["keys"] == X.NONE).all() and np.isposinf(ib["tile"][:, :3]).all()
        d2, nearest, _ = _distance(device, ib, P)
        assert np.isposinf(d2).all() and (nearest == -1).all()
        cast = _cast(device, ib, rays, 1, len(rays), POSE)[0]
        assert not cast["hit"].any() and (cast["face"] == -1).all() and np.isposinf(cast["t64"]).all()
        assert not cast["range"].any() and not cast["normal"].any()
    e = np.zeros((0, 3), np.float32)
    assert _distance(device, ix, e)[0].shape == (0,) and _cast(device, ix, e, 1, 0, POSE)[0]["hit"].shape == (0,)
    assert _build(device, e, np.zeros((0, 3), np.int32))["tile"].shape == (0, 6)
    # an order with entries out of range: skipped, not followed.  The faces it no longer names are not seen, so the
    # answer is the plain scan's on the mesh with those faces made invalid.
    order = ix["order"].copy()
    drop = np.r_[3, T - 1, T, 2 * T + 7, len(F) - 1]
    lost = order[drop].copy()
    order[drop] = (-1, len(F), 2 ** 31 - 1, -2 ** 31, len(F) + 5)
    ib = _build(device, V, F, order=order)
    tile, group = X.boxes(V, F, order)
    assert ib["tile"].tobytes() == tile.tobytes() and ib["group"].tobytes() == group.tobytes()
    F2 = F.copy()
    F2[lost] = -1
    _same_distance(_distance(device, ib, P), _raw_distance(device, P, V, F2, 0))
    _same_bytes(_cast(device, ib, rays, 1, len(rays), POSE)[0],
                _raw_cast(device, rays, 1, len(rays), POSE, V, F2, 0, near=NEAR, far=FAR))
    # a short workspace is refused with the size reported; so is a short index
    need = int(L.mslam_mesh_index_bytes(len(F)))
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    args = (_m.ptr(ix["v"]), _m.ptr(ix["f"]), ix["nf"], ix["nv"], _m.ptr(ix["o"]), _m.ptr(ws))
    assert L.mslam_mesh_index_boxes(*args, need - 1, 0) == -3
    assert f"{need} needed" in L.mslam_last_error().decode()
    assert L.mslam_mesh_index_boxes(*args, need, 0) == 0
    p = torch.from_numpy(P).to(device)
    d2 = torch.empty(len(P), dtype=torch.float64, device=device)
    nr = torch.empty(len(P), dtype=torch.int32, device=device)
    call = lambda nbytes, levels=2: L.mslam_mesh_distance_indexed(
        _m.ptr(p), len(P), _m.ptr(ix["v"]), _m.ptr(ix["f"]), ix["nf"], ix["nv"], _m.ptr(ix["o"]), _m.ptr(ix["ws"]),
        nbytes, levels, 0, _m.ptr(d2), _m.ptr(nr), 0)
    assert call(need - 1) == -3 and f"{need} needed" in L.mslam_last_error().decode()
    assert call(need, levels=3) == -1 and call(need) == 0
    torch.cuda.synchronize()
    ix["ops"].check()


# ----------------------------------------------------------------------------------------------------------------------
# that the index prunes: a shuffled mesh with the index against the same mesh in its extraction order without
# ----------------------------------------------------------------------------------------------------------------------
def test_pruning(device):
    """s_ref: the share of (wave, tile) scans that today's culled scan skips on the sphere in its extraction order, for
    samples of its surface in face order and for one 64x64 view from inside (every ray hits).  The indexed scan on the
    SHUFFLED sphere must skip at least half of s_ref: Morton tiles and cube-key tiles are both compact patches of
    different shape, and half is blind to that difference while it fails when culling is lost (the shuffled sphere
    without an index skips next to nothing).

    The input.  The sphere is the larger one of the existing sphere tests, r = 0.4: 6 668 faces, 53 tiles, under
    10 000 faces.  A Morton tile is a run of octree cells cut every 128 faces, so it is a compact patch only when the
    mesh holds several tiles per cell of the key's first level; the test asks for four per octant, 8 * 4 * 128 = 4 096
    faces, a condition on the input like s_ref >= 0.25 (for which the sphere would grow on, as far as 10 000 faces
    allow).  The smaller sphere, r = 0.2, is 14 tiles, fewer than two per octant: each tile's box is an octant or two and
    touches the centre, where the camera of the inside view stands, so no box test can exclude it.  Measured there, and
    not asserted: points 0.837 / 0.007 / 0.445, inside view 0.661 / 0.000 / 0.125 (extraction order, shuffled, shuffled
    with index).  At r = 0.4: points 0.790 / 0.001 / 0.595, inside view 0.691 / 0.000 / 0.704.

    For rays today's entry point keeps no counts, so its share is taken from the indexed entry with the identity order
    and levels = 1, which is today's scan over today's tiles.  All measured shares: DESIGN.md "Mesh index"."""
    from mast3r_slam.tsdf import sample_mesh

    rays = _view(64, 64)
    for r in (0.4, 0.45):
        mesh, V, F0 = _sphere(device, r)
        assert 8 * 4 * T <= len(F0) < 10000
        ident = np.arange(len(F0), dtype=np.int32)
        P = sample_mesh(mesh[0], mesh[2], 5000, seed=2)[0].cpu().numpy()
        coherent = _raw_distance(device, P, V, F0, 1)
        ray_coherent = _cast(device, _build(device, V, F0, order=ident), rays, 64, 64, INSIDE, levels=1)
        print(f"sphere r={r} F={len(F0)}: extraction order skips {coherent[2]:.3f} (points), "
              f"{ray_coherent[1]:.3f} (rays)")
        if coherent[2] >= 0.25 and ray_coherent[1] >= 0.25:
            break
    assert coherent[2] >= 0.25 and ray_coherent[1] >= 0.25
    F = shuffled(F0)
    lost = _raw_distance(device, P, V, F, 1)
    ix = _build(device, V, F)
    indexed = _distance(device, ix, P)
    _same_distance(indexed, _raw_distance(device, P, V, F, 0))
    ray_lost = _cast(device, _build(device, V, F, order=ident), rays, 64, 64, INSIDE, levels=1)
    ray_indexed = _cast(device, ix, rays, 64, 64, INSIDE)
    _same_bytes(ray_indexed[0], ray_lost[0])
    _same_bytes(ray_indexed[0], _raw_cast(device, rays, 64, 64, INSIDE, V, F, 0, near=NEAR, far=FAR))
    print(f"skipped share, points: extraction order {coherent[2]:.3f}, shuffled {lost[2]:.3f}, shuffled with index "
          f"{indexed[2]:.3f} (tiles alone {_distance(device, ix, P, 1)[2]:.3f}); 64x64 view: {ray_coherent[1]:.3f}, "
          f"{ray_lost[1]:.3f}, {ray_indexed[1]:.3f}")
    assert indexed[2] >= 0.5 * coherent[2]
    assert ray_indexed[1] >= 0.5 * ray_coherent[1]


# ----------------------------------------------------------------------------------------------------------------------
# Python
# ----------------------------------------------------------------------------------------------------------------------
def _shuffled_sphere(device):
    mesh, V, F0 = _sphere(device, 0.2)
    gt = (mesh[0], torch.from_numpy(shuffled(F0)).to(device))
    return mesh, gt


def test_query_sorting(device):
    from mast3r_slam.tsdf import MeshIndex, mesh_distance, observed_points, sample_mesh

    mesh, gt = _shuffled_sphere(device)
    ix = MeshIndex(*gt)
    P = sample_mesh(mesh[0], mesh[2], 3001, seed=4)[0]
    P = P[torch.randperm(len(P), generator=torch.Generator().manual_seed(2)).to(device)].contiguous()
    P[7] = 50.0
    want = mesh_distance(P, *gt, skip=False)
    for kw in (dict(index=ix), dict(index=ix, sort_queries=False), dict(index=True)):
        got = mesh_distance(P, *gt, **kw)
        assert got[0].dtype == want[0].dtype and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), kw
    poses = np.stack([INSIDE, OUTSIDE])
    K, hw = np.array([[40.0, 0, 20.0], [0, 40.0, 20.0], [0, 0, 1.0]]), (40, 40)
    Q = (P * 0.9).contiguous()
    seen = observed_points(Q, gt, poses, K, hw, near=0.0, tol=0.01)
    assert 0 < int(seen.sum()) < len(Q)
    for kw in (dict(index=ix), dict(index=ix, sort_queries=False), dict(index=True, compact_every=1)):
        assert torch.equal(observed_points(Q, gt, poses, K, hw, near=0.0, tol=0.01, **kw), seen), kw


def test_python_paths(device):
    from mast3r_slam.tsdf import (MeshIndex, align_meshes, build_mesh_index, compare_meshes, render_mesh,
                                  transform_mesh)

    mesh, gt = _shuffled_sphere(device)
    Tm = np.concatenate([[0.01, -0.008, 0.005], synthetic.quat_from_rotvec(np.array([0.02, -0.03, 0.015])), [1.03]])
    pred = (transform_mesh(mesh[0], Tm), mesh[2])
    ix = build_mesh_index(gt)
    assert isinstance(ix, MeshIndex) and ix.order.dtype == torch.int32 and ix.order.shape == (gt[1].shape[0],)
    n = 4000
    poses = np.stack([INSIDE, OUTSIDE])
    spec = dict(poses=poses, K=np.array([[40.0, 0, 20.0], [0, 40.0, 20.0], [0, 0, 1.0]]), hw=(40, 40), near=0.0)
    icp = dict(n_samples=2000, max_iters=10)
    for kw in (dict(), dict(observed=spec), dict(align="icp", align_kw=icp), dict(align="icp", align_kw=icp,
                                                                                observed=spec)):
        want = compare_meshes(pred, gt, n_samples=n, threshold=0.01, **kw)
        for index in (True, ix):
            got = compare_meshes(pred, gt, n_samples=n, threshold=0.01, index=index, **kw)
            assert got == want, (sorted(kw), [k for k in want if got[k] != want[k]])
    want = align_meshes(pred, gt, **icp)
    got = align_meshes(pred, gt, index=ix, **icp)
    assert torch.equal(got["T"], want["T"]) and np.array_equal(got["history"], want["history"])
    assert got["iterations"] == want["iterations"] == len(want["history"]) and got["rmse"] == want["rmse"]
    rays = _view(33, 47)
    for pose in (INSIDE, OUTSIDE):
        want = render_mesh(gt, pose, rays=rays, near=0.0, return_face=True, skip=False)
        for index in (True, ix):
            got = render_mesh(gt, pose, rays=rays, near=0.0, return_face=True, index=index)
            assert all(torch.equal(a, b) for a, b in zip(got, want))
    # an index of another mesh is refused: other tensors, even with the same contents
    other = (gt[0].clone(), gt[1])
    for call in (lambda: compare_meshes(pred, other, n_samples=n, index=ix),
                 lambda: align_meshes(pred, other, index=ix, **icp),
                 lambda: render_mesh(other, INSIDE, rays=rays, index=ix),
                 lambda: render_mesh((gt[0], gt[1][:-1]), INSIDE, rays=rays, index=ix)):
        with pytest.raises(ValueError, match="built for another mesh"):
            call()
    with pytest.raises(TypeError, match="index must be"):
        render_mesh(gt, INSIDE, rays=rays, index="yes")


def test_slam_system_with_index(device, monkeypatch):
    """The 20-frame run of the product tests, scored against the room with every face split at its edge midpoints three
    times (768 faces) and shuffled: evaluate_mesh and evaluate_depth with index=True equal index=None."""
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from test_slam_system_gpu import H, W, RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    Vr, Fr = subdivide(*synthetic.room_mesh(), 3)
    Fr = shuffled(Fr)
    assert len(Fr) == 768
    K = synthetic.intrinsics(H, W)
    n = 20000
    try:
        system.run(_frames(list(range(0, 60, 3)), device))
        results = {}
        for index in (None, True):
            results[index] = (system.evaluate_mesh(Vr, Fr, n_samples=n, threshold=VS, index=index),
                              system.evaluate_mesh(Vr, Fr, n_samples=n, threshold=VS, observed=True, gt_K=K,
                                                   index=index),
                              system.evaluate_depth(Vr, Fr, index=index))
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    for a, b in zip(results[None], results[True]):
        assert a == b, [k for k in a if a[k] != b[k]]
    every, seen, depth = results[True]
    assert 0.0 < every["recall"] <= seen["recall"] and 0 < seen["n_gt_observed"] < n
    assert np.isfinite(depth["depth_l1"]) and depth["both_hit_share"] > 0.0
