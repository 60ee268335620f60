"""GPU tests (-m gpu) of the point-cloud tools (csrc/cloud.hip, mast3r_slam/tsdf/cloud.py, SlamSystem.keyframe_cloud /
evaluate_cloud; DESIGN.md "Point clouds") against the numpy statement tests/cloud_numpy.py: the index, the nearest
neighbour in its three forms (plain, tiles, tiles and groups) byte for byte at the tile, group and block edges, the
traps of tests/test_cloud_cpu.py, robustness, culling, the voxel downsample, ICP and the figures.  Every operand of the
C entry points lies in a guarded buffer, and the guards are checked after every raw call."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from mast3r_slam import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_numpy as C  # noqa: E402
import meshalign_numpy as A  # noqa: E402
from test_cloud_cpu import duplicate_trap, f32_trap, lattice_trap  # noqa: E402
from mesh_support import BLOCK, G, T, VS, Operands  # noqa: E402

pytestmark = pytest.mark.gpu

# none, one; one short of a tile, a tile, one more; one short of a group of 32 tiles, a group, one more; two groups and
# a point
SIZES_N = (0, 1, 2, T - 1, T, T + 1, T * G - 1, T * G, T * G + 1, 2 * T * G + 1)
# none, one; around a wave; around a block; two blocks and a point
SIZES_Q = (0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)
MODES = ("plain", 1, 2)
SOLVE_TOL = 1e-9                      # the bar of tests/test_mesh_align_gpu.py


def _lib():
    import mslam_hip as _m

    return _m, _m.lib(), _m.stream_ptr()


def _build(device, P, order=None):
    """The index through the C entry points: mslam_mesh_index_point_keys over the box of the valid points, the mask, a
    stable torch.sort and mslam_cloud_index_boxes -> dict with the device operands (p, o, ws) and numpy copies of keys,
    order and boxes.  `order`: put this one in the place of the sorted one."""
    _m, L, st = _lib()
    ops = Operands(device)
    P = C.f32(P)
    N = len(P)
    p = ops.put(P, np.float32)
    bnd = ops.put(C.bounds(P), np.float32)
    keys = ops.out(torch.int64, (N,))
    _m.check(L.mslam_mesh_index_point_keys(_m.ptr(p), N, _m.ptr(bnd), _m.ptr(keys), st), "mesh_index_point_keys")
    keys = torch.where(torch.isfinite(p).all(1), keys, C.NONE) if N else keys
    srt = torch.sort(keys, stable=True)[1].to(torch.int32).cpu().numpy() if order is None else np.asarray(order, np.int32)
    o = ops.put(srt, np.int32)
    ntiles = (N + T - 1) // T
    ngroups = (ntiles + G - 1) // G
    need = int(L.mslam_cloud_index_bytes(N))
    assert need == 48 * (ntiles + ngroups)
    ws = ops.out(torch.float64, (need // 8,)).view(torch.uint8)
    _m.check(L.mslam_cloud_index_boxes(_m.ptr(p), N, _m.ptr(o), _m.ptr(ws), ws.numel(), st), "cloud_index_boxes")
    ops.check()
    box = ws[:need].cpu().numpy().view(np.float64).reshape(-1, 6)
    return dict(ops=ops, P=P, p=p, N=N, o=o, ws=ws, keys=keys.cpu().numpy(), order=srt, tile=box[:ntiles],
                group=box[ntiles:])


def _distance(device, ix, Q, mode):
    """mslam_cloud_distance -> (dist2, nearest, per-wave skip counts); mode "plain" (order NULL), 1 or 2 (levels)."""
    _m, L, st = _lib()
    ops = Operands(device)
    Q = C.f32(Q)
    n = len(Q)
    q = ops.put(Q, np.float32)
    d2, nearest = ops.out(torch.float64, (n,)), ops.out(torch.int32, (n,))
    counts = ops.out(torch.int32, (4 * ((n + BLOCK - 1) // BLOCK),))
    before = ix["ws"].clone()
    if mode == "plain":
        rc = L.mslam_cloud_distance(_m.ptr(q), n, _m.ptr(ix["p"]), ix["N"], 0, 0, 0, 1, _m.ptr(counts), _m.ptr(d2),
                                    _m.ptr(nearest), st)
    else:
        rc = L.mslam_cloud_distance(_m.ptr(q), n, _m.ptr(ix["p"]), ix["N"], _m.ptr(ix["o"]), _m.ptr(ix["ws"]),
                                    ix["ws"].numel(), mode, _m.ptr(counts), _m.ptr(d2), _m.ptr(nearest), st)
    _m.check(rc, "cloud_distance")
    ops.check()
    ix["ops"].check()
    assert torch.equal(before, ix["ws"])                                    # the scan only reads the index
    return d2.cpu().numpy(), nearest.cpu().numpy(), counts.cpu().numpy()


def _same(got, want):
    assert got[0].dtype == np.float64 and got[1].dtype == np.int32
    assert got[0].tobytes() == np.asarray(want[0], np.float64).tobytes()
    assert got[1].tobytes() == np.asarray(want[1], np.int32).tobytes()


@functools.lru_cache(maxsize=None)
def cloud(N, kind):
    """lattice: integer coordinates in [0, 6)^3, so duplicates and exact ties abound; random: uniform in the unit cube."""
    rng = np.random.default_rng(1000 * N + len(kind))
    if kind == "lattice":
        return rng.integers(0, 6, (N, 3)).astype(np.float32)
    return rng.uniform(0.0, 1.0, (N, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def queries(kind):
    """The largest query set; a smaller one is its head.  lattice: half-integer coordinates about the cloud's lattice,
    equidistant from several points; random: uniform about the unit cube.  Two of them far away."""
    n = max(SIZES_Q)
    rng = np.random.default_rng(7 + len(kind))
    Q = (rng.integers(-2, 14, (n, 3)) * 0.5 if kind == "lattice" else rng.uniform(-0.2, 1.2, (n, 3))).astype(np.float32)
    Q[3] += np.float32(30.0)
    Q[n // 2] -= np.float32(45.0)
    return Q


_CASES = {}


def _case(device, N, kind):
    """The cloud with its index and the numpy answer for the largest query set, built once per size."""
    if (N, kind) not in _CASES:
        P = cloud(N, kind)
        _CASES[N, kind] = (P, _build(device, P), C.nearest(queries(kind), P))
    return _CASES[N, kind]


# ----------------------------------------------------------------------------------------------------------------------
# the index and the scan against the statement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("N", SIZES_N)
def test_index_parity(device, N, kind):
    P, ix, _ = _case(device, N, kind)
    keys = C.point_keys(P)
    order = C.order_of(keys)
    tile, group = C.boxes(P, order)
    assert ix["keys"].dtype == np.int64 and ix["keys"].tobytes() == keys.tobytes()
    assert ix["order"].dtype == np.int32 and ix["order"].tobytes() == order.tobytes()
    assert ix["tile"].tobytes() == tile.tobytes() and ix["group"].tobytes() == group.tobytes()
    again = _build(device, P)                                               # run to run
    for k in ("keys", "order", "tile", "group"):
        assert again[k].tobytes() == ix[k].tobytes(), k


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("N", SIZES_N)
def test_scan_parity(device, N, kind):
    P, ix, want = _case(device, N, kind)
    Q = queries(kind)
    for n in SIZES_Q:
        for mode in MODES:
            got = _distance(device, ix, Q[:n], mode)
            _same(got, (want[0][:n], want[1][:n]))
            if mode == "plain":
                assert not got[2].any()
    if N >= T and kind == "lattice":
        two = np.sort(C.dist2_matrix(Q[:64], P), 1)[:, :2]
        assert (two[:, 0] == two[:, 1]).any()                               # the case does hold exact ties


@pytest.mark.parametrize("N", [T + 1, T * G + 1, 2 * T * G + 1])
def test_shuffled_cloud(device, N):
    """After shuffling the cloud dist2 is the same bytes and nearest names the same point - the lowest index, in the
    shuffled numbering, among the points at that distance."""
    for kind in ("lattice", "random"):
        P, ix, want = _case(device, N, kind)
        Q = queries(kind)[:BLOCK + 1]
        perm = np.random.default_rng(N).permutation(N)
        S = P[perm]
        sx = _build(device, S)
        ref = C.nearest(Q, S)
        assert ref[0].tobytes() == want[0][:len(Q)].tobytes()
        for mode in MODES:
            got = _distance(device, sx, Q, mode)
            _same(got, ref)
            m = got[1] >= 0
            assert m.all() and got[0].tobytes() == C.dist2_matrix(Q, S)[np.arange(len(Q)), got[1]].tobytes()
            if kind == "random":                                           # no two points at one distance
                assert np.array_equal(S[got[1]], P[want[1][:len(Q)]])
            else:                                                           # a tie: the lowest index of the new numbering
                assert (got[1] == np.argmin(C.dist2_matrix(Q, S), 1)).all()


def test_cpu_traps_on_the_device(device):
    q, P, want = f32_trap()
    ix = _build(device, P)
    for mode in MODES:
        d2, nn, _ = _distance(device, ix, q, mode)
        assert d2[0] == 16781312.0 and nn[0] == want
    cases = C.contraction_cases()
    assert cases
    for q, p in cases[:8]:
        ix = _build(device, p[None])
        for mode in MODES:
            d2, nn, _ = _distance(device, ix, q[None], mode)
            assert nn[0] == 0 and d2[0] == C.dist2_matrix(q[None], p[None])[0, 0] != C.dist2_fused(q, p)
    q, P, want = lattice_trap()
    ix = _build(device, P)
    assert (ix["order"][:T] >= 128).all()                                   # the higher index in the earlier tile
    for mode in MODES:
        d2, nn, _ = _distance(device, ix, q, mode)
        assert d2[0] == 16.0 and nn[0] == want
    q, P, order, want = duplicate_trap()
    ix = _build(device, P, order=order)
    for mode in MODES:
        d2, nn, _ = _distance(device, ix, q, mode)
        assert d2[0] == 0.0625 and nn[0] == want
    assert _distance(device, ix, P[200:201], 2)[1][0] == 3                  # on the duplicate itself


def test_robustness(device):
    _m, L, st = _lib()
    rng = np.random.default_rng(5)
    P = rng.uniform(0, 1, (3 * T + 5, 3)).astype(np.float32)
    bad = np.r_[0, 7, T - 1, T, 2 * T + 3, len(P) - 1]
    P[bad, [0, 1, 2, 0, 1, 2]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]
    Q = rng.uniform(-0.2, 1.2, (BLOCK + 1, 3)).astype(np.float32)
    Q[[0, 64, 200], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    Q[5], Q[6] = 1.0e6, -3.0e5                                                # far outside the box
    Q[10:20] = P[20:30]                                                       # on cloud points
    ix = _build(device, P)
    nv = len(P) - len(bad)
    assert C.valid(P)[ix["order"][:nv]].all() and not C.valid(P)[ix["order"][nv:]].any()   # the invalid points last
    want = C.nearest(Q, P)
    assert (want[1][[0, 64, 200]] == -1).all() and np.isposinf(want[0][[0, 64, 200]]).all()
    assert (want[0][10:20] == 0.0).all() and (want[1][[5, 6]] >= 0).all()
    for mode in MODES:
        got = _distance(device, ix, Q, mode)
        _same(got, want)
        assert C.valid(P)[got[1][got[1] >= 0]].all()
    # a cloud of copies of one point: the lowest index
    same = _build(device, np.repeat(P[1:2], 300, 0))
    for mode in MODES:
        d2, nn, _ = _distance(device, same, Q[1:60], mode)
        assert (nn == 0).all() and d2.tobytes() == C.nearest(Q[1:60], P[1:2])[0].tobytes()
    # no valid point, no point, no query
    for Pb in (P[bad], np.zeros((0, 3), np.float32)):
        ib = _build(device, Pb)
        assert (ib["keys"] == C.NONE).all() and np.isposinf(ib["tile"][:, :3]).all()
        for mode in MODES:
            d2, nn, _ = _distance(device, ib, Q, mode)
            assert np.isposinf(d2).all() and (nn == -1).all()
    assert _distance(device, ix, np.zeros((0, 3), np.float32), 2)[0].shape == (0,)
    # an order with entries out of range: skipped, not followed; the points it no longer names are not seen
    order = ix["order"].copy()
    drop = np.r_[3, T - 1, T, 2 * T + 7, nv - 1]
    lost = order[drop].copy()
    order[drop] = (-1, len(P), 2 ** 31 - 1, -2 ** 31, len(P) + 5)
    ib = _build(device, P, order=order)
    tile, group = C.boxes(P, order)
    assert ib["tile"].tobytes() == tile.tobytes() and ib["group"].tobytes() == group.tobytes()
    P2 = P.copy()
    P2[lost] = np.nan
    for mode in (1, 2):
        _same(_distance(device, ib, Q, mode), C.nearest(Q, P2))
    # a short workspace is refused with the size reported; so is a short index, and a bad `levels`
    need = int(L.mslam_cloud_index_bytes(len(P)))
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    args = (_m.ptr(ix["p"]), ix["N"], _m.ptr(ix["o"]), _m.ptr(ws))
    assert L.mslam_cloud_index_boxes(*args, need - 1, 0) == -3
    assert f"{need} needed" in L.mslam_last_error().decode()
    assert L.mslam_cloud_index_boxes(*args, need, 0) == 0
    q = torch.from_numpy(Q).to(device)
    d2 = torch.empty(len(Q), dtype=torch.float64, device=device)
    nr = torch.empty(len(Q), dtype=torch.int32, device=device)
    call = lambda nbytes, levels=2: L.mslam_cloud_distance(_m.ptr(q), len(Q), _m.ptr(ix["p"]), ix["N"], _m.ptr(ix["o"]),
                                                           _m.ptr(ix["ws"]), nbytes, levels, 0, _m.ptr(d2), _m.ptr(nr), 0)
    assert call(need - 1) == -3 and f"{need} needed" in L.mslam_last_error().decode()
    assert call(need, levels=3) == -1 and call(need) == 0
    torch.cuda.synchronize()
    ix["ops"].check()


def room_cloud(n_kf=4, n_pts=1000, step=80, h=96, w=128):
    """World points of the synthetic room seen from n_kf poses of the trajectory, n_pts each -> f32[n_kf * n_pts, 3]."""
    out = []
    for kf in range(n_kf):
        T_wc = synthetic.camera_pose(kf * step)
        X = synthetic.render_pointmap(T_wc, h, w).reshape(-1, 3)
        sel = np.random.default_rng(kf).permutation(len(X))[:n_pts]
        out.append(synthetic.sim3_act(T_wc, X[sel]).astype(np.float32))
    return np.concatenate(out)


def test_culling(device):
    """Two clusters of 4096 points, each inside a 1 m box, 10 m apart; the queries lie in the cluster at the lower
    coordinates, whose 32 tiles sort first.  By the time the other cluster's 32 tiles come, every query holds a finite
    best of at most 3 m^2, far below their boxes' bound of 81 m^2: every wave skips them all."""
    rng = np.random.default_rng(2)
    near, far = rng.uniform(0, 1, (4096, 3)), rng.uniform(0, 1, (4096, 3)) + [10.0, 0, 0]
    P = np.concatenate([far, near]).astype(np.float32)                     # the input order says nothing
    Q = rng.uniform(0.1, 0.9, (2 * BLOCK + 1, 3)).astype(np.float32)
    ix = _build(device, P)
    assert (ix["order"][:4096] >= 4096).all()
    want = C.nearest(Q, P)
    out = {}
    for mode in MODES:
        out[mode] = _distance(device, ix, Q, mode)
        _same(out[mode], want)
    for levels in (1, 2):
        assert out[levels][2].shape == (12,) and (out[levels][2] >= 32).all(), out[levels][2]
    # the room cloud: the skipped share of (wave, tile) scans, printed
    R = room_cloud(n_kf=6, n_pts=4000)
    rq = (R[::7] + np.float32(0.01)).astype(np.float32)
    rx = _build(device, R)
    ref = _distance(device, rx, rq, "plain")
    waves, ntiles = (len(rq) + 63) // 64, (len(R) + T - 1) // T
    for levels in (1, 2):
        got = _distance(device, rx, rq, levels)
        _same(got, ref)
        print(f"room cloud N={len(R)} n={len(rq)} levels={levels}: skipped share "
              f"{got[2][:waves].sum() / (waves * ntiles):.3f} (queries in input order)")


def test_python_distance_and_query_sorting(device):
    from mast3r_slam.tsdf import CloudIndex, cloud_distance

    P = cloud(T * G + 1, "random")
    Q = queries("random").copy()
    Q[9] = np.nan
    p, q = torch.from_numpy(P).to(device), torch.from_numpy(Q).to(device)
    want = C.nearest(Q, P)
    ix = CloudIndex(p)
    assert ix.order.dtype == torch.int32 and ix.order.cpu().numpy().tobytes() == C.order_of(C.point_keys(P)).tobytes()
    for kw in (dict(), dict(index=ix), dict(index=ix, sort_queries=False), dict(index=True)):
        d, nn = cloud_distance(q, p, **kw)
        assert d.dtype == torch.float64 and nn.dtype == torch.int32
        assert torch.equal(d, torch.sqrt(torch.from_numpy(want[0]).to(device)))
        assert nn.cpu().numpy().tobytes() == want[1].tobytes()
    with pytest.raises(ValueError, match="built for another cloud"):
        cloud_distance(q, p.clone(), index=ix)
    with pytest.raises(ValueError, match="built for another cloud"):
        cloud_distance(q, p[:-1], index=ix)
    with pytest.raises(TypeError, match="index must be"):
        cloud_distance(q, p, index="yes")
    one = torch.from_numpy(P[:1]).to(device)                                # N = 1: a zero-extent box
    assert torch.equal(cloud_distance(q, one, index=True)[0], cloud_distance(q, one)[0])


# ----------------------------------------------------------------------------------------------------------------------
# voxel downsample
# ----------------------------------------------------------------------------------------------------------------------
def _downsample_raw(device, P, col, vs):
    """mslam_cloud_voxel_keys, a stable torch.sort, the segment heads and mslam_cloud_voxel_reduce through the C entry
    points -> (centroid, count, first, color or None, keys of the voxels) numpy; guards checked."""
    _m, L, st = _lib()
    ops = Operands(device)
    P = C.f32(P)
    N = len(P)
    p = ops.put(P, np.float32)
    c = ops.put(col, np.uint8) if col is not None else None
    keys = ops.out(torch.int64, (N,))
    _m.check(L.mslam_cloud_voxel_keys(_m.ptr(p), N, vs, _m.ptr(keys), st), "cloud_voxel_keys")
    ops.check()
    assert keys.cpu().numpy().tobytes() == C.voxel_keys(P, vs).tobytes()
    sk, perm = torch.sort(keys, stable=True)
    head = sk != C.NONE
    if N > 1:
        head[1:] &= sk[1:] != sk[:-1]
    starts = torch.nonzero(head).reshape(-1)
    M = int(starts.shape[0])
    sk, perm, starts = ops.put(sk.cpu().numpy(), np.int64), ops.put(perm.cpu().numpy(), np.int64), ops.put(
        starts.cpu().numpy(), np.int64)
    cen, cnt, first = ops.out(torch.float32, (M, 3)), ops.out(torch.int32, (M,)), ops.out(torch.int32, (M,))
    color = ops.out(torch.uint8, (M, 3)) if col is not None else None
    _m.check(L.mslam_cloud_voxel_reduce(_m.ptr(p), _m.ptr(c), N, _m.ptr(sk), _m.ptr(perm), _m.ptr(starts), M,
                                        _m.ptr(cen), _m.ptr(cnt), _m.ptr(first), _m.ptr(color), st),
             "cloud_voxel_reduce")
    ops.check()
    return (cen.cpu().numpy(), cnt.cpu().numpy(), first.cpu().numpy(),
            None if color is None else color.cpu().numpy(), sk[starts].cpu().numpy())


def _voxel_cases():
    rng = np.random.default_rng(11)
    col = lambda n: rng.integers(0, 150, (n, 3)).astype(np.uint8)          # below 0xA5, the guards' fill of u8
    out = {}
    own = (np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.05 - 0.17)
    out["own"] = (rng.permutation(own).astype(np.float32), 0.03)           # every point in its own voxel
    for n in (1, 2, 257):
        out[f"one{n}"] = (rng.uniform(0.031, 0.059, (n, 3)).astype(np.float32), 0.03)    # all in one voxel
    mix = rng.uniform(-0.3, 0.3, (2000, 3)).astype(np.float32)
    mix[::50] = np.nan
    mix[7] = 3.0e30                                                         # beyond the key range
    mix[100:400] = rng.uniform(0.0, 0.03, (300, 3))                         # a crowded voxel among sparse ones
    out["mix"] = (mix, 0.03)
    out["empty"] = (np.zeros((0, 3), np.float32), 0.03)
    return {k: (P, vs, col(len(P))) for k, (P, vs) in out.items()}


@pytest.mark.parametrize("name", ["own", "one1", "one2", "one257", "mix", "empty"])
def test_downsample(device, name):
    from mast3r_slam.tsdf import downsample_cloud

    P, vs, col = _voxel_cases()[name]
    want = C.voxel_reduce(P, vs, col)
    if name == "own":
        assert (want[1] == 1).all() and len(want[1]) == len(P)
    if name.startswith("one"):
        assert want[1].tolist() == [len(P)]
    if name == "mix":
        assert want[1].max() >= 300 and (want[1] == 1).any() and want[1].sum() < len(P)
    got = _downsample_raw(device, P, col, vs)
    for g, w, dt in zip(got, want, (np.float32, np.int32, np.int32, np.uint8, np.int64)):
        assert g.dtype == dt and g.tobytes() == w.tobytes()
    assert _downsample_raw(device, P, None, vs)[3] is None
    p, c = torch.from_numpy(P).to(device), torch.from_numpy(col).to(device)
    for _ in range(2):                                                      # the Python layer, call after call
        cen, color, cnt, first = downsample_cloud(p, vs, c, return_first=True)
        for g, w in zip((cen, cnt, first, color), want):
            assert g.cpu().numpy().tobytes() == w.tobytes()
    cen2, none, cnt2 = downsample_cloud(p, vs)
    assert none is None and torch.equal(cen2, cen) and torch.equal(cnt2, cnt)
    # a shuffled input: the same voxels and counts; the centroids are the sums in the NEW index order
    perm = np.random.default_rng(3).permutation(len(P))
    S, sc = P[perm], col[perm]
    ws = C.voxel_reduce(S, vs, sc)
    assert ws[4].tobytes() == want[4].tobytes() and ws[1].tobytes() == want[1].tobytes()
    gs = _downsample_raw(device, S, sc, vs)
    for g, w in zip(gs, ws):
        assert g.tobytes() == w.tobytes()
    assert gs[3].tobytes() == want[3].tobytes()                             # integer sums: any order
    if len(P):
        assert np.abs(gs[0].astype(np.float64) - want[0]).max() <= 2.0 ** -23 * np.abs(want[0]).max()


def test_downsample_refusals(device):
    from mast3r_slam.tsdf import downsample_cloud

    p = torch.zeros((4, 3), dtype=torch.float32, device=device)
    for vs in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel must be positive"):
            downsample_cloud(p, vs)
    with pytest.raises(ValueError, match="colors must be"):
        downsample_cloud(p, 0.1, torch.zeros((3, 3), dtype=torch.uint8, device=device))
    with pytest.raises(RuntimeError, match="dtype"):
        downsample_cloud(p, 0.1, torch.zeros((4, 3), dtype=torch.float32, device=device))


# ----------------------------------------------------------------------------------------------------------------------
# ICP
# ----------------------------------------------------------------------------------------------------------------------
MOVE = A.sim3_from((5.0, (1.0, 2.0, 3.0)), (0.03, -0.03, 0.0265), 0.95)        # 5 degrees, 5 cm, scale 0.95
ICP_N, ICP_ITERS = 500, 12


@functools.lru_cache(maxsize=None)
def _icp_case():
    gt = room_cloud()
    pred = A.act(A.sim3_inv(MOVE), gt.astype(np.float64)).astype(np.float32)
    return pred, gt


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def test_align_clouds_iterations_and_recovery(device):
    """4 000 points of the synthetic room (four views) moved by 5 degrees / 5 cm / scale 0.95; 500 samples, 12
    iterations.  cloud_numpy's own run of the same iterations ends 2.6e-9 rad / 7.6e-9 m / 1.4e-9 from the truth (the
    f32 rounding of the moved cloud); the device may be ten times that, the margin test_mesh_align_gpu allows over its
    numpy run.  Every iteration: the moved sample is the statement's to an f32 ulp, its nearest neighbours and
    distances are numpy's on those very points, and the solve is numpy's Horn solve of the device's own sums."""
    from mast3r_slam.tsdf import CloudIndex, align_clouds

    pred, gt = _icp_case()
    p, g = torch.from_numpy(pred).to(device), torch.from_numpy(gt).to(device)
    src, idx = C.stride_sample(pred, ICP_N)
    trace = []
    res = align_clouds(p, g, n_samples=ICP_N, max_iters=ICP_ITERS, tol=0.0, _trace=trace)
    assert sorted(res) == ["T", "converged", "history", "inliers", "iterations", "rmse"]
    assert res["T"].dtype == torch.float64 and res["T"].is_cuda and res["history"].shape == (ICP_ITERS, 4)
    assert res["iterations"] == ICP_ITERS == len(trace)
    # tol = 0 stops only at a fixed point: exact pairs exist here, so the last two RMSEs may be the same number
    assert res["converged"] == (res["history"][-1, 1] == res["history"][-2, 1])
    assert res["rmse"] == res["history"][-1, 1] and res["inliers"] == res["history"][-1, 0] == ICP_N
    worst = 0.0
    for k, tr in enumerate(trace):
        tr = {key: v.cpu().numpy() for key, v in tr.items()}
        want_q = A.act(tr["T_before"], src.astype(np.float64))
        assert (np.abs(tr["moved"].astype(np.float64) - want_q) <= _ulp32(want_q)).all()
        st = C.icp_step(tr["T_before"], src, gt, moved=tr["moved"])
        assert tr["nearest"].tobytes() == st["nearest"].tobytes() and tr["dist2"].tobytes() == st["dist2"].tobytes()
        assert np.array_equal(tr["weights"], st["weights"].astype(np.float32)) and tr["status"][0] == C.OK
        want_T = A.horn_solve(tr["fit_log"][4:4 + A.N_SUMS], src[0].astype(np.float64), tr["dst"][0].astype(np.float64))
        diff = float(np.abs(tr["T"] - want_T).max())
        assert diff <= SOLVE_TOL, (k, diff)
        worst = max(worst, diff)
        assert res["history"][k, 0] == st["inliers"] and res["history"][k, 2] == tr["T"][7]
        assert abs(res["history"][k, 1] - st["rmse"]) <= ICP_N * 2.0 ** -52 * st["rmse"]
    T_np, hist_np = C.icp(src, gt, iters=ICP_ITERS)
    err, err_np = A.sim3_error(res["T"].cpu().numpy(), MOVE), A.sim3_error(T_np, MOVE)
    print("device (rad, m, scale) " + " ".join(f"{e:.3g}" for e in err) + "; numpy " + " ".join(
        f"{e:.3g}" for e in err_np) + f"; final rmse {res['rmse']:.3g} / {hist_np[-1, 1]:.3g}; solve within {worst:.2e}")
    assert all(e <= 10.0 * e_np for e, e_np in zip(err, err_np))
    assert np.array_equal(res["history"][:, 0], hist_np[:, 0])
    # with an index: the same transform and history, bit for bit; the stop rule from the history itself
    for index in (True, CloudIndex(g)):
        got = align_clouds(p, g, n_samples=ICP_N, max_iters=ICP_ITERS, tol=0.0, index=index)
        assert torch.equal(got["T"], res["T"]) and np.array_equal(got["history"], res["history"])
    tol = 0.5
    got = align_clouds(p, g, n_samples=ICP_N, max_iters=ICP_ITERS, tol=tol, check_every=3)
    h, it = got["history"], got["iterations"]
    change = np.abs(np.diff(h[:, 1])) / h[:-1, 1]
    assert len(h) == it and it % 3 == 0
    assert (got["converged"] and change[it - 2] <= tol) or (not got["converged"] and it == ICP_ITERS)
    # an init at the truth: one iteration changes next to nothing
    near = align_clouds(p, g, init=MOVE, n_samples=ICP_N, max_iters=1)
    assert max(A.sim3_error(near["T"].cpu().numpy(), MOVE)) <= 1e-6 and near["rmse"] <= 1e-6


def test_align_clouds_degenerate_and_refusals(device):
    from mast3r_slam.tsdf import align_clouds

    pred, gt = _icp_case()
    p, g = torch.from_numpy(pred).to(device), torch.from_numpy(gt).to(device)
    init = np.array([0.1, 0.2, 0.3, 0, 0, 0, 1, 1.5])
    res = align_clouds(p, g, init=init, trim=0.0, n_samples=100, max_iters=10, check_every=4)
    assert res["iterations"] == 4 and not res["converged"] and res["inliers"] == 0 and np.isposinf(res["rmse"])
    assert (res["history"][:, 3] == C.DEGENERATE).all() and (res["history"][:, 0] == 0).all()
    assert np.array_equal(res["T"].cpu().numpy(), init)                      # the state stays
    empty = torch.zeros((0, 3), dtype=torch.float32, device=device)
    nan = torch.full((5, 3), float("nan"), dtype=torch.float32, device=device)
    for a, b in ((p, empty), (empty, g), (nan, g), (p, nan)):
        res = align_clouds(a, b, n_samples=50, max_iters=2)
        assert res["history"][-1, 3] == C.DEGENERATE and res["inliers"] == 0
    with pytest.raises(ValueError, match="max_iters and check_every"):
        align_clouds(p, g, max_iters=0)
    with pytest.raises(ValueError, match="one value per iteration"):
        align_clouds(p, g, max_iters=3, trim=[0.1, 0.1])
    with pytest.raises(ValueError, match="trim must be"):
        align_clouds(p, g, trim=-1.0)


# ----------------------------------------------------------------------------------------------------------------------
# figures
# ----------------------------------------------------------------------------------------------------------------------
EXACT = ("accuracy_median", "completion_median", "precision", "recall", "n_pred", "n_gt", "accuracy_outliers",
         "completion_outliers", "threshold")
SUMS = ("accuracy", "completion", "accuracy_rmse", "completion_rmse")


def _check_figures(got, want):
    n = max(want["n_pred"], want["n_gt"])
    for k in EXACT:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in SUMS:
        assert abs(got[k] - want[k]) <= n * 2.0 ** -52 * want[k], (k, got[k], want[k])
    assert abs(got["chamfer"] - 0.5 * (want["accuracy"] + want["completion"])) <= n * 2.0 ** -52 * want["chamfer"]
    assert abs(got["fscore"] - want["fscore"]) <= 2.0 ** -51


def test_compare_clouds(device):
    from mast3r_slam.tsdf import CloudIndex, compare_clouds, downsample_cloud, transform_cloud

    rng = np.random.default_rng(8)
    gt = room_cloud(n_kf=3, n_pts=1500)
    pred = (room_cloud(n_kf=3, n_pts=1200, step=70) + rng.normal(0, 0.01, (3600, 3))).astype(np.float32)
    pred[::97] = np.nan
    pred[5] += np.float32(4.0)                                               # a far pair
    p, g = torch.from_numpy(pred).to(device), torch.from_numpy(gt).to(device)
    thr = 0.05
    want = C.figures(pred, gt, thr)
    got = compare_clouds(p, g, threshold=thr)
    _check_figures(got, want)
    assert got["n_pred"] == int(C.valid(pred).sum()) < len(pred) and got["accuracy_outliers"] == 0
    assert 0.0 < got["precision"] < 1.0 and 0.0 < got["recall"] < 1.0 and "alignment" not in got
    for index in (True, CloudIndex(g)):
        assert compare_clouds(p, g, threshold=thr, index=index) == got
    # max_dist moves exactly the far pairs into the outlier counts, and out of the means; precision and recall stay
    limit = 0.5
    wl = C.figures(pred, gt, thr, max_dist=limit)
    gl = compare_clouds(p, g, threshold=thr, max_dist=limit)
    _check_figures(gl, wl)
    d_acc = np.sqrt(C.nearest(pred, gt)[0])[C.valid(pred)]
    assert gl["accuracy_outliers"] == int((d_acc > limit).sum()) >= 1
    assert gl["precision"] == got["precision"] and gl["recall"] == got["recall"] and gl["accuracy"] < got["accuracy"]
    # a cloud against itself
    me = compare_clouds(g, g, threshold=thr, index=True)
    assert me["accuracy"] == me["completion"] == me["chamfer"] == 0.0 and me["fscore"] == 1.0
    # voxel= is the comparison of the two thinned clouds
    thin = compare_clouds(p, g, threshold=thr, voxel=VS)
    pp, gg = downsample_cloud(p, VS)[0], downsample_cloud(g, VS)[0]
    by_hand = compare_clouds(pp, gg, threshold=thr)
    assert {k: v for k, v in thin.items() if k != "voxel"} == {k: v for k, v in by_hand.items() if k != "voxel"}
    assert thin["voxel"] == VS and thin["n_pred"] == len(pp) < got["n_pred"]
    _check_figures(thin, C.figures(C.voxel_reduce(pred, VS)[0], C.voxel_reduce(gt, VS)[0], thr))
    # alignment: a given Sim3 is transform_cloud first; "icp" brings a moved cloud back
    moved = transform_cloud(p, A.sim3_inv(MOVE))
    given = compare_clouds(moved, g, threshold=thr, align=MOVE)
    assert given["alignment"]["rmse"] is None and given["alignment"]["T"] == list(MOVE)
    back = compare_clouds(transform_cloud(moved, MOVE), g, threshold=thr)
    assert {k: v for k, v in given.items() if k != "alignment"} == back
    icp = compare_clouds(moved, g, threshold=thr, align="icp", align_kw=dict(n_samples=1000, max_iters=30, trim=0.1),
                         index=True)
    print(f"accuracy in frame {got['accuracy']:.5f}, moved and given the Sim3 {given['accuracy']:.5f}, after ICP "
          f"{icp['accuracy']:.5f} ({icp['alignment']['iterations']} iterations)")
    assert icp["alignment"]["iterations"] >= 1 and icp["accuracy"] <= 2.0 * got["accuracy"]
    with pytest.raises(ValueError, match="no valid point"):
        compare_clouds(p[:0], g)
    with pytest.raises(ValueError, match="align_kw goes with"):
        compare_clouds(p, g, align_kw=dict(trim=1.0))
    with pytest.raises(ValueError, match="index=True"):
        compare_clouds(p, g, voxel=VS, index=CloudIndex(g))


# ----------------------------------------------------------------------------------------------------------------------
# the product
# ----------------------------------------------------------------------------------------------------------------------
def _rows(points, colors):
    """The rows (x, y, z, r, g, b) as a sorted array of byte strings: a set with multiplicity."""
    rec = np.concatenate([np.ascontiguousarray(points, np.float32).view(np.uint8).reshape(len(points), 12),
                          np.ascontiguousarray(colors, np.uint8).reshape(len(points), 3)], 1)
    return np.sort(np.ascontiguousarray(rec).view([("b", "V15")]).reshape(-1))


def test_slam_system_cloud(device, monkeypatch, tmp_path):
    """The 20-frame run of the product tests.  keyframe_cloud holds the rows save_reconstruction writes; evaluate_cloud
    against 200 000 surface samples of the room moved by a known Sim3 returns finite figures, and ICP from the
    trajectory's transform scores no worse than that transform alone plus 1e-4 m, the margin
    test_mesh_align_gpu.test_slam_system_evaluate_mesh_aligned allows the same comparison.  Measured on MI355X: 3
    keyframes, 18 580 points above confidence 2, 5 124 after thinning at 3 cm; accuracy in frame 13.533 mm (raw
    11.986 mm), by the trajectory's transform 14.300 mm, after ICP from there 13.909 mm (50 iterations)."""
    from mast3r_slam import evaluate as ev
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from mast3r_slam.tsdf import sample_mesh
    from test_slam_system_gpu import RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    move = A.sim3_from((25.0, (0.2, 1.0, 0.1)), (2.0, -1.0, 0.5), 1.6)
    s = move[7]
    rv, rf = synthetic.room_mesh()
    surface = sample_mesh(torch.from_numpy(rv).to(device), torch.from_numpy(rf).to(device), 200_000, seed=3)[0]
    moved = torch.from_numpy(A.act(move, surface.cpu().numpy().astype(np.float64)).astype(np.float32)).to(device)
    thr = 2.0                                                               # the room's confidences lie in [1, 3]
    frames = _frames(list(range(0, 60, 3)), device)
    for f in frames:
        f.uimg = torch.rand(f.uimg.shape, generator=torch.Generator().manual_seed(f.frame_id))
    try:
        system.run(frames)
        pts, col = system.keyframe_cloud(conf_threshold=thr)
        ev.save_reconstruction(tmp_path, "rec.ply", system.keyframes, thr)
        thin, thin_col = system.keyframe_cloud(conf_threshold=thr, voxel=VS)
        everything = system.keyframe_cloud(colors=False)
        in_frame = system.evaluate_cloud(surface, conf_threshold=thr)
        raw = system.evaluate_cloud(surface, conf_threshold=thr, voxel=0, index=True)
        centres = np.stack([system.keyframes[i].T_WC.data.reshape(8)[:3].cpu().numpy()
                            for i in range(len(system.keyframes))])
        gt_pos = A.act(move, centres.astype(np.float64)).astype(np.float32)
        T_traj = system.align_trajectory(gt_pos).cpu().numpy()
        kw = dict(threshold=VS * s, voxel=VS * s, conf_threshold=thr, index=True)
        by_traj = system.evaluate_cloud(moved, align=T_traj, **kw)
        icp = system.evaluate_cloud(moved, align="icp", init="trajectory", gt_positions=gt_pos,
                                    align_kw=dict(trim=0.12 * s), **kw)
        with pytest.raises(ValueError, match="gt_positions"):
            system.evaluate_cloud(moved, align="icp", init="trajectory")
        with pytest.raises(ValueError, match="go with align='icp'"):
            system.evaluate_cloud(moved, init=T_traj)
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    want_p, want_c = ev.load_ply_points(tmp_path / "rec.ply")
    assert pts.dtype == torch.float32 and col.dtype == torch.uint8 and pts.is_cuda and len(want_p) > 1000
    assert np.array_equal(_rows(pts.cpu().numpy(), col.cpu().numpy()), _rows(want_p, want_c))
    assert everything[1] is None and len(everything[0]) >= len(pts)
    assert 0 < len(thin) < len(pts) and thin_col.shape == thin.shape and thin_col.dtype == torch.uint8
    cen, _, _, color, _ = C.voxel_reduce(pts.cpu().numpy(), VS, col.cpu().numpy())
    assert thin.cpu().numpy().tobytes() == cen.tobytes() and thin_col.cpu().numpy().tobytes() == color.tobytes()
    for f in (in_frame, raw, by_traj, icp):
        assert all(np.isfinite(f[k]) for k in SUMS + ("accuracy_median", "completion_median", "fscore", "chamfer"))
    assert in_frame["voxel"] == in_frame["threshold"] == pytest.approx(tcfg["voxel_size"]) and raw["voxel"] is None
    assert raw["n_pred"] == len(pts) > in_frame["n_pred"] == len(thin) and raw["n_gt"] == 200_000
    print(f"{len(centres)} keyframes, {len(pts)} points, {len(thin)} after thinning; accuracy in frame "
          f"{in_frame['accuracy']:.6f} (raw {raw['accuracy']:.6f}) precision {in_frame['precision']:.4f}; by trajectory "
          f"{by_traj['accuracy'] / s:.6f} {by_traj['precision']:.4f}; icp from there {icp['accuracy'] / s:.6f} "
          f"{icp['precision']:.4f}, {icp['alignment']['iterations']} iterations")
    assert icp["accuracy"] / s <= by_traj["accuracy"] / s + 1e-4
    assert by_traj["alignment"]["iterations"] is None and icp["alignment"]["iterations"] >= 1
