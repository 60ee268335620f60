"""GPU tests (-m gpu) of the k nearest neighbours, the normals and the outlier filter of a point cloud
(csrc/cloud_knn.hip, mast3r_slam/tsdf/cloud.py, SlamSystem.keyframe_cloud / evaluate_cloud; DESIGN.md "Point clouds")
against the numpy statement tests/cloud_knn_numpy.py: the three forms of the scan (plain, tiles, tiles and groups) byte
for byte at the list, tile, group and block edges, the traps of tests/test_cloud_knn_cpu.py, exclusion, refusals,
robustness, culling, the normals' moments and directions, the outlier rules and the product.  Every operand of the C
entry points lies in a guarded buffer, and the guards are checked after every raw call."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from mast3r_slam import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_knn_numpy as K  # noqa: E402
import cloud_numpy as C  # noqa: E402
from mesh_support import BLOCK, G, T, VS, Operands  # noqa: E402
from test_cloud_cpu import duplicate_trap, f32_trap, lattice_trap  # noqa: E402
from test_cloud_gpu import _build, _distance, cloud, queries, room_cloud  # noqa: E402
from test_cloud_knn_cpu import duplicates_trap, kth_tie_trap  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 8, 9, 16, 17, 32)       # one, two; around the list capacities 8 and 16; the largest
SIZES_Q = (0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)
BIG = (T + 1, T * G + 1, 2 * T * G + 1)                  # a tile and a point, a group and a point, two and a point
# none, one, two; k - 1, k, k + 1 for every k; one short of a tile, a tile
SMALL = tuple(sorted({0, 1, 2, T - 1, T} | {k + d for k in KS for d in (-1, 0, 1)}))
MODES = ("plain", 1, 2)
MOMENTS = 15


def combos(N):
    """The (n, k) pairs scanned on a cloud of N points: a sparse product in which every k meets each of the three
    largest N and the three sizes around it, and every n is met."""
    if N == T + 1:
        return [(SIZES_Q[i % len(SIZES_Q)], k) for i, k in enumerate(KS)] + [(n, 9) for n in SIZES_Q]
    if N in BIG:
        ns = (65, 2 * BLOCK + 1, BLOCK, 1) if N == T * G + 1 else (BLOCK + 1, 63, 64, BLOCK - 1)
        return [(ns[i % 4], k) for i, k in enumerate(KS)]
    return [(65 if N < T - 1 else BLOCK + 1, k) for k in sorted({k for k in KS if abs(N - k) <= 1} | {3, 32})]


def _lib():
    import mslam_hip as _m

    return _m, _m.lib(), _m.stream_ptr()


def _knn(device, ix, Q, k, mode, exclude=None, keep=False):
    """mslam_cloud_knn -> (dist2, neighbors, per-wave skip counts); mode "plain" (order NULL), 1 or 2 (levels)."""
    _m, L, st = _lib()
    ops = Operands(device)
    Q = C.f32(Q)
    n = len(Q)
    q = ops.put(Q, np.float32)
    ex = ops.put(exclude, np.int32) if exclude is not None else None
    d2, nb = ops.out(torch.float64, (n, k)), ops.out(torch.int32, (n, k))
    counts = ops.out(torch.int32, (4 * ((n + BLOCK - 1) // BLOCK),))
    before = ix["ws"].clone()
    index = (0, 0, 0, 1) if mode == "plain" else (_m.ptr(ix["o"]), _m.ptr(ix["ws"]), ix["ws"].numel(), mode)
    rc = L.mslam_cloud_knn(_m.ptr(q), n, _m.ptr(ix["p"]), ix["N"], k, _m.ptr(ex), *index, _m.ptr(counts), _m.ptr(d2),
                           _m.ptr(nb), st)
    _m.check(rc, "cloud_knn")
    ops.check()
    ix["ops"].check()
    assert torch.equal(before, ix["ws"])                                    # the scan only reads the index
    return d2.cpu().numpy(), nb.cpu().numpy(), counts.cpu().numpy()


def _same(got, want):
    assert got[0].dtype == np.float64 and got[1].dtype == np.int32 and got[0].shape == got[1].shape
    assert got[0].tobytes() == np.ascontiguousarray(want[0], np.float64).tobytes()
    assert got[1].tobytes() == np.ascontiguousarray(want[1], np.int32).tobytes()


_CASES = {}


def _case(device, N, kind):
    """The cloud with its index and the statement's rows at k = 32 for the queries the cloud's combos need; the rows at
    a smaller k are their heads (the order is total), the rows of fewer queries their first rows."""
    if (N, kind) not in _CASES:
        P = cloud(N, kind)
        n = max(n for n, _ in combos(N))
        _CASES[N, kind] = (P, _build(device, P), K.knn(queries(kind)[:n], P, K.MAX_K))
    return _CASES[N, kind]


# ----------------------------------------------------------------------------------------------------------------------
# the scan against the statement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("N", SMALL + BIG)
def test_knn_parity(device, N, kind):
    P, ix, want = _case(device, N, kind)
    Q = queries(kind)
    for n, k in combos(N):
        for mode in MODES:
            got = _knn(device, ix, Q[:n], k, mode)
            _same(got, (want[0][:n, :k], want[1][:n, :k]))
            if mode == "plain":
                assert not got[2].any()
        if n and N < k:
            assert (want[1][:n, N:k] == -1).all()                           # fewer points than k: the rest is empty
    if N in BIG and kind == "lattice":
        d = want[0][:64]
        assert (d[:, 1:] == d[:, :-1]).any() and len(np.unique(P, axis=0)) < N   # the case does hold ties and duplicates


def test_statement_heads():
    """What _case relies on: the rows at k are the heads of the rows at 32."""
    P, Q = cloud(T + 1, "lattice"), queries("lattice")[:40]
    full = K.knn(Q, P, K.MAX_K)
    for k in (1, 9):
        part = K.knn(Q, P, k)
        assert part[0].tobytes() == np.ascontiguousarray(full[0][:, :k]).tobytes()
        assert part[1].tobytes() == np.ascontiguousarray(full[1][:, :k]).tobytes()


@pytest.mark.parametrize("N", [T + 1, 2 * T * G + 1])
def test_k1_is_cloud_distance(device, N):
    for kind in ("lattice", "random"):
        P, ix, _ = _case(device, N, kind)
        Q = queries(kind)[:BLOCK + 1]
        for mode in MODES:
            ref = _distance(device, ix, Q, mode)
            got = _knn(device, ix, Q, 1, mode)
            assert got[0].shape == (len(Q), 1)
            assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()


def test_cpu_traps_on_the_device(device):
    q, P, k, row = kth_tie_trap()
    ix = _build(device, P)
    for mode in MODES:
        d2, nb, _ = _knn(device, ix, q, k, mode)
        assert nb[0].tolist() == row and d2[0].tolist() == [0.0, 16.0]
        d2, nb, _ = _knn(device, ix, q, 3, mode)
        assert nb[0].tolist() == [0, 1, 129] and d2[0].tolist() == [0.0, 16.0, 16.0]
    P, plain, excluded = duplicates_trap()
    ix = _build(device, P)
    for mode in MODES:
        assert _knn(device, ix, P, 2, mode)[1].tolist() == plain
        d2, nb, _ = _knn(device, ix, P, 2, mode, exclude=np.arange(4))
        assert nb.tolist() == excluded and d2.tolist() == [[0, 1], [1, 1], [0, 1], [16, 25]]
        assert _knn(device, ix, P, 2, mode, exclude=[-1, 4, 2 ** 31 - 1, -2 ** 31])[1].tolist() == plain
    q, P, want = f32_trap()
    ix = _build(device, P)
    for mode in MODES:
        d2, nb, _ = _knn(device, ix, q, 2, mode)
        assert nb[0].tolist() == [want, 1 - want] and d2[0].tolist() == [16781312.0, 16781312.25]
    cases = C.contraction_cases()
    assert cases
    for q, p in cases[:8]:
        ix = _build(device, np.stack([p + np.float32(100.0), p]))
        for mode in MODES:
            d2, nb, _ = _knn(device, ix, q[None], 2, mode)
            assert nb[0].tolist() == [1, 0]
            assert d2[0, 0] == C.dist2_matrix(q[None], p[None])[0, 0] != C.dist2_fused(q, p)
    q, P, order, want = duplicate_trap()                                   # a given order that visits 200 before 3
    ix = _build(device, P, order=order)
    for mode in MODES:
        _same(_knn(device, ix, q, 9, mode), K.knn(q, P, 9))
        assert _knn(device, ix, q, 2, mode)[1][0].tolist() == [3, 200]


def test_exclusion(device):
    """Self-queries on the lattice cloud: every point left out of its own row, its duplicates still at distance 0;
    entries of -1 and N exclude nothing; sorted and unsorted queries give the same rows."""
    from mast3r_slam.tsdf import CloudIndex, cloud_knn

    N = T * G + 1
    P, ix, _ = _case(device, N, "lattice")
    n, k = 2 * BLOCK + 1, 9
    ex = np.arange(n, dtype=np.int32)
    ex[[5, 70]] = (-1, N)
    want = K.knn(P[:n], P, k, exclude=ex)
    own = want[1] == np.arange(n)[:, None]
    assert own[[5, 70]].any(1).all() and not np.delete(own, [5, 70], 0).any()
    assert (np.delete(want[0], [5, 70], 0)[:, 0] == 0.0).any()             # a duplicate elsewhere stays, at distance 0
    for mode in MODES:
        _same(_knn(device, ix, P[:n], k, mode, exclude=ex), want)
    p = torch.from_numpy(P).to(device)
    full = K.knn(P, P, k, exclude=np.arange(N))
    cx = CloudIndex(p)
    for kw in (dict(), dict(index=cx), dict(index=cx, sort_queries=False), dict(index=True)):
        d, nb = cloud_knn(p, p, k, exclude="self", **kw)
        assert d.dtype == torch.float64 and nb.dtype == torch.int32 and tuple(nb.shape) == (N, k)
        assert nb.cpu().numpy().tobytes() == full[1].tobytes()
        assert torch.equal(d, torch.sqrt(torch.from_numpy(full[0]).to(device)))
    e = torch.from_numpy(ex).to(device)
    for kw in (dict(index=cx), dict(index=cx, sort_queries=False)):
        nb = cloud_knn(p[:n].contiguous(), p, k, exclude=e, **kw)[1]
        assert nb.cpu().numpy().tobytes() == want[1].tobytes()
    with pytest.raises(ValueError, match="exclude='self' needs"):
        cloud_knn(p[:n].contiguous(), p, k, exclude="self")
    with pytest.raises(ValueError, match=r"k must be an integer in \[1, 32\]"):
        cloud_knn(p, p, 33)
    with pytest.raises(ValueError, match="exclude must be"):
        cloud_knn(p, p, 3, exclude=e)


def test_refusals_write_nothing(device):
    _m, L, st = _lib()
    P, ix, _ = _case(device, T + 1, "random")
    n = 70
    need = int(L.mslam_cloud_index_bytes(ix["N"]))
    for k, nbytes, rc, text in ((0, need, -1, "k must be in [1, 32]"), (33, need, -1, "k must be in [1, 32]"),
                                (-5, need, -1, "k must be"), (8, need - 1, -3, f"{need} needed")):
        ops = Operands(device)
        q = ops.put(queries("random")[:n], np.float32)
        rows = max(k, 1)
        d2, nb = ops.out(torch.float64, (n, rows)), ops.out(torch.int32, (n, rows))
        counts = ops.out(torch.int32, (4,))
        got = L.mslam_cloud_knn(_m.ptr(q), n, _m.ptr(ix["p"]), ix["N"], k, 0, _m.ptr(ix["o"]), _m.ptr(ix["ws"]), nbytes,
                                2, _m.ptr(counts), _m.ptr(d2), _m.ptr(nb), st)
        assert got == rc and text in L.mslam_last_error().decode()
        torch.cuda.synchronize()
        for g in ops.all.values():
            if g is not ops.all["0"]:
                assert bool((g.raw == g.pat).all())                        # nothing written
    ops = Operands(device)
    q = ops.put(queries("random")[:n], np.float32)
    d2, nb = ops.out(torch.float64, (n, 8)), ops.out(torch.int32, (n, 8))
    args = (_m.ptr(q), n, _m.ptr(ix["p"]), ix["N"], 8, 0, _m.ptr(ix["o"]), _m.ptr(ix["ws"]), need)
    assert L.mslam_cloud_knn(*args, 3, 0, _m.ptr(d2), _m.ptr(nb), st) == -1
    assert L.mslam_cloud_knn(*args, 2, 0, _m.ptr(d2), _m.ptr(nb), st) == 0
    ops.check()
    ix["ops"].check()


def test_robustness(device):
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
    for k in (3, 17):
        want = K.knn(Q, P, k)
        assert (want[1][[0, 64, 200]] == -1).all() and np.isposinf(want[0][[0, 64, 200]]).all()
        assert (want[0][10:20, 0] == 0.0).all() and (want[1][[5, 6]] >= 0).all()
        for mode in MODES:
            got = _knn(device, ix, Q, k, mode)
            _same(got, want)
            assert C.valid(P)[got[1][got[1] >= 0]].all()
    # a cloud of 300 copies of one point: the lowest indices, in order
    same = _build(device, np.repeat(P[1:2], 300, 0))
    for mode in MODES:
        d2, nb, _ = _knn(device, same, Q[1:60], 17, mode)
        assert (nb == np.arange(17)).all() and (d2 == d2[:, :1]).all()
        assert d2[:, 0].tobytes() == C.nearest(Q[1:60], P[1:2])[0].tobytes()
    # no valid point, no point, no query
    for Pb in (P[bad], np.zeros((0, 3), np.float32)):
        ib = _build(device, Pb)
        for mode in MODES:
            d2, nb, _ = _knn(device, ib, Q, 4, mode)
            assert np.isposinf(d2).all() and (nb == -1).all()
    assert _knn(device, ix, np.zeros((0, 3), np.float32), 5, 2)[0].shape == (0, 5)
    # a shuffled cloud: the same distances, and rows that name the same points where no two distances tie
    perm = rng.permutation(len(P))
    S = P[perm]
    sx = _build(device, S)
    want = K.knn(Q, P, 9)
    for mode in MODES:
        got = _knn(device, sx, Q, 9, mode)
        _same(got, K.knn(Q, S, 9))
        assert got[0].tobytes() == want[0].tobytes()
        distinct = (want[0][:, 1:] > want[0][:, :-1]).all(1) & (want[1] >= 0).all(1)
        assert distinct.sum() > 200 and np.array_equal(perm[got[1][distinct]], want[1][distinct])
    # an order with entries out of range: skipped, not followed; the points it no longer names are not seen
    order = ix["order"].copy()
    drop = np.r_[3, T - 1, T, 2 * T + 7, nv - 1]
    lost = order[drop].copy()
    order[drop] = (-1, len(P), 2 ** 31 - 1, -2 ** 31, len(P) + 5)
    ib = _build(device, P, order=order)
    P2 = P.copy()
    P2[lost] = np.nan
    for mode in (1, 2):
        _same(_knn(device, ib, Q, 9, mode), K.knn(Q, P2, 9))


def test_culling(device):
    """Two clusters of 4096 points, each inside a 1 m box, 10 m apart; the queries lie in the cluster at the lower
    coordinates.  After the home tile every list of k = 8 is full with a k-th best of at most 3 m^2, far below the
    bound of 81 m^2 of the other cluster's boxes: every wave skips its 32 tiles.  Without this the equality of the
    three forms would show nothing."""
    rng = np.random.default_rng(2)
    near, far = rng.uniform(0, 1, (4096, 3)), rng.uniform(0, 1, (4096, 3)) + [10.0, 0, 0]
    P = np.concatenate([far, near]).astype(np.float32)
    Q = rng.uniform(0.1, 0.9, (2 * BLOCK + 1, 3)).astype(np.float32)
    ix = _build(device, P)
    assert (ix["order"][:4096] >= 4096).all()
    want = K.knn(Q, P, 8)
    assert (want[1] >= 4096).all()
    out = {}
    for mode in MODES:
        out[mode] = _knn(device, ix, Q, 8, mode)
        _same(out[mode], want)
    for levels in (1, 2):
        assert out[levels][2].shape == (12,) and (out[levels][2] >= 32).all(), out[levels][2]
    # the room cloud in itself: the skipped share of (wave, tile) scans, printed
    R = room_cloud(n_kf=6, n_pts=4000)
    rx = _build(device, R)
    rq = R[::7].copy()
    waves, ntiles = (len(rq) + 63) // 64, (len(R) + T - 1) // T
    for k in (8, 32):
        ref = _knn(device, rx, rq, k, "plain")
        for levels in (1, 2):
            got = _knn(device, rx, rq, k, levels)
            _same(got, ref)
            print(f"room cloud N={len(R)} n={len(rq)} k={k} levels={levels}: skipped share "
                  f"{got[2][:waves].sum() / (waves * ntiles):.3f} (queries in input order)")


@pytest.mark.parametrize("layout", ["first query (nan, 0, 0)", "home tile in the last group"])
def test_home_tile_of_a_query_without_a_point(device, layout):
    """33 tiles in two groups: 32 x 128 points in a 1 m box at the low corner (tiles 0..31, group 0) and 128 points in
    a second box 10 m away (tile 32, group 1); one block of 64 queries whose first has a NaN, so the home tile is the
    one nearest to a point that no lane searches for; k = 8, tiles and groups.  The walk passes over the home tile, and
    a group that is voted away counts its tiles less the home tile when that lies in it: waves 1..3, which hold no
    query and so skip whatever they meet, count every tile but the home tile, 32, whichever group the vote removes.
      first query (nan, 0, 0)       the issue's layout: the other 63 queries lie in the far box.  The home tile lies in
        group 0, which is met first, with nothing but the home tile's own points in the lists: its box is no farther
        than they are, so the group is never voted away, and wave 0 counts only tiles of group 0 that all its lanes
        skip one by one.  It reports 0, the count of the kernel when it had its own copy of the walk (31 was expected
        there; DESIGN.md "Point clouds" has why no layout with the home tile in the first group can give it).
      home tile in the last group   the far box lies at (10, 10, 10), the first query is (nan, 10.5, 10.5), whose y
        and z pick tile 32, and the other 63 lie in the near box.  After group 0 every list is full within 3 m^2, group
        1 is voted away, and it counts 1 - 1 = 0 tiles: wave 0 reports only tiles of group 0, at most 31.
    In both layouts the counts with tiles alone, where no group is voted away, are the same."""
    rng = np.random.default_rng(11)
    issue = layout.startswith("first")
    shift = np.array([10.0, 0.0, 0.0] if issue else [10.0, 10.0, 10.0])
    near, far = rng.uniform(0, 1, (32 * T, 3)), rng.uniform(0, 1, (T, 3)) + shift
    P = np.concatenate([far, near]).astype(np.float32)                     # the input order says nothing
    Q = (rng.uniform(0.1, 0.9, (64, 3)) + (shift if issue else 0.0)).astype(np.float32)
    Q[0] = (np.nan, 0.0, 0.0) if issue else (np.nan, 10.5, 10.5)
    ix = _build(device, P)
    assert len(ix["tile"]) == 33 and len(ix["group"]) == 2 and (ix["order"][:32 * T] >= T).all()
    want = K.knn(Q, P, 8)
    assert np.isposinf(want[0][0]).all() and (want[1][0] == -1).all()
    assert ((want[1][1:] < T) == issue).all()                               # neighbours in the queries' own box
    plain = _knn(device, ix, Q, 8, "plain")
    _same(plain, want)
    got = _knn(device, ix, Q, 8, 2)
    _same(got, want)
    assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()
    print(f"{layout}: skip counts {got[2].tolist()}")
    assert got[2].shape == (4,) and (got[2][1:] == 32).all(), got[2]
    tiles = _knn(device, ix, Q, 8, 1)                                      # no group vote, the home tile passed over
    _same(tiles, want)
    assert np.array_equal(got[2], tiles[2]) and got[2][0] <= 31, (got[2], tiles[2])
    if issue:
        assert got[2][0] == 0, got[2]


# ----------------------------------------------------------------------------------------------------------------------
# normals
# ----------------------------------------------------------------------------------------------------------------------
def _normals(device, P, nb, viewpoint=None):
    """mslam_cloud_normals through the C entry point -> dict of numpy arrays; guards checked."""
    _m, L, st = _lib()
    ops = Operands(device)
    P = C.f32(P)
    N = len(P)
    nb = np.asarray(nb, np.int32).reshape(N, -1)
    k = nb.shape[1]
    p, rows = ops.put(P, np.float32), ops.put(nb, np.int32)
    vp, stride = None, 0
    if viewpoint is not None:
        v = np.asarray(viewpoint, np.float32)
        vp, stride = ops.put(v, np.float32), 3 if v.ndim == 2 else 0
    normal, curv = ops.out(torch.float32, (N, 3)), ops.out(torch.float32, (N,))
    count, mom = ops.out(torch.int32, (N,)), ops.out(torch.float64, (N, MOMENTS))
    _m.check(L.mslam_cloud_normals(_m.ptr(p), N, _m.ptr(rows), k, _m.ptr(vp), stride, _m.ptr(normal), _m.ptr(curv),
                                   _m.ptr(count), _m.ptr(mom), st), "cloud_normals")
    ops.check()                                          # a NaN curvature has other bits than the guards' pattern
    mom = mom.cpu().numpy()
    return dict(normal=normal.cpu().numpy(), curvature=curv.cpu().numpy(), count=count.cpu().numpy(),
                centroid=mom[:, :3], covariance=mom[:, 3:9], eigenvalues=mom[:, 9:12], normal64=mom[:, 12:15])


@functools.lru_cache(maxsize=None)
def wavy_sheet(N=BLOCK + 45):
    """Points of a gently curved, slightly noisy sheet: neighbourhoods with three well separated eigenvalues."""
    rng = np.random.default_rng(4)
    xy = rng.uniform(0, 1, (N, 2))
    z = 0.15 * np.sin(3.0 * xy[:, 0]) + 0.1 * xy[:, 1] ** 2 + rng.uniform(-0.002, 0.002, N)
    return np.c_[xy, z].astype(np.float32)


def test_normals_parity(device):
    """count, centroid, covariance: the statement's bytes.  The normal in f64: |n_gpu x n_stmt| <= 1e-12 where the two
    smallest eigenvalues differ by at least 1e-3 of the largest - a rounding error of ~1e-15 in the matrix over a gap of
    1e-3, by the first-order perturbation bound of an eigenvector; so the f32 normals differ by at most one rounding,
    2^-23.  Observed on MI355X: every bit of every output equal (the print below says so)."""
    P = wavy_sheet()
    k = 16
    ix = _build(device, P)
    nb = _knn(device, ix, P, k, 2)[1]
    assert nb.tobytes() == K.knn(P, P, k)[1].tobytes() and (nb[:, 0] == np.arange(len(P))).all()
    equal = []
    for vp in (None, [0.5, 0.5, 3.0], P + np.float32([0.1, -0.2, -1.0])):
        want = K.normals(P, nb, viewpoint=vp)
        lam = np.sort(want["eigenvalues"], 1)
        assert not want["degenerate"].any() and ((lam[:, 1] - lam[:, 0]) >= 1e-3 * lam[:, 2]).all()
        got = _normals(device, P, nb, viewpoint=vp)
        assert got["count"].tobytes() == want["count"].tobytes() and (got["count"] == k).all()
        assert got["centroid"].tobytes() == np.ascontiguousarray(want["centroid"]).tobytes()
        assert got["covariance"].tobytes() == np.ascontiguousarray(want["covariance"]).tobytes()
        cross = np.linalg.norm(np.cross(got["normal64"], want["normal64"]), axis=1)
        print(f"viewpoint {'none' if vp is None else np.shape(vp)}: max |n_gpu x n_stmt| {cross.max():.3g}, f64 normals "
              f"equal in every bit: {got['normal64'].tobytes() == want['normal64'].tobytes()}, eigenvalues: "
              f"{got['eigenvalues'].tobytes() == want['eigenvalues'].tobytes()}, f32 outputs: "
              f"{got['normal'].tobytes() == want['normal'].tobytes()}")
        assert (cross <= 1e-12).all()
        assert (np.sum(got["normal64"] * want["normal64"], 1) > 0.0).all()                  # and the same side
        assert np.abs(got["normal"].astype(np.float64) - want["normal"]).max() <= 2.0 ** -23
        assert np.abs(got["curvature"] - want["curvature"]).max() <= 2.0 ** -23
        assert np.abs(np.linalg.norm(got["normal64"], axis=1) - 1.0).max() <= 2.0 ** -50       # a few roundings
        equal.append(got)
    d = P.astype(np.float64)
    assert (np.sum(equal[1]["normal64"] * (np.float32([0.5, 0.5, 3.0]).astype(np.float64) - d), 1) >= 0.0).all()
    assert (np.sum(equal[2]["normal64"] * np.float32([0.1, -0.2, -1.0]).astype(np.float64), 1) > 0.0).all()
    big = np.take_along_axis(equal[0]["normal64"], np.abs(equal[0]["normal64"]).argmax(1)[:, None], 1)
    assert (big > 0.0).all()
    assert (equal[1]["normal64"][:, 2] > 0).all() and (equal[2]["normal64"][:, 2] < 0).all()   # both sides were met


def test_normals_exact_and_degenerate(device):
    from mast3r_slam.tsdf import cloud_normals

    rng = np.random.default_rng(1)
    plane = np.c_[rng.uniform(-1, 1, (BLOCK + 3, 2)), np.zeros(BLOCK + 3)].astype(np.float32)     # z = 0 exactly
    axis = {2: plane, 0: plane[:, [2, 0, 1]].copy(), 1: plane[:, [0, 2, 1]].copy()}
    for a, pts in axis.items():
        rows = K.knn(pts, pts, 8)[1]
        got = _normals(device, pts, rows)
        e = np.zeros(3, np.float32)
        e[a] = 1.0
        assert np.array_equal(got["normal"], np.tile(e, (len(pts), 1))) and (got["curvature"] == 0.0).all()
        assert (got["count"] == 8).all()
    rows = K.knn(plane, plane, 8)[1]
    assert np.array_equal(_normals(device, plane, rows, viewpoint=[0, 0, -2])["normal"][:, 2], -np.ones(len(plane)))
    # a viewpoint exactly in the tangent plane: s == 0, no flip
    assert np.array_equal(_normals(device, plane, rows, viewpoint=[9, 9, 0])["normal"][:, 2], np.ones(len(plane)))
    per_point = plane + np.float32([0, 0, -1])
    per_point[::2] = plane[::2] + np.float32([3, 0, 0])                                        # in the plane: no flip
    nz = _normals(device, plane, rows, viewpoint=per_point)["normal"][:, 2]
    assert (nz[::2] == 1.0).all() and (nz[1::2] == -1.0).all()
    # collinear, coincident, fewer than three neighbours, an invalid point: a zero normal and a NaN curvature
    line = (np.arange(12, dtype=np.float32)[:, None] * np.float32([1, 2, -1])).astype(np.float32)
    same = np.tile(np.float32([[0.3, -0.2, 0.9]]), (6, 1))
    few = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0]], np.float32)
    for pts, k, counts in ((line, 5, [5] * 12), (same, 4, [4] * 6), (few, 4, [2, 2, 0])):
        rows = K.knn(pts, pts, k)[1]
        want = K.normals(pts, rows)
        got = _normals(device, pts, rows)
        assert got["count"].tolist() == counts and not got["normal"].any() and np.isnan(got["curvature"]).all()
        assert want["degenerate"].all() and got["centroid"].tobytes() == np.ascontiguousarray(want["centroid"]).tobytes()
        assert got["covariance"].tobytes() == np.ascontiguousarray(want["covariance"]).tobytes()
    # rows with entries out of range are no neighbours
    rows = K.knn(plane, plane, 8)[1].copy()
    rows[:, 5:] = (len(plane), -7, 2 ** 31 - 1)
    got = _normals(device, plane, rows)
    assert (got["count"] == 5).all() and got["centroid"].tobytes() == K.normals(plane, rows)["centroid"].tobytes()
    # the Python layer: the same outputs in every form of the index
    P = wavy_sheet()
    p = torch.from_numpy(P).to(device)
    ref = _normals(device, P, K.knn(P, P, 16)[1], viewpoint=[0.5, 0.5, 3.0])
    for index in (None, True):
        nrm, curv, cnt = cloud_normals(p, 16, viewpoint=[0.5, 0.5, 3.0], index=index)
        assert nrm.dtype == torch.float32 and curv.dtype == torch.float32 and cnt.dtype == torch.int32
        assert nrm.cpu().numpy().tobytes() == ref["normal"].tobytes()
        assert curv.cpu().numpy().tobytes() == ref["curvature"].tobytes() and (cnt == 16).all()
    assert tuple(cloud_normals(p[:0], 4)[0].shape) == (0, 3)
    with pytest.raises(ValueError, match="viewpoint must be"):
        cloud_normals(p, 8, viewpoint=[1.0, 2.0])


# ----------------------------------------------------------------------------------------------------------------------
# outliers
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plane_with_flyers():
    """2 000 points of a jittered grid on a 1 m square of the plane z = 0 and 20 points half a metre off it."""
    rng = np.random.default_rng(6)
    g = np.stack(np.meshgrid(np.arange(50), np.arange(40), indexing="ij"), -1).reshape(-1, 2) / [50.0, 40.0]
    plane = np.c_[g + rng.uniform(0, 0.01, g.shape), np.zeros(len(g))]
    flyers = np.c_[rng.uniform(0.1, 0.9, (20, 2)), np.where(np.arange(20) % 2, 0.5, -0.5)]
    P = np.concatenate([plane, flyers]).astype(np.float32)
    where = rng.permutation(len(P))
    return P[where], np.flatnonzero(where >= 2000)


def test_outliers(device):
    from mast3r_slam.tsdf import CloudIndex, cloud_outliers, filter_cloud

    P, flyers = plane_with_flyers()
    P = P.copy()
    P[7] = np.nan
    k, ratio = 16, 2.0
    mean, scored = K.mean_distances(P, k)
    mu, sigma = K.statistics(mean, scored)
    p = torch.from_numpy(P).to(device)
    keep, info = cloud_outliers(p, k=k, std_ratio=ratio)
    assert sorted(info) == ["kept", "mean_distance", "mu", "n_valid", "sigma", "threshold"]
    assert abs(info["mu"] - mu) <= 1e-12 * mu and abs(info["sigma"] - sigma) <= 1e-12 * sigma
    assert info["threshold"] == info["mu"] + ratio * info["sigma"]
    gap = np.abs(mean[scored] - info["threshold"]).min() / info["threshold"]
    assert gap > 1e-9, gap                                                   # no mean_i at the threshold itself
    md = info["mean_distance"].cpu().numpy()
    # k square roots, each within a rounding of numpy's, summed in the same order
    assert md.dtype == np.float64 and np.array_equal(np.isnan(md), ~scored)
    assert (np.abs(md - mean)[scored] <= k * 2.0 ** -52 * mean[scored]).all()
    want = K.outliers(P, k, ratio, threshold=info["threshold"])
    got = keep.cpu().numpy()
    assert got.dtype == bool and np.array_equal(got, want)
    gone = sorted(set(flyers.tolist()) | {7})                                # the 20 go, the invalid point, nothing else
    assert np.flatnonzero(~got).tolist() == gone
    assert info["kept"] == len(P) - len(gone) == int(got.sum()) and info["n_valid"] == len(P) - 1
    print(f"mu {info['mu']:.6f} sigma {info['sigma']:.6f} threshold {info['threshold']:.6f}; closest mean_i "
          f"{gap:.3g} relative away; largest kept {mean[got].max():.6f}, smallest dropped {np.nanmin(mean[~got]):.6f}")
    for index in (None, CloudIndex(p)):
        again, other = cloud_outliers(p, k=k, std_ratio=ratio, index=index)
        assert torch.equal(again, keep) and other["threshold"] == info["threshold"]
    col = torch.arange(3 * len(P), device=device).reshape(-1, 3).to(torch.uint8)
    fp, fc, idx = filter_cloud(p, col, k=k, std_ratio=ratio)
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), np.flatnonzero(got))
    assert torch.equal(fp, p[idx]) and torch.equal(fc, col[idx]) and filter_cloud(p, k=k)[1] is None
    # the radius rule: a neighbour at a distance exactly equal to the radius counts
    L = np.zeros((5, 3), np.float32)
    L[:, 0] = [0, 1, 2, 3, 10]
    line = torch.from_numpy(L).to(device)
    for radius, mn in ((2.0, 2), (1.0, 2), (1.0, 1), (7.0, 1)):
        got = cloud_outliers(line, std_ratio=None, radius=radius, min_neighbors=mn)[0].cpu().numpy()
        assert np.array_equal(got, K.outliers(L, std_ratio=None, radius=radius, min_neighbors=mn)), (radius, mn)
    assert cloud_outliers(line, std_ratio=None, radius=2.0, min_neighbors=2)[0].tolist() == [True] * 4 + [False]
    both, info = cloud_outliers(line, k=1, std_ratio=1.9, radius=2.0, min_neighbors=2)
    assert both.tolist() == [True] * 4 + [False] and abs(info["sigma"] - np.sqrt(7.2)) <= 1e-12     # the sample sigma
    assert cloud_outliers(line, k=1, std_ratio=1.9)[0].all()
    with pytest.raises(ValueError, match="go together"):
        cloud_outliers(line, radius=1.0)
    with pytest.raises(ValueError, match="min_neighbors must be an integer"):
        cloud_outliers(line, radius=1.0, min_neighbors=33)


def test_compare_clouds_normals(device):
    from mast3r_slam.tsdf import cloud_distance, cloud_normals, compare_clouds

    rng = np.random.default_rng(8)
    gt = room_cloud(n_kf=3, n_pts=1500)
    pred = (room_cloud(n_kf=3, n_pts=1200, step=70) + rng.normal(0, 0.002, (3600, 3))).astype(np.float32)
    pred[::97] = np.nan
    p, g = torch.from_numpy(pred).to(device), torch.from_numpy(gt).to(device)
    base = compare_clouds(p, g, threshold=0.05, max_dist=0.5)
    got = compare_clouds(p, g, threshold=0.05, max_dist=0.5, normals=12)
    new = ("n_normal_pairs", "normal_consistency", "normal_consistency_accuracy", "normal_consistency_completion")
    assert sorted(got) == sorted(tuple(base) + new) and {k: got[k] for k in base} == base
    assert compare_clouds(p, g, threshold=0.05, max_dist=0.5, normals=12, index=True) == got
    # by hand, one direction
    n_p, n_g = cloud_normals(p, 12)[0].double().cpu().numpy(), cloud_normals(g, 12)[0].double().cpu().numpy()
    d, nn = (t.cpu().numpy() for t in cloud_distance(p, g))
    pair = (nn >= 0) & (d <= 0.5) & n_p.any(1) & n_g[np.maximum(nn, 0)].any(1)
    dots = np.abs(np.sum(n_p * n_g[np.maximum(nn, 0)], 1))[pair]
    assert abs(got["normal_consistency_accuracy"] - dots.mean()) <= 1e-12 and 0 < pair.sum() < got["n_normal_pairs"]
    assert got["normal_consistency"] == 0.5 * (got["normal_consistency_accuracy"] + got["normal_consistency_completion"])
    assert 0.5 < got["normal_consistency"] <= 1.0
    me = compare_clouds(g, g, normals=12)                                    # unit vectors rounded to f32
    assert abs(me["normal_consistency"] - 1.0) <= 2.0 ** -22 and 1.9 * len(gt) < me["n_normal_pairs"] <= 2 * len(gt)


# ----------------------------------------------------------------------------------------------------------------------
# the product
# ----------------------------------------------------------------------------------------------------------------------
def test_slam_system_cloud_normals(device, monkeypatch, tmp_path):
    """The 20-frame run of the product tests.  keyframe_cloud(normals=16): every non-zero normal looks at the camera
    centre of the keyframe its point came from, raw and thinned; outliers= drops points; evaluate_cloud() is the dict it
    was, evaluate_cloud(normals=16) adds the four figures.  The sanity floor of 0.9 holds against synthetic's
    ground-truth cloud of what the keyframes saw, and in the accuracy direction against 200 000 samples of the whole
    room's surface; the completion direction over the whole room does not measure normals (0.45: most of the room was
    never seen).  Measured on MI355X: see DESIGN.md "Point clouds"."""
    from mast3r_slam import evaluate as ev
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from mast3r_slam.tsdf import compare_clouds, sample_mesh
    from test_slam_system_gpu import H, W, RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    rv, rf = synthetic.room_mesh()
    surface = sample_mesh(torch.from_numpy(rv).to(device), torch.from_numpy(rf).to(device), 200_000, seed=3)[0]
    thr = 2.0
    try:
        system.run(_frames(list(range(0, 60, 3)), device))
        pts, col = system.keyframe_cloud(conf_threshold=thr)
        p3, c3, nrm = system.keyframe_cloud(conf_threshold=thr, normals=16)
        thin = system.keyframe_cloud(conf_threshold=thr, voxel=VS)
        t3, tc3, tn = system.keyframe_cloud(conf_threshold=thr, voxel=VS, normals=16)
        rule = dict(k=16, std_ratio=1.0)
        fp, fc = system.keyframe_cloud(conf_threshold=thr, voxel=VS, outliers=rule)
        fp3, _, fn3 = system.keyframe_cloud(conf_threshold=thr, voxel=VS, outliers=rule, normals=16, colors=False)
        n_kf = len(system.keyframes)
        centres = np.stack([system.keyframes[i].T_WC.data.reshape(8)[:3].cpu().numpy() for i in range(n_kf)])
        sizes = [int((system.keyframes[i].get_average_conf().reshape(-1) > thr).sum()) for i in range(n_kf)]
        plain = system.evaluate_cloud(surface, conf_threshold=thr)
        with_n = system.evaluate_cloud(surface, conf_threshold=thr, normals=16)
        filtered = system.evaluate_cloud(surface, conf_threshold=thr, outliers=rule, normals=16)
        # synthetic's ground-truth cloud: the noise-free pointmaps of the keyframes' true poses, in the world frame -
        # the part of the room the map saw (over the whole room's surface the completion direction pairs unseen walls
        # with whatever map point is nearest, and their normals have nothing to do with each other)
        poses = [synthetic.camera_pose(3 * int(system.keyframes[i].frame_id)) for i in range(n_kf)]
        seen = np.concatenate([synthetic.sim3_act(Tk, synthetic.render_pointmap(Tk, H, W).reshape(-1, 3))
                               for Tk in poses]).astype(np.float32)
        on_seen = system.evaluate_cloud(seen, conf_threshold=thr, normals=16)
        vs = float(system.tsdf_manager.volume.voxel_size)
        by_hand = compare_clouds(pts, surface, threshold=vs, voxel=vs)
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    assert torch.equal(p3, pts) and torch.equal(c3, col) and torch.equal(t3, thin[0]) and torch.equal(tc3, thin[1])
    assert nrm.dtype == torch.float32 and tuple(nrm.shape) == tuple(pts.shape) and sum(sizes) == len(pts) > 1000
    kf_of = np.repeat(np.arange(n_kf), sizes)
    first = C.voxel_reduce(pts.cpu().numpy(), VS)[2]
    for points, normals, kf in ((pts, nrm, kf_of), (t3, tn, kf_of[first])):
        n, x = normals.double().cpu().numpy(), points.double().cpu().numpy()
        live = n.any(1)
        assert live.mean() > 0.9 and np.abs(np.linalg.norm(n[live], axis=1) - 1.0).max() <= 2.0 ** -22
        assert (np.sum(n * (centres[kf].astype(np.float32).astype(np.float64) - x), 1)[live] >= 0.0).all()
    assert 0 < len(fp) < len(thin[0]) and fc.shape == fp.shape and torch.equal(fp3, fp) and fn3.shape == fp.shape
    keys = ["accuracy", "accuracy_median", "accuracy_outliers", "accuracy_rmse", "chamfer", "completion",
            "completion_median", "completion_outliers", "completion_rmse", "fscore", "max_dist", "n_gt", "n_pred",
            "precision", "recall", "threshold", "voxel"]
    assert sorted(plain) == keys and plain == by_hand
    assert {k: with_n[k] for k in keys} == plain and sorted(set(with_n) - set(keys)) == [
        "n_normal_pairs", "normal_consistency", "normal_consistency_accuracy", "normal_consistency_completion"]
    assert filtered["n_pred"] < plain["n_pred"]
    print(f"{n_kf} keyframes, {len(pts)} points, {len(thin[0])} thinned, {len(fp)} after the outlier filter; normal "
          f"consistency {with_n['normal_consistency']:.4f} (accuracy {with_n['normal_consistency_accuracy']:.4f}, "
          f"completion {with_n['normal_consistency_completion']:.4f}, {with_n['n_normal_pairs']} pairs); filtered "
          f"{filtered['normal_consistency']:.4f}, accuracy {plain['accuracy']:.5f} -> {filtered['accuracy']:.5f}; "
          f"against the {len(seen)} ground-truth points of the keyframes' views {on_seen['normal_consistency']:.4f} "
          f"(accuracy {on_seen['normal_consistency_accuracy']:.4f}, completion "
          f"{on_seen['normal_consistency_completion']:.4f}, {on_seen['n_normal_pairs']} pairs)")
    assert with_n["normal_consistency_accuracy"] > 0.9 and on_seen["normal_consistency"] > 0.9
    ev.save_cloud(tmp_path / "cloud.ply", p3, c3, nrm)
    back = ev.load_ply_points(tmp_path / "cloud.ply")
    assert back[0].tobytes() == pts.cpu().numpy().tobytes() and np.array_equal(back[1], col.cpu().numpy())
