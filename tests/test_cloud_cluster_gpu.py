"""GPU tests (-m gpu) of the radius count and the density clusters of a point cloud (csrc/cloud_cluster.hip,
mast3r_slam/tsdf/cloud_cluster.py, SlamSystem.keyframe_cloud(clusters=); DESIGN.md "Cloud clusters") against the numpy
statement tests/cloud_cluster_numpy.py: the three forms of the scan (plain, tiles, tiles and groups) byte for byte at
the tile, group and block edges, the traps of tests/test_cloud_cluster_cpu.py, a snake through every tile, the Python
layer, the floater that the point-wise rules keep, and the product.  Every operand of the C entry points lies in a
guarded buffer, and the guards are checked after every raw call."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_cluster_numpy as D  # noqa: E402
import cloud_knn_numpy as K  # noqa: E402
import cloud_numpy as C  # noqa: E402
import test_cloud_cluster_cpu as traps  # noqa: E402
from mesh_support import BLOCK, G, T, VS, Operands  # noqa: E402
from test_cloud_gpu import _build, cloud, queries  # noqa: E402

pytestmark = pytest.mark.gpu

# none, one, two; one short of a tile, a tile, one more; a group and a point; two groups and a point
SIZES_N = (0, 1, 2, T - 1, T, T + 1, T * G + 1, 2 * T * G + 1)
# none, one; around a wave; around a block; two blocks and a point
SIZES_Q = (0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)
MODES = ("plain", 1, 2)
MIN_POINTS = (1, 2, 4, 27)
# nothing but exact hits, the lattice's axis neighbours, its edge diagonals, about half the cloud (a ball of radius 5
# about queries in and around the lattice's cube of side 5, of radius 0.8 about the unit cube), everything
EPS2 = {"lattice": (0.0, 1.0, 2.0, 25.0, 1.0e30), "random": (0.0, 1.0, 2.0, 0.64, 1.0e30)}


def _lib():
    import mslam_hip as _m

    return _m, _m.lib(), _m.stream_ptr()


def _index_ops(_m, ix, mode):
    return (0, 0, 0, 1) if mode == "plain" else (_m.ptr(ix["o"]), _m.ptr(ix["ws"]), ix["ws"].numel(), mode)


def _count(device, ix, Q, eps2, mode):
    """mslam_cloud_radius_count -> (count, per-wave skip counts); mode "plain" (order NULL), 1 or 2 (levels)."""
    _m, L, st = _lib()
    ops = Operands(device)
    Q = C.f32(Q)
    n = len(Q)
    q = ops.put(Q, np.float32)
    count = ops.out(torch.int32, (n,))
    skips = ops.out(torch.int32, (4 * ((n + BLOCK - 1) // BLOCK),))
    before = ix["ws"].clone()
    rc = L.mslam_cloud_radius_count(_m.ptr(q), n, _m.ptr(ix["p"]), ix["N"], float(eps2), *_index_ops(_m, ix, mode),
                                    _m.ptr(skips), _m.ptr(count), st)
    _m.check(rc, "cloud_radius_count")
    ops.check()
    ix["ops"].check()
    assert torch.equal(before, ix["ws"])                                    # the scan only reads the index
    return count.cpu().numpy(), skips.cpu().numpy()


def _link(device, ix, eps2, core, mode, rows=None):
    """mslam_cloud_cluster_init, _link and _flatten -> (root, anchor, anchor_dist2, per-wave skip counts).  rows: None
    (self NULL: every point, in order) or the i32 list handed over as `self`."""
    _m, L, st = _lib()
    ops = Operands(device)
    N = ix["N"]
    n = N if rows is None else len(rows)
    c = ops.put(np.asarray(core, np.uint8).reshape(N), np.uint8)
    s = ops.put(rows, np.int32) if rows is not None else None
    parent = ops.out(torch.int32, (N,))
    anchor, dist2 = ops.out(torch.int32, (n,)), ops.out(torch.float64, (n,))
    skips = ops.out(torch.int32, (4 * ((n + BLOCK - 1) // BLOCK),))
    before = ix["ws"].clone()
    _m.check(L.mslam_cloud_cluster_init(N, _m.ptr(parent), st), "cloud_cluster_init")
    assert parent.cpu().numpy().tolist() == list(range(N))
    rc = L.mslam_cloud_cluster_link(_m.ptr(ix["p"]), N, _m.ptr(s), n, float(eps2), _m.ptr(c), *_index_ops(_m, ix, mode),
                                    _m.ptr(skips), _m.ptr(parent), _m.ptr(anchor), _m.ptr(dist2), st)
    _m.check(rc, "cloud_cluster_link")
    linked = parent.cpu().numpy()
    assert (linked <= np.arange(N)).all()                                   # the invariant of the union-find
    _m.check(L.mslam_cloud_cluster_flatten(N, _m.ptr(parent), st), "cloud_cluster_flatten")
    ops.check()
    ix["ops"].check()
    assert torch.equal(before, ix["ws"])
    return parent.cpu().numpy(), anchor.cpu().numpy(), dist2.cpu().numpy(), skips.cpu().numpy()


def _labels(device, root, core, anchor):
    """mslam_cloud_cluster_labels -> (label_root, is_cluster_root)."""
    _m, L, st = _lib()
    ops = Operands(device)
    N = len(root)
    r, c, a = ops.put(root, np.int32), ops.put(np.asarray(core, np.uint8), np.uint8), ops.put(anchor, np.int32)
    label_root, is_root = ops.out(torch.int32, (N,)), ops.out(torch.uint8, (N,))
    _m.check(L.mslam_cloud_cluster_labels(_m.ptr(r), _m.ptr(c), _m.ptr(a), N, _m.ptr(label_root), _m.ptr(is_root), st),
             "cloud_cluster_labels")
    ops.check()
    return label_root.cpu().numpy(), is_root.cpu().numpy()


def _same_link(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float64
    assert got[0].tobytes() == np.ascontiguousarray(want[0], np.int32).tobytes()
    assert got[1].tobytes() == np.ascontiguousarray(want[1], np.int32).tobytes()
    assert got[2].tobytes() == np.ascontiguousarray(want[2], np.float64).tobytes()


def _clusters_raw(device, P, eps2, min_points, mode, ix=None):
    """The whole chain through the C entry points, the ranking in numpy -> the dict of D.clusters."""
    ix = _build(device, P) if ix is None else ix
    P = ix["P"]
    N = len(P)
    count = _count(device, ix, P, eps2, mode)[0]
    core = C.valid(P) & (count >= min_points)
    rows = None if mode == "plain" else ix["order"]
    root, row_anchor, row_dist2, _ = _link(device, ix, eps2, core, mode, rows)
    anchor, dist2 = row_anchor, row_dist2
    if rows is not None:
        anchor, dist2 = np.empty_like(row_anchor), np.empty_like(row_dist2)
        anchor[rows], dist2[rows] = row_anchor, row_dist2
    label_root, is_root = _labels(device, root, core, anchor)
    dense = np.cumsum(is_root.astype(np.int64)) - 1
    labels = np.where(label_root >= 0, dense[np.maximum(label_root, 0)] if N else -1, -1).astype(np.int32)
    n_c = int(is_root.sum())
    return dict(count=count, core=core, root=root, anchor=anchor, anchor_dist2=dist2, labels=labels,
                sizes=np.bincount(labels[labels >= 0], minlength=n_c).astype(np.int32), n_clusters=n_c,
                n_noise=int((labels < 0).sum()), n_core=int(core.sum()))


def _same_clusters(got, want):
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        if isinstance(w, np.ndarray):
            assert got[k].dtype == w.dtype and got[k].tobytes() == w.tobytes(), k
        else:
            assert got[k] == w, k


_CASES = {}


def _case(device, N, kind):
    """The cloud with its index, built once per size."""
    if (N, kind) not in _CASES:
        P = cloud(N, kind)
        _CASES[N, kind] = (P, _build(device, P))
    return _CASES[N, kind]


def link_eps2(N, kind):
    """The radius of the link cases: the lattice's axis neighbours (and the duplicates on the point's own site); about
    six neighbours in the unit cube, 4/3 pi eps^3 N = 6."""
    return 1.0 if kind == "lattice" else float((1.5 / max(N, 2)) ** (2.0 / 3.0))


# ----------------------------------------------------------------------------------------------------------------------
# the radius count against the statement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("N", SIZES_N)
def test_radius_count_parity(device, N, kind):
    P, ix = _case(device, N, kind)
    Q = queries(kind)
    want = D.radius_count(Q, P, EPS2[kind])
    if N >= T:
        half = want[3].mean() / N
        assert 0.35 < half < 0.65, half                                      # "about half the cloud"
        assert (want[4] == N).sum() == len(Q)                               # everything
    for e, eps2 in enumerate(EPS2[kind]):
        for n in SIZES_Q:
            for mode in MODES:
                count, skips = _count(device, ix, Q[:n], eps2, mode)
                assert count.dtype == np.int32 and count.tobytes() == want[e][:n].tobytes(), (eps2, n, mode)
                if mode == "plain":
                    assert not skips.any()
    if N > T * G and kind == "lattice":
        assert want[1].max() > 32                                           # beyond the cap of the k-NN lists


def test_radius_count_culling(device):
    """Two clusters of 4096 points, each inside a 1 m box, 10 m apart (test_culling of test_cloud_gpu.py); the queries
    lie in the cluster at the lower coordinates.  With eps = 0.2 the other cluster's 32 tiles lie 81 m^2 beyond the
    bound of 0.04 m^2: every wave skips them all, and the counts are the plain scan's."""
    rng = np.random.default_rng(2)
    near, far = rng.uniform(0, 1, (4096, 3)), rng.uniform(0, 1, (4096, 3)) + [10.0, 0, 0]
    P = np.concatenate([far, near]).astype(np.float32)
    Q = rng.uniform(0.1, 0.9, (2 * BLOCK + 1, 3)).astype(np.float32)
    ix = _build(device, P)
    assert (ix["order"][:4096] >= 4096).all()
    eps2 = 0.2 * 0.2
    want = D.radius_count(Q, P, eps2)
    assert 40 < want.mean() < 400
    out = {mode: _count(device, ix, Q, eps2, mode) for mode in MODES}
    for mode in MODES:
        assert out[mode][0].tobytes() == want.tobytes()
    assert not out["plain"][1].any()
    for levels in (1, 2):
        assert out[levels][1].shape == (12,) and (out[levels][1] >= 32).all(), out[levels][1]
    # the link launch over the same index: the same rows in every form, and it skips as much
    core = C.valid(P) & (D.radius_count(P, P, eps2) >= 4)
    ref = _link(device, ix, eps2, core, "plain")
    assert not ref[3].any()
    for levels in (1, 2):
        got = _link(device, ix, eps2, core, levels)
        _same_link(got, ref)
        assert (got[3] >= 32).all(), got[3]


def test_radius_count_robustness_and_refusals(device):
    _m, L, st = _lib()
    P, eps2, _, _ = traps.invalid_trap()
    ix = _build(device, P)
    for mode in MODES:
        assert _count(device, ix, P, eps2, mode)[0].tolist() == [6, 0, 6, 6, 0, 6, 6, 0, 6]
        assert _count(device, ix, P, np.inf, mode)[0].tolist() == [6, 0, 6, 6, 0, 6, 6, 0, 6]
    bad = _build(device, P[[1, 4, 7]])
    for mode in MODES:
        assert _count(device, bad, P, np.inf, mode)[0].tolist() == [0] * 9
    for q, p, e2, want in traps.contraction_trap()[:16]:
        ix = _build(device, p[None])
        for mode in MODES:
            assert _count(device, ix, q[None], e2, mode)[0].tolist() == [want]
    P, ix = _case(device, T + 1, "random")
    need = int(L.mslam_cloud_index_bytes(ix["N"]))
    refused = ((-1.0, need, 2, -1, "eps2 must be >= 0"), (np.nan, need, 2, -1, "eps2 must"),
               (1.0, need, 3, -1, "levels must be"), (1.0, need - 1, 2, -3, f"{need} needed"))
    for eps2, nbytes, levels, rc, text in refused:
        ops = Operands(device)
        q = ops.put(queries("random")[:70], np.float32)
        count = ops.out(torch.int32, (70,))
        got = L.mslam_cloud_radius_count(_m.ptr(q), 70, _m.ptr(ix["p"]), ix["N"], eps2, _m.ptr(ix["o"]),
                                         _m.ptr(ix["ws"]), nbytes, levels, 0, _m.ptr(count), st)
        assert got == rc and text in L.mslam_last_error().decode()
        torch.cuda.synchronize()
        assert bool((ops.all["1"].raw == ops.all["1"].pat).all())            # nothing written


# ----------------------------------------------------------------------------------------------------------------------
# the link and the finish against the statement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("N", SIZES_N)
def test_link_parity(device, N, kind):
    P, ix = _case(device, N, kind)
    eps2 = link_eps2(N, kind)
    pairs = D.pairs_within(P, eps2)
    count = np.bincount(pairs[0], minlength=N).astype(np.int32)
    rng = np.random.default_rng(N)
    repeats = rng.integers(-3, N + 3, N + 70).astype(np.int32)              # repeats, gaps and entries out of range
    repeats[:4] = (-1, N, 2 ** 31 - 1, -2 ** 31)
    met = set()
    for mp in MIN_POINTS:
        core = C.valid(P) & (count >= mp)
        met.add((bool(core.any()), bool((~core).any())))
        for rows in (None, ix["order"], repeats):
            want = D.link(P, eps2, core, rows, pairs=pairs)
            first = None
            for mode in MODES:
                got = _link(device, ix, eps2, core, mode, rows)
                _same_link(got, want)
                if mode == "plain":
                    assert not got[3].any()
                    first = got
            again = _link(device, ix, eps2, core, 2, rows)                  # call after call
            _same_link(again, first)
        # the finish on the full rows
        root, anchor, _ = D.link(P, eps2, core, None, pairs=pairs)
        want = D.clusters(P, eps2, mp, pairs=pairs)
        label_root, is_root = _labels(device, root, core, anchor)
        assert is_root.dtype == np.uint8 and np.array_equal(is_root.astype(bool), core & (root == np.arange(N)))
        assert np.array_equal(label_root, np.where(anchor >= 0, root[np.maximum(anchor, 0)] if N else -1, -1))
        _same_clusters(_clusters_raw(device, P, eps2, mp, 2, ix), want)
    if N >= T and kind == "random":
        assert (True, True) in met                                          # core and other points in one cloud
    if N == 2 * T * G + 1:
        want = D.clusters(P, eps2, 4, pairs=pairs)
        assert want["n_clusters"] >= 1 and (kind == "lattice" or (want["n_noise"] > 0 and want["n_clusters"] > 3))


def test_labels_robustness(device):
    """An anchor outside [0, N) is never followed."""
    root = np.array([0, 0, 2, 3], np.int32)
    core = np.array([1, 1, 0, 1], np.uint8)
    anchor = np.array([0, 1, 4, -2 ** 31], np.int32)
    label_root, is_root = _labels(device, root, core, anchor)
    assert label_root.tolist() == [0, 0, -1, -1] and is_root.tolist() == [1, 0, 0, 1]


def test_cpu_traps_on_the_device(device):
    P, c = traps.lattice_trap()
    ix = _build(device, P)
    for mode in MODES:
        got = [_count(device, ix, P, e, mode)[0][c] for e in (1.0, 2.0, np.nextafter(2.0, 0.0), 3.0, 0.0)]
        assert got == [7, 19, 7, 27, 1]
    for trap, sizes in ((traps.bridge_trap("A"), [5, 4]), (traps.bridge_trap("B"), [4, 5]),
                        (traps.nearer_trap(), [4, 5])):
        P, eps2, mp, labels = trap
        want = D.clusters(P, eps2, mp)
        for mode in MODES:
            got = _clusters_raw(device, P, eps2, mp, mode)
            _same_clusters(got, want)
            assert got["labels"].tolist() == labels and got["sizes"].tolist() == sizes
    assert _clusters_raw(device, traps.bridge_trap("A")[0], 1.0, 4, 2)["anchor"][8] == 3
    assert _clusters_raw(device, traps.bridge_trap("B")[0], 1.0, 4, 2)["anchor"][8] == 1
    assert _clusters_raw(device, traps.nearer_trap()[0], 1.0, 4, 2)["anchor"][8] == 4
    P, eps2 = traps.chain_trap()
    for mode in MODES:
        got = _clusters_raw(device, P, eps2, 3, mode)
        _same_clusters(got, D.clusters(P, eps2, 3))
        assert got["labels"].tolist() == [0] * 7 and got["core"].tolist() == [False] + [True] * 5 + [False]
        assert _clusters_raw(device, P, eps2, 4, mode)["labels"].tolist() == [-1] * 7
    for mp in (2, 5):
        P = np.tile(np.float32([[0.3, -0.2, 0.9]]), (mp, 1))
        for mode in MODES:
            assert _clusters_raw(device, P, 0.0, mp, mode)["labels"].tolist() == [0] * mp
            assert _clusters_raw(device, P[:-1], 0.0, mp, mode)["labels"].tolist() == [-1] * (mp - 1)
    P, eps2, mp, labels = traps.invalid_trap()
    for mode in MODES:
        got = _clusters_raw(device, P, eps2, mp, mode)
        _same_clusters(got, D.clusters(P, eps2, mp))
        assert got["labels"].tolist() == labels
        assert _clusters_raw(device, P, eps2, 7, mode)["n_clusters"] == 0
    P, eps2, mp, labels, sizes = traps.numbering_trap()
    for mode in MODES:
        got = _clusters_raw(device, P, eps2, mp, mode)
        assert got["labels"].tolist() == labels and got["sizes"].tolist() == sizes
    # min_points = 1 and a permuted cloud
    rng = np.random.default_rng(3)
    P = rng.uniform(0, 1, (300, 3)).astype(np.float32)
    P[[5, 50]] = np.nan
    for mp in (1, 5):
        want = D.clusters(P, 0.01, mp)
        perm = rng.permutation(len(P))
        for mode in MODES:
            got = _clusters_raw(device, P, 0.01, mp, mode)
            _same_clusters(got, want)
            other = _clusters_raw(device, P[perm], 0.01, mp, mode)
            assert D.same_partition(other["labels"], got["labels"][perm])
        if mp == 1:
            assert want["n_noise"] == 2 and (want["labels"][C.valid(P)] >= 0).all()


@functools.lru_cache(maxsize=None)
def snake():
    """A helix of 2 T G + 1 = 8193 points, 64 to a turn of radius 1 and 0.3 up per turn: a point's two chain neighbours
    lie 0.098 away, the next ones 0.196 and the turns above and below 0.3; eps = 0.11.  The indices are shuffled."""
    n = 2 * T * G + 1
    t = np.arange(n) * (2.0 * np.pi / 64.0)
    H = np.stack([np.cos(t), np.sin(t), 0.3 * np.arange(n) / 64.0], 1).astype(np.float32)
    perm = np.random.default_rng(8193).permutation(n)
    return H[perm], perm, 0.11 * 0.11


def test_snake(device):
    """One cluster through every tile, group and block edge, with deep union-find trees: every point is within eps of
    its two chain neighbours only, so the component is one path of 8192 links whatever order they land in.  A
    correctness case, run once per form: it ends by the invariant parent[v] <= v."""
    P, perm, eps2 = snake()
    N = len(P)
    pairs = D.pairs_within(P, eps2)
    count = np.bincount(pairs[0], minlength=N)
    ends = np.flatnonzero((perm == 0) | (perm == N - 1))
    assert (np.delete(count, ends) == 3).all() and (count[ends] == 2).all()  # itself and the two chain neighbours
    ix = _build(device, P)
    want = D.clusters(P, eps2, 2, pairs=pairs)
    assert want["n_clusters"] == 1 and (want["root"] == 0).all() and want["sizes"].tolist() == [N]
    for mode in MODES:
        got = _clusters_raw(device, P, eps2, 2, mode, ix)
        _same_clusters(got, want)
        assert (got["root"] == 0).all() and (got["labels"] == 0).all()
    # min_points = 3: the two ends are border points of the same cluster, whose root is the lowest core index
    want = D.clusters(P, eps2, 3, pairs=pairs)
    got = _clusters_raw(device, P, eps2, 3, 2, ix)
    _same_clusters(got, want)
    lowest_core = int(np.flatnonzero(want["core"])[0])
    assert (got["labels"] == 0).all() and not got["core"][ends].any() and got["root"][lowest_core] == lowest_core
    assert (np.delete(got["root"], ends) == lowest_core).all()


# ----------------------------------------------------------------------------------------------------------------------
# the Python layer
# ----------------------------------------------------------------------------------------------------------------------
def test_python_radius_count(device):
    from mast3r_slam.tsdf import CloudIndex, cloud_radius_count

    P = cloud(T * G + 1, "random")
    Q = queries("random").copy()
    Q[9] = np.nan
    p, q = torch.from_numpy(P).to(device), torch.from_numpy(Q).to(device)
    radius = 0.3
    want = D.radius_count(Q, P, radius * radius)
    assert want[9] == 0 and want.max() > 32
    cx = CloudIndex(p)
    for kw in (dict(), dict(index=cx), dict(index=cx, sort_queries=False), dict(index=True)):
        got = cloud_radius_count(q, p, radius, **kw)
        assert got.dtype == torch.int32 and got.cpu().numpy().tobytes() == want.tobytes()
    assert cloud_radius_count(q, p, 0.0).cpu().numpy().tobytes() == D.radius_count(Q, P, 0.0).tobytes()
    assert tuple(cloud_radius_count(q[:0], p, 1.0).shape) == (0,) and not cloud_radius_count(q, p[:0], 1.0).any()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius must be finite"):
            cloud_radius_count(q, p, bad)
    with pytest.raises(ValueError, match="built for another cloud"):
        cloud_radius_count(q, p.clone(), 1.0, index=cx)
    with pytest.raises(TypeError, match="index must be"):
        cloud_radius_count(q, p, 1.0, index="yes")


def test_python_clusters(device):
    from mast3r_slam.tsdf import CloudIndex, cloud_clusters, filter_cloud_clusters

    rng = np.random.default_rng(9)
    blobs = [rng.normal(c, 0.05, (300, 3)) for c in ((0, 0, 0), (1, 0, 0), (0.5, 0.8, 0))]
    P = np.concatenate(blobs + [rng.uniform(-1, 2, (200, 3))]).astype(np.float32)
    P = P[rng.permutation(len(P))]
    P[[3, 400]] = np.nan
    eps, mp = 0.06, 8
    want = D.clusters(P, eps * eps, mp)
    assert want["n_clusters"] >= 3 and want["n_noise"] > 50 and (~want["core"] & (want["labels"] >= 0)).any()
    p = torch.from_numpy(P).to(device)
    for index in (True, None, CloudIndex(p)):
        labels, info = cloud_clusters(p, eps, mp, index=index)
        assert sorted(info) == ["core", "count", "n_clusters", "n_core", "n_noise", "sizes"]
        assert labels.dtype == torch.int32 and labels.cpu().numpy().tobytes() == want["labels"].tobytes()
        assert info["sizes"].dtype == torch.int32 and info["sizes"].cpu().numpy().tobytes() == want["sizes"].tobytes()
        assert info["core"].dtype == torch.bool and np.array_equal(info["core"].cpu().numpy(), want["core"])
        assert info["count"].dtype == torch.int32 and info["count"].cpu().numpy().tobytes() == want["count"].tobytes()
        assert (info["n_clusters"], info["n_noise"], info["n_core"]) == (want["n_clusters"], want["n_noise"],
                                                                         want["n_core"])
    big = cloud_clusters(p, eps, 5000)                                       # no upper limit: nothing is core
    assert (big[0] == -1).all() and big[1]["n_clusters"] == 0 and tuple(big[1]["sizes"].shape) == (0,)
    # the filter against the statement's rule
    col = torch.from_numpy(rng.integers(0, 255, (len(P), 3)).astype(np.uint8)).to(device)
    for kw in (dict(), dict(keep_largest=1), dict(keep_largest=2, keep_noise=True), dict(min_cluster_points=290),
               dict(min_cluster_points=290, keep_largest=0), dict(min_cluster_points=10 ** 6, keep_noise=True)):
        keep = D.keep_points(P, want["labels"], want["sizes"], **kw)
        fp, fc, idx = filter_cloud_clusters(p, col, eps=eps, min_points=mp, **kw)
        assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), np.flatnonzero(keep)), kw
        assert torch.equal(fp, p[idx]) and torch.equal(fc, col[idx])
    assert not np.isnan(filter_cloud_clusters(p, eps=eps, min_points=mp, keep_noise=True)[0].cpu().numpy()).any()
    assert filter_cloud_clusters(p, eps=eps, min_points=mp)[1] is None
    # ties between equal sizes go to the lower label
    L, eps2, mpl, labels, sizes = traps.numbering_trap()
    line = torch.from_numpy(L).to(device)
    got_labels, info = cloud_clusters(line, 1.0, mpl)
    assert got_labels.tolist() == labels and info["sizes"].tolist() == sizes
    assert filter_cloud_clusters(line, eps=1.0, min_points=mpl, keep_largest=1)[2].tolist() == [1, 5, 7, 11]
    assert filter_cloud_clusters(line, eps=1.0, min_points=mpl, keep_largest=1, keep_noise=True)[2].tolist() == [
        0, 1, 5, 7, 11]
    # an empty cloud, a cloud without a valid point
    for q in (p[:0], torch.full((5, 3), float("nan"), dtype=torch.float32, device=device)):
        for index in (True, None):
            labels, info = cloud_clusters(q, eps, 1, index=index)
            assert labels.dtype == torch.int32 and (labels == -1).all() and len(labels) == len(q)
            assert info["n_clusters"] == 0 and info["n_noise"] == len(q) and tuple(info["sizes"].shape) == (0,)
            fp, fc, idx = filter_cloud_clusters(q, eps=eps, min_points=1, keep_noise=True, index=index)
            assert tuple(fp.shape) == (0, 3) and fc is None and tuple(idx.shape) == (0,)
    # refusals
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps must be positive and finite"):
            cloud_clusters(p, bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="min_points must be an integer >= 1"):
            cloud_clusters(p, eps, bad)
    with pytest.raises(ValueError, match="eps must be given"):
        filter_cloud_clusters(p)
    with pytest.raises(ValueError, match="keep_largest must be >= 0"):
        filter_cloud_clusters(p, eps=eps, keep_largest=-1)
    with pytest.raises(ValueError, match="colors must be"):
        filter_cloud_clusters(p, col[:-1], eps=eps)
    with pytest.raises(ValueError, match="built for another cloud"):
        cloud_clusters(p.clone(), eps, index=CloudIndex(p))


# ----------------------------------------------------------------------------------------------------------------------
# the floater
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wall_with_floater():
    """A wall of 64 x 64 points at 2 cm spacing, a blob of 4 x 4 x 4 points at 2 cm spacing one metre in front of it,
    and five points on their own, shuffled -> (points, indices of the wall, of the blob, of the five)."""
    s = 0.02
    wall = np.stack(np.meshgrid(np.arange(64), np.arange(64), [0], indexing="ij"), -1).reshape(-1, 3) * s
    blob = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3) * s + [0.6, 0.6, 1.0]
    lone = np.array([[0.2, 0.3, 0.5], [1.0, 0.1, 0.4], [0.3, 1.1, 0.7], [-0.4, 0.6, 0.3], [0.7, 0.2, 1.6]])
    P = np.concatenate([wall, blob, lone]).astype(np.float32)
    where = np.random.default_rng(64).permutation(len(P))
    inv = np.argsort(where)                                                  # P[where][inv[k]] is row k of the stack
    return P[where], np.sort(inv[:4096]), np.sort(inv[4096:4160]), np.sort(inv[4160:])


def test_floater(device):
    """What no point-wise rule can say: the blob is dense - each of its points has 7 to 27 neighbours within 3 cm - so
    cloud_outliers keeps it, and only "this piece is not attached to the scene" removes it.  eps = 3 cm takes in the
    grid's diagonal (2.83 cm) and not the next spacing (4 cm); the smallest neighbourhood, a wall corner, holds 4."""
    from mast3r_slam.tsdf import cloud_clusters, cloud_outliers, filter_cloud_clusters

    P, wall, blob, lone = wall_with_floater()
    # the premise, on the CPU first: the statistical rule at its defaults keeps points of the blob
    assert K.outliers(P, 16, 2.0)[blob].any()
    p = torch.from_numpy(P).to(device)
    kept = cloud_outliers(p)[0].cpu().numpy()
    assert kept[blob].all()                                                  # the point-wise rule sees nothing wrong
    radius_rule = cloud_outliers(p, std_ratio=None, radius=0.03, min_neighbors=6)[0].cpu().numpy()
    assert radius_rule[blob].all() and not radius_rule[wall].all()           # the radius rule eats the wall's rim first
    eps, mp = 0.03, 4
    want = D.clusters(P, eps * eps, mp)
    assert want["count"][wall].min() == 4 and want["count"][blob].min() == 7 and (want["count"][lone] == 1).all()
    labels, info = cloud_clusters(p, eps, mp)
    assert labels.cpu().numpy().tobytes() == want["labels"].tobytes()
    assert info["n_clusters"] == 2 and info["n_noise"] == 5 and sorted(info["sizes"].tolist()) == [64, 4096]
    got = labels.cpu().numpy()
    assert len(set(got[wall])) == 1 and len(set(got[blob])) == 1 and got[wall][0] != got[blob][0] >= 0
    assert (got[lone] == -1).all()
    fp, fc, idx = filter_cloud_clusters(p, eps=eps, min_points=mp, keep_largest=1)
    assert fc is None and np.array_equal(idx.cpu().numpy(), wall)
    assert torch.equal(fp, p[torch.from_numpy(wall).to(device)])
    fp, _, idx = filter_cloud_clusters(p, eps=eps, min_points=mp, min_cluster_points=100)
    assert np.array_equal(idx.cpu().numpy(), wall)


# ----------------------------------------------------------------------------------------------------------------------
# the product
# ----------------------------------------------------------------------------------------------------------------------
def test_slam_system_cloud_clusters(device, monkeypatch):
    """The 20-frame run of the product tests.  keyframe_cloud(clusters=None) returns what keyframe_cloud() returns, byte
    for byte; with clusters= the cloud is the statement's selection of the unfiltered one, in order, and every non-zero
    normal still looks at the camera centre of the keyframe its point came from."""
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from test_slam_system_gpu import RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    thr = 2.0
    rule = dict(eps=2.5 * VS, min_points=4, keep_largest=1)
    try:
        system.run(_frames(list(range(0, 60, 3)), device))
        plain = system.keyframe_cloud(conf_threshold=thr)
        none = system.keyframe_cloud(conf_threshold=thr, clusters=None)
        thin = system.keyframe_cloud(conf_threshold=thr, voxel=VS)
        thin_none = system.keyframe_cloud(conf_threshold=thr, voxel=VS, clusters=None)
        u3 = system.keyframe_cloud(conf_threshold=thr, voxel=VS, normals=16)
        f3 = system.keyframe_cloud(conf_threshold=thr, voxel=VS, clusters=rule, normals=16)
        f2 = system.keyframe_cloud(conf_threshold=thr, voxel=VS, clusters=rule)
        n_kf = len(system.keyframes)
        centres = np.stack([system.keyframes[i].T_WC.data.reshape(8)[:3].cpu().numpy() for i in range(n_kf)])
        sizes = [int((system.keyframes[i].get_average_conf().reshape(-1) > thr).sum()) for i in range(n_kf)]
        scored = system.evaluate_cloud(thin[0], conf_threshold=thr, clusters=dict(rule, eps=2.5 * float(
            system.tsdf_manager.volume.voxel_size)), voxel=0)
        unscored = system.evaluate_cloud(thin[0], conf_threshold=thr, voxel=0)
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    assert len(plain) == len(none) == len(thin) == len(thin_none) == 2 and len(u3) == len(f3) == 3
    for a, b in zip(plain + thin, none + thin_none):
        assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    U, F = u3[0].cpu().numpy(), f3[0].cpu().numpy()
    assert torch.equal(u3[0], thin[0]) and len(F) == len(f3[1]) == len(f3[2]) and f3[2].dtype == torch.float32
    assert torch.equal(f2[0], f3[0]) and torch.equal(f2[1], f3[1])
    want = D.clusters(U, (2.5 * VS) ** 2, 4)
    keep = np.flatnonzero(D.keep_points(U, want["labels"], want["sizes"], keep_largest=1))
    assert 0 < len(keep) == want["sizes"].max() <= len(U)
    assert F.tobytes() == U[keep].tobytes()                                  # a subset, in order
    assert f3[1].cpu().numpy().tobytes() == u3[1].cpu().numpy()[keep].tobytes()
    kf_of = np.repeat(np.arange(n_kf), sizes)[C.voxel_reduce(plain[0].cpu().numpy(), VS)[2]][keep]
    n, x = f3[2].double().cpu().numpy(), F.astype(np.float64)
    live = n.any(1)
    assert live.mean() > 0.9 and np.abs(np.linalg.norm(n[live], axis=1) - 1.0).max() <= 2.0 ** -22
    assert (np.sum(n * (centres[kf_of].astype(np.float32).astype(np.float64) - x), 1)[live] >= 0.0).all()
    assert scored["n_pred"] <= unscored["n_pred"] and scored["n_pred"] > 0
    print(f"{n_kf} keyframes, {len(plain[0])} points, {len(U)} thinned, {want['n_clusters']} clusters, "
          f"{want['n_noise']} noise points, {len(F)} kept by keep_largest=1")
