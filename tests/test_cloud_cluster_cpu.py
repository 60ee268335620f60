"""The numpy statement of the cloud clusters (tests/cloud_cluster_numpy.py; DESIGN.md "Cloud clusters") on traps
computed by hand.  Each trap asserts the right answer and that the wrong implementation it is named after would give
another.  tests/test_cloud_cluster_gpu.py runs every trap through the kernels."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cc_numpy  # noqa: E402
import cloud_cluster_numpy as D  # noqa: E402
import cloud_numpy as C  # noqa: E402


def _line(xs):
    P = np.zeros((len(xs), 3), np.float32)
    P[:, 0] = xs
    return P


# ----------------------------------------------------------------------------------------------------------------------
# the traps: (points, eps2, min_points, labels, sizes) and what else a test needs
# ----------------------------------------------------------------------------------------------------------------------
def lattice_trap():
    """The 27 points of {0, 1, 2}^3, the centre (1, 1, 1) last -> (points, index of the centre)."""
    g = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3)
    g = np.concatenate([g[(g != 1).any(1)], [[1, 1, 1]]])
    return g.astype(np.float32), 26


def contraction_trap():
    """[(q, p, eps2, count)]: eps2 the statement's d2 where the fused sum is larger (the pair is within, fused it is
    not), and the fused sum where that is smaller (the pair is not within, fused it is)."""
    out = []
    for q, p in C.contraction_cases():
        d, fused = float(C.dist2_matrix(q[None], p[None])[0, 0]), C.dist2_fused(q, p)
        out.append((q, p, d, 1) if fused > d else (q, p, fused, 0))
    return out


def bridge_trap(tip_low="A"):
    """Two groups of four core points on a line and a point between their tips, one eps from each, eps2 = 1,
    min_points = 4: the groups' points see each other (4 or 5 within), the bridge sees itself and the two tips (3) and
    is not core.  tip_low "A": A's tip has the lower index (3 < 4); "B": B's tip has index 1, A's tip index 5, and the
    lowest index of all, 0, is still A's -> (points, eps2, min_points, labels)."""
    A, B, bridge = [-1.0, -0.75, -0.5, 0.0], [2.0, 2.5, 2.75, 3.0], 1.0
    if tip_low == "A":
        return _line(A + B + [bridge]), 1.0, 4, [0, 0, 0, 0, 1, 1, 1, 1, 0]
    #            0      1     2      3     4     5    6     7     8
    xs = [A[0], B[0], A[1], B[1], A[2], A[3], B[2], B[3], bridge]
    return _line(xs), 1.0, 4, [0, 1, 0, 1, 0, 0, 1, 1, 1]


def nearer_trap():
    """The bridge of bridge_trap with B moved 0.1 towards it: A's tip (index 3) at distance 1, B's tip (index 4) at
    about 0.9.  The bridge goes to B, the nearer, although A's core has the lower index."""
    A, B = [-1.0, -0.75, -0.5, 0.0], [1.9, 2.4, 2.65, 2.9]
    return _line(A + B + [1.0]), 1.0, 4, [0, 0, 0, 0, 1, 1, 1, 1, 1]


def chain_trap(n=7):
    return _line(np.arange(n, dtype=np.float32) * np.float32(0.25)), 0.0625        # spacing exactly eps = 0.25


def invalid_trap():
    """Six copies of the origin, a NaN, a +inf and a -inf point among them, min_points = 6."""
    P = np.zeros((9, 3), np.float32)
    P[1, 0], P[4, 1], P[7, 2] = np.nan, np.inf, -np.inf
    return P, 1.0, 6, [0, -1, 0, 0, -1, 0, 0, -1, 0]


def numbering_trap():
    """Three clusters on a line whose roots are 1, 2 and 4 (index 0 is noise, 3 a border point of the cluster of root
    2), min_points = 3, eps2 = 1: numbering by root, sizes with the border members."""
    #       0     1    2     3     4     5     6    7     8     9    10    11
    xs = [50.0, 0.0, 10.0, 12.0, 20.0, 0.5, 10.5, 1.0, 11.0, 20.5, 21.0, 0.25]
    return _line(xs), 1.0, 3, [-1, 0, 1, 1, 2, 0, 1, 0, 1, 2, 2, 0], [4, 4, 3]


# ----------------------------------------------------------------------------------------------------------------------
def test_within_means_less_or_equal():
    P, c = lattice_trap()
    assert D.radius_count(P, P, 1.0)[c] == 7                                 # itself and the six axis neighbours
    assert D.radius_count(P, P, 2.0)[c] == 19                                # and the twelve edge diagonals
    assert D.radius_count(P, P, np.nextafter(2.0, 0.0))[c] == 7              # the largest double below 2: not yet
    assert D.radius_count(P, P, 3.0)[c] == 27 and D.radius_count(P, P, 0.0).tolist() == [1] * 27
    d = C.dist2_matrix(P[c:c + 1], P)[0]
    assert int((d < 1.0).sum()) == 1 and int((d < 2.0).sum()) == 7           # THE WRONG FORM: a strict <
    many = D.radius_count(P, P, [0.0, 1.0, 2.0])
    assert many.shape == (3, 27) and many[:, c].tolist() == [1, 7, 19] and many.dtype == np.int32


def test_distance_is_bit_symmetric():
    rng = np.random.default_rng(0)
    P = (rng.uniform(-2, 2, (300, 3)) * rng.choice([1e-3, 1.0, 1e3], (300, 1))).astype(np.float32)
    d = C.dist2_matrix(P, P)
    assert d.tobytes() == np.ascontiguousarray(d.T).tobytes()
    i, j, dd = D.pairs_within(P, 1.0)                                        # asserts it block by block as well
    assert np.array_equal(dd, d[i, j]) and (dd <= 1.0).all() and len(i) == int((d <= 1.0).sum())


def test_contraction():
    cases = contraction_trap()
    assert {c[3] for c in cases} == {0, 1}                                   # both directions occur
    for q, p, eps2, want in cases:
        fused = C.dist2_fused(q, p)
        assert D.radius_count(q[None], p[None], eps2)[0] == want
        assert int(fused <= eps2) == 1 - want                                # THE WRONG FORM lands on the other side
        assert D.radius_count(p[None], q[None], eps2)[0] == want             # and the other way round: symmetric


def test_bridge_joins_nothing():
    P, eps2, mp, labels = bridge_trap()
    got = D.clusters(P, eps2, mp)
    assert got["count"].tolist() == [4, 4, 4, 5, 5, 4, 4, 4, 3]
    assert got["core"].tolist() == [True] * 8 + [False]
    assert got["labels"].tolist() == labels and got["sizes"].tolist() == [5, 4] and got["n_clusters"] == 2
    assert got["root"].tolist() == [0, 0, 0, 0, 4, 4, 4, 4, 8]
    wrong = D.clusters_through_border(P, eps2, mp)                           # THE WRONG FORM: one cluster
    assert wrong.tolist() == [0] * 9


def test_border_ties():
    # equidistant from cores of two clusters: the lower core INDEX, whichever cluster that is
    P, eps2, mp, labels = bridge_trap("A")
    got = D.clusters(P, eps2, mp)
    assert got["anchor"][8] == 3 and got["anchor_dist2"][8] == 1.0 and got["labels"][8] == 0
    d = C.dist2_matrix(P[8:9], P)[0]
    assert d[3] == d[4] == 1.0
    P, eps2, mp, labels = bridge_trap("B")
    got = D.clusters(P, eps2, mp)
    assert got["labels"].tolist() == labels and got["anchor"][8] == 1 and got["labels"][8] == 1
    assert got["root"][[0, 1]].tolist() == [0, 1]                            # not "the lower cluster": that is A, 0
    # textbook DBSCAN gives it to whoever comes first: visiting B first changes the answer, here it does not
    first_a = D.clusters_textbook(P, eps2, mp)
    first_b = D.clusters_textbook(P, eps2, mp, visit=[1, 0, 2, 3, 4, 5, 6, 7, 8])
    assert first_a[8] == first_a[0] and first_b[8] == first_b[1] and not D.same_partition(first_a, first_b)
    # unequal distances: the nearer core, although the other has the lower index
    P, eps2, mp, labels = nearer_trap()
    got = D.clusters(P, eps2, mp)
    assert got["labels"].tolist() == labels and got["anchor"][8] == 4
    assert got["anchor_dist2"][8] == C.dist2_matrix(P[8:9], P[4:5])[0, 0] < 1.0
    assert D.clusters_textbook(P, eps2, mp)[8] == 0                          # THE WRONG FORM: the first core met


def test_chain():
    P, eps2 = chain_trap()
    got = D.clusters(P, eps2, 3)
    assert got["count"].tolist() == [2, 3, 3, 3, 3, 3, 2]
    assert got["core"].tolist() == [False] + [True] * 5 + [False]
    assert got["labels"].tolist() == [0] * 7 and got["sizes"].tolist() == [7] and got["n_noise"] == 0
    assert got["anchor"].tolist() == [1, 1, 2, 3, 4, 5, 5] and got["root"].tolist() == [0, 1, 1, 1, 1, 1, 6]
    assert got["anchor_dist2"].tolist() == [0.0625, 0, 0, 0, 0, 0, 0.0625]
    none = D.clusters(P, eps2, 4)
    assert none["labels"].tolist() == [-1] * 7 and none["n_clusters"] == 0 and none["sizes"].shape == (0,)
    assert np.isposinf(none["anchor_dist2"]).all() and (none["anchor"] == -1).all()
    strict = (C.dist2_matrix(P, P) < eps2).sum(1)                            # THE WRONG FORM: nobody has a neighbour
    assert strict.tolist() == [1] * 7


def test_duplicates():
    for mp in (2, 5):
        P = np.tile(np.float32([[0.3, -0.2, 0.9]]), (mp, 1))
        for eps2 in (0.0, 1.0):
            got = D.clusters(P, eps2, mp)
            assert got["labels"].tolist() == [0] * mp and got["sizes"].tolist() == [mp]
            assert got["count"].tolist() == [mp] * mp
            assert D.clusters(P[:-1], eps2, mp)["labels"].tolist() == [-1] * (mp - 1)


def test_min_points_one():
    rng = np.random.default_rng(3)
    P = rng.uniform(0, 1, (200, 3)).astype(np.float32)
    P[[5, 50]] = np.nan
    eps2 = 0.1 ** 2
    got = D.clusters(P, eps2, 1)
    ok = C.valid(P)
    assert (got["labels"][ok] >= 0).all() and (got["labels"][~ok] == -1).all() and got["n_noise"] == 2
    i, j, _ = D.pairs_within(P, eps2)
    root = cc_numpy.labels(np.stack([i, j, j], 1), len(P))                   # the components of the eps graph
    assert np.array_equal(got["root"], root) and 1 < got["n_clusters"] < 198
    assert D.same_partition(got["labels"][ok], root[ok])


def test_invalid_points():
    P, eps2, mp, labels = invalid_trap()
    got = D.clusters(P, eps2, mp)
    assert got["labels"].tolist() == labels and got["sizes"].tolist() == [6]
    assert got["count"].tolist() == [6, 0, 6, 6, 0, 6, 6, 0, 6]              # counted by nobody, counting nobody
    assert D.radius_count(P[[1, 4, 7]], P, np.inf).tolist() == [0, 0, 0]
    assert D.radius_count(P, P[[1, 4, 7]], np.inf).tolist() == [0] * 9
    assert D.clusters(P, eps2, 7)["labels"].tolist() == [-1] * 9             # the three do not help to reach 7
    assert D.clusters(P[[1, 4, 7]], eps2, 1)["n_clusters"] == 0
    empty = D.clusters(np.zeros((0, 3), np.float32), eps2, 1)
    assert empty["labels"].shape == (0,) and empty["n_clusters"] == 0 and empty["sizes"].shape == (0,)


def test_numbering_and_sizes():
    P, eps2, mp, labels, sizes = numbering_trap()
    got = D.clusters(P, eps2, mp)
    assert got["labels"].tolist() == labels and got["sizes"].tolist() == sizes
    assert got["core"].tolist() == [False, True, True, False, True, True, True, True, True, True, True, True]
    assert np.flatnonzero(got["core"] & (got["root"] == np.arange(len(P)))).tolist() == [1, 2, 4]
    assert got["sizes"].sum() == len(P) - got["n_noise"] and got["n_noise"] == 1 and got["n_core"] == 10
    assert got["sizes"].dtype == np.int32 and got["labels"].dtype == np.int32
    # the selection rule: ties between the two clusters of four go to the lower label
    keep = lambda **kw: np.flatnonzero(D.keep_points(P, got["labels"], got["sizes"], **kw)).tolist()
    assert keep(keep_largest=1) == [1, 5, 7, 11] and keep(keep_largest=2) == [1, 2, 3, 5, 6, 7, 8, 11]
    assert keep(min_cluster_points=4) == keep(keep_largest=2) and keep(min_cluster_points=5) == []
    assert keep(min_cluster_points=4, keep_largest=0) == [] and keep() == list(range(1, 12))
    assert keep(keep_largest=1, keep_noise=True) == [0, 1, 5, 7, 11]


def test_permutation():
    rng = np.random.default_rng(9)
    blobs = [rng.normal(c, 0.05, (60, 3)) for c in ((0, 0, 0), (1, 0, 0), (0.5, 0.8, 0))]
    P = np.concatenate(blobs + [rng.uniform(-1, 2, (30, 3))]).astype(np.float32)
    eps2, mp = 0.08 ** 2, 5
    got = D.clusters(P, eps2, mp)
    assert got["n_clusters"] >= 3 and got["n_noise"] > 0 and (~got["core"] & (got["labels"] >= 0)).any()
    perm = rng.permutation(len(P))
    other = D.clusters(P[perm], eps2, mp)
    assert np.array_equal(other["count"], got["count"][perm]) and np.array_equal(other["core"], got["core"][perm])
    assert np.array_equal(other["anchor_dist2"], got["anchor_dist2"][perm])
    assert D.same_partition(other["labels"], got["labels"][perm])
    assert sorted(other["sizes"].tolist()) == sorted(got["sizes"].tolist())
    assert not D.same_partition([0, 0, 1], [0, 1, 1]) and D.same_partition([2, 2, -1, 0], [0, 0, -1, 5])
