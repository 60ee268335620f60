"""CPU tests of the statement of the cloud smoothing step (tests/cloud_mls_numpy.py; DESIGN.md "Cloud smoothing") on
hand-computed traps, each of which separates the right answer from a named wrong one, and the product property on the
corner fixture.  tests/test_cloud_mls_gpu.py runs the same traps through the kernel."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_mls_numpy as M  # noqa: E402

F = np.float32


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ----------------------------------------------------------------------------------------------------------------------
# the traps: every coordinate, weight and sum below is a dyadic number of a few bits, so the arithmetic is exact
# ----------------------------------------------------------------------------------------------------------------------
def plane_trap(above=True):
    """Four points on the plane z = 0.5 at (0.25 +- 0.5, 0.5 +- 0.5), the query over (or under) their centre at height
    0.375 from the plane; h2 = 1.  d2 = 0.640625, u = 0.359375, w = u u for all four; m = (0, 0, -+0.375) and
    C = diag(0.25, 0.25, 0), so the normal is e_z, t = -+0.375 and the query lands on (0.25, 0.5, 0.5) exactly.
    -> (Q, P, h2, the landing point)."""
    P = F([[-0.25, 0.0, 0.5], [0.75, 0.0, 0.5], [-0.25, 1.0, 0.5], [0.75, 1.0, 0.5]])
    Q = F([[0.25, 0.5, 0.875 if above else 0.125]])
    return Q, P, 1.0, F([[0.25, 0.5, 0.5]])


def rim_trap():
    """plane_trap with a fifth point at exactly d2 == h2 = 1 from the query, one unit along x: it counts (5, not 4) with
    weight 0, so min_points = 5 moves the query - a strict < would leave it - and no bit of the sums changes."""
    Q, P, h2, land = plane_trap()
    return Q, np.concatenate([P, Q + F([1.0, 0.0, 0.0])]), h2, land


def line_trap():
    """Four collinear points within the radius: the covariance has rank 1, the middle eigenvalue is 0."""
    return F([[0.0, 0.0, 0.25]]), F([[-0.5, 0, 0], [-0.25, 0, 0], [0.25, 0, 0], [0.5, 0, 0]]), 1.0


def gate_trap():
    """plane_trap with the normal e_z on its four points, and a fifth point on the axis between the query and the plane
    whose normal (0.6, 0, 0.8) makes the f64 cosine float(f32(0.8)) with e_z.  -> (Q, P, h2, landing point, query normal,
    point normals, that cosine)."""
    Q, P, h2, land = plane_trap()
    P = np.concatenate([P, F([[0.25, 0.5, 0.75]])])
    pn = F([[0, 0, 1]] * 4 + [[0.6, 0.0, 0.8]])
    return Q, P, h2, land, F([[0, 0, 1]]), pn, float(F(0.8))


def test_lands_on_the_plane_exactly():
    """Against p - t n (the wrong sign: 1.25 and -0.25), |t| (a query under the plane moves away) and a normal left at
    -e_z."""
    for above in (True, False):
        Q, P, h2, land = plane_trap(above)
        out = M.mls_step(Q, P, h2, 4, 1.0)
        assert bits(out["points"]) == bits(land) and out["moved"].tolist() == [True] and out["count"].tolist() == [4]
        assert bits(out["normals"]) == bits(F([[0, 0, 1]])) and bits(out["curvature"]) == bits(F([0.0]))
        mom = out["moments"][0]
        w = 0.359375 * 0.359375
        assert mom[0] == 4 * w and mom[1:4].tolist() == [0.0, 0.0, (-1.0 if above else 1.0) * 0.375 * 4 * w]
        assert mom[10:13].tolist() == [0.25, 0.25, 0.0] and mom[13:16].tolist() == [0.0, 0.0, 1.0]
        assert mom[16] == (-0.375 if above else 0.375) and mom[17] == 0.0


def test_a_neighbour_on_the_rim_counts_with_weight_zero():
    """Against d2 < h2 and against "weight 0 means left out"."""
    Q, P, h2, land = rim_trap()
    ref = M.mls_step(Q, P[:4], h2, 4, 1.0)
    out = M.mls_step(Q, P, h2, 5, 1.0)
    assert out["count"].tolist() == [5] and out["moved"].tolist() == [True] and bits(out["points"]) == bits(land)
    assert bits(out["moments"]) == bits(ref["moments"])
    first = M.mls_step(Q, P, h2, 5, 1.0, order=[4, 0, 1, 2, 3])          # met first: 0 + (-0) is still +0
    assert bits(first["moments"]) == bits(ref["moments"])
    # the same point one step of the last place outside: d2 > h2, it does not count and the query stays
    far = P.copy()
    far[4, 0] = np.nextafter(far[4, 0], F(np.inf))
    out = M.mls_step(Q, far, h2, 5, 1.0)
    assert out["count"].tolist() == [4] and out["moved"].tolist() == [False] and bits(out["points"]) == bits(Q)


def test_min_points_decides():
    """count == min_points - 1 stays with its input bits, normal 0 and curvature NaN; count == min_points moves."""
    Q, P, h2, land = plane_trap()
    stay = M.mls_step(Q, P, h2, 5, 1.0)
    assert stay["count"].tolist() == [4] and bits(stay["points"]) == bits(Q) and not stay["moved"][0]
    assert bits(stay["normals"]) == bits(F([[0, 0, 0]])) and np.isnan(stay["curvature"][0])
    assert stay["moments"][0, 13:].tolist() == [0.0] * 5 and stay["moments"][0, 0] > 0.0
    assert bits(M.mls_step(Q, P, h2, 4, 1.0)["points"]) == bits(land)
    # three points are a plane, two are not, whatever min_points says
    assert M.mls_step(Q, P[:3], h2, 1, 1.0)["moved"].tolist() == [True]
    two = M.mls_step(Q, P[:2], h2, 1, 1.0)
    assert two["count"].tolist() == [2] and not two["moved"][0] and bits(two["points"]) == bits(Q)


def test_collinear_and_coincident_neighbourhoods_stay():
    Q, P, h2 = line_trap()
    out = M.mls_step(Q, P, h2, 1, 1.0)
    assert out["count"].tolist() == [4] and not out["moved"][0] and bits(out["points"]) == bits(Q)
    assert bits(out["normals"]) == bits(F([[0, 0, 0]])) and np.isnan(out["curvature"][0])
    lam = np.sort(out["moments"][0, 10:13])
    assert lam[0] == 0.0 and lam[1] == 0.0 and lam[2] > 0.0
    # duplicates all count, and five copies of one point span nothing
    dup = np.tile(F([[0.25, 0.5, 0.5]]), (5, 1))
    out = M.mls_step(F([[0.25, 0.5, 0.75]]), dup, 1.0, 1, 1.0)
    assert out["count"].tolist() == [5] and not out["moved"][0] and np.isnan(out["curvature"][0])
    Q, P, h2, land = plane_trap()
    out = M.mls_step(Q, np.concatenate([P, P]), h2, 8, 1.0)                   # every point twice: count 8, the same plane
    assert out["count"].tolist() == [8] and bits(out["points"]) == bits(land)
    # a neighbourhood that lies on the rim altogether has S0 = 0: no plane
    rim = Q + F([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]])
    out = M.mls_step(Q, rim, 1.0, 1, 1.0)
    assert out["count"].tolist() == [4] and not out["moved"][0] and out["moments"][0, 0] == 0.0
    assert not np.isnan(out["moments"]).any()


def test_invalid_queries_and_points():
    """A NaN query keeps its payload and counts nothing; NaN points of the cloud are no neighbours."""
    Q, P, h2, land = plane_trap()
    odd = np.array([0x7FC12345, 0x3F000000, 0x3F000000], np.uint32).view(np.float32)[None]
    Q2 = np.concatenate([odd, Q, F([[np.inf, 0, 0]])])
    P2 = np.concatenate([F([[np.nan, 0.5, 0.5]]), P, F([[0.25, 0.5, -np.inf]])])
    out = M.mls_step(Q2, P2, h2, 4, 1.0)
    assert bits(out["points"][0]) == bits(odd[0]) and bits(out["points"][2]) == bits(Q2[2])
    assert out["count"].tolist() == [0, 4, 0] and out["moved"].tolist() == [False, True, False]
    assert bits(out["points"][1]) == bits(land[0])
    assert bits(out["moments"][1]) == bits(M.mls_step(Q, P, h2, 4, 1.0)["moments"][0])
    assert not out["moments"][[0, 2]].any()
    # no neighbour within the radius: the sums are the +0 they started from, also where w r would be -0
    lone = M.mls_step(F([[5, 5, 5]]), P, h2, 1, 1.0)
    assert lone["count"].tolist() == [0] and bits(lone["moments"]) == bits(np.zeros((1, M.MOMENTS)))
    none = M.mls_step(Q, P[:0], h2, 1, 1.0)                                   # an empty cloud: every query stays
    assert none["count"].tolist() == [0] and bits(none["points"]) == bits(Q)


def test_strength():
    Q, P, h2, land = plane_trap()
    assert bits(M.mls_step(Q, P, h2, 4, 0.0)["points"]) == bits(Q)
    half = M.mls_step(Q, P, h2, 4, 0.5)
    assert bits(half["points"]) == bits(F([[0.25, 0.5, 0.6875]])) and half["moments"][0, 16] == -0.375


@functools.lru_cache(maxsize=None)
def order_case():
    rng = np.random.default_rng(11)
    P = (rng.uniform(0, 1, (400, 3)) * [1, 1, 0.05]).astype(F)
    return P[:64].copy(), P, 0.3 * 0.3, rng.permutation(len(P))


def test_the_order_is_part_of_the_definition_and_its_effect_is_rounding():
    Q, P, h2, perm = order_case()
    a, b = M.mls_step(Q, P, h2, 6, 1.0), M.mls_step(Q, P, h2, 6, 1.0, order=perm)
    assert a["moved"].all() and a["count"].min() > 32 and np.array_equal(a["count"], b["count"])
    assert bits(a["moments"]) != bits(b["moments"])                           # some bit of some sum
    pa, pb = a["moments"][:, 16:17] * a["moments"][:, 13:16], b["moments"][:, 16:17] * b["moments"][:, 13:16]
    assert np.abs(pa - pb).max() <= 1e-12 * np.abs(Q).max()                  # t n before the rounding to f32
    assert np.abs(a["points"].astype(np.float64) - b["points"]).max() <= 2.0 ** -23
    # the identity order handed over is the default, and entries outside [0, N) are skipped
    assert bits(M.mls_step(Q, P, h2, 6, 1.0, order=np.arange(len(P)))["moments"]) == bits(a["moments"])
    wide = np.concatenate([[-1, len(P)], np.arange(len(P))])
    assert bits(M.mls_step(Q, P, h2, 6, 1.0, order=wide)["moments"]) == bits(a["moments"])


def test_gate():
    Q, P, h2, land, qn, pn, c = gate_trap()
    free = M.mls_step(Q, P, h2, 4, 1.0)
    assert free["count"].tolist() == [5] and bits(free["points"]) != bits(land)
    # exactly at cos_gate: passes; one step of the last place above: out, and the exact plane is back
    at = M.mls_step(Q, P, h2, 4, 1.0, qn=qn, pn=pn, cos_gate=c)
    assert at["count"].tolist() == [5] and bits(at["moments"]) == bits(free["moments"])
    out = M.mls_step(Q, P, h2, 4, 1.0, qn=qn, pn=pn, cos_gate=np.nextafter(c, 1.0))
    assert out["count"].tolist() == [4] and bits(out["points"]) == bits(land)
    tight = 0.9
    # a zero or non-finite query normal: not gated
    for a in (F([[0, 0, 0]]), F([[np.nan, 0, 1]]), F([[0, np.inf, 0]])):
        got = M.mls_step(Q, P, h2, 4, 1.0, qn=a, pn=pn, cos_gate=tight)
        assert got["count"].tolist() == [5] and bits(got["moments"]) == bits(free["moments"])
    # a zero or non-finite neighbour normal fails every cos_gate > 0 and passes cos_gate = 0
    for b in (F([0, 0, 0]), F([np.nan, 0, 1]), F([0, 0, np.inf])):
        pn2 = pn.copy()
        pn2[1] = b
        assert M.mls_step(Q, P, h2, 1, 1.0, qn=qn, pn=pn2, cos_gate=2.0 ** -60)["count"].tolist() == [4]
        assert M.mls_step(Q, P, h2, 1, 1.0, qn=qn, pn=pn2, cos_gate=0.0)["count"].tolist() == [5]
    # the sign of either normal changes nothing
    ref = M.mls_step(Q, P, h2, 4, 1.0, qn=qn, pn=pn, cos_gate=tight)
    assert ref["count"].tolist() == [4]
    sign = F([[1], [-1], [1], [-1], [-1]])
    for a, b in ((-qn, pn), (qn, pn * sign), (-qn, pn * -sign)):
        got = M.mls_step(Q, P, h2, 4, 1.0, qn=a, pn=b, cos_gate=tight)
        assert all(bits(got[k]) == bits(ref[k]) for k in ref)


# ----------------------------------------------------------------------------------------------------------------------
# the product property: noise goes, the edge stays sharper with the gate
# ----------------------------------------------------------------------------------------------------------------------
RADIUS, EDGE_ANGLE = 0.04, 30.0


@functools.lru_cache(maxsize=None)
def corner():
    """Two 0.4 m x 0.4 m sheets meeting at a right angle, 1 cm spacing, 4 mm noise: the floor (a + 0.005, b, 0) and the
    wall (0, b, a + 0.005), floor first -> (points f32[3200,3], near: the rows whose noiseless position is within 3 cm
    of the edge)."""
    a, b = [g.reshape(-1) for g in np.meshgrid(np.arange(0, 0.4, 0.01), np.arange(0, 0.4, 0.01), indexing="ij")]
    zero = np.zeros_like(a)
    clean = np.concatenate([np.stack([a + 0.005, b, zero], 1), np.stack([zero, b, a + 0.005], 1)])
    P = (clean + np.random.default_rng(7).normal(0, 0.004, clean.shape)).astype(F)
    return P, np.r_[a, a] + 0.005 <= 0.03


def corner_error(points):
    """The distance of every point to the L-shaped surface: the half planes z = 0, x >= 0 and x = 0, z >= 0."""
    x, z = points[:, 0].astype(np.float64), points[:, 2].astype(np.float64)
    return np.minimum(np.hypot(z, np.minimum(x, 0.0)), np.hypot(x, np.minimum(z, 0.0)))


@functools.lru_cache(maxsize=None)
def corner_smoothed(iterations=1, gated=False):
    return M.smooth(corner()[0], RADIUS, iterations, 6, 1.0, EDGE_ANGLE if gated else None)


def rmse(e):
    return math.sqrt(float(np.mean(e * e)))


def corner_figures(ungated, gated):
    """The figures the conditions are stated on, in metres."""
    P, near = corner()
    before, u, g = corner_error(P), corner_error(ungated), corner_error(gated)
    return dict(before=rmse(before), after=rmse(u), gated=rmse(g), near_ungated=rmse(u[near]), near_gated=rmse(g[near]))


def check_corner(f):
    assert f["after"] < 0.5 * f["before"], f
    assert f["near_gated"] < 0.75 * f["near_ungated"], f
    assert f["gated"] <= f["after"], f


def test_corner_fixture():
    """Measured with the statement (Jacobi): rmse 3.95 mm -> 1.35 mm over all points ungated and 1.11 mm gated; near the
    edge 3.27 mm ungated and 1.61 mm gated.  A second ungated iteration gives 1.43 mm, no better than the first: that
    is why `iterations` defaults to 1 (recorded here, not asserted)."""
    f = corner_figures(corner_smoothed(1, False)[0], corner_smoothed(1, True)[0])
    twice = rmse(corner_error(corner_smoothed(2, False)[0]))
    print("corner fixture, mm:", {k: round(1e3 * v, 3) for k, v in f.items()}, "two ungated iterations:",
          round(1e3 * twice, 3))
    assert int(corner()[1].sum()) == 240
    check_corner(f)
