"""The numpy statement of the cloud planes (tests/cloud_planes_numpy.py; DESIGN.md "Cloud planes") checked against
itself: the hash against Python integers written out a second time, traps computed by hand, and the six walls of the
room against the truth.  tests/test_cloud_planes_gpu.py runs every trap and the room through the kernels."""
import functools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_numpy as C  # noqa: E402
import cloud_planes_numpy as S  # noqa: E402

from mast3r_slam.synthetic import ROOM_HALF  # noqa: E402

TOL = 2.0 ** -7
Z = np.array([[0.0, 0.0, 1.0, 0.0]])                       # the plane z = 0


# ----------------------------------------------------------------------------------------------------------------------
# the hash
# ----------------------------------------------------------------------------------------------------------------------
def _mix_again(x):
    """SplitMix64's finaliser once more, with the reductions mod 2^64 written as `%`."""
    two64 = 2 ** 64
    x = (x + 11400714819323198485) % two64
    x = ((x ^ (x // 2 ** 30)) * 13787848793156543929) % two64
    x = ((x ^ (x // 2 ** 27)) * 10723151780598845931) % two64
    return x ^ (x // 2 ** 31)


def test_hash():
    # SplitMix64 seeded with 0 hands out mix(0), mix(golden), ...: the first is the published 0xE220A8397B1DCDAF
    assert S.mix(0) == 0xE220A8397B1DCDAF
    assert 0x9E3779B97F4A7C15 == 11400714819323198485 and 0xBF58476D1CE4E5B9 == 13787848793156543929
    assert 0x94D049BB133111EB == 10723151780598845931
    for x in (0, 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1, 0x0123456789ABCDEF):
        assert S.mix(x) == _mix_again(x) and 0 <= S.mix(x) < 2 ** 64
    for seed, r, h, j, M in ((0, 0, 0, 0, 1650), (7, 3, 1023, 2, 1000), (2 ** 64 - 1, 63, 5, 1, 2 ** 31 - 1),
                             (12345, 1, 2, 0, 3), (2 ** 64 + 5, 0, 1, 1, 17)):
        want = _mix_again(_mix_again(_mix_again(seed % 2 ** 64) ^ (r * 2 ** 32 + h)) ^ j) % M
        assert S.draw(seed, r, h, j, M) == want and 0 <= want < M
    assert S.draw(2 ** 64 + 5, 0, 1, 1, 17) == S.draw(5, 0, 1, 1, 17)           # the seed is taken mod 2^64
    # M = 2^31 - 1: the draws stay below M and use the high part of the range
    big = [S.draw(1, 0, h, j, 2 ** 31 - 1) for h in range(64) for j in range(3)]
    assert max(big) < 2 ** 31 - 1 and max(big) > 2 ** 30 and len(set(big)) == len(big)
    # M = 1: every draw is 0, every hypothesis void; M = 3: a hypothesis is void unless its draws are a permutation
    P = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    hyp, tri = S.hypotheses(P, [0], 5, 0, 64)
    assert np.isnan(hyp).all() and (tri == 0).all()
    hyp, tri = S.hypotheses(P, [0, 1, 2], 5, 0, 64)
    distinct = np.array([len(set(t)) == 3 for t in tri.tolist()])
    assert distinct.any() and (~distinct).any()
    assert np.isnan(hyp[~distinct]).all() and np.isfinite(hyp[distinct]).all()
    assert (np.abs(hyp[distinct][:, :3]) == [0.0, 0.0, 1.0]).all() and (hyp[distinct][:, 3] == 0.0).all()
    hyp, tri = S.hypotheses(P, [], 5, 0, 4)
    assert np.isnan(hyp).all() and (tri == -1).all()


# ----------------------------------------------------------------------------------------------------------------------
# the traps: data and the hand-computed answer
# ----------------------------------------------------------------------------------------------------------------------
def tol_trap():
    """Points exactly tol = 2^-7 from an axis-aligned plane support it, the next float beyond does not ->
    (points, planes f64[2,4], tol, support bool[2,M])."""
    up, down = np.nextafter(np.float32(TOL), np.float32(1)), np.nextafter(np.float32(-TOL), np.float32(-1))
    one_up = np.nextafter(np.float32(1 + TOL), np.float32(2))
    P = np.float32([[0.3, -0.2, TOL], [5.0, 1.0, -TOL], [0.1, 0.1, up], [0.2, 0.7, down], [1.0, 2.0, 0.0],
                    [0.5, 0.5, 1 + TOL], [0.5, 0.25, one_up], [0.0, 0.0, 1 - TOL]])
    planes = np.array([[0.0, 0.0, 1.0, 0.0], [0.0, 0.0, -1.0, 1.0]])          # z = 0, and z = 1 looking down
    want = np.array([[1, 1, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 1, 0, 1]], bool)
    return P, planes, TOL, want


def gate_trap():
    """Six points on z = 0 with the normals +z, -z, +x, zero, NaN and inf -> (points, normals, want {(gated,
    cos_angle): count of the plane z = 0})."""
    P = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 0, 0], [2, 1, 0]])
    Nm = np.float32([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 0, 0], [np.nan, 0, 1], [0, np.inf, 1]])
    return P, Nm, {(False, 0.0): 6, (True, 1.0): 2, (True, 0.0): 3, (True, 0.5): 2}


def min_points_trap():
    """Ten points of z = 0 and five elsewhere, no three of which lie on a plane with two more: every hypothesis drawn
    from the ten is z = 0 exactly (the cross product of two vectors with z = 0 has x = y = 0) and counts 10."""
    rng = np.random.default_rng(10)
    P = np.concatenate([np.c_[rng.uniform(-1, 1, (10, 2)), np.zeros(10)],
                        np.c_[rng.uniform(-1, 1, (5, 2)), rng.uniform(0.5, 3.0, 5)]]).astype(np.float32)
    return P[rng.permutation(15)], 1.0e-3


def collinear_trap():
    """The plane z = 0 whose only supporters lie on the x axis; the other points are far above ->
    (points, plane, origin, tol)."""
    P = np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [0.5, 1.0, 5.0], [1.5, -1.0, 6.0], [2.5, 2.0, 7.0]])
    return P, Z[0].copy(), np.zeros(3), TOL


def fewer_trap():
    """The plane z = 0, tol = 2^-4: 40 points on it, 6 at z = +tol at the far ends and 4 at z = -tol in the middle.  All
    50 support it.  The fit moves up by about tol / 25 and leaves the four behind: 46 < 50, the plane stays."""
    t = 2.0 ** -4
    g = np.stack(np.meshgrid(np.arange(10.0), np.arange(4.0), indexing="ij"), -1).reshape(-1, 2)
    ends = np.float32([[-20, 0, t], [-20, 1.5, t], [-20, 3, t], [29, 0, t], [29, 1.5, t], [29, 3, t]])
    mid = np.float32([[4.5, 0.5, -t], [4.5, 1.5, -t], [4.5, 2.5, -t], [5.5, 1.5, -t]])
    P = np.concatenate([np.c_[g, np.zeros(40)], ends, mid]).astype(np.float32)
    return P, Z[0].copy(), np.zeros(3), t


def test_traps():
    P, planes, tol, want = tol_trap()
    rem = np.arange(len(P))
    assert np.array_equal(S.support(P, None, rem, planes, tol), want)
    assert S.count(P, None, rem, planes, tol).tolist() == [3, 2]
    assert S.count(P, None, rem[[0, 2, 4]], planes, tol).tolist() == [2, 0]       # a list that skips points
    # void: a collinear triple, a repeated point
    a, b, c = (np.float64(x) for x in ([1, 0, 0], [2, 0, 0], [3, 0, 0]))
    assert np.isnan(S.plane_from_triple(a, b, c)).all() and np.isnan(S.plane_from_triple(a, a, c)).all()
    assert S.plane_from_triple(a, b, np.float64([0, 1, 0])).tolist() == [0.0, 0.0, 1.0, 0.0]   # (1,0,0) x (-1,1,0)
    assert S.count(P, None, rem, np.full((1, 4), np.nan), tol).tolist() == [0]
    # select: the lower h on ties, the edge of min_points
    assert S.select(np.int32([3, 7, 7, 2]), 1) == (1, 7, True)
    assert S.select(np.int32([3, 7, 7, 2]), 7) == (1, 7, True) and S.select(np.int32([3, 7, 7, 2]), 8) == (1, 7, False)
    Q, tol_q = min_points_trap()
    on = Q[:, 2] == 0
    for mp, n_planes in ((10, 1), (11, 0)):
        res = S.planes(Q, tol_q, max_planes=4, min_points=mp, hypotheses_per_round=64, seed=1)
        assert res["n_planes"] == n_planes and np.array_equal(res["labels"] == 0, on & (n_planes == 1))
    assert res["labels"].tolist() == [-1] * 15
    res = S.planes(Q, tol_q, max_planes=4, min_points=10, hypotheses_per_round=64, seed=1)
    assert res["counts"].tolist() == [10] and res["planes"][0].tolist() == [0.0, 0.0, 1.0, 0.0] and res["rmse"][0] == 0.0
    # the refit's two fall-backs
    L, plane, origin, tol_l = collinear_trap()
    got, sums, accepted = S.refit(L, None, np.arange(len(L)), plane, origin, tol_l)
    assert accepted == 0 and got.tolist() == plane.tolist() and sums[0] == 4.0 and S.fit(sums, origin)[1]
    F, plane, origin, tol_f = fewer_trap()
    rem = np.arange(len(F))
    got, sums, accepted = S.refit(F, None, rem, plane, origin, tol_f)
    cand, degenerate = S.fit(sums, origin)
    assert accepted == 0 and got.tolist() == plane.tolist() and sums[0] == 50.0 and not degenerate
    assert S.count(F, None, rem, cand[None], tol_f).tolist() == [46]
    assert S.refit(F, None, rem, plane, origin, 2.0 * tol_f)[2] == 2              # with room to move it is taken
    # the gate
    G, Nm, want = gate_trap()
    for (gated, cos_angle), n in want.items():
        assert S.count(G, Nm if gated else None, np.arange(6), Z, TOL, cos_angle).tolist() == [n], (gated, cos_angle)
    # NaN and inf points, and labelled points, never enter the list
    R = np.float32([[0, 0, 0], [np.nan, 0, 0], [1, 1, 1], [0, np.inf, 0], [2, 2, 2], [0, 0, -np.inf], [3, 3, 3]])
    assert S.remaining(R, [-1] * 7).tolist() == [0, 2, 4, 6] and S.remaining(R, [-1, -1, 0, -1, 5, -1, -1]).tolist() == [0, 6]
    # orientation: the largest component, the lowest axis on ties; the viewpoint's side
    assert S.orient([0.6, -0.8, 0.0, 2.0]).tolist() == [-0.6, 0.8, -0.0, -2.0]
    assert S.orient([-0.5, 0.5, 0.5, 1.0]).tolist() == [0.5, -0.5, -0.5, -1.0]
    assert S.orient([0.0, 0.0, 1.0, -1.5], viewpoint=[0, 0, 0]).tolist() == [-0.0, -0.0, -1.0, 1.5]
    assert S.orient([0.0, 0.0, 1.0, -1.5], viewpoint=[0, 0, 2]).tolist() == [0.0, 0.0, 1.0, -1.5]


def test_sums_order():
    """The sums in the statement's order are the plain sums up to rounding, and exact where the summands are."""
    rng = np.random.default_rng(4)
    for M in (3, 255, 256, 257, 3000):
        P = np.c_[rng.integers(-8, 9, (M, 2)), np.zeros(M)].astype(np.float32)
        got = S.sums(P, None, np.arange(M), Z[0], np.float64([1.0, -2.0, 0.0]), TOL)
        q = P.astype(np.float64) - [1.0, -2.0, 0.0]
        want = [M, *q.sum(0), (q[:, 0] ** 2).sum(), (q[:, 0] * q[:, 1]).sum(), 0.0, (q[:, 1] ** 2).sum(), 0.0, 0.0, 0.0]
        assert got.tolist() == want                                               # small integers: every order agrees
    v = rng.normal(size=(256, 2))
    assert np.allclose(S.block_sum(v), v.sum(0), rtol=0, atol=1e-12) and S.wave_sum(np.arange(64.0)) == 2016.0


# ----------------------------------------------------------------------------------------------------------------------
# the room against the truth
# ----------------------------------------------------------------------------------------------------------------------
ROOM_KW = dict(max_planes=16, min_points=15, hypotheses_per_round=128, seed=0)
ROOM_TOL = 0.01
ANGLE_BAR = 3 * 5.8e-4             # rad; the statement reaches 5.76e-4 on this fixture with seed 0
OFFSET_BAR = 3 * 2.8e-4            # m; it reaches 2.76e-4


@functools.lru_cache(maxsize=None)
def room_fixture(n_wall=1500, n_out=150, sigma=0.002, seed=0):
    """(points f32[N,3], wall i64[N]): n_wall samples of the ROOM_HALF box by area with Gaussian noise sigma on every
    coordinate, n_out points uniform in the box (wall -1), shuffled.  Wall 2 a + s is the one at (-1, +1)[s] ROOM_HALF[a]."""
    rng = np.random.default_rng(seed)
    h = ROOM_HALF
    areas = np.array([h[1] * h[2], h[1] * h[2], h[0] * h[2], h[0] * h[2], h[0] * h[1], h[0] * h[1]])
    wall = rng.choice(6, n_wall, p=areas / areas.sum())
    P = rng.uniform(-1, 1, (n_wall, 3)) * h
    P[np.arange(n_wall), wall // 2] = np.where(wall % 2 == 0, -1.0, 1.0) * h[wall // 2]
    P = P + rng.normal(0.0, sigma, P.shape)
    P = np.concatenate([P, rng.uniform(-1, 1, (n_out, 3)) * h]).astype(np.float32)
    perm = rng.permutation(len(P))
    return P[perm], np.concatenate([wall, np.full(n_out, -1)])[perm]


@functools.lru_cache(maxsize=None)
def room_planes():
    """The statement on the room, computed once and shared with the GPU tests."""
    return S.planes(room_fixture()[0], ROOM_TOL, **ROOM_KW)


def test_room_against_the_truth():
    """1 500 wall samples with 2 mm of noise and 150 outliers, tol 1 cm, 128 hypotheses, min_points 15, seed 0.  The
    statement finds exactly six planes, one per wall, with counts 354 249 349 161 236 153; the worst normal is 5.76e-4
    rad from its wall's and the worst offset 2.76e-4 m, so the bars are 3 x 5.8e-4 rad and 3 x 2.8e-4 m.  No junk plane
    (under 100 points) holds more than 2 % of the points; manhattan_deg, 0.0145 here, is a mean over pairs of planes
    each within the angle bar of its wall, so it lies under twice that bar."""
    from mast3r_slam.tsdf.cloud_planes import plane_figures

    P, wall = room_fixture()
    res = room_planes()
    big = np.flatnonzero(res["counts"] >= 100)
    assert len(big) == 6
    found, worst_angle, worst_offset = [], 0.0, 0.0
    for i in big:
        n, d = res["planes"][i, :3], res["planes"][i, 3]
        a = int(np.argmax(np.abs(n)))
        s = int(-d * n[a] > 0)                                                     # the wall lies at -d / n[a]
        found.append(2 * a + s)
        worst_angle = max(worst_angle, float(np.arccos(min(1.0, abs(n[a])))))
        worst_offset = max(worst_offset, abs(abs(float(d)) - float(ROOM_HALF[a])))
        assert n[a] > 0                                                            # oriented by the largest component
        members = wall[res["labels"] == i]
        assert (members == 2 * a + s).mean() > 0.97                                # its own wall's samples, and few others
    print(f"counts {res['counts'].tolist()}, worst angle {worst_angle:.3e} rad, worst offset {worst_offset:.3e} m")
    assert sorted(found) == [0, 1, 2, 3, 4, 5]
    assert worst_angle <= ANGLE_BAR and worst_offset <= OFFSET_BAR
    junk = np.delete(res["counts"], big)
    assert (junk <= 0.02 * len(P)).all()
    assert np.abs(np.linalg.norm(res["planes"][:, :3], axis=1) - 1.0).max() <= 2.0 ** -50
    assert np.array_equal(np.bincount(res["labels"][res["labels"] >= 0], minlength=res["n_planes"]), res["counts"])
    fig = plane_figures(res, P)
    want = S.figures(res, int(C.valid(P).sum()))
    print("figures", json.dumps(fig))
    assert fig == want and fig["n_planes"] == res["n_planes"]
    assert fig["manhattan_deg"] <= 2.0 * np.degrees(ANGLE_BAR)
    assert 0.85 < fig["plane_share"] <= 1500 / 1650 + 0.02 and 0.0015 < fig["plane_rmse"] < 0.0025
    assert plane_figures(res)["plane_share"] == fig["plane_share"]                 # without points: every point is valid
