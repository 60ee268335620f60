"""GPU tests (-m gpu) of the RANSAC plane segmentation of a point cloud (csrc/cloud_planes.hip,
mast3r_slam/tsdf/cloud_planes.py, SlamSystem.cloud_planes / evaluate_planarity; DESIGN.md "Cloud planes") against the
numpy statement tests/cloud_planes_numpy.py: every stage through its C entry point byte for byte at the wave, block and
chunk edges, the traps of tests/test_cloud_planes_cpu.py, the whole call on that file's room, the Python layer's
refusals and the product.  Every operand of the C entry points lies in a guarded buffer, and the guards are checked
after every raw call."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_numpy as C  # noqa: E402
import cloud_planes_numpy as S  # noqa: E402
import test_cloud_planes_cpu as traps  # noqa: E402
from mesh_support import Operands  # noqa: E402

pytestmark = pytest.mark.gpu

STATE, FIT = 8, 40                 # MSLAM_CLOUD_PLANES_STATE, MSLAM_CLOUD_PLANES_FIT
M_, FOUND, DONE, BEST_H, BEST_COUNT, STOPPED = range(6)
CHUNK = 1024                       # list rows per block of the count: 256 threads, 4 points per lane
MAX_BLOCKS = 1024                  # the cap of its grid
# none, one; around a wave; around a block of the sums; a chunk and a point; four chunks and a point
SIZES_M = (0, 1, 63, 64, 65, 255, 256, 257, CHUNK + 1, 4 * CHUNK + 1)
SIZES_H = (1, 63, 64, 65, 1024)
COS30 = math.cos(math.pi / 6.0)


def _lib():
    import mslam_hip as _m

    return _m, _m.lib(), _m.stream_ptr()


def _same(got, want, dtype):
    """Byte-equal, NaNs in the same places."""
    got, want = np.asarray(got), np.ascontiguousarray(want, dtype)
    assert got.dtype == dtype and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    nan = np.isnan(want) if want.dtype.kind == "f" else np.zeros(want.shape, bool)
    if want.dtype.kind == "f":
        assert np.array_equal(np.isnan(got), nan)
    assert np.where(nan, 0, got).tobytes() == np.where(nan, 0, want).tobytes()


def _state(M=0, found=0, done=0):
    s = np.zeros(STATE, np.int32)
    s[M_], s[FOUND], s[DONE] = M, found, done
    return s


def _remaining(device, P, labels, min_points):
    """mslam_cloud_planes_remaining -> (the list's first M entries, the state)."""
    _m, L, st = _lib()
    ops = Operands(device)
    N = len(P)
    p, lab = ops.put(P, np.float32), ops.put(labels, np.int32)
    offs = ops.put(np.full((N + 255) // 256, -7, np.int32), np.int32)
    rem = ops.put(np.full(N, -7, np.int32), np.int32)
    state = ops.put(_state(), np.int32)
    _m.check(L.mslam_cloud_planes_remaining(_m.ptr(p), N, _m.ptr(lab), min_points, _m.ptr(offs), _m.ptr(rem),
                                            _m.ptr(state), st), "cloud_planes_remaining")
    ops.check()
    s, r = state.cpu().numpy(), rem.cpu().numpy()
    assert (r[s[M_]:] == -7).all()                                           # nothing past the list
    return r[:s[M_]], s


def _draw(device, P, rem, seed, rnd, H, state=None):
    """mslam_cloud_planes_draw -> (hyp f64[H,4], triples i32[H,3]); with a state that is done: nothing is written."""
    _m, L, st = _lib()
    ops = Operands(device)
    p, r = ops.put(P, np.float32), ops.put(rem, np.int32)
    s = ops.put(_state(len(rem)) if state is None else state, np.int32)
    hyp, tri = ops.out(torch.float64, (H, 4)), ops.out(torch.int32, (H, 3))
    _m.check(L.mslam_cloud_planes_draw(_m.ptr(p), len(P), _m.ptr(r), len(rem), _m.ptr(s), seed, rnd, H, _m.ptr(hyp),
                                       _m.ptr(tri), st), "cloud_planes_draw")
    if state is not None and state[DONE]:
        torch.cuda.synchronize()
        assert all(bool((g.raw == g.pat).all()) for g in (ops.all["3"], ops.all["4"]))
        return None, None
    ops.check()
    return hyp.cpu().numpy(), tri.cpu().numpy()


def _count(device, P, Nm, rem, hyp, tol, cos_angle=0.0, state=None):
    """mslam_cloud_planes_count -> count i32[H]."""
    _m, L, st = _lib()
    ops = Operands(device)
    p, r = ops.put(P, np.float32), ops.put(rem, np.int32)
    nm = ops.put(Nm, np.float32) if Nm is not None else None
    s = ops.put(_state(len(rem)) if state is None else state, np.int32)
    h = ops.put(hyp, np.float64)
    H = len(hyp)
    count = ops.out(torch.int32, (H,))
    _m.check(L.mslam_cloud_planes_count(_m.ptr(p), _m.ptr(nm), len(P), _m.ptr(r), len(rem), _m.ptr(s), _m.ptr(h), H,
                                        float(tol), float(cos_angle), _m.ptr(count), st), "cloud_planes_count")
    ops.check()
    return count.cpu().numpy()


def _select(device, counts, min_points, P, hyp, tri, state=None):
    """mslam_cloud_planes_select -> (state, fit)."""
    _m, L, st = _lib()
    ops = Operands(device)
    c, p = ops.put(counts, np.int32), ops.put(P, np.float32)
    h, t = ops.put(hyp, np.float64), ops.put(tri, np.int32)
    s = ops.put(_state(len(P)) if state is None else state, np.int32)
    fit = ops.put(np.full(FIT, -5.0), np.float64)
    _m.check(L.mslam_cloud_planes_select(_m.ptr(c), len(counts), min_points, _m.ptr(p), len(P), _m.ptr(h), _m.ptr(t),
                                         _m.ptr(s), _m.ptr(fit), st), "cloud_planes_select")
    ops.check()
    return s.cpu().numpy(), fit.cpu().numpy()


def _fit0(plane, origin):
    f = np.zeros(FIT)
    f[0:4], f[4:7] = plane, origin
    return f


def _refit(device, P, Nm, rem, plane, origin, tol, cos_angle=0.0, iterations=2):
    """mslam_cloud_planes_refit -> (plane f64[4], sums f64[11], the state)."""
    _m, L, st = _lib()
    ops = Operands(device)
    p, r = ops.put(P, np.float32), ops.put(rem, np.int32)
    nm = ops.put(Nm, np.float32) if Nm is not None else None
    s = ops.put(_state(len(rem)), np.int32)
    fit = ops.put(_fit0(plane, origin), np.float64)
    partial = ops.put(np.full(S.SUMS * ((len(rem) + 255) // 256), np.nan), np.float64)
    _m.check(L.mslam_cloud_planes_refit(_m.ptr(p), _m.ptr(nm), len(P), _m.ptr(r), len(rem), float(tol),
                                        float(cos_angle), iterations, _m.ptr(partial), _m.ptr(s), _m.ptr(fit), st),
             "cloud_planes_refit")
    ops.check()
    f = fit.cpu().numpy()
    return f[0:4], f[8:19], s.cpu().numpy()


def _label(device, P, Nm, rem, plane, origin, sums, tol, cos_angle=0.0, viewpoint=None, found=0, max_planes=4):
    """mslam_cloud_planes_label -> (labels, planes f64[max_planes, ROW], the state)."""
    _m, L, st = _lib()
    ops = Operands(device)
    p, r = ops.put(P, np.float32), ops.put(rem, np.int32)
    nm = ops.put(Nm, np.float32) if Nm is not None else None
    vp = ops.put(viewpoint, np.float32) if viewpoint is not None else None
    s = ops.put(_state(len(rem), found), np.int32)
    f = _fit0(plane, origin)
    f[8:19] = sums
    fit = ops.put(f, np.float64)
    labels = ops.put(np.full(len(P), -1, np.int32), np.int32)
    planes = ops.put(np.full((max_planes, S.ROW), -5.0), np.float64)
    _m.check(L.mslam_cloud_planes_label(_m.ptr(p), _m.ptr(nm), len(P), _m.ptr(r), len(rem), float(tol),
                                        float(cos_angle), _m.ptr(vp), _m.ptr(fit), max_planes, _m.ptr(s),
                                        _m.ptr(labels), _m.ptr(planes), st), "cloud_planes_label")
    ops.check()
    return labels.cpu().numpy(), planes.cpu().numpy(), s.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# the stages against the statement
# ----------------------------------------------------------------------------------------------------------------------
_BIG = {}


def big_room():
    """4 700 points of the room with NaN, inf and labelled points among them, their walls' normals (some zero, some not
    finite), the remaining list, and 1024 hypotheses drawn from it with a void one put in."""
    if not _BIG:
        P, wall = traps.room_fixture(4400, 300, 0.002, 1)
        P = P.copy()
        rng = np.random.default_rng(5)
        Nm = np.zeros_like(P)
        on = wall >= 0
        Nm[np.flatnonzero(on), wall[on] // 2] = 1.0
        Nm[~on] = rng.normal(size=(int((~on).sum()), 3))
        Nm[rng.permutation(len(P))[:40]] = 0.0
        Nm[7], Nm[70] = (np.nan, 0, 1), (0, np.inf, 0)
        P[[3, 300, 3000]] = np.nan
        P[[30, 1300]] = np.inf
        labels = np.full(len(P), -1, np.int32)
        labels[rng.permutation(len(P))[:200]] = rng.integers(0, 5, 200)
        rem = S.remaining(P, labels)
        assert len(rem) >= max(SIZES_M)
        hyp, tri = S.hypotheses(P, rem, 11, 0, 1024)
        hyp[[0, 100]] = np.nan
        _BIG.update(P=P, Nm=Nm, labels=labels, rem=rem, hyp=hyp)
    return _BIG


def test_remaining_parity(device):
    B = big_room()
    for N in (1, 2, 255, 256, 257, 1025, len(B["P"])):
        P, labels = B["P"][:N], B["labels"][:N]
        want = S.remaining(P, labels)
        for mp in (1, 100):
            rem, state = _remaining(device, P, labels, mp)
            assert rem.tobytes() == want.tobytes() and state[M_] == len(want)
            assert state[DONE] == int(len(want) < max(3, mp)) and state[FOUND] == 0
    # a list that skips invalid points only, and one where nothing remains
    P = np.float32([[0, 0, 0], [np.nan, 0, 0], [1, 1, 1], [0, np.inf, 0], [2, 2, 2], [0, 0, -np.inf], [3, 3, 3]])
    assert _remaining(device, P, [-1] * 7, 1)[0].tolist() == [0, 2, 4, 6]
    rem, state = _remaining(device, P, [-1, -1, 0, -1, 5, -1, -1], 1)
    assert rem.tolist() == [0, 6] and state[DONE] == 1                       # M < 3
    rem, state = _remaining(device, P, [0] * 7, 1)
    assert rem.tolist() == [] and state[DONE] == 1


@pytest.mark.parametrize("M", (3, 4, 1000))
def test_draw_parity(device, M):
    B = big_room()
    rem = B["rem"][:M]
    for seed, rnd in ((0, 0), (2 ** 64 - 1, 63), (12345, 7)):
        want_hyp, want_tri = S.hypotheses(B["P"], rem, seed, rnd, 1024)
        hyp, tri = _draw(device, B["P"], rem, seed, rnd, 1024)
        _same(hyp, want_hyp, np.float64)
        _same(tri, want_tri, np.int32)
    void = np.isnan(want_hyp[:, 0])
    assert not void.all() and (void.any() or M == 1000)                      # short lists repeat a draw
    # H below a block of the draw, and every hypothesis of a list of one or two points is void
    hyp, tri = _draw(device, B["P"], rem, 3, 1, 65)
    _same(hyp, S.hypotheses(B["P"], rem, 3, 1, 65)[0], np.float64)
    for m in (1, 2):
        hyp, tri = _draw(device, B["P"], B["rem"][:m], 3, 1, 64)
        assert np.isnan(hyp).all() and np.isin(tri, B["rem"][:m]).all()
    # done: nothing is written
    assert _draw(device, B["P"], rem, 3, 1, 64, state=_state(M, 0, 1)) == (None, None)


@pytest.mark.parametrize("M", SIZES_M)
def test_count_parity(device, M):
    B = big_room()
    rem = B["rem"][:M] if M % 2 else B["rem"][-M:] if M else B["rem"][:0]
    tol = 0.01
    for Nm, cos_angle in ((None, 0.0), (B["Nm"], COS30)):
        want = S.count(B["P"], Nm, rem, B["hyp"], tol, cos_angle)
        if M > CHUNK:
            assert want.max() > 100 and (want == 0).sum() >= 2 and len(np.unique(want)) > 20    # not a trivial answer
        for H in SIZES_H:
            got = _count(device, B["P"], Nm, rem, B["hyp"][:H], tol, cos_angle)
            assert got.dtype == np.int32 and got.tobytes() == want[:H].tobytes(), (M, H, Nm is not None)
        if M == 4 * CHUNK + 1:
            gated = want
    if M == 4 * CHUNK + 1:
        assert (gated <= S.count(B["P"], None, rem, B["hyp"], tol)).all() and gated.sum() > 0


def test_count_traps_and_stride(device):
    P, planes, tol, want = traps.tol_trap()
    rem = np.arange(len(P), dtype=np.int32)
    assert _count(device, P, None, rem, planes, tol).tolist() == [3, 2]
    assert _count(device, P, None, rem[[0, 2, 4]], planes, tol).tolist() == [2, 0]
    assert _count(device, P, None, rem, np.full((3, 4), np.nan), tol).tolist() == [0, 0, 0]      # void
    G, Nm, answers = traps.gate_trap()
    for (gated, cos_angle), n in answers.items():
        got = _count(device, G, Nm if gated else None, np.arange(6, dtype=np.int32), traps.Z, traps.TOL, cos_angle)
        assert got.tolist() == [n], (gated, cos_angle)
    # done: the counts are zero; an entry of the list outside the cloud never counts
    assert _count(device, P, None, rem, planes, tol, state=_state(len(rem), 0, 1)).tolist() == [0, 0]
    assert _count(device, P, None, np.int32([0, -1, 8, 2 ** 31 - 1, 4]), planes, tol).tolist() == [2, 0]
    # more chunks than the grid has blocks: the blocks stride over the list
    rng = np.random.default_rng(12)
    n = MAX_BLOCKS * CHUNK + CHUNK + 5
    big = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    hyp = np.array([[0.0, 0.0, 1.0, 0.0], [0.6, 0.0, 0.8, -0.1], [np.nan] * 4])
    rem = np.arange(n, dtype=np.int32)
    want = S.count(big, None, rem, hyp, 0.05, chunk=1)
    assert want[0] > n // 25 and want[2] == 0
    assert _count(device, big, None, rem, hyp, 0.05).tobytes() == want.tobytes()


def test_select(device):
    B = big_room()
    P, hyp = B["P"], B["hyp"][:4]
    tri = np.int32([[5, 6, 8], [9, 10, 11], [12, 13, 14], [15, 16, 17]])
    state, fit = _select(device, np.int32([3, 7, 7, 2]), 7, P, hyp, tri)
    assert state[BEST_H] == 1 and state[BEST_COUNT] == 7 and state[DONE] == 0 and state[STOPPED] == 0
    _same(fit[0:4], hyp[1], np.float64)
    _same(fit[4:7], P[9].astype(np.float64), np.float64)
    state, fit = _select(device, np.int32([3, 7, 7, 2]), 8, P, hyp, tri)
    assert state[BEST_H] == 1 and state[DONE] == 1 and (fit == -5.0).all()   # min_points - 1 stops
    # the first maximum among 1024, in every lane's stride and across the lanes
    rng = np.random.default_rng(6)
    c = rng.integers(0, 50, 1024).astype(np.int32)
    H4 = np.tile(hyp, (256, 1))
    T4 = np.tile(tri, (256, 1))
    for where in ((1000, 70, 500), (64, 0), (1023,), (65, 129)):
        cc = c.copy()
        cc[list(where)] = 60
        state, _ = _select(device, cc, 1, P, H4, T4)
        assert (state[BEST_H], state[BEST_COUNT]) == S.select(cc, 1)[:2] == (min(where), 60)
    for H in (1, 63, 65):
        state, _ = _select(device, c[:H], 1, P, H4[:H], T4[:H])
        assert (state[BEST_H], state[BEST_COUNT]) == S.select(c[:H], 1)[:2]
    state, _ = _select(device, np.zeros(64, np.int32), 1, P, H4[:64], T4[:64])
    assert state[DONE] == 1                                                  # nothing but void hypotheses
    state, fit = _select(device, c, 1, P, H4, T4, state=_state(10, 2, 1))
    assert state.tolist() == _state(10, 2, 1).tolist() and (fit == -5.0).all()   # done: a no-op


@pytest.mark.parametrize("M", (3, 255, 256, 257, 5000))
def test_refit_parity(device, M):
    """M supporters of a tilted plane with noise inside tol: the block edge of the sums and, at 5000, the cross-block
    order; the plane it starts from is a little off, so that the candidates are taken."""
    rng = np.random.default_rng(M)
    n = np.array([0.3, -0.2, 0.9])
    n /= np.linalg.norm(n)
    xy = rng.uniform(-2, 2, (M, 2))
    z = (0.5 - n[0] * xy[:, 0] - n[1] * xy[:, 1]) / n[2] + rng.normal(0, 0.002, M)
    far = np.c_[rng.uniform(-2, 2, (50, 2)), rng.uniform(3, 4, 50)]
    P = np.concatenate([np.c_[xy, z], far]).astype(np.float32)
    P = P[rng.permutation(len(P))]
    rem = S.remaining(P, np.full(len(P), -1))
    start = np.array([*n, -0.5 + 0.001])
    origin = P[rem[0]].astype(np.float64)
    tol = 0.02
    assert S.count(P, None, rem, start[None], tol)[0] == M
    for iterations in (0, 1, 2):
        want_plane, want_sums, accepted = S.refit(P, None, rem, start, origin, tol, 0.0, iterations)
        plane, sums, state = _refit(device, P, None, rem, start, origin, tol, 0.0, iterations)
        _same(plane, want_plane, np.float64)
        _same(sums, want_sums, np.float64)
        assert sums[0] == M and (M == 3 or accepted == iterations)
    # the row and the labels of the refitted plane, both orientation rules
    for viewpoint, found in ((None, 0), (np.float32([0, 0, 5]), 1), (np.float32([0, 0, -5]), 3)):
        labels, planes, state = _label(device, P, None, rem, want_plane, origin, want_sums, tol, 0.0, viewpoint, found)
        want_row = S.row(want_plane, want_sums, origin, viewpoint)
        _same(planes[found], want_row, np.float64)
        assert (np.delete(planes, found, 0) == -5.0).all() and state[FOUND] == found + 1
        want_labels = np.full(len(P), -1, np.int32)
        want_labels[rem[S.support(P, None, rem, want_plane, tol)[0]]] = found
        assert labels.tobytes() == want_labels.tobytes() and (labels == found).sum() == M
        if viewpoint is not None:
            assert (planes[found, 2] > 0) == (viewpoint[2] > 0)
        else:
            assert planes[found, 2] > 0


def test_refit_fallbacks_and_gate(device):
    L, plane, origin, tol = traps.collinear_trap()
    rem = np.arange(len(L), dtype=np.int32)
    got, sums, state = _refit(device, L, None, rem, plane, origin, tol)
    assert got.tolist() == plane.tolist() and sums[0] == 4.0 and state[STOPPED] == 1          # degenerate
    F, plane, origin, tol = traps.fewer_trap()
    rem = np.arange(len(F), dtype=np.int32)
    want = S.refit(F, None, rem, plane, origin, tol)
    got, sums, state = _refit(device, F, None, rem, plane, origin, tol)
    assert got.tolist() == plane.tolist() and sums[0] == 50.0 and state[STOPPED] == 1         # fewer supporters
    _same(sums, want[1], np.float64)
    want = S.refit(F, None, rem, plane, origin, 2 * tol)
    got, sums, state = _refit(device, F, None, rem, plane, origin, 2 * tol)
    assert want[2] == 2 and state[STOPPED] == 0
    _same(got, want[0], np.float64)
    _same(sums, want[1], np.float64)
    # under the gate the supporters are those whose normals agree
    B = big_room()
    rem = B["rem"]
    start = np.array([0.0, 0.0, 1.0, 1.5])                                    # the floor
    origin = np.array([0.0, 0.0, -1.5])
    want = S.refit(B["P"], B["Nm"], rem, start, origin, 0.01, COS30)
    got, sums, state = _refit(device, B["P"], B["Nm"], rem, start, origin, 0.01, COS30)
    _same(got, want[0], np.float64)
    _same(sums, want[1], np.float64)
    assert 100 < sums[0] < S.count(B["P"], None, rem, start[None], 0.01)[0]
    labels, planes, _ = _label(device, B["P"], B["Nm"], rem, want[0], origin, want[1], 0.01, COS30)
    assert (labels == 0).sum() == sums[0] and planes[0, 4] == sums[0]


# ----------------------------------------------------------------------------------------------------------------------
# the whole call
# ----------------------------------------------------------------------------------------------------------------------
KEYS = dict(labels=np.int32, planes=np.float64, counts=np.int32, rmse=np.float64, centroids=np.float64,
            eigenvalues=np.float64)


def _same_result(got, want):
    assert sorted(got) == sorted(list(KEYS) + ["n_planes", "sum_r2"])
    assert got["n_planes"] == want["n_planes"]
    for k, dtype in KEYS.items():
        _same(got[k].cpu().numpy(), want[k], dtype)
    _same(got["sum_r2"].cpu().numpy(), want["rows"][:, 5], np.float64)


def test_room(device):
    from mast3r_slam.tsdf import cloud_planes, plane_figures

    P, wall = traps.room_fixture()
    want = traps.room_planes()
    p = torch.from_numpy(P).to(device)
    kw = dict(traps.ROOM_KW, hypotheses=traps.ROOM_KW["hypotheses_per_round"])
    del kw["hypotheses_per_round"]
    got = cloud_planes(p, traps.ROOM_TOL, **kw)
    _same_result(got, want)
    assert got["n_planes"] == 6 and got["counts"].tolist() == [354, 249, 349, 161, 236, 153]
    again = cloud_planes(p, traps.ROOM_TOL, **kw)
    for k in KEYS:
        assert torch.equal(got[k], again[k]), k                              # call after call
    assert plane_figures(got, p) == S.figures(want, len(P))
    # max_planes 1 and 64, a viewpoint inside the room, no refit
    for more in (dict(max_planes=1), dict(max_planes=64), dict(viewpoint=[0.5, 0.2, -0.3]), dict(refit_iterations=0),
                 dict(seed=2 ** 64 + 3, min_points=100)):
        k2 = dict(kw, **more)
        s2 = dict(traps.ROOM_KW, **more)
        res = cloud_planes(p, traps.ROOM_TOL, **k2)
        _same_result(res, S.planes(P, traps.ROOM_TOL, **s2))
        if "max_planes" in more:
            assert res["n_planes"] == min(6, more["max_planes"])
        if "viewpoint" in more:
            n, d = res["planes"][:, :3].cpu().numpy(), res["planes"][:, 3].cpu().numpy()
            assert (n @ np.float64(more["viewpoint"]) + d > 0).all()         # every wall faces the room
    # with normals: the walls' own, by value and from cloud_normals
    Nm = np.zeros_like(P)
    Nm[np.flatnonzero(wall >= 0), wall[wall >= 0] // 2] = 1.0
    res = cloud_planes(p, traps.ROOM_TOL, normals=torch.from_numpy(Nm).to(device), normal_angle=0.3, **kw)
    _same_result(res, S.planes(P, traps.ROOM_TOL, normals=Nm, cos_angle=math.cos(0.3), **traps.ROOM_KW))
    assert res["n_planes"] == 6 and (res["labels"].cpu().numpy()[wall < 0] == -1).all()
    from mast3r_slam.tsdf import cloud_normals

    n16 = cloud_normals(p, 16)[0]
    res = cloud_planes(p, traps.ROOM_TOL, normals=16, **kw)
    _same_result(res, S.planes(P, traps.ROOM_TOL, normals=n16.cpu().numpy(), cos_angle=math.cos(math.pi / 6.0), **traps.ROOM_KW))
    assert res["n_planes"] >= 6


def test_edges_of_the_whole_call(device):
    from mast3r_slam.tsdf import cloud_planes, plane_figures

    rng = np.random.default_rng(1)
    U = rng.uniform(-1, 1, (2000, 3)).astype(np.float32)                     # no plane: 1 mm slabs hold a few points
    res = cloud_planes(torch.from_numpy(U).to(device), 0.001, hypotheses=64, min_points=100)
    _same_result(res, S.planes(U, 0.001, hypotheses_per_round=64, min_points=100))
    assert res["n_planes"] == 0 and (res["labels"] == -1).all() and tuple(res["planes"].shape) == (0, 4)
    assert tuple(res["centroids"].shape) == (0, 3) and tuple(res["counts"].shape) == (0,)
    assert plane_figures(res) == dict(plane_share=0.0, plane_rmse=0.0, n_planes=0, manhattan_deg=0.0)
    for N in (0, 2):
        res = cloud_planes(torch.from_numpy(U[:N]).to(device), 0.5, min_points=1)
        assert res["n_planes"] == 0 and res["labels"].tolist() == [-1] * N and res["labels"].dtype == torch.int32
    nan = torch.full((5, 3), float("nan"), dtype=torch.float32, device=device)
    assert cloud_planes(nan, 0.5, min_points=1)["n_planes"] == 0
    # the traps of the CPU file through the whole call
    Q, tol = traps.min_points_trap()
    q = torch.from_numpy(Q).to(device)
    for mp in (10, 11):
        _same_result(cloud_planes(q, tol, max_planes=4, min_points=mp, hypotheses=64, seed=1),
                     S.planes(Q, tol, max_planes=4, min_points=mp, hypotheses_per_round=64, seed=1))
    res = cloud_planes(q, tol, max_planes=4, min_points=10, hypotheses=64, seed=1)
    assert res["counts"].tolist() == [10] and res["planes"][0].tolist() == [0.0, 0.0, 1.0, 0.0]
    assert cloud_planes(q, tol, max_planes=4, min_points=11, hypotheses=64, seed=1)["n_planes"] == 0
    # three points are a plane; a min_points of 1 labels everything in the end
    T3 = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]])
    res = cloud_planes(torch.from_numpy(T3).to(device), 0.01, min_points=3, hypotheses=32)
    _same_result(res, S.planes(T3, 0.01, min_points=3, hypotheses_per_round=32))
    assert res["counts"].tolist() == [3] and (res["labels"] == 0).sum() == 3


def test_refusals(device):
    from mast3r_slam.tsdf import cloud_planes

    _m, L, st = _lib()
    p = torch.from_numpy(traps.room_fixture()[0]).to(device)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tol must be positive and finite"):
            cloud_planes(p, bad)
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(ValueError, match=r"hypotheses must be an integer in \[1, 1024\]"):
            cloud_planes(p, 0.01, hypotheses=bad)
    for bad in (0, 65, -1):
        with pytest.raises(ValueError, match=r"max_planes must be an integer in \[1, 64\]"):
            cloud_planes(p, 0.01, max_planes=bad)
    with pytest.raises(ValueError, match="min_points must be an integer >= 1"):
        cloud_planes(p, 0.01, min_points=0)
    with pytest.raises(ValueError, match=r"normals must be \(1650,3\)"):
        cloud_planes(p, 0.01, normals=torch.zeros((1649, 3), device=device))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud_planes(p, 0.01, normals=torch.zeros((1650, 3)))
    with pytest.raises(RuntimeError, match="normals must have dtype"):
        cloud_planes(p, 0.01, normals=torch.zeros((1650, 3), dtype=torch.float64, device=device))
    with pytest.raises(ValueError, match="normals .* must be an integer in"):
        cloud_planes(p, 0.01, normals=33)
    with pytest.raises(ValueError, match="normal_angle needs normals"):
        cloud_planes(p, 0.01, normal_angle=0.2)
    with pytest.raises(ValueError, match="normal_angle must be in"):
        cloud_planes(p, 0.01, normals=16, normal_angle=2.0)
    with pytest.raises(ValueError, match="viewpoint must be 3 numbers"):
        cloud_planes(p, 0.01, viewpoint=[0, 0])
    with pytest.raises(TypeError, match="points must be a device tensor"):
        cloud_planes(p.cpu().numpy(), 0.01)
    # the C entry: nothing is written
    N = int(p.shape[0])
    need = int(L.mslam_cloud_planes_workspace_bytes(N, 128))
    assert need > 0 and L.mslam_cloud_planes_workspace_bytes(N, 1025) == 0
    refused = (dict(tol=0.0), dict(tol=float("nan")), dict(H=0), dict(H=1025), dict(max_planes=0), dict(max_planes=65),
               dict(min_points=0), dict(nbytes=need - 1, rc=-3), dict(cos=1.5, normals=True), dict(misaligned=True))
    for case in refused:
        ops = Operands(device)
        labels, rows, state = ops.out(torch.int32, (N,)), ops.out(torch.float64, (64, S.ROW)), ops.out(torch.int32, (STATE,))
        ws = ops.out(torch.float64, (need // 8 + 1,)).view(torch.uint8)
        nm = p if case.get("normals") else None
        rc = L.mslam_cloud_planes(_m.ptr(p), _m.ptr(nm), N, case.get("tol", 0.01), case.get("cos", 0.0),
                                  case.get("max_planes", 16), case.get("min_points", 100), case.get("H", 128), 2, 0, 0,
                                  _m.ptr(ws) + (8 if case.get("misaligned") else 0), case.get("nbytes", need),
                                  _m.ptr(labels), _m.ptr(rows), _m.ptr(state), st)
        assert rc == case.get("rc", -1) and "cloud_planes" in L.mslam_last_error().decode(), case
        torch.cuda.synchronize()
        for g in ops.all.values():
            assert bool((g.raw == g.pat).all()), case                        # nothing written


# ----------------------------------------------------------------------------------------------------------------------
# the product
# ----------------------------------------------------------------------------------------------------------------------
def test_slam_system_cloud_planes(device, monkeypatch, tmp_path):
    """The 20-frame run of the product tests: the map of a box room has planes, the figures are finite, and the JSON
    round-trips."""
    from mast3r_slam import evaluate
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from test_slam_system_gpu import RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    thr = 2.0
    try:
        system.run(_frames(list(range(0, 60, 3)), device))
        vs = float(system.tsdf_manager.volume.voxel_size)
        before = system.keyframe_cloud(conf_threshold=thr, voxel=vs)
        points, result = system.cloud_planes(conf_threshold=thr, voxel=vs, hypotheses=256, seed=4)
        figures = system.evaluate_planarity(conf_threshold=thr, voxel=vs, hypotheses=256, seed=4)
        after = system.keyframe_cloud(conf_threshold=thr, voxel=vs)
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    assert torch.equal(points, before[0]) and torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
    want = S.planes(points.cpu().numpy(), vs, hypotheses_per_round=256, seed=4)
    _same_result(result, want)
    assert result["n_planes"] >= 1 and int(result["counts"][0]) >= 100
    assert sorted(figures) == ["manhattan_deg", "n_planes", "plane_rmse", "plane_share"]
    assert all(isinstance(v, (int, float)) and np.isfinite(v) for v in figures.values())
    assert figures == S.figures(want, int(C.valid(points.cpu().numpy()).sum()))
    assert 0.0 < figures["plane_share"] <= 1.0 and 0.0 < figures["plane_rmse"] <= vs and figures["n_planes"] >= 1
    path = evaluate.save_plane_metrics(tmp_path, "planes.json", figures)
    with open(path) as f:
        assert json.load(f) == figures
    print(f"{len(points)} points, {json.dumps(figures)}")
