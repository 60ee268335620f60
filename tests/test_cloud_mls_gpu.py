"""GPU tests (-m gpu) of the cloud smoothing step (csrc/cloud_mls.hip, mast3r_slam/tsdf/cloud_smooth.py,
SlamSystem.keyframe_cloud(smooth=); DESIGN.md "Cloud smoothing") against the numpy statement tests/cloud_mls_numpy.py:
every output and the moments byte for byte in the three forms of the walk (plain, tiles, tiles and groups), each against
the statement with that form's order, at the tile, group and block edges; the gated form; culling; the traps of
tests/test_cloud_mls_cpu.py; the refusals; the Python layer; the product.  Every operand of the C entry point lies in a
guarded buffer, and the guards are checked after every raw call."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_mls_numpy as M  # noqa: E402
import cloud_numpy as C  # noqa: E402
import test_cloud_mls_cpu as traps  # noqa: E402
from mesh_support import BLOCK, G, T, VS, Operands  # noqa: E402
from test_cloud_cluster_gpu import EPS2  # noqa: E402
from test_cloud_gpu import _build, cloud, queries  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES_N = (0, 1, 2, T - 1, T, T + 1, T * G + 1, 2 * T * G + 1)
SIZES_Q = (0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)
MODES = ("plain", 1, 2)
TINY = 1.0e-30                      # below the square of any difference of two f32 numbers here: only exact duplicates join
H2 = {kind: tuple(e for e in EPS2[kind] if e != 0.0) + (TINY,) for kind in EPS2}
KEYS = ("points", "normals", "curvature", "count", "moments")
F = np.float32


def _lib():
    import mslam_hip as _m

    return _m, _m.lib(), _m.stream_ptr()


def _index_ops(_m, ix, mode):
    return (0, 0, 0, 1) if mode == "plain" else (_m.ptr(ix["o"]), _m.ptr(ix["ws"]), ix["ws"].numel(), mode)


def _order(ix, mode):
    return None if mode == "plain" else ix["order"]


def _step(device, ix, Q, h2, mode, min_points=6, strength=1.0, qn=None, pn=None, cos_gate=0.0):
    """mslam_cloud_mls_step -> (dict of numpy arrays under KEYS, per-wave skip counts)."""
    _m, L, st = _lib()
    ops = Operands(device)
    Q = C.f32(Q)
    n = len(Q)
    q = ops.put(Q, np.float32)
    a = ops.put(C.f32(qn), np.float32) if qn is not None else None
    b = ops.put(C.f32(pn), np.float32) if pn is not None else None
    out = dict(points=ops.out(torch.float32, (n, 3)), normals=ops.out(torch.float32, (n, 3)),
               curvature=ops.out(torch.float32, (n,)), count=ops.out(torch.int32, (n,)))
    skips = ops.out(torch.int32, (4 * ((n + BLOCK - 1) // BLOCK),))
    out["moments"] = ops.out(torch.float64, (n, M.MOMENTS))
    before = ix["ws"].clone()
    rc = L.mslam_cloud_mls_step(_m.ptr(q), n, _m.ptr(ix["p"]), ix["N"], float(h2), min_points, float(strength),
                                _m.ptr(a), _m.ptr(b), float(cos_gate), *_index_ops(_m, ix, mode), _m.ptr(skips),
                                *(_m.ptr(out[k]) for k in KEYS), st)
    _m.check(rc, "cloud_mls_step")
    ops.check()
    ix["ops"].check()
    assert torch.equal(before, ix["ws"])                                    # the step only reads the index
    return {k: v.cpu().numpy() for k, v in out.items()}, skips.cpu().numpy()


def _same(got, want, n=None, what=""):
    for k in KEYS:
        w = want[k] if n is None else want[k][:n]
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (k, what)
        assert got[k].tobytes() == np.ascontiguousarray(w).tobytes(), (k, what)


_CASES = {}


def _case(device, N, kind):
    """The cloud with its index, built once per size."""
    if (N, kind) not in _CASES:
        P = cloud(N, kind)
        _CASES[N, kind] = (P, _build(device, P))
    return _CASES[N, kind]


@functools.lru_cache(maxsize=None)
def normals_for(n, seed):
    """Unit-ish normals of both signs with zero rows, a NaN row and an infinite row among them."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (n, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    v[rng.random(n) < 0.3] = F([0, 0, 1])                                    # a common direction, so that the gate passes some
    v[rng.random(n) < 0.5] *= F(-1)
    v[::7] = 0
    if n > 3:
        v[3, 1], v[2, 0] = np.nan, np.inf
    return v


# ----------------------------------------------------------------------------------------------------------------------
# the step against the statement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("N", SIZES_N)
def test_step_parity(device, N, kind):
    P, ix = _case(device, N, kind)
    Q = queries(kind)
    strength = 1.0 if kind == "lattice" else 0.75
    met = set()
    for h2 in H2[kind]:
        want = {mode: M.mls_step(Q, P, h2, 6, strength, _order(ix, mode)) for mode in ("plain", 2)}
        want[1] = want[2]
        assert np.array_equal(want["plain"]["count"], want[2]["count"])    # the forms differ by rounding only
        met.add((h2, bool(want[2]["moved"].any()), int(want[2]["count"].max(initial=0))))
        if N >= T and h2 == H2[kind][2]:
            assert 0.35 < want[2]["count"].mean() / N < 0.65                # about half the cloud joins
        for n in SIZES_Q:
            got = {}
            for mode in MODES:
                got[mode], skips = _step(device, ix, Q[:n], h2, mode, 6, strength)
                _same(got[mode], want[mode], n, (h2, n, mode))
                if mode == "plain":
                    assert not skips.any()
            _same(got[1], got[2])                                           # culling a level more changes no byte
    if N > T * G and kind == "lattice":
        assert max(c for h2, _, c in met if h2 == 1.0) > 32                 # beyond the cap of the k-NN lists
        assert all(moved for h2, moved, _ in met if h2 != TINY)
        assert [(moved, c > 6) for h2, moved, c in met if h2 == TINY] == [(False, True)]   # duplicates join, and stay


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("N", (2, T + 1, T * G + 1))
def test_gated_step_parity(device, N, kind):
    P, ix = _case(device, N, kind)
    Q = queries(kind)
    pn, qn = normals_for(N, N), normals_for(len(Q), 5)
    h2 = H2[kind][2]
    free = M.mls_step(Q, P, h2, 4, 1.0, ix["order"])
    for cos_gate in (0.0, 0.5, math.cos(math.radians(30.0)), 1.0):
        want = {mode: M.mls_step(Q, P, h2, 4, 1.0, _order(ix, mode), qn, pn, cos_gate) for mode in ("plain", 2)}
        want[1] = want[2]
        if N > T and cos_gate == 0.5:
            gated = qn.any(1) & np.isfinite(qn).all(1) & C.valid(Q)
            assert (want[2]["count"][gated] < free["count"][gated]).any() and want[2]["moved"][gated].any()
            assert np.array_equal(want[2]["count"][~gated], free["count"][~gated])
        for n in (1, 65, BLOCK + 1, 2 * BLOCK + 1):
            got = {}
            for mode in MODES:
                got[mode], _ = _step(device, ix, Q[:n], h2, mode, 4, 1.0, qn[:n], pn, cos_gate)
                _same(got[mode], want[mode], n, (cos_gate, n, mode))
            _same(got[1], got[2])


def test_step_culling(device):
    """The two clusters of test_radius_count_culling: the queries lie in the one at the lower coordinates, and with a
    radius of 0.2 the other cluster's 32 tiles are skipped by every wave at both levels; the bytes are the statement's,
    gated or not."""
    rng = np.random.default_rng(2)
    near, far = rng.uniform(0, 1, (4096, 3)), rng.uniform(0, 1, (4096, 3)) + [10.0, 0, 0]
    P = np.concatenate([far, near]).astype(np.float32)
    Q = rng.uniform(0.1, 0.9, (2 * BLOCK + 1, 3)).astype(np.float32)
    ix = _build(device, P)
    assert (ix["order"][:4096] >= 4096).all()
    h2 = 0.2 * 0.2
    pn, qn = normals_for(len(P), 1), normals_for(len(Q), 2)
    for gate in (dict(), dict(qn=qn, pn=pn, cos_gate=0.5)):
        want = {mode: M.mls_step(Q, P, h2, 6, 1.0, _order(ix, mode), **gate) for mode in ("plain", 2)}
        want[1] = want[2]
        if not gate:
            assert 40 < want["plain"]["count"].mean() < 400
        assert want[2]["moved"].mean() > 0.9
        for mode in MODES:
            got, skips = _step(device, ix, Q, h2, mode, 6, 1.0, **gate)
            _same(got, want[mode], None, mode)
            if mode == "plain":
                assert not skips.any()
            else:
                assert skips.shape == (12,) and (skips >= 32).all(), skips


def test_cpu_traps_on_the_device(device):
    def both(Q, P, h2, mp, strength, order=None, **gate):
        """The statement's answer, checked against the kernel in the three forms (the index's order is `order`)."""
        ix = _build(device, P, order=np.arange(len(P)) if order is None else order)
        want = M.mls_step(Q, P, h2, mp, strength, ix["order"], **gate)
        if order is None:
            _same(_step(device, ix, Q, h2, "plain", mp, strength, **gate)[0], want)
        for mode in (1, 2):
            _same(_step(device, ix, Q, h2, mode, mp, strength, **gate)[0], want, None, mode)
        return want

    bits = traps.bits
    for above in (True, False):
        Q, P, h2, land = traps.plane_trap(above)
        out = both(Q, P, h2, 4, 1.0)
        assert bits(out["points"]) == bits(land) and bits(out["normals"]) == bits(F([[0, 0, 1]]))
    Q, P, h2, land = traps.rim_trap()
    assert both(Q, P, h2, 5, 1.0)["count"].tolist() == [5]
    assert bits(both(Q, P, h2, 5, 1.0, order=np.int32([4, 0, 1, 2, 3]))["points"]) == bits(land)
    far = P.copy()
    far[4, 0] = np.nextafter(far[4, 0], F(np.inf))
    assert both(Q, far, h2, 5, 1.0)["moved"].tolist() == [False]
    Q, P, h2, land = traps.plane_trap()
    assert both(Q, P, h2, 5, 1.0)["moved"].tolist() == [False] and both(Q, P, h2, 4, 1.0)["moved"].tolist() == [True]
    assert both(Q, P[:3], h2, 1, 1.0)["moved"].tolist() == [True] and not both(Q, P[:2], h2, 1, 1.0)["moved"][0]
    assert bits(both(Q, P, h2, 4, 0.0)["points"]) == bits(Q)
    assert bits(both(Q, P, h2, 4, 0.5)["points"]) == bits(F([[0.25, 0.5, 0.6875]]))
    assert both(Q, np.concatenate([P, P]), h2, 8, 1.0)["count"].tolist() == [8]
    rim = Q + F([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]])
    assert both(Q, rim, 1.0, 1, 1.0)["moments"][0, 0] == 0.0
    lq, lp, lh2 = traps.line_trap()
    assert both(lq, lp, lh2, 1, 1.0)["count"].tolist() == [4]
    assert both(F([[0.25, 0.5, 0.75]]), np.tile(F([[0.25, 0.5, 0.5]]), (5, 1)), 1.0, 1, 1.0)["count"].tolist() == [5]
    odd = np.array([0x7FC12345, 0x3F000000, 0x3F000000], np.uint32).view(np.float32)[None]
    Q2 = np.concatenate([odd, Q, F([[np.inf, 0, 0]])])
    P2 = np.concatenate([F([[np.nan, 0.5, 0.5]]), P, F([[0.25, 0.5, -np.inf]])])
    out = both(Q2, P2, h2, 4, 1.0)
    assert bits(out["points"][0]) == bits(odd[0]) and out["count"].tolist() == [0, 4, 0]
    # the order is the definition's: a permuted index order is met bit for bit, and differs from the plain form's
    Q, P, h2, perm = traps.order_case()
    a, b = both(Q, P, h2, 6, 1.0), both(Q, P, h2, 6, 1.0, order=perm.astype(np.int32))
    assert bits(a["moments"]) != bits(b["moments"])
    # the gate
    Q, P, h2, land, qn, pn, c = traps.gate_trap()
    assert both(Q, P, h2, 4, 1.0, qn=qn, pn=pn, cos_gate=c)["count"].tolist() == [5]
    out = both(Q, P, h2, 4, 1.0, qn=qn, pn=pn, cos_gate=float(np.nextafter(c, 1.0)))
    assert out["count"].tolist() == [4] and bits(out["points"]) == bits(land)
    for a in (F([[0, 0, 0]]), F([[np.nan, 0, 1]]), F([[0, np.inf, 0]])):
        assert both(Q, P, h2, 4, 1.0, qn=a, pn=pn, cos_gate=0.9)["count"].tolist() == [5]
    for b in (F([0, 0, 0]), F([np.nan, 0, 1]), F([0, 0, np.inf])):
        pn2 = pn.copy()
        pn2[1] = b
        assert both(Q, P, h2, 1, 1.0, qn=qn, pn=pn2, cos_gate=2.0 ** -60)["count"].tolist() == [4]
        assert both(Q, P, h2, 1, 1.0, qn=qn, pn=pn2, cos_gate=0.0)["count"].tolist() == [5]
    sign = F([[1], [-1], [1], [-1], [-1]])
    ref = both(Q, P, h2, 4, 1.0, qn=qn, pn=pn, cos_gate=0.9)
    for a, b in ((-qn, pn), (qn, pn * sign), (-qn, pn * -sign)):
        _same(both(Q, P, h2, 4, 1.0, qn=a, pn=b, cos_gate=0.9), ref)


def test_step_refusals(device):
    _m, L, st = _lib()
    P, ix = _case(device, T + 1, "random")
    need = int(L.mslam_cloud_index_bytes(ix["N"]))
    n = 70
    nan = float("nan")
    base = dict(n=n, N=ix["N"], h2=0.04, mp=6, strength=1.0, qn=False, pn=False, cos=0.5, order=True, nbytes=need,
                levels=2, null=None)
    refused = ((dict(n=-1), -1, "negative size"), (dict(N=-1), -1, "negative size"),
               (dict(h2=0.0), -1, "h2 must be"), (dict(h2=-1.0), -1, "h2 must be"), (dict(h2=nan), -1, "h2 must be"),
               (dict(h2=float("inf")), -1, "h2 must be"), (dict(mp=0), -1, "min_points must be"),
               (dict(strength=-0.1), -1, "strength must be"), (dict(strength=1.5), -1, "strength must be"),
               (dict(strength=nan), -1, "strength must be"), (dict(qn=True), -1, "go together"),
               (dict(pn=True), -1, "go together"), (dict(qn=True, pn=True, cos=-0.1), -1, "cos_gate must be"),
               (dict(qn=True, pn=True, cos=1.1), -1, "cos_gate must be"),
               (dict(qn=True, pn=True, cos=nan), -1, "cos_gate must be"), (dict(levels=3), -1, "levels must be"),
               (dict(nbytes=need - 1), -3, f"{need} needed"), (dict(nbytes=0, levels=1), -3, f"{need} needed"),
               (dict(null="q"), -1, "null pointer"), (dict(null="points"), -1, "null pointer"),
               (dict(null="normals"), -1, "null pointer"), (dict(null="curvature"), -1, "null pointer"),
               (dict(null="count"), -1, "null pointer"), (dict(null="p"), -1, "null pointer"))
    for change, rc, text in refused:
        a = dict(base, **change)
        ops = Operands(device)
        q = ops.put(queries("random")[:n], np.float32)
        qn, pn = ops.put(normals_for(n, 1), np.float32), ops.put(normals_for(ix["N"], 2), np.float32)
        out = dict(points=ops.out(torch.float32, (n, 3)), normals=ops.out(torch.float32, (n, 3)),
                   curvature=ops.out(torch.float32, (n,)), count=ops.out(torch.int32, (n,)),
                   moments=ops.out(torch.float64, (n, M.MOMENTS)))
        skips = ops.out(torch.int32, (4,))
        arg = lambda t, name: 0 if a["null"] == name else _m.ptr(t)
        got = L.mslam_cloud_mls_step(arg(q, "q"), a["n"], arg(ix["p"], "p"), a["N"], a["h2"], a["mp"], a["strength"],
                                     _m.ptr(qn) if a["qn"] else 0, _m.ptr(pn) if a["pn"] else 0, a["cos"],
                                     _m.ptr(ix["o"]), _m.ptr(ix["ws"]), a["nbytes"], a["levels"], _m.ptr(skips),
                                     *(arg(out[k], k) for k in KEYS), st)
        assert got == rc and text in L.mslam_last_error().decode(), (change, got, L.mslam_last_error())
        torch.cuda.synchronize()
        for g in ops.all.values():
            if g.t.data_ptr() not in (q.data_ptr(), qn.data_ptr(), pn.data_ptr()):
                assert bool((g.raw == g.pat).all()), change                  # nothing written
    # cos_gate is not read without the normals; n == 0 is fine after the checks, also with null pointers
    got, _ = _step(device, ix, queries("random")[:n], 0.04, 2, cos_gate=7.0)
    _same(got, M.mls_step(queries("random")[:n], P, 0.04, 6, 1.0, ix["order"]))
    assert L.mslam_cloud_mls_step(0, 0, _m.ptr(ix["p"]), ix["N"], 0.04, 6, 1.0, 0, 0, 0.0, _m.ptr(ix["o"]),
                                  _m.ptr(ix["ws"]), need, 2, 0, 0, 0, 0, 0, 0, st) == 0
    assert L.mslam_cloud_mls_step(0, 0, _m.ptr(ix["p"]), ix["N"], -1.0, 6, 1.0, 0, 0, 0.0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0,
                                  st) == -1
    # an empty cloud: every query stays, with or without the normals
    Q = queries("random")[:n]
    empty = _build(device, P[:0])
    for mode in MODES:
        for gate in (dict(), dict(qn=normals_for(n, 1), pn=P[:0], cos_gate=0.5)):
            got, _ = _step(device, empty, Q, 0.04, mode, 1, 1.0, **gate)
            _same(got, M.mls_step(Q, P[:0], 0.04, 1, 1.0, None, **gate))
            assert got["points"].tobytes() == Q.tobytes() and not got["count"].any()


# ----------------------------------------------------------------------------------------------------------------------
# the Python layer
# ----------------------------------------------------------------------------------------------------------------------
def _same_step(got, want):
    assert sorted(got) == ["count", "curvature", "moved", "normals", "points"]
    for k in ("points", "normals", "curvature", "count"):
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.tobytes() == want[k].tobytes(), k
    assert got["moved"].dtype == torch.bool and np.array_equal(got["moved"].cpu().numpy(), want["moved"])


def _same_smooth(got, want):
    (gp, gc, gi), (wp, wi) = got, want
    assert gp.dtype == torch.float32 and gp.cpu().numpy().tobytes() == wp.tobytes()
    assert sorted(gi) == sorted(wi)
    for k in ("normals", "curvature", "count"):
        g = gi[k].cpu().numpy()
        assert g.dtype == wi[k].dtype and g.tobytes() == wi[k].tobytes(), k
    assert np.array_equal(gi["moved"].cpu().numpy(), wi["moved"]) and gi["n_valid"] == wi["n_valid"]
    for k in ("rms_displacement", "max_displacement"):
        assert isinstance(gi[k], float) and abs(gi[k] - wi[k]) <= 1e-12 * max(wi[k], 1e-30), k


def test_python_cloud_mls(device):
    from mast3r_slam.tsdf import CloudIndex, cloud_mls

    P = cloud(T * G + 1, "random")
    Q = queries("random").copy()
    Q[9] = np.nan
    p, q = torch.from_numpy(P).to(device), torch.from_numpy(Q).to(device)
    cx = CloudIndex(p)
    order = cx.order.cpu().numpy()
    radius = 0.3
    h2 = radius * radius
    want = M.mls_step(Q, P, h2, 6, 1.0, order)
    assert want["count"].max() > 32 and want["count"][9] == 0 and want["moved"].mean() > 0.5
    for index in (True, cx):
        _same_step(cloud_mls(q, p, radius, index=index), want)
    _same_step(cloud_mls(q, p, radius, index=None), M.mls_step(Q, P, h2, 6, 1.0, None))   # the identity order
    _same_step(cloud_mls(q, p, radius, 40, 0.5, index=cx), M.mls_step(Q, P, h2, 40, 0.5, order))
    qn, pn = normals_for(len(Q), 3), normals_for(len(P), 4)
    got = cloud_mls(q, p, radius, normals=tuple(torch.from_numpy(a).to(device) for a in (qn, pn)), edge_angle=60.0,
                    index=cx)
    _same_step(got, M.mls_step(Q, P, h2, 6, 1.0, order, qn, pn, math.cos(math.radians(60.0))))
    assert tuple(cloud_mls(q[:0], p, radius)["points"].shape) == (0, 3)
    assert torch.equal(cloud_mls(q[:5], p[:0], radius)["points"], q[:5])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius must be positive and finite"):
            cloud_mls(q, p, bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="min_points must be an integer >= 1"):
            cloud_mls(q, p, radius, bad)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="strength must be in"):
            cloud_mls(q, p, radius, strength=bad)
    for kw in (dict(edge_angle=30.0), dict(normals=(q, p))):
        with pytest.raises(ValueError, match="go together"):
            cloud_mls(q, p, radius, **kw)
    for bad in (-1.0, 91.0, float("nan")):
        with pytest.raises(ValueError, match="edge_angle must be in"):
            cloud_mls(q, p, radius, normals=(q, p), edge_angle=bad)
    with pytest.raises(ValueError, match="normals must be"):
        cloud_mls(q, p, radius, normals=(p, q), edge_angle=30.0)
    with pytest.raises(ValueError, match="built for another cloud"):
        cloud_mls(q, p.clone(), radius, index=cx)
    with pytest.raises(TypeError, match="index must be"):
        cloud_mls(q, p, radius, index="yes")
    with pytest.raises(TypeError, match="must be a device tensor"):
        cloud_mls(Q, p, radius)


def test_python_smooth_cloud(device):
    from mast3r_slam.tsdf import CloudIndex, smooth_cloud

    rng = np.random.default_rng(5)
    a, b = [g.reshape(-1) for g in np.meshgrid(np.arange(24) * 0.01, np.arange(24) * 0.01, indexing="ij")]
    sheets = np.concatenate([np.stack([a + 0.005, b, 0 * a], 1), np.stack([0 * a, b, a + 0.005], 1)])
    P = (sheets + rng.normal(0, 0.003, sheets.shape)).astype(F)[rng.permutation(len(sheets))]
    P[[7, 500]] = np.nan
    col = torch.from_numpy(rng.integers(0, 255, (len(P), 3)).astype(np.uint8)).to(device)
    p = torch.from_numpy(P).to(device)
    before = p.clone()
    cx = CloudIndex(p)
    order = cx.order.cpu().numpy()
    for iterations in (1, 3):
        for edge_angle in (None, 30.0):
            want = M.smooth(P, 0.04, iterations, 6, 1.0, edge_angle, order)
            got = smooth_cloud(p, 0.04, iterations, edge_angle=edge_angle, colors=col, index=cx)
            _same_smooth(got, want)
            assert got[1].data_ptr() == col.data_ptr() or torch.equal(got[1], col)
            assert got[2]["n_valid"] == len(P) - 2 and 0.0 < got[2]["rms_displacement"] <= got[2]["max_displacement"]
            out = got[0].cpu().numpy()
            assert out[[7, 500]].tobytes() == P[[7, 500]].tobytes() and not got[2]["moved"][[7, 500]].any()
    _same_smooth(smooth_cloud(p, 0.04, 2, 4, 0.5, 45.0, index=None), M.smooth(P, 0.04, 2, 4, 0.5, 45.0, None))
    _same_smooth(smooth_cloud(p, 0.04), M.smooth(P, 0.04, order=order))
    assert smooth_cloud(p, 0.04)[1] is None and torch.equal(p.view(torch.int32), before.view(torch.int32))
    empty = smooth_cloud(p[:0], 0.04, edge_angle=30.0)
    assert tuple(empty[0].shape) == (0, 3) and empty[2]["n_valid"] == 0 and empty[2]["rms_displacement"] == 0.0
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="iterations must be an integer >= 1"):
            smooth_cloud(p, 0.04, bad)
    with pytest.raises(ValueError, match="radius must be positive and finite"):
        smooth_cloud(p, 0.0)
    with pytest.raises(ValueError, match="colors must be"):
        smooth_cloud(p, 0.04, colors=col[:-1])
    with pytest.raises(ValueError, match="edge_angle must be in"):
        smooth_cloud(p, 0.04, edge_angle=120.0)


def test_corner_fixture_on_the_device(device):
    """The fixture of tests/test_cloud_mls_cpu.py: the bytes are the statement's, so the figures are."""
    from mast3r_slam.tsdf import smooth_cloud

    P, _ = traps.corner()
    p = torch.from_numpy(P).to(device)
    out = {}
    for gated in (False, True):
        got = smooth_cloud(p, traps.RADIUS, edge_angle=traps.EDGE_ANGLE if gated else None, index=None)
        _same_smooth(got, traps.corner_smoothed(1, gated))
        out[gated] = smooth_cloud(p, traps.RADIUS, edge_angle=traps.EDGE_ANGLE if gated else None)[0].cpu().numpy()
    f = traps.corner_figures(out[False], out[True])                          # the product's form: the index's order
    print("corner fixture on the device, mm:", {k: round(1e3 * v, 3) for k, v in f.items()})
    traps.check_corner(f)


# ----------------------------------------------------------------------------------------------------------------------
# the product
# ----------------------------------------------------------------------------------------------------------------------
def test_slam_system_cloud_smooth(device, monkeypatch):
    """The 20-frame run of the product tests.  keyframe_cloud(smooth=None) returns what keyframe_cloud() returns, byte for
    byte; with smooth= the cloud is smooth_cloud of the unsmoothed one, colours and order kept; evaluate_cloud and
    cloud_planes hand the keyword on."""
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from mast3r_slam.tsdf import smooth_cloud
    from test_slam_system_gpu import RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    thr = 2.0
    rule = dict(radius=2.0 * VS, edge_angle=30.0)
    seen = []
    try:
        system.run(_frames(list(range(0, 60, 3)), device))
        plain = system.keyframe_cloud(conf_threshold=thr)
        none = system.keyframe_cloud(conf_threshold=thr, smooth=None)
        thin = system.keyframe_cloud(conf_threshold=thr, voxel=VS)
        thin_none = system.keyframe_cloud(conf_threshold=thr, voxel=VS, smooth=None)
        s2 = system.keyframe_cloud(conf_threshold=thr, voxel=VS, smooth=rule)
        s3 = system.keyframe_cloud(conf_threshold=thr, voxel=VS, smooth=rule, normals=16)
        u3 = system.keyframe_cloud(conf_threshold=thr, voxel=VS, normals=16)
        with pytest.raises(ValueError, match="smooth needs a radius"):
            system.keyframe_cloud(conf_threshold=thr, voxel=VS, smooth=dict(iterations=2))
        # the keyword is handed on: keyframe_cloud sees it
        inner = system.keyframe_cloud
        monkeypatch.setattr(system, "keyframe_cloud", lambda *a, **kw: (seen.append(kw.get("smooth")), inner(*a, **kw))[1])
        scored = system.evaluate_cloud(thin[0], conf_threshold=thr, smooth=rule, voxel=0)
        unscored = system.evaluate_cloud(thin[0], conf_threshold=thr, voxel=0)
        planes = system.cloud_planes(conf_threshold=thr, voxel=VS, smooth=rule, max_planes=2)
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    assert len(plain) == len(none) == len(thin) == len(thin_none) == len(s2) == 2 and len(s3) == len(u3) == 3
    for a, b in zip(plain + thin, none + thin_none):
        assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    want = smooth_cloud(thin[0], colors=thin[1], **rule)
    assert torch.equal(s2[0], want[0]) and torch.equal(s2[1], thin[1]) and s2[0].shape == thin[0].shape
    assert torch.equal(s3[0], s2[0]) and torch.equal(s3[1], s2[1]) and s3[2].shape == s3[0].shape
    assert want[2]["moved"].float().mean() > 0.5 and not torch.equal(s2[0], thin[0])
    assert 0.0 < want[2]["max_displacement"] <= 2.0 * VS * (1.0 + 1e-6)       # the plane passes through the ball
    assert not torch.equal(s3[2], u3[2])                                      # the normals are those of the moved points
    assert seen == [rule, None, rule]
    assert scored["n_pred"] == unscored["n_pred"] > 0 and scored["accuracy"] != unscored["accuracy"]
    assert torch.equal(planes[0], s2[0])
    print(f"{len(plain[0])} points, {len(thin[0])} thinned, {int(want[2]['moved'].sum())} moved, rms displacement "
          f"{1e3 * want[2]['rms_displacement']:.2f} mm, accuracy {scored['accuracy']:.5f} smoothed, "
          f"{unscored['accuracy']:.5f} not")
