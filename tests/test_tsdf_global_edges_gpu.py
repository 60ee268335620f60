"""GPU edge tests (-m gpu) of csrc/tsdf_global.hip through TSDFVolume / TSDFPoseOptimizer and the C ABI: the emit band
arithmetic, the replay switch points (48 / 49 / 2048 / 2049 samples in a voxel, more big voxels than blocks), the key
range and its reports, non-finite confidences and coordinates, probe wrap-around and the first-touch state across a
rehash, every gate of the query, and the pose step at its sizes and thresholds.

Inputs and references come from tests/tsdf_global_refs.py; tests/test_tsdf_global_refs_cpu.py shows, without a GPU, that
every input reaches its branch and that oracle.TSDFVolume equals the literal NumPy reference bit for bit on them.
Bars (those of tests/test_tsdf_gpu.py): keys and fused count exact, weight rtol 1e-12, tsdf rtol 1e-11 / atol 1e-13;
query status exact, value rtol 1e-12 / atol 1e-14, gradient rtol 1e-9 / atol 1e-12; H, b rtol 1e-9 / atol 1e-12, used
exact; one pose update atol 2e-4."""
import os
import sys

import numpy as np
import pytest
import torch

import oracle
from mast3r_slam import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_global_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1, 1], np.float32)


def _vol(device, vs, tr, mw=100.0, capacity=1 << 16, min_weight=1.0e-3, **kw):
    from mast3r_slam.tsdf import TSDFVolume

    return TSDFVolume(vs, tr, mw, min_weight, capacity=capacity, device=device, **kw)


def _same_voxels(got, want):
    k, t, w = got
    k_ref, t_ref, w_ref = want
    np.testing.assert_array_equal(k, k_ref)
    np.testing.assert_allclose(w, w_ref, rtol=1e-12)
    np.testing.assert_allclose(t, t_ref, rtol=1e-11, atol=1e-13)


def _same_query(got, want):
    val, grad, st = (x.cpu().numpy() if torch.is_tensor(x) else x for x in got)
    v_ref, g_ref, s_ref = want
    np.testing.assert_array_equal(st, s_ref)
    np.testing.assert_allclose(val, v_ref, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(grad, g_ref, rtol=1e-9, atol=1e-12)


def _both(device, case, capacity=1 << 16, passes=1):
    """The case integrated `passes` times into a device volume and the oracle, compared after every call.
    integrate() reads the header's overflow word and raises unless it is 0: no sample dropped, the max_band cap never
    fires."""
    p, c, o, vs, tr, mw, ss = case
    vol, ref = _vol(device, vs, tr, mw, capacity), oracle.TSDFVolume(vs, tr, mw)
    for _ in range(passes):
        assert vol.integrate(p, c, o, ss) == ref.integrate(p, c, o, ss)    # raises if the overflow word is not 0
        _same_voxels(vol.voxels(), ref.voxels())
    return vol, ref


# ----------------------------------------------------------------------------------------------------------------------
# 1-3  emit band arithmetic and the replay switch points
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in R.CASES if n.startswith("band_")])
def test_band_sweep(device, name):
    vol, _ = _both(device, R.CASES[name]())
    assert len(vol.voxels()[0]) >= 5


@pytest.mark.parametrize("name", ["replay_thresholds", "replay_floor"])
def test_replay_thresholds(device, name):
    """Voxels with exactly 47, 48 (one thread), 49, 2048 (one wave) and 2049 (selection scan) samples, arrival order
    shuffled, max_weight reached early; the second call replays onto averaged voxels.  (The selection scan reads its
    segment once per sample, one lane at work: the recipe's step keeps every voxel at one sample per ray, so 2049 is the
    longest segment and the call stays well under a second.)  With these weights the end value does not depend on the
    order beyond its rounding (tests/tsdf_global_refs.py: replay_thresholds); `replay_floor` is the same input with
    confidences of 1e-13, where the divisor's 1e-9 floor makes the last samples decide: a wrong order fails there."""
    vol, _ = _both(device, R.CASES[name](), passes=2)
    assert (vol.voxels()[2] == 5.0).any() == (name == "replay_thresholds")


def test_more_big_voxels_than_blocks(device):
    _both(device, R.CASES["many_big"]())


# ----------------------------------------------------------------------------------------------------------------------
# 4  key range and reports
# ----------------------------------------------------------------------------------------------------------------------
def test_key_range_ends_are_stored(device):
    vol, _ = _both(device, R.CASES["key_edges"](), capacity=1 << 10)
    assert vol.voxels()[0][:, 0].max() == R.KEY_BIAS - 1
    vol, _ = _both(device, R.CASES["key_edges_low"](), capacity=1 << 10)
    assert vol.voxels()[0][:, 0].min() == -R.KEY_BIAS


def test_sample_beyond_the_key_range_is_reported(device):
    """Code 1; everything in range is fused, the samples of the same ray included."""
    p, c, o, vs, tr, mw, ss = R.key_overflow_code1()
    vol, ref = _vol(device, vs, tr, mw, 1 << 10), oracle.TSDFVolume(vs, tr, mw)
    with pytest.raises(RuntimeError, match=r"overflow \(code 1\)"):
        vol.integrate(p, c, o, ss)
    assert int(vol._header()[4]) == ref.integrate(p, c, o, ss)
    k, t, w = ref.voxels()
    ok = R.in_key_range(k)
    assert 0 < ok.sum() < len(k)
    _same_voxels(vol.voxels(), (k[ok], t[ok], w[ok]))


def test_ray_of_2_to_the_20_samples_is_reported(device):
    """Code 3; the point is dropped as a whole (it still counts as fused, as it would in the reference), the others are
    fused as if it were not there."""
    (p, c, o, vs, tr, mw, ss), at = R.long_ray_code3()
    others = np.arange(len(p)) != at
    vol, ref = _vol(device, vs, tr, mw), oracle.TSDFVolume(vs, tr, mw)
    with pytest.raises(RuntimeError, match=r"overflow \(code 3\)"):
        vol.integrate(p, c, o, ss)
    assert int(vol._header()[4]) == ref.integrate(p[others], c[others], o, ss) + 1
    _same_voxels(vol.voxels(), ref.voxels())


# ----------------------------------------------------------------------------------------------------------------------
# 5  confidences and coordinates that are not finite
# ----------------------------------------------------------------------------------------------------------------------
def test_nonfinite_confidences_and_coordinates(device):
    """0, negative, -inf: nothing applied.  +inf: applied (weights inf, values inf / NaN as in the reference).  NaN: the
    reference lets `weight <= 0` pass and stores NaN; the kernel skips such samples (`if (!(w > 0.0)) continue`) - the
    documented deviation, pinned here: the voxels are the oracle's on the list without the NaN-confidence points, the
    fused count is the oracle's on the whole list."""
    p, c, o, vs, tr, mw, ss = R.CASES["conf_edges"]()
    keep = ~np.isnan(c)
    vol, full, ref = _vol(device, vs, tr, mw), oracle.TSDFVolume(vs, tr, mw), oracle.TSDFVolume(vs, tr, mw)
    assert vol.integrate(p, c, o, ss) == full.integrate(p, c, o, ss)
    ref.integrate(p[keep], c[keep], o, ss)
    _same_voxels(vol.voxels(), ref.voxels())
    assert np.isinf(vol.voxels()[2]).any() and not np.isnan(vol.voxels()[2]).any()
    # a NaN origin: every ray is skipped, the table is left as it was
    p, c, o2, vs, tr, mw, ss = R.CASES["nan_origin"]()
    assert vol.integrate(p, c, o2, ss) == 0
    _same_voxels(vol.voxels(), ref.voxels())
    assert int(vol._header()[1]) == 0


# ----------------------------------------------------------------------------------------------------------------------
# 6  the table: probe wrap-around, growth, first-touch state across the rehash
# ----------------------------------------------------------------------------------------------------------------------
def _growth_batches():
    rng = np.random.default_rng(64)
    origin = np.array([0.02, -0.01, 0.015], np.float32)
    out = []
    for n, ss in ((60, 1.0), (120, 0.5), (240, 1.0)):
        d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        out.append(((origin + d * rng.uniform(0.1, 0.3, (n, 1))).astype(np.float32), rng.uniform(0.5, 3.0, n), ss))
    return origin, out


def test_probe_wrap_and_state_across_rehash(device):
    p, c, o, vs, tr, mw, ss = R.CASES["wrap_table"]()
    small, big, ref = _vol(device, vs, tr, mw, R.WRAP_CAPACITY), _vol(device, vs, tr, mw, 1 << 16), oracle.TSDFVolume(vs, tr, mw)
    assert small.integrate(p, c, o, ss) == ref.integrate(p, c, o, ss) == big.integrate(p, c, o, ss)
    _same_voxels(small.voxels(), ref.voxels())
    total, _ = R.sample_counts(p, c, o, vs, tr, mw, ss)
    origin, batches = _growth_batches()
    caps = [small.capacity]
    for pts, conf, step in batches:
        reserve = 10 * len(pts)               # a ray of this setting has at most 2 * trunc / step + 1 = 9 samples
        n, cap = small.maintain(reserve=reserve)
        assert n + reserve <= 0.5 * cap and cap > caps[-1]
        caps.append(cap)
        for v in (small, big, ref):
            v.integrate(pts, conf, origin, step)
        for k, m in R.sample_counts(pts, conf, origin, vs, tr, mw, step)[0].items():
            total[k] = total.get(k, 0) + m
    assert len(caps) == 4                                          # grew three times
    ks, ts, ws = small.voxels()
    kb, tb, wb = big.voxels()
    for a, b in ((ks, kb), (ts, tb), (ws, wb)):
        np.testing.assert_array_equal(a, b)
    _same_voxels((ks, ts, ws), ref.voxels())
    # queries around every voxel centre: first-touch-only and averaged voxels as neighbours of both kinds
    once = np.array([total[tuple(k)] == 1 for k in ks.tolist()])
    kinds = set().union(*(cl[1] for cl in R.classify_queries(ks, ws, once, 1.0e-3, ks)))
    assert kinds == {"ff", "fa", "aa"} and 1000 < len(ks) < 4000 and 100 < once.sum() < len(ks) - 100
    q = np.concatenate((R.centres(ks, vs), R.centres(ks + np.array([0, 1, 0]), vs)))       # about 2 000 points
    got_s, got_b = small.query_batch(q), big.query_batch(q)
    for a, b in zip(got_s, got_b):
        assert torch.equal(a, b)
    _same_query(got_s, ref.query(q))


# ----------------------------------------------------------------------------------------------------------------------
# 7  query gates
# ----------------------------------------------------------------------------------------------------------------------
def _sparse(device, min_weight=1.0e-3, min_weight_ref=None, seed=11):
    p, c, o, vs, tr, mw = R.sparse_rays(seed)
    vol = _vol(device, vs, tr, mw, min_weight=min_weight)
    ref = oracle.TSDFVolume(vs, tr, mw, min_weight if min_weight_ref is None else min_weight_ref)
    n = len(p) // 2
    total = {}
    for sl, ss in ((slice(0, n), 1.0), (slice(n, None), 0.5)):
        assert vol.integrate(p[sl], c[sl], o, ss) == ref.integrate(p[sl], c[sl], o, ss)
        for k, m in R.sample_counts(p[sl], c[sl], o, vs, tr, mw, ss)[0].items():
            total[k] = total.get(k, 0) + m
    return vol, ref, vs, total


def test_query_pairs_and_states(device):
    """0, 1, 2 and 3 valid axis pairs; pairs of two first-touch voxels (float32 difference), mixed and averaged."""
    vol, ref, vs, total = _sparse(device)
    keys, t, w = vol.voxels()
    _same_voxels((keys, t, w), ref.voxels())
    once = np.array([total[tuple(k)] == 1 for k in keys.tolist()])
    cls = R.classify_queries(keys, w, once, 1.0e-3, keys)
    assert {c[0] for c in cls} == {0, 1, 2, 3} and set().union(*(c[1] for c in cls)) == {"ff", "fa", "aa"}
    q = np.concatenate((R.centres(keys, vs), R.centres(keys + np.array([1, 0, 0]), vs), R.centres(keys - np.array([0, 0, 1]), vs)))
    got = vol.query_batch(q)
    _same_query(got, ref.query(q))
    assert set(np.unique(got[2].cpu().numpy())) == {0, 1, 2}
    # the literal reference on the device's own voxels: the same answers, status for status
    lit = R.LiteralVolume(vs, 0.06)
    lit.load(keys, t, w, once)
    _same_query(got, lit.query_batch(q))


def test_query_weight_equal_to_min_weight(device):
    """`weight < min_weight` rejects: a voxel whose weight IS min_weight answers, one ulp more and it does not.  Device
    and oracle weights agree to 1e-12 only, so each gets its own dumped weight of the same voxel."""
    vol0, ref0, vs, _ = _sparse(device)
    keys, _, w = vol0.voxels()
    w_ref = ref0.voxels()[2]
    i = int(np.argsort(w)[len(w) // 2])
    q = R.centres(keys, vs)
    n_valid = []
    for bump in (False, True):
        mw_dev, mw_ref = (np.nextafter(x, np.inf) if bump else x for x in (float(w[i]), float(w_ref[i])))
        vol, ref, _, _ = _sparse(device, min_weight=mw_dev, min_weight_ref=mw_ref)
        got = vol.query_batch(q)
        _same_query(got, ref.query(q))
        st = got[2].cpu().numpy()
        assert (st[i] == 0) == bump
        n_valid.append(int((st > 0).sum()))
    assert n_valid[0] > n_valid[1]


def test_query_equal_neighbours_give_no_gradient(device):
    calls, (vs, tr, mw, ss) = R.equal_neighbours()
    vol, ref = _vol(device, vs, tr, mw, 1 << 10), oracle.TSDFVolume(vs, tr, mw)
    for p, c, o in calls:
        assert vol.integrate(p, c, o, ss) == ref.integrate(p, c, o, ss)
    keys, t, w = vol.voxels()
    _same_voxels((keys, t, w), ref.voxels())
    assert t[0] == t[2]
    got = vol.query_batch(R.centres(keys, vs))
    _same_query(got, ref.query(R.centres(keys, vs)))
    assert got[2].cpu().tolist() == [1, 1, 1] and not got[1].any()


def test_query_neighbour_out_of_the_key_range(device):
    """Centre voxel at index 2^20 - 1: its +x neighbour has no key; the pair is missing, nothing else changes."""
    p, c, o, vs, tr, mw, ss = R.CASES["key_edges"]()
    vol, ref = _both(device, (p, c, o, vs, tr, mw, ss), capacity=1 << 10)
    keys = vol.voxels()[0]
    edge = keys[keys[:, 0] == R.KEY_BIAS - 1]
    assert len(edge) > 0
    q = np.concatenate((R.centres(keys, vs), R.centres(edge + np.array([1, 0, 0]), vs)))
    got = vol.query_batch(q)
    _same_query(got, ref.query(q))
    st = got[2].cpu().numpy()
    assert (st[:len(keys)] > 0).all() and (st[len(keys):] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 8  NaN and inf query points
# ----------------------------------------------------------------------------------------------------------------------
def _pose_step(vol, pts, cf, pose=None, cam=0, update=0, lookup=None, lam=0.15, damping=1.0e-4):
    """mslam_tsdf_pose_step / _lookup through the C ABI: (H, b, used) device tensors; `pose` is updated in place."""
    import mslam_hip as _m

    dev = vol.device
    H = torch.zeros((7, 7), dtype=torch.float64, device=dev)
    b = torch.zeros(7, dtype=torch.float64, device=dev)
    used = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(64 * 36 * 8, dtype=torch.uint8, device=dev)
    tail = (pts.shape[0], _m.ptr(pose), cam, vol.voxel_size, vol.min_weight, lam, damping, update, _m.ptr(H), _m.ptr(b),
            _m.ptr(used), _m.ptr(ws), ws.numel(), _m.stream_ptr())
    if lookup is None:
        rc = _m.lib().mslam_tsdf_pose_step(_m.ptr(vol._table), vol.capacity, _m.ptr(pts), _m.ptr(cf), *tail)
    else:
        rc = _m.lib().mslam_tsdf_pose_step_lookup(_m.ptr(lookup), _m.ptr(pts), _m.ptr(cf), *tail)
    _m.check(rc, "tsdf_pose_step")
    return H, b, used


def test_nan_and_inf_query_points_miss_the_table(device):
    """floor(NaN / vs) has no voxel: the reference's astype(int) gives INT64_MIN and misses.  A cast of NaN on the device
    gives index 0, and the slabs through index 0 are populated here - status, look-up, normal equations and the refined
    pose must not see them."""
    from lietorch_hip import Sim3
    from mast3r_slam.tsdf import TSDFPoseOptimizer

    rng = np.random.default_rng(8)
    vs, tr = 0.03, 0.12
    o = np.array([0.011, 0.017, 0.013], np.float32)
    d = rng.normal(size=(1500, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = (o + d * rng.uniform(0.05, 0.3, (1500, 1))).astype(np.float32)
    c = rng.uniform(0.5, 3.0, 1500)
    vol, ref = _both(device, (p, c, o, vs, tr, 100.0, 0.5))
    have = {tuple(k) for k in vol.voxels()[0].tolist()}
    u = np.array([-0.135, -0.075, 0.045, 0.075, 0.105])
    a, b = (g.reshape(-1) for g in np.meshgrid(u, u))
    h = np.full_like(a, 0.015)
    finite = np.concatenate((np.stack((h, a, b), -1), np.stack((a, h, b), -1), np.stack((a, b, h), -1),
                             [[0.015, 0.015, 0.015]])).astype(np.float32)
    for q in finite:       # the voxel a NaN coordinate would be read as exists
        assert tuple(np.floor(q / np.float32(vs)).astype(int).tolist()) in have
    assert (0, 0, 0) in have
    st = vol.query_batch(finite)[2].cpu().numpy()
    assert (st == 2).all()                                    # ... with a gradient
    bad = finite.copy()
    bad[:25, 0] = np.nan; bad[25:50, 1] = np.nan; bad[50:75, 2] = np.nan; bad[75] = np.nan
    bad = np.concatenate((bad, [[np.inf, 0.1, 0.1], [0.1, -np.inf, 0.1], [np.inf, np.inf, -np.inf], [np.nan, np.inf, 0.1],
                                [3.0e38, 0.1, 0.1], [0.1, -3.0e38, 0.1]])).astype(np.float32)
    val, grad, st = vol.query_batch(bad)
    _same_query((val, grad, st), ref.query(bad))
    assert not st.any() and not val.any() and not grad.any()
    assert not vol.lookup7(vol._dev(bad, torch.float32)).any()
    # pose system and refinement: the same bits with and without them appended (every usable point keeps its thread,
    # one block either way, and a skipped point adds nothing to the sums)
    good = (finite + rng.normal(0, 0.004, finite.shape)).astype(np.float32)
    both = np.concatenate((good, bad))
    assert (len(good) + 255) // 256 == (len(both) + 255) // 256
    cg = rng.uniform(0.1, 3.0, len(good)).astype(np.float32)
    cb = np.concatenate((cg, np.ones(len(bad), np.float32)))
    opt = TSDFPoseOptimizer(vol, None, {"lambda": 0.15, "damping": 1e-4}, False, device)
    H0, b0, u0 = opt.normal_equations(good, cg)
    H1, b1, u1 = opt.normal_equations(both, cb)
    assert int(u0) > 40 and torch.isfinite(H1).all() and torch.isfinite(b1).all()
    assert torch.equal(H0, H1) and torch.equal(b0, b1) and torch.equal(u0, u1)
    pose = IDENTITY.copy(); pose[:3] = (0.003, -0.002, 0.001)
    new0 = opt.refine_pose(Sim3(torch.from_numpy(pose).reshape(1, 8).to(device)), good, cg, iterations=2).data
    new1 = opt.refine_pose(Sim3(torch.from_numpy(pose).reshape(1, 8).to(device)), both, cb, iterations=2).data
    assert torch.isfinite(new1).all() and torch.equal(new0, new1)
    assert not torch.equal(new0.cpu().reshape(-1), torch.from_numpy(pose))


# ----------------------------------------------------------------------------------------------------------------------
# 9  pose step
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room(device):
    """A small room view fused once; the literal reference holds the device's own voxels (first-touch state from the
    sample counts), so the pose comparisons below are about the query and the normal equations alone."""
    T = synthetic.camera_pose(0)
    X = synthetic.render_pointmap(T, 48, 64).reshape(-1, 3).astype(np.float32)
    pw = synthetic.sim3_act(T, X).astype(np.float32)
    org = T[:3].astype(np.float32)
    conf = np.full(len(X), 2.0)
    vol = _vol(device, 0.03, 0.12, capacity=1 << 18)
    ref = oracle.TSDFVolume(0.03, 0.12)
    assert vol.integrate(pw, conf, org) == ref.integrate(pw, conf, org)
    keys, t, w = vol.voxels()
    _same_voxels((keys, t, w), ref.voxels())
    counts, _ = R.sample_counts(pw, conf, org, 0.03, 0.12)
    lit = R.LiteralVolume(0.03, 0.12)
    lit.load(keys, t, w, [counts[tuple(k)] == 1 for k in keys.tolist()])
    rng = np.random.default_rng(9)
    n = 64 * 256 + 300
    pool = (pw[rng.integers(0, len(pw), n)] + rng.normal(0, 0.01, (n, 3))).astype(np.float32)
    pool[::9] += 50.0                                              # far from every voxel
    st = lit.query_batch(pool)[2]
    first = int(np.flatnonzero(st == 2)[0])
    pool[[0, first]] = pool[[first, 0]]                            # the single point of n = 1 is a usable one
    st[[0, first]] = st[[first, 0]]
    assert set(np.unique(st)) == {0, 1, 2}
    return dict(vol=vol, ref=ref, lit=lit, T=T.astype(np.float32), X=X, pool=pool, status=st,
                conf=rng.uniform(0.1, 3.0, n).astype(np.float32))


def _opt(vol, device, lam=0.15):
    from mast3r_slam.tsdf import TSDFPoseOptimizer

    return TSDFPoseOptimizer(vol, None, {"lambda": lam, "damping": 1e-4}, False, device)


@pytest.mark.parametrize("n", [0, 1, 255, 257, 64 * 256 + 300])
def test_normal_equations_at_block_edges(device, room, n):
    """One point, one short of and one past a block, and more points than 64 blocks hold (the grid-stride loop)."""
    pts, cf = room["pool"][:n], room["conf"][:n]
    H, b, used = _opt(room["vol"], device).normal_equations(pts, cf)
    H_ref, b_ref, used_ref = R.literal_pose_system(room["lit"], pts, cf, 0.15)
    assert int(used) == used_ref == int((room["status"][:n] == 2).sum())
    assert (n == 0) == (used_ref == 0)
    np.testing.assert_allclose(H.cpu().numpy(), H_ref, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(b.cpu().numpy(), b_ref, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("where", ["below", "at", "above"])
def test_weight_gate_of_the_pose_system(device, room, where):
    """lambda * conf (float32) just below, exactly at and just above 1e-6 on every row: at the gate the reference keeps
    the float32 product (9.99999997e-7), below it the double constant - 2.5e-9 apart, and with 4 000 rows beyond the bars
    (tests/test_tsdf_global_refs_cpu.py::test_pose_weight_gate shows that the other branch fails them)."""
    pts = room["pool"][room["status"] == 2][:4000]
    cf = R.gate_confidences(0.15, where, len(pts))
    H, b, used = _opt(room["vol"], device).normal_equations(pts, cf)
    H_ref, b_ref, used_ref = R.literal_pose_system(room["lit"], pts, cf, 0.15)
    assert int(used) == used_ref == len(cf)
    np.testing.assert_allclose(H.cpu().numpy(), H_ref, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(b.cpu().numpy(), b_ref, rtol=1e-9, atol=1e-12)


def test_five_usable_points_leave_the_pose_six_move_it(device, room):
    """`if len(residuals) < 6: break`.  The identity pose moves no point, so the camera-frame points are the world points."""
    from lietorch_hip import Sim3

    usable = room["pool"][room["status"] == 2]
    rest = room["pool"][room["status"] != 2][:300]
    opt = _opt(room["vol"], device)
    for k, moves in ((5, False), (6, True)):
        pts = np.concatenate((rest[:150], usable[:k], rest[150:]))
        cf = np.full(len(pts), 1.5, np.float32)
        assert int(opt.normal_equations(pts, cf)[2]) == k
        start = torch.from_numpy(IDENTITY).reshape(1, 8).to(device)
        new = opt.refine_pose(Sim3(start.clone()), pts, cf, iterations=1).data
        assert torch.equal(new, start) != moves and torch.isfinite(new).all()


def test_camera_frame_points_equal_moved_world_points(device, room):
    from lietorch_hip import Sim3

    vol = room["vol"]
    pose = room["T"].copy()
    pose[:3] += np.array([0.004, -0.003, 0.002], np.float32)
    pose_d = torch.from_numpy(pose).to(device)
    X = vol._dev(room["X"][::2], torch.float32)
    cf = vol._dev(room["conf"][:len(X)], torch.float32)
    world = Sim3(pose_d.reshape(1, 8)).act(X).contiguous()
    cam = _pose_step(vol, X, cf, pose=pose_d, cam=1)
    wld = _pose_step(vol, world, cf)
    assert int(cam[2]) > 500
    for a, b in zip(cam, wld):
        assert torch.equal(a, b)
    assert torch.equal(pose_d.cpu(), torch.from_numpy(pose))       # update_pose = 0 leaves it alone


def test_one_pose_update_against_the_fp64_reference(device, room, capsys):
    """delta from the reference's own H, b in float64, rounded to float32, retracted by oracle.sim3_retr; the bar is the
    one-step bar of test_pose_refinement_matches_oracle_iteration."""
    from lietorch_hip import Sim3

    X, cf = room["X"][::2], room["conf"][:len(room["X"][::2])]
    bad = room["T"].copy()
    bad[:3] += np.array([0.004, -0.003, 0.002], np.float32)
    H, b, used = R.literal_pose_system(room["lit"], oracle.sim3_act(bad, X), cf, 0.15)
    assert used >= 6
    want = oracle.sim3_retr(R.literal_step(H, b, 1e-4), bad)[0]
    new = _opt(room["vol"], device).refine_pose(Sim3(torch.from_numpy(bad).reshape(1, 8).to(device)), X, cf, iterations=1)
    got = new.data.cpu().numpy()[0]
    with capsys.disabled():
        print(f"\n[tsdf pose step] max |pose - fp64 reference| = {np.abs(got - want).max():.3e} "
              f"(step {np.abs(want - bad).max():.3e}, used {used})")
    assert np.abs(want - bad).max() > 1e-4                         # the step is visible at the bar
    np.testing.assert_allclose(got, want, atol=2e-4)


# ----------------------------------------------------------------------------------------------------------------------
# 10  look-up path and shards
# ----------------------------------------------------------------------------------------------------------------------
def test_lookup_path_and_shards_equal_the_table_path(device):
    import mslam_hip as _m

    T = synthetic.camera_pose(0)
    X = synthetic.render_pointmap(T, 96, 128).reshape(-1, 3)
    rng = np.random.default_rng(10)
    sel = rng.permutation(len(X))[:3000]
    X = X[sel].astype(np.float32)
    pw, conf, org = synthetic.sim3_act(T, X).astype(np.float32), rng.uniform(0.1, 8.0, 3000), T[:3].astype(np.float32)
    one = _vol(device, 0.03, 0.12, capacity=1 << 18)
    shards = [_vol(device, 0.03, 0.12, capacity=1 << 17, shard_id=r, num_shards=2) for r in range(2)]
    for v in [one] + shards:
        v.integrate(pw, conf, org, return_fused=False)
    q = one._dev((pw + rng.normal(0, 0.01, pw.shape)).astype(np.float32), torch.float32)
    lk = shards[0].lookup7(q) + shards[1].lookup7(q)
    assert torch.equal(lk, one.lookup7(q)) and min(int(s.lookup7(q)[:, :, 0].sum()) for s in shards) > 1000
    n = q.shape[0]
    val = torch.zeros(n, dtype=torch.float64, device=device)
    grad = torch.zeros((n, 3), dtype=torch.float64, device=device)
    st = torch.zeros(n, dtype=torch.uint8, device=device)
    _m.check(_m.lib().mslam_tsdf_query_lookup(_m.ptr(lk), n, 0.03, 1.0e-3, _m.ptr(val), _m.ptr(grad), _m.ptr(st),
                                              _m.stream_ptr()), "tsdf_query_lookup")
    for a, b in zip((val, grad, st), one.query_batch(q)):
        assert torch.equal(a, b)
    assert set(st.cpu().tolist()) == {0, 1, 2}
    # pose step: camera-frame points, the look-up made with the same pose
    cf = one._dev(rng.uniform(0.1, 3.0, n).astype(np.float32), torch.float32)
    pose = T.astype(np.float32)
    pose[:3] += np.array([0.004, -0.003, 0.002], np.float32)
    Xd = one._dev(X, torch.float32)
    p_tab, p_lk = (torch.from_numpy(pose).to(device) for _ in range(2))
    lk = shards[0].lookup7(Xd, pose=p_lk) + shards[1].lookup7(Xd, pose=p_lk)
    tab = _pose_step(one, Xd, cf, pose=p_tab, cam=1, update=1)
    via = _pose_step(one, Xd, cf, pose=p_lk, cam=1, update=1, lookup=lk)
    assert int(tab[2]) > 1000
    for a, b in zip(tab + (p_tab,), via + (p_lk,)):
        assert torch.equal(a, b)
    assert not torch.equal(p_tab.cpu(), torch.from_numpy(pose))
