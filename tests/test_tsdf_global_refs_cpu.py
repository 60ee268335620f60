"""CPU tests (-m "not gpu") of tests/tsdf_global_refs.py: the C oracle (oracle/tsdf_ref.c) is pinned, bit for bit, to the
literal NumPy restatement of the reference on every input the GPU edge tests use, the literal query and pose system are
pinned to the oracle and to the reference's own fixture, and every recipe is shown to reach the branch it is meant for
(sample counts at the replay thresholds, probe wrap-around, num == 1 / 2, the step clamp, the key range)."""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_global_refs as R  # noqa: E402


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "tsdf_global.npz"))


_built = {}


def _case(name):
    """(inputs, literal volume after one call, literal fused count): built once per case."""
    if name not in _built:
        inp = R.CASES[name]()
        p, c, o, vs, tr, mw, ss = inp
        lit = R.LiteralVolume(vs, tr, mw)
        _built[name] = (inp, lit, lit.integrate(p, c, o, ss))
    return _built[name]


@pytest.mark.parametrize("name", list(R.CASES))
def test_oracle_equals_literal_reference(name):
    """Fused count, keys, tsdf and weight: exactly equal on every case (no case needed the fall-back bars)."""
    (p, c, o, vs, tr, mw, ss), lit, fused = _case(name)
    assert len(p) <= 14000
    ref = oracle.TSDFVolume(vs, tr, mw)
    assert ref.integrate(p, c, o, ss) == fused
    k_ref, t_ref, w_ref = ref.voxels()
    k, t, w = lit.dump()
    np.testing.assert_array_equal(k_ref, k)
    np.testing.assert_array_equal(w_ref, w)
    np.testing.assert_array_equal(t_ref, t)
    # the vectorised per-ray form counts what the literal loop applied
    counts, nums = R.sample_counts(p, c, o, vs, tr, mw, ss)
    assert counts == lit.counts and nums == lit.nums


def test_second_pass_on_averaged_voxels():
    """replay_thresholds is integrated twice on the GPU: the oracle stays exact on top of existing values."""
    (p, c, o, vs, tr, mw, ss), _, _ = _case("replay_thresholds")
    lit, ref = R.LiteralVolume(vs, tr, mw), oracle.TSDFVolume(vs, tr, mw)
    p, c = p[::7], c[::7]           # the same voxels with fewer repeats: the second pass is what is new here
    for _ in range(2):
        assert ref.integrate(p, c, o, ss) == lit.integrate(p, c, o, ss)
    for a, b in zip(ref.voxels(), lit.dump()):
        np.testing.assert_array_equal(a, b)
    assert (lit.dump()[2] == mw).any()


# ----------------------------------------------------------------------------------------------------------------------
# the conditions that keep the GPU tests honest
# ----------------------------------------------------------------------------------------------------------------------
def test_replay_case_hits_every_threshold():
    _, lit, _ = _case("replay_thresholds")
    have = set(lit.counts.values())
    assert have == {47, 48, 49, 2048, 2049}, sorted(have)       # one sample per voxel and ray: nothing longer than 2049
    assert (lit.dump()[2] == 5.0).any()         # the clamp is reached


def _order_effect(name):
    """Largest relative change of a voxel value when the same points are fused in reverse order."""
    (p, c, o, vs, tr, mw, ss), _, _ = _case(name)
    fwd, rev = oracle.TSDFVolume(vs, tr, mw), oracle.TSDFVolume(vs, tr, mw)
    fwd.integrate(p, c, o, ss)
    rev.integrate(p[::-1], c[::-1], o, ss)
    np.testing.assert_array_equal(fwd.voxels()[0], rev.voxels()[0])
    return float(np.abs(fwd.voxels()[1] / rev.voxels()[1] - 1.0).max())


def test_replay_order_is_visible_in_the_floor_case():
    """With ordinary weights tsdf * weight is the running sum of value * w whatever the order (only the rounding moves,
    5e-15 here against a bar of 1e-11), so replay_thresholds checks the thresholds' bookkeeping - every sample applied
    once - and replay_floor checks the order: under the 1e-9 floor of the divisor the last samples decide."""
    _, lit, _ = _case("replay_floor")
    assert set(lit.counts.values()) == {47, 48, 49, 2048, 2049}
    assert 0.0 < lit.dump()[2].max() < 0.5e-9                    # two calls stay under the floor
    assert _order_effect("replay_floor") > 1e-2
    assert _order_effect("replay_thresholds") < 1e-12


def test_many_big_case_has_more_big_voxels_than_blocks():
    _, lit, _ = _case("many_big")
    assert sum(1 for n in lit.counts.values() if n > 48) > 2048
    assert max(lit.counts.values()) <= 2048 * 49      # nothing absurd


def test_wrap_case_wraps():
    (p, c, o, vs, tr, mw, ss), lit, _ = _case("wrap_table")
    cap = R.WRAP_CAPACITY
    homes = [R.home_slot(k, cap) for k in lit.voxels]
    assert len(homes) < cap // 2
    assert cap - 1 in homes and 0 in homes
    assert sum(1 for h in homes if h >= cap - 4) > 4


def test_band_cases_reach_their_branches():
    (p, c, o, vs, tr, mw, ss), lit, fused = _case("band_coarse")
    assert 1 in lit.nums and 2 in lit.nums
    assert 0 < fused < len(p)                                   # some rays are below the 1e-4 gate
    (p, c, o, vs, tr, mw, ss), lit, fused = _case("band_clamped")
    assert max(vs * ss, 1.0e-4) == 1.0e-4                       # the step clamp
    assert int(2.0 * tr / 1.0e-4) + 4 < 1000                    # max_band stays in the hundreds
    assert (np.linalg.norm(p - o, axis=1) < tr).all()           # camera inside the band on every ray
    assert max(lit.nums) < 400 and fused < len(p)
    (p, c, o, vs, tr, mw, ss), lit, fused = _case("band_thin")
    assert tr < vs
    for name in ("band_origin0", "band_negative", "band_corner"):
        (p, c, o, vs, tr, mw, ss), lit, fused = _case(name)
        L = np.linalg.norm(p.astype(np.float64) - o, axis=1)
        assert (L < 1.0e-4).any() and (L < tr).any() and (L > 20.0).any()
        assert 0 < len(p) - fused == int((np.linalg.norm(p - o, axis=1) < np.float32(1.0e-4)).sum())
    # band_corner: the origin is on a voxel corner in float32 arithmetic, and the samples of its axis rays lie on voxel
    # faces (their two off-axis coordinates are the origin's, whose quotients by the voxel size are whole numbers)
    (p, c, o, vs, tr, mw, ss), lit, fused = _case("band_corner")
    q = o / np.float32(vs)
    assert (q == np.round(q)).all() and (q != 0).all()
    on_faces = 0
    for point, axis in zip(p[:6], R.AXES):
        assert ((point - o != 0) == (axis != 0)).all()              # an axis ray in float32 too
        rs = R.ray_samples(point, o, vs, tr, ss)
        if rs is not None and len(rs[1]):
            off = axis == 0
            assert (rs[1][:, off] == q[off].astype(np.int64)).all()
            on_faces += len(rs[1])
    assert on_faces > 20


def test_key_range_cases():
    assert R.pack_key(-R.KEY_BIAS, 0, R.KEY_BIAS - 1) is not None
    assert R.pack_key(R.KEY_BIAS, 0, 0) is None and R.pack_key(0, -R.KEY_BIAS - 1, 0) is None
    _, lit, _ = _case("key_edges")
    keys = lit.dump()[0]
    assert keys[:, 0].max() == R.KEY_BIAS - 1 and R.in_key_range(keys).all()
    _, lit, _ = _case("key_edges_low")
    keys = lit.dump()[0]
    assert keys[:, 0].min() == -R.KEY_BIAS and R.in_key_range(keys).all()
    p, c, o, vs, tr, mw, ss = R.key_overflow_code1()
    counts, _ = R.sample_counts(p, c, o, vs, tr, mw, ss)
    xs = {k[0] for k in counts}
    assert max(xs) == R.KEY_BIAS and R.KEY_BIAS - 1 in xs       # dropped samples and kept ones on the same ray
    (p, c, o, vs, tr, mw, ss), at = R.long_ray_code3()
    L = np.linalg.norm(p[at] - o)
    assert (L + np.float32(tr)) / np.float32(vs * ss) >= 2.0 ** 20


def test_host_hash_equals_the_package_copy():
    from mast3r_slam.tsdf.global_volume import voxel_shard

    rng = np.random.default_rng(0)
    keys = rng.integers(-R.KEY_BIAS, R.KEY_BIAS, (500, 3))
    mine = [(R.mix64(R.pack_key(*k)) >> 40) % 3 for k in keys.tolist()]
    np.testing.assert_array_equal(voxel_shard(keys, 3), mine)


def test_conf_case_without_nan_confidences_has_no_nan():
    """What the device computes: NaN-confidence points count as fused but apply nothing."""
    p, c, o, vs, tr, mw, ss = R.CASES["conf_edges"]()
    keep = ~np.isnan(c)
    ref = oracle.TSDFVolume(vs, tr, mw)
    ref.integrate(p[keep], c[keep], o, ss)
    k, t, w = ref.voxels()
    assert len(k) > 100 and not np.isnan(w).any() and np.isinf(w).any()
    _, lit, fused = _case("conf_edges")
    assert np.isnan(lit.dump()[2]).any()                        # the reference lets them through
    assert fused == int(np.isfinite(p).all(axis=1).sum())
    assert _case("nan_origin")[2] == 0 and not _case("nan_origin")[1].voxels


# ----------------------------------------------------------------------------------------------------------------------
# query and pose system
# ----------------------------------------------------------------------------------------------------------------------
def _sparse(seed=11):
    p, c, o, vs, tr, mw = R.sparse_rays(seed)
    lit, ref = R.LiteralVolume(vs, tr, mw), oracle.TSDFVolume(vs, tr, mw)
    n = len(p) // 2
    for sl, ss in ((slice(0, n), 1.0), (slice(n, None), 0.5)):
        assert lit.integrate(p[sl], c[sl], o, ss) == ref.integrate(p[sl], c[sl], o, ss)
    return lit, ref, vs


def test_literal_query_equals_oracle_and_reaches_every_gate():
    lit, ref, vs = _sparse()
    keys, t, w = lit.dump()
    for a, b in zip(ref.voxels(), (keys, t, w)):
        np.testing.assert_array_equal(a, b)
    q = R.centres(keys, vs)
    val, grad, st = lit.query_batch(q)
    v_ref, g_ref, s_ref = ref.query(q)
    np.testing.assert_array_equal(st, s_ref)
    np.testing.assert_array_equal(val, v_ref)
    np.testing.assert_allclose(grad, g_ref, rtol=1e-15, atol=0)
    once = np.array([isinstance(lit.voxels[tuple(k)][0], np.float32) for k in keys.tolist()])
    cls = R.classify_queries(keys, w, once, lit.min_weight, keys)
    assert {c[0] for c in cls} == {0, 1, 2, 3}
    kinds = set().union(*(c[1] for c in cls))
    assert kinds == {"ff", "fa", "aa"}
    assert set(np.unique(st)) == {1, 2}
    # the float32 path matters: the float64 difference of two first-touch values is another number
    i = next(i for i, c in enumerate(cls) if c == (1, frozenset({"ff"})))
    a = next(a for a in range(3) if grad[i, a] != 0.0)
    hi, lo = keys[i].copy(), keys[i].copy()
    hi[a] += 1; lo[a] -= 1
    d32 = (lit.voxels[tuple(hi)][0] - lit.voxels[tuple(lo)][0]) / (2.0 * vs)
    assert isinstance(d32, np.float32) and np.sign(d32) == grad[i, a]


def test_equal_neighbours_give_status_one():
    calls, (vs, tr, mw, ss) = R.equal_neighbours()
    lit, ref = R.LiteralVolume(vs, tr, mw), oracle.TSDFVolume(vs, tr, mw)
    for p, c, o in calls:
        assert lit.integrate(p, c, o, ss) == ref.integrate(p, c, o, ss) == 1
    keys, t, w = lit.dump()
    assert {tuple(k) for k in keys.tolist()} == {(1, 1, 9), (2, 1, 9), (3, 1, 9)}
    assert t[0] == t[2] and t[0] != 0.0
    q = R.centres(keys, vs)
    np.testing.assert_array_equal(lit.query_batch(q)[2], [1, 1, 1])
    np.testing.assert_array_equal(ref.query(q)[2], [1, 1, 1])
    cls = R.classify_queries(keys, w, [False] * 3, lit.min_weight, keys)
    assert [c[0] for c in cls] == [0, 1, 0]


def _fixture_volume(fx):
    """The reference's own volume after both keyframes, as a literal volume: values from the fixture, the float32 state
    from the sample counts of the two calls."""
    total = {}
    for kf in range(2):
        counts, _ = R.sample_counts(fx[f"kf{kf}_points"], fx[f"kf{kf}_conf"], fx[f"kf{kf}_origin"], 0.03, 0.12)
        for k, n in counts.items():
            total[k] = total.get(k, 0) + n
    keys = fx["kf1_keys"]
    assert {tuple(k) for k in keys.tolist()} == set(total)
    once = np.array([total[tuple(k)] == 1 for k in keys.tolist()])
    lit = R.LiteralVolume(0.03, 0.12, 100.0, 1.0e-3)
    lit.load(keys, fx["kf1_tsdf"], fx["kf1_weight"], once)
    assert all(float(np.float32(t)) == t for t in fx["kf1_tsdf"][once])
    return lit


def test_literal_query_and_pose_system_match_reference_fixture(fx):
    lit = _fixture_volume(fx)
    val, grad, st = lit.query_batch(fx["query_points"])
    np.testing.assert_array_equal(st, fx["query_status"])
    np.testing.assert_allclose(val, fx["query_value"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(grad, fx["query_grad"], rtol=1e-9, atol=1e-12)
    H, b, used = R.literal_pose_system(lit, fx["query_points"], fx["pose_conf"], 0.15)
    assert used == int(fx["pose_used"])
    np.testing.assert_allclose(H, fx["pose_H"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(b, fx["pose_b"], rtol=1e-10, atol=1e-12)
    ref = oracle.TSDFVolume(0.03, 0.12, 100.0, 1.0e-3)
    for kf in range(2):
        ref.integrate(fx[f"kf{kf}_points"], fx[f"kf{kf}_conf"], fx[f"kf{kf}_origin"])
    H2, b2, used2 = ref.pose_system(fx["query_points"], fx["pose_conf"], 0.15)
    assert used2 == used
    np.testing.assert_allclose(H2, H, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(b2, b, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("where", ["below", "at", "above"])
def test_pose_weight_gate(where):
    """lambda * conf in float32 against 1e-6, every row on the same side: max() keeps the float32 product from the gate
    upwards and takes the float64 constant below it.  At the gate the two differ by 2.5e-9, and the system is large
    enough for that to fail the bars: the oracle must take the branch the literal reference takes."""
    lam = 0.15
    lit, ref, vs = _sparse()
    q = R.centres(lit.dump()[0], vs)
    pts = q[lit.query_batch(q)[2] == 2]
    pts = np.resize(pts, (8000, 3))
    conf = R.gate_confidences(lam, where, len(pts))
    w = np.float32(lam) * conf
    assert {"below": (w < R.GATE).all(), "at": (w == R.GATE).all(), "above": (w > R.GATE).all()}[where]
    H, b, used = R.literal_pose_system(lit, pts, conf, lam)
    H2, b2, used2 = ref.pose_system(pts, conf, lam)
    assert used == used2 == len(pts)
    np.testing.assert_allclose(H2, H, rtol=1e-10, atol=1e-12)       # the bars of tests/test_tsdf_oracle.py
    np.testing.assert_allclose(b2, b, rtol=1e-10, atol=1e-12)
    if where == "at":       # the other branch (the double constant on every row) is another system at these bars
        other = H * (1.0e-6 / float(R.GATE))
        assert not np.allclose(other, H, rtol=1e-9, atol=1e-12)
