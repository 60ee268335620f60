"""The recipes and references of tests/matching_refs.py on their own (no GPU): every recipe reaches the branch it is
named for, every closed-form or float64 expectation agrees with the oracle, and every trap separates the right answer
from the named wrong one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matching_refs as M  # noqa: E402
import oracle  # noqa: E402
from oracle import matching_py  # noqa: E402


# ---- xcd_remap -------------------------------------------------------------------------------------------------------
def test_xcd_remap_is_a_bijection():
    """common.h: "bijective for any grid size" - here for every grid up to 300 blocks, the grids of the n cases among them."""
    grids = set(range(1, 301)) | {(n + 255) // 256 for n in M.N_GRID}
    assert {g % 8 for g in ((n + 255) // 256 for n in M.N_GRID)} >= {0, 1, 7}
    for nblk in grids:
        assert sorted(M.xcd_remap(b, nblk) for b in range(nblk)) == list(range(nblk))


# ---- prep ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", M.PREP_SHAPES)
def test_prep_reference_against_oracle(h, w):
    """The float64 statement against the oracle's float32 numpy one.  The oracle rounds each product on its own, one
    rounding per tap more than the kernel's fmaf chain, so it is held to twice the kernel's bound; p_init is exact."""
    for b in M.PREP_B:
        for with_idx in (False, True):
            X11, X21, idx = M.prep_inputs(h, w, b, with_idx)
            rays, pts, p0, rb, pb = M.prep_ref(X11, X21, idx)
            o_rays, o_pts, o_p0 = matching_py.prep_for_iter_proj(X11, X21, idx)
            assert np.isfinite(rays).all() and np.isfinite(o_rays).all()
            assert (np.abs(o_rays - rays) <= 2 * rb).all() and (np.abs(o_pts - pts) <= 2 * pb).all()
            np.testing.assert_array_equal(o_p0, p0)
            assert p0.max() < 2 ** 24
            k_rays, k_pts, k_p0 = M.prep_kernel_model(X11, X21, idx)
            assert (np.abs(k_rays - rays) <= rb).all() and (np.abs(k_pts - pts) <= pb).all()
            np.testing.assert_array_equal(k_p0, p0)
            if with_idx:
                assert idx.min() == 0 and idx.max() == h * w - 1 and idx[0, :4].tolist() == [0, w - 1, w, h * w - 1]


def test_prep_planted_pixels():
    X11, X21, _ = M.prep_inputs(17, 33, 3, False)
    rays, pts, _, rb, _ = M.prep_ref(X11, X21, None)
    n = 17 * 33
    for bi in range(3):
        f = rays.reshape(3, n, 9)
        assert (f[bi, (3 + bi) % n, :3] == 0).all() and (pts[bi, bi % n] == 0).all()              # zero vector -> 0
        np.testing.assert_allclose(pts[bi, (5 + bi) % n], [6e-2, 0, 8e-2], rtol=1e-6)               # x / 1e-12
        np.testing.assert_allclose(np.linalg.norm(pts[bi, (10 + bi) % n]), 1, rtol=1e-12)           # small, normalised
        np.testing.assert_allclose(np.linalg.norm(pts[bi, (15 + bi) % n]), 1, rtol=1e-12)           # large
    sq = X21.astype(np.float32) ** 2
    assert np.isfinite(sq).all() and (sq[sq > 0] > 1e-30).all()      # squares neither overflow nor go subnormal
    # reflect on two rows: -1 -> 1 and 2 -> 0
    X11, X21, _ = M.prep_inputs(2, 2, 1, False)
    r = M._normalize64(X11)[0]
    rays = M.prep_ref(X11, X21, None)[0][0]
    gy00 = (-3 * r[1, 1] - 10 * r[1, 0] - 3 * r[1, 1] + 3 * r[1, 1] + 10 * r[1, 0] + 3 * r[1, 1]) / 32
    gx00 = (-3 * r[1, 1] + 3 * r[1, 1] - 10 * r[0, 1] + 10 * r[0, 1] - 3 * r[1, 1] + 3 * r[1, 1]) / 32
    np.testing.assert_allclose(rays[0, 0, 6:], gy00, atol=1e-15)
    np.testing.assert_allclose(rays[0, 0, 3:6], gx00, atol=1e-15)


# ---- iter_proj -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noisy():
    return M.noisy_case()


def test_noisy_recipe_reaches_every_transition(noisy):
    rays, pts, p0 = noisy
    acc = M.accept_trace(rays, pts, p0, 10)
    sh = M.transition_shares(acc)
    print("transition shares", sh)
    assert min(sh.values()) >= 0.01, sh
    _, conv = oracle.iter_proj(rays, pts, p0, 10, M.LAMBDA, M.THRESH)
    assert 0.05 < conv.mean() < 0.95
    # zero iterations: the closed form of the clamp
    p, c = oracle.iter_proj(rays, pts, p0, 0, M.LAMBDA, M.THRESH)
    np.testing.assert_array_equal(p, M.clamp_p(p0, *M.NOISY_HW))
    assert not c.any()


def test_sixty_iterations_take_lambda_to_zero(noisy):
    """lambda = 1e-8 * 10^(rejects - accepts): below 2^-126 from 31 net accepts on, 0 from 38 on."""
    rays, pts, p0 = noisy
    acc = M.accept_trace(rays, pts, p0, 60)
    net = np.cumsum(np.where(acc, 1, -1), -1).max(-1)
    print("points with lambda subnormal / zero", (net >= 31).sum(), (net >= 38).sum())
    assert (net >= 38).any()


def test_nonfinite_recipe_reaches_its_cells(noisy):
    rays, pts, p0 = M.nonfinite_case()
    h, w = M.NOISY_HW
    p, c = oracle.iter_proj(rays, pts, p0, 10, M.LAMBDA, M.THRESH)
    q, _ = oracle.iter_proj(*noisy, 10, M.LAMBDA, M.THRESH)
    assert np.isfinite(p).all()
    zx, zy = M.ZERO_PIX
    # the point that starts on the zero ray: norm 0, rinv inf, cost NaN, nothing is ever accepted
    k = zy * w + zx
    assert (p[:, k] == (zx, zy)).all() and not c[:, k].any()
    # other points are moved by the zero ray: a trial of theirs landed in one of its four cells
    moved = (p != q).any(-1)
    moved[:, [k, 3, 40]] = False
    near = (np.abs(q[..., 0] - zx) < 1) & (np.abs(q[..., 1] - zy) < 1)
    assert (moved & near).any()
    # points pinned to u == umax beside the NaN pixel sample it with weight exactly 0: NaN cost, they stay, unconverged
    for row in (M.NAN_ROW - 1, M.NAN_ROW):
        for col in (w - 2, w - 1):
            kk = row * w + col
            assert (p[:, kk] == (w - 2, row)).all() and not c[:, kk].any()
    assert (p[:, [3, 40]] != q[:, [3, 40]]).any()       # zero targets take another path


def test_singular_recipe_closed_form():
    rays, pts, p0, iters, lam = M.singular_case()
    p, c = oracle.iter_proj(rays, pts, p0, iters, lam, M.THRESH)
    assert (p == 1).all() and c.all()
    assert (rays[..., 3:] == 0).all() and len(np.unique(p0.reshape(-1, 2), axis=0)) == 42


def test_pinit_recipe_closed_form():
    rays, pts, p0, clamped = M.pinit_case()
    h, w = rays.shape[1:3]
    p, c = oracle.iter_proj(rays, pts, p0, 0, M.LAMBDA, M.THRESH)
    np.testing.assert_array_equal(p, clamped)
    np.testing.assert_array_equal(M.clamp_p(p0, h, w), clamped)
    assert np.isnan(p0).any() and np.isinf(p0).any() and (p0 == 1).any() and (p0[..., 0] == w - 2).any()
    p, _ = oracle.iter_proj(rays, pts, p0, 10, M.LAMBDA, M.THRESH)
    assert np.isfinite(p).all() and (p != clamped).any()


def test_small_images_pin_the_sample():
    rays, pts, p0 = M.iter_case(3, 3, 3, 50)
    p, _ = oracle.iter_proj(rays, pts, p0, 10, M.LAMBDA, M.THRESH)
    assert (p == 1).all()
    for h, w in M.SMALL_SHAPES[1:]:
        rays, pts, p0 = M.iter_case(h, w, 3, 200)
        p, _ = oracle.iter_proj(rays, pts, p0, 10, M.LAMBDA, M.THRESH)
        assert (p >= 1).all() and (p[..., 0] <= w - 2).all() and (p[..., 1] <= h - 2).all()
        assert len(np.unique(p[..., 0])) > 1 or w == 3


def test_pinhole_ground_truth():
    """Measured on the oracle: the figure quoted in matching_refs.PINHOLE_MEASURED."""
    rays, pts, p0, drawn = M.pinhole_case()
    p, c = oracle.iter_proj(rays, pts, p0, 10, 1e-8, 1e-6)
    err = np.hypot(*(p.astype(np.float64) - drawn).transpose(2, 0, 1)).max()
    print(f"pinhole: max distance to the drawn position {err:.3e} px, converged {c.mean():.3f}")
    assert c.all()
    assert err <= M.PINHOLE_BOUND
    assert err >= M.PINHOLE_MEASURED / 1.1          # the quoted measurement is the measurement


def test_warped_ground_truth_separates_stale_gradients():
    """Measured on the oracle (matching_refs.WARPED_MEASURED); the float64 iteration meets the bound too, and the one
    that keeps the first sample's gradient misses it by far - which the pinhole recipe, with its almost constant
    gradient, cannot show."""
    rays, pts, p0, drawn = M.warped_case()
    p, c = oracle.iter_proj(rays, pts, p0, 10, 1e-8, 1e-6)
    dist = lambda q: np.hypot(q[..., 0] - drawn[0, :, 0], q[..., 1] - drawn[0, :, 1]).max()
    err = dist(p[0].astype(np.float64))
    good, stale = dist(M.lm64(rays, pts, p0, 10, 1e-8)), dist(M.lm64(rays, pts, p0, 10, 1e-8, stale=True))
    print(f"warped: oracle {err:.3e} px, float64 iteration {good:.3e} px, stale gradient {stale:.3e} px, converged {c.mean():.3f}")
    assert c.all()
    assert M.WARPED_MEASURED / 1.1 <= err <= M.WARPED_BOUND
    assert good <= M.WARPED_BOUND and stale > 3 * M.WARPED_BOUND


def test_descent_in_float64(noisy):
    rays, pts, p0 = noisy
    h, w = M.NOISY_HW
    for iters in (1, 2, 10, 60):
        p, _ = oracle.iter_proj(rays, pts, p0, iters, M.LAMBDA, M.THRESH)
        c1, n1 = M.cost64(rays, pts, p)
        c0, n0 = M.cost64(rays, pts, M.clamp_p(p0, h, w))
        assert min(n0.min(), n1.min()) > 0.9 and np.abs(rays[..., :3]).max() <= 1 + 1e-6
        slack = M.cost_eval_bound(c0, n0) + M.cost_eval_bound(c1, n1)
        assert (c1 <= c0 + slack).all(), float((c1 - c0 - slack).max())
        assert (c1 < c0).mean() > 0.5 and slack.max() < 1e-4 * c0.max()


# ---- occlusion -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", M.OCC_SHAPES)
def test_occlusion_expectation_against_oracle(h, w):
    d = M.occlusion_case(h, w)
    p1, v = matching_py.occlusion_and_trunc(d["X11"], d["X21"], d["p"], d["valid_in"].astype(bool), M.OCC_THRESH)
    np.testing.assert_array_equal(p1, d["p1"])
    np.testing.assert_array_equal(v, d["valid"])
    pl = d["planted"]
    assert d["valid"][pl].sum() == 9 and (~d["valid"][pl]).sum() == 9                # 3 of 6 per batch item each way
    assert 0.2 < d["valid"].mean() < 0.5 and 0.25 < (d["valid_in"] == 0).mean() < 0.4
    fr = d["p"] - np.trunc(d["p"])
    assert (fr == 0).any() and (fr > 0.99).any()
    # a swapped u / v would look up another pixel (or none)
    assert (d["p1"][..., 0] > h).any()
    # `<=` would turn exactly the three d == thresh plants per batch item
    dd = d["X11"][np.arange(3)[:, None], p1[..., 1], p1[..., 0]] - d["X21"].reshape(3, -1, 3)
    dist = np.sqrt((dd.astype(np.float32) ** 2).sum(-1, dtype=np.float32))
    assert ((dist == np.float32(M.OCC_THRESH)) & pl).sum() == 9


# ---- refine_matches --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fdim", M.TRAP_FDIMS)
def test_refine_traps(fdim):
    for t in M.refine_traps(fdim):
        args = (t["D11"], t["D21"], t["p1"], t["radius"], t["dil"])
        np.testing.assert_array_equal(oracle.refine_matches(*args), t["expect"], err_msg=t["name"])
        np.testing.assert_array_equal(M.refine_model(*args)[0], t["expect"], err_msg=t["name"])
        for kw, wrong in t["wrong"]:
            assert tuple(wrong) != tuple(t["expect"][0, 0])
            np.testing.assert_array_equal(M.refine_model(*args, **kw)[0][0, 0], wrong, err_msg=f"{t['name']} {kw}")
        if t["fused"] is not None:
            np.testing.assert_array_equal(oracle.refine_matches(*args, fused_fma=True)[0, 0], t["fused"])
    names = {t["name"]: t for t in M.refine_traps(fdim)}
    sub = names["subnormal"]
    prod = (sub["D21"][0, 0, 0] * sub["D11"][0, 2, 3, 0])
    assert prod.dtype == np.float16 and 0 < float(prod) < M.HALF_MIN
    assert float(names["inf_first"]["D11"][0, 2, 1, 0]) * 2 > 65520          # rounds to +inf in half


@pytest.mark.parametrize("fdim", M.REFINE_FDIMS)
def test_refine_model_is_the_oracle_and_ties_occur(fdim):
    for kind in M.REFINE_KINDS:
        D11, D21, p1 = M.refine_random(fdim, 257, kind)
        for radius, dil in M.REFINE_RD:
            ref = oracle.refine_matches(D11, D21, p1, radius, dil)
            got, tied = M.refine_model(D11, D21, p1, radius, dil)
            np.testing.assert_array_equal(got, ref)
            if fdim == 0 or dil == 0:
                np.testing.assert_array_equal(ref, p1)
            if kind == "tie" and fdim >= 7 and radius * dil >= 1:
                assert tied.mean() > 0.01, (fdim, radius, dil, tied.mean())
                assert (M.refine_model(D11, D21, p1, radius, dil, ge=True)[0] != ref).any()
            if kind == "normal" and fdim >= 7 and radius * dil >= 1:
                assert (ref != p1).any()


def test_refine_outside_recipe():
    D11, D21, p1 = M.refine_outside()
    ref = oracle.refine_matches(D11, D21, p1, *M.OUTSIDE_RD)
    np.testing.assert_array_equal(M.refine_model(D11, D21, p1, *M.OUTSIDE_RD)[0], ref)
    assert ref[0, 4].tolist() == [-40, -40]
    h, w = M.REFINE_HW
    moved = ref[0, :4]
    assert (moved != p1[0, :4]).any(-1).all()            # the partly outside windows do find something
    assert (moved[:, 0] >= 0).all() and (moved[:, 0] < w).all() and (moved[:, 1] >= 0).all() and (moved[:, 1] < h).all()
    assert np.abs(p1).max() < 2 ** 20


# ---- the Python layer ------------------------------------------------------------------------------------------------
def test_match_recipe_leaves_out_few_points():
    """Points are compared where the oracle chain gives the same index and flag on the oracle's prep and on the kernel's
    (here: its float32 model); the two preps differ by rounding only, which flips an integer step at a few points."""
    from mast3r_slam.config import config

    d = M.match_case()
    cfg = config["matching"]
    i1, v1 = M.oracle_chain(d, matching_py.prep_for_iter_proj(d["X11"], d["X21"], d["idx"]), cfg)
    i2, v2 = M.oracle_chain(d, M.prep_kernel_model(d["X11"], d["X21"], d["idx"]), cfg)
    out = (i1 != i2) | (v1 != v2)
    print("left out", out.mean())
    assert out.mean() <= M.MATCH_LEFT_OUT
    assert v1.mean() > 0.2 and (d["idx"] != np.arange(d["idx"].shape[1])).any()
