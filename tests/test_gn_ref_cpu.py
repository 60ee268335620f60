"""CPU tests (-m "not gpu") of tests/gn_ref.py, the float64 reference that tests/test_gn_blocks_gpu.py and
tests/test_gn_loop_gpu.py hold the global Gauss-Newton kernels to: finite differences of the residuals, the float32 oracle
on plain graphs, the properties the GPU tests assume of their input sets, and the float32 baselines."""
import numpy as np
import pytest
import scipy.linalg

import gn_ref as G
import oracle
import tracker_ref as R
from mast3r_slam import synthetic


@pytest.fixture(scope="module")
def case_set():
    return G.cases()


@pytest.fixture(scope="module")
def refs(case_set):
    return {k: G.reference(c) for k, c in case_set.items()}


def oracle_blocks(c):
    g = c["g"]
    ie, je = G.edge_rows(g["ii"], g["jj"])
    return oracle.gn_edges(c["kind"], g["Twc"], g["Xs"], g["Cs"], g["K"], ie, je, g["idx_ii2jj"], g["valid_match"], g["Q"],
                           c["sigma_a"], c["sigma_b"], c["C_thresh"], c["Q_thresh"], height=c["h"], width=max(c["w"], 1),
                           pixel_border=c["pixel_border"], z_eps=c["z_eps"])


def oracle_step(c):
    g = c["g"]
    return oracle.gauss_newton(c["kind"], g["Twc"], g["Xs"], g["Cs"], g["K"], g["ii"], g["jj"], g["idx_ii2jj"], g["valid_match"],
                               g["Q"], c["sigma_a"], c["sigma_b"], c["C_thresh"], c["Q_thresh"], 1, 0.0, height=c["h"],
                               width=max(c["w"], 1), pixel_border=c["pixel_border"], z_eps=c["z_eps"])


# ---- finite differences ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", G.KINDS)
def test_jacobians_are_finite_differences_of_the_residuals(kind):
    """d e / d xi_i and d e / d xi_j of point_rows() against central differences of its float64 residuals under
    exp(eps e_k) Ti and exp(eps e_k) Tj, eps = 1e-6: truncation ~ eps^2 |e'''| / 6, rounding ~ 1e-16 |e| / eps; asserted at
    1e-7 of the largest entry of each Jacobian row's column (observed <= 3.1e-9)."""
    h, w = 12, 16
    g = synthetic.make_graph(n_kf=3, h=h, w=w, seed=2, pose_noise=0.05)
    Xi, Xj, ind = g["Xs"][2][g["idx_ii2jj"][0]], g["Xs"][1], g["idx_ii2jj"][0]
    Mi, Mj = R.sim3_matrix(g["Twc"][2]), R.sim3_matrix(g["Twc"][1])      # neither is the identity
    assert np.abs(Mi[:3, 3]).min() > 0.01
    kw = dict(ind=ind, K=g["K"], width=w, z_eps=1e-6)
    e, J, P = G.point_rows(kind, Mi, Mj, Xi, Xj, **kw)
    assert e.shape == (h * w, G.ROWS[kind]) and J.shape == (h * w, G.ROWS[kind], 14)
    eps = 1e-6
    fd = np.zeros_like(J)
    for k in range(14):
        d = [scipy.linalg.expm(R.sim3_generator(s * eps * np.eye(7)[k % 7])) for s in (1, -1)]
        ep, em = (G.point_rows(kind, D @ Mi if k < 7 else Mi, Mj if k < 7 else D @ Mj, Xi, Xj, **kw)[0] for D in d)
        fd[:, :, k] = (ep - em) / (2 * eps)
    err = np.abs(J - fd).max(0) / np.abs(J).max(0).clip(1e-300)
    print(f"fd {kind}: {err.max():.2e}")
    assert err.max() < 1e-7
    assert np.abs(J[:, :, :7] + J[:, :, 7:]).max() == 0


# ---- the float32 oracle on plain graphs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", G.KINDS)
def test_blocks_match_the_oracle(kind):
    """edges() against oracle.gn_edges on a plain make_graph input (production sigmas, pose-dependent gates off): every
    block and gradient to rel-L2 1e-5, the bar the float32 oracle and the kernels are held to against each other."""
    h, w = 24, 32
    g = synthetic.make_graph(n_kf=4, h=h, w=w, seed=3)
    c = G._case("plain", kind, g, G.SIGMAS[kind])
    ref = G.reference(c)
    Hr, gr = G.blocks(ref["H"], ref["g"])
    Ho, go = oracle_blocks(c)
    rel = lambda a, b: np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())
    worst = max(max(rel(Ho[b, e], Hr[b, e]) for b in range(4) for e in range(c["E"])),
                max(rel(go[b, e], gr[b, e]) for b in range(2) for e in range(c["E"])))
    print(f"oracle {kind}: rel-L2 {worst:.2e}")
    assert worst <= 1e-5
    np.testing.assert_allclose(ref["Hfam"].sum(0), ref["H"], rtol=0, atol=0)
    assert (np.abs(ref["H"]) <= ref["Habs"] * (1 + 1e-12) + 1e-300).all()


def test_solve_matches_the_oracle():
    """dense() + solve() against oracle.gn_solve on IDENTICAL float32 blocks (the oracle's), 6 keyframes."""
    g = synthetic.make_graph(n_kf=6, h=24, w=32, seed=7)
    c = G._case("plain", "rays", g, G.SIGMAS["rays"])
    Ho, go = oracle_blocks(c)
    ie, je = G.edge_rows(g["ii"], g["jj"])
    dx_o, failed = oracle.gn_solve(Ho, go, ie - 1, je - 1, 5)
    assert not failed
    H14 = np.block([[Ho[0].astype(np.float64), Ho[1]], [Ho[2], Ho[3]]])
    g14 = np.concatenate([go[0], go[1]], -1).astype(np.float64)
    sys = G.dense(dict(H=H14, g=g14, Habs=np.abs(H14), gabs=np.abs(g14)), ie, je, 5)
    dx = G.solve(sys)
    assert np.abs(dx - dx_o).max() <= 1e-6 * max(1.0, np.abs(dx).max())
    assert G.backward_error(sys, dx) < 1e-12


# ---- what the GPU tests assume of their inputs -------------------------------------------------------------------------
def test_populations(case_set, refs):
    """Outlier fractions, trace shares, gate shares and per-chunk survivor counts of the input sets."""
    for name, c in case_set.items():
        ref, kind = refs[name], c["kind"]
        g = c["g"]
        assert g["idx_ii2jj"].min() >= 0 and g["idx_ii2jj"].max() < c["HW"], name
        if not c["step"]:
            continue
        weak = "-weak-" in name
        if weak:
            assert G.weak_trace_share(ref).min() >= 0.90, (name, G.weak_trace_share(ref).min())
            assert 0.2 <= G.outlier_fraction(ref, kind, 1) <= 0.8, (name, G.outlier_fraction(ref, kind, 1))
        else:
            assert 0.2 <= G.outlier_fraction(ref, kind, 0) <= 0.8, (name, G.outlier_fraction(ref, kind, 0))
            if kind != "points":      # the gap the weak sets exist for
                assert G.weak_trace_share(ref).max() <= 1e-4, name
    # gates
    for name in ("gates", "gates-thresholds"):
        c, ref = case_set[name], refs[name]
        assert c["pixel_border"] == 2 and c["z_eps"] == 0.05
        cm = ref["compact"]
        zi, zj, ib = ref["valid_zi"][cm], ref["valid_zj"][cm], ref["in_border"][cm]
        assert (~zi).mean() >= 0.05 and (~zj).mean() >= 0.05 and (~ib).mean() >= 0.05, name
        assert (zi & zj & ib).mean() >= 0.30, name
        g = c["g"]
        ie, je = G.edge_rows(g["ii"], g["jj"])
        K = g["K"].astype(np.float64)
        behind = 0
        for e in range(c["E"]):
            k = np.flatnonzero(cm[e])
            _, _, P = G.point_rows("points", g["Twc"][ie[e]], g["Twc"][je[e]], g["Xs"][ie[e]][ref["ind"][e][k]], g["Xs"][je[e]][k])
            u, v = K[0, 0] * P[:, 0] / P[:, 2] + K[0, 2], K[1, 1] * P[:, 1] / P[:, 2] + K[1, 2]
            for x, hi in ((u, c["w"] - 1 - 2), (v, c["h"] - 1 - 2)):
                assert np.minimum(np.abs(x - 2), np.abs(x - hi)).min() >= G.BORDER_MARGIN
            assert np.abs(P[:, 2] - c["z_eps"]).min() >= G.Z_MARGIN
            zi_e = g["Xs"][ie[e]][ref["ind"][e][k]][:, 2].astype(np.float64)
            assert np.abs(zi_e - c["z_eps"]).min() >= G.Z_MARGIN
            assert (zi_e <= c["z_eps"]).any()
            behind += (P[:, 2] < 0).sum()
        assert behind >= 0.05 * cm.sum()
    assert (refs["gates-thresholds"]["compact"].sum() < 0.5 * refs["gates"]["compact"].sum())
    # chunks
    for name, c in case_set.items():
        if not c.get("chunks"):
            continue
        ref = refs[name]
        S, L = c["split"]
        counts = G.chunk_counts(ref["compact"], c["E"], c["HW"])
        assert counts.shape == (c["E"], S)
        if name.endswith("prescribed"):
            want = list(G.S18_SURVIVORS) + [L] * 7 + [4097, 0]
            assert (counts == np.array(want)[None]).all(), (name, counts)
        elif S == 18:
            assert (counts[:, 17] == 0).all() and (counts[:, :17] > 0).all()
        elif c["HW"] > 5:
            assert (counts > 0).all(), (name, counts)
        else:
            assert counts.sum() > 0, name
    assert (G.chunk_counts(refs["chunks-rays-1"]["compact"], 2, 1)[:, 0] == (1, 0)).all()      # an edge without a survivor
    n = G.chunk_counts(refs[f"chunks-rays-{G.CHUNK_S3}"]["compact"], 2, G.CHUNK_S3)
    assert (n % 4 != 0).any()                      # a tail behind the 4-per-lane groups


# ---- float32 baselines ------------------------------------------------------------------------------------------------
def pose_errors(T1, T0, dx):
    """Per unpinned pose: |log(T1 T0^-1) - dx| and roundtrip_tol(dx)."""
    return [(np.linalg.norm(R.sim3_log(T1[k + 1], T0[k + 1]) - dx[k].astype(np.float64)), R.roundtrip_tol(dx[k]))
            for k in range(len(dx))]


def test_fp32_baselines(case_set, refs):
    """The float32 oracle against the float64 reference, with the measures the GPU tests assert; the maxima are the
    constants in tests/gn_ref.py.  Also: the oracle's float32 retraction of its step returns that step through the float64
    logarithm within tracker_ref.roundtrip_tol, the tolerance the GPU test holds the kernel's poses to."""
    worst = dict(errH=(0.0, ""), errg=(0.0, ""), backward=(0.0, ""))
    for name, c in case_set.items():
        ref = refs[name]
        eH, eg = G.block_errors(ref, *oracle_blocks(c))
        m = dict(errH=eH.max(), errg=eg.max())
        if c["step"]:
            g = c["g"]
            T1, dx, it = oracle_step(c)
            ie, je = G.edge_rows(g["ii"], g["jj"])
            m["backward"] = G.backward_error(G.dense(ref, ie, je, c["P"] - 1), dx)
            for err, tol in pose_errors(T1, g["Twc"], dx):
                assert err <= tol, (name, err, tol)
        print(f"fp32 {name:34s} " + " ".join(f"{k} {v:.2e}" for k, v in m.items()))
        worst = {k: max(worst[k], (m[k], name)) if k in m else worst[k] for k in worst}
    print("fp32 baselines:", {k: (f"{v[0]:.3e}", v[1]) for k, v in worst.items()})
    for k, const in (("errH", G.FP32_ERRH_BASELINE), ("errg", G.FP32_ERRG_BASELINE), ("backward", G.FP32_BACKWARD_BASELINE)):
        assert 0.5 * const < worst[k][0] < 1.5 * const, (k, worst[k], const)
