"""GPU parity tests (-m gpu) for the Gauss-Newton backend and the Sim3 op set, through the C ABI.

Bars (SURVEY §8 tolerance table):
  Hs / gs per edge   rel-L2 <= 1e-5 vs the oracle (reduction order and the M B M^T regrouping differ)
  dx, updated Twc    abs <= 1e-5 after ONE iteration (fp64 solve both sides); <= 2e-4 after the full
                     loop (fp32 rounding of Hs feeds a 10-step nonlinear iteration)
  Sim3 ops           abs <= 2e-6

These bars do not see the weak residual family (distance | log depth: 1e-7 of the blocks at the production sigmas), the
chunked stream away from two shapes, or the loop state: tests/test_gn_blocks_gpu.py and tests/test_gn_loop_gpu.py hold the
same kernels to the float64 reference of tests/gn_ref.py there.
"""
import numpy as np
import pytest
import torch

import oracle
from mast3r_slam import synthetic

pytestmark = pytest.mark.gpu

PARAMS = {"rays": (0.003, 10.0), "calib": (1.0, 10.0), "points": (0.05, 0.0)}


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30)


def _graph(device, **kw):
    g = synthetic.make_graph(**kw)
    d = {k: _t(v, device) for k, v in g.items() if isinstance(v, np.ndarray)}
    return g, d


@pytest.mark.parametrize("kind", ["rays", "calib", "points"])
@pytest.mark.parametrize("shape", [(24, 32, 4), (96, 128, 6)])
def test_edge_blocks_match_oracle(device, kind, shape):
    import mast3r_slam_backends as be

    h, w, n_kf = shape
    g, d = _graph(device, n_kf=n_kf, h=h, w=w, seed=3)
    sa, sb = PARAMS[kind]
    uniq, ie, je, io, jo = oracle.edge_rows(g["ii"], g["jj"])
    Hs_ref, gs_ref = oracle.gn_edges(kind, g["Twc"], g["Xs"], g["Cs"], g["K"], ie, je, g["idx_ii2jj"],
                                     g["valid_match"], g["Q"], sa, sb, 0.0, 1.5, height=h, width=w,
                                     pixel_border=-10, z_eps=1e-6)
    Hs, gs = be.gn_blocks(kind, d["Twc"], d["Xs"], d["Cs"], d["K"], d["ii"], d["jj"], d["idx_ii2jj"],
                          d["valid_match"], d["Q"], sa, sb, 0.0, 1.5, height=h, width=w, pixel_border=-10, z_eps=1e-6)
    Hs, gs = Hs.cpu().numpy(), gs.cpu().numpy()
    assert Hs.shape == Hs_ref.shape and gs.shape == gs_ref.shape
    for e in range(Hs.shape[1]):
        for blk in range(4):
            assert _rel(Hs[blk, e], Hs_ref[blk, e]) <= 1e-5, (kind, e, blk, _rel(Hs[blk, e], Hs_ref[blk, e]))
        for blk in range(2):
            assert _rel(gs[blk, e], gs_ref[blk, e]) <= 1e-5


def test_edge_range_split_equals_whole(device):
    """Multi-GPU contract: accumulating edge ranges separately into zero-initialised buffers and
    summing them is bit-identical to one pass over all edges."""
    import mast3r_slam_backends as be

    g, d = _graph(device, n_kf=5, h=24, w=32, seed=1)
    args = ("rays", d["Twc"], d["Xs"], d["Cs"], None, d["ii"], d["jj"])
    E = g["ii"].shape[0]
    Hs_all, gs_all = be.gn_blocks(*args, d["idx_ii2jj"], d["valid_match"], d["Q"], 0.003, 10.0, 0.0, 1.5)
    cut = E // 3
    parts = []
    for e0, cnt in ((0, cut), (cut, E - cut)):
        Hs, gs = be.gn_blocks(*args, d["idx_ii2jj"][e0:e0 + cnt].contiguous(),
                              d["valid_match"][e0:e0 + cnt].contiguous(), d["Q"][e0:e0 + cnt].contiguous(),
                              0.003, 10.0, 0.0, 1.5, edge_begin=e0, edge_count=cnt)
        parts.append((Hs, gs))
    assert torch.equal(parts[0][0] + parts[1][0], Hs_all)
    assert torch.equal(parts[0][1] + parts[1][1], gs_all)


@pytest.mark.parametrize("kind", ["rays", "calib", "points"])
def test_one_iteration_dx_and_poses(device, kind):
    import mast3r_slam_backends as be

    h, w = 48, 64
    g, d = _graph(device, n_kf=6, h=h, w=w, seed=7)
    sa, sb = PARAMS[kind]
    T_ref, dx_ref, it = oracle.gauss_newton(kind, g["Twc"], g["Xs"], g["Cs"], g["K"], g["ii"], g["jj"],
                                            g["idx_ii2jj"], g["valid_match"], g["Q"], sa, sb, 0.0, 1.5, 1, 1e-8,
                                            height=h, width=w, pixel_border=-10, z_eps=1e-6)
    Twc = d["Twc"].clone()
    fn = {"rays": lambda: be.gauss_newton_rays(Twc, d["Xs"], d["Cs"], d["ii"], d["jj"], d["idx_ii2jj"],
                                               d["valid_match"], d["Q"], sa, sb, 0.0, 1.5, 1, 1e-8),
          "calib": lambda: be.gauss_newton_calib(Twc, d["Xs"], d["Cs"], d["K"], d["ii"], d["jj"], d["idx_ii2jj"],
                                                 d["valid_match"], d["Q"], h, w, -10, 1e-6, sa, sb, 0.0, 1.5, 1, 1e-8),
          "points": lambda: be.gauss_newton_points(Twc, d["Xs"], d["Cs"], d["ii"], d["jj"], d["idx_ii2jj"],
                                                   d["valid_match"], d["Q"], sa, 0.0, 1.5, 1, 1e-8)}[kind]
    (dx,) = fn()
    assert dx.shape == (5, 7) and dx.dtype == torch.float32
    np.testing.assert_allclose(dx.cpu().numpy(), dx_ref, rtol=0, atol=1e-5)
    np.testing.assert_allclose(Twc.cpu().numpy(), T_ref, rtol=0, atol=1e-5)
    np.testing.assert_array_equal(Twc[0].cpu().numpy(), g["Twc"][0])  # pinned pose untouched


@pytest.mark.parametrize("kind,n_kf", [("rays", 4), ("calib", 12), ("rays", 30)])
def test_full_loop_matches_oracle(device, kind, n_kf):
    """10 iterations with the device-side convergence flag; n_kf=30 exercises several Cholesky
    panels (203 unknowns -> 7 panels of 32)."""
    import mast3r_slam_backends as be

    h, w = 24, 32
    g, d = _graph(device, n_kf=n_kf, h=h, w=w, seed=11, stride=4)
    sa, sb = PARAMS[kind]
    T_ref, dx_ref, it_ref = oracle.gauss_newton(kind, g["Twc"], g["Xs"], g["Cs"], g["K"], g["ii"], g["jj"],
                                                g["idx_ii2jj"], g["valid_match"], g["Q"], sa, sb, 0.0, 1.5, 10,
                                                1e-8, height=h, width=w, pixel_border=-10, z_eps=1e-6)
    Twc = d["Twc"].clone()
    if kind == "rays":
        (dx,) = be.gauss_newton_rays(Twc, d["Xs"], d["Cs"], d["ii"], d["jj"], d["idx_ii2jj"], d["valid_match"],
                                     d["Q"], sa, sb, 0.0, 1.5, 10, 1e-8)
    else:
        (dx,) = be.gauss_newton_calib(Twc, d["Xs"], d["Cs"], d["K"], d["ii"], d["jj"], d["idx_ii2jj"],
                                      d["valid_match"], d["Q"], h, w, -10, 1e-6, sa, sb, 0.0, 1.5, 10, 1e-8)
    np.testing.assert_allclose(Twc.cpu().numpy(), T_ref, rtol=0, atol=2e-4)
    assert np.isfinite(dx.cpu().numpy()).all()


def test_early_termination_flag_and_llt_failure(device):
    import mast3r_slam_backends as be

    g, d = _graph(device, n_kf=4, h=24, w=32, seed=2)
    # huge delta_thresh: the reference breaks after the first iteration -> exactly one retraction
    T1_ref, _, it = oracle.gauss_newton("rays", g["Twc"], g["Xs"], g["Cs"], None, g["ii"], g["jj"], g["idx_ii2jj"],
                                        g["valid_match"], g["Q"], 0.003, 10.0, 0.0, 1.5, 10, 1e9)
    assert it == 1
    Twc = d["Twc"].clone()
    be.gauss_newton_rays(Twc, d["Xs"], d["Cs"], d["ii"], d["jj"], d["idx_ii2jj"], d["valid_match"], d["Q"],
                         0.003, 10.0, 0.0, 1.5, 10, 1e9)
    np.testing.assert_allclose(Twc.cpu().numpy(), T1_ref, atol=1e-5)
    # no valid residual at all -> H = 0 -> LLT fails -> dx = 0, poses unchanged (gn_kernels.cu:147-150)
    Twc = d["Twc"].clone()
    none = torch.zeros_like(d["valid_match"])
    (dx,) = be.gauss_newton_rays(Twc, d["Xs"], d["Cs"], d["ii"], d["jj"], d["idx_ii2jj"], none, d["Q"],
                                 0.003, 10.0, 0.0, 1.5, 10, 1e-8)
    assert not dx.cpu().numpy().any()
    assert torch.equal(Twc, d["Twc"])


def test_gn_error_behaviour(device):
    import mast3r_slam_backends as be

    g, d = _graph(device, n_kf=3, h=12, w=16, seed=2)
    with pytest.raises(RuntimeError, match="Xs must be contiguous"):
        be.gauss_newton_rays(d["Twc"], d["Xs"].transpose(1, 2).contiguous().transpose(1, 2), d["Cs"], d["ii"],
                             d["jj"], d["idx_ii2jj"], d["valid_match"], d["Q"], 0.003, 10.0, 0.0, 1.5, 10, 1e-8)


def test_sim3_ops_match_oracle(device):
    from lietorch_hip import Sim3

    rng = np.random.default_rng(0)
    xi = rng.normal(0, 0.3, (64, 7)).astype(np.float32)
    xi[0] = 0; xi[1, 3:6] = 0; xi[2, 6] = 0; xi[3, 3:] = 0
    T = Sim3.exp(_t(xi, device))
    np.testing.assert_allclose(T.data.cpu().numpy(), oracle.sim3_exp(xi), atol=2e-6)
    Tn = T.data.cpu().numpy()
    xi2 = rng.normal(0, 0.1, (64, 7)).astype(np.float32)
    np.testing.assert_allclose(T.retr(_t(xi2, device)).data.cpu().numpy(), oracle.sim3_retr(xi2, Tn), atol=2e-6)
    # rel = Ti^-1 * Tj
    rel = (T[:32].inv() * T[32:]).data.cpu().numpy()
    np.testing.assert_allclose(rel, oracle.sim3_rel(Tn[:32], Tn[32:]), atol=4e-6)
    X = rng.normal(0, 2, (500, 3)).astype(np.float32)
    Y = T[5:6].act(_t(X, device)).cpu().numpy()
    np.testing.assert_allclose(Y, oracle.sim3_act(Tn[5], X), atol=4e-6)
    # per-pose batches + identity + matrix()
    Xb = rng.normal(0, 2, (64, 10, 3)).astype(np.float32)
    Yb = T.view(64, 1).act(_t(Xb, device)) if False else Sim3(T.data[:, None, :]).act(_t(Xb, device))
    ref = np.stack([oracle.sim3_act(Tn[k], Xb[k]) for k in range(64)])
    np.testing.assert_allclose(Yb.cpu().numpy(), ref, atol=4e-6)
    I = Sim3.Identity(1, device=device)
    assert torch.equal(I.act(_t(X, device)), _t(X, device))
    M = T[7:8].matrix()[0].cpu().numpy()
    np.testing.assert_allclose(M[:3, :3] @ X[0] + M[:3, 3], oracle.sim3_act(Tn[7], X[:1])[0], atol=4e-6)


def test_edge_blocks_full_resolution(device):
    """BASELINE size: 384x512 pointmaps (196 608 points per keyframe), 4 keyframes, 10 directed edges: per-edge
    blocks against the oracle (rel-L2 <= 1e-5) and the multi-GPU edge split (bitwise)."""
    import mast3r_slam_backends as be

    g, d = _graph(device, n_kf=4, h=384, w=512, seed=5, stride=4, extra_edges=1)
    uniq, ie, je, io, jo = oracle.edge_rows(g["ii"], g["jj"])
    Hs_ref, gs_ref = oracle.gn_edges("rays", g["Twc"], g["Xs"], g["Cs"], None, ie, je, g["idx_ii2jj"], g["valid_match"],
                                     g["Q"], 0.003, 10.0, 0.0, 1.5)
    args = ("rays", d["Twc"], d["Xs"], d["Cs"], None, d["ii"], d["jj"])
    Hs, gs = be.gn_blocks(*args, d["idx_ii2jj"], d["valid_match"], d["Q"], 0.003, 10.0, 0.0, 1.5)
    for e in range(Hs.shape[1]):
        for blk in range(4):
            assert _rel(Hs[blk, e].cpu().numpy(), Hs_ref[blk, e]) <= 1e-5
        for blk in range(2):
            assert _rel(gs[blk, e].cpu().numpy(), gs_ref[blk, e]) <= 1e-5
    E = g["ii"].shape[0]
    cut = E // 2
    parts = [be.gn_blocks(*args, d["idx_ii2jj"][a:a + n].contiguous(), d["valid_match"][a:a + n].contiguous(),
                          d["Q"][a:a + n].contiguous(), 0.003, 10.0, 0.0, 1.5, edge_begin=a, edge_count=n)
             for a, n in ((0, cut), (cut, E - cut))]
    assert torch.equal(parts[0][0] + parts[1][0], Hs) and torch.equal(parts[0][1] + parts[1][1], gs)


def _gn_call(be, kind, Twc, d, h, w, sa, sb, iters, delta):
    if kind == "rays":
        return be.gauss_newton_rays(Twc, d["Xs"], d["Cs"], d["ii"], d["jj"], d["idx_ii2jj"], d["valid_match"],
                                    d["Q"], sa, sb, 0.0, 1.5, iters, delta)[0]
    return be.gauss_newton_calib(Twc, d["Xs"], d["Cs"], d["K"], d["ii"], d["jj"], d["idx_ii2jj"], d["valid_match"],
                                 d["Q"], h, w, -10, 1e-6, sa, sb, 0.0, 1.5, iters, delta)[0]


@pytest.mark.parametrize("kind,n_kf", [("rays", 110), ("calib", 110), ("rays", 125), ("calib", 125)])
def test_config3_graph_sizes(device, kind, n_kf):
    """BASELINE config 3's graph: the reference's keyframe capacity (110, frame.py:221) and the 125 keyframes a
    1 000-frame stream at one keyframe per 8 frames reaches; consecutive + 3 earlier edges per keyframe (SURVEY
    §8d), both directions.  One iteration: dx <= 1e-5 (poses <= 5e-5); full 10-iteration loop: poses <= 2e-4; and the
    LLT-failure path (no valid residual) leaves the poses untouched.  868 unknowns = 14 trailing-update steps of
    the blocked factorisation on 64x64 f64-MFMA tiles."""
    import mast3r_slam_backends as be

    h, w = 24, 32
    g, d = _graph(device, n_kf=n_kf, h=h, w=w, seed=21, stride=1, extra_edges=3, pose_noise=0.005)
    sa, sb = PARAMS[kind]
    args = (kind, g["Twc"], g["Xs"], g["Cs"], g["K"], g["ii"], g["jj"], g["idx_ii2jj"], g["valid_match"], g["Q"],
            sa, sb, 0.0, 1.5)
    kw = dict(height=h, width=w, pixel_border=-10, z_eps=1e-6)
    T1, dx1, _ = oracle.gauss_newton(*args, 1, 1e-8, **kw)
    Twc = d["Twc"].clone()
    dx = _gn_call(be, kind, Twc, d, h, w, sa, sb, 1, 1e-8)
    assert dx.shape == (n_kf - 1, 7)
    np.testing.assert_allclose(dx.cpu().numpy(), dx1, rtol=0, atol=1e-5)
    # a step difference d moves a translation by up to (1 + |t|) d and the room's poses have |t| <= 3.5 m
    np.testing.assert_allclose(Twc.cpu().numpy(), T1, rtol=0, atol=5e-5)
    T10, _, it = oracle.gauss_newton(*args, 10, 1e-8, **kw)
    Twc = d["Twc"].clone()
    _gn_call(be, kind, Twc, d, h, w, sa, sb, 10, 1e-8)
    np.testing.assert_allclose(Twc.cpu().numpy(), T10, rtol=0, atol=2e-4)
    np.testing.assert_array_equal(Twc[0].cpu().numpy(), g["Twc"][0])
    # LLT failure at this size
    Twc = d["Twc"].clone()
    dd = dict(d, valid_match=torch.zeros_like(d["valid_match"]))
    dx = _gn_call(be, kind, Twc, dd, h, w, sa, sb, 3, 1e-8)
    assert not dx.cpu().numpy().any() and torch.equal(Twc, d["Twc"])


@pytest.mark.parametrize("n_kf", [300, 450])
def test_no_pose_cap(device, n_kf):
    """Beyond the 417-pose limit of the round-1 solver (and through the multi-workgroup back-substitution used above
    2 048 unknowns).  A 450-pose chain has condition number ~1e7, so the fp32 rounding of the edge blocks (which both
    sides share only to 1e-5) is amplified in dx; the solver itself is therefore checked on IDENTICAL blocks - the
    oracle's assemble + dense LL^T (gn_kernels.cu:57-159) fed with the blocks the HIP kernels produced - to 1e-7 of
    the step, and the end-to-end step against the oracle loop to 1e-3 of the step."""
    import mast3r_slam_backends as be

    h, w = 12, 16
    g, d = _graph(device, n_kf=n_kf, h=h, w=w, seed=5, stride=1, extra_edges=3, pose_noise=0.005)
    Hs, gs = be.gn_blocks("rays", d["Twc"], d["Xs"], d["Cs"], None, d["ii"], d["jj"], d["idx_ii2jj"], d["valid_match"],
                          d["Q"], 0.003, 10.0, 0.0, 1.5)
    uniq, ie, je, io, jo = oracle.edge_rows(g["ii"], g["jj"])
    dx_same, failed = oracle.gn_solve(Hs.cpu().numpy(), gs.cpu().numpy(), io, jo, n_kf - 1)
    assert not failed
    Twc = d["Twc"].clone()
    dx = _gn_call(be, "rays", Twc, d, h, w, 0.003, 10.0, 1, 1e-8).cpu().numpy()
    scale = np.abs(dx_same).max()
    assert np.abs(dx - dx_same).max() <= 1e-6 * max(scale, 1.0), (np.abs(dx - dx_same).max(), scale)
    T1, dx1, _ = oracle.gauss_newton("rays", g["Twc"], g["Xs"], g["Cs"], None, g["ii"], g["jj"], g["idx_ii2jj"],
                                     g["valid_match"], g["Q"], 0.003, 10.0, 0.0, 1.5, 1, 1e-8)
    assert np.abs(dx - dx1).max() <= 1e-3 * max(np.abs(dx1).max(), 1.0)
    np.testing.assert_allclose(Twc.cpu().numpy(), oracle.sim3_retr_rows(dx_same, g["Twc"]), rtol=0, atol=2e-5)


def test_compaction_gates(device):
    """The once-per-call compaction applies exactly the reference's pose-independent gates (valid_match,
    Q > Q_thresh, Ci[idx] > C_thresh, Cj > C_thresh, gn_kernels.cu:905-925): blocks with non-trivial thresholds
    equal the oracle's, and points failing a gate contribute nothing."""
    import mast3r_slam_backends as be

    g, d = _graph(device, n_kf=5, h=48, w=64, seed=9)
    uniq, ie, je, io, jo = oracle.edge_rows(g["ii"], g["jj"])
    for kind in ("rays", "calib", "points"):
        sa, sb = PARAMS[kind]
        Hr, gr = oracle.gn_edges(kind, g["Twc"], g["Xs"], g["Cs"], g["K"], ie, je, g["idx_ii2jj"], g["valid_match"],
                                 g["Q"], sa, sb, 1.8, 2.4, height=48, width=64, pixel_border=3, z_eps=1e-6)
        Hs, gs = be.gn_blocks(kind, d["Twc"], d["Xs"], d["Cs"], d["K"], d["ii"], d["jj"], d["idx_ii2jj"],
                              d["valid_match"], d["Q"], sa, sb, 1.8, 2.4, height=48, width=64, pixel_border=3,
                              z_eps=1e-6)
        assert _rel(Hs.cpu().numpy(), Hr) <= 1e-5 and _rel(gs.cpu().numpy(), gr) <= 1e-5


def test_hub_keyframe_with_many_neighbours(device):
    """A keyframe connected to 44 others (a revisited place): its block row of the normal equations has more column
    blocks than the assemble kernel's LDS table holds (32), so the rest go through the read-modify-write path.  Solver
    checked on identical blocks against the oracle's assemble + dense LL^T, and end to end."""
    import mast3r_slam_backends as be

    h, w, n_kf = 12, 16, 46
    pairs = [(k - 1, k) for k in range(1, n_kf)] + [(0, k) for k in range(2, n_kf)]
    g, d = _graph(device, n_kf=n_kf, h=h, w=w, seed=8, stride=1, pose_noise=0.004, pairs=pairs)
    Hs, gs = be.gn_blocks("rays", d["Twc"], d["Xs"], d["Cs"], None, d["ii"], d["jj"], d["idx_ii2jj"], d["valid_match"],
                          d["Q"], 0.003, 10.0, 0.0, 1.5)
    uniq, ie, je, io, jo = oracle.edge_rows(g["ii"], g["jj"])
    # hub = keyframe 0 is the pinned one: its row is dropped; make keyframe 1 a hub too by pinning order: use jo/io as is
    dx_same, failed = oracle.gn_solve(Hs.cpu().numpy(), gs.cpu().numpy(), io, jo, n_kf - 1)
    assert not failed
    Twc = d["Twc"].clone()
    dx = _gn_call(be, "rays", Twc, d, h, w, 0.003, 10.0, 1, 1e-8).cpu().numpy()
    assert np.abs(dx - dx_same).max() <= 1e-6 * max(np.abs(dx_same).max(), 1.0)
    # the same with the hub NOT pinned (global ids reversed: the hub gets the largest id, i.e. the last block row)
    g2 = dict(g, ii=g["ii"].max() - g["ii"], jj=g["jj"].max() - g["jj"])
    order = np.argsort(np.unique(np.concatenate((g2["ii"], g2["jj"]))))    # rows follow the sorted ids: reverse the stacks
    Twc2, Xs2, Cs2 = g["Twc"][::-1].copy(), g["Xs"][::-1].copy(), g["Cs"][::-1].copy()
    d2 = {k: _t(v, device) for k, v in dict(Twc=Twc2, Xs=Xs2, Cs=Cs2, ii=g2["ii"], jj=g2["jj"], idx_ii2jj=g["idx_ii2jj"],
                                            valid_match=g["valid_match"], Q=g["Q"]).items()}
    Hs2, gs2 = be.gn_blocks("rays", d2["Twc"], d2["Xs"], d2["Cs"], None, d2["ii"], d2["jj"], d2["idx_ii2jj"],
                            d2["valid_match"], d2["Q"], 0.003, 10.0, 0.0, 1.5)
    _, _, _, io2, jo2 = oracle.edge_rows(g2["ii"], g2["jj"])
    assert (np.bincount(np.concatenate((io2[io2 >= 0], jo2[jo2 >= 0]))).max() // 2) >= 44    # a row with 44+ neighbours
    dx_same2, failed2 = oracle.gn_solve(Hs2.cpu().numpy(), gs2.cpu().numpy(), io2, jo2, n_kf - 1)
    assert not failed2
    T2 = d2["Twc"].clone()
    dx2 = _gn_call(be, "rays", T2, d2, h, w, 0.003, 10.0, 1, 1e-8).cpu().numpy()
    assert np.abs(dx2 - dx_same2).max() <= 1e-6 * max(np.abs(dx_same2).max(), 1.0)


@pytest.mark.parametrize("n_kf", [120, 420])
def test_banded_graph_with_loop_closures(device, n_kf):
    """The usual SLAM graph - consecutive + two recent neighbours, a loop closure to an early keyframe every 40th -
    where most 64x64 tiles of the trailing matrix lie outside the rows' envelopes and their workgroups leave without
    touching the matrix (chol_step_kernel, tmin32): solver on IDENTICAL blocks against the oracle's dense LL^T, with the
    one-workgroup (120 keyframes) and the per-panel (420) back-substitution."""
    import mast3r_slam_backends as be

    h, w = 12, 16
    rng = np.random.default_rng(n_kf)
    pairs = [(k - 1, k) for k in range(1, n_kf)]
    for k in range(3, n_kf):
        pairs += [(k - 2, k), (k - 3, k)]
        if k % 40 == 0:
            pairs.append((int(rng.integers(0, k // 3)), k))
    g, d = _graph(device, n_kf=n_kf, h=h, w=w, seed=6, stride=1, pose_noise=0.004, pairs=pairs)
    Hs, gs = be.gn_blocks("rays", d["Twc"], d["Xs"], d["Cs"], None, d["ii"], d["jj"], d["idx_ii2jj"], d["valid_match"],
                          d["Q"], 0.003, 10.0, 0.0, 1.5)
    uniq, ie, je, io, jo = oracle.edge_rows(g["ii"], g["jj"])
    dx_same, failed = oracle.gn_solve(Hs.cpu().numpy(), gs.cpu().numpy(), io, jo, n_kf - 1)
    assert not failed
    Twc = d["Twc"].clone()
    dx = _gn_call(be, "rays", Twc, d, h, w, 0.003, 10.0, 1, 1e-8).cpu().numpy()
    scale = np.abs(dx_same).max()
    assert np.abs(dx - dx_same).max() <= 1e-6 * max(scale, 1.0), (np.abs(dx - dx_same).max(), scale)
    np.testing.assert_allclose(Twc.cpu().numpy(), oracle.sim3_retr_rows(dx_same, g["Twc"]), rtol=0, atol=2e-5)


def _dense_normal_equations(Hs, gs, io, jo, N):
    """The reference's assembly (update_lhs / update_rhs, gn_kernels.cu:71-113, 1201-1206) as a dense fp64 system:
    blocks [ii, ij, ji, jj] of every directed edge summed into (7N, 7N), rhs blocks [i, j] into (7N); pinned rows
    (index < 0) dropped."""
    n = 7 * N
    H, b = np.zeros((n, n)), np.zeros(n)
    Hd, gd = Hs.astype(np.float64), gs.astype(np.float64)
    for e in range(len(io)):
        i, j = int(io[e]), int(jo[e])
        if i >= 0:
            H[7 * i:7 * i + 7, 7 * i:7 * i + 7] += Hd[0, e]
            b[7 * i:7 * i + 7] += gd[0, e]
        if i >= 0 and j >= 0:
            H[7 * i:7 * i + 7, 7 * j:7 * j + 7] += Hd[1, e]
            H[7 * j:7 * j + 7, 7 * i:7 * i + 7] += Hd[2, e]
        if j >= 0:
            H[7 * j:7 * j + 7, 7 * j:7 * j + 7] += Hd[3, e]
            b[7 * j:7 * j + 7] += gd[1, e]
    return H, b


def test_config5_graph_size(device):
    """BASELINE config 5: a 10 000-frame stream at one keyframe per 8 frames = 1 250 keyframes, consecutive + 3 random
    earlier edges per keyframe = 9 990 directed edges, 8 743 unknowns - eleven times the reference's
    110-slot store.  12x16 pointmaps keep the edge kernels small; what is under test is everything whose cost grows with
    the graph: index preparation, block assembly, the blocked fp64 LL^T (137 outer blocks) and the multi-workgroup back
    substitution.  The solver is checked on IDENTICAL blocks: the HIP blocks assembled as the reference assembles them
    and solved by LAPACK's dense Cholesky (the reference's SimplicialLLT solves the same system, gn_kernels.cu:132-153)
    - to 1e-6 of the step - and the poses against the retraction of that step."""
    import scipy.linalg

    import mast3r_slam_backends as be

    h, w, n_kf = 12, 16, 1250
    g, d = _graph(device, n_kf=n_kf, h=h, w=w, seed=50, stride=1, extra_edges=3, pose_noise=0.004)
    assert len(g["ii"]) >= 4 * (n_kf - 4) * 2 - 16
    Hs, gs = be.gn_blocks("rays", d["Twc"], d["Xs"], d["Cs"], None, d["ii"], d["jj"], d["idx_ii2jj"], d["valid_match"],
                          d["Q"], 0.003, 10.0, 0.0, 1.5)
    uniq, ie, je, io, jo = oracle.edge_rows(g["ii"], g["jj"])
    H, b = _dense_normal_equations(Hs.cpu().numpy(), gs.cpu().numpy(), io, jo, n_kf - 1)
    assert np.abs(H - H.T).max() <= 1e-9 * np.abs(H).max()
    x = scipy.linalg.cho_solve(scipy.linalg.cho_factor(H, lower=True), b)
    dx_same = -x.reshape(n_kf - 1, 7)                                  # "Accounting for negative here" :1208-1209
    Twc = d["Twc"].clone()
    dx = _gn_call(be, "rays", Twc, d, h, w, 0.003, 10.0, 1, 1e-8).cpu().numpy()
    assert dx.shape == (n_kf - 1, 7)
    scale = np.abs(dx_same).max()
    assert np.abs(dx - dx_same).max() <= 1e-6 * max(scale, 1.0), (np.abs(dx - dx_same).max(), scale)
    np.testing.assert_allclose(Twc.cpu().numpy(), oracle.sim3_retr_rows(dx_same.astype(np.float32), g["Twc"]), rtol=0, atol=2e-5)
    np.testing.assert_array_equal(Twc[0].cpu().numpy(), g["Twc"][0])
