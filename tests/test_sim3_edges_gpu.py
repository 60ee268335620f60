"""mslam_sim3_op, mslam_sim3_act and lietorch_hip.Sim3 at their edges against the float64 group of tests/sim3_ref.py:
the exponential on both sides of each of its thresholds, batch sizes around the 64- and 256-thread blocks, the broadcast
flags, pose boundaries inside a block, scales of 1e-3 to 1e3, rotations at pi, unit quaternions through 500 generations,
and the shapes and dtypes the class accepts.  Every tolerance is an exact equality, a bound derived where it stands, or
FACTOR x a float32 baseline that tests/test_sim3_ref_cpu.py re-measures; each test prints its error as a multiple of
the baseline."""
import numpy as np
import pytest
import torch

import mslam_hip
import sim3_ref as S
from lietorch_hip import Sim3

pytestmark = pytest.mark.gpu

INV, MUL, EXP, RETR = 0, 1, 2, 3
SIZES = (1, 63, 64, 65, 1000)      # below, at and above the op kernel's 64-thread block; many blocks
# | |q| - 1 | after the float32 sim3_unit (inv, mul, retr), worst case, u = 2^-24: q.q is four rounded squares and three
# rounded sums of positive terms (4u), its square root halves that and rounds (3u), the reciprocal rounds (4u), each
# product q_i * inv rounds (5u).
UNIT_BOUND = 5 * 2.0 ** -24


def _d(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _op(op, A, B, n, ba=0, bb=0):
    """mslam_sim3_op into a fresh (n,8) buffer of NaNs (a row the kernel skips stays NaN)."""
    out = torch.full((n, 8), float("nan"), dtype=torch.float32, device=A.device)
    rc = mslam_hip.lib().mslam_sim3_op(op, mslam_hip.ptr(A), mslam_hip.ptr(B), mslam_hip.ptr(out), n, ba, bb,
                                       mslam_hip.stream_ptr())
    mslam_hip.check(rc, "sim3_op")
    return out


def _act(T, X, num_poses, pts_per_pose, broadcast):
    Y = torch.full((num_poses * pts_per_pose, 3), float("nan"), dtype=torch.float32, device=X.device)
    rc = mslam_hip.lib().mslam_sim3_act(mslam_hip.ptr(T), mslam_hip.ptr(X), mslam_hip.ptr(Y), num_poses, pts_per_pose,
                                        broadcast, mslam_hip.stream_ptr())
    mslam_hip.check(rc, "sim3_act")
    return Y


def _hold(op, m):
    """Print every measure as a multiple of its baseline, then assert FACTOR x baseline."""
    base = S.BASELINES[op]
    print(f"sim3 {op:5s} " + "  ".join(f"{k} {m[k]:.2e} ({m[k] / base[k]:.2f} x baseline)" for k in base if k in m))
    for k in base:
        if k in m:
            assert m[k] <= S.FACTOR * base[k], (op, k, m[k])


def _unit_error(T):
    q = T.detach().cpu().numpy().reshape(-1, 8)[:, 3:7].astype(np.float64)
    return float(np.abs(np.linalg.norm(q, axis=1) - 1.0).max())


@pytest.fixture(scope="module")
def grid(device):
    xi, theta, sigma = S.exp_grid()
    M64 = S.exp_m(xi)
    xi_d = _d(xi, device)
    return dict(xi=xi, xi_d=xi_d, M64=M64, tol=S.exp_trans_tol(xi, M64), full=_op(EXP, xi_d, None, xi.shape[0]))


@pytest.fixture(scope="module")
def base(device):
    d = S.base_inputs()
    d.update({k + "_d": _d(v, device) for k, v in d.items()})
    return d


# ---- exp --------------------------------------------------------------------------------------------------------------
def test_exp_grid(grid):
    """The whole grid in one launch: translation inside the row's own tolerance (sim3_ref.exp_trans_tol), rotation and
    scale at FACTOR x baseline."""
    T = grid["full"].cpu().numpy()
    assert np.isfinite(T).all()
    e = S.pose_errors(T, grid["M64"])
    ratio = e["trans"] / grid["tol"]
    print(f"sim3 exp   trans worst error / row tolerance {ratio.max():.2f} (row {int(ratio.argmax())})")
    _hold("exp", dict(rot=float(e["rot"].max()), scale=float(e["scale"].max())))
    assert (e["trans"] <= grid["tol"]).all(), (np.flatnonzero(e["trans"] > grid["tol"])[:8], ratio.max())


def test_exp_unit_quaternions(grid):
    """Every quaternion of the grid satisfies | |q| - 1 | <= 2^-23, the norm taken in float64.  The op kernel normalises
    exp's quaternion with the norm in double (sim3_unit_f64, gn.hip), each component rounded once: 2^-24 at most.  The
    float32 sim3_unit, which exp used before, gave 2.10 x 2^-24 on this grid, above the bound on 4 of the 1456 rows."""
    err = _unit_error(grid["full"])
    print(f"sim3 exp   | |q| - 1 | max {err:.3e} = {err * 2.0 ** 24:.2f} x 2^-24 (bound 2)")
    assert err <= 2.0 ** -23


def test_exp_small_angle_quaternion_bits(grid):
    """Below theta^2 = 1e-6 so3_exp is a series in theta^2 and the normalisation a reciprocal square root in double:
    +, -, x, / and sqrt only, no library function, each correctly rounded on the host and on the device and the library
    built without contraction.  So the kernel's quaternion equals the float32 restatement's bit for bit on those rows
    (7 of the 13 theta values, 0 to 9.9e-4).  No accuracy measure can see the series' theta^2 term - it moves the angle
    by theta^3 / 12 < 1e-10 - but it decides the last bit of q."""
    xi = grid["xi"]
    phi = xi[:, 3:6]
    small = phi[:, 0] * phi[:, 0] + phi[:, 1] * phi[:, 1] + phi[:, 2] * phi[:, 2] < np.float32(1e-6)
    assert small.sum() == 7 * 8 * len(S.SIGMAS)
    got, want = _bits(grid["full"])[small, 3:7], S.exp32(xi)[small, 3:7].view(np.int32)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(1))[:8]


def test_exp_rows_are_independent(grid):
    """Prefixes of 1, 63, 64 and 65 rows and 20 single rows, each as its own call, give the bits of the full launch."""
    full = _bits(grid["full"])
    for n in (1, 63, 64, 65):
        assert np.array_equal(_bits(_op(EXP, grid["xi_d"][:n].contiguous(), None, n)), full[:n]), n
    for r in np.random.default_rng(2).choice(full.shape[0], 20, replace=False):
        assert np.array_equal(_bits(_op(EXP, grid["xi_d"][r:r + 1].contiguous(), None, 1))[0], full[r]), r


# ---- inv, mul, retr ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_inv_mul_retr_against_float64(base, n):
    """The first n rows of the baseline inputs (scales 1e-3..1e3, |t| to 1e3, identities, rotations at pi, both signs
    of q; steps from the well-conditioned cells): rotation, scale and scaled translation at FACTOR x baseline, unit
    quaternions to UNIT_BOUND."""
    A, B, xi = base["A"][:n], base["B"][:n], base["xi"][:n]
    Ad, Bd, xid = (base[k][:n].contiguous() for k in ("A_d", "B_d", "xi_d"))
    runs = {"inv": (_op(INV, Ad, None, n), S.inv_m(A), S.size_inv(A)),
            "mul": (_op(MUL, Ad, Bd, n), S.mul_m(A, B), S.size_mul(A, B)),
            "retr": (_op(RETR, xid, Bd, n), S.retr_m(xi, B), S.size_mul(S.exp_m(xi), B))}
    for op, (T, M64, size) in runs.items():
        assert torch.isfinite(T).all(), op
        _hold(op, S.measure(T.cpu().numpy(), M64, size))
        assert _unit_error(T) <= UNIT_BOUND, op


@pytest.mark.parametrize("op", [INV, MUL, EXP, RETR])
def test_zero_rows_is_a_no_op(base, op):
    out = torch.full((4, 8), 7.0, dtype=torch.float32, device=base["A_d"].device)
    A = base["xi_d"] if op in (EXP, RETR) else base["A_d"]
    rc = mslam_hip.lib().mslam_sim3_op(op, mslam_hip.ptr(A), mslam_hip.ptr(base["B_d"]), mslam_hip.ptr(out), 0, 0, 0,
                                       mslam_hip.stream_ptr())
    assert rc == 0
    assert torch.equal(out, torch.full_like(out, 7.0))


@pytest.mark.parametrize("op", [INV, MUL, EXP, RETR])
def test_broadcast_flags(base, op):
    """bcast_a / bcast_b read row 0 for every output row: each setting gives the bits of a plain call on materialised
    copies; with both set every row is row 0's result.  Both operands are full n-row buffers with distinct rows, so a
    flag that is ignored shows as a difference and nothing is read outside a buffer."""
    n = 65
    A = (base["xi_d"] if op in (EXP, RETR) else base["A_d"])[:n].contiguous()
    B = base["B_d"][:n].contiguous()
    A0, B0 = A[:1].expand(n, -1).contiguous(), B[:1].expand(n, -1).contiguous()
    plain = _op(op, A, B, n)
    for ba, bb in ((0, 0), (1, 0), (0, 1), (1, 1)):
        got = _op(op, A, B, n, ba, bb)
        want = _op(op, A0 if ba else A, B0 if bb else B, n)
        assert np.array_equal(_bits(got), _bits(want)), (op, ba, bb)
        binary = op in (MUL, RETR)
        if ba or (bb and binary):
            assert not np.array_equal(_bits(got), _bits(plain)), (op, ba, bb)
        if ba and (bb or not binary):
            assert np.array_equal(_bits(got), np.broadcast_to(_bits(got)[:1], (n, 8))), (op, ba, bb)


def test_class_broadcast_shapes(base):
    """(1,)*(n,), (n,)*(1,), retr of xi (1,7) on n poses and of xi (n,7) on one pose, through the class: the shape of
    the larger operand, the bits of the C call on materialised copies."""
    n = 65
    A, B, xi = (base[k][:n].contiguous() for k in ("A_d", "B_d", "xi_d"))
    rep = lambda t: t[:1].expand(n, -1).contiguous()
    cases = [(Sim3(A[:1]) * Sim3(B), _op(MUL, rep(A), B, n)),
             (Sim3(A) * Sim3(B[:1]), _op(MUL, A, rep(B), n)),
             (Sim3(B).retr(xi[:1]), _op(RETR, rep(xi), B, n)),
             (Sim3(B[:1]).retr(xi), _op(RETR, xi, rep(B), n))]
    for k, (got, want) in enumerate(cases):
        assert got.data.shape == (n, 8) and got.shape == (n,), k
        assert np.array_equal(_bits(got.data), _bits(want)), k
    got = Sim3(A[:60].reshape(5, 12, 8)) * Sim3(B[:1])
    assert got.data.shape == (5, 12, 8) and np.array_equal(_bits(got.data).reshape(60, 8), _bits(cases[1][1])[:60])
    got = Sim3(B[:1]).retr(xi[:60].reshape(5, 12, 7))
    assert got.data.shape == (5, 12, 8) and np.array_equal(_bits(got.data).reshape(60, 8), _bits(cases[3][1])[:60])


# ---- act --------------------------------------------------------------------------------------------------------------
def _integer_poses(n):
    T = np.zeros((n, 8), np.float32)
    T[:, 0] = 1000.0 * (1 + np.arange(n))
    T[:, 6] = 1.0
    T[:, 7] = 1.0
    return T


def test_act_pose_index_is_exact(device):
    """Pure translations t = (1000 (k + 1), 0, 0), identity rotation, s = 1, integer points below 500: every result
    is an integer below 2^24, exact in float32, and a point that takes its neighbour's pose is off by 1000.  Pose counts
    {1, 2, 3, 65} x points per pose {1, 7, 255, 256, 257}: pose boundaries at, before and after the 256-thread block's."""
    rng = np.random.default_rng(4)
    for num_poses in (1, 2, 3, 65):
        T = _integer_poses(num_poses)
        for ppp in (1, 7, 255, 256, 257):
            X = rng.integers(-499, 500, (num_poses * ppp, 3)).astype(np.float32)
            want = X.copy()
            want[:, 0] += np.repeat(T[:, 0], ppp)
            got = _act(_d(T, device), _d(X, device), num_poses, ppp, 0).cpu().numpy()
            assert np.array_equal(got, want), (num_poses, ppp)


def test_act_broadcast_pose_is_exact(device):
    """broadcast_pose = 1 with totals of 1, 255, 256 and 257 points: every point takes pose 0, both as the class calls it
    (one pose, all points under it) and with `total` distinct poses in the buffer and one point each - there a flag that
    is ignored gives point k pose k, and still reads inside the buffer."""
    rng = np.random.default_rng(6)
    for total in (1, 255, 256, 257):
        T = _integer_poses(total)
        X = rng.integers(-499, 500, (total, 3)).astype(np.float32)
        want = X.copy()
        want[:, 0] += T[0, 0]
        Td, Xd = _d(T, device), _d(X, device)
        assert np.array_equal(_act(Td, Xd, 1, total, 1).cpu().numpy(), want), total
        assert np.array_equal(_act(Td, Xd, total, 1, 1).cpu().numpy(), want), total


def test_act_against_float64(base):
    """Random poses and points over the full ranges, |Y - Y64|_inf / (s |X| + |t|) at FACTOR x baseline: one point per
    pose (the pairing the baseline was measured on), 125 poses x 8 points, and pose 3 broadcast over all points."""
    A, X = base["A"], base["X"]
    n = S.N_BASE
    for name, (Y, Aeff) in {
            "1000x1": (_act(base["A_d"], base["X_d"], n, 1, 0), A),
            "125x8": (_act(base["A_d"], base["X_d"], 125, 8, 0), np.repeat(A[:125], 8, 0)),
            "bcast": (_act(base["A_d"][3:4].contiguous(), base["X_d"], 1, n, 1), np.repeat(A[3:4], n, 0))}.items():
        err = S.scaled(np.abs(Y.cpu().numpy() - S.act(Aeff, X)).max(1), S.size_act(Aeff, X))
        print(f"sim3 act {name}:", end=" ")
        _hold("act", dict(trans=float(err.max())))


# ---- the generation cycle ---------------------------------------------------------------------------------------------
def test_generation_cycle_keeps_similarities(base):
    """500 rounds of T_rel = T_k^-1 T_f; T_f = T_k T_rel on 64 pose pairs through the class (the frontend's cycle;
    sim3.h's sim3_unit exists for it).  At rounds 1, 10, 100 and 500 every quaternion of T_rel and T_f is unit to 2^-22,
    and T_f has drifted from its start by at most rounds x FACTOR x one round's float32 error - linear accumulation,
    the worst case.  One round's error, from the baselines e = {rot, scale, trans} of inv and mul:
      rotation  R_f' = R_k (R_k^-1 R_f): e_inv.rot + 2 e_mul.rot;  scale likewise.
      translation: t_rel = s_ki R_ki t_f + t_ki carries (e_inv.scale + e_inv.rot) |t_f| / s_k from the inverse's scale
        and rotation, e_inv.trans |t_k| / s_k from its translation and e_mul.trans (|t_f| + |t_k|) / s_k of its own;
        t_f' = s_k R_k t_rel + t_k multiplies that by s_k and adds e_mul.trans (s_k |t_rel| + |t_k|) with
        s_k |t_rel| <= |t_f| + |t_k|.  The sum is at most
        (e_inv.rot + e_inv.scale + e_inv.trans + 2 e_mul.trans) (|t_f| + 2 |t_k|), so the drift of t_f is measured over
        |t_f| + 2 |t_k|."""
    n = 64
    Tk_np, Tf_np = base["A"][:n], base["B"][:n]
    Tk, Tf = Sim3(base["A_d"][:n].contiguous()), Sim3(base["B_d"][:n].contiguous())
    M0 = S.matrices(Tf_np)
    size = np.linalg.norm(Tf_np[:, :3].astype(np.float64), axis=1) + 2 * np.linalg.norm(Tk_np[:, :3].astype(np.float64), axis=1)
    bi, bm = S.BASELINES["inv"], S.BASELINES["mul"]
    per_round = dict(rot=bi["rot"] + 2 * bm["rot"], scale=bi["scale"] + 2 * bm["scale"],
                     trans=bi["rot"] + bi["scale"] + bi["trans"] + 2 * bm["trans"])
    for r in range(1, 501):
        Trel = Tk.inv() * Tf
        Tf = Tk * Trel
        if r in (1, 10, 100, 500):
            assert _unit_error(Trel.data) <= 2.0 ** -22 and _unit_error(Tf.data) <= 2.0 ** -22, r
            m = S.measure(Tf.data.cpu().numpy(), M0, size)
            print(f"sim3 cycle round {r:3d}: " + "  ".join(f"{k} {m[k]:.2e} ({m[k] / (r * per_round[k]):.2f} x rounds x "
                                                             f"baseline)" for k in per_round))
            for k in per_round:
                assert m[k] <= r * S.FACTOR * per_round[k], (r, k, m[k])


# ---- the class on the device ------------------------------------------------------------------------------------------
def test_class_matrix_identity_view_index(base):
    dev = base["A_d"].device
    A = base["A"][:60]
    T = Sim3(base["A_d"][:60].clone())
    M = T.view(5, 12).matrix()
    assert M.shape == (5, 12, 4, 4)
    M = M.cpu().numpy().reshape(60, 4, 4).astype(np.float64)
    want = S.matrices(A)
    # an entry of R is quadratic in q and below 1: a few float32 roundings, and q is unit to 4 ulps (8 ulps of R); 32 ulps
    # of s in all.  The translation column and the last row are copied.
    assert (np.abs(M - want)[:, :3, :3].max((1, 2)) <= 32 * S.F32_EPS * A[:, 7]).all()
    assert np.array_equal(M[:, :3, 3], A[:, :3].astype(np.float64)) and np.array_equal(M[:, 3], want[:, 3])
    I = Sim3.Identity(3, 2, device=dev)
    assert I.shape == (3, 2) and I.data.dtype == torch.float32 and I.device.type == "cuda"
    assert torch.equal(I.data, torch.tensor([0, 0, 0, 0, 0, 0, 1, 1.0], device=dev).expand(3, 2, 8))
    assert torch.equal(I.matrix(), torch.eye(4, device=dev).expand(3, 2, 4, 4))
    X = base["X_d"][:50]
    assert torch.equal(Sim3.Identity(1, device=dev).act(X), X)
    assert np.array_equal(_bits((I.view(6) * T[:6]).data), _bits(_op(MUL, I.data.view(6, 8), T.data[:6].contiguous(), 6)))
    assert torch.equal(T.view(5, 12)[2, 3].data, T.data[27]) and torch.equal(T[7:9].data, T.data[7:9])
    T[4] = Sim3.Identity(device=dev)
    T[5:7] = base["B_d"][:2]
    assert torch.equal(T.data[4], I.data[0, 0]) and torch.equal(T.data[5:7], base["B_d"][:2])
    assert torch.equal(T.data[7:], base["A_d"][7:60]) and torch.equal(T.clone().data, T.data)


def test_class_non_contiguous_data(base):
    """Sim3(d[:, None, :])[pin:] (as the global optimiser builds its poses) and d[::2]: inv, *, retr, act and matrix
    give the bits of contiguous copies."""
    d, xi, X = base["A_d"][:40], base["xi_d"][:40], base["X_d"]
    pin = 2
    views = {"unsqueezed": Sim3(d[:, None, :])[pin:], "strided": Sim3(d[::2])}
    assert not views["strided"].data.is_contiguous()
    for name, V in views.items():
        C = Sim3(V.data.contiguous().clone())
        m = V.data.reshape(-1, 8).shape[0]
        other = Sim3(base["B_d"][:m].reshape(*V.data.shape[:-1], 8))
        step = xi[:m].reshape(*V.data.shape[:-1], 7)
        Xs = X[:m * 5].reshape(*V.data.shape[:-1], 5, 3) if name == "strided" else X[:m * 5].reshape(m, 5, 3)
        pairs = [(V.inv(), C.inv()), (V * other, C * other), (other * V, other * C), (V.retr(step), C.retr(step))]
        for k, (a, b) in enumerate(pairs):
            assert a.data.shape == b.data.shape and np.array_equal(_bits(a.data), _bits(b.data)), (name, k)
        assert torch.equal(V.act(Xs), C.act(Xs)) and torch.equal(V.matrix(), C.matrix()), name
        ref = _op(INV, C.data.reshape(-1, 8), None, m)
        assert np.array_equal(_bits(V.inv().data).reshape(-1, 8), _bits(ref)), name


def test_class_converts_float64_poses(base):
    """inv, * and retr of float64 pose data: converted to float32 before the kernel reads it (the bytes of a double
    read as floats would be garbage without any error), float32 result with the bits of the float32 call."""
    dev = base["A_d"].device
    A32, B32, xi = base["A_d"][:65].contiguous(), base["B_d"][:65].contiguous(), base["xi_d"][:65].contiguous()
    A64, B64 = Sim3(A32.double()), Sim3(B32.double())
    for k, (got, want) in enumerate([(A64.inv(), Sim3(A32).inv()), (A64 * B64, Sim3(A32) * Sim3(B32)),
                                     (A64 * Sim3(B32), Sim3(A32) * Sim3(B32)), (B64.retr(xi.double()), Sim3(B32).retr(xi)),
                                     (Sim3.exp(xi.double()), Sim3.exp(xi))]):
        assert got.data.dtype == torch.float32 and got.data.shape == want.data.shape, k
        assert np.array_equal(_bits(got.data), _bits(want.data)), k
    assert torch.equal(A64.act(base["X_d"][:65].double()), Sim3(A32).act(base["X_d"][:65]))
    I = Sim3.Identity(4, device=dev, dtype=torch.float64)
    assert torch.equal(I.inv().data, Sim3.Identity(4, device=dev).data)
    assert np.array_equal(_bits((I * B64[:4]).data), _bits((Sim3.Identity(4, device=dev) * Sim3(B32[:4])).data))


def test_class_act_shape_rule(base):
    """The pose batch shape, trailing 1s dropped, must lead X.shape[:-1]: one pose for all points, (N,1) poses against
    (N,P,3) and (N,) against (N,3) pass and match per-pose calls; two poses against X of shape (3,2,3) - where pose 0
    used to take the first three points - and every other mismatch raise."""
    A, X = base["A_d"], base["X_d"]
    Xb = X[:70].reshape(7, 10, 3)
    Y = Sim3(A[:7, None, :]).act(Xb)
    assert Y.shape == (7, 10, 3)
    for k in range(7):
        assert torch.equal(Y[k], Sim3(A[k:k + 1]).act(Xb[k]))
        assert torch.equal(Y[k], Sim3(A[k]).act(Xb[k]))
    assert torch.equal(Sim3(A[:7]).act(Xb), Y)
    assert torch.equal(Sim3(A[:7]).act(Xb[:, 0]), Y[:, 0])
    assert torch.equal(Sim3(A[:1]).act(Xb), Sim3(A[:1, None, None]).act(Xb))
    assert torch.equal(Sim3(A[:14].reshape(7, 2, 8)).act(Xb.reshape(7, 2, 5, 3))[3, 1], Sim3(A[7:8]).act(Xb[3, 5:]))
    for poses, pts in ((A[:2], X[:18].reshape(3, 2, 3, 3)[:, :, 0]), (A[:2], X[:6]), (A[:3], X[:6].reshape(2, 3, 3)),
                       (A[:6].reshape(2, 3, 8), X[:4].reshape(2, 2, 3)),
                       (A[:5], X[:5].reshape(5, 3)[0])):
        with pytest.raises(RuntimeError, match="Sim3.act"):
            Sim3(poses).act(pts)


def test_class_refuses_sizes_that_do_not_broadcast(base):
    A, B, xi = base["A_d"], base["B_d"], base["xi_d"]
    with pytest.raises(RuntimeError, match="cannot broadcast"):
        Sim3(A[:3]) * Sim3(B[:5])
    with pytest.raises(RuntimeError, match="cannot broadcast"):
        Sim3(B[:5]).retr(xi[:3])
    with pytest.raises(RuntimeError, match="device tensors only"):
        Sim3(A[:3].cpu()) * Sim3(B[:3])
