"""GPU tests (-m gpu) of csrc/matching.hip at its edges: prep_iter_proj, iter_proj, match_occlusion, refine_matches and
pixel_to_lin through the C entry points of mslam_hip, every operand in a guarded buffer (kernel_refs.Guarded), against
the recipes and references of tests/matching_refs.py (checked on their own in tests/test_matching_refs_cpu.py): the
bit-exact C oracle where bit-exactness is the contract, closed forms written out in the recipe, and float64 numpy with
bounds derived from the kernel's operation count.

After every launch the guards in front of and behind every operand must be bit-identical and p_new, converged, p1,
p1_new, idx, rays, pts and p_init fully written; `valid` is read-modify-write, so only its guards are checked."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R  # noqa: E402
import matching_refs as M  # noqa: E402
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu


def _m():
    import mslam_hip as m

    return m


def _g(device, a):
    """Input operand in a guarded buffer (bool as uint8)."""
    a = torch.from_numpy(np.ascontiguousarray(a))
    a = a.to(torch.uint8) if a.dtype == torch.bool else a
    return R.Guarded(device, a.dtype, src=a)


def _p(g):
    """Device address of a guarded buffer's interior, also where it is empty (an empty tensor's data_ptr() is 0)."""
    return 0 if g is None else g.raw.data_ptr() + R.GUARD_BYTES


def _fetch(*tensors):
    """One device-to-host copy for all results (float32 and the integers in use are exact in float64)."""
    flat = torch.cat([t.reshape(-1).double() for t in tensors]).cpu().numpy()
    out, o = [], 0
    for t in tensors:
        out.append(flat[o:o + t.numel()].reshape(tuple(t.shape)))
        o += t.numel()
    return out


def _untouched(g):
    return bool((g.raw == g.pat).all())


# ---- launches --------------------------------------------------------------------------------------------------------
def _prep(device, X11, X21, idx, what):
    m = _m()
    b, h, w, _ = X11.shape
    bufs = {"X11": _g(device, X11), "X21": _g(device, X21), "rays": R.Guarded(device, torch.float32, (b, h, w, 9)),
            "pts": R.Guarded(device, torch.float32, (b, h * w, 3)), "p_init": R.Guarded(device, torch.float32, (b, h * w, 2))}
    if idx is not None:
        bufs["idx_init"] = _g(device, idx)
    rc = m.lib().mslam_prep_iter_proj(_p(bufs["X11"]), _p(bufs["X21"]), _p(bufs.get("idx_init")), _p(bufs["rays"]),
                                      _p(bufs["pts"]), _p(bufs["p_init"]), b, h, w, m.stream_ptr())
    m.check(rc, what)
    R.check_guards(bufs, ["rays", "pts", "p_init"], what)
    return bufs


def _iter_proj(device, rays, pts, p0, iters, lam, thr, what):
    m = _m()
    b, h, w, _ = rays.shape
    n = pts.shape[1]
    bufs = {"rays": _g(device, rays), "pts": _g(device, pts), "p_init": _g(device, p0),
            "p_new": R.Guarded(device, torch.float32, (b, n, 2)), "converged": R.Guarded(device, torch.uint8, (b, n))}
    rc = m.lib().mslam_iter_proj(_p(bufs["rays"]), _p(bufs["pts"]), _p(bufs["p_init"]), _p(bufs["p_new"]),
                                 _p(bufs["converged"]), b, h, w, n, int(iters), float(lam), float(thr), m.stream_ptr())
    m.check(rc, what)
    R.check_guards(bufs, ["p_new", "converged"], what)
    return bufs["p_new"].t, bufs["converged"].t


def _refine(device, D11, D21, p1, radius, dil, what):
    m = _m()
    b, h, w, f = D11.shape
    n = D21.shape[1]
    bufs = {"D11": _g(device, D11), "D21": _g(device, D21), "p1": _g(device, p1),
            "p1_new": R.Guarded(device, torch.int64, (b, n, 2))}
    rc = m.lib().mslam_refine_matches(_p(bufs["D11"]), _p(bufs["D21"]), _p(bufs["p1"]), _p(bufs["p1_new"]), b, h, w, n, f,
                                      int(radius), int(dil), m.stream_ptr())
    m.check(rc, what)
    R.check_guards(bufs, ["p1_new"], what)
    return bufs["p1_new"].t


def _exact(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.size} elements differ, first at {i}: {got[i]!r} != {want[i]!r}")


# ---- 1. prep_iter_proj -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_idx", (False, True), ids=("noidx", "idx"))
@pytest.mark.parametrize("b", M.PREP_B)
@pytest.mark.parametrize("h,w", M.PREP_SHAPES)
def test_prep_against_float64(device, h, w, b, with_idx):
    """Partial 16x16 tiles, 2-wide images (reflect -1 -> 1 and 2 -> 0), blockIdx.z > 0 with another image per batch item,
    the idx_init path, the zero / 1e-13 / small / large planted vectors: every element within the bound derived in
    matching_refs.prep_ref from the kernel's operation sequence, p_init exact."""
    X11, X21, idx = M.prep_inputs(h, w, b, with_idx)
    rays, pts, p0, rb, pb = M.prep_ref(X11, X21, idx)
    bufs = _prep(device, X11, X21, idx, f"prep {h}x{w} b{b}")
    g_rays, g_pts, g_p0 = _fetch(bufs["rays"].t, bufs["pts"].t, bufs["p_init"].t)
    ratio = {"rays": (np.abs(g_rays - rays)[..., :3] / rb[..., :3]).max(), "grad": (np.abs(g_rays - rays)[..., 3:] / rb[..., 3:]).max(),
             "pts": (np.abs(g_pts - pts) / pb).max()}
    print(f"prep {h}x{w} b{b} idx{int(with_idx)} err/bound: " + " ".join(f"{k} {v:.3f}" for k, v in ratio.items()))
    assert max(ratio.values()) <= 1.0, ratio
    _exact(g_p0, p0, "p_init")


def test_prep_golden_in_guarded_buffers(device, golden_dir):
    g = np.load(os.path.join(golden_dir, "prep_iter_proj.npz"))
    bufs = _prep(device, g["X11"], g["X21"], None, "prep golden")
    rays, pts = _fetch(bufs["rays"].t, bufs["pts"].t)
    np.testing.assert_allclose(rays, g["rays_with_grad"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(pts, g["pts3d_norm"], rtol=0, atol=2e-7)


# ---- 2. iter_proj ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _noisy():
    return M.noisy_case()


@functools.lru_cache(maxsize=None)
def _nonfinite():
    return M.nonfinite_case()


def _vs_oracle(device, rays, pts, p0, iters, lam, thr, what):
    p_ref, c_ref = oracle.iter_proj(rays, pts, p0, iters, lam, thr)
    p, c = _fetch(*_iter_proj(device, rays, pts, p0, iters, lam, thr, what))
    _exact(p, p_ref, what + " p_new")
    _exact(c, c_ref, what + " converged")
    return p.astype(np.float32), c


@pytest.mark.parametrize("iters", M.ITERS)
def test_iter_proj_every_transition_and_descent(device, iters):
    """The noisy recipe (every accept / reject transition occurs in more than 1 % of its points: the sample carried over
    from the trial) bit for bit at 0, 1, 2, 10 and 60 iterations (lambda reaches the subnormals and zero), and the same
    with a zero ray, a NaN border pixel of weight 0 and zero targets.  Independent of the oracle: the float64 cost of
    the result is not above that of the clamped start, up to the float32 evaluation error of both."""
    rays, pts, p0 = _noisy()
    h, w = M.NOISY_HW
    p, _ = _vs_oracle(device, rays, pts, p0, iters, M.LAMBDA, M.THRESH, f"noisy it{iters}")
    start = M.clamp_p(p0, h, w)
    if iters == 0:
        _exact(p, start, "clamped start")
    c1, n1 = M.cost64(rays, pts, p)
    c0, n0 = M.cost64(rays, pts, start)
    slack = M.cost_eval_bound(c0, n0) + M.cost_eval_bound(c1, n1)
    assert (c1 <= c0 + slack).all(), f"cost rises by {float((c1 - c0 - slack).max())} over the slack"
    if iters:
        assert (c1 < c0).mean() > 0.5
    _vs_oracle(device, *_nonfinite(), iters, M.LAMBDA, M.THRESH, f"nonfinite it{iters}")


def test_iter_proj_singular_system(device):
    """det == 0 -> delta NaN -> the clamp answers 1 on both axes -> the step to (1, 1) is accepted: closed form."""
    rays, pts, p0, iters, lam = M.singular_case()
    p, c = _fetch(*_iter_proj(device, rays, pts, p0, iters, lam, M.THRESH, "singular"))
    assert (p == 1).all(), f"{(p != 1).any(-1).sum()} points not at (1, 1), e.g. {p[(p != 1).any(-1)][:3]}"
    assert (c == 1).all()
    _vs_oracle(device, rays, pts, p0, iters, lam, M.THRESH, "singular")


def test_iter_proj_start_outside_nonfinite_and_on_the_bounds(device):
    rays, pts, p0, clamped = M.pinit_case()
    p, c = _fetch(*_iter_proj(device, rays, pts, p0, 0, M.LAMBDA, M.THRESH, "p_init it0"))
    _exact(p, clamped, "clamp closed form")
    assert not c.any()
    for iters in (1, 10):
        _vs_oracle(device, rays, pts, p0, iters, M.LAMBDA, M.THRESH, f"p_init it{iters}")


@pytest.mark.parametrize("b", (1, 3))
@pytest.mark.parametrize("h,w", M.SMALL_SHAPES)
def test_iter_proj_small_and_nonsquare_images(device, h, w, b):
    rays, pts, p0 = M.iter_case(h, w, b, 300)
    p, _ = _vs_oracle(device, rays, pts, p0, 10, M.LAMBDA, M.THRESH, f"{h}x{w} b{b}")
    if (h, w) == (3, 3):
        assert (p == 1).all()


@pytest.mark.parametrize("n", M.N_GRID)
def test_iter_proj_any_number_of_points(device, n):
    """n independent of h*w on an 8x9 image, b = 3: grids of 1, 2, 7, 8, 9, 15 and 17 blocks through the XCD remap, every
    point written once and right."""
    rays, pts, p0 = M.iter_case(8, 9, 3, n, seed=n)
    _vs_oracle(device, rays, pts, p0, 10, M.LAMBDA, M.THRESH, f"n{n}")


def test_iter_proj_pinhole_ground_truth(device):
    """Sub-pixel positions drawn on an analytic pinhole ray image are found again to three times what the bilinear model
    costs the oracle (matching_refs.PINHOLE_MEASURED), and every point converges."""
    rays, pts, p0, drawn = M.pinhole_case()
    p, c = _fetch(*_iter_proj(device, rays, pts, p0, 10, 1e-8, 1e-6, "pinhole"))
    err = np.hypot(p[..., 0] - drawn[..., 0], p[..., 1] - drawn[..., 1]).max()
    print(f"pinhole: max distance {err:.3e} px")
    assert err <= M.PINHOLE_BOUND
    assert (c == 1).all()


def test_iter_proj_warped_ground_truth(device):
    """The same on a ray image whose gradient changes eleven-fold across the image, from starts up to 16 px on the steep
    side: met only if an accepted trial hands its gradient on (a stale gradient leaves 0.3 px, matching_refs.lm64)."""
    rays, pts, p0, drawn = M.warped_case()
    p, c = _fetch(*_iter_proj(device, rays, pts, p0, 10, 1e-8, 1e-6, "warped"))
    err = np.hypot(p[..., 0] - drawn[..., 0], p[..., 1] - drawn[..., 1]).max()
    print(f"warped: max distance {err:.3e} px")
    assert err <= M.WARPED_BOUND
    assert (c == 1).all()


def test_iter_proj_empty_and_argument_errors(device):
    m = _m()
    rays, pts, p0 = M.iter_case(8, 9, 3, 40)
    bufs = {"rays": _g(device, rays), "pts": _g(device, pts), "p_init": _g(device, p0),
            "p_new": R.Guarded(device, torch.float32, (3, 40, 2)), "converged": R.Guarded(device, torch.uint8, (3, 40))}

    def call(b=3, h=8, w=9, n=40, iters=10, null=None):
        a = [0 if k == null else _p(bufs[k]) for k in ("rays", "pts", "p_init", "p_new", "converged")]
        return m.lib().mslam_iter_proj(*a, b, h, w, n, iters, M.LAMBDA, M.THRESH, m.stream_ptr())

    assert call(b=0) == 0 and call(n=0) == 0
    for kw in (dict(h=2), dict(w=2), dict(n=-1), dict(b=-1), dict(iters=-1), dict(null="p_new"), dict(null="rays")):
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    assert _untouched(bufs["p_new"]) and _untouched(bufs["converged"])
    R.check_guards(bufs, [], "iter_proj refused calls")


# ---- 3. match_occlusion ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", M.OCC_SHAPES)
def test_match_occlusion(device, h, w):
    """Ragged h*w (255, 259), b = 3, u > h, fractions .0 and .999: p1 exact; valid against float64 with every unplanted
    distance at least 1e-3 from the threshold, the planted |d| == thresh invalid and the float32 below it valid, NaN
    invalid, and what came in invalid stays invalid."""
    m = _m()
    d = M.occlusion_case(h, w)
    bufs = {"X11": _g(device, d["X11"]), "X21": _g(device, d["X21"]), "p": _g(device, d["p"]),
            "p1": R.Guarded(device, torch.int64, (3, h * w, 2)), "valid": _g(device, d["valid_in"])}
    rc = m.lib().mslam_match_occlusion(_p(bufs["X11"]), _p(bufs["X21"]), _p(bufs["p"]), _p(bufs["p1"]), _p(bufs["valid"]),
                                       3, h, w, M.OCC_THRESH, m.stream_ptr())
    m.check(rc, "match_occlusion")
    R.check_guards(bufs, ["p1"], f"match_occlusion {h}x{w}")
    p1, valid = _fetch(bufs["p1"].t, bufs["valid"].t)
    _exact(p1, d["p1"], "p1")
    _exact(valid[d["planted"]], d["valid"][d["planted"]], "planted threshold decisions")
    _exact(valid, d["valid"], "valid")
    assert m.lib().mslam_match_occlusion(_p(bufs["X11"]), _p(bufs["X21"]), _p(bufs["p"]), 0, _p(bufs["valid"]), 3, h, w,
                                         M.OCC_THRESH, m.stream_ptr()) != 0
    assert m.lib().mslam_match_occlusion(_p(bufs["X11"]), _p(bufs["X21"]), _p(bufs["p"]), _p(bufs["p1"]), _p(bufs["valid"]),
                                         0, h, w, M.OCC_THRESH, m.stream_ptr()) == 0


# ---- 4. refine_matches -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fdim", M.TRAP_FDIMS)
def test_refine_traps(device, fdim):
    """Closed forms on the unrolled (24) and the generic (40) path: scan order and strict `>`, the sequential half sum,
    unfused products, half subnormals, the 2^-14 threshold, +-inf and NaN scores."""
    traps = M.refine_traps(fdim)
    outs = [_refine(device, t["D11"], t["D21"], t["p1"], t["radius"], t["dil"], t["name"]) for t in traps]
    got = _fetch(*outs)
    bad = [f"{t['name']}: {g[0, 0].astype(int).tolist()} instead of {t['expect'][0, 0].tolist()}"
           for t, g in zip(traps, got) if not np.array_equal(g, t["expect"])]
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("fdim", M.REFINE_FDIMS)
def test_refine_random_against_oracle(device, fdim):
    """fdim 0 and 1, the odd 7, the unrolled 16 and 24, the generic 8, 32, 40; radius or dilation_max of 0; n = 1 and 257
    with b = 3; normal descriptors and descriptors whose scores tie in half (more than 1 % of the points)."""
    cases, outs = [], []
    for kind in M.REFINE_KINDS:
        for n in M.REFINE_N:
            D11, D21, p1 = M.refine_random(fdim, n, kind)
            for radius, dil in M.REFINE_RD:
                cases.append((f"f{fdim} {kind} n{n} r{radius} d{dil}", oracle.refine_matches(D11, D21, p1, radius, dil), p1,
                              fdim == 0 or dil == 0))
                outs.append(_refine(device, D11, D21, p1, radius, dil, cases[-1][0]))
    for (what, ref, p1, unchanged), got in zip(cases, _fetch(*outs)):
        _exact(got, ref, what)
        if unchanged:
            _exact(got, p1, what + " unchanged")


def test_refine_start_outside_the_image(device):
    D11, D21, p1 = M.refine_outside()
    (got,) = _fetch(_refine(device, D11, D21, p1, *M.OUTSIDE_RD, "outside"))
    _exact(got, oracle.refine_matches(D11, D21, p1, *M.OUTSIDE_RD), "outside")
    assert got[0, 4].tolist() == [-40, -40]


def test_refine_empty_and_argument_errors(device):
    m = _m()
    D11, D21, p1 = M.refine_random(24, 257, "normal")
    bufs = {"D11": _g(device, D11), "D21": _g(device, D21), "p1": _g(device, p1),
            "p1_new": R.Guarded(device, torch.int64, (3, 257, 2))}

    def call(b=3, n=257, f=24, null=None):
        a = [0 if k == null else _p(bufs[k]) for k in ("D11", "D21", "p1", "p1_new")]
        return m.lib().mslam_refine_matches(*a, b, 9, 11, n, f, 3, 5, m.stream_ptr())

    assert call(b=0) == 0 and call(n=0) == 0
    for kw in (dict(n=-1), dict(b=-1), dict(f=-1), dict(null="p1_new"), dict(null="D11")):
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    assert _untouched(bufs["p1_new"])
    R.check_guards(bufs, [], "refine_matches refused calls")


# ---- 5. pixel_to_lin and the Python layer ----------------------------------------------------------------------------
@pytest.mark.parametrize("b,n", [(1, 1), (1, 255), (1, 257), (3, 85), (257, 1)])
def test_pixel_to_lin_guarded(device, b, n):
    m = _m()
    rng = np.random.default_rng(b * 1000 + n)
    w = 70001
    p1 = np.stack((rng.integers(0, w, (b, n)), rng.integers(0, 1 << 20, (b, n))), -1).astype(np.int64)
    p1[0, 0] = (w - 1, 70000)                   # w * v beyond 2^32
    bufs = {"p1": _g(device, p1), "idx": R.Guarded(device, torch.int64, (b, n))}
    m.check(m.lib().mslam_pixel_to_lin(_p(bufs["p1"]), _p(bufs["idx"]), b, n, w, m.stream_ptr()), "pixel_to_lin")
    R.check_guards(bufs, ["idx"], f"pixel_to_lin {b}x{n}")
    want = p1[..., 0] + w * p1[..., 1]
    assert want[0, 0] > 2 ** 32
    assert torch.equal(bufs["idx"].t.cpu(), torch.from_numpy(want))
    assert m.lib().mslam_pixel_to_lin(_p(bufs["p1"]), _p(bufs["idx"]), 0, n, w, m.stream_ptr()) == 0
    assert m.lib().mslam_pixel_to_lin(_p(bufs["p1"]), 0, b, n, w, m.stream_ptr()) != 0


def test_pixel_to_lin_leading_shapes_and_round_trip(device):
    from mast3r_slam import matching

    rng = np.random.default_rng(3)
    w, h = 19, 17
    for shape in ((255,), (3, 85), (3, 1, 85), (1,), (257,)):
        p = np.stack((rng.integers(0, w, shape), rng.integers(0, h, shape)), -1).astype(np.int64)
        t = torch.from_numpy(p).to(device)
        idx = matching.pixel_to_lin(t, w)
        assert idx.shape == shape and idx.dtype == torch.int64
        back = matching.lin_to_pixel(idx, w)
        assert torch.equal(idx.cpu(), torch.from_numpy(p[..., 0] + w * p[..., 1])) and torch.equal(back, t)


def test_match_against_the_oracle_on_its_own_prep(device):
    """matching.match with b = 3 at 17x19, a starting index map, X11 / X21 / D11 as permuted views and a float32 D21,
    against the oracle chain on the ORACLE's prep.  The two preps differ by rounding, which can flip an integer step; a
    point is compared where the oracle chain gives the same index and flag on both preps (its own and the kernel's,
    fetched from the device), and at most 2 % of the points may be left out."""
    from mast3r_slam import matching
    from mast3r_slam.config import config
    from oracle import matching_py

    d = M.match_case()
    cfg = config["matching"]
    view = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2))).to(device).permute(0, 2, 3, 1)
    X11, X21, D11 = view(d["X11"]), view(d["X21"]), view(d["D11"])
    assert not X11.is_contiguous() and not D11.is_contiguous()
    D21 = torch.from_numpy(d["D21"]).to(device)
    assert D21.dtype == torch.float32
    idx0 = torch.from_numpy(d["idx"]).to(device)
    idx, valid = matching.match(X11, X21, D11, D21, idx0)
    h, w = M.MATCH_HW
    assert idx.shape == (3, h * w) and valid.shape == (3, h * w, 1) and valid.dtype == torch.bool
    k_prep = [t.cpu().numpy() for t in matching.prep_for_iter_proj(X11, X21, idx0)]
    i_o, v_o = M.oracle_chain(d, matching_py.prep_for_iter_proj(d["X11"], d["X21"], d["idx"]), cfg)
    i_k, v_k = M.oracle_chain(d, k_prep, cfg)
    keep = (i_o == i_k) & (v_o == v_k)
    print(f"match: {1 - keep.mean():.4f} of the points left out")
    assert 1 - keep.mean() <= M.MATCH_LEFT_OUT
    idx, valid = idx.cpu().numpy(), valid.cpu().numpy()[..., 0]
    _exact(idx[keep], i_o[keep], "idx")
    _exact(valid[keep], v_o[keep], "valid")
    assert v_o.mean() > 0.2
