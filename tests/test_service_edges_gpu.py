"""GPU tests (-m gpu) of the service kernels around the network at the edges of their tiles, waves and chunks:
csrc/retrieval.hip (mslam_gemm_f64, mslam_asmk_aggregate, mslam_asmk_search), csrc/quality.hip
(mslam_quality_reduce_grid, mslam_quality_classify) and csrc/tsdf_local.hip (mslam_tsdf_local_build / _raycast), each
against the CPU statement in tests/service_refs.py (checked on its own in tests/test_service_refs_cpu.py).

The kernels are called through mslam_hip like the product's wrappers call them, so that every operand can live in a guarded
buffer (kernel_refs.Guarded): the guards in front and behind must come back bit-identical and no output element may be
left unwritten.  Where a product wrapper reaches the case it is run as well and must return the same bits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R  # noqa: E402
import service_refs as S  # noqa: E402

pytestmark = pytest.mark.gpu

# Largest relative deviation of the alpha = 2.0 / 2.5 scores from the float64-pow reference measured on the MI355X
# (test_asmk_search_powf prints it); the test asserts four times that, and never more than 16 ulp of float32.
POWF_MEASURED = 9.03e-8
POWF_BOUND = min(4 * POWF_MEASURED, 16 * 2.0 ** -23)


def _m():
    import mslam_hip as m

    return m


def _t(a):
    """numpy / torch -> torch; uint32 as the int32 of the same bits, bool as uint8."""
    if isinstance(a, np.ndarray):
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        a = torch.from_numpy(np.ascontiguousarray(a))
    return a.to(torch.uint8) if a.dtype == torch.bool else a


def _g(device, a):
    a = _t(a)
    return R.Guarded(device, a.dtype, src=a)


def _p(g):
    return 0 if g is None else _m().ptr(g.t)


def _same(got, want):
    """Bit-for-bit up to the NaN payload: NaN where the reference is NaN, equal elsewhere (+-inf included)."""
    got, want = got.cpu(), want.cpu()
    z = torch.zeros_like(want)
    return torch.equal(got.isnan(), want.isnan()) and torch.equal(torch.where(want.isnan(), z, got),
                                                                  torch.where(want.isnan(), z, want))


# ---- 1. mslam_gemm_f64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.gemm_cases(), ids=lambda c: "x".join(map(str, c[:3])) + "-" + "".join(map(str, c[3:])))
def test_gemm_f64_exact(device, case):
    """Operands on the 2^-12 grid: every product and partial sum is exact in float64, so the int64 result must come back
    bit for bit - partial row, column and K tiles, each operand type pair, both layouts of B, centre and bias or NULL."""
    from mast3r_slam.retrieval_database import _gemm_f64

    m = _m()
    M, N, K, a32, b32, bt, cen, bias = case
    d = S.gemm_exact(case)
    bufs = {"A": _g(device, d["A"]), "B": _g(device, d["B"]), "out": R.Guarded(device, torch.float64, (M, N))}
    if cen:
        bufs["centre"] = _g(device, d["centre"])
    if bias:
        bufs["bias"] = _g(device, d["bias"])
    rc = m.lib().mslam_gemm_f64(_p(bufs["A"]), a32, _p(bufs["B"]), b32, bt, _p(bufs.get("centre")), _p(bufs.get("bias")),
                                _p(bufs["out"]), M, N, K, m.stream_ptr())
    m.check(rc, "gemm_f64")
    got = bufs["out"].t.cpu()
    if not torch.equal(got, d["ref"]):
        bad = (got != d["ref"]).nonzero()
        r, c = bad[0].tolist()
        raise AssertionError(f"{len(bad)} wrong elements, first at ({r}, {c}): {float(got[r, c])!r} != {float(d['ref'][r, c])!r}")
    w = _gemm_f64(bufs["A"].t, bufs["B"].t, bt, centre=bufs["centre"].t if cen else None,
                  bias=bufs["bias"].t if bias else None)
    assert torch.equal(w.cpu(), d["ref"])
    R.check_guards(bufs, ["out"], f"gemm_f64 {case}")


# ---- 2. mslam_asmk_aggregate -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", S.ASMK_DIMS)
def test_asmk_aggregate_signatures(device, dim):
    """Signatures bit for bit against the sequential float32 loop: 1, 2, 3 (odd: the upper half of a ballot is dropped) and
    5 words, a second pass of the dimension loop with 32 and with 288 live lanes, 1 / 255 / 257 / 700 descriptors, single
    and five-fold assignment (a word named twice counts once).  The planted columns of service_refs.planted_columns give
    another bit under any other summation order."""
    m = _m()
    for n_des in S.ASMK_NDES:
        for ma in S.ASMK_M:
            d = S.asmk_aggregate_inputs(dim, n_des, ma)
            want, _, uniq = S.asmk_aggregate_ref(d["des"], d["cent"], d["codes"])
            U, W = want.shape
            bufs = {k: _g(device, d[k]) for k in ("des", "cent", "codes", "uniq")}
            bufs["sig"] = R.Guarded(device, torch.int32, (U, W))
            rc = m.lib().mslam_asmk_aggregate(_p(bufs["des"]), _p(bufs["cent"]), _p(bufs["codes"]), _p(bufs["uniq"]),
                                              _p(bufs["sig"]), n_des, ma, dim, U, S.ASMK_NCENT, m.stream_ptr())
            what = f"asmk_aggregate dim {dim} n_des {n_des} m {ma}"
            m.check(rc, what)
            got = bufs["sig"].t.cpu().numpy().view(np.uint32)
            if not np.array_equal(got, want):
                u, w = np.argwhere(got != want)[0]
                diff = int(got[u, w] ^ want[u, w])
                col = 32 * w + 31 - (diff.bit_length() - 1)
                raise AssertionError(f"{what}: {np.count_nonzero(got != want)} wrong words, first: word id {uniq[u]}, "
                                     f"dimension {col} (planted: {S.planted_columns(dim)})")
            R.check_guards(bufs, ["sig"], what)


# ---- 3. mslam_asmk_search --------------------------------------------------------------------------------------------
def _search(device, m, f, q_words, q_sig, alpha, thr, what):
    n_img = len(f["img_start"]) - 1
    bufs = {"e_word": _g(device, f["e_word"]), "e_sig": _g(device, f["e_sig"]), "img_start": _g(device, f["img_start"]),
            "q_words": _g(device, q_words), "q_sig": _g(device, q_sig),
            "scores": R.Guarded(device, torch.float64, (n_img,))}
    rc = m.lib().mslam_asmk_search(_p(bufs["e_word"]), _p(bufs["e_sig"]), _p(bufs["img_start"]), n_img, _p(bufs["q_words"]),
                                   _p(bufs["q_sig"]), len(q_words), q_sig.shape[1], float(thr), float(alpha),
                                   _p(bufs["scores"]), m.stream_ptr())
    m.check(rc, what)
    R.check_guards(bufs, ["scores"], what)
    return bufs["scores"].t.cpu().numpy()


@pytest.mark.parametrize("W", S.SEARCH_W)
def test_asmk_search_scores(device, W):
    """Images of 0, 1, 255, 256, 257 and 600 entries (the 256-entry chunk of the block loop), scalar (W = 1, 2, 3, 5) and
    uint4 (W = 4, 8, 32) popcount, 1 / 7 / 300 query words of which a quarter is absent, against the oracle's IVF.search at
    the bar of test_retrieval_gpu; one entry dropped or counted twice moves a score by more than 100 times that bar."""
    m = _m()
    f = S.search_file(W)
    for n_q in S.SEARCH_NQ:
        q_words, q_sig = S.search_query(W, n_q)
        for thr in (0.0, -1.0):
            want = S.search_oracle(f["e_word"], f["e_sig"], f["img_start"], q_words, q_sig, 3.0, thr)
            got = _search(device, m, f, q_words, q_sig, 3.0, thr, f"asmk_search W {W} n_q {n_q} thr {thr}")
            np.testing.assert_allclose(got, want, rtol=S.SEARCH_RTOL, atol=S.SEARCH_ATOL)
            assert got[1] == 0.0 and got[-1] == 0.0                                   # the empty images
            assert n_q < 300 or np.count_nonzero(got) == len(got) - 2


@pytest.mark.parametrize("W", S.SEARCH_W)
def test_asmk_search_gate_is_exact(device, W):
    """One-entry images at Hamming counts 12 W, 12 W + 1, 20 W: sim == threshold (0.25) takes part with 0.25^3 exactly,
    the next count does not; with threshold -1 a negative sim keeps its sign through the cube."""
    m = _m()
    g = S.gate_file(W)
    got = _search(device, m, g, g["q_words"], g["q_sig"], 3.0, 0.25, f"asmk_search gate W {W}")
    np.testing.assert_array_equal(got, [0.25 ** 3, 0.0, 0.0])
    got = _search(device, m, g, g["q_words"], g["q_sig"], 3.0, -1.0, f"asmk_search gate W {W} thr -1")
    want = S.search_oracle(g["e_word"], g["e_sig"], g["img_start"], g["q_words"], g["q_sig"], 3.0, -1.0)
    assert got[0] == 0.25 ** 3 and got[2] == -0.25 ** 3
    np.testing.assert_allclose(got, want, rtol=S.SEARCH_RTOL, atol=S.SEARCH_ATOL)


def test_asmk_search_powf(device, capsys):
    """alpha = 2.0 and 2.5 (powf instead of the cube) against float64 pow of the float32 sim, thresholds 0 and 0.25.
    Measured on the MI355X: largest relative deviation of a score 9.03e-8 (0.76 ulp of float32; powf plus the two
    roundings of a contribution to float32); asserted: four times that, 3.6e-7, itself capped at 16 ulp of float32
    (1.9e-6), so that a wrong exponent or base fails (alpha 2 against 2.5 moves a score by tens of percent) and a library
    update does not."""
    m = _m()
    worst = 0.0
    for W in S.SEARCH_W:
        f = S.search_file(W)
        q_words, q_sig = S.search_query(W, 300)
        for alpha in (2.0, 2.5):
            for thr in (0.0, 0.25):
                want, _ = S.search_pow64(f["e_word"], f["e_sig"], f["img_start"], q_words, q_sig, alpha, thr)
                got = _search(device, m, f, q_words, q_sig, alpha, thr, f"asmk_search W {W} alpha {alpha} thr {thr}")
                nz = want != 0
                assert np.array_equal(got != 0, nz) and nz.sum() >= 4
                worst = max(worst, float(np.max(np.abs(got[nz] - want[nz]) / want[nz])))
    with capsys.disabled():
        print(f"\n[asmk_search powf] largest relative deviation {worst:.3e}, asserted bound {POWF_BOUND:.3e}")
    assert POWF_BOUND <= 16 * 2.0 ** -23
    assert worst <= POWF_BOUND, (worst, POWF_BOUND)


# ---- 4. mslam_quality_reduce_grid ------------------------------------------------------------------------------------
def _reduce(device, m, x, y, valid, h, w, ps, mode, what):
    bufs = {"x": _g(device, x), "out": R.Guarded(device, torch.float32, (h // ps, w // ps))}
    if y is not None:
        bufs["y"] = _g(device, y)
    if valid is not None:
        bufs["valid"] = _g(device, valid)
    rc = m.lib().mslam_quality_reduce_grid(_p(bufs["x"]), _p(bufs.get("y")), _p(bufs.get("valid")), h, w, ps, mode,
                                           S.C_THR, S.Q_THR, _p(bufs["out"]), m.stream_ptr())
    m.check(rc, what)
    R.check_guards(bufs, ["out"], what)
    return bufs["out"].t.cpu()


def _check_reduce(device, d, ps, key):
    """All three modes on x / C / Q (`key` = "" or "_nan"), without and with the mask; every comparison is made before
    the first one is reported."""
    m = _m()
    h, w = d["h"], d["w"]
    x, C, Q = d["x" + key], d["C" + key], d["Q" + key]
    bad = []
    for valid in (None, d["valid"]):
        what = f"reduce_grid ps {ps} {h}x{w} {'nan' if key else 'plain'} mask {valid is not None}"
        got = _reduce(device, m, x, None, valid, h, w, ps, 0, what + " median")
        want = S.reduce_median_ref(x, ps, valid)
        if not _same(got, want):
            bad.append(f"{what} median:\n{got}\n{want}")
        got = _reduce(device, m, x, None, valid, h, w, ps, 1, what + " mean")
        mean, bound = S.reduce_mean_ref(x, ps, valid)
        exact, zero = bound == 0, torch.zeros_like(mean)
        err = torch.where(exact, zero, (got.double() - mean).abs())
        if not _same(torch.where(exact, got.double(), zero), torch.where(exact, mean, zero)) or not (err <= bound).all():
            bad.append(f"{what} mean:\n{got}\n{mean}\nerror {err}\nbound {bound}")
    got = _reduce(device, m, C, Q, None, h, w, ps, 2, f"reduce_grid ps {ps} u")
    want = S.reduce_u_ref(C, Q, ps)
    if not torch.equal(got.isnan(), want.isnan()) or not bool(((got - want).nan_to_num(0.0).abs() <= 6e-8).all()):
        bad.append(f"reduce_grid ps {ps} {'nan' if key else 'plain'} u:\n{got}\n{want}")
    assert not bad, "\n".join(bad)
    return got


@pytest.mark.parametrize("ps", S.REDUCE_PS + ("14x42x56",))
def test_reduce_grid_edges(device, ps):
    """ps 1 ... 32 on (3 ps + 1) x (2 ps + ps / 2) images (cropped rows and columns, patch stride != row length) and ps 14
    on 42 x 56: blocks wider than the patch (ps < 8), the padded bitonic sort (ps 3, 5, 14, 31), 1024 threads (ps 32).
    Random values with +-inf at valid pixels; masks with 0, 1, 2, 3 and all pixels valid.  Median exact, u to one ulp of
    the root (6e-8), mean within (log2 1024 + 2) 2^-24 sum|x| / denom of the float64 mean."""
    from mast3r_slam import quality_core as qc

    hw = None
    if isinstance(ps, str):
        ps, hw = 14, (42, 56)
    d = S.reduce_inputs(ps, hw)
    u = _check_reduce(device, d, ps, "")
    t = lambda a: a.to(device)
    h, w = d["h"], d["w"]
    assert _same(qc.reduce_grid(t(d["x"]), h, w, ps, valid=t(d["valid"])), S.reduce_median_ref(d["x"], ps, d["valid"]))
    assert torch.equal(qc.u_from_CQ(t(d["C"]), t(d["Q"]), S.C_THR, S.Q_THR, h, w, ps).cpu(), u)


@pytest.mark.parametrize("ps", S.REDUCE_PS)
def test_reduce_grid_nan_follows_the_reference(device, ps):
    """NaN at valid pixels.  Without a mask the reference applies no nan_to_num: the median of an all-NaN patch is NaN and
    the mean over a NaN is NaN; u ignores a pixel whose C or Q is NaN (torch.clamp keeps NaN, nanmedian skips it) and an
    all-NaN patch gives NaN.  With a mask NaN pixels are skipped and an empty patch gives 0."""
    d = S.reduce_inputs(ps)
    _check_reduce(device, d, ps, "_nan")


def test_reduce_grid_limits(device):
    from mast3r_slam import quality_core as qc

    m = _m()
    x = torch.zeros(66, 66, device=device)
    out = R.Guarded(device, torch.float32, (2, 2))
    rc = m.lib().mslam_quality_reduce_grid(m.ptr(x), 0, 0, 66, 66, 33, 0, 0.0, 0.0, _p(out), m.stream_ptr())
    with pytest.raises(RuntimeError, match="patch 33 x 33 exceeds 1024 pixels"):
        m.check(rc, "quality_reduce_grid")
    R.check_guards({"out": out}, [], "reduce_grid ps 33")
    assert not bool((out.raw != out.pat).any())                          # rejected, not launched
    assert qc.reduce_grid(x[:7], 7, 66, 8).shape == (0, 8)               # h < ps: an empty grid
    assert qc.reduce_grid(x[:, :7].contiguous(), 66, 7, 8, method="mean").shape == (8, 0)


# ---- 5. mslam_quality_classify ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.CLASSIFY_N)
def test_classify_edges(device, n):
    """1, 2, 3 patches, 48, and around and above the 1024 threads of the block (several elements per thread, up to the
    cap): random input, four-level input whose MAD is 0 (z = (x - m) / 1e-6), constant input (all classes and priorities
    0), delta_cov with values exactly at the threshold.  Classes exact, priorities rtol 1e-6 / atol 1e-7."""
    from mast3r_slam import quality_core as qc

    m = _m()
    for kind in S.CLASSIFY_KINDS:
        dc, r, u = S.classify_inputs(n, kind)
        want_c, want_p = S.classify_ref(dc, r, u)
        bufs = {"dc": _g(device, dc), "r": _g(device, r), "u": _g(device, u),
                "cls": R.Guarded(device, torch.int64, (n,)), "pri": R.Guarded(device, torch.float32, (n,))}
        rc = m.lib().mslam_quality_classify(_p(bufs["dc"]), _p(bufs["r"]), _p(bufs["u"]), n, S.THR_ZR, S.THR_ZU, S.THR_DC,
                                            _p(bufs["cls"]), _p(bufs["pri"]), m.stream_ptr())
        what = f"classify n {n} {kind}"
        m.check(rc, what)
        R.check_guards(bufs, ["cls", "pri"], what)
        got_c, got_p = bufs["cls"].t.cpu(), bufs["pri"].t.cpu()
        assert torch.equal(got_c, want_c), f"{what}: {(got_c != want_c).sum()} classes differ"
        np.testing.assert_allclose(got_p.numpy(), want_p.numpy(), rtol=1e-6, atol=1e-7, err_msg=what)
        if kind == "equal":
            assert not got_c.any() and not got_p.any()
        wc, wp = qc.classify(bufs["dc"].t, bufs["r"].t, bufs["u"].t, S.THR_ZR, S.THR_ZU, S.THR_DC)
        assert torch.equal(wc.cpu(), got_c) and torch.equal(wp.cpu(), got_p)


@pytest.mark.parametrize("n", (0, 4097))
def test_classify_rejects_sizes_outside_the_block(device, n):
    m = _m()
    x = torch.zeros(4097, device=device)
    cls, pri = R.Guarded(device, torch.int64, (4097,)), R.Guarded(device, torch.float32, (4097,))
    rc = m.lib().mslam_quality_classify(m.ptr(x), m.ptr(x), m.ptr(x), n, 1.0, 1.0, 0.02, _p(cls), _p(pri), m.stream_ptr())
    with pytest.raises(RuntimeError, match="outside 1..4096"):
        m.check(rc, "quality_classify")
    R.check_guards({"cls": cls, "pri": pri}, [], f"classify n {n}")
    assert not bool((cls.raw != cls.pat).any()) and not bool((pri.raw != pri.pat).any())


# ---- 6. local TSDF ---------------------------------------------------------------------------------------------------
CFG = dict(voxel_size=S.VOXEL, trunc_dist=S.TRUNC, max_grid_dim=64, roi_size=0.4, ray_samples=64,
           max_displacement=S.MAX_DISP, min_weight_threshold=0.01, confidence_boost=0.08, confidence_max=1.3,
           min_hit_rate=0.05, min_confidence=S.MIN_CONF)


class _WorldPose:
    """Pose whose act() returns the given world points and whose translation is the given camera centre."""
    def __init__(self, origin, Xw):
        self.data = torch.cat([origin, torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0], device=origin.device)]).reshape(1, 8)
        self._Xw = Xw

    def act(self, X):
        return self._Xw


@pytest.mark.parametrize("name", S.BUILD_CASES)
def test_local_build_edges(device, name):
    """nx != ny != nz grids against oracle/tsdf_refine_py.py (linspace="scalar") at the bars of test_build_and_raycast:
    touched set exact, weights rtol 1e-6 / atol 1e-7, TSDF atol 1e-6.  Cases: service_refs.build_inputs."""
    from mast3r_slam.tsdf_refine import TSDFRefiner

    m = _m()
    b = S.build_case(name)
    nx, ny, nz = b["dims"]
    n = len(b["Xw"])
    bufs = {k: _g(device, b[k]) for k in ("Xw", "C", "origin", "mn", "mx")}
    bufs["tsdf"] = R.Guarded(device, torch.float32, (nz, ny, nx))
    bufs["weights"] = R.Guarded(device, torch.float32, (nz, ny, nx))
    L = m.lib()
    ws = torch.empty(L.mslam_tsdf_local_workspace_bytes(n), dtype=torch.uint8, device=device)
    rc = L.mslam_tsdf_local_build(_p(bufs["Xw"]), _p(bufs["C"]), _p(bufs["origin"]), _p(bufs["mn"]), _p(bufs["mx"]), n, nx, ny,
                                  nz, S.VOXEL, S.TRUNC, S.MIN_CONF, _p(bufs["tsdf"]), _p(bufs["weights"]), m.ptr(ws),
                                  ws.numel(), m.stream_ptr())
    what = f"tsdf_local_build {name}"
    m.check(rc, what)
    R.check_guards(bufs, ["tsdf", "weights"], what)
    tsdf, weights = bufs["tsdf"].t.cpu().numpy(), bufs["weights"].t.cpu().numpy()
    np.testing.assert_array_equal(weights > 0, b["weights"] > 0)
    np.testing.assert_allclose(weights, b["weights"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(tsdf, b["tsdf"], rtol=0, atol=1e-6)
    if name == "four":
        assert (tsdf == 1).all() and (weights == 0).all()
    ref = TSDFRefiner(CFG, None, None, device)
    ref._grid_dims = lambda mn, mx: list(b["dims"])        # the oracle's grid: this test is about the kernels
    wt, ww = ref._build_tsdf_robust(bufs["Xw"].t, bufs["C"].t, None, bufs["mn"].t, bufs["mx"].t, 0, 0,
                                    _WorldPose(bufs["origin"].t, bufs["Xw"].t))
    assert np.array_equal(wt.cpu().numpy(), tsdf) and np.array_equal(ww.cpu().numpy(), weights)


@pytest.mark.parametrize("name", S.RAYCAST_CASES)
def test_local_raycast_edges(device, name):
    """Ray casts with both outcomes well populated (service_refs.raycast_inputs) against the oracle: hit flags exact,
    refined points atol 1e-6, and a ray that misses returns its original point bit for bit with hit = 0."""
    from mast3r_slam.tsdf_refine import TSDFRefiner

    m = _m()
    c = S.raycast_case(name)
    nz, ny, nx = c["vol"].shape
    n_sel = len(c["sel"])
    bufs = {"vol": _g(device, c["vol"]), "mn": _g(device, c["mn"]), "mx": _g(device, c["mx"]), "X": _g(device, c["X"]),
            "sel": _g(device, c["sel"]), "surf": R.Guarded(device, torch.float32, (n_sel, 3)),
            "hit": R.Guarded(device, torch.uint8, (n_sel,))}
    rc = m.lib().mslam_tsdf_local_raycast(_p(bufs["vol"]), nx, ny, nz, _p(bufs["mn"]), _p(bufs["mx"]), _p(bufs["X"]),
                                          _p(bufs["sel"]), n_sel, c["n_samples"], S.MAX_DISP, _p(bufs["surf"]),
                                          _p(bufs["hit"]), m.stream_ptr())
    what = f"tsdf_local_raycast {name}"
    m.check(rc, what)
    R.check_guards(bufs, ["surf", "hit"], what)
    surf, hit = bufs["surf"].t.cpu().numpy(), bufs["hit"].t.cpu().numpy()
    np.testing.assert_array_equal(hit, c["hit"].astype(np.uint8))
    np.testing.assert_allclose(surf, c["surf"], rtol=0, atol=1e-6)
    miss = hit == 0
    assert np.array_equal(surf[miss].view(np.int32), c["X"][c["sel"]][miss].view(np.int32))
    if c["n_samples"] == 64 and n_sel:
        ref = TSDFRefiner(CFG, None, None, device)
        n = len(c["X"])
        Xr, hits = ref._extract_surface_safe(bufs["vol"].t, bufs["mn"].t, bufs["mx"].t, None,
                                             torch.ones(n, dtype=torch.bool, device=device), 0, 0, bufs["X"].t,
                                             order=bufs["sel"].t)
        assert np.array_equal(Xr.cpu().numpy()[c["sel"]], surf) and np.array_equal(hits.cpu().numpy()[c["sel"]], hit == 1)
        rest = np.setdiff1d(np.arange(n), c["sel"])
        assert np.array_equal(Xr.cpu().numpy()[rest].view(np.int32), c["X"][rest].view(np.int32)) and not hits.cpu().numpy()[rest].any()
