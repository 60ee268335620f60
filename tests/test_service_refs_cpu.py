"""The references and input recipes of tests/service_refs.py on their own (no GPU): the exactness preconditions of the
fp64 GEMM inputs, the aggregation reference against the oracle and its order traps, the sensitivity of the search scores,
the four-class condition of the classification inputs, and the touched / hit rates of the local-TSDF cases."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import service_refs as S  # noqa: E402
from kernel_refs import NAN_BITS, SENTINEL  # noqa: E402
from oracle import asmk_py  # noqa: E402


# ---- GEMM ------------------------------------------------------------------------------------------------------------
def test_gemm_cases_cover_types_layouts_and_epilogues():
    cases = S.gemm_cases()
    assert {c[:3] for c in cases} == set(S.GEMM_SHAPES)
    for a32 in (0, 1):
        for b32 in (0, 1):
            mine = [c for c in cases if c[3:5] == (a32, b32)]
            assert {c[5] for c in mine} == {0, 1} and {c[6] for c in mine} == {0, 1} and {c[7] for c in mine} == {0, 1}


@pytest.mark.parametrize("case", S.gemm_cases(), ids=str)
def test_gemm_inputs_are_exact(case):
    """Operands exact in their storage type, every partial sum below 2^52 units, and float64 matmul in torch's own order
    reproduces the int64 result bit for bit."""
    M, N, K, a32, b32, bt, cen, bias = case
    d = S.gemm_exact(case)
    assert d["mag"] < 2 ** 52 and K <= 200
    assert d["A"].dtype == (torch.float32 if a32 else torch.float64) and d["A"].shape == (M, K)
    assert d["B"].shape == ((N, K) if bt else (K, N))
    A, B = d["A"].double(), d["B"].double()
    assert torch.equal(A * 4096, (A * 4096).round()) and float(A.abs().max()) <= 8.0
    x = (A - d["centre"]) if cen else A
    y = x @ (B.T if bt else B)
    if bias:
        y = y + d["bias"]
    assert torch.equal(y, d["ref"])


# ---- ASMK aggregation ------------------------------------------------------------------------------------------------
def test_aggregate_ref_equals_the_oracle_on_the_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "retrieval_asmk.npz"))
    for i in (1, 5, 11):
        des, codes = g[f"local_{i}"], g[f"topk_{i}"]
        for m in (1, 5):
            sig, _, uniq = S.asmk_aggregate_ref(des, g["centroids"], codes[:, :m])
            o_sig, o_uniq = asmk_py.aggregate_image(des, codes[:, :m], g["centroids"])
            np.testing.assert_array_equal(uniq, o_uniq)
            np.testing.assert_array_equal(sig, o_sig)


def test_order_traps_separate_the_sequential_sum_from_the_others():
    seq, pair, f64 = S.sum_sequential_f32, S.sum_pairwise_f32, lambda v: float(np.sum(np.array(v, np.float64)))
    rev = lambda v: S.sum_sequential_f32(v[::-1])
    assert seq(S.TRAP25) == 0.0 and f64(S.TRAP25) == 1.0          # a + (b + c) also gives 0 here: 1 - 2^25 is a tie
    assert seq(S.TRAP24) == 0.0 and pair(S.TRAP24) == 1.0 and f64(S.TRAP24) == 1.0 and rev(S.TRAP24) == 1.0
    a, b, c = S.TRAP24
    assert float(np.float32(np.float32(a + c) + np.float32(b))) == 1.0
    assert seq(S.TRAP_OPP) == 1.0 and pair(S.TRAP_OPP) == 0.0 and f64(S.TRAP_OPP) == 0.0 and rev(S.TRAP_OPP) == 0.0


@pytest.mark.parametrize("m", S.ASMK_M)
@pytest.mark.parametrize("dim", (96, 288))
def test_aggregate_inputs_plant_what_they_promise(dim, m):
    for n_des in S.ASMK_NDES:
        d = S.asmk_aggregate_inputs(dim, n_des, m)
        sig, ades, uniq = S.asmk_aggregate_ref(d["des"], d["cent"], d["codes"])
        assert sig.shape == (len(uniq), dim // 32) and sig.dtype == np.uint32
        row = int(np.nonzero(uniq == S.TRAP_WORD)[0][0])
        bit = lambda col: int(sig[row, col // 32] >> (31 - col % 32)) & 1
        if n_des < 4:
            assert not sig[row].any()
            continue
        cols = S.planted_columns(dim)
        for name, (col, want) in cols.items():
            assert bit(col) == want, name
        # the same columns summed another way give other bits
        members = np.nonzero((d["codes"] == S.TRAP_WORD).any(1))[0]
        res = lambda col: list((d["des"][members, col] - d["cent"][S.TRAP_WORD, col]).astype(np.float64))
        assert np.sum(res(cols["trap25"][0])) > 0 and np.sum(res(cols["trap24"][0])) > 0 and np.sum(res(cols["opp"][0])) <= 0
        assert S.sum_pairwise_f32(res(cols["opp"][0])) <= 0
        assert S.sum_sequential_f32(res(cols["trap24"][0])[::-1]) > 0
        assert np.array_equal(ades[row, [c for c, _ in cols.values()]], np.array([0, 0, 0, 0, 1], np.float32))
        counts = np.array([(d["codes"] == w).any(1).sum() for w in uniq])
        assert counts.min() == 1 and counts.max() >= n_des // 3 and uniq[-1] == S.LONE_WORD
        if m == 5:
            assert (np.sort(d["codes"], 1)[:, 1:] == np.sort(d["codes"], 1)[:, :-1]).any(1).sum() > n_des // 2


# ---- ASMK search -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", S.SEARCH_W)
def test_search_scores_notice_every_single_entry(W):
    """The explicit statement of the contract agrees with the oracle, and taking any one contributing entry away moves
    its image's score by more than 100 times the tolerance of the comparison."""
    f = S.search_file(W)
    args = (f["e_word"], f["e_sig"], f["img_start"])
    assert np.diff(f["img_start"]).tolist() == list(S.SEARCH_ENTRIES)
    for s, e in zip(f["img_start"][:-1], f["img_start"][1:]):
        assert (np.diff(f["e_word"][s:e]) > 0).all()
    for n_q in S.SEARCH_NQ:
        q_words, q_sig = S.search_query(W, n_q)
        assert (np.diff(q_words) > 0).all() and (n_q < 4 or (q_words >= S.SEARCH_VOCAB).any())
        want = S.search_oracle(*args, q_words, q_sig, 3.0, 0.0)
        ok, sim = S.search_terms(*args, q_words, q_sig, 0.0)
        match, _ = S.search_terms(*args, q_words, q_sig, -1.0)
        assert ok.any() and (n_q < 300 or (match & ~ok).any())          # some asked-for entries fall below the threshold
        mine, contrib = S.search_pow64(*args, q_words, q_sig, 3.0, 0.0)
        np.testing.assert_allclose(mine, want, rtol=S.SEARCH_RTOL, atol=S.SEARCH_ATOL)
        img = np.repeat(np.arange(len(want)), np.diff(f["img_start"]))
        tol = S.SEARCH_ATOL + S.SEARCH_RTOL * np.abs(want[img])
        assert (np.abs(contrib[ok]) > 100 * tol[ok]).all()
        for k in np.nonzero(ok)[0][[0, -1]]:                             # and for real, through the oracle
            keep = np.arange(len(img)) != k
            start = np.concatenate(([0], np.cumsum(np.bincount(img[keep], minlength=len(want))))).astype(np.int32)
            less = S.search_oracle(f["e_word"][keep], f["e_sig"][keep], start, q_words, q_sig, 3.0, 0.0)
            assert abs(less[img[k]] - want[img[k]]) > 100 * tol[k]
            others = np.arange(len(want)) != img[k]
            np.testing.assert_array_equal(less[others], want[others])


@pytest.mark.parametrize("W", S.SEARCH_W)
def test_search_gate_values_are_exact(W):
    g = S.gate_file(W)
    args = (g["e_word"], g["e_sig"], g["img_start"], g["q_words"], g["q_sig"])
    cnt = S.popcount32(g["e_sig"] ^ g["q_sig"])
    assert cnt.tolist() == [12 * W, 12 * W + 1, 20 * W]
    np.testing.assert_array_equal(S.search_oracle(*args, 3.0, 0.25), [0.25 ** 3, 0.0, 0.0])
    low = S.search_oracle(*args, 3.0, -1.0)
    assert low[0] == 0.25 ** 3 and low[2] == -0.25 ** 3 and 0 < low[1] < low[0]


# ---- quality: patch statistics ---------------------------------------------------------------------------------------
def test_guard_patterns_are_what_no_kernel_writes():
    for dt, bits in NAN_BITS.items():
        x = torch.tensor([bits], dtype={2: torch.int16, 4: torch.int32, 8: torch.int64}[torch.empty((), dtype=dt).element_size()])
        assert x.view(dt).isnan().all()
    assert SENTINEL[torch.uint8] > 1 and SENTINEL[torch.int64] > 3


@pytest.mark.parametrize("ps", S.REDUCE_PS)
def test_reduce_inputs_hold_the_promised_patches(ps):
    d = S.reduce_inputs(ps)
    h, w = d["h"], d["w"]
    assert (h, w) == (3 * ps + 1, 2 * ps + ps // 2)
    n = ps * ps
    cnt = S.grid_view(d["valid"].float(), ps).sum(-1).flatten().long().tolist()
    assert cnt[:5] == [min(p, n) for p in range(4)] + [n]
    med, medm = S.reduce_median_ref(d["x"], ps), S.reduce_median_ref(d["x"], ps, d["valid"])
    assert med.shape == (h // ps, w // ps) and not med.isnan().any() and medm.flatten()[0] == 0
    if ps > 1:
        assert medm.flatten()[1] == S.FLT_MAX               # the only valid pixel is +inf: nan_to_num of the masked path
        # lower median of an even count: patch 2 has two valid pixels, the smaller one is the median
        X = S.grid_view(d["x"], ps).flatten(0, 1)[2][S.grid_view(d["valid"].float(), ps).flatten(0, 1)[2] > 0.5]
        assert X.numel() == 2 and medm.flatten()[2] == X.min()
    p = d["all_nan_patch"]
    assert S.reduce_median_ref(d["x_nan"], ps).flatten()[p].isnan()
    assert S.reduce_median_ref(d["x_nan"], ps, d["valid"]).flatten()[p] == 0
    mean, bound = S.reduce_mean_ref(d["x_nan"], ps)
    assert mean.flatten()[p].isnan() and bound.flatten()[p] == 0
    assert torch.equal(mean.isnan(), S.grid_view(d["x_nan"], ps).isnan().any(-1))
    mean, bound = S.reduce_mean_ref(d["x"], ps, d["valid"])
    assert mean.isfinite().all() and (bound[mean.abs() < S.FLT_MAX] >= 0).all()
    # float32 torch agrees with the float64 mean inside the bound wherever the bound applies
    m32 = torch.nan_to_num(torch.nanmean(S.grid_view(d["x"], ps).masked_fill(
        S.grid_view(d["valid"].float(), ps) < 0.5, float("nan")), dim=-1), nan=0.0)
    assert ((m32.double() - mean).abs() <= bound).all()
    u, un = S.reduce_u_ref(d["C"], d["Q"], ps), S.reduce_u_ref(d["C_nan"], d["Q_nan"], ps)
    assert not u.isnan().any() and un.flatten()[p].isnan() and (ps == 1 or un.isnan().sum() == 1)
    assert float(u.min()) >= 0 and float(u.max()) <= 1
    if ps >= 5:
        assert not torch.equal(u.flatten()[:5], un.flatten()[:5])     # ignoring the NaN pixels moves a median


# ---- quality: classification -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.CLASSIFY_KINDS)
def test_classify_inputs_reach_every_class(kind):
    for n in S.CLASSIFY_N:
        dc, r, u = S.classify_inputs(n, kind)
        cls, pri = S.classify_ref(dc, r, u)
        assert cls.dtype == torch.int64 and pri.dtype == torch.float32 and cls.shape == (n,)
        assert float(pri.min()) >= 0 and float(pri.max()) <= 1
        if kind == "equal":
            assert not cls.any() and not pri.any()
            continue
        if kind == "quant" and n >= 3:
            assert float(S.lower_median((r - S.lower_median(r)).abs())) == 0.0          # the MAD is 0
        if n >= 48:
            assert sorted(cls.unique().tolist()) == [0, 1, 2, 3], (kind, n)
            at = dc == np.float32(S.THR_DC)
            assert at.sum() >= n // 3 and not (cls[at] == 1).any() and (n < 1023 or (cls[at] == 2).any())
            assert abs(float(pri.max()) - 1) < 1e-5


def test_classify_ref_is_the_robust_z_of_torch():
    dc, r, u = S.classify_inputs(1025, "random")
    m = torch.median(r)
    z = (r - m) / (torch.median((r - m).abs()) + 1e-6)
    cls, _ = S.classify_ref(dc, r, u, thr_zu=-1e9)          # zu > thr always: class 2 <=> dc >= thr and zr > thr
    assert torch.equal(cls == 2, (dc >= S.THR_DC) & (z > S.THR_ZR))


# ---- local TSDF ------------------------------------------------------------------------------------------------------
def test_build_cases_have_the_stated_grids_and_counts():
    want = {"main": (16, 10, 5), "long": (64, 25, 1), "tiny": (3, 2, 2), "inside": (16, 10, 5), "four": (16, 10, 5),
            "five": (16, 10, 5)}
    for name in S.BUILD_CASES:
        b = S.build_case(name)
        assert b["dims"] == want[name], name
        assert b["tsdf"].shape == b["dims"][::-1]
        touched = b["weights"] > 0
        if name == "four":
            assert b["n_valid"] == 4 and not touched.any() and (b["tsdf"] == 1).all()
        elif name == "five":
            assert b["n_valid"] == 5 and touched.any()
        elif name == "long":       # thin slab: a third of the voxels, over the whole length of the capped axis
            assert touched.mean() > 0.25 and touched.any(axis=(0, 1)).sum() >= 60, (name, touched.mean())
        else:
            assert touched.mean() > (0.3 if name == "inside" else 0.9), (name, touched.mean())
    b = S.build_case("main")
    v = b["valid"]
    assert not v[1400:1430].any() and v[1430:1436].all() and not v[1436]       # conf <= min, NaN, inf out; faces in
    assert 0.5 < v[:1400].mean() < 0.9                                          # a good part lies outside the ROI
    assert (S.build_case("tiny")["weights"] > 25).all()       # a sample adds less than 1: every voxel replays dozens
    b = S.build_case("long")
    act = (b["mx"] - b["mn"]) / np.array(b["dims"], np.float32)
    assert act[0] > 1.09 * S.VOXEL
    b = S.build_case("inside")
    d = np.linalg.norm(b["Xw"] - b["origin"], axis=1)
    assert (d[:5] < 0.05).all() and b["valid"][:5].all() and (d > 0.05).sum() > 300


def test_raycast_cases_keep_both_outcomes():
    rate = {k: S.raycast_case(k)["hit"].mean() for k in ("sigma4", "sigma30", "built", "zero", "samples2")}
    assert rate["sigma4"] >= 0.9 and 0.1 <= rate["sigma30"] <= 0.8 and 0.3 <= rate["built"] <= 0.95, rate
    assert rate["zero"] == 0.0, rate
    for name in S.RAYCAST_CASES:
        c = S.raycast_case(name)
        miss = ~c["hit"]
        np.testing.assert_array_equal(c["surf"][miss], c["X"][c["sel"]][miss])
        assert len(c["sel"]) == 0 or (c["surf"][c["hit"]] != c["X"][c["sel"]][c["hit"]]).any(1).all()
        assert len(np.unique(c["sel"])) == len(c["sel"])
    e = S.raycast_case("edge_rays")
    first = {int(p): k for k, p in enumerate(e["sel"])}
    assert not e["hit"][[first[i] for i in (0, 1, 2, 5)]].any() and e["hit"].any()
    assert [len(S.raycast_case(f"sel{n}")["sel"]) for n in (0, 1, 63, 64, 65)] == [0, 1, 63, 64, 65]
    assert (np.diff(S.raycast_case("sigma4")["sel"]) < 0).any()
    # the zero case does cross the surface: the same rays hit in the analytic volume
    z = S.raycast_inputs("zero")
    from oracle import tsdf_refine_py as TR
    dims = TR.grid_dims(z["mn"], z["mx"], S.VOXEL, 64)[:3]
    _, hits = TR.extract_surface(S.analytic_volume(z["mn"], z["mx"], dims), z["mn"], z["mx"], np.ones(len(z["X"]), bool),
                                 z["X"], z["sel"][:20], 64, S.MAX_DISP, "scalar")
    assert hits.sum() >= 15
