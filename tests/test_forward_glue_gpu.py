"""GPU tests (-m gpu) of the code BETWEEN the building blocks of the MASt3R forward: the RoPE / head-split epilogue of the
attention projections (both of its forms), the grouped (two decoder sides, one grid) launches, the pixel scatter of the
transposed convolutions, the second residual of the implicit-conv GEMM, the grouped LayerNorms, the bilinear upsample,
both forms of the head post-process, patchify / concat / cast.  Each entry point builds its launch with the helper the
forward itself uses (csrc/mast3r.hip), so the stride arithmetic and the choice of form are what is tested.

As in tests/test_kernel_edges_gpu.py: integer operands make everything up to the first rounding EXACT (torch.equal),
everything else is held to a per-element bound derived in tests/kernel_refs.py (never a norm over a tensor), every
operand lives in a guarded buffer, no output element may stay unwritten, and what a launch must not touch keeps its
pattern.  Every bounded test prints its largest err/bound ratio."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R  # noqa: E402
from test_kernel_edges_gpu import CONV_CFGS, GEMM_CFGS  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
ROPE_LEN = 1024


def _lib():
    import mslam_hip as m

    return m


def _p(g):
    return 0 if g is None else _lib().ptr(g.t)


def _check_bound(what, got, ref, bound):
    """every element of `got` within `bound` of `ref` (float64, CPU); prints and returns the largest err/bound"""
    err = (got.detach().cpu().double() - ref).abs()
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(ratio.max())
    print(f"{what}: max err/bound {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: err/bound up to {worst}"
    return worst


def _assert_equal(what, got, want):
    want = want.to(got.device)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} wrong elements, first at {i}: {float(got[i])} != {float(want[i])}")


def _untouched(g):
    return bool((g.raw == g.pat).all())


# ---- 1. RoPE tables --------------------------------------------------------------------------------------------------
_tables_cache = {}


def _rope_tables():
    """the library's tables, f32 numpy [1024,16] each, inside guarded host arrays"""
    if not _tables_cache:
        m = _lib()
        pad, n = 64, ROPE_LEN * 16
        raw = [np.full(n + 2 * pad, np.float32(-7.25), np.float32) for _ in range(2)]
        m.check(m.lib().mslam_rope_tables(raw[0][pad:].ctypes.data, raw[1][pad:].ctypes.data, ROPE_LEN), "rope_tables")
        for r in raw:
            assert (r[:pad] == -7.25).all() and (r[pad + n:] == -7.25).all(), "rope_tables wrote outside its arrays"
        _tables_cache["cos"] = raw[0][pad:pad + n].reshape(ROPE_LEN, 16).copy()
        _tables_cache["sin"] = raw[1][pad:pad + n].reshape(ROPE_LEN, 16).copy()
    return _tables_cache["cos"], _tables_cache["sin"]


def test_rope_tables(device):
    """The host loop mslam_mast3r_create fills its tables with, at the production length 1024, against the reference
    model's order of operations (fp32 inv_freq, fp32 product, float64 cos / sin); bound in kernel_refs.rope_tables_ref."""
    c, s = _rope_tables()
    rc, rs, bc, bs = R.rope_tables_ref(ROPE_LEN)
    _check_bound("rope cos", torch.from_numpy(c), rc, bc)
    _check_bound("rope sin", torch.from_numpy(s), rs, bs)
    assert (c[0] == 1.0).all() and (s[0] == 0.0).all()


# ---- 2. attention projection -----------------------------------------------------------------------------------------
# token grid (rows, columns) -> the other k/v grids (same columns: tok_w is shared) it is paired with for kv_ntok != ntok
ATTN_GRIDS = {
    (2, 2): [(4, 2)],              # 4 tokens: scalar path, the smallest V^T store
    (4, 6): [(2, 6)],              # 24 tokens: scalar path
    (4, 8): [(8, 8), (3, 8)],      # 32 tokens: wide path; kv 64 wide as well; kv 24 narrow -> scalar path
    (8, 12): [(16, 12), (4, 12)],  # 96 tokens: wide path, three row tiles per image; kv 192 wide; kv 48 narrow -> scalar
    (5, 4): [(3, 4)],              # 20 tokens: scalar path, ntok not a multiple of 8
}
ATTN_DIMS = [(1, 1, 64), (3, 3, 200), (1, 3, 200), (3, 1, 64)]    # (B, heads, K)


@pytest.mark.parametrize("B,heads,K", ATTN_DIMS)
@pytest.mark.parametrize("grid", list(ATTN_GRIDS))
def test_attn_project(device, grid, B, heads, K):
    """A, W, bias integers (|pre-activation| <= 16 K + 64 < 2^24, exact in any accumulation order).  V^T must be the
    integers rounded once to bf16 and transposed, bit for bit; q and k lie within the bound of
    kernel_refs.attn_project_ref, computed from the library's own table values.  Forms: {q,k,v}, {q}, {k,v} with
    sec_base 1, {k,v} with its own token count (both wide, and wide ntok with narrow kv_ntok); each as a single problem and
    as the grouped launch of two sides with their own W and bias.  B = 3 puts batch boundaries inside a 32-row tile."""
    m = _lib()
    gh, gw = grid
    ntok, sd = gh * gw, heads * 64
    g = torch.Generator().manual_seed(gh * 1000 + gw * 100 + B * 10 + heads + K)
    cos_np, sin_np = _rope_tables()
    cos, sin = torch.from_numpy(cos_np).double(), torch.from_numpy(sin_np).double()
    tab = {"cos": R.Guarded(device, F32, src=torch.from_numpy(cos_np)), "sin": R.Guarded(device, F32, src=torch.from_numpy(sin_np))}
    nmax = max([ntok] + [a * b for a, b in ATTN_GRIDS[grid]])
    A2 = R.rand_int(g, (2, B * nmax, K), 4)                       # per side, rows of the largest token count
    W2, b2 = R.rand_int(g, (2, 3 * sd, K), 4), R.rand_int(g, (2, 3 * sd), 64)
    forms = [("qkv", 0, 3, ntok, ntok), ("q", 0, 1, ntok, ntok), ("kv", 1, 2, ntok, ntok)]
    forms += [(f"kv{a}x{b}", 1, 2, ntok, a * b) for a, b in ATTN_GRIDS[grid]]
    worst = 0.0
    for name, sec_base, nsec, nt, kvt in forms:
        rows = B * (nt if sec_base == 0 else kvt)
        cols = slice(sec_base * sd, (sec_base + nsec) * sd)
        for sides in (1, 2):
            what = f"attn grid {grid} B {B} heads {heads} K {K} form {name} sides {sides}"
            A = A2[:sides, :rows].reshape(sides * rows, K)
            bufs = {"A": R.Guarded(device, BF, src=A), **tab}
            for s in range(sides):
                bufs[f"W{s}"] = R.Guarded(device, BF, src=W2[s, cols])
                bufs[f"b{s}"] = R.Guarded(device, F32, src=b2[s, cols])
            outs = {"q": R.Guarded(device, BF, (sides, B, heads, nt, 64)), "k": R.Guarded(device, BF, (sides, B, heads, kvt, 64)),
                    "vt": R.Guarded(device, BF, (sides, B, heads, 64, kvt))}
            made = [n for n, sec in (("q", 0), ("k", 1), ("vt", 2)) if sec_base <= sec < sec_base + nsec]
            rc = m.lib().mslam_gemm_attn_bf16(_p(bufs["A"]), _p(bufs["W0"]), _p(bufs["b0"]), _p(bufs.get("W1")),
                                              _p(bufs.get("b1")), _p(outs["q"]), _p(outs["k"]), _p(outs["vt"]), rows, K, nsec,
                                              sec_base, heads, nt, kvt, gw, _p(tab["cos"]), _p(tab["sin"]), ROPE_LEN, 0.125,
                                              m.stream_ptr())
            m.check(rc, what)
            R.check_guards({**bufs, **outs}, made, what)
            for n in outs:
                if n not in made:
                    assert _untouched(outs[n]), f"{what}: {n} is not produced by this launch but was written"
            for s in range(sides):
                pre, mag = R.gemm_int_ref(A2[s, :rows], W2[s, cols], b2[s, cols], None, R.ACT_NONE)
                assert mag < 2 ** 24
                ref = R.attn_project_ref(pre, B, heads, sec_base, nt, kvt, gw, cos, sin, 0.125)
                assert sorted(ref) == sorted(made)
                for n in made:
                    if n == "vt":
                        _assert_equal(f"{what} side {s} vt", outs["vt"].t[s], ref["vt"])
                    else:
                        y, _, bound = ref[n]
                        err = (outs[n].t[s].cpu().double() - y).abs()
                        assert bool((err <= bound).all()), f"{what} side {s} {n}: err/bound up to {float((err / bound).max())}"
                        worst = max(worst, float(torch.where(err > 0, err / bound, torch.zeros_like(err)).max()))
    print(f"attn_project grid {grid} B {B} heads {heads} K {K}: max err/bound {worst:.3f}")


# ---- 3. grouped plain GEMM -------------------------------------------------------------------------------------------
# (M, N, K) -> the configuration the heuristic of csrc/gemm.hip takes for TWO problems of that shape (the tile override
# is not consulted for grouped launches); blocks(bm, bn) = 2 ceil(M / bm) ceil(N / bn)
GROUPED_SHAPES = [
    ((4, 8, 8), 643),            # 2 tiles of 64x64; none of the earlier rules: K < 2048 -> ring of 3
    ((65, 72, 72), 643),         # 4 tiles per problem
    ((129, 123, 136), 643),      # odd N: scalar epilogue
    ((129, 64, 72), 643),        # 3 tiles per problem: odd and below the 8 XCDs the grid is dealt over
    ((65, 72, 2048), 644),       # blocks(64, 64) = 8 < 512 and K >= 2048 -> ring of 4
    ((1024, 1024, 64), 642),     # blocks(256,256) = 32, blocks(128,128) = 128 < 256, blocks(64,64) = 512 -> 642
    ((1024, 2048, 64), 1282),    # blocks(256,256) = 64 < 128, blocks(128,128) = 256 -> 1282
    ((2048, 2048, 64), 2256),    # blocks(256,256) = 128 -> 2256
    ((16384, 128, 64), 2128),    # narrow N and blocks(256,128) = 128 -> 2128
]


def _expected_cfg(M, N, K):
    """the rule of launch_gemm_impl for groups == 2, restated"""
    blocks = lambda bm, bn: 2 * -(-M // bm) * -(-N // bn)
    narrow = N <= 128 or 256 < N <= 384
    if narrow and blocks(256, 128) >= 128:
        return 2128
    if blocks(256, 256) >= 128:
        return 2256
    if blocks(128, 128) >= 256:
        return 1282
    if blocks(64, 64) >= 512:
        return 642
    return 644 if K >= 2048 else 643


def _int_gemm(A, W, bias, res, act):
    """gemm_int_ref; for the large shapes through float64 (exact: every value is an integer below 2^53)"""
    if A.shape[0] * W.shape[0] * A.shape[1] <= 5e7:
        return R.gemm_int_ref(A, W, bias, res, act)
    x = (A.double() @ W.double().T).to(torch.int64) + bias
    if act == R.ACT_RELU:
        x = x.clamp_min(0)
    if res is not None:
        x = x + res
    return x, 16 * A.shape[1] + 128


@pytest.mark.parametrize("shape,cfg", GROUPED_SHAPES)
def test_gemm_grouped_exact(device, shape, cfg):
    """Two problems of one shape in one grid as linear_residual (f32 out = residual + ..., in place) and linear_bf16 (bf16
    out, no residual) launch them, act none and ReLU, integer operands as in test_gemm_exact: both sides must equal the
    int64 result bit for bit, and the same problem run alone through mslam_gemm_bf16."""
    m = _lib()
    M, N, K = shape
    assert _expected_cfg(M, N, K) == cfg
    g = torch.Generator().manual_seed(M * 131 + N * 17 + K)
    A, W = R.rand_int(g, (2, M, K), 4), R.rand_int(g, (2, N, K), 4)
    bias, res = R.rand_int(g, (2, N), 64), R.rand_int(g, (2, M, N), 64)
    bufs = {"A": R.Guarded(device, BF, src=A.reshape(2 * M, K)), "res": R.Guarded(device, F32, src=res)}
    for s in range(2):
        bufs[f"W{s}"] = R.Guarded(device, BF, src=W[s])
        bufs[f"b{s}"] = R.Guarded(device, F32, src=bias[s])
        bufs[f"A{s}"] = R.Guarded(device, BF, src=A[s])
        bufs[f"res{s}"] = R.Guarded(device, F32, src=res[s])
    out_f, out_b = R.Guarded(device, F32, (2, M, N)), R.Guarded(device, BF, (2, M, N))
    one_f, one_b = R.Guarded(device, F32, (M, N)), R.Guarded(device, BF, (M, N))
    for act in (R.ACT_NONE, R.ACT_RELU):
        for out_bf16 in (0, 1):
            what = f"grouped gemm {shape} act {act} bf16 {out_bf16}"
            if out_bf16:
                out = out_b.refill()
            else:
                out = out_f
                out.refill().t.copy_(res)        # the residual stream: read and overwritten in place
            rc = m.lib().mslam_gemm_grouped_bf16(_p(bufs["A"]), _p(bufs["W0"]), _p(bufs["b0"]), _p(bufs["W1"]), _p(bufs["b1"]),
                                                 0 if out_bf16 else _p(out), _p(out), M, N, K, act, out_bf16, m.stream_ptr())
            m.check(rc, what)
            R.check_guards({**bufs, "out": out}, ["out"], what)
            for s in range(2):
                ref, mag = _int_gemm(A[s], W[s], bias[s], None if out_bf16 else res[s], act)
                assert mag < 2 ** 24
                want = R.to_bf16_once(ref) if out_bf16 else ref.to(F32)
                _assert_equal(f"{what} side {s}", out.t[s], want)
                one = (one_b if out_bf16 else one_f).refill()
                rc = m.lib().mslam_gemm_bf16(_p(bufs[f"A{s}"]), _p(bufs[f"W{s}"]), _p(bufs[f"b{s}"]),
                                             0 if out_bf16 else _p(bufs[f"res{s}"]), _p(one), M, N, K, act, out_bf16,
                                             m.stream_ptr())
                m.check(rc, what + " alone")
                R.check_guards({**bufs, "one": one}, ["one"], what + " alone")
                assert torch.equal(one.t, out.t[s]), f"{what} side {s}: differs from the problem run alone"


def test_gemm_grouped_gelu_rounded(device):
    """The fc1 launch of a decoder layer (bf16 out, GELU, both sides) on rounded operands: each side within the bound of
    kernel_refs.gemm_f64_ref and bit-identical to the side run alone."""
    m = _lib()
    M, N, K = 129, 123, 136
    g = torch.Generator().manual_seed(M + N + K)
    A = (torch.rand(2, M, K, generator=g) * 2 - 1).to(BF)
    W = ((torch.rand(2, N, K, generator=g) * 2 - 1) / K ** 0.5).to(BF)
    bias = torch.rand(2, N, generator=g) - 0.5
    bufs = {"A": R.Guarded(device, BF, src=A.reshape(2 * M, K))}
    for s in range(2):
        bufs[f"W{s}"], bufs[f"b{s}"] = R.Guarded(device, BF, src=W[s]), R.Guarded(device, F32, src=bias[s])
        bufs[f"A{s}"] = R.Guarded(device, BF, src=A[s])
    out, one = R.Guarded(device, BF, (2, M, N)), R.Guarded(device, BF, (M, N))
    rc = m.lib().mslam_gemm_grouped_bf16(_p(bufs["A"]), _p(bufs["W0"]), _p(bufs["b0"]), _p(bufs["W1"]), _p(bufs["b1"]), 0,
                                         _p(out), M, N, K, R.ACT_GELU, 1, m.stream_ptr())
    m.check(rc, "grouped gelu")
    R.check_guards({**bufs, "out": out}, ["out"], "grouped gelu")
    for s in range(2):
        ref, bound = R.gemm_f64_ref(A[s], W[s], bias[s], torch.zeros(M, N), R.ACT_GELU, True)
        _check_bound(f"grouped gelu side {s}", out.t[s], ref, bound)
        one.refill()
        m.check(m.lib().mslam_gemm_bf16(_p(bufs[f"A{s}"]), _p(bufs[f"W{s}"]), _p(bufs[f"b{s}"]), 0, _p(one), M, N, K,
                                        R.ACT_GELU, 1, m.stream_ptr()), "gelu alone")
        R.check_guards({**bufs, "one": one}, ["one"], "gelu alone")
        assert torch.equal(one.t, out.t[s]), f"side {s} differs from the problem run alone"


# ---- 4. ConvTranspose2d ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 1, 1, 8, 8), (2, 3, 5, 24, 16), (1, 4, 6, 72, 12)])
def test_conv_transpose_exact(device, B, H, W, Cin, Cout, s):
    """Integer operands: every output pixel (b, y s + i, x s + j, co) must be the integer rounded once to bf16, under every
    plain-GEMM tile (the override applies: one ungrouped problem of shape B H W x Cout s s x Cin); Cout s s = 48 / 192 is
    no multiple of 64, bias is indexed by column / (s s)."""
    m = _lib()
    g = torch.Generator().manual_seed(H * W + Cin + Cout + s)
    x, w, bias = R.rand_int(g, (B, Cin, H, W), 4), R.rand_int(g, (Cin, Cout, s, s), 4), R.rand_int(g, (Cout,), 64)
    ref = R.conv_transpose_ref(x, w, bias)
    assert float(R.conv_transpose_ref(x.abs(), w.abs(), bias.abs()).max()) < 2 ** 24
    want = R.to_bf16_once(ref)
    bufs = {"x": R.Guarded(device, BF, src=x.permute(0, 2, 3, 1).contiguous()),
            "w": R.Guarded(device, BF, src=R.conv_transpose_weight(w)), "bias": R.Guarded(device, F32, src=bias)}
    out = R.Guarded(device, BF, (B, H * s, W * s, Cout))
    Mg, Ng = B * H * W, Cout * s * s
    try:
        for cfg in GEMM_CFGS:
            m.check(m.lib().mslam_gemm_tile_override(Mg, Ng, Cin, cfg), "override")
            what = f"conv_transpose {(B, H, W, Cin, Cout, s)} cfg {cfg}"
            out.refill()
            rc = m.lib().mslam_conv_transpose_nhwc_bf16(_p(bufs["x"]), _p(bufs["w"]), _p(bufs["bias"]), _p(out), B, H, W, Cin,
                                                        Cout, s, m.stream_ptr())
            m.check(rc, what)
            R.check_guards({**bufs, "out": out}, ["out"], what)
            _assert_equal(what, out.t, want)
    finally:
        m.lib().mslam_gemm_tile_override(Mg, Ng, Cin, 0)


# ---- 5. convolution with two residuals -------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 5, 7, 8, 8), (3, 8, 8, 64, 8), (1, 4, 4, 128, 12)])
def test_conv2d_two_residuals_exact(device, B, H, W, Cin, Cout):
    """The second residual of the implicit-conv GEMM (the `extra` operand of a DPT residual unit), 3x3 stride 1, integer
    operands: both residuals, either one alone, relu_in 0 / 1, act none / ReLU, every conv tile; Cout = 12 takes the
    scalar epilogue."""
    m = _lib()
    ks, stride = 3, 1
    g = torch.Generator().manual_seed(H * W + Cin + Cout)
    x = R.rand_int(g, (B, Cin, H, W), 4).to(BF)
    x[R.rand_int(g, x.shape, 4) == 0] = -0.0
    w, bias = R.rand_int(g, (Cout, Cin, ks, ks), 4), R.rand_int(g, (Cout,), 64)
    r1, r2 = R.rand_int(g, (B, H, W, Cout), 64), R.rand_int(g, (B, H, W, Cout), 64)
    M, K = B * H * W, ks * ks * Cin
    mag = R.conv_ref(x.abs(), w.abs(), bias.abs(), r1.abs(), stride, 0, R.ACT_NONE, res2=r2.abs())
    assert float(mag.max()) < 2 ** 24
    bufs = {"x": R.Guarded(device, BF, src=x.permute(0, 2, 3, 1).contiguous()),
            "w": R.Guarded(device, BF, src=w.permute(0, 2, 3, 1).reshape(Cout, K).contiguous()),
            "bias": R.Guarded(device, F32, src=bias), "r1": R.Guarded(device, BF, src=r1), "r2": R.Guarded(device, BF, src=r2)}
    out = R.Guarded(device, BF, (B, H, W, Cout))
    cases = []
    for relu_in in (0, 1):
        for act in (R.ACT_NONE, R.ACT_RELU):
            for has1, has2 in ((1, 1), (1, 0), (0, 1)):
                ref = R.conv_ref(x, w, bias, r1 if has1 else None, stride, relu_in, act, res2=r2 if has2 else None)
                cases.append((relu_in, act, has1, has2, R.to_bf16_once(ref).to(device)))
    try:
        for cfg in CONV_CFGS:
            m.check(m.lib().mslam_gemm_tile_override(-M, Cout, K, cfg), "override")
            for relu_in, act, has1, has2, want in cases:
                what = f"conv2 {(B, H, W, Cin, Cout)} cfg {cfg} relu_in {relu_in} act {act} res {has1}{has2}"
                out.refill()
                rc = m.lib().mslam_conv2d_res2_nhwc_bf16(_p(bufs["x"]), _p(bufs["w"]), _p(bufs["bias"]),
                                                         _p(bufs["r1"]) if has1 else 0, _p(bufs["r2"]) if has2 else 0, _p(out),
                                                         B, H, W, Cin, Cout, ks, stride, relu_in, act, m.stream_ptr())
                m.check(rc, what)
                R.check_guards({**bufs, "out": out}, ["out"], what)
                _assert_equal(what, out.t, want)
    finally:
        m.lib().mslam_gemm_tile_override(-M, Cout, K, 0)


# ---- 6. grouped LayerNorm --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3, 6, 50])
@pytest.mark.parametrize("D", [768, 1024, 192])
def test_layernorm_group(device, D, M):
    """Both stacked sides in one launch (vector kernels at D = 768 / 1024, the per-side fallback at 192), four independent
    affine pairs; single form: out_self only; cross form: norm_y of each side's rows lands in the OTHER side's block of
    out_mem.  M % 4 != 0: a block of 4 rows holds rows of both sides.  Bound: kernel_refs.layernorm_ref, bf16 output."""
    m = _lib()
    g = torch.Generator().manual_seed(D * 64 + M)
    eps = 1e-6
    names = ("self0", "self1", "mem0", "mem1")
    sets = {k: (torch.rand(D, generator=g) + 0.5, torch.rand(D, generator=g) - 0.5) for k in names}
    aff = {}
    for k in names:
        aff[k + "_w"], aff[k + "_b"] = R.Guarded(device, F32, src=sets[k][0]), R.Guarded(device, F32, src=sets[k][1])
    oself, omem = R.Guarded(device, BF, (2 * M, D)), R.Guarded(device, BF, (2 * M, D))
    for kind in ("random", "offset"):
        x = torch.randn(2 * M, D, generator=g) * 3 + 0.5 if kind == "random" else 1000.0 + torch.randn(2 * M, D, generator=g)
        bufs = {"x": R.Guarded(device, F32, src=x), **aff}
        for cross in (0, 1):
            what = f"layernorm_group D {D} M {M} {kind} cross {cross}"
            oself.refill()
            omem.refill()
            mem = [_p(aff[k]) if cross else 0 for k in ("mem0_w", "mem0_b", "mem1_w", "mem1_b")]
            rc = m.lib().mslam_layernorm_group_bf16(_p(bufs["x"]), _p(aff["self0_w"]), _p(aff["self0_b"]), _p(aff["self1_w"]),
                                                    _p(aff["self1_b"]), *mem, _p(oself), _p(omem) if cross else 0, M, D, eps,
                                                    m.stream_ptr())
            m.check(rc, what)
            R.check_guards({**bufs, "out_self": oself, "out_mem": omem}, ["out_self"] + (["out_mem"] if cross else []), what)
            ys, bs, ym, bm = R.layernorm_group_ref(x, sets, M, eps, bool(cross))
            _check_bound(what + " self", oself.t, ys, bs)
            if cross:
                _check_bound(what + " mem", omem.t, ym, bm)
            else:
                assert _untouched(omem), f"{what}: out_mem written by the single form"


# ---- 7. bilinear upsample --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 8), (1, 1, 5, 8), (2, 3, 5, 24), (3, 7, 2, 136), (1, 12, 16, 256)])
def test_upsample2x(device, B, H, W, C):
    """Every element within kernel_refs.upsample2x_ref's bound of the float64 align_corners=True interpolation (a wrong
    border row or the align_corners=False grid is far outside it); the four corners of every image equal the input's
    corners bit for bit; a constant image comes back bit for bit."""
    m = _lib()
    g = torch.Generator().manual_seed(H * 100 + W + C)
    x = (torch.randn(B, H, W, C, generator=g) * 2).to(BF)
    const = torch.full((B, H, W, C), 1.2345).to(BF)
    out = R.Guarded(device, BF, (B, 2 * H, 2 * W, C))
    for name, src in (("random", x), ("constant", const)):
        what = f"upsample2x {(B, H, W, C)} {name}"
        bufs = {"x": R.Guarded(device, BF, src=src)}
        out.refill()
        rc = m.lib().mslam_upsample2x_nhwc_bf16(_p(bufs["x"]), _p(out), B, H, W, C, m.stream_ptr())
        m.check(rc, what)
        R.check_guards({**bufs, "out": out}, ["out"], what)
        got = out.t.cpu()
        if name == "constant":
            assert torch.equal(got, const[:, :1, :1].expand(B, 2 * H, 2 * W, C)), what
        else:
            y, _, bound = R.upsample2x_ref(src)
            _check_bound(what, got, y, bound)
            for oy, iy in ((0, 0), (2 * H - 1, H - 1)):
                for ox, ix in ((0, 0), (2 * W - 1, W - 1)):
                    assert torch.equal(got[:, oy, ox], src[:, iy, ix]), f"{what}: corner ({oy}, {ox})"


# ---- 8. head post-process --------------------------------------------------------------------------------------------
HEAD_CASES = [
    # P, fc, desc, B, H, W, extra columns of lf, forms (0: the dispatch, 1: forced generic)
    (16, 128, 24, 1, 16, 16, 0, (0, 1)),     # production form: one patch
    (16, 128, 24, 2, 32, 48, 64, (0, 1)),    # production form: 2 x 3 patches, batch 2, lf_ld > (desc + 1) P^2
    (8, 64, 16, 1, 16, 24, 0, (0,)),         # generic only
    (16, 128, 31, 1, 16, 16, 0, (0,)),       # generic only: the largest descriptor
]


@pytest.mark.parametrize("P,fc,desc,B,H,W,pad,forms", HEAD_CASES)
def test_head_post(device, P, fc, desc, B, H, W, pad, forms):
    """Both forms of the tail of a head against kernel_refs.head_post_ref on inputs with d from 0 to about 10 and conf
    logits of +-20: points, conf, descriptors and desc-conf per element, |‖D‖ - 1| <= 1e-6, and the pixel with an all-zero
    feature row (zero xyz bias) gives the point exactly 0."""
    m = _lib()
    lf_ld = (desc + 1) * P * P + pad
    feat, w4, b4, lf = R.head_inputs(B, H, W, P, fc, desc, lf_ld, 1000 * P + desc + H + W)
    ref = R.head_post_ref(feat, w4, b4, lf, desc, P)
    bufs = {"feat": R.Guarded(device, BF, src=feat), "w4": R.Guarded(device, F32, src=w4), "b4": R.Guarded(device, F32, src=b4),
            "lf": R.Guarded(device, F32, src=lf)}
    outs = {"X": R.Guarded(device, F32, (B, H, W, 3)), "C": R.Guarded(device, F32, (B, H, W)),
            "D": R.Guarded(device, F32, (B, H, W, desc)), "Q": R.Guarded(device, F32, (B, H, W))}
    for force in forms:
        what = f"head_post P {P} fc {fc} desc {desc} {(B, H, W)} generic {force}"
        for o in outs.values():
            o.refill()
        rc = m.lib().mslam_head_post(_p(bufs["feat"]), fc, _p(bufs["w4"]), _p(bufs["b4"]), _p(bufs["lf"]), lf_ld, desc, P, B, H,
                                     W, _p(outs["X"]), _p(outs["C"]), _p(outs["D"]), _p(outs["Q"]), force, m.stream_ptr())
        m.check(rc, what)
        R.check_guards({**bufs, **outs}, list(outs), what)
        for k in ("X", "C", "D", "Q"):
            _check_bound(f"{what} {k}", outs[k].t, *ref[k])
        X = outs["X"].t.cpu()
        assert bool(torch.isfinite(X).all()) and float(X[0, 1 % H, 2 % W].abs().max()) == 0.0, what
        nrm = outs["D"].t.cpu().double().norm(dim=-1)
        print(f"{what}: max | |D| - 1 | {float((nrm - 1).abs().max()):.2e}")
        assert float((nrm - 1).abs().max()) <= 1e-6, what


# ---- 9. patchify, concat, cast ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,B,H,W", [(16, 1, 16, 16), (16, 2, 32, 48), (8, 1, 8, 24)])
def test_patchify_exact(device, P, B, H, W):
    m = _lib()
    g = torch.Generator().manual_seed(P + H + W)
    img = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    bufs = {"img": R.Guarded(device, F32, src=img)}
    out = R.Guarded(device, BF, (B * (H // P) * (W // P), 3 * P * P))
    what = f"patchify P {P} {(B, H, W)}"
    m.check(m.lib().mslam_patchify_bf16(_p(bufs["img"]), _p(out), B, H, W, P, m.stream_ptr()), what)
    R.check_guards({**bufs, "out": out}, ["out"], what)
    _assert_equal(what, out.t, R.patchify_ref(img, P))


@pytest.mark.parametrize("rows,ca,cb", [(1, 8, 8), (50, 1024, 768), (7, 24, 40)])
def test_concat2_exact(device, rows, ca, cb):
    m = _lib()
    g = torch.Generator().manual_seed(rows + ca + cb)
    a, b = torch.randn(rows, ca, generator=g).to(BF), torch.randn(rows, cb, generator=g).to(BF)
    bufs = {"a": R.Guarded(device, BF, src=a), "b": R.Guarded(device, BF, src=b)}
    out = R.Guarded(device, BF, (rows, ca + cb))
    what = f"concat2 {(rows, ca, cb)}"
    m.check(m.lib().mslam_concat2_bf16(_p(bufs["a"]), ca, _p(bufs["b"]), cb, _p(out), rows, m.stream_ptr()), what)
    R.check_guards({**bufs, "out": out}, ["out"], what)
    assert torch.equal(out.t.cpu().view(torch.int16), torch.cat([a, b], 1).view(torch.int16)), what


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 4 * 256 * 3 + 2])
def test_cast_f32_bf16_exact(device, n):
    """float4 body and scalar tail: one round-to-nearest-even per element, on ties of both parities, +-0, a carry into the
    next binade and the largest finite value that stays finite (as far as n holds them), bit for bit."""
    m = _lib()
    x = R.cast_edge_values(n, torch.Generator().manual_seed(n))
    bufs = {"x": R.Guarded(device, F32, src=x)}
    out = R.Guarded(device, BF, (n,))
    m.check(m.lib().mslam_cast_f32_bf16(_p(bufs["x"]), _p(out), n, m.stream_ptr()), f"cast {n}")
    R.check_guards({**bufs, "out": out}, ["out"], f"cast {n}")
    assert torch.equal(out.t.cpu().view(torch.int16), R.to_bf16_once(x).view(torch.int16)), f"cast {n}"
