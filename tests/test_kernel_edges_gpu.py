"""GPU tests (-m gpu) of the four building blocks of the MASt3R forward at the edges of their tiles: mslam_gemm_bf16 under
every tile configuration, mslam_conv2d_nhwc_bf16 under the conv tile override, mslam_attention_bf16 over uneven and
empty key splits, mslam_layernorm_f32 - each against the int64 / float64 statement in tests/kernel_refs.py.

Integer-valued operands make GEMM and convolution EXACT (every intermediate is an integer below 2^24, so any fp32
accumulation order gives the same bits): those tests use torch.equal, a wrong K tail, tap or row cannot hide behind a
tolerance.  The rounded tests assert a derived per-element bound (docstrings in kernel_refs.py), never a norm over the
whole output.  Every operand lives in a guarded buffer (kernel_refs.Guarded): NaN-pattern guards in front and behind
must come back bit-identical, no output element may be left unwritten, and a read that escapes an input shows as NaN."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

GEMM_CFGS = (0, 642, 643, 644, 1262, 1263, 1242, 1282, 1283, 2128, 2256, 2192, 2258, 8256)   # 0: the heuristic
CONV_CFGS = (0, 642, 644, 1262, 1242, 1283, 2128, 2256, 2192, 8256)                            # 8256 routes to 2256


def _lib():
    import mslam_hip as m

    return m


def _p(g):
    return 0 if g is None else _lib().ptr(g.t)


# ---- 1. exact GEMM ---------------------------------------------------------------------------------------------------
GEMM_EXACT_SHAPES = [
    (1, 8, 8),          # minimum problem
    (64, 64, 64),       # exact tile, nk = 1
    (65, 72, 72),       # one past the 64 tile, K tail of 8
    (129, 136, 128),    # nk = 2
    (129, 136, 200),    # nk = 4, tail 8
    (193, 264, 136),    # past the 192-row and the 256-column tile
    (257, 264, 520),    # past the 256-row and the 256-column tile
    (250, 123, 584),    # odd N: scalar epilogue, 8256 falls back
    (300, 7, 64),       # N < 8
    (33, 40, 192),      # nk = 3
    (1100, 136, 72),    # partial last row-panel group for every BM
]


@pytest.mark.parametrize("M,N,K", GEMM_EXACT_SHAPES)
def test_gemm_exact(device, M, N, K):
    """A, W integers in [-4, 4], bias and residual integers in [-64, 64]: the int64 result is below 2^24 in every
    intermediate (16 K + 128, K <= 584), so every configuration must return it bit for bit - f32 as is, bf16 as the
    integer rounded once to nearest-even - with bias and residual present or NULL, without and with ReLU."""
    m = _lib()
    g = torch.Generator().manual_seed(M * 131 + N * 17 + K)
    A, W = R.rand_int(g, (M, K), 4), R.rand_int(g, (N, K), 4)
    bias, res = R.rand_int(g, (N,), 64), R.rand_int(g, (M, N), 64)
    bufs = {"A": R.Guarded(device, torch.bfloat16, src=A), "W": R.Guarded(device, torch.bfloat16, src=W),
            "bias": R.Guarded(device, torch.float32, src=bias), "res": R.Guarded(device, torch.float32, src=res)}
    outs = {0: R.Guarded(device, torch.float32, (M, N)), 1: R.Guarded(device, torch.bfloat16, (M, N))}
    cases = []
    for has_bias, has_res in ((1, 1), (0, 1), (1, 0)):
        for act in (R.ACT_NONE, R.ACT_RELU):
            ref, mag = R.gemm_int_ref(A, W, bias if has_bias else None, res if has_res else None, act)
            assert mag < 2 ** 24
            cases.append((has_bias, has_res, act, {0: ref.to(torch.float32).to(device), 1: R.to_bf16_once(ref).to(device)}))
    try:
        for cfg in GEMM_CFGS:
            m.check(m.lib().mslam_gemm_tile_override(M, N, K, cfg), "override")
            for has_bias, has_res, act, want in cases:
                for out_bf16 in (0, 1):
                    what = f"gemm {M}x{N}x{K} cfg {cfg} bias {has_bias} res {has_res} act {act} bf16 {out_bf16}"
                    out = outs[out_bf16].refill()
                    rc = m.lib().mslam_gemm_bf16(_p(bufs["A"]), _p(bufs["W"]), _p(bufs["bias"]) if has_bias else 0,
                                                 _p(bufs["res"]) if has_res else 0, _p(out), M, N, K, act, out_bf16,
                                                 m.stream_ptr())
                    m.check(rc, what)
                    R.check_guards({**bufs, "out": out}, ["out"], what)
                    if not torch.equal(out.t, want[out_bf16]):
                        bad = (out.t != want[out_bf16]).nonzero()
                        r, c = bad[0].tolist()
                        raise AssertionError(f"{what}: {len(bad)} wrong elements, first at ({r}, {c}): "
                                             f"{float(out.t[r, c])} != {float(want[out_bf16][r, c])}")
    finally:
        m.lib().mslam_gemm_tile_override(M, N, K, 0)


# ---- 2. rounded GEMM, including GELU ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(129, 136, 200), (250, 123, 584)])
def test_gemm_rounded(device, M, N, K):
    """Random bf16 operands, f32 bias and residual, act in {none, GELU, ReLU}, f32 and bf16 output, every configuration:
    each element within the bound derived in kernel_refs.gemm_f64_ref of the float64 result, and every configuration
    bit-identical to the heuristic's choice (all tilings accumulate an element over K in the same order)."""
    m = _lib()
    g = torch.Generator().manual_seed(M + N + K)
    A = (torch.rand(M, K, generator=g) * 2 - 1).to(torch.bfloat16)
    W = ((torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
    bias, res = torch.rand(N, generator=g) - 0.5, torch.rand(M, N, generator=g)
    bufs = {"A": R.Guarded(device, torch.bfloat16, src=A), "W": R.Guarded(device, torch.bfloat16, src=W),
            "bias": R.Guarded(device, torch.float32, src=bias), "res": R.Guarded(device, torch.float32, src=res)}
    outs = {0: R.Guarded(device, torch.float32, (M, N)), 1: R.Guarded(device, torch.bfloat16, (M, N))}
    first = {}
    try:
        for cfg in GEMM_CFGS:
            m.check(m.lib().mslam_gemm_tile_override(M, N, K, cfg), "override")
            for act in (R.ACT_NONE, R.ACT_GELU, R.ACT_RELU):
                for out_bf16 in (0, 1):
                    what = f"gemm {M}x{N}x{K} cfg {cfg} act {act} bf16 {out_bf16}"
                    out = outs[out_bf16].refill()
                    rc = m.lib().mslam_gemm_bf16(_p(bufs["A"]), _p(bufs["W"]), _p(bufs["bias"]), _p(bufs["res"]), _p(out),
                                                 M, N, K, act, out_bf16, m.stream_ptr())
                    m.check(rc, what)
                    R.check_guards({**bufs, "out": out}, ["out"], what)
                    if cfg == 0:
                        first[act, out_bf16] = out.t.clone()
                    else:
                        assert torch.equal(out.t, first[act, out_bf16]), f"{what}: differs from the heuristic's tile"
    finally:
        m.lib().mslam_gemm_tile_override(M, N, K, 0)
    for (act, out_bf16), got in first.items():
        ref, bound = R.gemm_f64_ref(A, W, bias, res, act, out_bf16)
        err = (got.cpu().double() - ref).abs()
        ratio = err / bound
        print(f"gemm_rounded {M}x{N}x{K} act {act} bf16 {out_bf16}: max err/bound {float(ratio.max()):.3f}")
        assert bool((err <= bound).all()), f"act {act} bf16 {out_bf16}: err/bound up to {float(ratio.max())}"


# ---- 3. exact convolution --------------------------------------------------------------------------------------------
CONV_SHAPES = [
    (1, 5, 7, 8, 8, 3, 1),        # every 8-wide chunk is a different tap
    (2, 9, 13, 24, 40, 3, 2),     # odd sizes, stride 2, 64 % Cin != 0
    (1, 6, 10, 72, 16, 1, 2),     # 1x1 stride 2
    (1, 17, 19, 40, 136, 3, 1),   # M = 323, crosses 256
    (3, 8, 8, 64, 8, 3, 1),       # batch boundaries inside one row tile
    (1, 4, 4, 128, 12, 3, 1),     # Cout % 8 != 0
]


@pytest.mark.parametrize("B,H,W,Cin,Cout,ks,stride", CONV_SHAPES)
def test_conv2d_exact(device, B, H, W, Cin, Cout, ks, stride):
    """Integer image and weights in [-4, 4] (the image partly negative, with some -0.0, so the ReLU on load matters),
    integer bias and bf16 residual in [-64, 64]: float64 F.conv2d is exact, the device result must equal it rounded once
    to bf16, under every tile forced through the conv override (M < 0), relu_in 0/1, act none/ReLU, residual or NULL."""
    m = _lib()
    g = torch.Generator().manual_seed(H * W + Cin + Cout)
    x = R.rand_int(g, (B, Cin, H, W), 4).to(torch.bfloat16)
    x[R.rand_int(g, x.shape, 4) == 0] = -0.0
    w = R.rand_int(g, (Cout, Cin, ks, ks), 4)
    bias = R.rand_int(g, (Cout,), 64)
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    res = R.rand_int(g, (B, Ho, Wo, Cout), 64)
    M, K = B * Ho * Wo, ks * ks * Cin
    mag = R.conv_ref(x.abs(), w.abs(), bias.abs(), res.abs(), stride, 0, R.ACT_NONE)
    assert float(mag.max()) < 2 ** 24
    bufs = {"x": R.Guarded(device, torch.bfloat16, src=x.permute(0, 2, 3, 1).contiguous()),
            "w": R.Guarded(device, torch.bfloat16, src=w.permute(0, 2, 3, 1).reshape(Cout, K).contiguous()),
            "bias": R.Guarded(device, torch.float32, src=bias), "res": R.Guarded(device, torch.bfloat16, src=res)}
    out = R.Guarded(device, torch.bfloat16, (B, Ho, Wo, Cout))
    cases = []
    for relu_in in (0, 1):
        for act in (R.ACT_NONE, R.ACT_RELU):
            for has_res in (1, 0):
                ref = R.conv_ref(x, w, bias, res if has_res else None, stride, relu_in, act)
                cases.append((relu_in, act, has_res, R.to_bf16_once(ref).to(device)))
    try:
        for cfg in CONV_CFGS:
            m.check(m.lib().mslam_gemm_tile_override(-M, Cout, K, cfg), "override")
            for relu_in, act, has_res, want in cases:
                what = f"conv {(B, H, W, Cin, Cout, ks, stride)} cfg {cfg} relu_in {relu_in} act {act} res {has_res}"
                out.refill()
                rc = m.lib().mslam_conv2d_nhwc_bf16(_p(bufs["x"]), _p(bufs["w"]), _p(bufs["bias"]),
                                                    _p(bufs["res"]) if has_res else 0, _p(out), B, H, W, Cin, Cout, ks,
                                                    stride, relu_in, act, m.stream_ptr())
                m.check(rc, what)
                R.check_guards({**bufs, "out": out}, ["out"], what)
                if not torch.equal(out.t, want):
                    bad = (out.t != want).nonzero()
                    i = tuple(bad[0].tolist())
                    raise AssertionError(f"{what}: {len(bad)} wrong elements, first at (b, oy, ox, co) = {i}: "
                                         f"{float(out.t[i])} != {float(want[i])}")
    finally:
        m.lib().mslam_gemm_tile_override(-M, Cout, K, 0)


# ---- 4. attention ----------------------------------------------------------------------------------------------------
def _run_attention(device, q, k, v, what):
    m = _lib()
    B, H, nq, _ = q.shape
    nk = k.shape[2]
    bufs = {"q": R.Guarded(device, torch.bfloat16, src=q), "k": R.Guarded(device, torch.bfloat16, src=k),
            "vt": R.Guarded(device, torch.bfloat16, src=v.transpose(-1, -2).contiguous()),
            "o": R.Guarded(device, torch.bfloat16, (B, nq, H * 64))}
    rc = m.lib().mslam_attention_bf16(_p(bufs["q"]), _p(bufs["k"]), _p(bufs["vt"]), _p(bufs["o"]), B, H, nq, nk,
                                      m.stream_ptr())
    m.check(rc, what)
    R.check_guards(bufs, ["o"], what)
    return bufs["o"].t.cpu().double()


@pytest.mark.parametrize("kind", ["leak", "spike"])
@pytest.mark.parametrize("B,H,nq,nk", R.ATTN_SHAPES)
def test_attention_bounded(device, B, H, nq, nk, kind):
    """Every output element within kernel_refs.attention_bound of the float64 softmax(q k^T) v, over 1, 2, 5, 6, 7 and 10
    key tiles on the 4-split path (empty splits, a partial tile alone in its split, uneven tile counts per wave) and on
    the 2-split path.  `leak`: every real score is <= -8, so a zero-filled padded key that took part (score 0) would own
    over 99 % of the softmax.  nq not a multiple of 64: a store for a row >= nq lands in the next batch element's rows
    (B > 1: wrong values) or in the guard behind O."""
    q, k, v = R.attention_inputs(B, H, nq, nk, kind)
    ref, pabs, smax = R.attention_ref(q, k, v)
    if kind == "leak":
        assert smax <= -8.0
    out = _run_attention(device, q, k, v, f"attention {(B, H, nq, nk)} {kind}")
    err, bound = (out - ref).abs(), R.attention_bound(ref, pabs)
    print(f"attention {(B, H, nq, nk)} {kind}: max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), f"err/bound up to {float((err / bound).max())}"


def test_attention_vt_tail_stays_inside_its_head(device):
    """nk = 72: the second key tile holds 8 keys, its other V^T chunks lie past the row's end.  Head 1 carries +inf at
    keys 0-7 of every feature: should the tail of head 0's V^T rows be fetched from what follows them instead of being
    zero-filled, the zero probabilities of the masked keys turn it into NaN (0 x inf).  Head 0 must stay finite and
    inside the bound; head 1 (inf by construction) is not checked."""
    B, H, nq, nk = 1, 2, 33, 72
    q, k, v = R.attention_inputs(B, H, nq, nk, "leak")
    v[0, 1, 0:8, :] = float("inf")
    out = _run_attention(device, q, k, v, "attention V^T tail")[..., :64]
    v[0, 1] = 0.0
    ref, pabs, _ = R.attention_ref(q, k, v)
    ref, pabs = ref[..., :64], pabs[..., :64]
    assert bool(torch.isfinite(out).all())
    err, bound = (out - ref).abs(), R.attention_bound(ref, pabs)
    assert bool((err <= bound).all()), f"err/bound up to {float((err / bound).max())}"


# ---- 5. LayerNorm ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 7])
@pytest.mark.parametrize("D", [8, 63, 65, 100, 768, 1024, 2048])
@pytest.mark.parametrize("kind", ["random", "constant", "offset"])
def test_layernorm_bounded(device, D, rows, kind):
    """Every element within the bound derived in kernel_refs.layernorm_ref of the float64 result: the generic kernel
    (D = 8 ... 2048, D not a multiple of 64) and both vector kernels (768, 1024), rows % 4 != 0, bf16-only, f32-only and
    both outputs; a constant row (variance 0: eps decides) and an offset row (x = 1000 + N(0,1): a one-pass variance
    fails it)."""
    m = _lib()
    g = torch.Generator().manual_seed(D * 8 + rows)
    if kind == "random":
        x = torch.randn(rows, D, generator=g) * 3 + 0.5
    elif kind == "constant":
        x = (torch.rand(rows, 1, generator=g) * 6 - 3).expand(rows, D).contiguous()
    else:
        x = 1000.0 + torch.randn(rows, D, generator=g)
    w, b = torch.rand(D, generator=g) + 0.5, torch.rand(D, generator=g) - 0.5
    eps = 1e-6
    bufs = {"x": R.Guarded(device, torch.float32, src=x), "w": R.Guarded(device, torch.float32, src=w),
            "b": R.Guarded(device, torch.float32, src=b)}
    ob, of = R.Guarded(device, torch.bfloat16, (rows, D)), R.Guarded(device, torch.float32, (rows, D))
    for use_bf, use_f in ((1, 0), (0, 1), (1, 1)):
        what = f"layernorm {rows}x{D} {kind} bf16 {use_bf} f32 {use_f}"
        ob.refill()
        of.refill()
        rc = m.lib().mslam_layernorm_f32(_p(bufs["x"]), _p(bufs["w"]), _p(bufs["b"]), _p(ob) if use_bf else 0,
                                         _p(of) if use_f else 0, rows, D, eps, m.stream_ptr())
        m.check(rc, what)
        used = [(n, buf, is_bf) for n, buf, is_bf, on in (("ob", ob, True, use_bf), ("of", of, False, use_f)) if on]
        R.check_guards({**bufs, **{n: buf for n, buf, _ in used}}, [n for n, _, _ in used], what)
        for _, buf, is_bf in used:
            ref, bound = R.layernorm_ref(x, w, b, eps, is_bf)
            err = (buf.t.cpu().double() - ref).abs()
            assert bool((err <= bound).all()), f"{what}: err/bound up to {float((err / bound).max())}"
