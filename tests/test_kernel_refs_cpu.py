"""CPU tests of tests/kernel_refs.py: the references and bounds that tests/test_kernel_edges_gpu.py holds the HIP kernels
to are themselves checked here - against an independent statement of the same operation, and (for the bounds) against a
CPU emulation of a correct kernel in the kernel's number formats, so a bound is shown to admit a correct kernel."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R  # noqa: E402


def test_gemm_int_ref_matches_float64_matmul():
    g = torch.Generator().manual_seed(0)
    A, W = R.rand_int(g, (65, 72), 4), R.rand_int(g, (23, 72), 4)
    bias, res = R.rand_int(g, (23,), 64), R.rand_int(g, (65, 23), 64)
    for b, r in ((bias, res), (None, res), (bias, None)):
        for act in (R.ACT_NONE, R.ACT_RELU):
            got, mag = R.gemm_int_ref(A, W, b, r, act)
            x = torch.matmul(A.double(), W.double().T) + (0 if b is None else b.double())
            x = F.relu(x) if act == R.ACT_RELU else x
            x = x + (0 if r is None else r.double())
            assert torch.equal(got.double(), x)
            assert got.abs().max() <= mag <= 16 * 72 + 128


def test_to_bf16_once_on_half_way_cases():
    """Integers whose bf16 neighbours are 2, 4, ... 128 apart, including every exact tie (to even, both parities), the
    values next to a tie, a carry into the next binade, negatives and zero."""
    vals = [0, 1, -1, 255, 256, 257, 258, 259, 260, 261, 262, 263, 264, 510, 511, 512, 513, 514, 515, 516, 518, 1020,
            1022, 1023, 1024, 1026, 1028, 1030, 1032, 9343, 9344, 9408, 9472, 65280, 65408, 65472, 65535, 16777215]
    x = torch.tensor(vals + [-v for v in vals] + list(range(-9500, 9501)), dtype=torch.int64)
    assert torch.equal(R.to_bf16_once(x), x.to(torch.float32).to(torch.bfloat16))
    assert float(R.to_bf16_once(torch.tensor([257]))[0]) == 256.0 and float(R.to_bf16_once(torch.tensor([259]))[0]) == 260.0
    assert float(R.to_bf16_once(torch.tensor([258]))[0]) == 258.0   # representable: 8 significand bits
    assert float(R.to_bf16_once(torch.tensor([513]))[0]) == 512.0 and float(R.to_bf16_once(torch.tensor([514]))[0]) == 512.0
    assert float(R.to_bf16_once(torch.tensor([518]))[0]) == 520.0   # tie 518 between 516 and 520: to even (520 = 130 * 4)
    with pytest.raises(AssertionError):
        R.to_bf16_once(torch.tensor([2 ** 24 + 1]))


def _conv_direct(x, w, bias, res, stride, relu_in, act):
    """The convolution as seven loops over (b, oy, ox, co, dy, dx, ci) in int64 numpy, NHWC out."""
    x, w = np.asarray(x, np.int64), np.asarray(w, np.int64)
    B, Cin, H, W = x.shape
    Cout, _, ks, _ = w.shape
    pad = ks // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    out = np.zeros((B, Ho, Wo, Cout), np.int64)
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for co in range(Cout):
                    s = int(bias[co])
                    for dy in range(ks):
                        for dx in range(ks):
                            iy, ix = oy * stride - pad + dy, ox * stride - pad + dx
                            if 0 <= iy < H and 0 <= ix < W:
                                for ci in range(Cin):
                                    v = int(x[b, ci, iy, ix])
                                    s += (max(v, 0) if relu_in else v) * int(w[co, ci, dy, dx])
                    s = max(s, 0) if act == R.ACT_RELU else s
                    out[b, oy, ox, co] = s + (0 if res is None else int(res[b, oy, ox, co]))
    return out


@pytest.mark.parametrize("stride", [1, 2])
def test_conv_ref_matches_direct_loops(stride):
    g = torch.Generator().manual_seed(3)
    B, H, W, Cin, Cout, ks = 1, 5, 7, 8, 8, 3
    x, w = R.rand_int(g, (B, Cin, H, W), 4), R.rand_int(g, (Cout, Cin, ks, ks), 4)
    bias = R.rand_int(g, (Cout,), 64)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = R.rand_int(g, (B, Ho, Wo, Cout), 64)
    for relu_in in (0, 1):
        for act in (R.ACT_NONE, R.ACT_RELU):
            for r in (res, None):
                got = R.conv_ref(x, w, bias, r, stride, relu_in, act)
                want = _conv_direct(x.numpy(), w.numpy(), bias.numpy(), None if r is None else r.numpy(), stride, relu_in, act)
                assert got.shape == want.shape and np.array_equal(got.numpy(), want.astype(np.float64))


def test_gemm_f64_ref_bound_admits_an_fp32_kernel():
    """A correct kernel in the kernel's formats - fp32 accumulation in another order (torch's), fp32 epilogue with the
    library's erf GELU, one bf16 rounding - stays inside the derived bound; a result with one K chunk of 8 dropped does
    not."""
    g = torch.Generator().manual_seed(1)
    M, N, K = 129, 136, 200
    A = (torch.rand(M, K, generator=g) * 2 - 1).to(torch.bfloat16)
    W = ((torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
    bias, res = torch.rand(N, generator=g) - 0.5, torch.rand(M, N, generator=g)
    for act in (R.ACT_NONE, R.ACT_GELU, R.ACT_RELU):
        for out_bf16 in (0, 1):
            ref, bound = R.gemm_f64_ref(A, W, bias, res, act, out_bf16)

            def emulate(Ae):
                x = Ae.float() @ W.float().T + bias
                x = F.gelu(x) if act == R.ACT_GELU else (F.relu(x) if act == R.ACT_RELU else x)
                x = x + res
                return (x.to(torch.bfloat16) if out_bf16 else x).double()

            assert bool(((emulate(A) - ref).abs() <= bound).all())
            if act == R.ACT_NONE:
                cut = A.clone()
                cut[:, K - 8:] = 0
                assert not bool(((emulate(cut) - ref).abs() <= bound).all())


@pytest.mark.parametrize("kind", ["leak", "spike"])
def test_attention_bound_admits_the_emulated_kernel(kind):
    """fp32 scores, bf16 P, fp32 accumulation, bf16 output on the very inputs of the GPU test: the error peaks at about
    half the bound, so the bound admits a correct kernel - while one zero-filled padded key taking part (`leak`) or one
    dropped key breaks it."""
    worst = 0.0
    for B, H, nq, nk in R.ATTN_SHAPES:
        q, k, v = R.attention_inputs(B, H, nq, nk, kind)
        ref, pabs, smax = R.attention_ref(q, k, v)
        bound = R.attention_bound(ref, pabs)
        ratio = float(((R.attention_emulate(q, k, v).double() - ref).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (B, H, nq, nk, ratio)
        if kind == "leak":
            assert smax <= -8.0
            zk, zv = torch.zeros(B, H, 1, 64, dtype=torch.bfloat16), torch.zeros(B, H, 1, 64, dtype=torch.bfloat16)
            leaked = R.attention_emulate(q, torch.cat([k, zk], 2), torch.cat([v, zv], 2)).double()
            assert not bool(((leaked - ref).abs() <= bound).all())
        if nk > 8:
            dropped = R.attention_emulate(q, k[:, :, :-1], v[:, :, :-1]).double()
            assert not bool(((dropped - ref).abs() <= bound).all())
    print(f"attention emulation, {kind}: worst err/bound {worst:.3f}")


def test_layernorm_bound_admits_two_pass_fp32_and_rejects_one_pass():
    g = torch.Generator().manual_seed(2)
    for D in (8, 63, 65, 100, 768, 1024, 2048):
        w, b = torch.rand(D, generator=g) + 0.5, torch.rand(D, generator=g) - 0.5
        rows = {"random": torch.randn(7, D, generator=g) * 3 + 0.5,
                "constant": (torch.rand(7, 1, generator=g) * 6 - 3).expand(7, D).contiguous(),
                "offset": 1000.0 + torch.randn(7, D, generator=g)}
        for kind, x in rows.items():
            ref, bound = R.layernorm_ref(x, w, b, 1e-6, False)
            mean = x.mean(1, keepdim=True)
            d = x - mean
            y = d * torch.rsqrt((d * d).mean(1, keepdim=True) + 1e-6) * w + b
            assert bool(((y.double() - ref).abs() <= bound).all()), (D, kind)
            refb, boundb = R.layernorm_ref(x, w, b, 1e-6, True)
            assert bool(((y.to(torch.bfloat16).double() - refb).abs() <= boundb).all()), (D, kind)
            if kind == "offset" and D >= 63:
                var1 = ((x * x).mean(1, keepdim=True) - mean * mean).clamp_min(0.0)
                y1 = d * torch.rsqrt(var1 + 1e-6) * w + b
                assert not bool(((y1.double() - ref).abs() <= bound).all()), D
                assert float(bound.max()) < 5e-3


def test_guarded_buffer_sees_stray_writes_and_unwritten_elements():
    dev = torch.device("cpu")
    for dtype in (torch.bfloat16, torch.float32):
        src = torch.arange(15, dtype=torch.float32).reshape(3, 5)
        a, o = R.Guarded(dev, dtype, src=src), R.Guarded(dev, dtype, (3, 5))
        assert a.raw.numel() * a.raw.element_size() == 2 * R.GUARD_BYTES + 15 * a.raw.element_size()
        assert torch.equal(a.t.float(), src) and bool(torch.isnan(o.t.float()).all())
        assert bool(torch.isnan(a.raw.view(dtype)[:a.g].float()).all()) and R.GUARD_BYTES % 256 == 0
        R.check_guards({"a": a, "o": o}, [], "fresh")
        with pytest.raises(AssertionError, match="o has unwritten"):
            R.check_guards({"a": a, "o": o}, ["o"], "unwritten")
        o.t[:] = 1.0
        o.t[2, 4] = float("nan")      # a computed NaN is not the pattern
        R.check_guards({"a": a, "o": o}, ["o"], "written")
        o.raw[o.g + o.n] = 0          # first word behind
        with pytest.raises(AssertionError, match="guard of o"):
            R.check_guards({"a": a, "o": o}, ["o"], "behind")
        o.refill()
        a.raw[a.g - 1] = 0            # last word in front
        with pytest.raises(AssertionError, match="guard of a"):
            R.check_guards({"a": a, "o": o}, [], "front")


# ======================================================================================================================
# References of the forward's glue (tests/test_forward_glue_gpu.py).  Each one: against an independent statement of the
# operation, its bound against a correct fp32 emulation in the kernel's number formats (no more than about half of the
# part of the bound that precedes the bf16 rounding; the whole bound with it), and against one named mutation each.
# ======================================================================================================================
def _inside(got, ref, bound):
    return bool(((got.double() - ref).abs() <= bound).all())


def _ratio(got, ref, bound):
    err = (got.double() - ref).abs()
    return float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())


def _rope_emulate(length):
    """the table loop with correctly rounded fp32 functions (what a good libm's powf / cosf / sinf return in all but rare
    cases): every operation evaluated in float64 and rounded to fp32 once"""
    import math

    inv_freq = np.array([np.float32(1.0) / np.float32(math.pow(100.0, float(np.float32(2 * i) / np.float32(32.0))))
                         for i in range(16)], dtype=np.float32)
    ang = (np.arange(length, dtype=np.float32)[:, None] * inv_freq[None]).astype(np.float32)
    return (torch.from_numpy(np.cos(ang.astype(np.float64)).astype(np.float32)),
            torch.from_numpy(np.sin(ang.astype(np.float64)).astype(np.float32)))


def test_rope_tables_ref_and_bound():
    c, s, bc, bs = R.rope_tables_ref(1024)
    # independent statement: mpmath-free, the angle in float64 from the exact rational exponent
    p = torch.arange(1024, dtype=torch.float64)[:, None]
    ang = p * 100.0 ** (-torch.arange(16, dtype=torch.float64) / 16.0)[None]
    assert float((c - ang.cos()).abs().max()) <= 1024 * 2.0 ** -23 and float((s - ang.sin()).abs().max()) <= 1024 * 2.0 ** -23
    assert float(bs[0].max()) == 0.0 and float(bc.max()) < 3e-4
    ec, es = _rope_emulate(1024)
    assert _ratio(ec, c, bc) <= 0.5 and _ratio(es, s, bs) <= 0.5, (_ratio(ec, c, bc), _ratio(es, s, bs))
    # mutations: base 10000 (the 1-D RoPE default), cos and sin exchanged
    ang_m = p * 10000.0 ** (-torch.arange(16, dtype=torch.float64) / 16.0)[None]
    assert not _inside(ang_m.cos(), c, bc)
    assert not _inside(es, c, bc)


def _attn_case(B, heads, gh, gw, K, seed):
    g = torch.Generator().manual_seed(seed)
    ntok, N = gh * gw, 3 * heads * 64
    A, W, bias = R.rand_int(g, (B * ntok, K), 4), R.rand_int(g, (N, K), 4), R.rand_int(g, (N,), 64)
    pre, mag = R.gemm_int_ref(A, W, bias, None, R.ACT_NONE)
    assert mag < 2 ** 24
    return pre, ntok


def _attn_emulate(pre, B, heads, sec, ntok, tok_w, cos, sin, scale, swap_xy=False, flip=False):
    """fp32 emulation of one RoPE section -> bf16 [B,heads,ntok,64]"""
    x = pre.reshape(B, ntok, heads, 64).permute(0, 2, 1, 3).float()
    n = torch.arange(ntok)
    py, px = n // tok_w, n % tok_w
    if swap_xy:
        py, px = px, py
    c32, s32 = cos.float(), sin.float()
    out = torch.empty_like(x)
    for h, pos in ((0, py), (1, px)):
        a, b = x[..., 32 * h:32 * h + 16], x[..., 32 * h + 16:32 * h + 32]
        c, s = c32[pos], s32[pos]
        if flip:
            s = -s
        out[..., 32 * h:32 * h + 16] = (a * c - b * s) * scale
        out[..., 32 * h + 16:32 * h + 32] = (b * c + a * s) * scale
    return out


def test_attn_project_ref_matches_oracle_rope2d_and_head_split():
    """4 x 6 grid: the q and k of the reference against oracle.mast3r_ref.rope2d on the reference's own head split
    (reshape(B, N, 3, heads, 64).transpose(1, 3)), v^T exact; then the bound: admits the fp32 emulation, rejects the
    mutations."""
    from oracle import mast3r_ref as O

    B, heads, gh, gw = 2, 3, 4, 6
    pre, ntok = _attn_case(B, heads, gh, gw, 64, 5)
    cos, sin = (t.float().double() for t in R.rope_tables_ref(64)[:2])       # fp32 values, as the device's tables are
    ref = R.attn_project_ref(pre, B, heads, 0, ntok, ntok, gw, cos, sin, 0.125)
    qkv = pre.double().reshape(B, ntok, 3, heads, 64).transpose(1, 3)          # [B,heads,3,ntok,64]
    pos = O.positions(B, gh, gw, "cpu")
    for name, j, scale in (("q", 0, 0.125), ("k", 1, 1.0)):
        want = O.rope2d(qkv[:, :, j], pos, 100.0) * scale
        y, f32, bound = ref[name]
        assert y.shape == want.shape
        # rope2d forms its cos / sin in fp32: 2^-24 of |v| + |partner| per term
        assert bool(((y - want).abs() <= 4e-7 * (qkv[:, :, j].abs().max() + 1)).all()), name
    assert torch.equal(ref["vt"].double(), qkv[:, :, 2].transpose(-1, -2)) or \
        torch.equal(ref["vt"], R.to_bf16_once(qkv[:, :, 2].transpose(-1, -2).contiguous()))
    sd = heads * 64
    for name, j, scale in (("q", 0, 0.125), ("k", 1, 1.0)):
        y, f32, bound = ref[name]
        sec = pre[:, j * sd:(j + 1) * sd]
        emu = _attn_emulate(sec, B, heads, j, ntok, gw, cos, sin, scale)
        assert _ratio(emu, y, f32) <= 0.5, (name, _ratio(emu, y, f32))
        assert _inside(emu.to(torch.bfloat16), y, bound), name
        assert not _inside(_attn_emulate(sec, B, heads, j, ntok, gw, cos, sin, scale, swap_xy=True).to(torch.bfloat16), y, bound)
        assert not _inside(_attn_emulate(sec, B, heads, j, ntok, gw, cos, sin, scale, flip=True).to(torch.bfloat16), y, bound)
    # q_scale applied to k
    y, _, bound = ref["k"]
    assert not _inside(_attn_emulate(pre[:, sd:2 * sd], B, heads, 1, ntok, gw, cos, sin, 0.125).to(torch.bfloat16), y, bound)
    # V stored untransposed: the same bytes read as [B,heads,64,ntok] are not the reference
    v_plain = R.to_bf16_once(pre[:, 2 * sd:].reshape(B, ntok, heads, 64).permute(0, 2, 1, 3).contiguous())
    assert not torch.equal(v_plain.reshape(-1), ref["vt"].reshape(-1))
    # side 1 using side 0's bias: another bias is outside the bound / not equal
    g = torch.Generator().manual_seed(6)
    other = R.attn_project_ref(pre + R.rand_int(g, (pre.shape[1],), 64), B, heads, 0, ntok, ntok, gw, cos, sin, 0.125)
    assert not _inside(other["q"][0], ref["q"][0], ref["q"][2]) and not torch.equal(other["vt"], ref["vt"])


def test_attn_project_ref_sections_and_kv_ntok():
    """{k, v} with sec_base 1 and its own token count: the same numbers as sections 1, 2 of the joint call."""
    B, heads = 2, 1
    pre, ntok = _attn_case(B, heads, 4, 6, 64, 7)
    cos, sin = (t.float().double() for t in R.rope_tables_ref(64)[:2])       # fp32 values, as the device's tables are
    full = R.attn_project_ref(pre, B, heads, 0, ntok, ntok, 6, cos, sin, 0.125)
    kv = R.attn_project_ref(pre[:, 64:], B, heads, 1, 32, ntok, 6, cos, sin, 0.125)
    assert set(kv) == {"k", "vt"} and torch.equal(kv["k"][0], full["k"][0]) and torch.equal(kv["vt"], full["vt"])
    q = R.attn_project_ref(pre[:, :64], B, heads, 0, ntok, 32, 6, cos, sin, 0.125)
    assert set(q) == {"q"} and torch.equal(q["q"][0], full["q"][0])


def test_layernorm_group_ref_blocks_and_mutations():
    g = torch.Generator().manual_seed(8)
    M, D, eps = 3, 192, 1e-6
    x = torch.randn(2 * M, D, generator=g) * 3 + 0.5
    sets = {k: (torch.rand(D, generator=g) + 0.5, torch.rand(D, generator=g) - 0.5) for k in ("self0", "self1", "mem0", "mem1")}
    ys, bs, ym, bm = R.layernorm_group_ref(x, sets, M, eps, True)
    ln = lambda rows, k: F.layer_norm(rows.double(), (D,), sets[k][0].double(), sets[k][1].double(), eps)
    assert torch.allclose(ys, torch.cat([ln(x[:M], "self0"), ln(x[M:], "self1")]), rtol=0, atol=1e-12)
    assert torch.allclose(ym, torch.cat([ln(x[M:], "mem0"), ln(x[:M], "mem1")]), rtol=0, atol=1e-12)
    ln32 = lambda rows, k: F.layer_norm(rows, (D,), sets[k][0], sets[k][1], eps).to(torch.bfloat16)
    assert _inside(torch.cat([ln32(x[:M], "self0"), ln32(x[M:], "self1")]), ys, bs)
    assert _inside(torch.cat([ln32(x[M:], "mem0"), ln32(x[:M], "mem1")]), ym, bm)
    # norm_y written to its own side's block; side 1 with side 0's affine pair
    assert not _inside(torch.cat([ln32(x[:M], "mem1"), ln32(x[M:], "mem0")]), ym, bm)
    assert not _inside(torch.cat([ln32(x[:M], "self0"), ln32(x[M:], "self0")]), ys, bs)
    y1, b1, none1, none2 = R.layernorm_group_ref(x, sets, M, eps, False)
    assert torch.equal(y1, ys) and none1 is None and none2 is None


@pytest.mark.parametrize("s", [2, 4])
def test_conv_transpose_ref_matches_torch(s):
    g = torch.Generator().manual_seed(9 + s)
    B, H, W, Cin, Cout = 2, 3, 5, 8, 6
    x, w, bias = R.rand_int(g, (B, Cin, H, W), 4), R.rand_int(g, (Cin, Cout, s, s), 4), R.rand_int(g, (Cout,), 64)
    got = R.conv_transpose_ref(x, w, bias)
    want = F.conv_transpose2d(x.double(), w.double(), bias.double(), stride=s).permute(0, 2, 3, 1)
    assert torch.equal(got, want)
    # the GEMM form with the kernel's row order co*s*s + i*s + j, scattered by hand
    Wm = R.conv_transpose_weight(w)
    assert Wm.shape == (Cout * s * s, Cin)
    flat = x.permute(0, 2, 3, 1).reshape(-1, Cin).double() @ Wm.double().T       # [B*H*W, Cout*s*s]
    out = torch.zeros_like(got)
    for n in range(Cout * s * s):
        co, i, j = n // (s * s), (n % (s * s)) // s, n % s
        out[:, i::s, j::s, co] = flat[:, n].reshape(B, H, W) + float(bias[co])
    assert torch.equal(out, got)
    # mutation: sub-pixels (i, j) exchanged
    assert not torch.equal(R.conv_transpose_ref(x, w.transpose(2, 3), bias), got)


def test_conv_ref_second_residual():
    g = torch.Generator().manual_seed(10)
    x, w, bias = R.rand_int(g, (1, 8, 5, 7), 4), R.rand_int(g, (8, 8, 3, 3), 4), R.rand_int(g, (8,), 64)
    r1, r2 = R.rand_int(g, (1, 5, 7, 8), 64), R.rand_int(g, (1, 5, 7, 8), 64)
    for relu_in in (0, 1):
        base = _conv_direct(x.numpy(), w.numpy(), bias.numpy(), None, 1, relu_in, R.ACT_NONE)
        for a, b in ((r1, r2), (r1, None), (None, r2)):
            want = base + (0 if a is None else a.numpy()) + (0 if b is None else b.numpy())
            assert np.array_equal(R.conv_ref(x, w, bias, a, 1, relu_in, R.ACT_NONE, res2=b).numpy(), want.astype(np.float64))


def _upsample_emulate(x):
    """the kernel's arithmetic in fp32 torch: fp32 scale, coordinate, floor, three lerps"""
    v = x.float()
    B, H, W, C = v.shape

    def axis(n):
        no = 2 * n
        sc = torch.tensor(float(n - 1)) / torch.tensor(float(no - 1)) if no > 1 else torch.tensor(0.0)
        f = sc * torch.arange(no, dtype=torch.float32)
        i0 = f.long().clamp_max(n - 1)
        return i0, (i0 + 1).clamp_max(n - 1), f - i0
    y0, y1, wy = axis(H)
    x0, x1, wx = axis(W)
    g = lambda yi, xi: v[:, yi][:, :, xi]
    wx_, wy_ = wx[None, None, :, None], wy[None, :, None, None]
    top = g(y0, x0) + wx_ * (g(y0, x1) - g(y0, x0))
    bot = g(y1, x0) + wx_ * (g(y1, x1) - g(y1, x0))
    return top + wy_ * (bot - top)


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 8), (1, 1, 5, 8), (2, 3, 5, 24), (3, 7, 2, 136), (1, 12, 16, 256)])
def test_upsample2x_ref_matches_interpolate(B, H, W, C):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = (torch.randn(B, H, W, C, generator=g) * 2).to(torch.bfloat16)
    y, f32, bound = R.upsample2x_ref(x)
    nchw = x.double().permute(0, 3, 1, 2)
    want = F.interpolate(nchw, scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    assert float((y - want).abs().max()) <= 1e-12
    emu = _upsample_emulate(x)
    assert _ratio(emu, y, f32) <= 0.5, _ratio(emu, y, f32)
    assert _inside(emu.to(torch.bfloat16), y, bound)
    if H * W > 1:
        wrong = F.interpolate(nchw, scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        assert not _inside(wrong.float().to(torch.bfloat16), y, bound)
    const = torch.full((B, H, W, C), 1.2345).to(torch.bfloat16)
    yc, f32c, bc = R.upsample2x_ref(const)
    assert torch.equal(yc, const.double().expand(B, 1, 1, C).expand(B, 2 * H, 2 * W, C) if H * W == 1 else
                       const.double()[:, :1, :1].expand(B, 2 * H, 2 * W, C))


def _head_emulate(feat, w4, b4, lf, desc, P, swap_ij=False, no_one=False):
    B, H, W, fc = feat.shape
    l = feat.float() @ w4.T + b4
    d = l[..., :3].norm(dim=-1, keepdim=True)
    X = l[..., :3] * (torch.expm1(d) / d.clamp_min(1e-8))
    C = torch.exp(l[..., 3]) + (0.0 if no_one else 1.0)
    lfv = lf[:, :(desc + 1) * P * P]
    if swap_ij:
        lfv = lfv.reshape(-1, desc + 1, P, P).transpose(2, 3).reshape(lf.shape[0], -1)
    sh = R.pixel_shuffle_lf(lfv, B, H, W, P, desc + 1)
    v = sh[..., :desc]
    return {"X": X, "C": C, "D": v / v.norm(dim=-1, keepdim=True), "Q": torch.exp(sh[..., desc])}


@pytest.mark.parametrize("P,fc,desc,B,H,W,pad", [(16, 128, 24, 1, 16, 16, 0), (8, 64, 16, 1, 16, 24, 5)])
def test_head_post_ref_matches_pixel_shuffle_and_formulas(P, fc, desc, B, H, W, pad):
    lf_ld = (desc + 1) * P * P + pad
    feat, w4, b4, lf = R.head_inputs(B, H, W, P, fc, desc, lf_ld, 11)
    ref = R.head_post_ref(feat, w4, b4, lf, desc, P)
    # independent statement: F.pixel_shuffle on the NCHW token map + the post-process formulas of the oracle
    nh, nw = H // P, W // P
    tokmap = lf[:, :(desc + 1) * P * P].double().reshape(B, nh, nw, -1).permute(0, 3, 1, 2)
    sh = F.pixel_shuffle(tokmap, P).permute(0, 2, 3, 1)
    l = F.conv2d(feat.double().permute(0, 3, 1, 2), w4.double()[:, :, None, None], b4.double()).permute(0, 2, 3, 1)
    d = l[..., :3].norm(dim=-1, keepdim=True)
    assert torch.allclose(ref["X"][0], l[..., :3] / d.clip(min=1e-8) * torch.expm1(d), rtol=1e-12, atol=1e-300)
    assert torch.allclose(ref["C"][0], 1 + l[..., 3].exp(), rtol=1e-12)
    assert torch.allclose(ref["D"][0], sh[..., :desc] / sh[..., :desc].norm(dim=-1, keepdim=True), rtol=1e-12)
    assert torch.allclose(ref["Q"][0], sh[..., desc].exp(), rtol=1e-12)
    assert float(d.max()) > 6.0 and float(l[..., 3].abs().max()) > 12.0
    zx, zb = ref["X"][0][0, 1 % H, 2 % W], ref["X"][1][0, 1 % H, 2 % W]
    assert float(zx.abs().max()) == 0.0 and float(zb.max()) == 0.0
    emu = _head_emulate(feat, w4, b4, lf, desc, P)
    for k in ("X", "C", "D", "Q"):
        y, bound = ref[k]
        assert _inside(emu[k], y, bound), k
        # where e^l3 < 1 the bound of C is little more than the one rounding of the final sum (half an ulp of C), which
        # a correct kernel reaches: the half-of-the-bound check is made where the propagated terms lead
        sel = ref["C"][0] >= 2.0 if k == "C" else torch.ones_like(y, dtype=torch.bool)
        assert _ratio(emu[k][sel], y[sel], bound[sel]) <= 0.5, (k, _ratio(emu[k][sel], y[sel], bound[sel]))
    assert bool(torch.isfinite(emu["X"]).all()) and float(emu["X"][0, 1 % H, 2 % W].abs().max()) == 0.0
    # mutations: sub-pixel (i, j) exchanged; conf without the 1 +
    sw = _head_emulate(feat, w4, b4, lf, desc, P, swap_ij=True)
    assert not _inside(sw["D"], *ref["D"]) and not _inside(sw["Q"], *ref["Q"])
    assert not _inside(_head_emulate(feat, w4, b4, lf, desc, P, no_one=True)["C"], *ref["C"])


@pytest.mark.parametrize("P,B,H,W", [(16, 1, 16, 16), (8, 2, 8, 24)])
def test_patchify_ref_matches_unfold(P, B, H, W):
    g = torch.Generator().manual_seed(12)
    img = torch.randn(B, 3, H, W, generator=g)
    want = F.unfold(img, P, stride=P).transpose(1, 2).reshape(-1, 3 * P * P)     # columns in Conv2d weight order
    assert torch.equal(R.patchify_ref(img, P), want.to(torch.bfloat16))


def test_cast_edge_values_cover_ties_zeros_and_carry():
    x = R.cast_edge_values(1025, torch.Generator().manual_seed(13))
    assert bool(torch.isfinite(x).all()) and x.unique().numel() >= 1024
    want = R.to_bf16_once(x)
    assert torch.equal(want, x.to(torch.bfloat16))
    b = want.view(torch.int16).to(torch.int64) & 0xFFFF
    assert b[:3].tolist() == [0x3F80, 0x3F82, 0x3F80]       # tie down to even, tie up to even, carry into the next binade
    assert b[6:8].tolist() == [0x0000, 0x8000] and bool(torch.isfinite(want.float()).all())
