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
