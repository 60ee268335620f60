"""Plain torch references and the guarded-buffer harness of tests/test_kernel_edges_gpu.py: the four building blocks of
the MASt3R forward (csrc/gemm_kernel.h + gemm8p.hip, the implicit-im2col view of the same kernel, attention.hip, the
LayerNorm kernels of mast3r.hip) stated once in int64 / float64 on the CPU, each with the per-element error bound its
test asserts.  Nothing here touches the device except Guarded, which allocates where it is told to; the references and
the bounds are checked on their own in tests/test_kernel_refs_cpu.py."""
import math

import torch
import torch.nn.functional as F

# NaN bit patterns the guards and the not-yet-written outputs are filled with (sign 0, exponent all ones, mantissa != 0);
# neither is the canonical quiet NaN an instruction produces, so "still holds the pattern" means "never stored".
NAN_BITS = {torch.bfloat16: 0x7FDE, torch.float32: 0x7FD5A5A5}
_INT_VIEW = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
GUARD_BYTES = 4096   # in front and behind; a multiple of 256, so the interior stays 16-byte aligned

ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
U23 = 2.0 ** -23


class Guarded:
    """A tensor of `shape` inside a larger allocation: GUARD_BYTES of NaN pattern in front and behind, the interior either
    a copy of `src` (an input) or the same pattern (an output).  guards_ok(): the guards are bit-identical to what was
    written; all_written(): no interior element still holds the pattern.  Both return 0-d bool tensors on the device."""

    def __init__(self, device, dtype, shape=None, src=None):
        if src is not None:
            shape = tuple(src.shape)
        self.n = int(math.prod(shape))
        self.g = GUARD_BYTES // torch.empty((), dtype=dtype).element_size()
        self.pat = NAN_BITS[dtype]
        self.raw = torch.full((self.n + 2 * self.g,), self.pat, dtype=_INT_VIEW[dtype], device=device)
        self.t = self.raw[self.g:self.g + self.n].view(dtype).view(shape)
        assert self.t.data_ptr() % 16 == 0
        if src is not None:
            self.t.copy_(src.to(dtype))

    def refill(self):
        self.raw.fill_(self.pat)
        return self

    def guards_ok(self):
        return (self.raw[:self.g] == self.pat).all() & (self.raw[self.g + self.n:] == self.pat).all()

    def all_written(self):
        return (self.raw[self.g:self.g + self.n] != self.pat).all()


def check_guards(bufs, outs, what):
    """bufs: {name: Guarded} of every operand of a launch, outs: the names that the launch must have written in full.
    One device->host transfer for all flags."""
    names = list(bufs)
    flags = [bufs[k].guards_ok() for k in names] + [bufs[k].all_written() for k in outs]
    flags = torch.stack(flags).tolist()
    bad = [f"guard of {k} changed" for k, ok in zip(names, flags) if not ok]
    bad += [f"{k} has unwritten elements" for k, ok in zip(outs, flags[len(names):]) if not ok]
    assert not bad, f"{what}: {', '.join(bad)}"


# ---- bf16 ------------------------------------------------------------------------------------------------------------
def to_bf16_once(x):
    """Round-to-nearest-even to bf16 of values that float32 holds exactly (integers below 2^24 in the exact tests), done
    on the bit pattern: add 0x7FFF plus the lowest kept bit, drop the low half.  One rounding, no library cast."""
    f = x.to(torch.float32)
    assert torch.equal(f.to(x.dtype), x), "to_bf16_once: value not exact in float32"
    bits = f.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16
    bits = torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16)
    return bits.view(torch.bfloat16)


def rand_int(g, shape, lim):
    """Uniform integers in [-lim, lim] as int64."""
    return torch.randint(-lim, lim + 1, shape, generator=g, dtype=torch.int64)


# ---- GEMM: out = act(A W^T + bias) + residual -----------------------------------------------------------------------
def gemm_int_ref(A, W, bias, res, act):
    """int64 statement of mslam_gemm_bf16 for integer operands: A [M,K], W [N,K], bias [N] or None, res [M,N] or None,
    act in {ACT_NONE, ACT_RELU}.  Returns (result int64 [M,N], largest sum of magnitudes met on the way): while that is
    below 2^24 every product, partial sum and epilogue value is an integer float32 holds, whatever the order."""
    assert act in (ACT_NONE, ACT_RELU)
    x = A @ W.T
    mag = A.abs() @ W.abs().T
    if bias is not None:
        x = x + bias
        mag = mag + bias.abs()
    if act == ACT_RELU:
        x = x.clamp_min(0)
    if res is not None:
        x = x + res
        mag = mag + res.abs()
    return x, int(mag.max())


def gelu_f64(x):
    return 0.5 * x * (1.0 + torch.special.erf(x / math.sqrt(2.0)))


def gemm_f64_ref(A, W, bias, res, act, out_bf16):
    """float64 statement of mslam_gemm_bf16 on bf16-rounded A [M,K], W [N,K] and f32 bias [N], res [M,N]; returns
    (y, bound), both float64 [M,N], with |kernel - y| <= bound per element.  Derivation of the bound:

      accumulation  the K products a_k w_k are exact in fp32 (8 x 8 significand bits); K additions in any order, each
                    rounded (or, in the matrix core, possibly truncated: 2^-23 per step instead of 2^-24), leave at
                    most K 2^-23 S with S = sum_k |a_k| |w_k|
      bias add      one fp32 addition: 2^-23 (|acc| + |bias|)
      activation    ReLU is 1-Lipschitz and exact.  GELU is 1.13-Lipschitz (max |GELU'| = 1.129), so the error so far
                    is scaled by 1.13; its evaluation (csrc/gemm_kernel.h gelu_erf: Abramowitz-Stegun 7.1.26, |error|
                    <= 1.5e-7 on erf, one rcp, one exp2, 8 fma) adds |x| (1.5e-7 + 4 2^-23)
      residual add  one fp32 addition: 2^-23 (|act(x)| + |res|)
      bf16 output   2^-8 |y| (the unit roundoff of bf16, 8 significand bits: reached at the foot of a binade)"""
    A, W, bias, res = A.double(), W.double(), bias.double(), res.double()
    K = A.shape[1]
    acc = A @ W.T
    S = A.abs() @ W.abs().T
    x = acc + bias
    err = K * U23 * S + U23 * (acc.abs() + bias.abs())
    if act == ACT_GELU:
        a = gelu_f64(x)
        err = 1.13 * err + x.abs() * (1.5e-7 + 4 * U23)
    elif act == ACT_RELU:
        a = x.clamp_min(0.0)
    else:
        a = x
    y = a + res
    err = err + U23 * (a.abs() + res.abs())
    if out_bf16:
        err = err + 2.0 ** -8 * y.abs()
    return y, err


# ---- convolution ----------------------------------------------------------------------------------------------------
def conv_ref(x, w, bias, res, stride, relu_in, act):
    """float64 statement of mslam_conv2d_nhwc_bf16: x [B,Cin,H,W], w [Cout,Cin,ks,ks], bias [Cout], res [B,Ho,Wo,Cout] or
    None, zero padding ks // 2; returns float64 [B,Ho,Wo,Cout] (exact for the integer operands of the exact test)."""
    assert act in (ACT_NONE, ACT_RELU)
    x = x.double()
    if relu_in:
        x = x.clamp_min(0.0)
    y = F.conv2d(x, w.double(), bias.double(), stride=stride, padding=w.shape[-1] // 2)
    if act == ACT_RELU:
        y = y.clamp_min(0.0)
    y = y.permute(0, 2, 3, 1)
    if res is not None:
        y = y + res.double()
    return y.contiguous()


# ---- attention ------------------------------------------------------------------------------------------------------
ATTN_SHAPES_SPLIT4 = [(1, 2, 1, 8), (1, 2, 31, 64), (1, 2, 33, 72), (2, 3, 65, 264), (1, 2, 200, 328), (1, 1, 64, 448),
                      (1, 2, 32, 584)]           # (B, heads, nq, nk): 1, 1, 2, 5, 6, 7 and 10 key tiles, <= 256 blocks
ATTN_SHAPES_SPLIT2 = [(3, 11, 520, 264), (3, 11, 520, 72)]   # 297 blocks
ATTN_SHAPES = ATTN_SHAPES_SPLIT4 + ATTN_SHAPES_SPLIT2


def attention_inputs(B, H, nq, nk, kind):
    """bf16 q (pre-scaled by d^-1/2), k, v [B,H,n,64].  `spike`: one key x6 (the online-softmax rescale across tiles).
    `leak`: q[..., 0] = 2 and k[..., 0] = -16 push every real score far below 0, the score of a zero-filled padded
    key, which would then own the softmax if it took part."""
    g = torch.Generator().manual_seed(1000 * nq + nk + B)
    q = (torch.randn(B, H, nq, 64, generator=g) * 0.125 * 1.5).to(torch.bfloat16)
    k = (torch.randn(B, H, nk, 64, generator=g) * 1.5).to(torch.bfloat16)
    v = torch.randn(B, H, nk, 64, generator=g).to(torch.bfloat16)
    if kind == "spike":
        k[0, 0, min(3, nk - 1)] *= 6.0
    else:
        assert kind == "leak"
        q[..., 0] = 2.0
        k[..., 0] = -16.0
    return q, k, v


def _heads_last(o):
    B, H, nq, d = o.shape
    return o.transpose(1, 2).reshape(B, nq, H * d).contiguous()


def attention_ref(q, k, v):
    """float64 softmax(q k^T) v on the bf16 inputs.  Returns (o, pabs, smax): o and pabs = sum_j p_j |v_j| as
    [B, nq, H*64] (the kernel's output layout), smax the largest score."""
    s = q.double() @ k.double().transpose(-1, -2)
    p = torch.softmax(s, -1)
    return _heads_last(p @ v.double()), _heads_last(p @ v.double().abs()), float(s.max())


def attention_bound(o, pabs):
    """|kernel - o| <= 2^-7 sum_j p_j |v_j| + 2^-8 |o| + 1e-6.  To first order the kernel loses at most 2^-8 (relative,
    per probability; 2^-9 on average) where P is rounded to bf16 for the second MFMA and as much of |o| at the bf16
    output; the fp32 terms (scores, exp2, the running sums) are negligible for nk <= 584.  The bound is twice the
    typical loss and above the worst case; tests/test_kernel_refs_cpu.py shows a correct kernel at half of it."""
    return 2.0 ** -7 * pabs + 2.0 ** -8 * o.abs() + 1e-6


def attention_emulate(q, k, v):
    """The kernel's number formats on the CPU: fp32 scores, fp32 softmax sum of the unrounded probabilities, P rounded
    to bf16 for the P V product, fp32 accumulation, bf16 output.  A correct kernel in these formats."""
    s = q.float() @ k.float().transpose(-1, -2)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    l = p.sum(-1, keepdim=True)
    o = (p.to(torch.bfloat16).float() @ v.float()) / l
    return _heads_last(o.to(torch.bfloat16))


# ---- LayerNorm ------------------------------------------------------------------------------------------------------
def layernorm_ref(x, w, b, eps, out_bf16):
    """float64 LayerNorm (biased variance, eps inside the root) of f32 x [rows,D]; returns (y, bound) with
    |kernel - y| <= bound per element.  The kernels are two-pass (mean, then the variance of x - mean), one wave per row:
    a lane adds its D/64 values in sequence, six butterfly steps add the lanes, one division.  With u = 2^-24:

      mean       at most D/64 + 7 roundings, each relative to partial sums bounded by sum |x|:
                 |mean' - mean| <= (D/64 + 7) u mean|x|.  It shifts every x - mean by that much, and y by |w| rstd times
                 it: the first term.  (Its effect on the variance is second order, delta^2 / (var + eps), below 1e-5 of
                 the rounding term's allowance for the rows used.)
      rounding   x - mean', the square and the sum (3 + D/64 + 6 roundings on the variance), / D, + eps, rsqrt (2 ulp):
                 rstd is off by at most (D/128 + 8) u relative; (x - mean') rstd w adds 3 u: together below
                 (D/64 + 16) 2u |y - b|.  The final + b rounds once more: u (|y - b| + |b|), inside 4u |b| plus the
                 slack of the term before.
      bf16 out   2^-8 |y|.

    A one-pass variance E[x^2] - mean^2 misses this bound by orders of magnitude on the offset row (x = 1000 + N(0,1):
    cancellation of 1e6-sized terms at u leaves percents of the variance; the bound there is about 1e-3)."""
    x, w, b = x.double(), w.double(), b.double()
    D = x.shape[1]
    u = 2.0 ** -24
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + eps)
    y = (x - mean) * rstd * w + b
    bound = w.abs() * rstd * (D / 64 + 7) * u * x.abs().mean(1, keepdim=True) + (D / 64 + 16) * 2 * u * (y - b).abs() \
        + 4 * u * b.abs()
    if out_bf16:
        bound = bound + 2.0 ** -8 * y.abs()
    return y, bound
