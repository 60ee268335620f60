"""Plain torch references and the guarded-buffer harness of tests/test_kernel_edges_gpu.py: the four building blocks of
the MASt3R forward (csrc/gemm_kernel.h + gemm8p.hip, the implicit-im2col view of the same kernel, attention.hip, the
LayerNorm kernels of mast3r.hip) stated once in int64 / float64 on the CPU, each with the per-element error bound its
test asserts.  Nothing here touches the device except Guarded, which allocates where it is told to; the references and
the bounds are checked on their own in tests/test_kernel_refs_cpu.py.  The second half holds the same for the glue between
those blocks (tests/test_forward_glue_gpu.py)."""
import math

import torch
import torch.nn.functional as F

# NaN bit patterns the guards and the not-yet-written outputs are filled with (sign 0, exponent all ones, mantissa != 0);
# neither is the canonical quiet NaN an instruction produces, so "still holds the pattern" means "never stored".
NAN_BITS = {torch.bfloat16: 0x7FDE, torch.float16: 0x7D5A, torch.float32: 0x7FD5A5A5, torch.float64: 0x7FF5A5A5A5A5A5A5}
_INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
# Integer outputs have no NaN: guards and unwritten interior hold a sentinel that no result of the kernels under test
# takes (class ids are 0..3, hit flags 0 / 1; a 32-bit signature word equals it with probability 2^-32).
SENTINEL = {torch.int32: 0x5AD5A5A5, torch.int64: 0x5AD5A5A55AD5A5A5, torch.uint8: 0xA5}
GUARD_BYTES = 4096   # in front and behind; a multiple of 256, so the interior stays 16-byte aligned

ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
U23 = 2.0 ** -23


class Guarded:
    """A tensor of `shape` inside a larger allocation: GUARD_BYTES of NaN pattern (integer types: SENTINEL) in front and
    behind, the interior either a copy of `src` (an input) or the same pattern (an output).  guards_ok(): the guards are
    bit-identical to what was written; all_written(): no interior element still holds the pattern.  Both return 0-d bool
    tensors on the device."""

    def __init__(self, device, dtype, shape=None, src=None):
        if src is not None:
            shape = tuple(src.shape)
        self.n = int(math.prod(shape))
        self.g = GUARD_BYTES // torch.empty((), dtype=dtype).element_size()
        self.pat = NAN_BITS[dtype] if dtype in NAN_BITS else SENTINEL[dtype]
        self.raw = torch.full((self.n + 2 * self.g,), self.pat, dtype=_INT_VIEW.get(dtype, dtype), device=device)
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
def conv_ref(x, w, bias, res, stride, relu_in, act, res2=None):
    """float64 statement of mslam_conv2d_nhwc_bf16: x [B,Cin,H,W], w [Cout,Cin,ks,ks], bias [Cout], res [B,Ho,Wo,Cout] or
    None, zero padding ks // 2; returns float64 [B,Ho,Wo,Cout] (exact for the integer operands of the exact test).
    res2: the second residual of mslam_conv2d_res2_nhwc_bf16, added like the first, after the activation."""
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
    if res2 is not None:
        y = y + res2.double()
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


# ======================================================================================================================
# The glue of the forward (tests/test_forward_glue_gpu.py): RoPE / head split, grouped launches, the DPT tail.
# ======================================================================================================================
U24 = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
BF16_U = 2.0 ** -8        # unit roundoff of bf16 relative to the value (reached at the foot of a binade)
# No accuracy table of the device math library (expf, expm1f) or of the host libm (powf, cosf, sinf) ships with the
# toolchain's documentation, so these are ALLOWANCES, not citations: 4 ulp, an ulp being at most 2^-23 of the value.
# sqrtf and the fp32 division are correctly rounded (csrc/Makefile: -fhip-fp32-correctly-rounded-divide-sqrt).
FN_ULP = 4
FN_REL = FN_ULP * U23


# ---- RoPE tables -----------------------------------------------------------------------------------------------------
def rope_tables_ref(length, base=100.0, nfreq=16):
    """cos, sin [length, nfreq] of the RoPE2D angle in the reference model's own order (pos_embed.py:120-130): inv_freq
    and the product p * inv_freq in fp32, cos and sin of that fp32 angle in float64.  Returns (cos, sin, bound_cos,
    bound_sin), each bound per element:

      angle      the library's inv_freq (powf, one division) may differ from torch's by 1 ulp: p 2^-23 inv_freq; both
                 products p * inv_freq are rounded once, half an ulp each: 2^-23 angle.  Together 2 2^-23 angle, and
                 |cos'|, |sin'| <= 1 carry it to the result unscaled
      function   FN_ULP ulp of the result, |result| <= 1: FN_ULP 2^-23 |result|  (an allowance, see FN_ULP)

    p = 0 gives angle 0 and the bound of sin is 0 there: sinf(0) must be exactly 0."""
    i = torch.arange(0, 2 * nfreq, 2, dtype=torch.float32)
    inv_freq = 1.0 / (base ** (i / (2 * nfreq)))
    p = torch.arange(length, dtype=torch.float32)
    ang = torch.einsum("i,j->ij", p, inv_freq)
    assert ang.dtype == torch.float32
    a = ang.double()
    c, s = a.cos(), a.sin()
    return c, s, 2 * U23 * a + FN_REL * c.abs(), 2 * U23 * a + FN_REL * s.abs()


# ---- attention projection: GEMM + RoPE2D + head split ----------------------------------------------------------------
def attn_project_ref(pre, B, heads, sec_base, ntok, kv_ntok, tok_w, cos, sin, q_scale):
    """The EPI_ATTN epilogue on the exact integer pre-activation pre int64 [M, nsec*heads*64] (= A W^T + bias, below 2^24)
    with the table values cos, sin float64 [len,16] the device itself uses.  Section j of the columns is section
    sec_base + j of (q, k, v); rows are B images of ntok (q) or kv_ntok (k, v) tokens.  Returns a dict with

      "vt"        bf16 [B,heads,64,kv_ntok]: the integers rounded once to bf16 and transposed - EXACT
      "q" / "k"   (y, bound) float64 [B,heads,n,64].  Feature f of a head: half = f // 32 chooses the position (0: y =
                  n // tok_w, 1: x = n % tok_w), i = f % 16 the frequency, the partner sits 16 features away inside the
                  half:  y = (v c - partner s) scale for f % 32 < 16,  (v c + partner s) scale otherwise  (rot_half).

    Bound of q / k per element, S = (|v c| + |partner s|) |scale|:
      fp32       v c and partner s rounded (2^-24 each of its own product), their sum rounded (2^-24 S / |scale| at
                 most), the scaling rounded (0.125 is exact, another scale costs 2^-24): at most 4 2^-24 S; a contracted
                 multiply-add only removes roundings
      bf16       one rounding of the fp32 value: 2^-8 (|y| + the fp32 term)."""
    sec_dim = heads * 64
    nsec = pre.shape[1] // sec_dim
    assert pre.shape[1] == nsec * sec_dim and sec_base + nsec <= 3
    out = {}
    for j in range(nsec):
        sec = sec_base + j
        n = ntok if sec == 0 else kv_ntok
        x = pre[:, j * sec_dim:(j + 1) * sec_dim].reshape(B, n, heads, 64).permute(0, 2, 1, 3)   # [B,heads,n,64]
        if sec == 2:
            out["vt"] = to_bf16_once(x).transpose(-1, -2).contiguous()
            continue
        v = x.double()
        tok = torch.arange(n)
        pos = torch.stack((tok // tok_w, tok % tok_w), 0)            # [2, n]: y, x
        f = torch.arange(64)
        half, i, lo = f // 32, f % 16, (f % 32) < 16
        c, s = cos[pos[half], i[:, None]].T, sin[pos[half], i[:, None]].T             # [n, 64]
        partner = v[..., torch.where(lo, f + 16, f - 16)]
        sign = torch.where(lo, -1.0, 1.0).double()
        scale = q_scale if sec == 0 else 1.0
        y = (v * c + sign * partner * s) * scale
        S = ((v * c).abs() + (partner * s).abs()) * abs(scale)
        f32 = 4 * U24 * S
        out["q" if sec == 0 else "k"] = (y, f32, BF16_U * (y.abs() + f32) + f32)
    return out


# ---- LayerNorm of the two stacked decoder sides ----------------------------------------------------------------------
def layernorm_group_ref(x, sets, M, eps, cross):
    """x f32 [2M, D]; sets = {"self0": (w, b), "self1": ..., "mem0": ..., "mem1": ...}.  out_self[row] = self_s(x[row]) for
    row in side s.  cross: out_mem rows [0, M) = mem0 of side 1's rows, rows [M, 2M) = mem1 of side 0's rows (a side's
    memory is the OTHER side's tokens, normalised with the attending side's norm_y).  bf16 output; every block is
    layernorm_ref with its bound.  Returns (y_self, bound_self, y_mem, bound_mem), the last two None without cross."""
    def ln(rows, name):
        return layernorm_ref(rows, sets[name][0], sets[name][1], eps, True)
    a, b = x[:M], x[M:]
    ys = [ln(a, "self0"), ln(b, "self1")]
    y_self, b_self = torch.cat([ys[0][0], ys[1][0]]), torch.cat([ys[0][1], ys[1][1]])
    if not cross:
        return y_self, b_self, None, None
    ym = [ln(b, "mem0"), ln(a, "mem1")]
    return y_self, b_self, torch.cat([ym[0][0], ym[1][0]]), torch.cat([ym[0][1], ym[1][1]])


# ---- ConvTranspose2d, kernel == stride -------------------------------------------------------------------------------
def conv_transpose_ref(x, w, bias):
    """x [B,Cin,H,W], w [Cin,Cout,s,s] (torch's ConvTranspose2d layout), bias [Cout] -> float64 NHWC [B,H*s,W*s,Cout]:
    with kernel == stride the patches do not overlap, out[b, y s + i, x s + j, co] = sum_ci x[b,ci,y,x] w[ci,co,i,j] +
    bias[co].  Exact for the integer operands of the test."""
    B, Cin, H, W = x.shape
    _, Cout, s, _ = w.shape
    y = torch.einsum("bcyx,cdij->byixjd", x.double(), w.double()) + bias.double()
    return y.reshape(B, H * s, W * s, Cout).contiguous()


def conv_transpose_weight(w):
    """[Cin,Cout,s,s] -> the GEMM matrix [Cout*s*s, Cin], row co*s*s + i*s + j."""
    Cin, Cout, s, _ = w.shape
    return w.permute(1, 2, 3, 0).reshape(Cout * s * s, Cin).contiguous()


# ---- bilinear x2, align_corners=True ---------------------------------------------------------------------------------
def _lerp_axis(n, dtype=torch.float64):
    """source coordinate, lower index, upper index and weight of the 2n outputs along an axis of n samples"""
    no = 2 * n
    f = torch.arange(no, dtype=dtype) * ((n - 1) / (no - 1)) if no > 1 else torch.zeros(no, dtype=dtype)
    i0 = f.floor().long().clamp_max(n - 1)
    i1 = (i0 + 1).clamp_max(n - 1)
    return f, i0, i1, f - i0


def upsample2x_ref(x):
    """x bf16 NHWC [B,H,W,C] -> (y, bound) float64 [B,2H,2W,C] of F.interpolate(scale_factor=2, mode='bilinear',
    align_corners=True): output o samples the source at f = o (n-1)/(2n-1), y = lerp_y(lerp_x).  Bound per element:

      weights    the kernel forms f as float(n-1)/float(2n-1) (correctly rounded) times o (rounded): |f' - f| <=
                 2.01 2^-24 f; f' - floor is exact.  Bilinear interpolation is continuous and piecewise linear in f, so
                 the result moves by at most that times the largest difference between vertically (for fy) or
                 horizontally (fx) adjacent samples within one cell of the footprint - also when f' falls on the other
                 side of an integer
      fp32       three lerps a + w (b - a) of values bounded by vmax = the largest of the 4 neighbours: each difference,
                 product and sum rounded, 20 2^-24 vmax in all
      bf16       2^-8 (|y| + the terms above).
    A constant image has all differences 0 and every lerp exact: it must come back bit for bit."""
    v = x.double()
    B, H, W, C = v.shape
    fy, y0, y1, wy = _lerp_axis(H)
    fx, x0, x1, wx = _lerp_axis(W)
    wy_, wx_ = wy[None, :, None, None], wx[None, None, :, None]
    g = lambda yi, xi: v[:, yi][:, :, xi]
    v00, v01, v10, v11 = g(y0, x0), g(y0, x1), g(y1, x0), g(y1, x1)
    top, bot = v00 + wx_ * (v01 - v00), v10 + wx_ * (v11 - v10)
    y = top + wy_ * (bot - top)

    def local_diff(t, dim):       # largest |difference| along `dim` over the cells i-1, i, i+1, indexed by the cell i
        n = t.shape[dim]
        if n == 1:
            return torch.zeros_like(t)
        d = t.diff(dim=dim).abs()
        pad = [0, 0] * (t.dim() - 1 - dim) + [1, 1]
        dp = F.pad(d, pad)
        m = torch.maximum(torch.maximum(dp.narrow(dim, 0, n - 1), dp.narrow(dim, 1, n - 1)), dp.narrow(dim, 2, n - 1))
        return torch.cat([m, m.narrow(dim, n - 2, 1)], dim)          # cell n-1 (the clamped last sample): as n-2
    dy, dx = local_diff(v, 1), local_diff(v, 2)
    gy = torch.maximum(dy[:, y0][:, :, x0], dy[:, y0][:, :, x1])
    gx = torch.maximum(dx[:, y0][:, :, x0], dx[:, y1][:, :, x0])
    vmax = torch.maximum(torch.maximum(v00.abs(), v01.abs()), torch.maximum(v10.abs(), v11.abs()))
    f32 = 2.01 * U24 * (fy[None, :, None, None] * gy + fx[None, None, :, None] * gx) + 20 * U24 * vmax
    return y, f32, BF16_U * (y.abs() + f32) + f32


# ---- tail of a head: 1x1 conv to 4 channels, pixel shuffle, post-processing ------------------------------------------
def pixel_shuffle_lf(lf, B, H, W, P, nch):
    """lf [B*(H/P)*(W/P), ld] -> [B,H,W,nch]: channel c of pixel (y, x) is column c*P*P + (y%P)*P + x%P of its token."""
    nh, nw = H // P, W // P
    t = lf[:, :nch * P * P].reshape(B, nh, nw, nch, P, P)
    return t.permute(0, 1, 4, 2, 5, 3).reshape(B, H, W, nch)


def head_post_ref(feat, w4, b4, lf, desc_dim, P):
    """feat bf16 [B,H,W,fc], w4 f32 [4,fc], b4 f32 [4], lf f32 [tokens, ld].  float64 statement of the tail of a head
    (catmlp_dpt_head.py:25-39, postprocess.py:22-58) and its per-element bounds; returns a dict name -> (y, bound) for X
    [B,H,W,3], C [B,H,W], D [B,H,W,desc_dim], Q [B,H,W].

      l          l_o = b4_o + sum_c w4[o,c] f_c.  A sum of fc + 1 terms in fp32, in any order and with fused
                 multiply-adds or without: |l' - l| <= dl_o = (fc + 1) 2^-24 S_o,  S_o = |b4_o| + sum_c |w4[o,c] f_c|
      X          X_i = l_i g(d), d = |l[0:3]|, g(d) = expm1(d) / max(d, 1e-8), g' = (e^d d - expm1(d)) / d^2.
                 To first order |dX_i| <= g dl_i + |l_i| g' dd with dd <= sum_j |l_j| / d dl_j; the second-order part
                 is smaller by a factor of about dd < 1e-3 (dl is below 129 2^-24 S), covered by the factor 1.001.
                 d itself: three squares and two sums (3 2^-24 relative on d^2), the root halves it and rounds once:
                 2.5 2^-24 d, which moves X_i by |l_i| g' times that.  expm1f FN_ULP ulp, the division and the product
                 with l_i one rounding each: (FN_ULP 2^-23 + 2 2^-24) |X_i|.
                 d = 0 (all l zero, S = 0): X = 0 with bound 0, the kernel's 0 * (0 / 1e-8) is exactly that
      C          1 + e^l3: e^l3 moves by e^l3 (e^dl3 - 1) <= 1.001 e^l3 dl3; expf FN_ULP ulp of e^l3; the sum rounds once
      D          D_c = v_c / |v|: |v|^2 is a sum of desc_dim products (desc_dim 2^-24 relative), the root halves it
                 and rounds once, 1 / . and the product round once each: (desc_dim / 2 + 3) 2^-24 |D_c|
      Q          e^v of an exact input: FN_ULP ulp."""
    B, H, W, fc = feat.shape
    f, w, b = feat.double(), w4.double(), b4.double()
    l = f @ w.T + b                                         # [B,H,W,4]
    S = f.abs() @ w.abs().T + b.abs()
    dl = (fc + 1) * U24 * S
    xyz, dxyz = l[..., :3], dl[..., :3]
    d = xyz.norm(dim=-1, keepdim=True)
    ds = d.clamp_min(1e-300)
    g = torch.where(d > 0, torch.expm1(d) / d.clamp_min(1e-8), torch.ones_like(d))
    gp = torch.where(d > 1e-4, (torch.exp(d) * d - torch.expm1(d)) / (ds * ds), 0.5 + d / 3)
    X = xyz * torch.where(d > 0, torch.expm1(d) / d.clamp_min(1e-8), torch.zeros_like(d))
    dd = (xyz.abs() / ds * dxyz).sum(-1, keepdim=True)
    bX = 1.001 * (g * dxyz + xyz.abs() * gp * dd) + xyz.abs() * gp * 2.5 * U24 * d + (FN_REL + 2 * U24) * X.abs()
    e3 = torch.exp(l[..., 3])
    C = 1.0 + e3
    bC = 1.001 * e3 * dl[..., 3] + FN_REL * e3 + U24 * C
    sh = pixel_shuffle_lf(lf.double(), B, H, W, P, desc_dim + 1)
    v = sh[..., :desc_dim]
    D = v / v.norm(dim=-1, keepdim=True)
    bD = (desc_dim / 2 + 3) * U24 * D.abs()
    Q = torch.exp(sh[..., desc_dim])
    return {"X": (X, bX), "C": (C, bC), "D": (D, bD), "Q": (Q, FN_REL * Q)}


def head_inputs(B, H, W, P, fc, desc, lf_ld, seed, zero_bias=True):
    """feat, w4, b4, lf with d spanning 0 ... about 10 and the conf logit +-20; pixel (0, 1, 2) has an all-zero feature
    row, and the xyz bias is zero, so its point is exactly 0."""
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(B, H, W, fc, generator=g)
    feat = (feat * torch.rand(B, H, W, 1, generator=g)).to(torch.bfloat16)      # per-pixel amplitude in [0, 1)
    feat[0, 1 % H, 2 % W] = 0.0
    w4 = torch.randn(4, fc, generator=g) / fc ** 0.5
    w4[:3] *= 2.5          # d = |l[0:3]| up to about 10
    w4[3] *= 9.0           # conf logit up to about +-20
    b4 = torch.randn(4, generator=g)
    if zero_bias:
        b4[:3] = 0.0
    ntoken = B * (H // P) * (W // P)
    lf = torch.randn(ntoken, lf_ld, generator=g)
    return feat, w4, b4, lf


# ---- patchify ----------------------------------------------------------------------------------------------------
def patchify_ref(img, P):
    """img f32 [B,3,H,W] -> bf16 [B*(H/P)*(W/P), 3*P*P], column c*P*P + ky*P + kx: each pixel rounded once."""
    B, C, H, W = img.shape
    nh, nw = H // P, W // P
    t = img.reshape(B, C, nh, P, nw, P).permute(0, 2, 4, 1, 3, 5).reshape(B * nh * nw, C * P * P)
    return to_bf16_once(t.contiguous())


def cast_edge_values(n, g):
    """n normal finite f32 values with distinct random ones in the bulk and, at the front (as far as n allows), the cases
    a bf16 rounding can get wrong: exact ties of both parities (round to even: down and up), a carry into the next
    binade, the neighbours of a tie, +-0, the largest value that does not overflow."""
    bits = [0x3F808000, 0x3F818000, 0x3F7F8000, 0x3F7FFFFF, 0x3F807FFF, 0x3F808001, 0x00000000, 0x80000000, 0xBF808000,
            0xBF818000, 0x7F7F7FFF, 0x00800000, 0x3FFF8000, 0xC07F8000]
    x = (torch.randn(n, generator=g) * 3).float()
    e = torch.tensor(bits[:n], dtype=torch.int64)
    e = torch.where(e >= 2 ** 31, e - 2 ** 32, e).to(torch.int32).view(torch.float32)
    x[:len(e)] = e
    return x
