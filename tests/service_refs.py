"""Plain CPU references and input recipes of tests/test_service_edges_gpu.py: the kernels around the network -
csrc/retrieval.hip (fp64 GEMM, ASMK aggregation and search), csrc/quality.hip (patch statistics, classification) and
csrc/tsdf_local.hip (local volume build, ray cast) - each stated once in int64 / float32 / float64 on the CPU, with the
inputs that reach the tile, wave and chunk edges of those kernels.  Nothing here touches the device; the references and
the properties the recipes promise are checked on their own in tests/test_service_refs_cpu.py."""
import functools
import math

import numpy as np
import torch

from oracle import asmk_py
from oracle import tsdf_refine_py as TR

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
U24 = 2.0 ** -24

# ======================================================================================================================
# mslam_gemm_f64: out[M,N] = (A - centre) . B (+ bias), exact
# ======================================================================================================================
GEMM_SHAPES = [(1, 1, 1), (63, 65, 31), (64, 64, 32), (65, 63, 33), (5, 129, 4), (130, 70, 100)]   # 64x64 tiles, K by 32
GEMM_LIM = 2 ** 15       # operands, centre and bias are integers in [-2^15, 2^15] times 2^-12


def gemm_cases():
    """[(M, N, K, a_is_f32, b_is_f32, b_transposed, centre, bias)]: every (A, B) type pair with both layouts of B, with
    and without a centre, with and without a bias (three cases per pair), every shape twice."""
    out = []
    for p, (a32, b32) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        for c, (bt, cen, bias) in enumerate(((0, 1, 0), (1, 0, 1), (p & 1, 1, 1))):
            out.append(GEMM_SHAPES[(3 * p + c) % len(GEMM_SHAPES)] + (a32, b32, bt, cen, bias))
    return out


def gemm_exact(case):
    """Operands of one case and the exact result.  With a = A 2^12 etc. the result is ((a - c) . b + bias 2^12) 2^-24:
    int64 arithmetic, converted once.  `mag` = the largest sum of magnitudes in units of 2^-24: while it is below 2^52 every
    product and every partial sum, in any order, is an integer float64 holds."""
    M, N, K, a32, b32, bt, cen, bias = case
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K * 17 + a32 * 8 + b32 * 4 + bt * 2 + cen)
    r = lambda *shape: torch.randint(-GEMM_LIM, GEMM_LIM + 1, shape, generator=g, dtype=torch.int64)
    a, b, c, bi = r(M, K), r(K, N), r(K), r(N)
    a[0, 0], b[0, 0], c[0], bi[0] = GEMM_LIM, -GEMM_LIM, -GEMM_LIM, GEMM_LIM          # the extremes take part
    a[-1, -1], b[-1, -1] = -GEMM_LIM, GEMM_LIM
    ac = a - c if cen else a
    full = ac @ b
    mag = ac.abs() @ b.abs()
    if bias:
        full = full + bi * 2 ** 12
        mag = mag + bi.abs() * 2 ** 12
    s = 2.0 ** -12
    A = (a.double() * s).to(torch.float32 if a32 else torch.float64)
    B = ((b.T.contiguous() if bt else b).double() * s).to(torch.float32 if b32 else torch.float64)
    assert torch.equal(A.double(), a.double() * s) and int(mag.max()) < 2 ** 52
    return dict(A=A, B=B, centre=c.double() * s if cen else None, bias=bi.double() * s if bias else None,
                ref=full.double() * 2.0 ** -24, mag=int(mag.max()))


# ======================================================================================================================
# mslam_asmk_aggregate
# ======================================================================================================================
ASMK_DIMS = (32, 64, 96, 160, 288, 544, 1024)     # 1, 2, 3 (odd), 5 words; a second d0 pass of 32 and of 288 lanes; full
ASMK_NDES = (1, 255, 257, 700)
ASMK_M = (1, 5)
ASMK_NCENT = 24
TRAP_WORD, LONE_WORD = 3, 23
_POOL = np.array([3, 0, 5, 7, 8, 11, 13, 17, 19, 22])
_POOL_P = 0.5 ** np.arange(1, 11) / (0.5 ** np.arange(1, 11)).sum()     # from half of the descriptors to one in 1000
TRAP25 = [2.0 ** 25, 1.0, -2.0 ** 25]          # sequential fp32: 0;  exact: 1
TRAP24 = [2.0 ** 24, 1.0, -2.0 ** 24]          # sequential fp32: 0;  every other association, and exact: 1
TRAP_OPP = [2.0 ** 24, 3.0, -2.0 ** 24, -3.0]  # sequential fp32: 1;  pairwise, reversed and exact: 0


def planted_columns(dim):
    """{name: (column, expected bit of TRAP_WORD)}; columns in the first and in the last signature word."""
    return {"eq": (0, 0), "pair": (1, 0), "trap25": (dim - 3, 0), "trap24": (dim - 2, 0), "opp": (dim - 1, 1)}


def asmk_aggregate_inputs(dim, n_des, m):
    """des f32 [n_des, dim], cent f32 [24, dim], codes i64 [n_des, m], uniq (sorted).  Codes are drawn from ten words with
    probabilities 1/2, 1/4, ...: TRAP_WORD has about half of the descriptors (more with m = 5), the rarest a handful, and
    LONE_WORD exactly one.  With m = 5 rows name a word several times.  In the planted columns every member of TRAP_WORD
    sits on the centroid (residual exactly 0), except the members a < b < c < d that carry the patterns above."""
    rng = np.random.default_rng(7919 * dim + 31 * n_des + m)
    cent = rng.standard_normal((ASMK_NCENT, dim)).astype(F32)
    des = rng.standard_normal((n_des, dim)).astype(F32)
    codes = rng.choice(_POOL, size=(n_des, m), p=_POOL_P).astype(np.int64)
    cols = planted_columns(dim)
    if n_des < 4:
        codes[0, 0] = TRAP_WORD
        des[0] = cent[TRAP_WORD]                # the descriptor IS the centroid: every bit of the word is 0
        return dict(des=des, cent=cent, codes=codes, uniq=np.unique(codes), abcd=None)
    a, b, c, d = 0, n_des // 3, n_des // 2, n_des - 1
    codes[[a, b, c, d], 0] = TRAP_WORD
    codes[2, m - 1] = LONE_WORD
    if m == 5:
        codes[1] = [TRAP_WORD, TRAP_WORD, 5, TRAP_WORD, 5]
    cent[TRAP_WORD, [cols[k][0] for k in ("pair", "trap25", "trap24", "opp")]] = [0.5, 0.0, 0.0, 0.0]
    members = (codes == TRAP_WORD).any(1)
    for col, _ in cols.values():
        des[members, col] = cent[TRAP_WORD, col]
    des[a, cols["pair"][0]], des[c, cols["pair"][0]] = 0.5 + 0.125, 0.5 - 0.125
    for name, pat in (("trap25", TRAP25), ("trap24", TRAP24), ("opp", TRAP_OPP)):
        for f, v in zip((a, b, c, d), pat):
            des[f, cols[name][0]] = v
    return dict(des=des, cent=cent, codes=codes, uniq=np.unique(codes), abcd=(a, b, c, d))


def pack_bits(bits):
    """bool [U, dim] -> uint32 [U, dim/32], the first dimension of a word in its most significant bit."""
    U, dim = bits.shape
    w = (bits.reshape(U, dim // 32, 32).astype(np.uint64) << np.arange(31, -1, -1, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32)


def asmk_aggregate_ref(des, cent, codes):
    """The arithmetic contract of csrc/retrieval.hip as an explicit loop: per word, the float32 residuals of its member
    descriptors (a descriptor that names the word in any of its m assignments, once) added in descriptor order, acc = r for
    the first and acc = float32(acc + r) after; bit = acc > 0.  -> (sig uint32 [U, dim/32], ades f32 [U, dim], uniq)."""
    des, cent = np.ascontiguousarray(des, F32), np.ascontiguousarray(cent, F32)
    uniq = np.unique(codes)
    ades = np.zeros((len(uniq), des.shape[1]), F32)
    for i, word in enumerate(uniq):
        acc = None
        for f in np.nonzero((codes == word).any(axis=1))[0]:
            r = des[f] - cent[word]
            acc = r if acc is None else acc + r
            assert acc.dtype == F32
        ades[i] = acc
    return pack_bits(ades > 0), ades, uniq


def sum_sequential_f32(v):
    acc = F32(v[0])
    for x in v[1:]:
        acc = F32(acc + F32(x))
    return float(acc)


def sum_pairwise_f32(v):
    if len(v) == 1:
        return float(F32(v[0]))
    h = len(v) // 2
    return float(F32(F32(sum_pairwise_f32(v[:h])) + F32(sum_pairwise_f32(v[h:]))))


# ======================================================================================================================
# mslam_asmk_search
# ======================================================================================================================
SEARCH_W = (1, 2, 3, 4, 5, 8, 32)                   # scalar popcount: 1, 2, 3, 5; uint4 loads: 4, 8, 32
SEARCH_NQ = (1, 7, 300)
SEARCH_ENTRIES = (257, 0, 1, 255, 600, 256, 0)      # per image: none, one, around the 256-entry chunk of the block loop
SEARCH_VOCAB, SEARCH_WORDS = 900, 1200              # the file uses words < 900, queries words < 1200
SEARCH_RTOL, SEARCH_ATOL = 2e-7, 1e-13              # the bar of tests/test_retrieval_gpu.py


def _flip(rng, sig, nflip):
    """sig uint32 [W] with `nflip` distinct bits inverted."""
    W = sig.shape[0]
    bits = np.zeros(32 * W, bool)
    bits[rng.permutation(32 * W)[:nflip]] = True
    return sig ^ pack_bits(bits[None])[0]


@functools.lru_cache(maxsize=None)
def search_file(W):
    """A synthetic inverted file as flat arrays: e_word i32 [E] (ascending inside an image), e_sig u32 [E, W], img_start
    i32 [n_img + 1], and `base` u32 [1200, W], the signature a query holds for each word.  An entry is its word's base
    signature with 10-30 % of the bits inverted (sim 0.4 ... 0.8: comparable contributions) or, one in five, with 55-70 %
    inverted (sim < 0: below every threshold >= 0)."""
    rng = np.random.default_rng(1000 + W)
    nb = 32 * W
    base = rng.integers(0, 2 ** 32, (SEARCH_WORDS, W), dtype=np.uint64).astype(np.uint32)
    words, sigs, starts = [], [], [0]
    for k in SEARCH_ENTRIES:
        w = np.sort(rng.choice(SEARCH_VOCAB, k, replace=False))
        for x in w:
            far = rng.random() < 0.2 and k != 1              # the one-entry image always takes part
            lo, hi = (math.ceil(0.55 * nb), math.floor(0.7 * nb)) if far else (math.ceil(0.1 * nb), math.floor(0.3 * nb))
            sigs.append(_flip(rng, base[x], int(rng.integers(lo, hi + 1))))
        words.append(w)
        starts.append(starts[-1] + k)
    return dict(e_word=np.concatenate(words).astype(np.int32), e_sig=np.stack(sigs).astype(np.uint32),
                img_start=np.array(starts, np.int32), base=base, W=W)


def search_query(W, n_q):
    """q_words i32 [n_q] ascending, q_sig u32 [n_q, W]: a quarter of the words are absent from the file (>= 900); the word
    of the one-entry image is always asked for."""
    f = search_file(W)
    rng = np.random.default_rng(77 * W + n_q)
    lone = int(f["e_word"][f["img_start"][2]])
    n_abs = n_q // 4
    rest = np.setdiff1d(np.arange(SEARCH_VOCAB), [lone])
    q = np.concatenate(([lone], rng.choice(rest, n_q - 1 - n_abs, replace=False),
                        rng.choice(np.arange(SEARCH_VOCAB, SEARCH_WORDS), n_abs, replace=False)))
    q = np.sort(q).astype(np.int32)
    assert len(np.unique(q)) == n_q
    return q, f["base"][q]


def make_ivf(e_word, e_sig, img_start):
    """oracle.asmk_py.IVF holding the flat arrays."""
    ivf = asmk_py.IVF(e_sig.shape[1])
    n = np.diff(img_start)
    ivf.words, ivf.vecs = e_word.astype(np.int64), np.ascontiguousarray(e_sig, np.uint32)
    ivf.imids = np.repeat(np.arange(len(n)), n).astype(np.int64)
    ivf.norm_factor, ivf.n_images = n.astype(np.float64), len(n)
    return ivf


def search_oracle(e_word, e_sig, img_start, q_words, q_sig, alpha, thr):
    return make_ivf(e_word, e_sig, img_start).search(np.ascontiguousarray(q_sig, np.uint32), q_words.astype(np.int64),
                                                     alpha, thr)


def popcount32(x):
    return np.unpackbits(np.ascontiguousarray(x, np.uint32).view(np.uint8), axis=-1).sum(-1).astype(np.int64)


def search_terms(e_word, e_sig, img_start, q_words, q_sig, thr):
    """Per entry of the file: (takes part: its word is asked for and sim >= thr, sim float32 = -2 (count / bits) + 1)."""
    pos = np.minimum(np.searchsorted(q_words, e_word), len(q_words) - 1)
    match = q_words[pos] == e_word
    h = popcount32(e_sig ^ q_sig[pos]).astype(F32) / F32(32 * e_sig.shape[1])
    sim = (F32(-2.0) * h + F32(1.0)).astype(F32)
    return match & (sim >= F32(thr)), sim


def search_pow64(e_word, e_sig, img_start, q_words, q_sig, alpha, thr):
    """The search with the power taken in float64 (of the float32 sim) and nothing rounded to float32 after it: the
    reference of the alpha != 3 path.  -> (scores f64 [n_img], contributions f64 [E], 0 where an entry takes no part)."""
    ok, sim = search_terms(e_word, e_sig, img_start, q_words, q_sig, thr)
    n = np.diff(img_start)
    nf = np.repeat(np.sqrt(n.astype(np.float64)), n)
    c = np.where(ok, np.power(np.where(ok, sim, 1).astype(np.float64), float(alpha)) / np.maximum(nf, 1.0), 0.0)
    rq = float(np.sqrt(F32(len(q_words))))
    scores = np.array([c[s:e].sum() for s, e in zip(img_start[:-1], img_start[1:])]) / rq
    return scores, c / rq


def gate_file(W):
    """Three one-entry images of one word and the query of that word: Hamming counts 12 W (sim exactly 0.25), 12 W + 1
    (just below) and 20 W (sim exactly -0.25)."""
    rng = np.random.default_rng(500 + W)
    q = rng.integers(0, 2 ** 32, (1, W), dtype=np.uint64).astype(np.uint32)
    sig = np.stack([_flip(rng, q[0], k) for k in (12 * W, 12 * W + 1, 20 * W)])
    return dict(e_word=np.full(3, 41, np.int32), e_sig=sig, img_start=np.arange(4, dtype=np.int32),
                q_words=np.array([41], np.int32), q_sig=q)


# ======================================================================================================================
# mslam_quality_reduce_grid
# ======================================================================================================================
REDUCE_PS = (1, 2, 3, 5, 8, 14, 16, 31, 32)
C_THR, Q_THR = 2.0, 1.5


def reduce_hw(ps):
    return 3 * ps + 1, 2 * ps + ps // 2


def grid_view(x, ps):
    """[h, w] -> [h // ps, w // ps, ps * ps]: whole patches only, a patch's pixels row by row."""
    h, w = x.shape
    gh, gw = h // ps, w // ps
    return x[:gh * ps, :gw * ps].reshape(gh, ps, gw, ps).permute(0, 2, 1, 3).reshape(gh, gw, ps * ps)


def _nan_to_num(v):
    return torch.nan_to_num(v, nan=0.0)     # also +-inf -> +-FLT_MAX, as in the reference


def reduce_median_ref(x, ps, valid=None):
    """float32: nanmedian of each patch; with a mask, masked pixels count as NaN and the result goes through nan_to_num."""
    X = grid_view(x, ps)
    if valid is None:
        return torch.nanmedian(X, dim=-1).values
    X = X.masked_fill(grid_view(valid.float(), ps) < 0.5, float("nan"))
    return _nan_to_num(torch.nanmedian(X, dim=-1).values)


def reduce_mean_ref(x, ps, valid=None):
    """float64 mean (no mask: of all pixels, NaN included) or nanmean over the valid pixels + nan_to_num, and the bound
    of the kernel's float32 evaluation: a fixed binary tree over 1024 slots (10 levels) and one division, each rounding at
    most 2^-24 of the sum of magnitudes: (ceil(log2 1024) + 2) 2^-24 sum|x| / denom.  -> (mean, bound); where the mean is
    not finite, or was replaced by nan_to_num, the bound is 0: the kernel has to give exactly that."""
    X = grid_view(x, ps).double()
    if valid is None:
        mean = X.mean(-1)
        bound = 12 * U24 * X.abs().sum(-1) / X.shape[-1]
    else:
        X = X.masked_fill(grid_view(valid.float(), ps) < 0.5, float("nan"))
        keep = ~X.isnan()
        cnt = keep.sum(-1)
        Xz = torch.where(keep, X, torch.zeros_like(X))
        raw = Xz.sum(-1) / cnt                                   # 0 / 0 = NaN
        mean = torch.nan_to_num(raw, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX)
        bound = 12 * U24 * Xz.abs().sum(-1) / cnt.clamp_min(1)
    bound = torch.where(mean.isfinite() & (mean.abs() < FLT_MAX) & bound.isfinite(), bound, torch.zeros_like(bound))
    return mean, bound


def reduce_u_ref(C, Q, ps, c_thr=C_THR, q_thr=Q_THR):
    """float32: U = 1 - sqrt(clamp(clamp(C / (C_thr + 1e-8), 0, 1) clamp(Q / (Q_thr + 1e-8), 0, 1), 0, 1)) and its patch
    nanmedian (no mask, no nan_to_num); torch.clamp keeps NaN."""
    Cn = torch.clamp(C / (c_thr + 1e-8), 0, 1)
    Qn = torch.clamp(Q / (q_thr + 1e-8), 0, 1)
    U = 1 - torch.sqrt(torch.clamp(Cn * Qn, 0, 1))
    return torch.nanmedian(grid_view(U, ps), dim=-1).values


def _patch_pixels(ps, py, px):
    """(rows, columns) of the pixels of patch (py, px), row by row."""
    k = torch.arange(ps * ps)
    return py * ps + k // ps, px * ps + k % ps


def reduce_inputs(ps, hw=None):
    """x, C, Q f32 [h, w] and valid bool [h, w] plus their NaN variants.  Patches are numbered row by row; patch p has
    min(p, ps^2) valid pixels for p = 0 .. 3 (scattered, not the first ones), all pixels valid for p = 4, a random half
    after that.  The cropped rows and columns hold NaN, inf and valid flags that must not be read as part of a patch.
      plain  +inf at the only valid pixel of patch 1, -inf in patch 4, +inf at a valid pixel of patch 5
      NaN    one of the three valid pixels of patch 3, a masked pixel of patch 2, a fifth of patch 4, all of patch 5
             (C in patches 3 and 5, Q in patch 4: a pixel is ignored whichever of the two is NaN)"""
    h, w = hw or reduce_hw(ps)
    gh, gw, n = h // ps, w // ps, ps * ps
    g = torch.Generator().manual_seed(100 + ps + h)
    x = torch.randn(h, w, generator=g)
    C = torch.rand(h, w, generator=g) * 3.0 - 0.3             # below 0, inside and above C_thr
    Q = torch.rand(h, w, generator=g) * 2.5 - 0.2
    valid = torch.rand(h, w, generator=g) < 0.5
    xn, Cn, Qn = x.clone(), C.clone(), Q.clone()
    nan, inf = float("nan"), float("inf")
    pix = {}
    for p in range(gh * gw):
        rows, cols = _patch_pixels(ps, p // gw, p % gw)
        perm = torch.randperm(n, generator=g)
        rows, cols = rows[perm], cols[perm]
        if p <= 3:
            valid[rows, cols] = False
            valid[rows[:min(p, n)], cols[:min(p, n)]] = True
        elif p == 4:
            valid[rows, cols] = True
        vi = valid[rows, cols].nonzero().flatten()
        pix[p] = (rows, cols, vi, (~valid[rows, cols]).nonzero().flatten())
    at = lambda p, i: (pix[p][0][i], pix[p][1][i])
    for t in (x, xn, C, Cn):
        if len(pix[1][2]):
            t[at(1, pix[1][2][0])] = inf
        if gh * gw > 4:
            t[at(4, pix[4][2][-1])] = -inf
        if gh * gw > 5 and len(pix[5][2]):
            t[at(5, pix[5][2][0])] = inf
    if gh * gw > 3 and len(pix[3][2]):
        xn[at(3, pix[3][2][0])] = nan
        Cn[at(3, pix[3][2][0])] = nan
    if len(pix[2][3]):
        xn[at(2, pix[2][3][0])] = nan
        Qn[at(2, pix[2][3][0])] = nan
    if gh * gw > 4:
        some = pix[4][2][:max(1, n // 5)]
        xn[at(4, some)] = nan
        Qn[at(4, some)] = nan
    last = min(5, gh * gw - 1)
    xn[pix[last][0], pix[last][1]] = nan
    Cn[pix[last][0], pix[last][1]] = nan
    for t in (x, xn, C, Cn, Q, Qn):                            # what the crop drops
        t[gh * ps:, :] = nan
        t[:gh * ps, gw * ps:] = inf
    valid[gh * ps:, :] = True
    valid[:, gw * ps:] = True
    return dict(h=h, w=w, x=x, x_nan=xn, C=C, C_nan=Cn, Q=Q, Q_nan=Qn, valid=valid, all_nan_patch=last)


# ======================================================================================================================
# mslam_quality_classify
# ======================================================================================================================
CLASSIFY_N = (1, 2, 3, 48, 1023, 1024, 1025, 2500, 4096)
CLASSIFY_KINDS = ("random", "quant", "equal")
THR_ZR, THR_ZU, THR_DC = 1.0, 1.0, 0.02


def classify_inputs(n, kind):
    """delta_cov, r, u f32 [n].  delta_cov straddles THR_DC, every third value exactly equal to it (class 2, not 1).
    quant: r and u take four levels, more than half of them the second: the MAD is 0 and z = (x - m) / 1e-6.
    equal: all three constant."""
    g = torch.Generator().manual_seed(4000 + n)
    dc = torch.rand(n, generator=g) * 0.05
    dc[::3] = THR_DC                                     # rounded to float32 like the kernel's argument
    if kind == "random":
        return dc, torch.rand(n, generator=g), torch.rand(n, generator=g)
    if kind == "quant":
        lv = torch.tensor([0.0, 0.25, 0.5, 0.75])
        pr = torch.tensor([0.1, 0.6, 0.15, 0.15])
        r = lv[torch.multinomial(pr, n, True, generator=g)]
        u = lv[torch.multinomial(pr, n, True, generator=g)]
        if n >= 3:
            r[:2], u[:2] = lv[1], lv[1]                  # small n: keep the majority
        return dc, r, u
    assert kind == "equal"
    return torch.full((n,), 0.01), torch.full((n,), 0.3), torch.full((n,), 0.7)


def lower_median(x):
    return torch.sort(x).values[(x.numel() - 1) // 2]


def classify_ref(dc, r, u, thr_zr=THR_ZR, thr_zu=THR_ZU, thr_dc=THR_DC):
    """float32 on the CPU in the reference's order: z = (x - lower median) / (lower median of |x - m| + 1e-6); classes 1,
    2, 3 assigned in that order (a later one overwrites); the priority of each class; division by max + 1e-6.
    -> (class ids int64 [n], priorities f32 [n])."""
    dc, r, u = dc.float(), r.float(), u.float()

    def z(x):
        m = lower_median(x)
        return (x - m) / (lower_median((x - m).abs()) + 1e-6)

    zr, zu = z(r), z(u)
    assert zr.dtype == torch.float32
    cls = torch.zeros(dc.shape, dtype=torch.int64)
    cls[(dc < thr_dc) & (zu > thr_zu)] = 1
    cls[(dc >= thr_dc) & (zr > thr_zr) & (zu > thr_zu)] = 2
    cls[(zr > thr_zr) & (zu <= thr_zu)] = 3
    zero = torch.zeros_like(r)
    p1 = (1 - dc.clamp(0, 1)) + zu.clamp_min(0)
    p2 = zr.clamp_min(0) + zu.clamp_min(0)
    p3 = zr.clamp_min(0) + (1 - u).clamp_min(0)
    p = torch.where(cls == 1, p1, torch.where(cls == 2, p2, torch.where(cls == 3, p3, zero)))
    return cls, p / (p.max() + 1e-6)


# ======================================================================================================================
# local TSDF (csrc/tsdf_local.hip): oracle/tsdf_refine_py.py with linspace="scalar" on the cases below
# ======================================================================================================================
VOXEL, TRUNC, MIN_CONF, MAX_DISP = 0.02, 0.08, 0.2, 0.015
ROI_MAIN = ([-0.15, -0.09, 0.95], [0.15, 0.09, 1.05])        # 16 x 10 x 5: 0.3 / 0.02 is above 15 in float32
ROI_LONG = ([-0.7, -0.25, 0.99], [0.7, 0.25, 1.01])          # 1.4 x 0.5 x 0.02 -> 64 (capped) x 25 x 1
ROI_TINY = ([-0.029, -0.019, 0.981], [0.029, 0.019, 1.019])  # 3 x 2 x 2
BUILD_CASES = ("main", "long", "tiny", "inside", "four", "five")


def plane_points(rng, n, xr, yr, sigma):
    """n points of the plane z = 1 + 0.1 x with x, y uniform in +-xr, +-yr and N(0, sigma) added to every coordinate."""
    x, y = rng.uniform(-xr, xr, n), rng.uniform(-yr, yr, n)
    return (np.stack([x, y, 1 + 0.1 * x], 1) + rng.normal(0, sigma, (n, 3))).astype(F32)


def _roi(r):
    return np.array(r[0], F32), np.array(r[1], F32)


def build_inputs(name):
    """Xw f32 [n, 3], C f32 [n], origin f32 [3], xyz_min, xyz_max f32 [3] of a build case.
      main    1500 points, a quarter outside the ROI; from index 1400 on: confidence exactly min_confidence (excluded)
              and below it, NaN and inf coordinates, six points exactly on the six ROI faces (included), one point
              closer than 0.05 to the camera
      long    1500 plane points along the capped axis plus 750 inside the slab; the voxel is 1.4 / 64 wide, one z layer
      tiny    600 points in 12 voxels: each voxel replays more than a hundred samples in (point, sample) order
      inside  the camera inside the ROI; five points inside the ROI and closer to it than 0.05 (skipped rays), the
              others start their samples at 0.05
      four / five   exactly 4 / 5 valid points among 40: untouched volume / built volume"""
    rng = np.random.default_rng(sum(map(ord, name)))
    origin = np.zeros(3, F32)
    if name == "long":
        mn, mx = _roi(ROI_LONG)
        X = plane_points(rng, 2250, 0.75, 0.27, 0.003)
        X[1500:, 2] = (1 + rng.uniform(-0.012, 0.012, 750)).astype(F32)    # the plane meets the thin slab only at |x| < 0.1:
        C = rng.uniform(0.25, 1.0, 2250).astype(F32)                       # 750 more points inside it anywhere along x
    elif name == "tiny":
        mn, mx = _roi(ROI_TINY)
        X = plane_points(rng, 600, 0.033, 0.022, 0.003)
        C = rng.uniform(0.25, 1.0, 600).astype(F32)
    elif name == "inside":
        mn, mx = _roi(ROI_MAIN)
        origin = np.array([0.0, 0.0, 0.97], F32)
        X = plane_points(rng, 400, 0.16, 0.1, 0.003)
        X[:5] = origin + rng.uniform(0.005, 0.02, (5, 3)).astype(F32)
        C = rng.uniform(0.25, 1.0, 400).astype(F32)
    elif name in ("four", "five"):
        mn, mx = _roi(ROI_MAIN)
        k = 4 if name == "four" else 5
        X = plane_points(rng, 40, 0.14, 0.08, 0.003)
        C = rng.uniform(0.25, 1.0, 40).astype(F32)
        bad = np.setdiff1d(np.arange(40), [3, 11, 19, 27, 35][:k])
        X[bad[0::3], 0] += 1.0
        C[bad[1::3]] = F32(MIN_CONF)
        X[bad[2::3], 1] = np.nan
    else:
        assert name == "main"
        mn, mx = _roi(ROI_MAIN)
        X = plane_points(rng, 1500, 0.2, 0.12, 0.003)
        C = rng.uniform(0.25, 1.0, 1500).astype(F32)
        X[1400:1440] = plane_points(rng, 40, 0.14, 0.08, 0.003)
        C[1400:1410] = F32(MIN_CONF)
        C[1410:1420] = 0.1
        X[1420:1425, 0] = np.nan
        X[1425:1428, 2] = np.inf
        X[1428:1430, 1] = -np.inf
        for j in range(6):
            X[1430 + j, j % 3] = (mn, mx)[j // 3][j % 3]
        X[1436] = [0.01, 0.01, 0.02]
    return dict(Xw=X, C=C, origin=origin, mn=mn, mx=mx)


@functools.lru_cache(maxsize=None)
def build_case(name):
    """The inputs plus the oracle's result: dims (nx, ny, nz), tsdf, weights f32 [nz, ny, nx], n_valid."""
    d = build_inputs(name)
    nx, ny, nz, _ = TR.grid_dims(d["mn"], d["mx"], VOXEL, 64)
    tsdf, weights = TR.build_tsdf(d["Xw"], d["C"], d["origin"], d["mn"], d["mx"], VOXEL, TRUNC, 64, MIN_CONF, "scalar")
    X, C = d["Xw"], d["C"]
    valid = np.isfinite(X).all(1) & (X >= d["mn"]).all(1) & (X <= d["mx"]).all(1) & (C > F32(MIN_CONF))
    return dict(d, dims=(nx, ny, nz), tsdf=tsdf, weights=weights, n_valid=int(valid.sum()), valid=valid)


def analytic_volume(mn, mx, dims):
    """clip((1 + 0.1 x - z) / 0.08, -1, 1) at the positions min + i * (roi / n) that grid index i stands for."""
    nx, ny, nz = dims
    act = (mx.astype(np.float64) - mn) / np.array(dims)
    x = mn[0] + np.arange(nx) * act[0]
    z = mn[2] + np.arange(nz) * act[2]
    v = np.clip((1 + 0.1 * x[None, None, :] - z[:, None, None]) / 0.08, -1, 1)
    return np.ascontiguousarray(np.broadcast_to(v, (nz, ny, nx)), F32)


def layered_volume(dims):
    """z layers +0.5, +0.5, 0, 0, -0.5: every sample between layers 2 and 3 interpolates to exactly 0, so the pairs
    (+, 0) and (0, -) have products 0 and -0: neither is < 0, and the ray past them only sees (-, -)."""
    nx, ny, nz = dims
    assert nz == 5
    v = np.array([0.5, 0.5, 0.0, 0.0, -0.5], F32)
    return np.ascontiguousarray(np.broadcast_to(v[:, None, None], (nz, ny, nx)), F32)


RAYCAST_CASES = ("sigma4", "sigma30", "built", "zero", "edge_rays", "samples1", "samples2", "sel0", "sel1", "sel63",
                 "sel64", "sel65")


def raycast_inputs(name):
    """vol f32 [nz, ny, nx], mn, mx, X f32 [n, 3], sel_pix i64 [n_sel] (indices into X, not monotone), n_samples.
      sigma4 / sigma30   analytic volume, 400 noisy plane points, 300 of them selected in random order
      built              the volume the oracle builds in case `main` and the first 300 of its points, reversed
      zero               layered_volume: interpolated values of exactly 0
      edge_rays          depth below 0.05 (returned untouched), rays that enter the ROI late, leave it early or never
                         meet it, next to ordinary ones
      samples1 / samples2, sel0 ... sel65   n_samples 1, 2 and n_sel around the 64-thread block on the sigma4 points"""
    mn, mx = _roi(ROI_MAIN)
    dims = TR.grid_dims(mn, mx, VOXEL, 64)[:3]
    rng = np.random.default_rng(sum(map(ord, name)) + 5)
    vol, n_samples = analytic_volume(mn, mx, dims), 64
    if name == "built":
        b = build_case("main")
        vol, X = b["tsdf"], b["Xw"]
        sel = np.arange(300)[::-1].copy()
    elif name == "sigma30":
        X = plane_points(rng, 400, 0.14, 0.08, 0.030)
        sel = rng.permutation(400)[:300]
    elif name == "zero":
        vol = layered_volume(dims)
        X = plane_points(rng, 100, 0.14, 0.08, 0.004)
        sel = rng.permutation(100)
    elif name == "edge_rays":
        X = plane_points(rng, 64, 0.14, 0.08, 0.004)
        X[0] = [0.001, 0.001, 0.01]                    # depth < 0.05
        X[1] = [0.0, 0.0, 0.049]
        X[2] = [0.0, 0.0, -1.0]
        X[3] = [0.14, 0.08, 0.90]                      # samples reach the ROI only in the far half
        X[4] = [0.10, 0.0, 1.12]                       # samples start inside and leave through the top
        X[5] = [0.5, 0.5, 1.0]                         # never inside
        X[6] = [0.16, 0.0, 1.0]                        # x beyond the face for most of the way
        X[7] = [-0.149, -0.089, 1.0]
        sel = rng.permutation(64)
    else:
        X = plane_points(np.random.default_rng(9), 400, 0.14, 0.08, 0.004)
        sel = np.random.default_rng(10).permutation(400)[:300]
        if name.startswith("samples"):
            n_samples = int(name[7:])
        elif name.startswith("sel"):
            sel = sel[:int(name[3:])]
        else:
            assert name == "sigma4"
    return dict(vol=vol, mn=mn, mx=mx, X=X, sel=sel.astype(np.int64), n_samples=n_samples)


@functools.lru_cache(maxsize=None)
def raycast_case(name):
    """The inputs plus the oracle's result per selected ray: surf f32 [n_sel, 3] (the original point where the ray
    misses), hit bool [n_sel]."""
    d = raycast_inputs(name)
    n = len(d["X"])
    Xr, hits = TR.extract_surface(d["vol"], d["mn"], d["mx"], np.ones(n, bool), d["X"], d["sel"], d["n_samples"], MAX_DISP,
                                  "scalar")
    return dict(d, surf=Xr[d["sel"]], hit=hits[d["sel"]])
