"""Input recipes and references for the edge tests of csrc/matching.hip (tests/test_matching_edges_gpu.py); every recipe
and every expectation is checked on its own, without a GPU, in tests/test_matching_refs_cpu.py.

Three kinds of reference:
  * the bit-exact C oracle (oracle.iter_proj / oracle.refine_matches) where bit-exactness is the contract; it shares its
    statement of the arithmetic with the kernel, so it is not independent;
  * closed-form expected values, written out by hand in the recipe;
  * float64 numpy statements with bounds derived from the kernel's operation count.

The kernels' contract - no recipe here goes beyond it, because beyond it a kernel may read or write outside its buffers:
  * iter_proj:        h, w >= 3 (the clamp box [1, w-2] x [1, h-2] must not be empty);
  * match_occlusion:  every p inside the image, 0 <= trunc(p) < (w, h);
  * refine_matches:   p1 within int32 (the recipes stay within +-2^20);
  * prep_iter_proj:   idx_init in [0, h*w)."""
import numpy as np

import oracle
from oracle import matching_py
from mast3r_slam import synthetic

U = 2.0 ** -24            # unit roundoff of float32: |fl(x) - x| <= U |x| for a correctly rounded operation
TINY = 2.0 ** -149        # one float32 subnormal step: what a gradual underflow can add to an operation's error
HALF_MIN = 2.0 ** -14     # numeric_limits<half>::min(), the score a refine_matches candidate has to beat


def gamma(n):
    """n correctly rounded operations in a row: prod (1 + d_i) = 1 + t with |t| <= gamma(n) (Higham, lemma 3.1)."""
    return n * U / (1.0 - n * U)


def xcd_remap(bid, nblk, nxcd=8):
    """common.h's block remap restated: hardware block id -> logical tile id."""
    q, r = divmod(nblk, nxcd)
    xcd = bid % nxcd
    base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return base + bid // nxcd


# ======================================================================================================================
# 1. prep_iter_proj
# ======================================================================================================================
PREP_SHAPES = [(2, 2), (2, 37), (17, 3), (15, 16), (16, 16), (17, 33), (31, 18)]
PREP_B = (1, 3)
KX = np.array([[-3, 0, 3], [-10, 0, 10], [-3, 0, 3]], np.float64) / 32.0   # 3/32 and 10/32 are exact in float32
# |x| = 0 -> 0;  |x| = 1e-13 < 1e-12 -> x / 1e-12;  a small and a large vector whose squares stay normal in float32
PREP_PLANTS = np.array([[0, 0, 0], [6e-14, 0, 8e-14], [3e-10, -4e-10, 1e-10], [1e15, -2e15, 5e14]], np.float32)

# normalize3 of the kernel: s = fmaf(z, z, fmaf(y, y, x*x)) - three roundings on a sum of non-negative terms, relative
# error <= gamma(3); sqrtf halves it and rounds once (<= gamma(3)/2 + U, i.e. 2.5 roundings); the divide rounds once more:
# 3.5 roundings per component.  Under the 1e-12 clamp the error is the rounding of the constant to float32 plus the divide,
# two roundings.  A component of exactly 0 stays 0.
RAY_REL = gamma(3.5)


def prep_inputs(h, w, b, with_idx):
    """X11, X21 f32[b,h,w,3] (another random image per batch item, z around 3), idx_init i64[b,h*w] or None."""
    rng = np.random.default_rng(1000 * h + 10 * w + b)
    n = h * w

    def cloud():
        x = rng.normal(0, 1, (b, h, w, 3))
        x[..., 2] = 3 + 0.3 * rng.normal(size=(b, h, w))
        return x.astype(np.float32)

    X11, X21 = cloud(), cloud()
    f11, f21 = X11.reshape(b, n, 3), X21.reshape(b, n, 3)
    for bi in range(b):
        for k in range(4):
            f21[bi, (5 * k + bi) % n] = PREP_PLANTS[k]
            if n > 4:                       # a 2x2 image keeps its four random rays for the reflect check
                f11[bi, (7 * k + 3 + bi) % n] = PREP_PLANTS[k]
    idx = None
    if with_idx:
        idx = rng.integers(0, n, (b, n)).astype(np.int64)
        idx[:, :4] = [0, w - 1, w, n - 1]
    return X11, X21, idx


def _normalize64(x):
    x = x.astype(np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-12)


def prep_ref(X11, X21, idx):
    """float64 statement of prep_for_iter_proj and the per-element bound of the kernel's float32 operation sequence.

    rays and pts: RAY_REL |value| (see above).  A gradient is one product and five fmaf over the six non-zero taps,
    visited row-major: tap j of m goes through m - j roundings (the first through m: its product and m - 1 sums), each
    tap carries the error of its ray, and the coefficients are exact.  So
        |g - g64| <= sum_j |k_j| |a_j| (RAY_REL + gamma(n_j) (1 + RAY_REL)),  n_j = 6, 5, 4, 3, 2, 1,
    plus one subnormal step per operation.  Every float32 operation is taken as correctly rounded, sqrtf and the divide
    included: the build does not relax them.
    Returns (rays_with_grad, pts, p_init) in float64 / float32 and (rays_bound, pts_bound)."""
    b, h, w, _ = X11.shape
    rays = _normalize64(X11)
    pad = np.pad(rays, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="reflect")
    out, bnd = [rays], [RAY_REL * np.abs(rays) + TINY]
    for K in (KX, KX.T):
        taps = [(dy, dx) for dy in range(3) for dx in range(3) if K[dy, dx] != 0]
        g, e = np.zeros_like(rays), np.zeros_like(rays)
        for j, (dy, dx) in enumerate(taps):
            win = pad[:, dy:dy + h, dx:dx + w]
            nj = len(taps) - j if j else len(taps)
            g += K[dy, dx] * win
            e += abs(K[dy, dx]) * np.abs(win) * (RAY_REL + gamma(nj) * (1 + RAY_REL))
        out.append(g)
        bnd.append(e + len(taps) * TINY)
    pts = _normalize64(X21).reshape(b, h * w, 3)
    if idx is None:
        idx = np.broadcast_to(np.arange(h * w, dtype=np.int64), (b, h * w))
    p_init = np.stack((idx % w, idx // w), -1).astype(np.float32)
    return np.concatenate(out, -1), pts, p_init, np.concatenate(bnd, -1), RAY_REL * np.abs(pts) + TINY


def _fma32(a, b, c):
    """float32 fmaf through float64: the product is exact there, the sum is rounded twice (differs from one rounding on
    a tie of the second only, about one case in 2^29)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def prep_kernel_model(X11, X21, idx):
    """The kernel's own float32 operation order in numpy: a stand-in for the HIP prep where no GPU is at hand (how far
    the rounding difference between the two preps reaches into the integer outputs of the matching chain)."""
    b, h, w, _ = X11.shape

    def norm3(x):
        x = x.astype(np.float32)
        s = _fma32(x[..., 2], x[..., 2], _fma32(x[..., 1], x[..., 1], x[..., 0] * x[..., 0]))
        return x / np.maximum(np.sqrt(s), np.float32(1e-12))[..., None]

    rays = norm3(X11)
    pad = np.pad(rays, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="reflect")
    out = [rays]
    for K in (KX, KX.T):
        taps = [(dy, dx) for dy in range(3) for dx in range(3) if K[dy, dx] != 0]
        g = None
        for dy, dx in taps:
            win, k = pad[:, dy:dy + h, dx:dx + w], np.float32(K[dy, dx])
            g = k * win if g is None else _fma32(np.broadcast_to(k, win.shape), win, g)
        out.append(g)
    if idx is None:
        idx = np.broadcast_to(np.arange(h * w, dtype=np.int64), (b, h * w))
    return (np.concatenate(out, -1), norm3(X21).reshape(b, h * w, 3),
            np.stack((idx % w, idx // w), -1).astype(np.float32))


# ======================================================================================================================
# 2. iter_proj
# ======================================================================================================================
LAMBDA, THRESH = 1e-8, 1e-6
PAIRS = ((0, 4), (10, 13), (20, 26))
NOISY_HW, NOISY_NOISE = (20, 28), 0.02
ITERS = (0, 1, 2, 10, 60)
N_GRID = (1, 255, 256, 257) + tuple(256 * t - 100 for t in (7, 8, 9, 15, 17))   # on the 8x9 image
SMALL_SHAPES = [(3, 3), (3, 7), (6, 3), (20, 28)]


def noisy_case(b=3, h=NOISY_HW[0], w=NOISY_HW[1], noise=NOISY_NOISE):
    """make_pair data with point noise, prepared by the oracle's prep: (rays f32[b,h,w,9], pts f32[b,hw,3], p0)."""
    prs = [synthetic.make_pair(i, j, h=h, w=w, seed=2, noise=noise) for i, j in PAIRS[:b]]
    X11, X21 = (np.stack([p[k] for p in prs]) for k in ("X11", "X21"))
    return matching_py.prep_for_iter_proj(X11, X21)


def accept_trace(rays, pts, p0, K, lam=LAMBDA, thr=THRESH):
    """bool[b,n,K]: point accepted its trial at iteration k - exactly when the oracle's (u, v) after k + 1 iterations
    differs from that after k (an accepted trial has a smaller cost, so it is another position)."""
    prev, _ = oracle.iter_proj(rays, pts, p0, 0, lam, thr)
    acc = []
    for k in range(1, K + 1):
        cur, _ = oracle.iter_proj(rays, pts, p0, k, lam, thr)
        acc.append((cur != prev).any(-1))
        prev = cur
    return np.stack(acc, -1)


def transition_shares(acc):
    """Share of points that show accept->accept, accept->reject, reject->accept, reject->reject somewhere."""
    a, n = acc[..., :-1], acc[..., 1:]
    return {"aa": (a & n).any(-1).mean(), "ar": (a & ~n).any(-1).mean(), "ra": (~a & n).any(-1).mean(),
            "rr": (~a & ~n).any(-1).mean()}


ZERO_PIX, NAN_ROW = (1, 1), 5      # (x, y) of the zero ray: the corner every clamped trial lands on; row of the NaN pixel


def nonfinite_case():
    """noisy_case with, in every batch item: the ray at ZERO_PIX zero (a sample that lands on it exactly has norm 0,
    rinv = inf and a NaN cost; partly weighted it shortens the sampled ray), the pixel (w-1, NAN_ROW) NaN in all nine
    channels (weight exactly 0 for u == umax: 0 * NaN), and the targets of points 3 and 40 zero."""
    rays, pts, p0 = noisy_case()
    rays, pts = rays.copy(), pts.copy()
    rays[:, ZERO_PIX[1], ZERO_PIX[0], :3] = 0
    rays[:, NAN_ROW, -1, :] = np.nan
    pts[:, (3, 40)] = 0
    return rays, pts, p0


def iter_case(h, w, b, n, seed=0):
    """A noisy pinhole point map through the oracle's prep, n targets that are noisy rays of random pixels, and starting
    points up to two pixels outside the image."""
    rng = np.random.default_rng(seed + 100 * h + w)
    uu, vv = np.meshgrid(np.arange(w) - w / 2 + 0.5, np.arange(h) - h / 2 + 0.5)
    f = 0.9 * max(h, w)
    d = np.stack((uu / f, vv / f, np.ones_like(uu)), -1)
    depth = 3 + 0.5 * np.sin(0.7 * uu + 0.3 * vv) + rng.normal(0, 0.02, (b, h, w))
    X11 = (d[None] * depth[..., None]).astype(np.float32)
    rays, _, _ = matching_py.prep_for_iter_proj(X11, X11)
    bi = np.arange(b)[:, None]
    t = rays[bi, rng.integers(0, h, (b, n)), rng.integers(0, w, (b, n)), :3] + rng.normal(0, 0.02, (b, n, 3))
    pts = (t / np.linalg.norm(t, axis=-1, keepdims=True)).astype(np.float32)
    p0 = np.stack((rng.uniform(-2, w + 2, (b, n)), rng.uniform(-2, h + 2, (b, n))), -1).astype(np.float32)
    return rays, pts, p0


def singular_case(h=6, w=7, b=3):
    """Gradient channels zero, every target the ray at (1, 1), lambda 0: A = 0, det = 0, det_inv = inf, delta = inf * 0
    = NaN, u + NaN = NaN, and fminf(fmaxf(NaN, 1), umax) = 1.  The trial (1, 1) samples the target itself, so it is
    accepted from everywhere else.  Closed form: every point ends at exactly (1, 1), converged.  A clamp that hands the
    NaN on, or that answers a NaN with the other bound, fails this.  (rays, pts, p0, max_iter, lambda)."""
    rays, _, _ = iter_case(h, w, b, 1, seed=3)
    rays = rays.copy()
    rays[..., 3:] = 0
    pts = np.repeat(rays[:, 1, 1, None, :3], h * w, axis=1)
    idx = np.arange(h * w)
    p0 = np.broadcast_to(np.stack((idx % w, idx // w), -1).astype(np.float32), (b, h * w, 2)).copy()
    return rays, pts, p0, 3, 0.0


def pinit_case(h=8, w=9):
    """Starting points outside the image, non-finite and exactly on the clamp bounds, all pairs of them; `clamped` is the
    closed form of the clamp (what max_iter = 0 returns): NaN and everything below 1 -> 1, everything above -> the upper
    bound."""
    rays, _, _ = iter_case(h, w, 1, 1, seed=5)

    def column(m):
        return np.array([[-5, 1], [m + 5, m], [1e30, m], [np.inf, m], [-np.inf, 1], [np.nan, 1], [1.0, 1], [m, m],
                         [0.5, 1], [m + 0.5, m], [-1e30, 1], [2.25, 2.25]], np.float32)

    cu, cv = column(w - 2), column(h - 2)
    iu, iv = np.meshgrid(np.arange(len(cu)), np.arange(len(cv)))
    p0 = np.stack((cu[iu.ravel(), 0], cv[iv.ravel(), 0]), -1)[None]
    clamped = np.stack((cu[iu.ravel(), 1], cv[iv.ravel(), 1]), -1)[None]
    n = p0.shape[1]
    rng = np.random.default_rng(9)
    t = rays[0, rng.integers(0, h, n), rng.integers(0, w, n), :3] + rng.normal(0, 0.02, (n, 3))
    pts = (t / np.linalg.norm(t, axis=-1, keepdims=True)).astype(np.float32)[None]
    return rays, pts, p0, clamped


def clamp_p(p, h, w):
    """fminf(fmaxf(p, 1), (w-2, h-2)): a NaN comes out as 1."""
    return np.fmin(np.fmax(p.astype(np.float32), np.float32(1)), np.array([w - 2, h - 2], np.float32))


# Largest distance from the oracle's p_new to the drawn position on pinhole_case(), all points converged (measured by
# tests/test_matching_refs_cpu.py::test_pinhole_ground_truth, which prints it).  The error is that of the bilinear model
# of the ray image; oracle and kernel are both held to three times the measurement.
PINHOLE_MEASURED = 3.4e-3
PINHOLE_BOUND = 3 * PINHOLE_MEASURED


def pinhole_case():
    """Ground truth that owes nothing to the oracle: a 24x32 analytic pinhole ray image (focal length 30 px, centre
    (w/2, h/2)), targets the exact rays of sub-pixel positions drawn uniformly in [2, w-3] x [2, h-3], identity start.
    Returns (rays, pts, p0, drawn f64[1,n,2])."""
    h, w, f = 24, 32, 30.0

    def ray(u, v):
        d = np.stack(((u - w / 2) / f, (v - h / 2) / f, np.ones_like(u)), -1)
        return d / np.linalg.norm(d, axis=-1, keepdims=True)

    uu, vv = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    r = ray(uu, vv).astype(np.float32)[None]
    gx, gy = matching_py.img_gradient(r)
    rng = np.random.default_rng(11)
    drawn = np.stack((rng.uniform(2, w - 3, h * w), rng.uniform(2, h - 3, h * w)), -1)
    pts = ray(drawn[:, 0], drawn[:, 1]).astype(np.float32)[None]
    p0 = np.stack((uu.ravel(), vv.ravel()), -1).astype(np.float32)[None]
    return np.concatenate((r, gx, gy), -1), pts, p0, drawn[None]


# The same on warped_case(): measured by test_warped_ground_truth_separates_stale_gradients.
WARPED_MEASURED = 1.09e-2
WARPED_BOUND = 3 * WARPED_MEASURED


def warped_case():
    """A ray image whose gradient changes eleven-fold across the image: x = (exp(k (u - w/2)) - 1) / (k f) with k = 0.08,
    y as in the pinhole.  Targets are the exact rays of drawn sub-pixel positions; every start lies 0 ... 16 px on the
    steep side of its target (u0 >= u*), from where Newton steps undershoot and converge.  The gradient at the start is
    up to e^1.28 = 3.6 times the one at the target, so an iteration that keeps using the gradient of an earlier sample
    (not handing the trial's gradient on when the trial is accepted) contracts by 1 - e^(-k du) per step only and is
    tenths of a pixel off after 10 iterations.  Returns (rays, pts, p0, drawn f64[1,n,2])."""
    h, w, f, k = 24, 32, 30.0, 0.08

    def ray(u, v):
        d = np.stack((np.expm1(k * (u - w / 2)) / (k * f), (v - h / 2) / f, np.ones_like(u)), -1)
        return d / np.linalg.norm(d, axis=-1, keepdims=True)

    uu, vv = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    r = ray(uu, vv).astype(np.float32)[None]
    gx, gy = matching_py.img_gradient(r)
    rng = np.random.default_rng(13)
    n = h * w
    drawn = np.stack((rng.uniform(2, w - 3, n), rng.uniform(2, h - 3, n)), -1)
    pts = ray(drawn[:, 0], drawn[:, 1]).astype(np.float32)[None]
    p0 = np.stack((np.minimum(drawn[:, 0] + rng.uniform(0, 16, n), w - 2), np.clip(drawn[:, 1] + rng.uniform(-3, 3, n), 1, h - 2)), -1)
    return np.concatenate((r, gx, gy), -1), pts, p0.astype(np.float32)[None], drawn[None]


def lm64(rays, pts, p0, iters, lam, stale=False):
    """The iteration in float64, one batch item, to show on the CPU what a recipe separates.  stale: the gradient of
    the first sample is never replaced (the named wrong variant of the kernel's carried-over sample)."""
    img = rays[0].astype(np.float64)
    h, w = img.shape[:2]
    t = pts[0].astype(np.float64)
    hi = np.array([w - 2, h - 2], np.float64)
    p = np.clip(p0[0].astype(np.float64), 1, hi)

    def sample(p):
        u0, v0 = np.floor(p[:, 0]).astype(int), np.floor(p[:, 1]).astype(int)
        du, dv = (p[:, 0] - u0)[:, None], (p[:, 1] - v0)[:, None]
        s = ((1 - du) * (1 - dv) * img[v0, u0] + du * (1 - dv) * img[v0, u0 + 1] + (1 - du) * dv * img[v0 + 1, u0]
             + du * dv * img[v0 + 1, u0 + 1])
        e = s[:, :3] / np.linalg.norm(s[:, :3], axis=-1, keepdims=True) - t
        return e, s[:, 3:6], s[:, 6:9]

    e, gx, gy = sample(p)
    lam = np.full(len(p), lam, np.float64)
    for _ in range(iters):
        A00, A01, A11 = (gx * gx).sum(-1) + lam, (gx * gy).sum(-1), (gy * gy).sum(-1) + lam
        b0, b1 = -(e * gx).sum(-1), -(e * gy).sum(-1)
        det = A00 * A11 - A01 * A01
        q = np.clip(p + np.stack((A11 * b0 - A01 * b1, A00 * b1 - A01 * b0), -1) / det[:, None], 1, hi)
        f, hx, hy = sample(q)
        ok = (f * f).sum(-1) < (e * e).sum(-1)
        p, e = np.where(ok[:, None], q, p), np.where(ok[:, None], f, e)
        if not stale:
            gx, gy = np.where(ok[:, None], hx, gx), np.where(ok[:, None], hy, gy)
        lam = np.where(ok, lam * 0.1, lam * 10)
    return p


def cost64(rays, pts, p):
    """Squared distance between the target and the renormalised float64 bilinear sample of the ray channels at p.
    Returns (cost, norm of the sample before it is renormalised)."""
    b = rays.shape[0]
    r = rays[..., :3].astype(np.float64)
    u, v = p[..., 0].astype(np.float64), p[..., 1].astype(np.float64)
    u0, v0 = np.floor(u).astype(int), np.floor(v).astype(int)
    du, dv = (u - u0)[..., None], (v - v0)[..., None]
    bi = np.arange(b)[:, None]
    s = ((1 - du) * (1 - dv) * r[bi, v0, u0] + du * (1 - dv) * r[bi, v0, u0 + 1]
         + (1 - du) * dv * r[bi, v0 + 1, u0] + du * dv * r[bi, v0 + 1, u0 + 1])
    nrm = np.linalg.norm(s, axis=-1)
    e = s / nrm[..., None] - pts.astype(np.float64)
    return (e * e).sum(-1), nrm


def cost_eval_bound(cost, nrm):
    """Bound on |float32 cost - cost64| for the kernel's evaluation, ray components and weights at most 1 in magnitude:
      * du, dv are exact; each weight is rounded once; a channel is one product and three fmaf over weights that sum
        to 1: absolute error <= (gamma(4) + U) sum w |r| <= 5.1 U =: ds per channel;
      * renormalising: dot3 (3 roundings), sqrtf (half of that, plus 1), the reciprocal (1), the product (1):
        4.5 roundings on a component of at most 1, and the sample's own error, a vector of length <= sqrt(3) ds, scaled
        by 1/nrm and at most doubled by the renormalisation's derivative while ds << nrm;
      * e = n - t rounds once on |e| <= 2:  de = gamma(4.5) + 2 sqrt(3) ds / nrm + 2 U per component;
      * cost = dot3(e, e): |sum (e_i + d_i)^2 - sum e_i^2| <= 2 sqrt(3 cost) de + 3 de^2, plus gamma(3) cost."""
    ds = 5.1 * U
    de = gamma(4.5) + 2 * np.sqrt(3) * ds / nrm + 2 * U
    return 2 * np.sqrt(3 * cost) * de + 3 * de * de + gamma(3) * cost


# ======================================================================================================================
# 3. match_occlusion
# ======================================================================================================================
OCC_SHAPES = [(5, 51), (7, 37)]          # h*w = 255 and 259; w > h, so a swapped u / v reads another pixel
OCC_THRESH = float(np.float32(0.1))


def occlusion_case(h, w, b=3):
    """X11, X21 f32[b,h,w,3], p f32[b,hw,2], valid on entry u8[b,hw], expected p1 i64 and valid bool.

    Every difference X11[p1] - X21 is either shorter than 0.05 or longer than 0.2, except the planted ones: there X21 is
    0 and the looked-up pixel is (d, 0, 0), (0, -d, 0), ... with d == thresh (invalid: `<` is strict) or the float32
    just below it (valid); with one non-zero component the float32 distance is exactly |d|.  One looked-up pixel holds
    a NaN (invalid); a third of the points come in invalid and stay so."""
    rng = np.random.default_rng(7 * h + w)
    n = h * w
    X11 = rng.normal(0, 1, (b, h, w, 3)).astype(np.float32)
    frac = rng.choice(np.array([0.0, 0.999, 0.5, 0.25], np.float32), (b, n, 2))
    frac = np.where(rng.random((b, n, 2)) < 0.5, frac, rng.random((b, n, 2)).astype(np.float32))
    p = np.stack((rng.integers(1, w - 1, (b, n)), rng.integers(1, h - 1, (b, n))), -1).astype(np.float32) + frac
    p = np.minimum(p, np.array([w - 2 + 0.999, h - 2 + 0.999], np.float32)).astype(np.float32)
    p1 = np.trunc(p).astype(np.int64)
    assert (p1[..., 0] >= 1).all() and (p1[..., 0] <= w - 2).all() and (p1[..., 1] >= 1).all() and (p1[..., 1] <= h - 2).all()
    assert (p1[..., 0] > h).any()
    # planted: points 0..5 of every batch item, each looking up a pixel of its own
    t_eq, t_below = np.float32(OCC_THRESH), np.nextafter(np.float32(OCC_THRESH), np.float32(0))
    plants = [(0, t_eq, False), (1, t_below, True), (2, -t_eq, False), (0, -t_below, True), (1, t_eq, False),
              (2, t_below, True)]
    planted = np.zeros((b, n), bool)
    expect_planted = np.zeros((b, n), bool)
    for bi in range(b):
        for k, (comp, d, ok) in enumerate(plants):
            p[bi, k] = (1 + k + 0.999, 1 + (k + bi) % (h - 2) + 0.999 * (k % 2))
            X11[bi, int(p[bi, k, 1]), int(p[bi, k, 0])] = 0
            X11[bi, int(p[bi, k, 1]), int(p[bi, k, 0]), comp] = d
            planted[bi, k], expect_planted[bi, k] = True, ok
    p1 = np.trunc(p).astype(np.int64)
    bi = np.arange(b)[:, None]
    look = X11[bi, p1[..., 1], p1[..., 0]]
    dirs = rng.normal(size=(b, n, 3))
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    length = np.where(rng.random((b, n)) < 0.5, rng.uniform(0, 0.05, (b, n)), rng.uniform(0.2, 0.5, (b, n)))
    X21 = (look - dirs * length[..., None]).astype(np.float32)
    X21[planted] = 0
    # a NaN at the pixel point 10 looks up (after X21 is made, so only the X11 side carries it)
    nan_pix = p1[:, 10].copy()
    X11[np.arange(b), nan_pix[:, 1], nan_pix[:, 0], 1] = np.nan
    valid_in = (rng.random((b, n)) > 1 / 3)
    valid_in[:, :11] = True
    # expectation: float64 numpy, the planted closed forms on top
    d64 = X11[bi, p1[..., 1], p1[..., 0]].astype(np.float64) - X21.astype(np.float64)
    dist = np.sqrt((d64 * d64).sum(-1))
    with np.errstate(invalid="ignore"):
        ok = dist < OCC_THRESH
        margin = np.abs(dist - OCC_THRESH)
    ok[planted] = expect_planted[planted]
    assert (margin[~planted & ~np.isnan(dist)] >= 1e-3).all()
    assert np.isnan(dist[:, 10]).all() and not ok[:, 10].any()
    return dict(X11=X11, X21=X21.reshape(b, h, w, 3), p=p, valid_in=valid_in.astype(np.uint8), p1=p1,
                valid=valid_in & ok, planted=planted)


# ======================================================================================================================
# 4. refine_matches
# ======================================================================================================================
def _h(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def _ftz(x):
    return np.where(np.abs(x) < HALF_MIN, np.float32(0), x)


def _score(a, c, acc, ftz):
    """a, c f32[n,f] holding half values.  `half`: products and sums rounded to half one by one, k = 0, 1, ... (a half
    product is exact in float32 and a float32 sum of two halves rounds to half like the half sum itself); `float`:
    exact products summed in float32; `pairwise`: half products, half sums over a binary tree."""
    n, f = a.shape
    with np.errstate(over="ignore", invalid="ignore"):
        if acc == "float":
            s = np.zeros(n, np.float32)
            for k in range(f):
                s = s + a[:, k] * c[:, k]
            return s
        prod = _h(a * c)
        if ftz:
            prod = _ftz(prod)
        if acc == "pairwise":
            terms = [prod[:, k] for k in range(f)] or [np.zeros(n, np.float32)]
            while len(terms) > 1:
                terms = [_h(terms[i] + terms[i + 1]) if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
            return terms[0]
        s = np.zeros(n, np.float32)
        for k in range(f):
            s = _h(s + prod[:, k])
            if ftz:
                s = _ftz(s)
        return s


def refine_model(D11, D21, p1, radius, dilation_max, v_outer=False, ge=False, acc="half", ftz=False):
    """refine_matches in numpy, all points of a batch item at once, with the switches of the named wrong variants:
    v as the outer loop, `>=` for `>`, float32 or pairwise accumulation, half subnormals flushed to zero.
    Returns (p1_new i64[b,n,2], tied bool[b,n]): tied = a candidate other than the current winner met the running
    maximum exactly, which is where `>` and `>=` part."""
    D11, D21 = np.asarray(D11, np.float16), np.asarray(D21, np.float16)
    b, h, w, f = D11.shape
    n = D21.shape[1]
    out, tied_all = np.zeros((b, n, 2), np.int64), np.zeros((b, n), bool)
    for bi in range(b):
        a = D21[bi].astype(np.float32)
        u0, v0 = p1[bi, :, 0].astype(np.int64), p1[bi, :, 1].astype(np.int64)
        un, vn = u0.copy(), v0.copy()
        mx = np.full(n, HALF_MIN, np.float32)
        has, tied = np.zeros(n, bool), np.zeros(n, bool)
        for d in range(dilation_max, 0, -1):
            rd = radius * d
            offs = range(0, 2 * rd + 1, d)
            for o1 in offs:
                for o2 in offs:
                    ii, jj = (o2, o1) if v_outer else (o1, o2)
                    u, v = u0 - rd + ii, v0 - rd + jj
                    inside = (u >= 0) & (u < w) & (v >= 0) & (v < h)
                    c = D11[bi, np.clip(v, 0, h - 1), np.clip(u, 0, w - 1)].astype(np.float32)
                    sf = _score(a, c, acc, ftz)
                    with np.errstate(invalid="ignore"):
                        win = inside & ((sf >= mx) if ge else (sf > mx))
                        tied |= inside & has & (sf == mx) & ((u != un) | (v != vn))
                    mx = np.where(win, sf, mx)
                    un, vn = np.where(win, u, un), np.where(win, v, vn)
                    has |= win
            u0, v0 = un.copy(), vn.copy()
        out[bi, :, 0], out[bi, :, 1], tied_all[bi] = un, vn, tied
    return out, tied_all


def _trap(name, fdim, d21, cands, expect, wrong=(), fused=None, centre=(2, 2), radius=1, dil=1, hw=(5, 5)):
    """One point at `centre` of an hw image; cands: {(u, v): leading descriptor values}, the rest zero.  wrong: pairs of
    (refine_model switches, the answer that variant must give); fused: the answer of the oracle's fused_fma variant."""
    h, w = hw
    D11 = np.zeros((1, h, w, fdim), np.float16)
    D21 = np.zeros((1, 1, fdim), np.float16)
    with np.errstate(over="ignore"):
        D21[0, 0, :len(d21)] = d21
        for (u, v), vals in cands.items():
            D11[0, v, u, :len(vals)] = vals
    return dict(name=name, D11=D11, D21=D21, p1=np.array([[centre]], np.int64), radius=radius, dil=dil,
                expect=np.array([[expect]], np.int64), wrong=list(wrong), fused=fused)


TRAP_FDIMS = (24, 40)       # the unrolled 16-byte path and the generic loop (zero padded: + 0 changes no half sum)


def refine_traps(fdim):
    """Closed-form cases of refine_matches; each docstring line says what the expected answer rests on."""
    x = 1 + 2.0 ** -10
    big = 60000.0           # 2 * 60000 overflows half: the product is +inf
    return [
        # equal top scores at (u0-1, v0+1) and (u0+1, v0-1): u is the outer loop and `>` keeps the first
        _trap("scan_order", fdim, [1], {(1, 3): [0.5], (3, 1): [0.5]}, (1, 3),
              wrong=[(dict(v_outer=True), (3, 1)), (dict(ge=True), (3, 1))]),
        # A = 2048 + 23 x 1 stays 2048 in a sequential half sum (ties to even); B = 2050 wins
        _trap("half_sum", fdim, [1] * 24, {(1, 1): [2048] + [1] * 23, (3, 3): [2050]}, (3, 3),
              wrong=[(dict(acc="float"), (1, 1)), (dict(acc="pairwise"), (1, 1))]),
        # A: -(1+2^-9) + fl(x*x) + 2^-13 = 2^-13 with rounded products, 2^-13 + 2^-20 fused; B = 2^-13 + 2^-21 between
        _trap("unfused", fdim, [-(1 + 2.0 ** -9), x, 1], {(3, 1): [1, x, 2.0 ** -13], (3, 3): [0, 0, 2.0 ** -13 + 2.0 ** -21]},
              (3, 3), fused=(3, 1)),
        # 24 products of 2^-18, each a half subnormal: their sum 1.5 * 2^-14 beats 2^-14
        _trap("subnormal", fdim, [2.0 ** -9] * 24, {(3, 2): [2.0 ** -9] * 24}, (3, 2), wrong=[(dict(ftz=True), (2, 2))]),
        # a score of exactly 2^-14 does not win (`>` is strict), the next half does
        _trap("threshold_equal", fdim, [1], {(3, 2): [HALF_MIN]}, (2, 2), wrong=[(dict(ge=True), (3, 2))]),
        _trap("threshold_next", fdim, [1], {(3, 2): [HALF_MIN + 2.0 ** -24]}, (3, 2)),
        # +inf wins once; the later +inf is not greater
        _trap("inf_first", fdim, [2], {(1, 2): [big], (3, 2): [big]}, (1, 2), wrong=[(dict(ge=True), (3, 2))]),
        # inf - inf = NaN never wins, before or after a finite winner
        _trap("inf_minus_inf", fdim, [2, 2], {(1, 2): [big, -big], (3, 2): [0.25], (3, 3): [big, -big]}, (3, 2)),
        _trap("neg_inf", fdim, [2], {(1, 2): [-big]}, (2, 2)),
        _trap("nan_d11", fdim, [1], {(1, 2): [np.nan], (3, 2): [0.5], (3, 3): [np.nan]}, (3, 2)),
        _trap("nan_d21", fdim, [np.nan], {(u, v): [1] for u in range(5) for v in range(5)}, (2, 2)),
    ]


REFINE_HW = (9, 11)
REFINE_FDIMS = (0, 1, 7, 8, 16, 24, 32, 40)
REFINE_RD = ((0, 1), (1, 0), (1, 1), (2, 3), (3, 5))
REFINE_N = (1, 257)
REFINE_KINDS = ("normal", "tie")


def refine_random(fdim, n, kind, b=3):
    """Random descriptors on the 9x11 image; `tie`: components in {-0.5, 0, 0.5}, so that scores are small multiples of
    0.25, exact in half, and many candidates share the maximum."""
    h, w = REFINE_HW
    rng = np.random.default_rng(fdim * 1000 + n + (kind == "tie"))
    if kind == "tie":
        D11 = rng.integers(-1, 2, (b, h, w, fdim)) * 0.5
        D21 = rng.integers(-1, 2, (b, n, fdim)) * 0.5
    else:
        D11, D21 = rng.normal(size=(b, h, w, fdim)), rng.normal(size=(b, n, fdim))
    p1 = np.stack((rng.integers(0, w, (b, n)), rng.integers(0, h, (b, n))), -1).astype(np.int64)
    return D11.astype(np.float16), D21.astype(np.float16), p1


OUTSIDE_RD = (3, 5)


def refine_outside():
    """p1 outside the 9x11 image (all within +-2^20): windows partly outside follow the oracle, (-40, -40) is out of
    reach of radius 3 x dilation 5 and comes back unchanged."""
    h, w = REFINE_HW
    D11, D21, _ = refine_random(24, 5, "normal", b=1)
    p1 = np.array([[(-1, 2), (w, 2), (2, -3), (w + 2, h + 2), (-40, -40)]], np.int64)
    return D11, D21, p1


# ======================================================================================================================
# 5. the Python layer
# ======================================================================================================================
MATCH_HW = (17, 19)
MATCH_LEFT_OUT = 0.02


def match_case(b=3):
    """make_pair data at 17x19 with a starting index map; D21 stays float32."""
    h, w = MATCH_HW
    prs = [synthetic.make_pair(i, j, h=h, w=w, seed=4) for i, j in PAIRS[:b]]
    d = {k: np.stack([p[k] for p in prs]) for k in ("X11", "X21", "D11", "D21")}
    rng = np.random.default_rng(21)
    idx = np.arange(h * w)[None] + rng.integers(-2, 3, (b, h * w)) + w * rng.integers(-2, 3, (b, h * w))
    d["idx"] = np.clip(idx, 0, h * w - 1).astype(np.int64)
    return d


def oracle_chain(d, prep, cfg):
    """The oracle's iter_proj, occlusion test, refine_matches and pixel_to_lin on a given prep: (idx, valid)."""
    rays, pts, p0 = prep
    b, h, w, _ = d["X11"].shape
    p, conv = oracle.iter_proj(rays, pts, p0, cfg["max_iter"], cfg["lambda_init"], cfg["convergence_thresh"])
    p1, v = matching_py.occlusion_and_trunc(d["X11"], d["X21"], p, conv, cfg["dist_thresh"])
    if cfg["radius"] > 0:
        p1 = oracle.refine_matches(d["D11"].astype(np.float16), d["D21"].reshape(b, h * w, -1).astype(np.float16), p1,
                                   cfg["radius"], cfg["dilation_max"])
    return matching_py.pixel_to_lin(p1, w), v
