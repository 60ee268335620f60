"""Pure-numpy statement, all float64, of the render-quality figures (csrc/image_metrics.hip, DESIGN.md "Render
quality"): PSNR and SSIM of a rendering `a` against an image `b`, f32[N,h,w,C] with C in 1..4 and data range 1, under an
optional pixel mask bool[N,h,w] (None: all true).

PSNR per image: mse = sum over masked-in pixels and channels of (a-b)^2 / (C n_pixels), psnr = 10 log10(1 / mse), +inf
for mse == 0, NaN without a masked-in pixel.

SSIM per image (Wang, Bovik, Sheikh, Simoncelli 2004): separable Gaussian window of 11 taps, sigma 1.5,
g[i] = exp(-0.5 (i/1.5)^2) / sum, i = -5..5; K1 = 0.01, K2 = 0.03, C1 = K1^2, C2 = K2^2; per channel
mu_a = G*a, mu_b = G*b, v_a = G*(a^2) - mu_a^2, v_b = G*(b^2) - mu_b^2, c_ab = G*(ab) - mu_a mu_b (no sample-covariance
factor), S = (2 mu_a mu_b + C1)(2 c_ab + C2) / ((mu_a^2 + mu_b^2 + C1)(v_a + v_b + C2)).  A window centre is valid when
its whole 11x11 window lies inside the image (rows 5..h-6, columns 5..w-6) and all 121 mask pixels are true; ssim = mean
of S over valid centres and channels (NaN without one), ssim_map = the channel mean at valid centres, NaN elsewhere.
With a full mask this is what scikit-image's structural_similarity(gaussian_weights=True, sigma=1.5,
use_sample_covariance=False, data_range=1, channel_axis=-1) returns (scikit-image is not a dependency: the CPU test
checks the agreement with scipy.ndimage.gaussian_filter(truncate=3.5) cropped by 5 instead).

A masked-out pixel never influences an output, whatever it holds; a non-finite masked-in value propagates to its
image's figures (NaN) and is not trapped.

Bounds (values in [0,1]; u = 2^-53).  For another float64 evaluation with a different summation order:
  * one window moment G*x is two 11-term weighted sums, weights positive with sum 1: each term passes through one
    product and at most 10 additions per pass, so |computed - exact| <= gamma_n max|x| with gamma_n = n u / (1 - n u)
    and n = 2 * 11 roundings, + 1 for the product x*x or x*y inside, + 1 of slack: n = 24 (moment_error).  The full 2-D
    sum (121 terms, weights g[i] g[j]) has n = 1 + 1 + 1 + 120 roundings: moment_error(124).
  * the cancellation: mu^2 and mu_a mu_b carry 2 e_m + e_m^2 + u, so v and c, differences of two numbers of size <= 1,
    carry e_v = e_m + (2 e_m + e_m^2 + u) + u in ABSOLUTE terms however small they are.
  * the denominators: S = R1 R2 with R1 = N1 / D1, R2 = N2 / D2, |N1| <= D1, |N2| <= D2 (Cauchy-Schwarz; the weights
    are positive), D1 >= C1, D2 >= C2.  An absolute error e_N above and e_D below moves a ratio of size <= 1 by at most
    (e_N + e_D) / (D - e_D) <= (e_N + e_D) / (C - e_D): the small constants amplify the cancellation error, by 1/C1
    and 1/C2 (their sum is below the 1/(C1 C2) of the product form).  e_N1 = 2 e_mu2 + 3u, e_D1 = 2 e_mu2 + 6u,
    e_N2 = 2 e_v + u, e_D2 = 2 e_v + 2u (the additions round numbers below 2.0002, resp. 0.51).
  * s_error = e_R1 + e_R2 + e_R1 e_R2 + 4u (the products and the division of the final expression).
Two evaluations that each meet s_error differ by at most s_bound = 2 s_error = 5.3e-10 per centre.  The map is
stored as f32: map_bound adds the rounding 2^-24 of a value of size <= 1 (+ the channel mean's roundings).
The per-image sums: squared error, n terms each with relative error <= 3u, any summation order <= (n - 1) u relative:
se_bound = 2 (n + 4) u total.  S: n terms of size <= 1 + s_error each off by s_error, summation (n - 1) u sum|S|:
s_sum_bound = 2 (n s_error + n^2 u (1 + s_error))."""
import numpy as np

RADIUS, TAPS, SIGMA = 5, 11, 1.5
K1, K2 = 0.01, 0.03
C1, C2 = K1 ** 2, K2 ** 2
U = 2.0 ** -53


def window():
    """The 11 normalised Gaussian taps, f64."""
    i = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    g = np.exp(-0.5 * (i / SIGMA) ** 2)
    return g / g.sum()


# ---- bounds ----------------------------------------------------------------------------------------------------------
def moment_error(roundings=24):
    return roundings * U / (1.0 - roundings * U)


def s_error(roundings=24):
    """|computed - exact| of S at one centre and channel for an evaluation whose moments pass `roundings` roundings."""
    e_m = moment_error(roundings)
    e_mu2 = 2.0 * e_m + e_m * e_m + U
    e_v = e_m + e_mu2 + U
    e_r1 = ((2.0 * e_mu2 + 3.0 * U) + (2.0 * e_mu2 + 6.0 * U)) / (C1 - (2.0 * e_mu2 + 6.0 * U))
    e_r2 = ((2.0 * e_v + U) + (2.0 * e_v + 2.0 * U)) / (C2 - (2.0 * e_v + 2.0 * U))
    return e_r1 + e_r2 + e_r1 * e_r2 + 4.0 * U


def s_bound(roundings=24, other=None):
    """Largest difference of S between two evaluations, of `roundings` and `other` (default: the same) roundings."""
    return s_error(roundings) + s_error(roundings if other is None else other)


S_BOUND = s_bound()


def map_bound(channels):
    """ssim_map (f32) against the definition's (f64)."""
    return S_BOUND + channels * U + 2.0 ** -24 * (1.0 + S_BOUND)


def se_bound(n_terms, total):
    return 2.0 * (n_terms + 4) * U * total


def s_sum_bound(n_terms):
    return 2.0 * (n_terms * s_error() + n_terms * n_terms * U * (1.0 + s_error()))


# ---- the definition --------------------------------------------------------------------------------------------------
def _filter(x, g, axis):
    """Valid-mode correlation of x with the taps g along `axis`, taps added in order."""
    n = x.shape[axis] - (len(g) - 1)
    idx = [slice(None)] * x.ndim
    out = 0.0
    for k in range(len(g)):
        idx[axis] = slice(k, k + n)
        out = out + g[k] * x[tuple(idx)]
    return out


def _smooth(x, g, order):
    """G*x at the centres whose window lies in the image: [N,h,w,C] -> [N,h-10,w-10,C].  order: "rows" (along a row
    first, then down the column: the kernel's), "cols" (the reverse) or "full" (one 2-D sum with weights g[i] g[j])."""
    if order == "rows":
        return _filter(_filter(x, g, 2), g, 1)
    if order == "cols":
        return _filter(_filter(x, g, 1), g, 2)
    assert order == "full"
    n, m = x.shape[1] - (len(g) - 1), x.shape[2] - (len(g) - 1)
    out = 0.0
    for i in range(len(g)):
        for j in range(len(g)):
            out = out + (g[i] * g[j]) * x[:, i:i + n, j:j + m]
    return out


def ssim_terms(a, b, g=None, order="rows", cov_factor=1.0, c1=C1, c2=C2):
    """S f64[N,h-10,w-10,C] at every centre whose window lies in the image (h, w >= 11)."""
    g = window() if g is None else g
    mu_a, mu_b = _smooth(a, g, order), _smooth(b, g, order)
    v_a = cov_factor * (_smooth(a * a, g, order) - mu_a * mu_a)
    v_b = cov_factor * (_smooth(b * b, g, order) - mu_b * mu_b)
    c_ab = cov_factor * (_smooth(a * b, g, order) - mu_a * mu_b)
    return ((2.0 * mu_a * mu_b + c1) * (2.0 * c_ab + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (v_a + v_b + c2))


def valid_centres(mask, taps=TAPS):
    """bool[N,h,w]: the whole window lies in the image and every mask pixel under it is true."""
    n, h, w = mask.shape
    out = np.zeros((n, h, w), bool)
    r = taps // 2
    if h >= taps and w >= taps:
        ok = np.ones((n, h - 2 * r, w - 2 * r), bool)
        for i in range(taps):
            for j in range(taps):
                ok &= mask[:, i:i + h - 2 * r, j:j + w - 2 * r]
        out[:, r:h - r, r:w - r] = ok
    return out


def _evaluate(a, b, mask, g, order, cov_factor, data_range, channel_factor):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and a.ndim == 4 and 1 <= a.shape[3] <= 4
    n, h, w, c = a.shape
    mask = np.ones((n, h, w), bool) if mask is None else np.asarray(mask, bool)
    assert mask.shape == (n, h, w)
    r = len(g) // 2
    valid = valid_centres(mask, len(g))
    with np.errstate(all="ignore"):
        sq = np.where(mask[..., None], (a - b) ** 2, 0.0)
        se = np.array([sq[i].sum() for i in range(n)])
        n_pixels = mask.reshape(n, -1).sum(1).astype(np.int64)
        mse = se / ((c if channel_factor else 1) * n_pixels)          # 0 / 0 = NaN without a pixel
        psnr = np.where(mse == 0.0, np.inf, 10.0 * np.log10(data_range ** 2 / mse))
        s_map = np.full((n, h, w), np.nan)
        s_sum = np.zeros(n)
        if h >= len(g) and w >= len(g):
            S = ssim_terms(a, b, g, order, cov_factor, (K1 * data_range) ** 2, (K2 * data_range) ** 2)
            inner = valid[:, r:h - r, r:w - r]
            s_sum = np.array([S[i][inner[i]].sum() for i in range(n)])
            s_map[:, r:h - r, r:w - r] = np.where(inner, S.sum(-1) / c, np.nan)
        n_windows = valid.reshape(n, -1).sum(1).astype(np.int64)
        ssim = s_sum / (c * n_windows)
    return dict(psnr=psnr, ssim=ssim, mse=mse, n_pixels=n_pixels, n_windows=n_windows, ssim_map=s_map,
                sums=np.stack([se, s_sum], 1), valid=valid)


def image_metrics(a, b, mask=None, order="rows"):
    """The definition.  a, b [N,h,w,C], mask bool[N,h,w] or None -> dict of psnr, ssim, mse f64[N], n_pixels, n_windows
    i64[N], ssim_map f64[N,h,w], sums f64[N,2] (squared error; S over valid centres and channels), valid bool[N,h,w]."""
    return _evaluate(a, b, mask, window(), order, 1.0, 1.0, True)


# ---- named wrong implementations (the traps) ---------------------------------------------------------------------------
def _hide(x, mask):
    return np.where(mask[..., None], np.asarray(x, np.float64), 0.0)


def wrong(name, a, b, mask=None):
    """One of the implementations the tests must tell from the definition -> the same dict."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    g, kw = window(), dict(order="rows", cov_factor=1.0, data_range=1.0, channel_factor=True)
    if name == "uniform_window":
        g = np.full(TAPS, 1.0 / TAPS)
    elif name == "sample_covariance":
        kw["cov_factor"] = 121.0 / 120.0
    elif name == "zero_padded_border":
        pad = ((0, 0), (RADIUS, RADIUS), (RADIUS, RADIUS))
        full = np.ones(a.shape[:3], bool) if mask is None else np.asarray(mask, bool)
        a, b = np.pad(_hide(a, full), pad + ((0, 0),)), np.pad(_hide(b, full), pad + ((0, 0),))
        mask = None                                          # every pixel of the image becomes a centre
    elif name == "mask_ignored":
        mask = None
    elif name == "mask_zeroes_pixels":
        a, b, mask = _hide(a, mask), _hide(b, mask), None
    elif name == "data_range_255":
        kw["data_range"] = 255.0
    elif name == "luminance_first":
        lum = np.array([0.299, 0.587, 0.114])
        a, b = (a @ lum)[..., None], (b @ lum)[..., None]
    elif name == "no_channel_factor":
        kw["channel_factor"] = False
    else:
        raise KeyError(name)
    return _evaluate(a, b, mask, g, **kw)


# name -> (the figure it moves, whether the trap needs a mask with holes)
TRAPS = {"uniform_window": ("ssim", False), "sample_covariance": ("ssim", False), "zero_padded_border": ("ssim", False),
         "mask_ignored": ("ssim", True), "mask_zeroes_pixels": ("ssim", True), "data_range_255": ("ssim", False),
         "luminance_first": ("ssim", False), "no_channel_factor": ("mse", False)}


def trap_input(seed=0, n=1, h=23, w=31, c=3):
    """A pair on which every trap separates: a smooth pattern plus noise per channel, b = a + noise, a mask with a few
    holes, and in the holes values that differ wildly (finite, so that the mask-ignoring traps stay finite)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([0.5 + 0.3 * np.sin(0.7 * x + 0.4 * y + k) for k in range(c)], -1)
    a = np.clip(base[None] + 0.15 * rng.standard_normal((n, h, w, c)), 0.0, 1.0).astype(np.float32)
    b = np.clip(a * np.linspace(0.7, 1.0, c) + 0.08 * rng.standard_normal((n, h, w, c)), 0.0, 1.0).astype(np.float32)
    mask = rng.uniform(size=(n, h, w)) > 0.01
    mask[:, h // 2, w // 2] = False
    a[~mask] = 1.0
    b[~mask] = 0.0
    return a, b, mask


def sums_bounds(ref, channels):
    """f64[N,2]: se_bound and s_sum_bound of every image of the definition's dict `ref`."""
    n_se = ref["n_pixels"].astype(np.float64) * channels
    n_s = ref["n_windows"].astype(np.float64) * channels
    return np.stack([se_bound(n_se, ref["sums"][:, 0]), s_sum_bound(n_s)], 1)


def figure_bounds(ref, channels):
    """dict of f64[N]: the bounds on mse and ssim that follow from the sums' (the divisions add one rounding each)."""
    sb = sums_bounds(ref, channels)
    n_se = np.maximum(ref["n_pixels"].astype(np.float64) * channels, 1.0)
    n_s = np.maximum(ref["n_windows"].astype(np.float64) * channels, 1.0)
    with np.errstate(invalid="ignore"):
        return dict(mse=sb[:, 0] / n_se + 2.0 * U * np.abs(ref["mse"]), ssim=sb[:, 1] / n_s + 2.0 * U)
