#!/usr/bin/env python3
"""Event timing of the render-quality kernel (csrc/image_metrics.hip) on 1 and 8 pairs of 384x512x3 images with a hit
mask of about 60 % (a disc, so that windows survive), medians of repeated calls with HIP events after warm-up: (a)
tsdf.image_metrics, PSNR and SSIM in one launch; (b) the same figures written the way a user would write them without
it, five depthwise torch.nn.functional.conv2d calls per separable pass in float64 on the device plus the masked
reductions (at most 5 repetitions).  (b) is there for context, not as a pass mark; both are checked against each other
before they are timed.
Not part of bench.py.
    python tools/image_metrics_time.py [--reps 20] [--hw 384 512]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam-quality-dualtsdf_amd")]
import numpy as np
import torch
import torch.nn.functional as F

from mast3r_slam.tsdf.image_metrics import gaussian_window, image_metrics

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--hw", type=int, nargs=2, default=(384, 512))
ap.add_argument("--batches", type=int, nargs="+", default=(1, 8))
args = ap.parse_args()
dev = torch.device("cuda:0")
h, w = args.hw
print(f"image={h}x{w}x3 device={torch.cuda.get_device_name(dev)}", flush=True)
C1, C2 = 0.01 ** 2, 0.03 ** 2


def timed(fn, reps):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def conv2d_metrics(a, b, mask, g):
    """The figures with torch alone, float64: a, b [N,h,w,3], mask bool[N,h,w], g f64[11] -> (psnr, ssim) f64[N]."""
    n, c = a.shape[0], a.shape[3]
    x, y = a.permute(0, 3, 1, 2).double(), b.permute(0, 3, 1, 2).double()
    kr, kc = g.view(1, 1, 1, -1).expand(c, 1, 1, -1), g.view(1, 1, -1, 1).expand(c, 1, -1, 1)
    G = lambda t: F.conv2d(F.conv2d(t, kr, groups=c), kc, groups=c)
    mu_x, mu_y = G(x), G(y)
    v_x, v_y, c_xy = G(x * x) - mu_x * mu_x, G(y * y) - mu_y * mu_y, G(x * y) - mu_x * mu_y
    S = (2 * mu_x * mu_y + C1) * (2 * c_xy + C2) / ((mu_x * mu_x + mu_y * mu_y + C1) * (v_x + v_y + C2))
    m = mask.view(n, 1, h, w).double()
    ones = torch.ones(11, dtype=torch.float64, device=a.device)
    valid = F.conv2d(F.conv2d(m, ones.view(1, 1, 1, -1)), ones.view(1, 1, -1, 1)) == 121.0
    ssim = (S * valid).sum((1, 2, 3)) / (c * valid.sum((1, 2, 3)))
    mse = ((x - y) ** 2 * m).sum((1, 2, 3)) / (c * m.sum((1, 2, 3)))
    return 10.0 * torch.log10(1.0 / mse), ssim


yy, xx = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
disc = ((yy - h / 2) / (h / 2)) ** 2 + ((xx - w / 2) / (w / 2)) ** 2 < 0.6 * 4.0 / np.pi     # area share 0.6
g = torch.from_numpy(gaussian_window()).to(dev)
for n in args.batches:
    gen = torch.Generator(device=dev).manual_seed(n)
    a = torch.rand((n, h, w, 3), device=dev, generator=gen)
    b = (a + 0.1 * torch.randn((n, h, w, 3), device=dev, generator=gen)).clamp(0, 1)
    mask = disc.expand(n, h, w).contiguous()
    out = image_metrics(a, b, mask)
    psnr, ssim = conv2d_metrics(a, b, mask, g)
    d_psnr, d_ssim = float((out["psnr"] - psnr).abs().max()), float((out["ssim"] - ssim).abs().max())
    assert d_psnr < 1e-9 and d_ssim < 1e-9, (d_psnr, d_ssim)
    k_med, k_min, k_max = timed(lambda: image_metrics(a, b, mask), args.reps)
    m_med, m_min, m_max = timed(lambda: image_metrics(a, b, mask, ssim_map=True), args.reps)
    t_med, t_min, t_max = timed(lambda: conv2d_metrics(a, b, mask, g), min(args.reps, 5))
    print(f"pairs={n} hit_share={float(mask.float().mean()):.4f} window_share={float(out['n_windows'].sum()) / (n * h * w):.4f} "
          f"psnr={float(out['psnr'][0]):.3f} ssim={float(out['ssim'][0]):.4f} (conv2d differs by {d_psnr:.1e} dB, {d_ssim:.1e})",
          flush=True)
    print(f"  (a) image_metrics_ms median={k_med:.3f} min={k_min:.3f} max={k_max:.3f}; with ssim_map median={m_med:.3f}",
          flush=True)
    print(f"  (b) torch_conv2d_f64_ms median={t_med:.3f} min={t_min:.3f} max={t_max:.3f}  ratio (b)/(a)={t_med / k_med:.1f}",
          flush=True)
