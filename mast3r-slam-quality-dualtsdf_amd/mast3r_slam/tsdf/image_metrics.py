"""Render quality: PSNR and SSIM of renderings against images on the device (csrc/image_metrics.hip, DESIGN.md "Render
quality"; the definition is tests/imgmetrics_numpy.py).  One launch scores a batch of pairs; there is no CPU path."""
import numpy as np
import torch

import mslam_hip as _m

RADIUS, TAPS, SIGMA = 5, 11, 1.5
TILE_H, TILE_W = (_m.header_constants()["MSLAM_IMAGE_METRICS_TILE_" + k] for k in ("H", "W"))


def gaussian_window():
    """The 11 taps g[i] = exp(-0.5 (i/1.5)^2), i = -5..5, over their sum: numpy float64."""
    i = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    g = np.exp(-0.5 * (i / SIGMA) ** 2)
    return g / g.sum()


_windows = {}


def _window(device):
    key = (device.type, device.index)
    if key not in _windows:
        _windows[key] = torch.from_numpy(gaussian_window()).to(device)
    return _windows[key]


def _image_arg(x, name, device, what):
    """f32[N,h,w,C] contiguous device tensor of an image or a batch given as a numpy array or a tensor."""
    if isinstance(x, np.ndarray):
        if x.dtype.kind != "f":
            raise ValueError(f"{what}: {name} must be a float array, got {x.dtype}")
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if not torch.is_tensor(x):
        raise TypeError(f"{what}: {name} must be a numpy array or a tensor")
    if not x.is_floating_point():
        raise ValueError(f"{what}: {name} must be a float tensor, got {x.dtype}")
    if x.dim() not in (3, 4):
        raise ValueError(f"{what}: {name} must be (h,w,C) or (N,h,w,C), got {tuple(x.shape)}")
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if not 1 <= x.shape[3] <= 4:
        raise ValueError(f"{what}: {name} must have 1 to 4 channels, got {int(x.shape[3])}")
    if min(x.shape[:3]) < 1:
        raise ValueError(f"{what}: {name} is empty, shape {tuple(x.shape)}")
    if device is not None:
        x = x.to(device)
    return x.detach().to(torch.float32).contiguous()


def image_metrics(pred, target, mask=None, ssim_map=False):
    """PSNR and SSIM of `pred` against `target`: (h,w,C) or (N,h,w,C) float images with C in 1..4 and data range 1,
    numpy arrays or tensors (at least one of them on the device; non-contiguous views are copied).  `mask`: bool (h,w)
    or (N,h,w), None = every pixel.  Per image: the squared error is averaged over the masked-in pixels and the
    channels; SSIM is Wang et al.'s (Gaussian window of 11 taps, sigma 1.5, K1 = 0.01, K2 = 0.03, per channel, no
    sample-covariance factor), averaged over the window centres whose whole 11x11 window lies in the image and is
    masked-in.  A masked-out pixel influences nothing; a non-finite masked-in value makes its image's figures NaN.

    Returns device tensors: psnr f64[N] (+inf for identical images, NaN without a pixel), ssim f64[N] (NaN without a
    window), mse f64[N], n_pixels i64[N], n_windows i64[N], and with `ssim_map=True` ssim_map f32[N,h,w] (NaN away from
    the valid centres).  Nothing is read back: the host sees a figure when the caller converts it."""
    what = "image_metrics"
    device = next((x.device for x in (pred, target, mask) if torch.is_tensor(x) and x.is_cuda), None)
    if device is None:
        raise RuntimeError(f"{what}: no operand is on a HIP device; there is no CPU path")
    a = _image_arg(pred, "pred", device, what)
    b = _image_arg(target, "target", device, what)
    if a.shape != b.shape:
        raise ValueError(f"{what}: pred {tuple(a.shape)} and target {tuple(b.shape)} differ in shape")
    n, h, w, c = (int(x) for x in a.shape)
    m = None
    if mask is not None:
        m = torch.from_numpy(np.ascontiguousarray(mask)) if isinstance(mask, np.ndarray) else mask
        if not torch.is_tensor(m) or m.dtype != torch.bool:
            raise ValueError(f"{what}: mask must be a bool array or tensor")
        if m.dim() == 2:
            m = m.unsqueeze(0)
        if tuple(m.shape) != (n, h, w):
            raise ValueError(f"{what}: mask must be {(n, h, w)}, got {tuple(m.shape)}")
        m = m.to(device).contiguous()
    L = _m.lib()
    ws_bytes = L.mslam_image_metrics_workspace_bytes(n, h, w, c)
    if ws_bytes == 0:
        raise ValueError(f"{what}: {n} images of {h}x{w} are outside the kernel's grid")
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=device)
    sums = torch.empty((n, 2), dtype=torch.float64, device=device)
    counts = torch.empty((n, 2), dtype=torch.int64, device=device)
    smap = torch.empty((n, h, w), dtype=torch.float32, device=device) if ssim_map else None
    with torch.cuda.device(device):
        _m.check(L.mslam_image_metrics(_m.ptr(a), _m.ptr(b), _m.ptr(m.view(torch.uint8)) if m is not None else 0, n, h,
                                       w, c, _m.ptr(_window(device)), _m.ptr(sums), _m.ptr(counts), _m.ptr(smap),
                                       _m.ptr(ws), _m.stream_ptr()), "image_metrics")
    out = figures(sums, counts, c)
    if ssim_map:
        out["ssim_map"] = smap
    return out


def figures(sums, counts, channels):
    """The figures of the kernel's sums f64[N,2] and counts i64[N,2]: mse = squared error / (C n_pixels),
    psnr = 10 log10(1 / mse) (+inf for 0, NaN for 0/0), ssim = S / (C n_windows) (NaN for 0/0)."""
    n_pixels, n_windows = counts[:, 0], counts[:, 1]
    mse = sums[:, 0] / (channels * n_pixels).double()
    psnr = torch.where(mse == 0, torch.full_like(mse, float("inf")), 10.0 * torch.log10(1.0 / mse))
    ssim = sums[:, 1] / (channels * n_windows).double()
    return dict(psnr=psnr, ssim=ssim, mse=mse, n_pixels=n_pixels, n_windows=n_windows)
