"""GPU test (-m gpu) of csrc/image_metrics.hip and mast3r_slam.tsdf.image_metrics against the float64 definition
(tests/imgmetrics_numpy.py) with its derived bounds.  Every operand of every launch, the workspace included, lies in a
guarded buffer (kernel_refs.Guarded); the shapes are the smallest at which the tiling can go wrong."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imgmetrics_numpy as M  # noqa: E402
from kernel_refs import Guarded, check_guards  # noqa: E402

pytestmark = pytest.mark.gpu

import mslam_hip as _m  # noqa: E402

TH, TW = (_m.header_constants()["MSLAM_IMAGE_METRICS_TILE_" + k] for k in ("H", "W"))
SHAPES = [(11, 11), (10, 40), (40, 10), (11, 12), (12, 11), (TH, TW), (TH + 10, TW), (TH + 11, TW), (TH, TW + 10),
          (TH, TW + 11), (37, 53)]
OUTS = ("sums", "counts", "ssim_map", "workspace")


def _pair(seed, n, h, w, c):
    rng = np.random.default_rng(seed)
    a = rng.uniform(size=(n, h, w, c)).astype(np.float32)
    b = np.clip(a + 0.2 * rng.standard_normal((n, h, w, c)), 0, 1).astype(np.float32)
    return a, b


def _masks(seed, n, h, w):
    rng = np.random.default_rng(seed)
    holes = rng.uniform(size=(n, h, w)) > 0.05
    single = np.ones((n, h, w), bool)
    single[:, h // 2, w // 2] = False
    seam = np.ones((n, h, w), bool)
    seam[:, min(TH, h - 1), min(TW, w - 1)] = False          # the first pixel of the next tile, where there is one
    sparse = rng.uniform(size=(n, h, w)) > 0.003               # a few holes: most windows stay valid
    return dict(none=None, holes=holes, sparse=sparse, single=single, seam=seam, empty=np.zeros((n, h, w), bool))


def _buffers(device, a, b, mask, want_map=True):
    n, h, w, c = a.shape
    ws = _m.lib().mslam_image_metrics_workspace_bytes(n, h, w, c)
    assert ws > 0 and ws % 8 == 0
    bufs = dict(a=Guarded(device, torch.float32, src=torch.from_numpy(a)),
                b=Guarded(device, torch.float32, src=torch.from_numpy(b)),
                window=Guarded(device, torch.float64, src=torch.from_numpy(M.window())),
                sums=Guarded(device, torch.float64, (n, 2)), counts=Guarded(device, torch.int64, (n, 2)),
                workspace=Guarded(device, torch.float64, (ws // 8,)))
    if mask is not None:
        bufs["mask"] = Guarded(device, torch.uint8, src=torch.from_numpy(mask.astype(np.uint8)))
    if want_map:
        bufs["ssim_map"] = Guarded(device, torch.float32, (n, h, w))
    return bufs


def _launch(bufs, shape, **override):
    n, h, w, c = shape
    p = {k: _m.ptr(v.t) for k, v in bufs.items()}
    arg = dict(a=p["a"], b=p["b"], mask=p.get("mask", 0), n=n, h=h, w=w, c=c, window=p["window"], sums=p["sums"],
               counts=p["counts"], ssim_map=p.get("ssim_map", 0), workspace=p["workspace"])
    arg.update(override)
    return _m.lib().mslam_image_metrics(arg["a"], arg["b"], arg["mask"], arg["n"], arg["h"], arg["w"], arg["c"],
                                        arg["window"], arg["sums"], arg["counts"], arg["ssim_map"], arg["workspace"],
                                        _m.stream_ptr())


def _run(device, a, b, mask=None, want_map=True, what="image_metrics"):
    """One guarded launch -> (sums f64[n,2], counts i64[n,2], ssim_map f32[n,h,w] or None) as numpy."""
    bufs = _buffers(device, a, b, mask, want_map)
    _m.check(_launch(bufs, a.shape), what)
    check_guards(bufs, [k for k in OUTS if k in bufs], what)
    return (bufs["sums"].t.cpu().numpy(), bufs["counts"].t.cpu().numpy(),
            bufs["ssim_map"].t.cpu().numpy() if want_map else None)


def _check_against_definition(device, a, b, mask, what):
    c = a.shape[3]
    ref = M.image_metrics(a, b, mask)
    sums, counts, smap = _run(device, a, b, mask, what=what)
    assert np.array_equal(counts[:, 0], ref["n_pixels"]) and np.array_equal(counts[:, 1], ref["n_windows"]), what
    assert np.array_equal(np.isnan(smap), ~ref["valid"]), f"{what}: NaN pattern of the map"
    if ref["valid"].any():
        err = np.abs(smap.astype(np.float64) - ref["ssim_map"])[ref["valid"]].max()
        assert err <= M.map_bound(c), f"{what}: map off by {err:.3e}, bound {M.map_bound(c):.3e}"
    d, bound = np.abs(sums - ref["sums"]), M.sums_bounds(ref, c)
    assert (d <= bound).all(), f"{what}: sums off by {d.tolist()}, bounds {bound.tolist()}"
    return ref, sums, counts, smap


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_against_definition(device, hw, c):
    from mast3r_slam.tsdf.image_metrics import figures, image_metrics

    h, w = hw
    for n in (1, 3):
        a, b = _pair(100 * h + w + c + n, n, h, w, c)
        for name, mask in _masks(h * w + n, n, h, w).items():
            what = f"{n}x{h}x{w}x{c} mask {name}"
            ref, sums, counts, smap = _check_against_definition(device, a, b, mask, what)
            # the Python figures follow from the sums
            fig = {k: v.cpu().numpy() for k, v in figures(torch.from_numpy(sums).to(device),
                                                          torch.from_numpy(counts).to(device), c).items()}
            with np.errstate(all="ignore"):
                mse = sums[:, 0] / (c * counts[:, 0])
                psnr = np.where(mse == 0, np.inf, 10 * np.log10(1 / mse))
                ssim = sums[:, 1] / (c * counts[:, 1])
            assert np.array_equal(fig["mse"], mse, equal_nan=True) and np.array_equal(fig["ssim"], ssim, equal_nan=True), what
            assert np.allclose(fig["psnr"], psnr, rtol=0, atol=1e-12, equal_nan=True), what     # two log10s, one ulp each
            fb = M.figure_bounds(ref, c)
            for k in ("mse", "ssim"):
                ok = np.isnan(ref[k]) & np.isnan(fig[k]) | (np.abs(fig[k] - ref[k]) <= fb[k])
                assert ok.all(), f"{what}: {k} {fig[k]} against {ref[k]}"
            out = image_metrics(torch.from_numpy(a).to(device), b, None if mask is None else torch.from_numpy(mask),
                                ssim_map=True)
            assert out["psnr"].dtype == out["ssim"].dtype == out["mse"].dtype == torch.float64
            assert out["n_pixels"].dtype == out["n_windows"].dtype == torch.int64 and out["ssim_map"].dtype == torch.float32
            for k in fig:
                assert out[k].is_cuda and np.array_equal(out[k].cpu().numpy(), fig[k], equal_nan=True), (what, k)
            assert np.array_equal(out["ssim_map"].cpu().numpy(), smap, equal_nan=True), what


def test_without_map(device):
    a, b = _pair(5, 2, 37, 53, 3)
    mask = _masks(5, 2, 37, 53)["holes"]
    with_map, without = _run(device, a, b, mask), _run(device, a, b, mask, want_map=False)
    assert np.array_equal(with_map[0], without[0]) and np.array_equal(with_map[1], without[1]) and without[2] is None


@pytest.mark.parametrize("name", sorted(M.TRAPS))
def test_traps(device, name):
    figure, needs_mask = M.TRAPS[name]
    a, b, mask = M.trap_input()
    mask = mask if needs_mask else None
    c = a.shape[3]
    ref, sums, counts, _ = _check_against_definition(device, a, b, mask, f"trap {name}")
    bad = M.wrong(name, a, b, mask)[figure][0]
    got = (sums[0, 1] / (c * counts[0, 1])) if figure == "ssim" else (sums[0, 0] / (c * counts[0, 0]))
    bound = M.figure_bounds(ref, c)[figure][0]
    assert abs(got - ref[figure][0]) <= bound and abs(got - bad) >= 999.0 * bound, (name, got, ref[figure][0], bad)


def test_identical_images(device):
    a, _ = _pair(7, 2, 37, 53, 3)
    sums, counts, smap = _run(device, a, a.copy(), _masks(7, 2, 37, 53)["single"])
    assert (sums[:, 0] == 0).all()
    from mast3r_slam.tsdf.image_metrics import figures

    fig = figures(torch.from_numpy(sums), torch.from_numpy(counts), 3)
    assert (fig["mse"] == 0).all() and torch.isinf(fig["psnr"]).all() and (fig["psnr"] > 0).all()
    assert (np.abs(fig["ssim"].numpy() - 1.0) <= M.S_BOUND).all() and np.nanmax(np.abs(smap - 1.0)) <= M.map_bound(3)


def test_closed_forms(device):
    for p, q in ((0.25, 0.5), (0.0, 1.0), (0.75, 0.75)):
        a, b = np.full((1, 20, 40, 3), p, np.float32), np.full((1, 20, 40, 3), q, np.float32)
        sums, counts, smap = _run(device, a, b)
        want = (2 * p * q + M.C1) / (p * p + q * q + M.C1)
        assert abs(sums[0, 1] / (3 * counts[0, 1]) - want) <= M.S_BOUND and np.nanmax(np.abs(smap - want)) <= M.map_bound(3)
        if p != q:
            mse = sums[0, 0] / (3 * counts[0, 0])
            assert abs(-10 * np.log10(mse) + 20 * np.log10(abs(p - q))) <= 1e-12


def test_masked_out_values_do_not_matter(device):
    a, b = _pair(9, 2, TH + 11, TW + 11, 3)
    mask = _masks(9, 2, TH + 11, TW + 11)["holes"]
    mask[:, TH, TW] = mask[:, 0, 0] = mask[:, -1, -1] = False
    a[~mask], b[~mask] = 0.0, 0.0
    base = _run(device, a, b, mask)
    for junk in (np.nan, np.inf, 1.0e30):
        a2, b2 = a.copy(), b.copy()
        a2[~mask], b2[~mask] = junk, -junk
        b2[0, TH, TW] = junk
        for x, y in zip(base, _run(device, a2, b2, mask)):
            assert np.array_equal(x.view(np.int64 if x.dtype.itemsize == 8 else np.int32),
                                  y.view(np.int64 if y.dtype.itemsize == 8 else np.int32)), junk


def test_non_finite_masked_in_value(device):
    a, b = _pair(11, 3, 37, 53, 3)
    mask = _masks(11, 3, 37, 53)["single"]                     # the hole is at (18, 26)
    base = _run(device, a, b, mask)
    a2 = a.copy()
    a2[1, 20, 30, 2] = np.nan
    sums, counts, smap = _run(device, a2, b, mask)
    assert np.isnan(sums[1]).all() and np.array_equal(counts, base[1])
    for i in (0, 2):
        assert np.array_equal(sums[i], base[0][i]) and np.array_equal(smap[i], base[2][i], equal_nan=True)


def test_determinism(device):
    from mast3r_slam.tsdf.image_metrics import image_metrics

    n, h, w, c = 3, TH + 11, 2 * TW + 3, 3
    a, b = _pair(13, n, h, w, c)
    mask = _masks(13, n, h, w)["single"] & _masks(13, n, h, w)["seam"]
    first, second = _run(device, a, b, mask), _run(device, a, b, mask)
    for x, y in zip(first, second):
        assert np.array_equal(x, y, equal_nan=True)
    for i in range(n):                                         # alone or at any position of a batch
        alone = _run(device, a[i:i + 1], b[i:i + 1], mask[i:i + 1])
        for x, y in zip(first, alone):
            assert np.array_equal(x[i], y[0], equal_nan=True), i
    order = [2, 0, 1]
    moved = _run(device, a[order], b[order], mask[order])
    for x, y in zip(first, moved):
        assert np.array_equal(x[order], y, equal_nan=True)
    # non-contiguous views are copied: same bits
    ta, tb, tm = (torch.from_numpy(x).to(device) for x in (a, b, mask))
    want = image_metrics(ta, tb, tm, ssim_map=True)
    wide = torch.zeros((n, h, w, 4), device=device)
    wide[..., :3] = ta
    tb_t = tb.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    tm_t = tm.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert not wide[..., :3].is_contiguous() and not tb_t.is_contiguous() and not tm_t.is_contiguous()
    got = image_metrics(wide[..., :3], tb_t, tm_t, ssim_map=True)
    for k in want:
        assert torch.equal(want[k].view(torch.int64 if want[k].element_size() == 8 else torch.int32),
                           got[k].view(torch.int64 if got[k].element_size() == 8 else torch.int32)), k
    assert np.array_equal(want["ssim_map"].cpu().numpy(), first[2], equal_nan=True)
    single = image_metrics(ta[0], tb[0], tm[0])                # (h,w,C) is a batch of one
    assert single["psnr"].shape == (1,) and single["psnr"][0] == want["psnr"][0] and "ssim_map" not in single


def test_argument_errors(device):
    from mast3r_slam.tsdf.image_metrics import image_metrics

    EINVAL = _m.header_constants()["MSLAM_EINVAL"]
    a, b = _pair(15, 2, 20, 24, 3)
    mask = np.ones((2, 20, 24), bool)
    bufs = _buffers(device, a, b, mask)
    bad = [dict(n=0), dict(n=-1), dict(h=0), dict(w=0), dict(h=-3), dict(c=0), dict(c=5), dict(a=0), dict(b=0),
           dict(window=0), dict(sums=0), dict(counts=0), dict(workspace=0)]
    for override in bad:
        assert _launch(bufs, a.shape, **override) == EINVAL, override
        assert _m.lib().mslam_last_error().decode().startswith("image_metrics"), override
    torch.cuda.synchronize()
    check_guards(bufs, [], "refused calls")
    untouched = torch.stack([(bufs[k].raw == bufs[k].pat).all() for k in OUTS]).tolist()
    assert all(untouched), dict(zip(OUTS, untouched))
    _m.check(_launch(bufs, a.shape), "image_metrics")           # and the same buffers still serve a good call
    check_guards(bufs, OUTS, "after refused calls")
    ta, tb, tm = (torch.from_numpy(x).to(device) for x in (a, b, mask))
    with pytest.raises(ValueError, match="differ in shape"):
        image_metrics(ta, tb[:, :19])
    with pytest.raises(ValueError, match="1 to 4 channels"):
        image_metrics(torch.zeros((2, 20, 24, 5), device=device), torch.zeros((2, 20, 24, 5), device=device))
    with pytest.raises(ValueError, match="float"):
        image_metrics((ta * 255).to(torch.uint8), tb)
    with pytest.raises(ValueError, match="float"):
        image_metrics(ta, (b * 255).astype(np.uint8))
    with pytest.raises(ValueError, match=r"\(h,w,C\) or \(N,h,w,C\)"):
        image_metrics(ta[0, 0], tb[0, 0])
    with pytest.raises(ValueError, match="mask must be"):
        image_metrics(ta, tb, tm[:1])
    with pytest.raises(ValueError, match="mask must be a bool"):
        image_metrics(ta, tb, tm.float())
    with pytest.raises(RuntimeError, match="no CPU path"):
        image_metrics(a, b)
