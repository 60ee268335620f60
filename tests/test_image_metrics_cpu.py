"""CPU checks of the render-quality definition (tests/imgmetrics_numpy.py): agreement with scipy.ndimage, the mask
rules, the soundness of the derived bounds and that they are not vacuous (every named wrong implementation lies at least
1000 bounds away on the trap input), the closed forms, the JSON writer and the declarations of the entry points."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imgmetrics_numpy as M  # noqa: E402


def _pair(seed, n, h, w, c):
    rng = np.random.default_rng(seed)
    a = rng.uniform(size=(n, h, w, c)).astype(np.float32)
    b = np.clip(a + 0.2 * rng.standard_normal((n, h, w, c)), 0, 1).astype(np.float32)
    return a, b


def test_weights_equal_scipy_kernel():
    from scipy.ndimage import gaussian_filter1d

    impulse = np.zeros(41)
    impulse[20] = 1.0
    k = gaussian_filter1d(impulse, M.SIGMA, truncate=3.5, mode="constant")
    assert np.count_nonzero(k) == M.TAPS and np.count_nonzero(k[15:26]) == M.TAPS     # radius int(3.5 * 1.5 + 0.5) = 5
    g = M.window()
    assert g.dtype == np.float64 and g.shape == (11,) and abs(g.sum() - 1.0) <= 4 * M.U
    assert np.abs(k[15:26] - g).max() <= 4 * M.U                 # exp(-0.5 / s^2 * i^2) against exp(-0.5 (i/s)^2)
    assert np.array_equal(g, g[::-1])


def test_definition_against_scipy():
    from scipy.ndimage import gaussian_filter

    a, b = _pair(0, 2, 23, 31, 3)
    ref = M.image_metrics(a, b)
    A, B = a.astype(np.float64), b.astype(np.float64)

    def G(x):
        return np.stack([np.stack([gaussian_filter(x[i, ..., k], M.SIGMA, truncate=3.5, mode="reflect")
                                   for k in range(x.shape[3])], -1) for i in range(x.shape[0])])[:, 5:-5, 5:-5]

    mu_a, mu_b = G(A), G(B)
    v_a, v_b, c_ab = G(A * A) - mu_a ** 2, G(B * B) - mu_b ** 2, G(A * B) - mu_a * mu_b
    S = (2 * mu_a * mu_b + M.C1) * (2 * c_ab + M.C2) / ((mu_a ** 2 + mu_b ** 2 + M.C1) * (v_a + v_b + M.C2))
    mine = M.ssim_terms(A, B)
    err = np.abs(S - mine).max()
    print(f"S against scipy.ndimage on 2 x 23x31x3: max difference {err:.3e} (bound {M.S_BOUND:.3e})")
    assert S.shape == mine.shape == (2, 13, 21, 3) and err < M.S_BOUND
    assert np.abs(ref["ssim"] - S.mean((1, 2, 3))).max() < M.S_BOUND
    assert np.array_equal(ref["n_windows"], [13 * 21] * 2) and np.array_equal(ref["n_pixels"], [23 * 31] * 2)
    assert np.allclose(ref["ssim_map"][:, 5:-5, 5:-5], S.mean(-1), rtol=0, atol=M.S_BOUND)
    assert np.isnan(ref["ssim_map"][:, :5]).all() and np.isnan(ref["ssim_map"][:, :, -5:]).all()
    mse = ((A - B) ** 2).mean((1, 2, 3))
    assert np.allclose(ref["mse"], mse, rtol=1e-13, atol=0) and np.allclose(ref["psnr"], -10 * np.log10(mse), rtol=1e-13)


def test_masks():
    a, b = _pair(1, 2, 30, 34, 3)
    mask = np.ones((2, 30, 34), bool)
    mask[0, 12, 14] = False
    ref = M.image_metrics(a, b, mask)
    valid = ref["valid"]
    # every centre whose window touches the hole is invalid; the neighbour 6 pixels away is valid
    assert not valid[0, 7:18, 9:20].any()
    assert valid[0, 12, 20] and valid[0, 12, 8] and valid[0, 18, 14] and valid[0, 6, 14]
    assert valid[0].sum() == 20 * 24 - 121 and valid[1].sum() == 20 * 24
    assert np.array_equal(ref["n_windows"], [20 * 24 - 121, 20 * 24]) and np.array_equal(ref["n_pixels"], [30 * 34 - 1, 30 * 34])
    assert np.array_equal(np.isnan(ref["ssim_map"]), ~valid)
    # a masked-out pixel never influences an output
    for junk in (np.nan, np.inf, -np.inf, 1.0e30):
        a2, b2 = a.copy(), b.copy()
        a2[0, 12, 14], b2[0, 12, 14, 1] = junk, -junk
        other = M.image_metrics(a2, b2, mask)
        for k in ("psnr", "ssim", "mse", "n_pixels", "n_windows", "ssim_map", "sums"):
            assert np.array_equal(ref[k], other[k], equal_nan=True), (junk, k)
    # a non-finite masked-in value propagates to its image alone
    a2 = a.copy()
    a2[1, 3, 3, 0] = np.nan
    other = M.image_metrics(a2, b, mask)
    assert np.isnan(other["psnr"][1]) and np.isnan(other["ssim"][1]) and np.isnan(other["mse"][1])
    for k in ("psnr", "ssim", "mse"):
        assert other[k][0] == ref[k][0]
    # no pixel, no window
    none = M.image_metrics(a, b, np.zeros((2, 30, 34), bool))
    assert np.isnan(none["psnr"]).all() and np.isnan(none["ssim"]).all() and np.isnan(none["ssim_map"]).all()
    assert not none["n_pixels"].any() and not none["n_windows"].any()
    # images below the window: PSNR alone
    for h, w in ((10, 40), (40, 10)):
        a3, b3 = _pair(2, 1, h, w, 1)
        small = M.image_metrics(a3, b3)
        assert small["n_windows"][0] == 0 and np.isnan(small["ssim"][0]) and np.isfinite(small["psnr"][0])
        assert small["n_pixels"][0] == h * w and np.isnan(small["ssim_map"]).all()
    one = M.image_metrics(*_pair(3, 1, 11, 11, 4))
    assert one["n_windows"][0] == 1 and np.isfinite(one["ssim_map"][0, 5, 5]) and np.isnan(one["ssim_map"]).sum() == 120


def test_bound_is_sound():
    """Row pass first, column pass first and the full 2-D sum are three float64 evaluations of the same expression."""
    assert 1e-10 < M.S_BOUND < 1e-8
    worst = 0.0
    for seed, (n, h, w, c) in enumerate([(2, 23, 31, 3), (1, 37, 53, 4), (3, 11, 12, 1)]):
        a, b = _pair(10 + seed, n, h, w, c)
        if seed == 1:                                          # flat, dark and equal regions: the smallest denominators
            a[:, :20] = 0.0
            b[:, :20] = 0.0
            a[:, 20:, :25] = 1.0
        rows, cols, full = (M.image_metrics(a, b, order=o) for o in ("rows", "cols", "full"))
        A, B = a.astype(np.float64), b.astype(np.float64)
        s = {o: M.ssim_terms(A, B, order=o) for o in ("rows", "cols", "full")}
        d_rc, d_rf = np.abs(s["rows"] - s["cols"]).max(), np.abs(s["rows"] - s["full"]).max()
        worst = max(worst, d_rc, d_rf)
        assert d_rc < M.S_BOUND and d_rf < M.S_BOUND and d_rf < M.s_bound(24, 124)
        sb = M.sums_bounds(rows, c)
        for other in (cols, full):
            assert (np.abs(rows["sums"] - other["sums"]) <= sb).all()
            fb = M.figure_bounds(rows, c)
            assert (np.abs(rows["ssim"] - other["ssim"]) <= fb["ssim"]).all() and (fb["ssim"] < 4 * M.S_BOUND).all()
    print(f"largest difference between summation orders {worst:.3e}, bound {M.S_BOUND:.3e}")
    assert M.s_bound(24, 124) > M.S_BOUND > M.s_error() > 0


@pytest.mark.parametrize("name", sorted(M.TRAPS))
def test_traps_exceed_the_bound_1000_times(name):
    figure, needs_mask = M.TRAPS[name]
    a, b, mask = M.trap_input()
    mask = mask if needs_mask else None
    ref, bad = M.image_metrics(a, b, mask), M.wrong(name, a, b, mask)
    bound = M.figure_bounds(ref, a.shape[3])[figure][0]
    gap = abs(ref[figure][0] - bad[figure][0])
    print(f"{name}: {figure} {ref[figure][0]:.6f} against {bad[figure][0]:.6f}, gap / bound = {gap / bound:.3e}")
    assert np.isfinite(gap) and gap >= 1000.0 * bound


def test_closed_forms():
    for p, q in ((0.25, 0.5), (0.0, 1.0), (0.75, 0.75), (0.0, 0.0)):
        a, b = np.full((1, 15, 17, 3), p, np.float32), np.full((1, 15, 17, 3), q, np.float32)
        m = M.image_metrics(a, b)
        want = (2 * p * q + M.C1) / (p * p + q * q + M.C1)
        assert abs(m["ssim"][0] - want) <= M.S_BOUND and np.nanmax(np.abs(m["ssim_map"] - want)) <= M.S_BOUND
        if p != q:
            assert abs(m["psnr"][0] + 20 * np.log10(abs(p - q))) <= 1e-12      # the offsets are exact in binary
        else:
            assert m["mse"][0] == 0 and m["psnr"][0] == np.inf


def test_save_render_metrics_round_trip(tmp_path):
    from mast3r_slam import evaluate

    metrics = dict(psnr=23.5, ssim=0.81, psnr_min=20.25, ssim_min=float("nan"), hit_share=0.75, window_share=0.5, n_views=2,
                   per_view=dict(psnr=[26.75, 20.25], ssim=[0.81, float("nan")], n_pixels=[100, 50], n_windows=[4, 0]))
    path = evaluate.save_render_metrics(tmp_path / "sub", "render.json", metrics)
    with open(path) as f:
        text = f.read()
    back = json.loads(text)
    assert os.path.dirname(str(path)) == str(tmp_path / "sub") and text.endswith("\n")
    assert list(back) == sorted(metrics)
    assert json.dumps(back, sort_keys=True) == json.dumps(metrics, sort_keys=True)      # NaN != NaN: compare the text


def test_entry_points_are_declared_and_exported():
    import mslam_hip

    sig = mslam_hip.parse_header(mslam_hip._header_text())
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert sig["mslam_image_metrics_workspace_bytes"] == (ctypes.c_size_t, [i] * 4)
    assert sig["mslam_image_metrics"] == (i, [vp] * 3 + [i] * 4 + [vp] * 6)
    c = mslam_hip.header_constants()
    th, tw = c["MSLAM_IMAGE_METRICS_TILE_H"], c["MSLAM_IMAGE_METRICS_TILE_W"]
    assert th * tw % 256 == 0 and th >= 1 and tw >= 1
    L = mslam_hip.lib()
    tiles = lambda h, w: -(-h // th) * -(-w // tw)
    assert L.mslam_image_metrics_workspace_bytes(3, 37, 53, 3) == 3 * tiles(37, 53) * 32
    for bad in ((0, 8, 8, 3), (1, 0, 8, 3), (1, 8, 0, 3), (1, 8, 8, 0), (1, 8, 8, 5)):
        assert L.mslam_image_metrics_workspace_bytes(*bad) == 0
    from mast3r_slam.tsdf import image_metrics as f
    from mast3r_slam.tsdf.image_metrics import gaussian_window

    assert callable(f) and np.array_equal(gaussian_window(), M.window())
