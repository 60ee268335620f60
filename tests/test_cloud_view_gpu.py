"""The cloud-view kernels (csrc/cloud_view.hip; DESIGN.md "Cloud views") against their numpy statement
(tests/cloudview_numpy.py), byte for byte, through the raw C entry points with every operand in a guarded buffer; then
the Python layer (render_cloud, observed_cloud_points, compare_clouds(observed=...)) and the product."""
import math

import numpy as np
import pytest
import torch

import cloud_numpy as C
import cloudview_numpy as CV
import cloudview_support as S
from kernel_refs import Guarded
from mast3r_slam import synthetic
from mesh_support import VS, Operands

pytestmark = pytest.mark.gpu

SPLAT_KEYS = ("near", "far", "radius", "point_size", "max_radius")
SIZES_N = (0, 1, 63, 64, 65, 255, 256, 257, 1000)         # none, one; around a wave; around a block; four blocks
IMAGES = ((1, 1), (3, 5), (8, 8), (16, 16), (17, 33))
VIEWS = (1, 2, 8, 9)                                      # around observed_cloud_points' chunk of 8


def _k4(K):
    K = np.asarray(K, np.float64).reshape(3, 3)
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def _camera(hw):
    h, w = hw
    return np.array([[0.8 * w, 0, w / 2.0 - 0.3], [0, 0.9 * w, h / 2.0 + 0.2], [0, 0, 1.0]])


def _poses(rng, V):
    """Cameras near the origin that look roughly along +z, each with a scale different from 1."""
    out = []
    for _ in range(V):
        q = synthetic.quat_from_rotvec(rng.normal(0, 0.25, 3))
        out.append(np.concatenate((rng.normal(0, 0.2, 3), q, [rng.uniform(0.5, 2.5)])))
    return np.stack(out).astype(np.float32).reshape(-1, 8)


def _points(rng, n):
    """In front of the cameras, behind them and beside the frustum; some at equal places, one NaN and one inf."""
    p = (rng.uniform(-1, 1, (n, 3)) * [1.5, 1.5, 3.0] + [0, 0, 2.0]).astype(np.float32)
    if n > 8:
        p[::9] = p[1]
        p[5, 1] = np.nan
        p[7, 2] = np.inf
    return p


def _splat(device, pts, poses, K, hw, near=0.05, far=10.0, radius=0, point_size=None, max_radius=8):
    """mslam_cloud_view_splat through the C entry point -> zbuf as a device tensor i64[V,h,w]; guards checked."""
    import mslam_hip as _m

    ops = Operands(device)
    pts, poses = np.asarray(pts, np.float32).reshape(-1, 3), np.asarray(poses, np.float32).reshape(-1, 8)
    p, c = ops.put(pts, np.float32), ops.put(poses, np.float32)
    z = ops.out(torch.int64, (len(poses),) + tuple(hw))
    _m.check(_m.lib().mslam_cloud_view_splat(_m.ptr(p), len(pts), _m.ptr(c), len(poses), *_k4(K), hw[0], hw[1],
                                             float(near), float(far), radius, -1.0 if point_size is None else point_size,
                                             max_radius, _m.ptr(z), 0, _m.stream_ptr()), "cloud_view_splat")
    ops.check()
    return z


def _resolve(device, z, poses, colors=None, n=0):
    """mslam_cloud_view_resolve of the z-buffer z (numpy u64 or a device tensor) -> numpy (range, index, hit[, rgb])."""
    import mslam_hip as _m

    ops = Operands(device)
    zh = z.cpu().numpy() if torch.is_tensor(z) else np.asarray(z).view(np.int64)
    V, h, w = zh.shape
    zd, c = ops.put(zh, np.int64), ops.put(np.asarray(poses, np.float32).reshape(-1, 8), np.float32)
    col = ops.put(colors, np.uint8) if colors is not None else None
    out = [ops.out(torch.float32, (V, h, w)), ops.out(torch.int32, (V, h, w)), ops.out(torch.uint8, (V, h, w))]
    if colors is not None:
        out.append(ops.out(torch.uint8, (V, h, w, 3)))
    _m.check(_m.lib().mslam_cloud_view_resolve(_m.ptr(zd), _m.ptr(c), V, h, w, _m.ptr(col), n, _m.ptr(out[0]),
                                               _m.ptr(out[1]), _m.ptr(out[2]),
                                               _m.ptr(out[3]) if colors is not None else 0, _m.stream_ptr()),
             "cloud_view_resolve")
    ops.check()
    return tuple(t.cpu().numpy() for t in out)


def _visible(device, queries, z, poses, K, hw, near=0.05, far=10.0, tol=0.01, rel_tol=0.0, seen=None):
    """mslam_cloud_view_visible -> seen u8[m] as numpy; `seen`: the start."""
    import mslam_hip as _m

    ops = Operands(device)
    q = np.asarray(queries, np.float32).reshape(-1, 3)
    qd, c = ops.put(q, np.float32), ops.put(np.asarray(poses, np.float32).reshape(-1, 8), np.float32)
    zd = ops.put(z.cpu().numpy() if torch.is_tensor(z) else np.asarray(z).view(np.int64), np.int64)
    s = ops.put(np.zeros(len(q), np.uint8) if seen is None else seen, np.uint8)
    _m.check(_m.lib().mslam_cloud_view_visible(_m.ptr(qd), len(q), _m.ptr(zd), _m.ptr(c), len(c), *_k4(K), hw[0], hw[1],
                                               float(near), float(far), float(tol), float(rel_tol), _m.ptr(s),
                                               _m.stream_ptr()), "cloud_view_visible")
    ops.check()
    return s.cpu().numpy()


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _colors(rng, n):
    c = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    c[c == 0xA5] = 0xA4                                   # the guards' "never written" pattern for u8
    return c


def _check_case(device, pts, poses, K, hw, kw, colors=None, queries=None, vis_kw=None):
    """Splat, resolve and visible of one case, each equal to the statement; returns the statement's arrays."""
    want_z = CV.splat(pts, poses, K, hw, **kw)
    z = _splat(device, pts, poses, K, hw, **kw)
    assert z.cpu().numpy().view(np.uint64).tobytes() == want_z.tobytes()
    want = CV.resolve(want_z, poses, colors)
    _same(_resolve(device, z, poses, colors, len(pts)), want)
    if queries is not None:
        nf = {k: v for k, v in kw.items() if k in ("near", "far")}
        want_seen = CV.visible(queries, want_z, poses, K, hw, **nf, **vis_kw)
        got = _visible(device, queries, z, poses, K, hw, **nf, **vis_kw)
        assert got.dtype == np.uint8 and got.tobytes() == want_seen.tobytes()
        return want_z, want, want_seen
    return want_z, want


def _options(rng, k, K):
    size = 6.0 / max(K[0, 0], K[1, 1])                    # rho = floor(3 / z): 0 far away, the cap below z = 3 / 8
    return (dict(), dict(radius=1), dict(radius=8), dict(point_size=size), dict(point_size=size, radius=1, max_radius=5),
            dict(near=0.5, far=3.0, radius=2))[k % 6]


def test_sizes(device):
    """Every point count with every image, the view counts and the options cycling through them; queries are the cloud
    and as many points from elsewhere."""
    rng = np.random.default_rng(0)
    hits = shares = 0
    for i, n in enumerate(SIZES_N):
        for j, hw in enumerate(IMAGES):
            V, K = VIEWS[(i + j) % len(VIEWS)], _camera(hw)
            kw = _options(rng, i + 2 * j, K)
            pts, poses = _points(rng, n), _poses(rng, V)
            queries = np.concatenate((pts, _points(rng, n)))
            start = (rng.uniform(size=len(queries)) < 0.2).astype(np.uint8)
            _, res, seen = _check_case(device, pts, poses, K, hw, kw, _colors(rng, n) if (i + j) % 2 else None, queries,
                                       dict(tol=float(rng.choice([0.0, 0.02])), rel_tol=float(rng.choice([0.0, 0.01])),
                                            seen=start))
            assert np.all(seen[start == 1] == 1)                              # rows already set stay set
            hits += int(res[2].sum())
            shares += int(seen.sum()) - int(start.sum())
    assert hits > 1000 and shares > 1000


def test_views_around_the_chunk(device):
    rng = np.random.default_rng(1)
    pts = _points(rng, 257)
    for V in VIEWS:
        hw = (17, 33)
        K = _camera(hw)
        _check_case(device, pts, _poses(rng, V), K, hw, _options(rng, 3, K), _colors(rng, 257), _points(rng, 300),
                    dict(tol=0.01))


def test_mixed_footprints(device):
    """point_size gives every rho from 0 to the cap in one launch."""
    rng = np.random.default_rng(2)
    hw = (17, 33)
    K = _camera(hw)
    pts = (rng.uniform(-0.2, 0.2, (400, 3)) + [0, 0, 0.0]).astype(np.float32)
    pts[:, 2] = np.geomspace(0.2, 8.0, 400).astype(np.float32)
    size = 6.0 / K[1, 1]
    rho = CV.footprint(pts[:, 2].astype(np.float64), K, 0, size, 8)
    assert sorted(set(rho.tolist())) == list(range(9))
    _check_case(device, pts, S.EYE[None], K, hw, dict(point_size=size))
    _check_case(device, pts, _poses(rng, 2), K, hw, dict(point_size=size, max_radius=6))


def test_traps(device):
    """Every hand-computed case of test_cloud_view_cpu.py on the device."""
    for name, points, kw, want in S.SPLAT_CASES:
        _, (rng, index, hit) = _check_case(device, np.asarray(points, np.float32), S.EYE[None], S.K4, S.HW, kw)
        assert np.array_equal(index[0], want), name
    for name, cloud, queries, kw, want in S.VISIBLE_CASES:
        splat_kw = {k: v for k, v in kw.items() if k in SPLAT_KEYS}
        vis_kw = {k: v for k, v in kw.items() if k in ("tol", "rel_tol")}
        seen = _check_case(device, np.asarray(cloud, np.float32), S.EYE[None], S.K4, S.HW, splat_kw,
                           queries=np.asarray(queries, np.float32), vis_kw=vis_kw)[2]
        assert seen.tolist() == want, name


def test_contention(device):
    """1000 points into one 3x3 block of pixels, four f32 ranges among them, three runs: the statement every time."""
    rng = np.random.default_rng(3)
    hw, K = (8, 8), np.array([[4.0, 0, 4.0], [0, 4.0, 4.0], [0, 0, 1.0]])
    z = rng.choice(np.array([1.0, 1.0, 1.0, 1.5, 2.0, 2.5], np.float32), 1000)
    # |x|, |y| < 2^-14: r - z < 2^-28, below half an ulp of f32 at 1, so every range rounds to its z
    pts = np.stack((rng.integers(-200, 200, 1000) * 2.0 ** -22, rng.integers(-200, 200, 1000) * 2.0 ** -22, z), 1)
    pts = pts.astype(np.float32)
    want = CV.splat(pts, S.EYE[None], K, hw, radius=1)
    assert (want != CV.EMPTY).sum() == 9 and len(set(CV.range_bits(np.linalg.norm(pts.astype(np.float64), axis=1)))) == 4
    for _ in range(3):
        got = _splat(device, pts, S.EYE[None], K, hw, radius=1)
        assert got.cpu().numpy().view(np.uint64).tobytes() == want.tobytes()
    # the winner is the lowest index among the points of the smallest f32 range
    r32 = np.linalg.norm(pts.astype(np.float64), axis=1).astype(np.float32)
    assert int(want[0, 4, 4] & np.uint64(0xFFFFFFFF)) == int(np.flatnonzero(r32 == r32.min())[0])


def test_permutation(device):
    rng = np.random.default_rng(4)
    hw = (16, 16)
    K = _camera(hw)
    pts, poses = _points(rng, 1000), _poses(rng, 2)
    perm = rng.permutation(len(pts))
    kw = dict(point_size=6.0 / K[1, 1])
    a = _resolve(device, _splat(device, pts, poses, K, hw, **kw), poses)
    b = _resolve(device, _splat(device, pts[perm], poses, K, hw, **kw), poses)
    hit = a[2] > 0
    assert hit.sum() > 50 and a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes()
    # the same point up to the duplicates, where the lower index of each order wins
    assert np.array_equal(pts[a[1][hit]], pts[perm][b[1][hit]])
    dup = np.isin(a[1][hit], np.arange(0, 1000, 9))
    assert np.array_equal(perm[b[1][hit]][~dup], a[1][hit][~dup])


def test_empty_pixels_observe(device):
    """A sparse cloud on a large image: queries on empty pixels are observed however far behind."""
    rng = np.random.default_rng(5)
    hw = (17, 33)
    K = _camera(hw)
    cloud = np.array([[0, 0, 1.0], [0.3, 0.1, 1.0]], np.float32)
    q = (rng.uniform(-1, 1, (500, 3)) * [2.0, 1.0, 0.0] + [0, 0, 5.0]).astype(np.float32)
    want_z, _, seen = _check_case(device, cloud, S.EYE[None], K, hw, dict(), queries=q, vis_kw=dict(tol=0.0))
    in_view, px, py, _, _ = CV.project(q, S.EYE, K, hw, 0.05, 10.0)
    empty = want_z[0][py, px] == CV.EMPTY
    assert np.array_equal(seen.astype(bool), in_view & empty) and 10 < seen.sum() < 500 and (in_view & ~empty).any()


def _untouched(g):
    return bool((g.raw == g.pat).all())


def test_refusals(device):
    """Bad arguments return MSLAM_EINVAL and write nothing."""
    import mslam_hip as _m

    L, st = _m.lib(), _m.stream_ptr()
    EINVAL = _m.header_constants().get("MSLAM_EINVAL")
    ops = Operands(device)
    p, c = ops.put(np.zeros((4, 3)), np.float32), ops.put(np.tile(S.EYE, (2, 1)), np.float32)
    z = Guarded(device, torch.int64, (2, 4, 5))
    k4 = _k4(S.K4)

    def splat(n=4, V=2, h=4, w=5, near=0.05, far=10.0, radius=0, size=-1.0, max_radius=8, k=k4):
        return L.mslam_cloud_view_splat(_m.ptr(p), n, _m.ptr(c), V, *k, h, w, near, far, radius, size, max_radius,
                                        _m.ptr(z.t), 0, st)

    bad = [splat(n=-1), splat(V=-1), splat(h=-1), splat(w=-1), splat(radius=-1), splat(radius=3, max_radius=2),
           splat(max_radius=9), splat(radius=9, max_radius=9), splat(h=1 << 16, w=1 << 16), splat(V=2, h=1 << 15, w=1 << 15),
           splat(near=2.0, far=1.0), splat(near=math.nan), splat(size=math.inf), splat(k=(math.nan, 4.0, 2.0, 2.0))]
    assert all(rc != 0 for rc in bad) and (EINVAL is None or all(rc == EINVAL for rc in bad))
    assert b"cloud_view_splat" in L.mslam_last_error()
    out = [Guarded(device, torch.float32, (2, 4, 5)), Guarded(device, torch.int32, (2, 4, 5)),
           Guarded(device, torch.uint8, (2, 4, 5)), Guarded(device, torch.uint8, (2, 4, 5, 3))]
    col = ops.put(np.zeros((4, 3)), np.uint8)
    zin = ops.put(np.full((2, 4, 5), -1), np.int64)

    def resolve(V=2, h=4, w=5, n=4, colors=col, rgb=out[3].t):
        return L.mslam_cloud_view_resolve(_m.ptr(zin), _m.ptr(c), V, h, w, _m.ptr(colors), n, _m.ptr(out[0].t),
                                          _m.ptr(out[1].t), _m.ptr(out[2].t), _m.ptr(rgb), st)

    bad = [resolve(V=-1), resolve(h=-2), resolve(n=-1), resolve(h=1 << 16, w=1 << 16), resolve(colors=None),
           resolve(rgb=None)]
    assert all(rc != 0 for rc in bad)
    seen = Guarded(device, torch.uint8, (4,))

    def visible(m=4, V=2, h=4, w=5, near=0.05, far=10.0, tol=0.0, rel_tol=0.0):
        return L.mslam_cloud_view_visible(_m.ptr(p), m, _m.ptr(zin), _m.ptr(c), V, *k4, h, w, near, far, tol, rel_tol,
                                          _m.ptr(seen.t), st)

    bad = [visible(m=-1), visible(V=-1), visible(w=-1), visible(h=1 << 16, w=1 << 16), visible(near=1.0, far=0.5),
           visible(tol=-1.0), visible(rel_tol=-0.5), visible(tol=math.nan)]
    assert all(rc != 0 for rc in bad)
    torch.cuda.synchronize()
    assert all(_untouched(g) for g in [z, seen] + out)
    ops.check()
    # and the same operands are accepted when the arguments are right
    assert splat() == 0 and resolve() == 0 and visible() == 0
    torch.cuda.synchronize()
    assert not _untouched(z) and not _untouched(out[0])


# ----------------------------------------------------------------------------------------------------------------------
# the Python layer
# ----------------------------------------------------------------------------------------------------------------------
def _dev(device, a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(device)


def test_render_cloud(device):
    from mast3r_slam.tsdf import render_cloud

    rng = np.random.default_rng(6)
    hw = (17, 33)
    K = _camera(hw)
    pts, poses, col = _points(rng, 600), _poses(rng, 3), _colors(rng, 600)
    p, c = _dev(device, pts), _dev(device, col, np.uint8)
    for kw in (dict(), dict(radius=1), dict(point_size=6.0 / K[1, 1], near=0.3, far=4.0)):
        want = CV.resolve(CV.splat(pts, poses, K, hw, **kw), poses, col)
        got = render_cloud(p, poses, K, hw, colors=c, **kw)
        assert [tuple(t.shape) for t in got] == [(3, 17, 33)] * 3 + [(3, 17, 33, 3)] and got[2].dtype == torch.bool
        _same([t.cpu().numpy() for t in (got[0], got[1], got[2].to(torch.uint8), got[3])], want)
        plain = render_cloud(p, torch.from_numpy(poses), K, hw, **kw)
        assert len(plain) == 3 and all(torch.equal(a, b) for a, b in zip(plain, got))
        one = render_cloud(p, poses[1], K, hw, colors=c, **kw)
        assert tuple(one[0].shape) == hw and tuple(one[3].shape) == hw + (3,)
        assert all(torch.equal(a, b[1]) for a, b in zip(one, got))
        assert want[2].sum() > 20
    # range * ray is the camera-frame point: the winner, moved into the camera, up to the f32 rounding of the range
    rng_, idx, hit = render_cloud(p, poses[0], K, hw)
    T = poses[0].astype(np.float64)
    cam = synthetic.sim3_act(synthetic.sim3_inv(T), pts[idx.cpu().numpy()[hit.cpu().numpy()]].astype(np.float64))
    assert np.allclose(np.linalg.norm(cam, axis=1), rng_.cpu().numpy()[hit.cpu().numpy()], rtol=1e-5)
    empty = render_cloud(p[:0], poses[0], K, hw)
    assert not empty[2].any() and (empty[1] == -1).all() and (empty[0] == 0).all()
    with pytest.raises(ValueError, match="max_radius"):
        render_cloud(p, poses[0], K, hw, radius=9, max_radius=9)
    with pytest.raises(ValueError, match="hw"):
        render_cloud(p, poses[0], K, None)
    with pytest.raises(ValueError, match="point_size"):
        render_cloud(p, poses[0], K, hw, point_size=-1.0)
    with pytest.raises(ValueError, match=r"colors must be \(600,3\)"):
        render_cloud(p, poses[0], K, hw, colors=c[:5])
    with pytest.raises(TypeError, match="device tensor"):
        render_cloud(pts, poses[0], K, hw)
    with pytest.raises(ValueError, match="pose"):
        render_cloud(p, poses[0][:7], K, hw)


@pytest.fixture(scope="module")
def room():
    pts, V, F = S.lattice_room()
    return pts, S.plate_cameras()


def test_observed_cloud_points(device, room):
    from mast3r_slam.tsdf import observed_cloud_points

    rng = np.random.default_rng(7)
    hw = (17, 33)
    K = _camera(hw)
    cloud, q, poses = _points(rng, 1000), _points(rng, 700), _poses(rng, 9)
    c, qd = _dev(device, cloud), _dev(device, q)
    for kw in (dict(), dict(tol=0.0), dict(point_size=6.0 / K[1, 1]), dict(radius=2, rel_tol=0.02, near=0.3, far=4.0)):
        want = CV.observed(q, cloud, poses, K, hw, **kw)
        for chunk in (1, 3, 8):
            got = observed_cloud_points(qd, c, poses, K, hw, chunk=chunk, **kw)
            assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want), (kw, chunk)
        assert 0.02 < want.mean() < 0.98
    me = observed_cloud_points(c, c, poses, K, hw, tol=0.0)
    assert np.array_equal(me.cpu().numpy(), CV.observed(cloud, cloud, poses, K, hw, tol=0.0))
    assert not observed_cloud_points(qd, c, poses[:0], K, hw).any()
    assert observed_cloud_points(qd[:0], c, poses, K, hw).shape == (0,)
    # the lattice room at 48x64, as in the CPU file
    pts, cams = room
    K2, hw2 = synthetic.intrinsics(48, 64), (48, 64)
    want = CV.observed(pts, pts, cams, K2, hw2, point_size=2 * S.SPACING)
    d = _dev(device, pts)
    got = observed_cloud_points(d, d, cams, K2, hw2, point_size=2 * S.SPACING)
    assert np.array_equal(got.cpu().numpy(), want) and 0.1 < want.mean() < 0.9
    with pytest.raises(ValueError, match="chunk"):
        observed_cloud_points(qd, c, poses, K, hw, chunk=0)
    with pytest.raises(ValueError, match="tol"):
        observed_cloud_points(qd, c, poses, K, hw, tol=-1.0)


EXACT = ("accuracy_median", "completion_median", "precision", "recall", "n_pred", "n_gt", "accuracy_outliers",
         "completion_outliers")
SUMS = ("accuracy", "completion", "accuracy_rmse", "completion_rmse")


def test_compare_clouds_observed(device, room):
    """compare_clouds(observed=...) against figures assembled in numpy from the statement's mask of the thinned ground
    truth: the accuracy half is the full comparison's, bit for bit, the completion half is taken over the mask."""
    from mast3r_slam.tsdf import compare_clouds, downsample_cloud

    gt, cams = room
    rng = np.random.default_rng(8)
    seen_all = CV.observed(gt, gt, cams, synthetic.intrinsics(48, 64), (48, 64), point_size=0.1)
    pred = (gt[seen_all][::2] + rng.normal(0, 0.01, (int(seen_all.sum() + 1) // 2, 3))).astype(np.float32)
    K, hw, voxel, thr = synthetic.intrinsics(48, 64), (48, 64), 0.05, 0.05
    p, g = _dev(device, pred), _dev(device, gt)
    plain = compare_clouds(p, g, threshold=thr, voxel=voxel)
    got = compare_clouds(p, g, threshold=thr, voxel=voxel, observed=dict(poses=cams, K=K, hw=hw))
    pp, gg = downsample_cloud(p, voxel)[0].cpu().numpy(), downsample_cloud(g, voxel)[0].cpu().numpy()
    mask = CV.observed(gg, gg, cams, K, hw, point_size=2 * voxel)
    acc, comp = C._direction(pp, gg, thr, np.inf), C._direction(gg[mask], pp, thr, np.inf)
    want = dict(accuracy=acc["mean"], accuracy_median=acc["median"], accuracy_rmse=acc["rmse"], precision=acc["within"],
                n_pred=acc["n"], accuracy_outliers=0, completion=comp["mean"], completion_median=comp["median"],
                completion_rmse=comp["rmse"], recall=comp["within"], n_gt=comp["n"], completion_outliers=0)
    n = max(want["n_pred"], len(gg))
    for k in EXACT:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in SUMS:
        assert abs(got[k] - want[k]) <= n * 2.0 ** -52 * want[k], (k, got[k], want[k])
    pr, rc = want["precision"], want["recall"]
    assert abs(got["fscore"] - 2.0 * pr * rc / (pr + rc)) <= 2.0 ** -51
    assert abs(got["chamfer"] - 0.5 * (want["accuracy"] + want["completion"])) <= n * 2.0 ** -52 * got["chamfer"]
    assert got["n_gt_observed"] == int(mask.sum()) == got["n_gt"] and got["gt_observed_share"] == mask.sum() / len(gg)
    assert 0.1 < got["gt_observed_share"] < 0.9
    for k in ("accuracy", "accuracy_median", "accuracy_rmse", "precision", "n_pred", "accuracy_outliers"):
        assert got[k] == plain[k], k                                          # bit for bit
    assert "gt_observed_share" not in plain and got["recall"] > plain["recall"] and plain["n_gt"] == len(gg)
    print(f"lattice room, {len(gg)} thinned points, {got['n_gt_observed']} observed: recall {plain['recall']:.4f} -> "
          f"{got['recall']:.4f}, completion {plain['completion']:.4f} -> {got['completion']:.4f}")
    # explicit options are the defaults' equals; normals ride along, the accuracy half unchanged
    same = compare_clouds(p, g, threshold=thr, voxel=voxel,
                          observed=dict(poses=cams, K=K, hw=hw, point_size=2 * voxel, tol=4 * voxel, frame="gt"))
    assert same == got
    nrm = compare_clouds(p, g, threshold=thr, voxel=voxel, normals=8, observed=dict(poses=cams, K=K, hw=hw))
    nrm_plain = compare_clouds(p, g, threshold=thr, voxel=voxel, normals=8)
    assert nrm["normal_consistency_accuracy"] == nrm_plain["normal_consistency_accuracy"]
    assert {k: nrm[k] for k in got} == got and math.isfinite(nrm["normal_consistency_completion"])
    # frame: the poses lie in pred's frame and the alignment moves them; the mask is that of the composed poses
    import meshalign_numpy as A
    import raycast_numpy as R

    move = A.sim3_from((10.0, (0.2, 1.0, 0.1)), (0.3, -0.2, 0.1), 1.25)
    inv = A.sim3_inv(move)
    p_moved = _dev(device, A.act(inv, pred.astype(np.float64)))
    cams_pred = np.stack([R.compose(inv, c) for c in cams])
    in_pred = compare_clouds(p_moved, g, threshold=thr, voxel=voxel, align=move,
                             observed=dict(poses=cams_pred, K=K, hw=hw, frame="pred"))
    back = np.stack([R.compose(move, c) for c in cams_pred]).astype(np.float32)
    mask2 = CV.observed(gg, gg, back, K, hw, point_size=2 * voxel)
    # compose_sim3 and raycast_numpy.compose are one f64 formula on the host, so the cameras are the same bits; against
    # the cameras themselves the moved ones carry a rounding (1e-6 m at most), which moves every pixel border by as much,
    # and the lattice lines its points up along them: that part agrees up to 0.5 % of the points
    assert in_pred["n_gt_observed"] == int(mask2.sum())
    assert abs(int(mask2.sum()) - int(mask.sum())) <= 0.005 * len(gg)
    in_gt = compare_clouds(p_moved, g, threshold=thr, voxel=voxel, align=move, observed=dict(poses=cams, K=K, hw=hw))
    assert in_gt["n_gt_observed"] == int(mask.sum())
    # refusals
    with pytest.raises(ValueError, match="voxel.*point_size.*radius"):
        compare_clouds(p, g, threshold=thr, observed=dict(poses=cams, K=K, hw=hw))
    with pytest.raises(ValueError, match="needs poses, K and hw"):
        compare_clouds(p, g, voxel=voxel, observed=dict(poses=cams, K=K))
    with pytest.raises(ValueError, match="needs poses, K and hw"):
        compare_clouds(p, g, voxel=voxel, observed=dict(poses=cams, K=K, hw=hw, skip=True))
    with pytest.raises(ValueError, match="'gt' or 'pred'"):
        compare_clouds(p, g, voxel=voxel, observed=dict(poses=cams, K=K, hw=hw, frame="map"))
    away = np.array([[0, 0, 50.0, 0, 0, 0, 1, 1]], np.float32)
    with pytest.raises(ValueError, match="no ground-truth point is observed"):
        compare_clouds(p, g, voxel=voxel, observed=dict(poses=away, K=K, hw=hw))
    by_radius = compare_clouds(p, g, threshold=thr, observed=dict(poses=cams, K=K, hw=hw, radius=1))
    assert by_radius["n_gt_observed"] == int(CV.observed(gt, gt, cams, K, hw, radius=1).sum())


# ----------------------------------------------------------------------------------------------------------------------
# the product
# ----------------------------------------------------------------------------------------------------------------------
def test_slam_system_cloud_views(device, monkeypatch):
    """The 20-frame run of test_cloud_gpu.test_slam_system_cloud, scored against the lattice room cloud: the cull keeps
    a part of the ground truth and raises recall, accuracy and precision stay bit for bit, and the map's TSDF agrees in
    depth with the splatted scan."""
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from test_slam_system_gpu import H, W, RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    gt = S.lattice_room()[0]
    K = synthetic.intrinsics(H, W)
    thr = 2.0                                                               # the room's confidences lie in [1, 3]
    frames = _frames(list(range(0, 60, 3)), device)
    for f in frames:
        f.uimg = torch.rand(f.uimg.shape, generator=torch.Generator().manual_seed(f.frame_id))
    try:
        system.run(frames)
        every = system.evaluate_cloud(gt, conf_threshold=thr)
        seen = system.evaluate_cloud(gt, conf_threshold=thr, observed=True, gt_K=K)
        wide = system.evaluate_cloud(gt, conf_threshold=thr, observed=dict(point_size=0.2), gt_K=K)
        depth = system.evaluate_cloud_depth(gt, gt_K=K)
        view = system.render_cloud_view(K=K)
        n_kf = len(system.keyframes)
        with pytest.raises(ValueError, match="no projection"):
            system.evaluate_cloud(gt, conf_threshold=thr, observed=True)
        with pytest.raises(ValueError, match="no projection"):
            system.evaluate_cloud_depth(gt)
        with pytest.raises(ValueError, match="no projection"):
            system.render_cloud_view()
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    print(f"{n_kf} keyframes; observed share {seen['gt_observed_share']:.4f} ({seen['n_gt_observed']} of {every['n_gt']}); "
          f"recall {every['recall']:.4f} -> {seen['recall']:.4f}, completion {every['completion']:.4f} -> "
          f"{seen['completion']:.4f}; depth L1 {depth['depth_l1']:.5f} over {depth['both_hit_share']:.3f} of the pixels")
    assert 0.0 < seen["gt_observed_share"] < 1.0 and seen["n_gt_observed"] == seen["n_gt"] < every["n_gt"]
    assert seen["recall"] > every["recall"]
    for k in ("accuracy", "accuracy_median", "accuracy_rmse", "precision", "n_pred"):
        assert seen[k] == every[k] == wide[k], k
    assert 0.0 < wide["gt_observed_share"] < 1.0
    assert all(math.isfinite(depth[k]) for k in ("depth_l1", "depth_l1_median", "both_hit_share"))
    assert depth["both_hit_share"] > 0.0 and depth["n_pixels"] == n_kf * H * W
    rng_, idx, hit, rgb = view
    assert tuple(rng_.shape) == (H, W) == tuple(hit.shape) and tuple(rgb.shape) == (H, W, 3) and rgb.dtype == torch.uint8
    assert hit.any() and (idx[hit] >= 0).all() and (rng_[hit] > 0).all()
