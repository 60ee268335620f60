"""CPU tests (-m "not gpu") of the global-TSDF view rendering: the C ABI of the ray cast, and the numpy statement of the
march (tests/render_numpy.py) on analytic volumes and on the oracle's fused room.  Bounds:
* plane (a linear field: trilinear sampling and the secant between two samples are exact): range within 1e-9 voxel;
* sphere: range within 9 h / (16 rho) voxel and normals within asin(3.1 h / rho), derived in the test;
* room: hit points within 0.28 voxel of the walls (observed max 0.224 voxel, + 25 %), every normal into the room."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_numpy as R  # noqa: E402

from mast3r_slam import synthetic  # noqa: E402

VS = 0.03
EYE = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0], np.float32)


def test_library_exports_the_render_entry_points():
    import mslam_hip

    assert os.path.exists(mslam_hip.LIB_PATH), "build libmslam_hip.so first (__graft_entry__.build())"
    handle = ctypes.CDLL(mslam_hip.LIB_PATH)
    names = ("mslam_tsdf_render_workspace_bytes", "mslam_tsdf_render_blocks", "mslam_tsdf_render")
    for s in names:
        assert hasattr(handle, s), f"{s} not exported"
        assert s in mslam_hip.exported_symbols()
    L = mslam_hip.lib()
    assert L.mslam_tsdf_render_workspace_bytes(1000) == 0                 # not a power of two
    assert L.mslam_tsdf_render_workspace_bytes(1 << 20) >= (1 << 20) // 4 * 8
    # argument checks happen before any device work
    assert L.mslam_tsdf_render_blocks(None, 1 << 20, 0.0, None, 0, None) != 0
    assert b"null pointer" in L.mslam_last_error()
    from mast3r_slam.tsdf import TSDFVolume, render_from_voxels  # noqa: F401

    assert callable(TSDFVolume.render)


def _pose(t, rotvec, s=1.0):
    return np.concatenate((t, synthetic.quat_from_rotvec(np.asarray(rotvec, np.float64)), [s])).astype(np.float32)


def test_plane_is_rendered_to_rounding():
    """f(p) = c - n.p with a normal off every axis, band of +-4 voxels inside a box.  The field is linear, so the
    trilinear sample equals f and the secant through two samples crosses the level where f does: the range differs from
    the analytic one by rounding only (1e-9 voxel), the normal is -n."""
    n = np.array([0.3, -0.45, 0.84])
    n /= np.linalg.norm(n)
    c = 1.7
    lo, hi = np.array([-1.2, -1.2, 0.8]), np.array([1.2, 1.2, 3.2])
    k, v, w = R.sample_sdf(lambda p: c - p @ n, lo, hi, VS, 4 * VS)
    for pose, level in ((EYE, 0.0), (_pose([0.1, -0.2, 0.3], [0.1, 0.2, -0.15], 0.8), 0.0), (EYE, 0.02)):
        rays = R.unit_rays(36, 48, synthetic.intrinsics(36, 48))
        rng, nrm, hit = R.render(k, v, w, VS, 0.5, pose, rays, far=4.0, level=level, dtype=np.float64)
        d = R.ray_dirs(pose, rays).reshape(36, 48, 3)
        o, s = pose[:3].astype(np.float64), float(pose[7])
        cos = d @ n
        with np.errstate(divide="ignore"):
            t_true = (c - level - o @ n) / cos
        P = o + t_true[..., None] * d
        # the ray crosses the band |f| <= 4 h within 8 h of the hit when cos >= 0.5: keep that stretch inside the box
        must = (cos >= 0.5) & (t_true > 0.3) & ((P > lo + 9 * VS) & (P < hi - 9 * VS)).all(-1)
        assert must.sum() > 200
        assert hit[must].all()
        err = np.abs(rng * s - t_true)[must].max() / VS
        print(f"plane: {int(must.sum())} rays, max range error {err:.3g} voxel")
        assert err <= 1e-9
        assert np.abs(nrm[must] + n).max() <= 1e-9


def test_sphere_range_and_normals_within_the_curvature_bound():
    """Sphere of radius r seen from outside, h = voxel size, rho = distance to the centre (>= r - h around the surface).
    The SDF |p - c| - r has second derivatives (I - n n^T) / rho: pure ones sum to 2 / rho, mixed ones are <= 1 / (2 rho).
    * Trilinear interpolation: |F - f| <= sum_i h^2 / 8 |d_ii f| = h^2 / (4 rho).
    * The secant between samples step = h / 2 apart: f along the ray has |f''| <= 1 / rho, so its secant is within
      step^2 / (8 rho) = h^2 / (32 rho) of f, and the secant of the interpolation error is within h^2 / (4 rho).
      At the located range |f - level| <= 9 h^2 / (32 rho).
    * f falls along the ray at rate cos(incidence); for cos >= 0.5 the range error is <= 9 h^2 / (16 rho), i.e.
      9 h / (16 rho) voxel: 0.036 voxel for r = 0.5, h = 0.03.
    * Gradient: each component of the interpolant's gradient is an edge difference quotient (within h / 2 |d_ii f| of the
      derivative) blended across the cell (the derivative changes by <= h (|d_ij f| + |d_ik f|) there): 1.5 h / rho per
      component, 2.6 h / rho as a vector; blending the two samples' gradients adds the true gradient's change over one
      step, 0.5 h / rho.  Angle <= asin(3.1 h / rho) = 11.4 degrees here.
    Rays with cos >= 0.5 stay in the band long enough to have valid samples on both sides of the surface: all hit."""
    c, r = np.array([0.02, -0.01, 2.0]), 0.5
    k, v, w = R.sample_sdf(lambda p: np.linalg.norm(p - c, axis=-1) - r, c - r - 5 * VS, c + r + 5 * VS, VS, 4 * VS)
    rho = r - VS
    bound_range = 9.0 * VS / (16.0 * rho)
    bound_angle = np.arcsin(3.1 * VS / rho)
    for pose in (EYE, _pose([0.3, 0.2, 0.1], [0.1, -0.15, 0.3], 1.3)):
        rays = R.unit_rays(48, 64, synthetic.intrinsics(48, 64))
        rng, nrm, hit = R.render(k, v, w, VS, 0.5, pose, rays, far=4.0, dtype=np.float64)
        d = R.ray_dirs(pose, rays).reshape(48, 64, 3)
        o, s = pose[:3].astype(np.float64), float(pose[7])
        b = d @ (o - c)
        disc = b * b - ((o - c) @ (o - c) - r * r)
        t_true = -b - np.sqrt(np.maximum(disc, 0.0))
        n_true = (o + t_true[..., None] * d - c) / r
        must = (disc > 0) & (-(n_true * d).sum(-1) >= 0.5)
        assert must.sum() > 100
        assert hit[must].all()
        err = np.abs(rng * s - t_true)[must].max() / VS
        ang = np.arccos(np.clip((nrm[must] * n_true[must]).sum(-1), -1.0, 1.0)).max()
        print(f"sphere: {int(must.sum())} rays, max range error {err:.4f} voxel (bound {bound_range:.4f}), "
              f"max normal angle {np.degrees(ang):.3f} deg (bound {np.degrees(bound_angle):.2f})")
        assert err <= bound_range
        assert ang <= bound_angle
        # rays that pass the sphere by more than the band see nothing
        clear = disc < -((r + 6 * VS) ** 2 - r * r)
        assert not hit[clear].any()


def test_room_view_from_the_oracle_lies_on_the_walls():
    """The oracle's fused room (the volume of test_room_mesh_from_the_oracle_lies_on_the_walls) seen from poses of the
    trajectory that were not fused (frames 15, 5, 25; frames 0, 10, 20 were).  Perpendicular distance of every hit point
    to the nearest wall: observed max 0.224 voxel (0.224 / 0.216 / 0.219 for the three poses), bound 0.28 = observed
    + 25 % (the marching-cubes surface of the same data: observed 0.46, bound 0.5).  Every normal points into the room.
    Of the rays whose analytic hit point lies within one voxel of a valid voxel's centre at least 90 % must hit
    (observed 99.9 / 99.9 / 98.9 %)."""
    import oracle

    ref = oracle.TSDFVolume(VS, 0.12)
    for kf in range(3):
        T = synthetic.camera_pose(kf * 10)
        X = synthetic.render_pointmap(T, 96, 128).reshape(-1, 3)
        rng = np.random.default_rng(kf)
        ref.integrate(synthetic.sim3_act(T, X).astype(np.float32), rng.uniform(0.5, 2.0, len(X)),
                      T[:3].astype(np.float32))
    k, t, w = ref.voxels()
    ok = w >= 1.0e-3
    pk = np.sort(R.pack(k[ok]))
    H = synthetic.ROOM_HALF
    h, wd = 48, 64
    rays = R.unit_rays(h, wd, synthetic.intrinsics(h, wd))
    off = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    for frame in (15, 5, 25):
        pose = synthetic.camera_pose(frame).astype(np.float32)
        r, n, hit = R.render(k, t, w, VS, 1.0e-3, pose, rays, far=8.0, dtype=np.float64)
        d = R.ray_dirs(pose, rays).reshape(h, wd, 3)
        o = pose[:3].astype(np.float64)
        P = (o + r[..., None] * d)[hit]
        gap = np.abs(H[None] - np.abs(P))
        a = np.argmin(gap, 1)
        inward = -np.sign(P[np.arange(len(P)), a])
        into_room = n[hit][np.arange(len(P)), a] * inward > 0
        # analytic hit points that lie within one voxel of a valid voxel's centre
        Pa = (o + synthetic.ray_box_depth(o, d.reshape(-1, 3))[:, None] * d.reshape(-1, 3))
        cand = np.floor(Pa / VS).astype(np.int64)[:, None, :] + off[None]
        dist = np.linalg.norm((cand + 0.5) * VS - Pa[:, None, :], axis=-1)
        q = R.pack(cand)
        pos = np.minimum(np.searchsorted(pk, q), len(pk) - 1)
        near = ((pk[pos] == q) & (dist <= VS)).any(1).reshape(h, wd)
        print(f"room frame {frame}: {hit.mean():.4f} of the rays hit, {hit[near].mean():.4f} of the {int(near.sum())} "
              f"near a valid voxel; max wall distance {gap.min(1).max() / VS:.4f} voxel")
        assert near.mean() > 0.9
        assert hit[near].mean() >= 0.9
        assert gap.min(1).max() < 0.28 * VS
        assert into_room.all()


def test_depth_view_pngs_round_trip(tmp_path):
    from PIL import Image

    from mast3r_slam import evaluate

    g = np.random.default_rng(2)
    rng = g.uniform(0.2, 9.0, (5, 7)).astype(np.float32)
    rng[0, 0] = 70.0                                                   # beyond 16 bits of millimetres: clipped
    nrm = g.normal(size=(5, 7, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    hit = g.uniform(size=(5, 7)) > 0.3
    hit[0, 0] = True
    dp, npth = evaluate.save_depth_view(tmp_path / "views", "kf3.png", rng, nrm, hit)
    assert dp.name == "kf3_depth.png" and npth.name == "kf3_normal.png"
    d, n = Image.open(dp), Image.open(npth)
    assert d.mode.startswith("I;16") and n.mode == "RGB"
    d, n = np.asarray(d).astype(np.int64), np.asarray(n)
    want = np.where(hit, np.clip(np.rint(rng.astype(np.float64) * 1000.0), 0, 65535), 0).astype(np.int64)
    assert np.array_equal(d, want) and d[0, 0] == 65535
    assert np.array_equal(n, np.where(hit[..., None], np.rint(0.5 * (nrm.astype(np.float64) + 1.0) * 255.0), 0).astype(np.uint8))
    # world-frame normals with the view's pose: the rotation is undone
    pose = _pose([1.0, 2.0, 3.0], [0.2, -0.4, 0.1], 1.5)
    world = synthetic.quat_rotate(pose[3:7].astype(np.float64), nrm.astype(np.float64).reshape(-1, 3)).reshape(nrm.shape)
    _, np2 = evaluate.save_depth_view(tmp_path, "w.png", rng, world, hit, pose=pose)
    assert np.abs(np.asarray(Image.open(np2)).astype(np.int64) - n.astype(np.int64)).max() <= 1
