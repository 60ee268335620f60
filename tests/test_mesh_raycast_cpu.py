"""CPU tests of the numpy statement of the mesh ray caster (tests/raycast_numpy.py, DESIGN.md "Mesh ray casting"): the
room against synthetic.ray_box_depth, rays aimed at corners, edges and wall diagonals, hand cases, and the observed
rule on a scene whose mask follows from the geometry.

The bound on t against ray_box_depth.  u = 2^-53, L the largest |v - o| coordinate in play, d the ray with |d| >= 1 and
|d[kz]| >= |d| / sqrt 3.  A sheared x = q[kx] - Sx q[kz] carries |dx| <= 6 u L (one rounding in each q, in S, in the
product and in the difference; |S| <= 1), an edge function x y' - y x' of |x|, |y| <= 2 L therefore |dU| <= 64 u L^2.
t = sum U_i z_i / det moves by sum dU_i (z_i - t) / det with |z_i - t| <= 2 sqrt 3 L, and det is twice the face's area
seen along the ray, >= 2 A cos(theta) for a face of area A whose normal makes the angle theta with the ray; the
roundings of the sum and the quotient add 8 u sqrt 3 L.  ray_box_depth itself is two roundings of t.  Together
    |t - t_box| <= u (384 sqrt 3 L^3 / (2 A cos theta) + 14 L) + 4 u t ,
with A = 6 m^2, the room's smallest triangle, and L = 4.5 m (|o| <= 1.2 m inside a room of half-width 3 m)."""
import os
import sys

import numpy as np

from mast3r_slam import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raycast_numpy as R  # noqa: E402

U53 = 2.0 ** -53
IDENT = np.array([0, 0, 0, 0, 0, 0, 1, 1], np.float32)


def wall_cos(o, d):
    """cos of the angle between each ray and the normal of the wall it hits."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (synthetic.ROOM_HALF - o) / d, (-synthetic.ROOM_HALF - o) / d)
    t = np.where(np.abs(d) < 1e-12, np.inf, t)
    a = np.argmin(t, 1)
    return np.abs(np.take_along_axis(d, a[:, None], 1)[:, 0]) / np.linalg.norm(d, axis=1)


def t_bound(o, d, t):
    L, A = 4.5, 6.0
    return U53 * (384.0 * np.sqrt(3.0) * L ** 3 / (2.0 * A * wall_cos(o, d)) + 14.0 * L) + 4.0 * U53 * t


def test_room_against_ray_box_depth():
    V, F = synthetic.room_mesh()
    h, w = 48, 64
    rays = synthetic.pixel_rays(h, w, synthetic.intrinsics(h, w)).reshape(-1, 3).astype(np.float32)
    worst = 0.0
    for k in (0, 7, 100, 333, 512, 999):
        pose = synthetic.camera_pose(k).astype(np.float32)
        o, d, _ = R.directions(pose, rays)
        assert np.abs(o).max() <= 1.2001 and np.linalg.norm(d, axis=1).min() >= 1.0 - 1e-6
        t64, face = R.cast(o, d, V, F, 0.0, np.inf)
        assert (face >= 0).all() and np.isfinite(t64).all()                # no miss
        want = synthetic.ray_box_depth(o, d)
        err, bound = np.abs(t64 - want), t_bound(o, d, want)
        assert (err <= bound).all(), (k, (err / bound).max())
        worst = max(worst, float((err / want).max()))
        # the face hit lies on the wall ray_box_depth found: its three corners share that coordinate
        p = o + want[:, None] * d
        a = np.argmin(np.abs(np.abs(p) - synthetic.ROOM_HALF), 1)
        tri = V[F[face]]                                                   # (n, 3, 3)
        plane = np.take_along_axis(tri, a[:, None, None].repeat(3, 1), 2)[:, :, 0]
        assert (plane == plane[:, :1]).all()
        rng, nrm, hit, face2, t2 = R.render(pose, rays, V, F, 0.05, 10.0)
        assert hit.all() and np.array_equal(face2, face) and np.array_equal(t2, t64)
        assert np.array_equal(rng, t64.astype(np.float32))                 # scale 1
        assert (np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0) <= 1e-6).all()
        assert ((nrm.astype(np.float64) * d).sum(1) < 0.0).all()           # towards the camera
    print(f"room 48x64, 6 poses: largest relative difference to ray_box_depth {worst:.3g}")


def test_corners_edges_and_diagonals_all_hit():
    """Rays through vertices, along edges' points and through the walls' diagonals - the edges two faces share - from
    random interior origins: watertight means every one hits."""
    V, F = synthetic.room_mesh()
    rng = np.random.default_rng(5)
    Vd = V.astype(np.float64)
    targets = [Vd]
    for a, b in {tuple(sorted(e)) for f in F for e in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0]))}:
        s = np.concatenate([np.linspace(0.0, 1.0, 9), rng.uniform(0.0, 1.0, 8)])[:, None]
        targets.append(Vd[a] + s * (Vd[b] - Vd[a]))                        # 12 box edges and 6 diagonals
    targets = np.concatenate(targets)
    misses = 0
    for _ in range(40):
        o = (rng.uniform(-0.95, 0.95, 3) * synthetic.ROOM_HALF).astype(np.float32)
        d = (targets - o.astype(np.float64)).astype(np.float32)
        for scale in (1.0, 0.37):                                          # the target at t = 1 and at t = 1 / 0.37
            t64, face = R.cast(o.astype(np.float64), (d * np.float32(scale)).astype(np.float64), V, F, 0.0, np.inf)
            misses += int((face < 0).sum())
            assert (np.abs(t64 * scale - 1.0) <= 1e-6).all()
    assert misses == 0


def _tri(z=2.0, flip=False):
    V = np.array([[-1, -1, z], [1, -1, z], [0, 1, z]], np.float32)
    return V, np.array([[0, 2, 1] if flip else [0, 1, 2]], np.int32)


def test_hand_cases():
    o = np.zeros(3)
    up = np.array([[0.0, 0.0, 1.0]])
    V, F = _tri()
    # the tie rule: two coincident faces, the lowest index wins whatever their winding
    for faces in ([[0, 1, 2], [0, 1, 2]], [[0, 2, 1], [0, 1, 2]], [[1, 2, 0], [2, 1, 0]]):
        t, f = R.cast(o, up, V, np.array(faces, np.int32), 0.0, 10.0)
        assert t[0] == 2.0 and f[0] == 0
    # back faces are hit, and the normal faces the origin either way
    for flip in (False, True):
        rng, nrm, hit, f, t = R.render(IDENT, up, *_tri(flip=flip), 0.05, 10.0)
        assert hit[0] == 1 and f[0] == 0 and t[0] == 2.0 and rng[0] == 2.0 and np.array_equal(nrm[0], [0, 0, -1])
    # a scaled pose: range is t / s
    pose = np.array([0, 0, 0, 0, 0, 0, 1, 4], np.float32)
    assert R.render(pose, up, V, F, 0.05, 10.0)[0][0] == 0.5
    # near and far are inclusive
    assert R.cast(o, up, V, F, 2.0, 10.0)[1][0] == 0 and R.cast(o, up, V, F, 0.0, 2.0)[1][0] == 0
    assert R.cast(o, up, V, F, np.nextafter(2.0, 3.0), 10.0)[1][0] == -1
    assert R.cast(o, up, V, F, 0.0, np.nextafter(2.0, 1.0))[1][0] == -1
    # behind the origin: t < 0 is outside [near, far]
    assert R.cast(o, -up, V, F, 0.0, np.inf)[1][0] == -1
    # a ray in the face's plane has U = V = W = 0: a miss
    t, f = R.cast(np.array([-3.0, 0.0, 2.0]), np.array([[1.0, 0.0, 0.0], [1.0, 0.25, 0.0]]), V, F, 0.0, np.inf)
    assert (f == -1).all() and np.isinf(t).all()
    # a degenerate face and faces out of range are skipped: the valid face behind them is hit
    V2 = np.concatenate([np.array([[-1, 0, 1], [0, 0, 1], [1, 0, 1]], np.float32), V])
    F2 = np.array([[0, 1, 2], [0, 0, 1], [3, 4, 9], [-1, 3, 4], [3, 4, 5]], np.int32)
    t, f = R.cast(o, up, V2, F2, 0.0, np.inf)
    assert t[0] == 2.0 and f[0] == 4
    assert R.cast(o, up, V2, F2[:4], 0.0, np.inf)[1][0] == -1 and R.cast(o, up, V2, F2[:0], 0.0, np.inf)[1][0] == -1
    # a zero or non-finite direction misses
    bad = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 1.0], [0.0, np.inf, 1.0]])
    big = np.array([[-9, -9, 2], [9, -9, 2], [0, 9, 2]], np.float32)
    t, f = R.cast(o, bad, big, F, 0.0, np.inf)
    assert (f == -1).all() and np.isinf(t).all()
    rng, nrm, hit, f, t = R.render(IDENT, bad[:1], big, F)
    assert rng[0] == 0.0 and not nrm.any() and hit[0] == 0
    # kz is the FIRST axis of largest |d|, and the winding swap for d[kz] < 0 keeps the hit
    for d in ([1.0, 1.0, 1.0], [-1.0, -1.0, -1.0], [0.0, -1.0, 1.0]):
        d = np.array([d])
        W = (3.0 * d + np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0.5]])).astype(np.float32)
        t, f = R.cast(o, d, W, F, 0.0, np.inf)
        assert f[0] == 0 and abs(t[0] - 3.0) < 0.5


def occluder_scene():
    """The room plus a quad at z = 0.75, |x|, |y| <= 0.25, in front of the wall z = 1.5 for a camera at the origin that
    looks along +z with f = 40 px at 48x64: the quad's shadow on the wall is |x|, |y| <= 0.5, and the wall is in view
    for -0.8125 <= x / z < 0.7875, -0.6125 <= y / z < 0.5875.  Returns (V, F, poses, K, hw, points, want)."""
    V, F = synthetic.room_mesh()
    quad = np.array([[-0.25, -0.25, 0.75], [0.25, -0.25, 0.75], [0.25, 0.25, 0.75], [-0.25, 0.25, 0.75]], np.float32)
    V = np.concatenate([V, quad])
    F = np.concatenate([F, np.array([[8, 9, 10], [8, 10, 11]], np.int32)])
    K = np.array([[40.0, 0, 32.0], [0, 40.0, 24.0], [0, 0, 1.0]])
    hw = (48, 64)
    g = -1.4 + 0.1 * np.arange(28) + 0.0137
    x, y = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    wall = np.stack([x, y, np.full_like(x, 1.5)], 1)
    for a, lo, hi in ((x, -0.8125, 0.7875), (y, -0.6125, 0.5875)):           # no point within 1e-3 of a border
        assert min(np.abs(a / 1.5 - lo).min(), np.abs(a / 1.5 - hi).min(), np.abs(np.abs(a) - 0.5).min()) > 1e-3
    in_view = (x / 1.5 >= -0.8125) & (x / 1.5 < 0.7875) & (y / 1.5 >= -0.6125) & (y / 1.5 < 0.5875)
    shadow = (np.abs(x) < 0.5) & (np.abs(y) < 0.5)
    pts, want = [wall], [in_view & ~shadow]
    on_quad = np.array([[0.1, -0.2, 0.75], [-0.2, 0.05, 0.75], [0.0, 0.0, 0.75]])
    r = np.linalg.norm(on_quad, axis=1, keepdims=True)
    pts += [on_quad, on_quad * (1.0 + 0.005 / r), on_quad * (1.0 + 0.02 / r)]   # on it, 5 mm behind it (tol), 2 cm
    want += [np.ones(3, bool), np.ones(3, bool), np.zeros(3, bool)]
    pts.append(np.array([[0.0, 0.0, -1.5], [0.3, 0.2, -1.0],                 # behind the camera
                         [0.0, 0.0, 0.04], [0.0, 0.0, 0.06],                 # nearer than near = 0.05, and just not
                         [0.9, 0.0, 1.0], [-0.7, 0.5, 1.0], [0.0, 0.7, 1.0]]))   # free space beside the quad: out, in, out
    want.append(np.array([False, False, False, True, False, True, False]))
    return V, F, IDENT[None], K, hw, np.concatenate(pts).astype(np.float32), np.concatenate(want)


def test_observed_rule_on_the_occluder_scene():
    V, F, poses, K, hw, pts, want = occluder_scene()
    got = R.observed(pts, V, F, poses, K, hw, near=0.05, far=10.0, tol=0.01)
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    assert 0.2 < want.mean() < 0.8
    # far: the wall lies 1.5 m and more away
    assert not R.observed(pts[:784], V, F, poses, K, hw, far=1.4).any()
    # a second camera behind the quad, looking back (a half turn about y), sees the shadow but not what is behind it
    back = np.array([0, 0, 1.4, 0, 1, 0, 0, 1], np.float32)
    both = R.observed(pts, V, F, np.stack([IDENT, back]), K, hw)
    assert (both >= got).all() and not both[:784][(np.abs(pts[:784, :2]) < 0.5).all(1)].any()
    assert not both[-7:-5].any()                                             # the quad hides the points at z < 0 from it
    # a scaled pose sees what the unscaled one sees
    scaled = IDENT.copy()
    scaled[7] = 3.0
    assert np.array_equal(R.observed(pts, V, F, scaled[None], K, hw), got)


def test_compose_moves_poses():
    rng = np.random.default_rng(2)
    T = np.concatenate([rng.normal(size=3), synthetic.quat_from_rotvec(rng.normal(size=3)), [1.7]])
    pose = synthetic.camera_pose(40)
    pose[7] = 0.6
    X = rng.normal(size=(5, 3))
    want = synthetic.sim3_act(T, synthetic.sim3_act(pose, X))
    assert np.abs(synthetic.sim3_act(R.compose(T, pose), X) - want).max() < 1e-12
