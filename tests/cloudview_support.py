"""What the CPU and the GPU tests of the cloud views share: the exact little camera, the trap cases with the answers worked
out by hand, and the lattice room with its plate.  A plain module like mesh_support.py; the CPU file checks the numpy
statement (cloudview_numpy.py) against the hand-computed answers, the GPU file checks the kernels against the statement
on the same cases."""
import numpy as np

from mast3r_slam import synthetic

# the exact camera: identity pose, fx = fy = 4, cx = cy = 2, an image of 4 rows and 5 columns.  A point (x, y, 1) lands
# at u = 4 x + 2, v = 4 y + 2 with no rounding, so pixel (px, py) is hit by ((px - 2) / 4, (py - 2) / 4, 1).
EYE = np.array([0, 0, 0, 0, 0, 0, 1, 1], np.float32)
K4 = np.array([[4.0, 0, 2.0], [0, 4.0, 2.0], [0, 0, 1.0]])
HW = (4, 5)


def at(px, py, z=1.0):
    """The point that lands exactly at pixel (px, py) at camera z (r is not z off the axis)."""
    return [(px - 2.0) / 4.0 * z, (py - 2.0) / 4.0 * z, z]


def f32_up(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def f32_down(x):
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


def square(px, py, rho, index=0):
    """The index image of one point of footprint rho at (px, py): `index` inside the clipped square, -1 outside."""
    h, w = HW
    out = np.full((h, w), -1, np.int32)
    out[max(py - rho, 0):min(py + rho, h - 1) + 1, max(px - rho, 0):min(px + rho, w - 1) + 1] = index
    return out


EMPTY_IMAGE = np.full(HW, -1, np.int32)
TINY = 1.0e-30

# (name, points, options of the splat, the index image worked out by hand)
SPLAT_CASES = [
    # u = 4 x + 2: -0.5 at x = -0.625 (in, pixel 0), w - 0.5 = 4.5 at x = 0.625 (out); the same for v with h - 0.5 = 3.5
    ("u at -0.5", [[-0.625, 0, 1]], dict(near=0.0), square(0, 2, 0)),
    ("u at w-0.5", [[0.625, 0, 1]], dict(near=0.0), EMPTY_IMAGE),
    ("u below w-0.5", [[f32_down(0.625), 0, 1]], dict(near=0.0), square(4, 2, 0)),
    ("u below -0.5", [[f32_down(-0.625), 0, 1]], dict(near=0.0), EMPTY_IMAGE),
    ("v at -0.5", [[0, -0.625, 1]], dict(near=0.0), square(2, 0, 0)),
    ("v at h-0.5", [[0, 0.375, 1]], dict(near=0.0), EMPTY_IMAGE),
    ("v below h-0.5", [[0, f32_down(0.375), 1]], dict(near=0.0), square(2, 3, 0)),
    ("z zero", [[0, 0, 0]], dict(near=0.0), EMPTY_IMAGE),
    ("z zero off axis", [[0.25, 0, 0]], dict(near=0.0), EMPTY_IMAGE),
    ("z negative", [[0, 0, -1]], dict(near=0.0), EMPTY_IMAGE),
    # on the axis r = z
    ("r at near", [[0, 0, 0.5]], dict(near=0.5, far=2.0), square(2, 2, 0)),
    ("r below near", [[0, 0, f32_down(0.5)]], dict(near=0.5, far=2.0), EMPTY_IMAGE),
    ("r at far", [[0, 0, 2]], dict(near=0.5, far=2.0), square(2, 2, 0)),
    ("r above far", [[0, 0, f32_up(2.0)]], dict(near=0.5, far=2.0), EMPTY_IMAGE),
    ("nan x", [[np.nan, 0, 1]], dict(near=0.0), EMPTY_IMAGE),
    ("nan z", [[0, 0, np.nan]], dict(near=0.0), EMPTY_IMAGE),
    ("inf z", [[0, 0, np.inf]], dict(near=0.0, far=np.inf), EMPTY_IMAGE),
    ("inf x", [[np.inf, 0, 1]], dict(near=0.0, far=np.inf), EMPTY_IMAGE),
    ("-inf y", [[0, -np.inf, 1]], dict(near=0.0, far=np.inf), EMPTY_IMAGE),
    # the footprint against each border and a corner
    ("clip left", [at(0, 2)], dict(radius=1), square(0, 2, 1)),
    ("clip right", [at(4, 2)], dict(radius=1), square(4, 2, 1)),
    ("clip top", [at(2, 0)], dict(radius=1), square(2, 0, 1)),
    ("clip bottom", [at(2, 3)], dict(radius=1), square(2, 3, 1)),
    ("clip corner", [at(0, 0)], dict(radius=2), square(0, 0, 2)),
    ("clip far corner", [at(4, 3)], dict(radius=8), square(4, 3, 8)),
    # rho = floor(0.5 point_size 4 / z) = floor(2 point_size / z): the steps of the floor
    ("size step at 0.5", [at(2, 2)], dict(point_size=0.5), square(2, 2, 1)),
    ("size below 0.5", [at(2, 2)], dict(point_size=float(np.nextafter(0.5, 0.0))), square(2, 2, 0)),
    ("size step at 1", [at(2, 2)], dict(point_size=1.0), square(2, 2, 2)),
    ("size below 1", [at(2, 2)], dict(point_size=float(np.nextafter(1.0, 0.0))), square(2, 2, 1)),
    ("size, z at 2", [[0, 0, 2]], dict(point_size=1.0), square(2, 2, 1)),
    ("size, z above 2", [[0, 0, f32_up(2.0)]], dict(point_size=1.0), square(2, 2, 0)),
    ("size under radius", [at(2, 2)], dict(point_size=0.25, radius=1), square(2, 2, 1)),
    ("size over max_radius", [at(2, 2)], dict(point_size=1.0, max_radius=1), square(2, 2, 1)),
    # the clamp: 2e30 / 1e-30 = 2e60, and 0.5 * 1e308 * 4 overflows to +inf: both give max_radius, taken in f64
    ("tiny z, huge size", [[0, 0, TINY]], dict(near=0.0, point_size=1.0e30), square(2, 2, 8)),
    ("tiny z, size overflow", [[0, 0, TINY]], dict(near=0.0, point_size=1.0e308, max_radius=1), square(2, 2, 1)),
    # ties.  (2^-13, 0, 1) has r = sqrt(1 + 2^-26) = 1 + 2^-27 in f64, 1.0 in f32, and lands at u = 2 + 2^-11: pixel 2.
    # It comes first, so it wins although the second point is nearer in f64.
    ("equal f32 ranges", [[2.0 ** -13, 0, 1], [0, 0, 1]], dict(), square(2, 2, 0)),
    ("nearer wins", [[0, 0, 1], [0, 0, f32_down(1.0)]], dict(), square(2, 2, 0, 1)),
    ("duplicate", [[0.25, 0, 1], [0, 0, 1], [0, 0, 1]], dict(), np.maximum(square(2, 2, 0, 1), square(3, 2, 0, 0))),
    # the order of the range bits is unsigned: a signed 64-bit minimum would keep the empty all-ones pixel (-1), and
    # f32 +inf (far = inf; r = 3.4e38 sqrt(1 + 1/16) overflows f32, v = 4 / 4 + 2 = 3) has the highest bits below empty,
    # is a hit, and loses to any finite range
    ("f32 range overflow", [[0, 8.5e37, 3.4e38]], dict(far=np.inf), square(2, 3, 0)),
    ("overflow loses", [[0, 8.5e37, 3.4e38], [0, 0.25, 1]], dict(far=np.inf), square(2, 3, 0, 1)),
]

# (name, cloud, queries, options of the splat and the test, seen worked out by hand)
VISIBLE_CASES = [
    # r64 = 1 + 2^-27 is above its own f32 rounding 1.0: with the left side rounded to f32 the point sees itself
    ("self at tol 0", [[2.0 ** -13, 0, 1]], [[2.0 ** -13, 0, 1]], dict(tol=0.0), [1]),
    ("loser of a tie at tol 0", [[2.0 ** -13, 0, 1], [0, 0, 1]], [[0, 0, 1], [2.0 ** -13, 0, 1]], dict(tol=0.0), [1, 1]),
    # <= at equality: 1.5 <= 1.0 * 1 + 0.5, and 1.5 <= 1.0 * 1.25 + 0.25, every number exact
    ("tol at equality", [[0, 0, 1]], [[0, 0, 1.5], [0, 0, f32_up(1.5)]], dict(tol=0.5), [1, 0]),
    ("rel_tol at equality", [[0, 0, 1]], [[0, 0, 1.5], [0, 0, f32_up(1.5)]], dict(tol=0.25, rel_tol=0.25), [1, 0]),
    ("behind at tol 0", [[0, 0, 1]], [[0, 0, f32_up(1.0)], [0, 0, 1], [0, 0, 0.5]], dict(tol=0.0), [0, 1, 1]),
    ("empty pixel observes", [[0, 0, 1]], [at(0, 0, 3.0), at(4, 3, 0.5)], dict(tol=0.0), [1, 1]),
    ("not in view", [[0, 0, 1]], [[0, 0, -1], [0.625, 0, 1], [np.nan, 0, 1], [0, 0, 20]], dict(tol=0.0), [0, 0, 0, 0]),
    ("footprint occludes", [[0, 0, 1]], [at(3, 2, 2.0), at(4, 2, 2.0)], dict(tol=0.0, radius=1), [0, 1]),
]


# ----------------------------------------------------------------------------------------------------------------------
# the lattice room: the six walls of synthetic.ROOM_HALF and a plate in front of the +x wall, as points and as a mesh
# ----------------------------------------------------------------------------------------------------------------------
SPACING = 0.05
PLATE_X, PLATE_LO, PLATE_HI = 2.2, (-0.5, -0.45), (0.7, 0.55)                # 1.2 m along y, 1.0 m along z


def _lattice(lo, hi, d):
    n = int(round((hi - lo) / d))
    return lo + (np.arange(n) + 0.5) * d


def lattice_room(d=SPACING):
    """(points f32[N,3], vertices f32[12,3], faces i32[14,3]): every wall and the plate sampled at the centres of the
    cells of a lattice of spacing d, and room_mesh() with the plate as two more faces."""
    H = synthetic.ROOM_HALF
    pts = []
    for axis in range(3):
        a, b = [k for k in range(3) if k != axis]
        A, B = np.meshgrid(_lattice(-H[a], H[a], d), _lattice(-H[b], H[b], d), indexing="ij")
        for side in (-1.0, 1.0):
            p = np.empty(A.shape + (3,))
            p[..., axis], p[..., a], p[..., b] = side * H[axis], A, B
            pts.append(p.reshape(-1, 3))
    Y, Z = np.meshgrid(_lattice(PLATE_LO[0], PLATE_HI[0], d), _lattice(PLATE_LO[1], PLATE_HI[1], d), indexing="ij")
    pts.append(np.stack((np.full(Y.shape, PLATE_X), Y, Z), -1).reshape(-1, 3))
    V, F = synthetic.room_mesh()
    corners = [[PLATE_X, y, z] for y, z in ((PLATE_LO[0], PLATE_LO[1]), (PLATE_HI[0], PLATE_LO[1]),
                                            (PLATE_HI[0], PLATE_HI[1]), (PLATE_LO[0], PLATE_HI[1]))]
    V = np.concatenate((V, np.array(corners, np.float32)))
    F = np.concatenate((F, np.array([[8, 9, 10], [8, 10, 11]], np.int32)))
    return np.concatenate(pts).astype(np.float32), V, F


def plate_cameras():
    """Three cameras in the room that look at the plate and the +x wall behind it."""
    out = []
    for x, yaw in ((0.0, 0.0), (0.8, 0.3), (-1.0, -0.2)):
        q = synthetic.quat_from_rotvec(np.array([0.05, np.pi / 2 + yaw, 0.0]))
        out.append(np.concatenate(([x, 0.1, 0.05], q, [1.0])))
    return np.stack(out).astype(np.float32)
