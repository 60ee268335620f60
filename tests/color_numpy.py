"""Pure-numpy statement of the colour fusion and the colour sample of the global TSDF (csrc/tsdf_color.hip, DESIGN.md
"Colour"): the sample walk of the TSDF integrate in f32 with f64 weights, the integer sums per voxel, and the trilinear
colour sample with default substitution on the lattice of the mesh and the views (tests/render_numpy.py)."""
import numpy as np

_BIAS = 1 << 20
_CORNERS = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], np.int64)
SCALE = float(1 << 20)     # weight units per unit of weight

# the room texture (synthetic.render_rgb) as a function of the world point, in [0, 1]; WAVES[c] = (axis, k, axis, k)
WAVES = ((0, 3.1, 1, 1.7), (1, 2.3, 2, 2.9), (2, 4.1, 0, 1.3))


def texture(p):
    """0.5 * (sin(...) + 1) of synthetic.render_rgb's formula at world points (...,3) -> (...,3) f64."""
    p = np.asarray(p, np.float64)
    return np.stack([0.5 * (np.sin(k0 * p[..., a0] + k1 * p[..., a1]) + 1.0) for a0, k0, a1, k1 in WAVES], -1)


def lipschitz():
    """Largest Lipschitz constant of a texture channel: 0.5 * |k|."""
    return max(0.5 * float(np.hypot(k0, k1)) for _, k0, _, k1 in WAVES)


def pack(keys):
    k = np.asarray(keys, np.int64) + _BIAS
    return (k[..., 0] << 42) | (k[..., 1] << 21) | k[..., 2]


def walk(points, conf, origin, voxel_size, trunc, step_scale=0.5):
    """The in-band samples of TSDFVolume.integrate (tsdf_emit_kernel): -> (point index i64[m], key i64[m,3], w f64[m]).
    f32 ray length (products summed in f64, rounded once), num = int(maxd / step), linspace distances with the exact end
    point, band |sdf| <= trunc, w = conf * exp(-|sdf| / trunc) in f64, key = floor(f32 sample / f32 voxel size)."""
    f32 = np.float32
    pts = np.asarray(points, f32).reshape(-1, 3)
    conf = np.asarray(conf, np.float64).reshape(-1)
    org = np.asarray(origin, f32).reshape(3)
    vs, tr = f32(voxel_size), f32(trunc)
    step = f32(max(float(voxel_size) * float(step_scale), 1.0e-4))
    idx, keys, ws = [], [], []
    for i in range(len(pts)):
        r = pts[i] - org
        sq = f32((np.float64(r[0] * r[0]) + np.float64(r[1] * r[1])) + np.float64(r[2] * r[2]))
        L = f32(np.sqrt(sq))
        if not np.isfinite(L) or L < f32(1.0e-4):
            continue
        d = r / L
        maxd = f32(L + tr)
        if not f32(maxd / step) < f32(1048576.0):
            continue
        num = max(int(f32(maxd / step)), 1)
        if num > 1:
            lstep = f32(maxd / f32(num - 1))
            dist = (np.arange(num).astype(f32) * lstep).astype(f32)
            dist[-1] = maxd
        else:
            dist = np.zeros(1, f32)
        sdf = (L - dist).astype(f32)
        band = np.abs(sdf) <= tr
        dist, sdf = dist[band], sdf[band]
        e = (-np.abs(sdf) / tr).astype(f32)
        w = conf[i] * np.exp(e.astype(np.float64))
        s = (org[None] + (dist[:, None] * d[None]).astype(f32)).astype(f32)
        k = np.floor((s / vs).astype(f32)).astype(np.int64)
        ok = w > 0.0
        idx.append(np.full(int(ok.sum()), i, np.int64)), keys.append(k[ok]), ws.append(w[ok])
    if not idx:
        return np.zeros(0, np.int64), np.zeros((0, 3), np.int64), np.zeros(0)
    return np.concatenate(idx), np.concatenate(keys), np.concatenate(ws)


def fuse(sums, points, conf, rgb, origin, voxel_size, trunc, step_scale=0.5):
    """Adds one integrate call to `sums`, a dict packed key -> [sum_w, sum_wr, sum_wg, sum_wb] of python ints:
    wq = rint(w * 2^20), c8 = rint(255 * clamp(c, 0, 1)) in f32."""
    idx, keys, w = walk(points, conf, origin, voxel_size, trunc, step_scale)
    c = np.clip(np.asarray(rgb, np.float32).reshape(-1, 3), np.float32(0), np.float32(1))
    c8 = np.rint(np.float32(255.0) * c).astype(np.int64)
    wq = np.rint(np.minimum(w * SCALE, 2.0 ** 53)).astype(np.int64)
    pk = pack(keys)
    for j in range(len(pk)):
        if wq[j] == 0:
            continue
        s = sums.setdefault(int(pk[j]), [0, 0, 0, 0])
        q = int(wq[j])
        s[0] += q
        for a in range(3):
            s[1 + a] += q * int(c8[idx[j], a])
    return sums


def sums_for(sums, keys):
    """u64[n,4] of the dict `sums` at keys i64[n,3] (zeros where absent)."""
    out = np.zeros((len(keys), 4), np.uint64)
    for j, k in enumerate(pack(keys)):
        s = sums.get(int(k))
        if s is not None:
            out[j] = s
    return out


def _lerp(a, b, f):
    return a + f * (b - a)


def sample(keys, sums, voxel_size, points, default_rgb=(0.5, 0.5, 0.5)):
    """Trilinear colour at world points f32[n,3] -> (rgb f64[n,3], count i64[n]).  keys i64[m,3], sums u64[m,4]: the
    voxels' colour sums; c(k) = sum_wc / (255 * sum_w) in f64 where sum_w > 0, `default_rgb` elsewhere.  Lattice:
    g = p / vs - 0.5, base = floor(g), corner c = dx + 2 dy + 4 dz, a + f (b - a) along x, y, z."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    sums = np.asarray(sums, np.uint64).reshape(-1, 4)
    has = sums[:, 0] > 0
    pk = pack(keys[has])
    o = np.argsort(pk, kind="stable")
    pk = pk[o]
    sw = sums[has][o]
    col = sw[:, 1:].astype(np.float64) / (255.0 * sw[:, :1].astype(np.float64)) if len(sw) else np.zeros((0, 3))
    dflt = np.asarray(default_rgb, np.float64)
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        g = p / float(voxel_size) - 0.5
        b = np.floor(g)
        f = g - b
        ok = (np.abs(b) < float(_BIAS)).all(1)
    base = np.where(ok[:, None], b, 0.0).astype(np.int64)
    v = np.empty((len(p), 8, 3))
    count = np.zeros(len(p), np.int64)
    for c in range(8):
        k = base + _CORNERS[c]
        inside = ok & (np.abs(k + 0.5) < _BIAS).all(1)
        found = np.zeros(len(p), bool)
        pos = np.zeros(len(p), np.int64)
        if len(pk):
            q = pack(np.where(inside[:, None], k, 0))
            pos = np.minimum(np.searchsorted(pk, q), len(pk) - 1)
            found = inside & (pk[pos] == q)
        v[:, c] = np.where(found[:, None], col[pos] if len(pk) else dflt[None], dflt[None])
        count += found
    fx, fy, fz = (np.where(ok, f[:, a], 0.0)[:, None] for a in range(3))
    c00, c10 = _lerp(v[:, 0], v[:, 1], fx), _lerp(v[:, 2], v[:, 3], fx)
    c01, c11 = _lerp(v[:, 4], v[:, 5], fx), _lerp(v[:, 6], v[:, 7], fx)
    out = _lerp(_lerp(c00, c10, fy), _lerp(c01, c11, fy), fz)
    return np.where(ok[:, None], out, dflt[None]), count


def hit_points(pose, rays, rng):
    """World points f32 of a view's range image: o + (double)range * s * d, d = render_numpy.ray_dirs, rounded once."""
    import render_numpy as R

    pose64 = np.asarray(pose, np.float32).astype(np.float64)
    rays = np.asarray(rays, np.float32)
    d = R.ray_dirs(pose, rays).reshape(rays.shape)
    return (pose64[:3] + (np.asarray(rng, np.float32).astype(np.float64) * pose64[7])[..., None] * d).astype(np.float32)
