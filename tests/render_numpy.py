"""Pure-numpy ray cast of a sparse voxel set: the test-side statement of TSDFVolume.render (csrc/tsdf_render.hip,
DESIGN.md "View rendering").  Brute force: every sample of every ray, no empty-space skipping.  Same lattice, validity
and sign rules as the mesh (tests/mc_numpy.py), same f64 formulae in the same order as the kernel, so the device result
must match it to within f32 rounding of identical f64 values."""
import numpy as np

_BIAS = 1 << 20
_CORNERS = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], np.int64)


def pack(keys):
    k = np.asarray(keys, np.int64) + _BIAS
    return (k[..., 0] << 42) | (k[..., 1] << 21) | k[..., 2]


def ray_dirs(pose, rays):
    """World directions f64[n,3] of unit camera-frame rays f32[n,3] under pose (8,) f32 [t, q(xyzw), s]: the quaternion
    rotation r + w u + q x u, u = 2 q x r, in f64 on the f32 inputs (no renormalisation)."""
    q = np.asarray(pose, np.float32).astype(np.float64)[3:7]
    r = np.asarray(rays, np.float32).astype(np.float64).reshape(-1, 3)
    u0 = 2.0 * (q[1] * r[:, 2] - q[2] * r[:, 1])
    u1 = 2.0 * (q[2] * r[:, 0] - q[0] * r[:, 2])
    u2 = 2.0 * (q[0] * r[:, 1] - q[1] * r[:, 0])
    d0 = (r[:, 0] + q[3] * u0) + (q[1] * u2 - q[2] * u1)
    d1 = (r[:, 1] + q[3] * u1) + (q[2] * u0 - q[0] * u2)
    d2 = (r[:, 2] + q[3] * u2) + (q[0] * u1 - q[1] * u0)
    return np.stack((d0, d1, d2), 1)


def _lerp(a, b, f):
    return a + f * (b - a)


class Sampler:
    """Trilinear samples of the valid voxels (weight >= min_weight) of a voxel set."""

    def __init__(self, keys, tsdf, weight, voxel_size, min_weight):
        keys = np.asarray(keys, np.int64).reshape(-1, 3)
        ok = np.asarray(weight, np.float64).reshape(-1) >= min_weight
        pk = pack(keys[ok])
        o = np.argsort(pk, kind="stable")
        self.pk, self.val = pk[o], np.asarray(tsdf, np.float64).reshape(-1)[ok][o]
        self.vs = float(voxel_size)

    def _find(self, k):
        n = len(self.pk)
        inside = (np.abs(k + 0.5) < _BIAS).all(-1)
        if n == 0:
            return np.full(k.shape[:-1], -1, np.int64)
        q = pack(np.where(inside[..., None], k, 0))
        p = np.minimum(np.searchsorted(self.pk, q), n - 1)
        return np.where((self.pk[p] == q) & inside, p, -1)

    def __call__(self, p):
        """p f64[m,3] -> (valid bool[m], value f64[m], gradient f64[m,3]); value / gradient are 0 where invalid."""
        vs = self.vs
        g = p / vs - 0.5
        b = np.floor(g)
        f = g - b
        finite = (np.abs(b) < float(_BIAS)).all(1)
        base = np.where(finite[:, None], b, 0.0).astype(np.int64)
        idx = np.stack([self._find(base + _CORNERS[c]) for c in range(8)], 1)
        valid = finite & (idx >= 0).all(1)
        v = np.where(valid[:, None], self.val[np.maximum(idx, 0)] if len(self.val) else 0.0, 0.0)
        fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
        c00, c10 = _lerp(v[:, 0], v[:, 1], fx), _lerp(v[:, 2], v[:, 3], fx)
        c01, c11 = _lerp(v[:, 4], v[:, 5], fx), _lerp(v[:, 6], v[:, 7], fx)
        c0, c1 = _lerp(c00, c10, fy), _lerp(c01, c11, fy)
        val = _lerp(c0, c1, fz)
        gx = _lerp(_lerp(v[:, 1] - v[:, 0], v[:, 3] - v[:, 2], fy), _lerp(v[:, 5] - v[:, 4], v[:, 7] - v[:, 6], fy), fz) / vs
        gy = _lerp(c10 - c00, c11 - c01, fz) / vs
        gz = (c1 - c0) / vs
        grad = np.stack((gx, gy, gz), 1)
        return valid, np.where(valid, val, 0.0), np.where(valid[:, None], grad, 0.0)


def render(keys, tsdf, weight, voxel_size, min_weight, pose, rays, near=0.05, far=10.0, level=0.0, step=None,
           dtype=np.float32):
    """rays f32[h,w,3] (or [n,3]) unit, camera frame; pose (8,) f32.  -> (range[...], normal[...,3], hit bool[...]) with
    the shape of rays; range and normal in `dtype` (f32 as the device returns them, f64 to look at the march itself)."""
    rays = np.asarray(rays, np.float32)
    shape = rays.shape[:-1]
    pose = np.asarray(pose, np.float32).astype(np.float64)
    d = ray_dirs(pose, rays)
    o, s = pose[:3], pose[7]
    n = len(d)
    vs, lv, near, far = float(voxel_size), float(level), float(near), float(far)
    step = 0.5 * vs if step is None else float(step)
    S = Sampler(keys, tsdf, weight, vs, min_weight)
    rng = np.zeros(n, dtype)
    nrm = np.zeros((n, 3), dtype)
    hit = np.zeros(n, bool)
    live = np.arange(n)
    pv = np.zeros(n, bool)
    pf = np.zeros(n)
    pg = np.zeros((n, 3))
    k = 0
    while len(live):
        tk = near + k * step
        if not tk <= far:
            break
        dl = d[live]
        valid, f, g = S(o[None] + tk * dl)
        if k >= 1:
            h = pv[live] & valid & (pf[live] >= lv) & (f < lv)
            if h.any():
                i = live[h]
                fr = (pf[i] - lv) / (pf[i] - f[h])
                ts = (near + (k - 1) * step) + step * fr
                gi = pg[i] + fr[:, None] * (g[h] - pg[i])
                ln = np.sqrt((gi[:, 0] * gi[:, 0] + gi[:, 1] * gi[:, 1]) + gi[:, 2] * gi[:, 2])
                with np.errstate(invalid="ignore", divide="ignore"):
                    nrm[i] = np.where(ln[:, None] > 0.0, gi / ln[:, None], 0.0).astype(dtype)
                rng[i] = (ts / s).astype(dtype)
                hit[i] = True
        pv[live], pf[live], pg[live] = valid, f, g
        live = live[~hit[live]]
        k += 1
    return rng.reshape(shape), nrm.reshape(shape + (3,)), hit.reshape(shape)


def unit_rays(h, w, K):
    """Pinhole rays f32[h,w,3] of unit length (synthetic.pixel_rays, normalised)."""
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64), indexing="xy")
    r = np.stack(((u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)), -1)
    return (r / np.linalg.norm(r, axis=-1, keepdims=True)).astype(np.float32)


def sample_sdf(sdf, lo, hi, voxel_size, band):
    """Voxels (keys i64[n,3], tsdf f64[n], weight f64[n] = 1) with |sdf(centre)| <= band inside the box [lo, hi]."""
    vs = float(voxel_size)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ax = [np.arange(int(np.floor(lo[a] / vs)) - 1, int(np.ceil(hi[a] / vs)) + 2) for a in range(3)]
    k = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    v = sdf((k.astype(np.float64) + 0.5) * vs)
    m = np.abs(v) <= band
    return k[m], v[m], np.ones(int(m.sum()))
