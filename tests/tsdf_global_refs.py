"""Plain references and edge-case inputs for csrc/tsdf_global.hip (tests/test_tsdf_global_edges_gpu.py); every recipe and
every condition the GPU tests rely on is checked without a GPU in tests/test_tsdf_global_refs_cpu.py.

Two references:
  * LiteralVolume / literal_pose_system: the reference's integrate / _update_voxel / query / _estimate_gradient and the
    optimizer's _build_linear_system / _accumulate_system / _sim3_jacobian / solve, restated step by step on a Python dict
    with NumPy scalars of the dtypes the reference sees (points and origin float32, confidences float64).  np.linalg.norm,
    np.linspace, np.floor(..).astype(int) and np.clip are the real ones, so NumPy's promotion and rounding are the ground
    truth here and nobody's reading of them.  One Python iteration per ray sample: CPU test only.
  * oracle.TSDFVolume (C): what the GPU tests compare with; the CPU test pins it to the literal reference, bit for bit, on
    every entry of CASES.

sample_counts() is the per-ray vectorised form of the same arithmetic (array operations are the scalar operations element
by element), used to prove that an input really reaches a branch: 48 / 49 / 2048 / 2049 samples in one voxel, probe
wrap-around, num == 1 / 2."""
import math

import numpy as np

KEY_BIAS = 1 << 20
MASK64 = (1 << 64) - 1


# ======================================================================================================================
# host copies of the device hash (csrc/tsdf_table.h)
# ======================================================================================================================
def mix64(k):
    k &= MASK64
    k ^= k >> 33; k = (k * 0xff51afd7ed558ccd) & MASK64
    k ^= k >> 33; k = (k * 0xc4ceb9fe1a85ec53) & MASK64
    k ^= k >> 33
    return k


def pack_key(x, y, z):
    """The 3 x 21 bit biased key, or None when an index is outside [-2^20, 2^20)."""
    b = (int(x) + KEY_BIAS, int(y) + KEY_BIAS, int(z) + KEY_BIAS)
    if any(not 0 <= c < 2 * KEY_BIAS for c in b):
        return None
    return (b[0] << 42) | (b[1] << 21) | b[2]


def home_slot(key3, capacity):
    return mix64(pack_key(*key3)) & (capacity - 1)


def in_key_range(keys):
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    return ((keys >= -KEY_BIAS) & (keys < KEY_BIAS)).all(axis=1)


# ======================================================================================================================
# the literal reference
# ======================================================================================================================
class LiteralVolume:
    """voxels: dict (ix, iy, iz) -> [tsdf, weight]; tsdf keeps the NumPy scalar type it was given (np.float32 after the
    first touch, np.float64 once averaged), which is what the gradient's float32 path depends on."""

    def __init__(self, voxel_size, truncation, max_weight=100.0, min_weight=1.0e-3):
        self.voxel_size = float(voxel_size)
        self.truncation = float(truncation)
        self.max_weight = float(max_weight)
        self.min_weight = float(min_weight)
        self.voxels = {}
        self.nums = []          # num_samples of every fused ray of the last integrate
        self.counts = {}        # samples applied per voxel by the last integrate

    def index(self, p):
        with np.errstate(invalid="ignore", over="ignore"):      # NaN / inf -> INT64_MIN, as in the reference
            return tuple(np.floor(p / self.voxel_size).astype(int).tolist())

    def integrate(self, points, conf, origin, step_scale=0.5):
        points = np.asarray(points, np.float32).reshape(-1, 3)
        conf = np.asarray(conf, np.float64).reshape(-1)
        origin = np.asarray(origin, np.float32).reshape(3)
        self.nums, self.counts = [], {}
        if points.size == 0:
            return 0
        step = max(self.voxel_size * step_scale, 1.0e-4)
        trunc = self.truncation
        fused = 0
        for point, c in zip(points, conf):
            ray = point - origin
            length = np.linalg.norm(ray)
            if not np.isfinite(length) or length < 1.0e-4:
                continue
            direction = ray / length
            reach = length + trunc
            num = max(1, int(reach / step))
            self.nums.append(num)
            for dist in np.linspace(0.0, reach, num):
                sample = origin + dist * direction
                sdf = length - dist
                if abs(sdf) > trunc:
                    continue
                value = np.clip(sdf / trunc, -1.0, 1.0)
                weight = c * math.exp(-abs(sdf) / trunc)
                self.update(sample, value, weight)
            fused += 1
        return fused

    def update(self, sample, value, weight):
        if weight <= 0.0:
            return
        key = self.index(sample)
        self.counts[key] = self.counts.get(key, 0) + 1
        cell = self.voxels.get(key)
        if cell is None:
            self.voxels[key] = [value, weight]
            return
        total = min(cell[1] + weight, self.max_weight)
        with np.errstate(invalid="ignore"):     # inf and NaN weights: silent here as in the reference's own run
            cell[0] = (cell[0] * cell[1] + value * weight) / max(1.0e-9, total)
        cell[1] = total

    def dump(self):
        """(keys i64[n,3], tsdf f64[n], weight f64[n]) in lexicographic key order, like oracle.TSDFVolume.voxels()."""
        if not self.voxels:
            return np.zeros((0, 3), np.int64), np.zeros(0), np.zeros(0)
        keys = np.array(sorted(self.voxels), np.int64).reshape(-1, 3)
        t = np.array([float(self.voxels[tuple(k)][0]) for k in keys.tolist()])
        w = np.array([float(self.voxels[tuple(k)][1]) for k in keys.tolist()])
        return keys, t, w

    def load(self, keys, tsdf, weight, first_touch):
        """Voxels as arrays; first_touch[i]: the value is still the float32 sample (it is exact in float32 then)."""
        for k, t, w, f in zip(np.asarray(keys).tolist(), tsdf, weight, first_touch):
            self.voxels[tuple(k)] = [np.float32(t) if f else np.float64(t), np.float64(w)]

    # ------------------------------------------------------------------
    def query(self, p):
        p = np.asarray(p, np.float32)
        cell = self.voxels.get(self.index(p))
        if cell is None or cell[1] < self.min_weight:
            return None, None
        return cell[0], self.gradient(p)

    def gradient(self, p):
        base = self.index(p)
        step = np.eye(3, dtype=int)
        grad = np.zeros(3, dtype=np.float64)
        pairs = 0.0
        for axis in range(3):
            hi = self.voxels.get(tuple(base[i] + step[axis, i] for i in range(3)))
            lo = self.voxels.get(tuple(base[i] - step[axis, i] for i in range(3)))
            if hi is None or lo is None:
                continue
            if hi[1] < self.min_weight or lo[1] < self.min_weight:
                continue
            grad[axis] = (hi[0] - lo[0]) / (2.0 * self.voxel_size)
            pairs += 1.0
        if pairs == 0.0:
            return None
        norm = np.linalg.norm(grad)
        if norm < 1.0e-9:
            return None
        return grad / norm

    def query_batch(self, points):
        """(value f64[n], grad f64[n,3], status u8[n]): 0 = (None, None), 1 = (value, None), 2 = (value, gradient)."""
        points = np.asarray(points, np.float32).reshape(-1, 3)
        n = len(points)
        val, grad, st = np.zeros(n), np.zeros((n, 3)), np.zeros(n, np.uint8)
        for i, p in enumerate(points):
            v, g = self.query(p)
            if v is None:
                continue
            val[i], st[i] = v, 1
            if g is not None:
                grad[i], st[i] = g, 2
        return val, grad, st


def literal_pose_system(vol, points_world, conf, lam):
    """(H f64[7,7], b f64[7], used): the optimizer's linear system for float32 world points and float32 confidences.
    `used` counts the residuals that were accumulated (the reference tests len(residuals) before its finiteness filter;
    the two differ only for non-finite values, which no input here produces)."""
    points_world = np.asarray(points_world, np.float32).reshape(-1, 3)
    conf = np.asarray(conf, np.float32).reshape(-1)
    residuals, jacobians, weights = [], [], []
    for p, c in zip(points_world, conf):
        value, grad = vol.query(p)
        if value is None or grad is None:
            continue
        J = np.zeros(7, dtype=np.float64)
        J[:3] = grad
        J[3:6] = -np.cross(p, grad)
        J[6] = float(np.dot(p, grad))
        residuals.append(value)
        jacobians.append(J)
        weights.append(lam * c)
    H = np.zeros((7, 7), dtype=np.float64)
    b = np.zeros(7, dtype=np.float64)
    used = 0
    for r, J, w in zip(residuals, jacobians, weights):
        if not np.isfinite(r) or not np.all(np.isfinite(J)):
            continue
        root = math.sqrt(max(w, 1.0e-6))
        Jw = root * J
        H += np.outer(Jw, Jw)
        b += Jw * r * root
        used += 1
    return H, b, used


GATE = np.float32(1.0e-6)      # 9.99999997e-7: not the double 1e-6, which is what makes the gate visible


def gate_confidences(lam, where, n):
    """n float32 confidences whose float32 product with lambda is, for EVERY one of them, `where` the 1e-6 gate:
    "at" (the product is float32(1e-6) itself), "below" or "above" (the nearest products on that side).  Neighbouring
    confidences move the product by less than one of its ulps, so the gate itself is hit.  No other row is mixed in:
    a single ordinary confidence would outweigh the gate rows 1e5 times and hide them.
    max(w, 1.0e-6) keeps the float32 product from the gate upwards (sqrt of 9.99999997e-7 at it) and takes the double
    constant below it: relative to the double constant that is 2.5e-9 in every entry of H, which the systems built from
    these confidences are sized to show at the bars (H, b grow with n, the absolute bar does not)."""
    lamf = np.float32(lam)
    c = np.float32(GATE / lamf)
    run = [c]
    for _ in range(40):
        run = [np.nextafter(run[0], np.float32(0.0))] + run + [np.nextafter(run[-1], np.float32(1.0))]
    run = np.array(run, np.float32)
    prod = lamf * run
    pick = {"at": run[prod == GATE], "below": run[prod < GATE][-3:], "above": run[prod > GATE][:3]}[where]
    assert len(pick) > 0
    return np.resize(pick, n).astype(np.float32)


def literal_step(H, b, damping):
    """delta of one update, solved in float64 and rounded to float32 as the reference hands it to Sim3.exp."""
    return np.linalg.solve(H + damping * np.eye(7), -b).astype(np.float32)


# ======================================================================================================================
# per-ray vectorised form: which voxels a ray's samples fall in
# ======================================================================================================================
def ray_samples(point, origin, voxel_size, trunc, step_scale):
    """(num, keys i64[m,3], e f32[m]) of one ray: its num_samples, the voxel of every in-band sample and the exponent of
    its weight (weight = conf * exp(e)); None for a ray the reference skips."""
    point = np.asarray(point, np.float32)
    origin = np.asarray(origin, np.float32)
    step = max(voxel_size * step_scale, 1.0e-4)
    ray = point - origin
    length = np.linalg.norm(ray)
    if not np.isfinite(length) or length < 1.0e-4:
        return None
    direction = ray / length
    reach = length + trunc
    num = max(1, int(reach / step))
    dist = np.linspace(0.0, reach, num)
    sdf = length - dist
    band = ~(np.abs(sdf) > trunc)
    samples = origin[None, :] + dist[band, None] * direction[None, :]
    keys = np.floor(samples / voxel_size).astype(int)
    return num, keys.astype(np.int64), -np.abs(sdf[band]) / trunc


def sample_counts(points, conf, origin, voxel_size, trunc, max_weight=100.0, step_scale=0.5):
    """(counts dict key -> samples one integrate call applies to that voxel, nums list of num_samples per fused ray)."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    conf = np.asarray(conf, np.float64).reshape(-1)
    cache, counts, nums = {}, {}, []
    for p, c in zip(points, conf):
        tag = p.tobytes()
        if tag not in cache:
            cache[tag] = ray_samples(p, origin, voxel_size, trunc, step_scale)
        rs = cache[tag]
        if rs is None:
            continue
        num, keys, e = rs
        nums.append(num)
        w = c * np.exp(e.astype(np.float64))
        for k in keys[~(w <= 0.0)].tolist():
            k = tuple(k)
            counts[k] = counts.get(k, 0) + 1
    return counts, nums


def rays_through(targets, origin, voxel_size, trunc, step_scale, seed, tries=4000, reach=(0.2, 1.5)):
    """Rays (points f32[m,3]) from `origin` that apply at least one sample to every voxel of `targets`: seeded random
    end points around each target's centre until one ray's samples include it."""
    rng = np.random.default_rng(seed)
    origin = np.asarray(origin, np.float32)
    out = []
    for t in targets:
        centre = (np.asarray(t, np.float64) + 0.5) * voxel_size
        for _ in range(tries):
            p = (centre + rng.uniform(-0.5, 0.5, 3) * voxel_size).astype(np.float32)
            rs = ray_samples(p, origin, voxel_size, trunc, step_scale)
            if rs is not None and (rs[1] == np.asarray(t)).all(axis=1).any():
                out.append(p)
                break
        else:
            raise RuntimeError(f"no ray from {origin} reaches voxel {t}")
    return np.array(out, np.float32).reshape(-1, 3)


# ======================================================================================================================
# CASES: name -> builder() -> (points f32[n,3], conf f64[n], origin f32[3], voxel_size, trunc, max_weight, step_scale)
# ======================================================================================================================
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)


def _directions(rng, n):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:len(AXES) * (n // 40 + 1)] = np.tile(AXES, (n // 40 + 1, 1))     # axis rays: samples on voxel faces
    return d


def band_sweep(origin, voxel_size, trunc, step_scale, n, lo, hi, seed):
    """n rays from `origin`, lengths geometric in [lo, hi], random directions plus the six axis directions."""
    rng = np.random.default_rng(seed)
    origin = np.asarray(origin, np.float32)
    length = np.geomspace(lo, hi, n)[rng.permutation(n)]
    points = (origin.astype(np.float64) + length[:, None] * _directions(rng, n)).astype(np.float32)
    return points, rng.uniform(0.1, 8.0, n), origin, voxel_size, trunc, 100.0, step_scale


REPLAY_REPEATS = (47, 48, 49, 2048, 2049)
REPLAY_DIRS = np.array([[0.83, 0.41, 0.37], [-0.29, 0.91, 0.31], [0.23, -0.37, 0.90], [-0.79, -0.53, -0.31],
                        [0.35, 0.27, -0.89]], np.float64)


def replay_thresholds(conf_scale=1.0):
    """Five rays in disjoint directions repeated 47 / 48 / 49 / 2048 / 2049 times and shuffled.  The step is two voxels
    (step_scale 2) and every direction's largest component is above 0.8, so two samples of a ray never share a voxel:
    each voxel holds exactly its ray's repeat count in one call.  Varied confidences against max_weight = 5: the clamp is
    reached within the first few samples.
    What the order of the replay changes: the running update keeps tsdf * weight equal to the sum of value * w (before
    and after the clamp alike), so with ordinary weights the end value is sum(value * w) / min(sum(w), max_weight) in any
    order and only its rounding differs - far below the bars.  `conf_scale` = 1e-13 is the case in which the order is
    visible: the summed weight stays under the 1e-9 floor of the divisor, every update is
    tsdf <- (tsdf * weight + value * w) / 1e-9, a recursion that forgets, and the end value is set by the last samples."""
    rng = np.random.default_rng(48)
    ends = (REPLAY_DIRS / np.linalg.norm(REPLAY_DIRS, axis=1, keepdims=True)).astype(np.float32)
    points = np.concatenate([np.repeat(e[None], r, axis=0) for e, r in zip(ends, REPLAY_REPEATS)])
    points = points[rng.permutation(len(points))]
    return points, conf_scale * rng.uniform(0.5, 3.0, len(points)), np.zeros(3, np.float32), 0.03, 0.12, 5.0, 2.0


MANY_BIG_RAYS, MANY_BIG_REPEATS = 270, 49


def many_big():
    """270 rays spread over a sphere of 0.5 m, each repeated 49 times: every voxel they touch holds more than kSortMax
    samples, and there are more of them than the wave kernel has blocks (2048)."""
    rng = np.random.default_rng(2048)
    i = np.arange(MANY_BIG_RAYS) + 0.5
    phi, z = i * math.pi * (3.0 - math.sqrt(5.0)), 1.0 - 2.0 * i / MANY_BIG_RAYS
    r = np.sqrt(1.0 - z * z)
    ends = (0.5 * np.stack((r * np.cos(phi), r * np.sin(phi), z), -1)).astype(np.float32)
    points = np.repeat(ends, MANY_BIG_REPEATS, axis=0)[rng.permutation(MANY_BIG_RAYS * MANY_BIG_REPEATS)]
    return points, rng.uniform(0.5, 3.0, len(points)), np.zeros(3, np.float32), 0.03, 0.12, 100.0, 0.5


def key_edges():
    """voxel_size 1, origin five metres from the points: the rays end (point + trunc) at x = 2^20 - 0.5, so voxel index
    2^20 - 1 is the last one stored and no sample lies beyond it."""
    E = float(KEY_BIAS)
    pts = np.array([[E - 2.0, 0.25, -0.75], [E - 2.0, 1.75, -0.75]], np.float32)
    org = np.array([E - 7.0, 0.25, -0.75], np.float32)
    return pts, np.array([1.0, 2.5]), org, 1.0, 1.5, 100.0, 0.5


def key_edges_low():
    """The mirror image: the rays end at x = -2^20 exactly, the lowest index there is."""
    E = float(KEY_BIAS)
    pts = np.array([[-(E - 1.5), 0.25, -0.75], [-(E - 1.5), -1.25, 0.5]], np.float32)
    org = np.array([-(E - 6.0), 0.25, -0.75], np.float32)
    return pts, np.array([1.5, 0.75]), org, 1.0, 1.5, 100.0, 0.5


def conf_edges():
    """Confidences 0, negative, +-inf and NaN on ordinary rays; points with NaN / +-inf coordinates among them."""
    rng = np.random.default_rng(5)
    n = 240
    points = (rng.normal(size=(n, 3)) * 0.4 + np.array([0.0, 0.0, 1.0])).astype(np.float32)
    conf = rng.uniform(0.2, 4.0, n)
    conf[0::12] = 0.0
    conf[1::12] = -1.5
    conf[2::24] = np.inf
    conf[3::24] = -np.inf
    conf[4::24] = np.nan
    points[5::40, 0] = np.nan
    points[6::40, 1] = np.inf
    points[7::40, 2] = -np.inf
    points[8::40] = np.nan
    return points, conf, np.array([0.05, -0.02, 0.01], np.float32), 0.03, 0.12, 100.0, 0.5


def nan_origin():
    p, c, o, vs, tr, mw, ss = conf_edges()
    return p, c, np.array([0.0, np.nan, 0.0], np.float32), vs, tr, mw, ss


WRAP_CAPACITY = 1024


def wrap_table(capacity=WRAP_CAPACITY, seed=1023):
    """Single rays chosen so that, on a table of 1024 slots, slots 1023 and 0 are both home slots and more than four
    keys have their home in the last four slots: whatever the insertion order, a probe runs over the table's end."""
    rng = np.random.default_rng(seed)
    vs, tr, ss = 0.03, 0.06, 0.5
    origin = np.array([0.02, -0.01, 0.015], np.float32)
    cand = (rng.normal(size=(4000, 3)) * 0.6).astype(np.float32)
    last, tail, zero, fill = [], [], [], []
    for p in cand:
        rs = ray_samples(p, origin, vs, tr, ss)
        if rs is None:
            continue
        homes = {home_slot(k, capacity) for k in map(tuple, rs[1].tolist())}
        if capacity - 1 in homes and len(last) < 2:
            last.append(p)
        elif homes & {capacity - 4, capacity - 3, capacity - 2} and len(tail) < 6:
            tail.append(p)
        elif 0 in homes and len(zero) < 2:
            zero.append(p)
        elif len(fill) < 30:
            fill.append(p)
    points = np.array(last + tail + zero + fill, np.float32)
    points = points[rng.permutation(len(points))]
    return points, rng.uniform(0.5, 3.0, len(points)), origin, vs, tr, 100.0, ss


_NEG = (-1.3, 0.77, -2.1)
_CORNER = (0.12, -0.06, 0.03)      # float32(c) / float32(0.03) is exactly 4, -2, 1 (0.09 would give 3.0000002)

CASES = {
    # band sweep: three origins at the default setting (lengths from below the 1e-4 gate to 30 m) ...
    "band_origin0": lambda: band_sweep((0, 0, 0), 0.03, 0.12, 0.5, 700, 5e-5, 30.0, 1),
    "band_negative": lambda: band_sweep(_NEG, 0.03, 0.12, 0.5, 700, 5e-5, 30.0, 2),
    "band_corner": lambda: band_sweep(_CORNER, 0.03, 0.12, 0.5, 700, 5e-5, 30.0, 3),
    # ... a step so coarse that rays have one or two samples, the step clamp on short rays (camera inside the band,
    # max_band = 404), and a band thinner than a voxel
    "band_coarse": lambda: band_sweep(_NEG, 0.03, 0.12, 10.0, 400, 5e-5, 2.0, 4),
    "band_clamped": lambda: band_sweep(_CORNER, 0.01, 0.02, 1.0e-3, 120, 5e-5, 0.019, 5),
    "band_thin": lambda: band_sweep((0, 0, 0), 0.05, 0.02, 0.5, 500, 5e-5, 30.0, 6),
    "replay_thresholds": replay_thresholds,
    "replay_floor": lambda: replay_thresholds(1.0e-13),
    "many_big": many_big,
    "key_edges": key_edges,
    "key_edges_low": key_edges_low,
    "conf_edges": conf_edges,
    "nan_origin": nan_origin,
    "wrap_table": wrap_table,
}


def key_overflow_code1():
    """key_edges plus one ray whose last samples fall in voxel index 2^20: those samples are dropped and reported."""
    p, c, o, vs, tr, mw, ss = key_edges()
    bad = np.array([[float(KEY_BIAS) - 1.0, 0.25, 1.25]], np.float32)
    return np.concatenate((p, bad)), np.concatenate((c, [1.25])), o, vs, tr, mw, ss


def long_ray_code3():
    """band_origin0's first rays plus one point 20 km away: at the default 1.5 cm step its ray has more than 2^20
    samples; the point is dropped and reported, the others are fused."""
    p, c, o, vs, tr, mw, ss = band_sweep((0, 0, 0), 0.03, 0.12, 0.5, 200, 1e-3, 3.0, 7)
    far = np.array([[12000.0, -16000.0, 300.0]], np.float32)
    at = 77
    return (np.concatenate((p[:at], far, p[at:])), np.concatenate((c[:at], [2.0], c[at:])), o, vs, tr, mw, ss), at


# ======================================================================================================================
# volumes for the query and pose tests
# ======================================================================================================================
def sparse_rays(seed, n=220, repeats=40):
    """Single rays (voxels touched once keep their float32 value) plus a few repeated ones (averaged voxels), in a box of
    about 0.4 m so that neighbours of every kind occur: (points, conf, origin, vs, trunc, max_weight) and the step scales
    of the two calls (1.0: about one sample per voxel, 0.5: about two)."""
    rng = np.random.default_rng(seed)
    origin = np.array([0.013, -0.021, 0.017], np.float32)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:12] = np.tile(AXES, (2, 1))
    points = (origin + d * rng.uniform(0.1, 0.22, (n, 1))).astype(np.float32)
    points = np.concatenate((points, points[rng.integers(0, n, repeats)]))
    return points, rng.uniform(0.5, 3.0, len(points)), origin, 0.03, 0.06, 100.0


def centres(keys, voxel_size):
    return ((np.asarray(keys, np.float64) + 0.5) * voxel_size).astype(np.float32)


def classify_queries(keys, weight, touched_once, min_weight, query_keys):
    """For every query voxel: (valid axis pairs, set of pair state kinds among 'ff' first/first, 'fa' mixed, 'aa'
    averaged/averaged), from the dumped voxels - how the tests prove that every gate was reached."""
    table = {tuple(k): (w, f) for k, w, f in zip(np.asarray(keys).tolist(), weight, touched_once)}
    out = []
    for q in np.asarray(query_keys).tolist():
        c = table.get(tuple(q))
        if c is None or c[0] < min_weight:
            out.append((-1, frozenset()))
            continue
        pairs, kinds = 0, set()
        for a in range(3):
            hi, lo = list(q), list(q)
            hi[a] += 1; lo[a] -= 1
            vh, vl = table.get(tuple(hi)), table.get(tuple(lo))
            if vh is None or vl is None or vh[0] < min_weight or vl[0] < min_weight:
                continue
            pairs += 1
            kinds.add("ff" if vh[1] and vl[1] else ("aa" if not vh[1] and not vl[1] else "fa"))
        out.append((pairs, frozenset(kinds)))
    return out


def equal_neighbours():
    """voxel_size 0.05, trunc 0.02 (a band inside one voxel): three rays along +z, one per call with its own origin, whose
    x index is 1, 2, 3 and whose z arithmetic is identical.  Voxels (1,1,k) and (3,1,k) then hold the same value, (2,1,k)
    has no other neighbours: the query of (2,1,k) has one valid pair and a zero gradient -> status 1.
    Returns [(points, conf, origin)] * 3 and (vs, trunc, max_weight, step_scale)."""
    calls = []
    for ix, conf in ((1, 1.0), (2, 2.0), (3, 1.0)):
        x = np.float32(0.05 * ix + 0.025)
        calls.append((np.array([[x, 0.075, 0.475]], np.float32), np.array([conf]), np.array([x, 0.075, 0.0], np.float32)))
    return calls, (0.05, 0.02, 100.0, 0.5)
