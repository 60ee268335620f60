"""Numpy statement of the point-cloud tools (DESIGN.md "Point clouds"; the kernels are csrc/cloud.hip, the Python layer
mast3r_slam/tsdf/cloud.py): validity, the exact nearest neighbour with its tie rule, the cloud index, the voxel keys and
the voxel reduce with world_to_key's arithmetic, the figures of compare_clouds and one iteration of align_clouds.
Everything is f64 on the f32 inputs, and the operation order written here is the kernel's.  Beside the statement stand
the WRONG forms its tests must tell from it: f32 arithmetic, a fused multiply-add, the first point met on a tie."""
import math
from fractions import Fraction

import numpy as np

import meshalign_numpy as A
import meshindex_numpy as X

TILE, GROUP = X.TILE, X.GROUP
NONE = X.NONE                      # INT64_MAX: an invalid point's Morton key, an undefined voxel key
KEY_BIAS = 1 << 20                 # kKeyBias of csrc/tsdf_table.h: voxel indices lie in [-2^20, 2^20)
OK, DEGENERATE = A.OK, A.DEGENERATE


def f32(points):
    return np.asarray(points, np.float32).reshape(-1, 3)


def valid(points):
    """bool[N]: the three coordinates are finite."""
    return np.isfinite(f32(points)).all(1)


# ----------------------------------------------------------------------------------------------------------------------
# nearest neighbour
# ----------------------------------------------------------------------------------------------------------------------
def dist2_matrix(queries, points):
    """f64[n,N]: (dx dx + dy dy) + dz dz of the f64 differences, two roundings per a * b + c."""
    q, p = f32(queries).astype(np.float64), f32(points).astype(np.float64)
    with np.errstate(all="ignore"):
        d = q[:, None, :] - p[None, :, :]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest(queries, points, chunk=2048):
    """(dist2 f64[n], nearest i32[n]): brute force, the lowest index on ties (argmin returns the first minimum); +inf and
    -1 for a query with a non-finite coordinate and for a cloud without a valid point."""
    q, p = f32(queries), f32(points)
    ok_p, ok_q = valid(p), valid(q)
    best = np.full(len(q), np.inf)
    idx = np.full(len(q), -1, np.int32)
    if not ok_p.any():
        return best, idx
    for s in range(0, len(q), chunk):
        d = dist2_matrix(q[s:s + chunk], p)
        d[:, ~ok_p] = np.inf
        j = np.argmin(d, 1)
        m = ok_q[s:s + chunk]
        best[s:s + chunk][m] = d[np.arange(len(j)), j][m]
        idx[s:s + chunk][m] = j[m]
    return best, idx


def nearest_f32(queries, points):
    """THE WRONG FORM: the same scan in f32 arithmetic."""
    q, p = f32(queries), f32(points)
    d = q[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == np.float32
    return d2.min(1), np.argmin(d2, 1).astype(np.int32)


def nearest_in_order(queries, points, order, tie="index"):
    """(dist2, nearest) of a scan that visits the points in `order`.  tie "index": d < best or (d == best and j < best_j)
    on the original index, the kernel's rule; "first": strict <, THE WRONG FORM of a permuted scan."""
    q, p = f32(queries), f32(points)
    ok = valid(p)
    best = np.full(len(q), np.inf)
    idx = np.full(len(q), -1, np.int32)
    for j in np.asarray(order, np.int64):
        if not (0 <= j < len(p)) or not ok[j]:
            continue
        d = dist2_matrix(q, p[j:j + 1])[:, 0]
        better = d < best
        if tie == "index":
            better |= (d == best) & (j < idx)
        better &= valid(q)
        best = np.where(better, d, best)
        idx = np.where(better, np.int32(j), idx)
    return best, idx


def _round(x):
    """A Fraction rounded to the nearest f64 (ties to even: Python's float(Fraction) is correctly rounded)."""
    return float(x)


def dist2_fused(q, p):
    """THE WRONG FORM: fma(dz, dz, fma(dy, dy, dx * dx)) of the f64 differences - what a contracting compiler makes of
    the sum - emulated exactly with fractions.  q, p: three f32 numbers each."""
    d = [float(np.float64(np.float32(a)) - np.float64(np.float32(b))) for a, b in zip(q, p)]
    acc = _round(Fraction(d[0]) * Fraction(d[0]))
    acc = _round(Fraction(d[1]) * Fraction(d[1]) + Fraction(acc))
    return _round(Fraction(d[2]) * Fraction(d[2]) + Fraction(acc))


def contraction_cases(seed=0, tries=4000):
    """[(q, p)] f32 pairs whose fused squared distance has other bits than the statement's."""
    rng = np.random.default_rng(seed)
    found = []
    for _ in range(tries):
        q, p = rng.uniform(-2.0, 2.0, 3).astype(np.float32), rng.uniform(-2.0, 2.0, 3).astype(np.float32)
        if dist2_fused(q, p) != float(dist2_matrix(q[None], p[None])[0, 0]):
            found.append((q, p))
    return found


# ----------------------------------------------------------------------------------------------------------------------
# the cloud index
# ----------------------------------------------------------------------------------------------------------------------
def bounds(points):
    """f32[6] = lo.xyz, hi.xyz over the VALID points; (+inf, -inf) without one, zeros for an empty cloud."""
    p = f32(points)
    if not len(p):
        return np.zeros(6, np.float32)
    ok = valid(p)
    lo = np.where(ok[:, None], p, np.float32(np.inf)).min(0)
    hi = np.where(ok[:, None], p, np.float32(-np.inf)).max(0)
    return np.concatenate([lo, hi]).astype(np.float32)


def point_keys(points, bnd=None):
    """int64[N]: the Morton code of each valid point in the box of the valid points, INT64_MAX for an invalid one."""
    p = f32(points)
    with np.errstate(all="ignore"):
        keys = X.point_keys(p, bounds(p) if bnd is None else bnd)
    return np.where(valid(p), keys, NONE)


def order_of(keys):
    return X.order_of(keys)


def boxes(points, order):
    """(tile f64[ntiles,6], group f64[ngroups,6]): lo.xyz, hi.xyz over the valid points order[128 t + k] of tile t, an
    entry outside [0, N) skipped; then over the tiles of each group of 32.  An empty one is (+inf, -inf)."""
    p = f32(points)
    ok = valid(p)
    n = len(p)
    order = np.asarray(order, np.int64)
    ntiles = (n + TILE - 1) // TILE
    ngroups = (ntiles + GROUP - 1) // GROUP
    empty = np.array([np.inf] * 3 + [-np.inf] * 3)
    tile = np.tile(empty, (ntiles, 1))
    for t in range(ntiles):
        o = order[TILE * t:TILE * (t + 1)]
        o = o[(o >= 0) & (o < n)]
        o = o[ok[o]]
        if len(o):
            tile[t, :3], tile[t, 3:] = p[o].astype(np.float64).min(0), p[o].astype(np.float64).max(0)
    group = np.tile(empty, (ngroups, 1))
    for g in range(ngroups):
        part = tile[GROUP * g:GROUP * (g + 1)]
        group[g, :3], group[g, 3:] = part[:, :3].min(0), part[:, 3:].max(0)
    return tile, group


# ----------------------------------------------------------------------------------------------------------------------
# voxel downsample
# ----------------------------------------------------------------------------------------------------------------------
def voxel_keys(points, voxel_size):
    """int64[N]: world_to_key of csrc/tsdf_table.h - q = floor(f32 coordinate / f32 voxel_size) in f32, refused unless
    |q| < 2^21 (decided on the float), then the index range [-2^20, 2^20) per axis, packed x << 42 | y << 21 | z with the
    bias 2^20 - or INT64_MAX for an invalid or out-of-range point."""
    p = f32(points)
    vs = np.float32(voxel_size)
    with np.errstate(all="ignore"):
        q = np.floor(p / vs)
    assert q.dtype == np.float32
    with np.errstate(all="ignore"):
        ok = valid(p) & (np.abs(q) < np.float32(2.0 * KEY_BIAS)).all(1)
    k = np.where(ok[:, None], q, 0).astype(np.int64) + KEY_BIAS
    ok &= ((k >= 0) & (k < 2 * KEY_BIAS)).all(1)
    keys = (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]
    return np.where(ok, keys, NONE)


def voxel_reduce(points, voxel_size, colors=None):
    """(centroid f32[M,3], count i32[M], first i32[M], color u8[M,3] or None, keys i64[M]) in key order.  The centroid
    is the f64 sum of the members in original index order, one addition at a time (cumsum, not numpy's pairwise sum),
    divided by the count and rounded once; the colour (2 sum + count) // (2 count) in integers."""
    p = f32(points)
    keys = voxel_keys(p, voxel_size)
    perm = np.argsort(keys, kind="stable")
    sk = keys[perm]
    live = sk != NONE
    head = live & np.r_[True, sk[1:] != sk[:-1]] if len(sk) else live
    starts = np.flatnonzero(head)
    ends = np.r_[starts[1:], int(live.sum())]
    M = len(starts)
    centroid = np.zeros((M, 3), np.float32)
    count, first = np.zeros(M, np.int32), np.zeros(M, np.int32)
    color = None if colors is None else np.zeros((M, 3), np.uint8)
    for v, (s, e) in enumerate(zip(starts, ends)):
        members = perm[s:e]
        assert (np.diff(members) > 0).all()                      # a stable sort: original index order
        total = np.cumsum(p[members].astype(np.float64), 0)[-1]
        centroid[v] = (total / float(e - s)).astype(np.float32)
        count[v], first[v] = e - s, members[0]
        if colors is not None:
            c = np.asarray(colors, np.uint8).reshape(-1, 3)[members].astype(np.int64).sum(0)
            color[v] = (2 * c + (e - s)) // (2 * (e - s))
    return centroid, count, first, color, sk[starts]


# ----------------------------------------------------------------------------------------------------------------------
# figures
# ----------------------------------------------------------------------------------------------------------------------
def _direction(queries, points, threshold, max_dist):
    d2 = nearest(queries, points)[0]
    d = np.sqrt(d2)
    ok = valid(queries)
    kept = ok & (d <= max_dist)
    m = int(kept.sum())
    s = np.sort(d[kept])
    return dict(mean=math.fsum(d[kept]) / m if m else math.nan,
                median=0.5 * (s[(m - 1) // 2] + s[m // 2]) if m else math.nan,
                rmse=math.sqrt(math.fsum(d2[kept]) / m) if m else math.nan,
                within=int((ok & (d <= threshold)).sum()) / int(ok.sum()),
                outliers=int((ok & ~(d <= max_dist)).sum()), n=int(ok.sum()), kept=m)


def figures(pred, gt, threshold=0.05, max_dist=None):
    """The dict of compare_clouds for clouds in one frame, with exact (fsum) means."""
    limit = np.inf if max_dist is None else float(max_dist)
    a, c = _direction(pred, gt, threshold, limit), _direction(gt, pred, threshold, limit)
    prec, rec = a["within"], c["within"]
    return dict(accuracy=a["mean"], accuracy_median=a["median"], accuracy_rmse=a["rmse"], completion=c["mean"],
                completion_median=c["median"], completion_rmse=c["rmse"], precision=prec, recall=rec,
                fscore=2.0 * prec * rec / (prec + rec) if prec + rec > 0.0 else 0.0,
                chamfer=0.5 * (a["mean"] + c["mean"]), n_pred=a["n"], n_gt=c["n"], threshold=float(threshold),
                accuracy_outliers=a["outliers"], completion_outliers=c["outliers"], n_pred_kept=a["kept"],
                n_gt_kept=c["kept"])


# ----------------------------------------------------------------------------------------------------------------------
# ICP
# ----------------------------------------------------------------------------------------------------------------------
def stride_sample(points, n_samples):
    """(f32[n,3], indices): the valid points at floor(i N / n), i < n = min(n_samples, N)."""
    idx = np.flatnonzero(valid(points))
    N = len(idx)
    n = min(int(n_samples), N)
    idx = idx[(np.arange(n, dtype=np.int64) * N) // max(n, 1)]
    return f32(points)[idx], idx


def icp_step(T, src, gt, trim=np.inf, with_scale=True, moved=None):
    """One iteration of align_clouds from the state T f64[8] on the sample src f32[n,3]: move (f64, rounded once; or
    take `moved` as given), nearest neighbours, weights, the Horn solve of the TOTAL transform src -> gt[nearest] about
    the origins src[0], dst[0] (the statement of mslam_mesh_align_fit_pairs).  A degenerate solve keeps T."""
    P = f32(src).astype(np.float64)
    if moved is None:
        moved = A.act(T, P).astype(np.float32)
    d2, nn = nearest(moved, gt)
    has = nn >= 0
    with np.errstate(all="ignore"):
        w = (has & (np.sqrt(d2) <= np.float64(trim))).astype(np.float64)
    C = np.where(has[:, None], f32(gt)[np.maximum(nn, 0)], np.float32(0)).astype(np.float64)
    out = dict(moved=moved, dist2=d2, nearest=nn, weights=w, dst=C)
    if len(P) == 0:
        return dict(out, T=np.asarray(T, np.float64), status=DEGENERATE, rmse=np.inf, inliers=0, sums=np.zeros(A.N_SUMS))
    r = C - P
    sums = A.sum_terms(P, C, w, w > 0.0, P[0], C[0], (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]).sum(0)
    Tn = A.horn_solve(sums, P[0], C[0], with_scale)
    pairs = w.sum()
    rmse = math.sqrt(math.fsum(d2[w > 0.0]) / pairs) if pairs > 0 else np.inf
    return dict(out, sums=sums, T=np.asarray(T, np.float64) if Tn is None else Tn,
                status=DEGENERATE if Tn is None else OK, rmse=rmse, inliers=int(pairs))


def icp(src, gt, T0=None, iters=50, trim=np.inf, with_scale=True):
    """`iters` steps from T0 (f64[8] or None) -> (T f64[8], history f64[iters,4]: inliers, rmse at T_k, scale after the
    solve, status)."""
    T = A.init_state() if T0 is None else np.asarray(T0, np.float64)
    hist = np.zeros((iters, 4))
    for k in range(iters):
        st = icp_step(T, src, gt, trim, with_scale)
        T = st["T"]
        hist[k] = st["inliers"], st["rmse"], T[7], st["status"]
    return T, hist
