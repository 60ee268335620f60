"""Point clouds on the device: a spatial index, the exact nearest neighbour of points in a cloud, the voxel downsample,
trimmed point-to-point ICP and the accuracy / completion / precision / recall / F-score / Chamfer figures between two
clouds - what scores the product's own output (evaluate.save_reconstruction's cloud) against a scan without faces.

No counterpart in the reference.  The kernels are csrc/cloud.hip (DESIGN.md "Point clouds"); the numpy statement of the
same definitions is tests/cloud_numpy.py.  A cloud is points f32[N,3]; a point is valid when its three coordinates are
finite.  An invalid point is never anyone's nearest neighbour, is never fused into a voxel and enters no figure.
"""
import math

import torch

import mslam_hip as _m

from ._mesh_args import _points_arg, _sim3_arg
from .mesh_align import (DEGENERATE, LOG_DOUBLES, OK, STATE_BYTES, _alignment_arg, _icp_args, _icp_run,
                         _read_state)
from .mesh_index import _index_arg, _sorted_scan, _SpatialIndex
from .mesh_metrics import _fscore_chamfer

_NONE = torch.iinfo(torch.int64).max


def _valid(points):
    return torch.isfinite(points).all(1)


class CloudIndex(_SpatialIndex):
    """The index of the cloud `points` f32[N,3] (a device tensor), built once and passed as `index=` to cloud_distance,
    align_clouds and compare_clouds for that same tensor.  It keeps the tensor (never copied or permuted), `order`
    i32[N] - the valid points by the Morton code of their place in the box of the valid points, invalid points last,
    from a stable sort - and the workspace of the boxes of the 128-point tiles and of the groups of 32 tiles."""

    def __init__(self, points):
        what = "CloudIndex"
        self.shape = tuple(points.shape) if torch.is_tensor(points) else None
        self.pointer = points.data_ptr() if self.shape is not None else None
        self.p = _points_arg(points, "points", what)
        self.N = int(self.p.shape[0])
        dev = self.device = self.p.device
        if self.N:
            ok = _valid(self.p)
            inf = torch.tensor(math.inf, dtype=torch.float32, device=dev)
            self.bounds = torch.cat((torch.where(ok[:, None], self.p, inf).amin(0),
                                     torch.where(ok[:, None], self.p, -inf).amax(0))).contiguous()
            keys = torch.where(ok, self.point_keys(self.p), _NONE)
        else:
            self.bounds = torch.zeros(6, dtype=torch.float32, device=dev)
            keys = torch.empty(0, dtype=torch.int64, device=dev)
        self._build(keys, self.N, "cloud_index", (_m.ptr(self.p), self.N))

    def check(self, points, what):
        """Raises ValueError unless the index was built for this very tensor: the same shape and data pointer."""
        same = (torch.is_tensor(points) and self.shape is not None and tuple(points.shape) == self.shape
                and points.data_ptr() in (self.pointer, self.p.data_ptr()))
        if not same:
            raise ValueError(f"{what}: the CloudIndex was built for another cloud (shape or data pointer differs)")
        return self


def _distance2(queries, points, index=None, sort_queries=True, levels=2):
    """(dist2 f64[n], nearest i32[n]) of the checked arguments."""
    n, N = int(queries.shape[0]), int(points.shape[0])
    # without an index: no order, no boxes, and levels 1, which the plain scan does not read
    order, ws, ws_bytes, levels = (0, 0, 0, 1) if index is None else (_m.ptr(index.order), _m.ptr(index.ws),
                                                                      index.ws_bytes, levels)

    def scan(q, dist2, nearest):
        _m.check(_m.lib().mslam_cloud_distance(_m.ptr(q), n, _m.ptr(points), N, order, ws, ws_bytes, levels, 0,
                                               _m.ptr(dist2), _m.ptr(nearest), _m.stream_ptr()), "cloud_distance")

    return _sorted_scan(queries, index, sort_queries, scan)


def cloud_distance(queries, points, index=None, sort_queries=True):
    """Exact nearest neighbour of the queries f32[n,3] in the cloud `points` f32[N,3] -> (distance f64[n], nearest i32[n])
    device tensors: the distance to the nearest valid point and the lowest index of a point at that distance; +inf and
    -1 for a query with a non-finite coordinate and for a cloud without a valid point.  The squared distance is the f64
    sum of the squared f64 differences of the f32 coordinates.  `index`: None - the plain scan of every point; True - a
    CloudIndex of the cloud is built first; a CloudIndex built for this tensor - tiles and groups of tiles whose boxes
    lie beyond a query block's current bests are not scanned, and with `sort_queries` the queries are scanned in the
    order of their Morton keys and the results scattered back.  The same bits in every form (DESIGN.md "Point
    clouds")."""
    what = "cloud_distance"
    queries = _points_arg(queries, "queries", what)
    index = _index_arg(CloudIndex, index, what, points)
    points = _points_arg(points, "points", what)
    if queries.device != points.device:
        raise ValueError(f"{what}: queries and points are on different devices")
    dist2, nearest = _distance2(queries, points, index, sort_queries)
    return torch.sqrt(dist2), nearest


def _colors_arg(colors, n, what):
    if not torch.is_tensor(colors):
        raise TypeError(f"{what}: colors must be a device tensor")
    if tuple(colors.shape) != (n, 3):
        raise ValueError(f"{what}: colors must be ({n},3), got {tuple(colors.shape)}")
    _m.require_dtype(colors, torch.uint8, "colors")
    _m.ptr(colors)
    return colors.contiguous()


def downsample_cloud(points, voxel, colors=None, return_first=False):
    """The cloud thinned on the grid of cell size `voxel`, the global TSDF's grid (floor(f32 x / f32 voxel) per axis):
    one point per occupied cell, in key order -> (points f32[M,3], colors u8[M,3] or None, count i32[M]).  A point is
    the centroid of its cell's members: their f64 sum in original index order, divided by the count and rounded once;
    a colour (`colors` u8[N,3]) is the rounded integer mean per channel, halves up.  Invalid points and points outside
    the TSDF's key range are dropped.  The same bits on every call; the order of summation is the definition, so a
    shuffled cloud gives the same cells and counts and centroids that may differ in the last bit.  One host read: the
    number of cells.  `return_first`: also first i32[M], the lowest original index in each cell."""
    what = "downsample_cloud"
    points = _points_arg(points, "points", what)
    N, dev = int(points.shape[0]), points.device
    if not (float(voxel) > 0.0 and math.isfinite(float(voxel))):
        raise ValueError(f"{what}: voxel must be positive and finite, got {voxel}")
    if colors is not None:
        colors = _colors_arg(colors, N, what)
        if colors.device != dev:
            raise ValueError(f"{what}: points and colors are on different devices")
    L, st = _m.lib(), _m.stream_ptr()
    keys = torch.empty(N, dtype=torch.int64, device=dev)
    _m.check(L.mslam_cloud_voxel_keys(_m.ptr(points), N, float(voxel), _m.ptr(keys), st), "cloud_voxel_keys")
    skeys, perm = torch.sort(keys, stable=True)
    head = skeys != _NONE
    if N > 1:
        head[1:] &= skeys[1:] != skeys[:-1]
    starts = torch.nonzero(head).reshape(-1)                                     # the host read: M
    M = int(starts.shape[0])
    centroid = torch.empty((M, 3), dtype=torch.float32, device=dev)
    count = torch.empty(M, dtype=torch.int32, device=dev)
    first = torch.empty(M, dtype=torch.int32, device=dev)
    color = torch.empty((M, 3), dtype=torch.uint8, device=dev) if colors is not None else None
    _m.check(L.mslam_cloud_voxel_reduce(_m.ptr(points), _m.ptr(colors), N, _m.ptr(skeys), _m.ptr(perm), _m.ptr(starts), M,
                                        _m.ptr(centroid), _m.ptr(count), _m.ptr(first), _m.ptr(color), st),
             "cloud_voxel_reduce")
    return (centroid, color, count, first) if return_first else (centroid, color, count)


# not merged with mesh_align.transform_mesh: this one is an elementwise f64 sum in a stated order, that one a matmul,
# they round differently and tests pin the bits of each
def transform_cloud(points, T, _normalise=True):
    """The points f32[n,3] moved by the Sim3 T [t(3), q(xyzw), s]: s (R p) + t per coordinate in f64, rounded once to
    f32.  Elementwise torch ops on the points' device, one multiply or add each; the quaternion is normalised first
    (align_clouds, whose state is normalised already, passes it as it is)."""
    T = _sim3_arg(T, "transform_cloud", points.device, torch.float64)
    x, y, z, w = T[3:7] / torch.sqrt((T[3:7] * T[3:7]).sum()) if _normalise else T[3:7]
    R = ((1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)),
         (2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)),
         (2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)))
    p = points.to(torch.float64)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    return torch.stack([T[7] * ((r[0] * px + r[1] * py) + r[2] * pz) + T[k] for k, r in enumerate(R)], 1).to(
        torch.float32).contiguous()


def stride_sample(points, n_samples):
    """The deterministic subsample of the valid points of `points`: those at floor(i N / n) of the N valid ones, i < n
    = min(n_samples, N), in index order -> (f32[n,3], their original indices i64[n]).  One host read: N."""
    idx = torch.nonzero(_valid(points)).reshape(-1)
    N = int(idx.shape[0])
    n = min(int(n_samples), N)
    pick = (torch.arange(n, dtype=torch.int64, device=points.device) * N) // max(n, 1)
    idx = idx[pick]
    return points[idx].contiguous(), idx


def align_clouds(pred, gt, init=None, n_samples=20000, max_iters=50, trim=math.inf, with_scale=True, tol=1e-6,
                 check_every=5, index=None, _trace=None):
    """Trimmed point-to-point ICP of the cloud `pred` onto the cloud `gt` (f32[N,3] device tensors): the Sim3 T with
    T(pred) ~ gt.  The arguments, the returned dict and the stop rule are align_meshes' (mesh_align._icp_args, _icp_run).

    The source sample is stride_sample(pred, n_samples), drawn once.  Every iteration moves it by the current T (f64,
    rounded once to f32), finds each moved point's nearest neighbour in gt (cloud_distance; `index`: None, True or a
    CloudIndex of gt), gives a pair the weight 1 when it has a neighbour and its distance is <= `trim` (gt's units;
    +inf keeps all; a sequence gives one value per iteration), and replaces T by the closed-form similarity of the
    ORIGINAL sample onto the neighbours (mslam_mesh_align_fit_pairs; `with_scale=False`: scale 1).  A degenerate
    iteration (fewer than 3 pairs, no spread) leaves T as it was.  Nothing is read back except the log, once every
    `check_every` iterations; the loop stops when the RMSE of two successive iterations differs by at most `tol`
    relative, when an iteration is degenerate, or after `max_iters`.  Like every ICP it is a LOCAL method and needs
    `init` (a Sim3, default the identity) beyond a modest offset.

    Returns a dict: T (f64[8] device tensor), iterations, converged, rmse and inliers (of the last iteration: the pairs
    within trim under the T that iteration started from, and their RMSE), history (numpy f64[iterations, 4]: inliers,
    rmse, scale after the solve, status)."""
    what = "align_clouds"
    max_iters, check_every, trims = _icp_args(what, max_iters, check_every, tol, trim)
    if int(n_samples) < 1:
        raise ValueError(f"{what}: n_samples must be >= 1, got {n_samples}")
    pred = _points_arg(pred, "pred", what)
    index = _index_arg(CloudIndex, index, what, gt)
    gt = _points_arg(gt, "gt", what)
    if pred.device != gt.device:
        raise ValueError(f"{what}: pred and gt are on different devices")
    dev = pred.device
    src = stride_sample(pred, n_samples)[0]
    n = int(src.shape[0])
    T = torch.tensor([0, 0, 0, 0, 0, 0, 1, 1], dtype=torch.float64, device=dev)
    if init is not None:
        T = _sim3_arg(init, what, dev, torch.float64).clone()
        T[3:7] = T[3:7] / torch.sqrt((T[3:7] * T[3:7]).sum())
    L, st = _m.lib(), _m.stream_ptr()
    ws_bytes = int(L.mslam_mesh_align_workspace_bytes(n, 0, 0))
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    state = torch.empty(STATE_BYTES, dtype=torch.uint8, device=dev)
    fit_log = torch.zeros(LOG_DOUBLES, dtype=torch.float64, device=dev)
    log = torch.zeros((max_iters, 4), dtype=torch.float64, device=dev)
    inf = torch.tensor(math.inf, dtype=torch.float64, device=dev)

    def step(it):
        nonlocal T
        moved = transform_cloud(src, T, _normalise=False)
        dist2, nearest = _distance2(moved, gt, index)
        has = nearest >= 0
        w = (has & (torch.sqrt(dist2) <= trims[it])).to(torch.float32)
        if n and int(gt.shape[0]):
            dst = torch.where(has[:, None], gt[nearest.clamp_min(0).long()], torch.zeros_like(moved)).contiguous()
            _m.check(L.mslam_mesh_align_fit_pairs(_m.ptr(src), _m.ptr(dst), _m.ptr(w), n, 1 if with_scale else 0,
                                                  _m.ptr(ws), ws_bytes, _m.ptr(state), _m.ptr(fit_log), st),
                     "mesh_align_fit_pairs")
            T_new, _, status = _read_state(state)
        else:                                                              # no sample or no target: nothing to fit
            dst, T_new = torch.zeros_like(moved), T
            status = torch.full((1,), DEGENERATE, dtype=torch.int32, device=dev)
        T_before = T
        T = torch.where(status == OK, T_new, T)
        w64 = w.to(torch.float64)
        pairs = w64.sum()
        rmse = torch.where(pairs > 0, torch.sqrt((w64 * torch.where(has, dist2, torch.zeros_like(dist2))).sum()
                                                 / pairs), inf)
        log[it] = torch.stack((pairs, rmse, T[7], status[0].to(torch.float64)))
        if _trace is not None:
            _trace.append(dict(T_before=T_before, moved=moved, dist2=dist2, nearest=nearest, weights=w, dst=dst,
                               fit_log=fit_log.clone(), T=T, status=status.clone()))

    iterations, converged, hist = _icp_run(step, log, max_iters, check_every, tol)
    return dict(T=T, iterations=iterations, converged=converged, rmse=float(hist[-1, 1]), inliers=int(hist[-1, 0]),
                history=hist)


def _direction(queries, points, index, threshold, max_dist):
    """The figures of one direction as 0-d f64 device tensors: mean, median, rmse over the valid queries within
    max_dist, the share of the valid queries within threshold, the valid queries beyond max_dist, the valid queries."""
    dev = queries.device
    dist2 = _distance2(queries, points, index)[0]
    d = torch.sqrt(dist2)
    ok = _valid(queries)
    kept = ok & (d <= max_dist)
    m = kept.sum()
    mf = m.to(torch.float64)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    mean = torch.where(kept, d, zero).sum() / mf
    rmse = torch.sqrt(torch.where(kept, dist2, zero).sum() / mf)
    s = torch.sort(torch.where(kept, d, torch.full_like(d, math.inf)))[0]
    if int(s.shape[0]):
        lo, hi = ((m - 1).clamp_min(0) // 2).reshape(1), (m // 2).clamp_max(int(s.shape[0]) - 1).reshape(1)
        median = torch.where(m > 0, 0.5 * (s[lo] + s[hi])[0], zero * math.nan)
    else:
        median = zero * math.nan
    n_ok = ok.sum().to(torch.float64)
    within = (ok & (d <= threshold)).sum().to(torch.float64) / n_ok
    return [mean, median, rmse, within, (ok & ~(d <= max_dist)).sum().to(torch.float64), n_ok]


def compare_clouds(pred, gt, threshold=0.05, voxel=None, max_dist=None, align=None, align_kw=None, index=None):
    """Quality of the cloud `pred` against the ground-truth cloud `gt` (f32[N,3] device tensors, one frame): the figure
    set of compare_meshes, from the points themselves.  Returns Python numbers: accuracy / accuracy_median /
    accuracy_rmse (every valid pred point to its nearest gt point: mean, median, root mean square), completion /
    completion_median / completion_rmse (gt to pred), precision / recall (share of the valid pred / gt points within
    `threshold`), fscore (their harmonic mean, 0 when both are 0), chamfer = (accuracy + completion) / 2, n_pred, n_gt
    (the valid points that were scored), threshold, voxel, max_dist, accuracy_outliers, completion_outliers.  The means
    are f64 sums; one host read of the figures (and one per downsample_cloud).  ValueError when a cloud has no valid
    point.

    `voxel`: both clouds are thinned by downsample_cloud(., voxel) first, so that the figures weigh space and not how
    long the camera looked at it.  `max_dist`: pairs farther apart are left out of the means, medians and rms values and
    counted in accuracy_outliers / completion_outliers; they still count against precision and recall.

    `align`: None - the clouds are taken as they are; a Sim3 - pred is moved by it first (transform_cloud); "icp" - by
    align_clouds(pred, gt, **align_kw) (a local method: pass align_kw=dict(init=...) beyond a modest offset).  With
    alignment the dict gains `alignment`: T (8 floats), rmse and iterations (None for a given Sim3).

    `index`: None - plain scans, every pair is measured; True - a CloudIndex of each cloud is built; a CloudIndex of
    `gt` (without `voxel`, which makes a new tensor) - that one and a new one of pred.  The dict is the same, value for
    value."""
    what = "compare_clouds"
    threshold = float(threshold)
    limit = math.inf if max_dist is None else float(max_dist)
    if not limit >= 0.0:
        raise ValueError(f"{what}: max_dist must be >= 0, got {max_dist}")
    if voxel is not None and isinstance(index, CloudIndex):
        raise ValueError(f"{what}: voxel= thins gt into a new tensor; pass index=True with it")
    pred = _points_arg(pred, "pred", what)
    gt_given = gt
    gt = _points_arg(gt, "gt", what)
    if pred.device != gt.device:
        raise ValueError(f"{what}: pred and gt are on different devices")
    if voxel is not None:
        pred, gt = downsample_cloud(pred, voxel)[0], downsample_cloud(gt, voxel)[0]
        gt_given = gt
    g_index = _index_arg(CloudIndex, index, what, gt_given)
    T, alignment = _alignment_arg(what, align, align_kw, lambda **kw: align_clouds(pred, gt, index=g_index, **kw))
    if T is not None:
        pred = transform_cloud(pred, T)
    p_index = CloudIndex(pred) if g_index is not None else None
    figures = _direction(pred, gt, g_index, threshold, limit) + _direction(gt, pred, p_index, threshold, limit)
    (acc, acc_med, acc_rms, prec, acc_out, n_pred, comp, comp_med, comp_rms, rec, comp_out,
     n_gt) = torch.stack(figures).tolist()                                    # the one host read of the figures
    if n_pred == 0 or n_gt == 0:
        raise ValueError(f"{what}: a cloud has no valid point ({int(n_pred)} in pred, {int(n_gt)} in gt)")
    out = dict(accuracy=acc, accuracy_median=acc_med, accuracy_rmse=acc_rms, completion=comp,
               completion_median=comp_med, completion_rmse=comp_rms, precision=prec, recall=rec,
               **_fscore_chamfer(prec, rec, acc, comp), n_pred=int(n_pred), n_gt=int(n_gt), threshold=threshold, voxel=None if voxel is None else float(voxel),
               max_dist=None if max_dist is None else limit, accuracy_outliers=int(acc_out),
               completion_outliers=int(comp_out))
    if alignment is not None:
        out["alignment"] = alignment
    return out
