"""Point clouds on the device: a spatial index, the exact nearest neighbour of points in a cloud, the voxel downsample,
trimmed point-to-point ICP and the accuracy / completion / precision / recall / F-score / Chamfer figures between two
clouds - what scores the product's own output (evaluate.save_reconstruction's cloud) against a scan without faces.
Below them the k nearest neighbours under a total order, and what stands on them: normals, the statistical and the
radius outlier rule, the normal-consistency figures of compare_clouds.  The views of a cloud and the observed part that
compare_clouds(observed=...) scores are cloud_view.py's; the count within a radius and the density clusters are
cloud_cluster.py's.

No counterpart in the reference.  The kernels are csrc/cloud.hip and csrc/cloud_knn.hip (DESIGN.md "Point clouds"); the
numpy statements of the same definitions are tests/cloud_numpy.py and tests/cloud_knn_numpy.py.  A cloud is points f32[N,3]; a point is valid when its three coordinates are
finite.  An invalid point is never anyone's nearest neighbour, is never fused into a voxel and enters no figure.
"""
import math

import numpy as np
import torch

import mslam_hip as _m

from ._mesh_args import _points_arg, _sim3_arg
from .mesh_align import (DEGENERATE, LOG_DOUBLES, OK, STATE_BYTES, _alignment_arg, _icp_args, _icp_run,
                         _icp_setup, _metric_arg, _read_state, _state_run)
from .mesh_index import _NEAREST, _index_arg, _index_ops, _sorted_scan, _SpatialIndex
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

    def scan(q, dist2, nearest):
        _m.check(_m.lib().mslam_cloud_distance(_m.ptr(q), n, _m.ptr(points), N, *_index_ops(index, levels), 0,
                                               _m.ptr(dist2), _m.ptr(nearest), _m.stream_ptr()), "cloud_distance")

    return _sorted_scan(queries, index, sort_queries, _NEAREST, scan)


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


def _align_clouds_plane(what, src, gt, init, trims, with_scale, tol, max_iters, check_every, index, normals,
                        point_weight, trace):
    """align_clouds with metric="plane" on the checked arguments: the normals, the state, and mesh_align._state_run
    over mslam_icp_plane_step_cloud."""
    n, N, dev = int(src.shape[0]), int(gt.shape[0]), src.device
    if torch.is_tensor(normals):
        if tuple(normals.shape) != (N, 3):
            raise ValueError(f"{what}: normals must be gt's, ({N},3), got {tuple(normals.shape)}")
        _m.require_dtype(normals, torch.float32, "normals")
        _m.ptr(normals)
        if normals.device != dev:
            raise ValueError(f"{what}: normals and gt are on different devices")
        normals = normals.contiguous()
    else:
        k = _k_arg(normals, what, "normals")
        normals = (cloud_normals(gt, k, index=index if index is not None else True)[0] if N
                   else torch.zeros((0, 3), dtype=torch.float32, device=dev))
    T0 = None if init is None else _sim3_arg(init, what, dev, torch.float32)
    L, st = _m.lib(), _m.stream_ptr()
    ws_bytes = int(L.mslam_icp_plane_workspace_bytes(n, 0))
    ws, state = _icp_setup(dev, ws_bytes, T0)

    def launch(it, nearest, moved, dist2, closest, log_row):
        _m.check(L.mslam_icp_plane_step_cloud(_m.ptr(src), n, _m.ptr(gt), _m.ptr(normals), N, *_index_ops(index),
                                              trims[it], point_weight, 1 if with_scale else 0, _m.ptr(ws), ws_bytes,
                                              _m.ptr(state), _m.ptr(nearest), _m.ptr(moved), _m.ptr(dist2), closest,
                                              log_row, st), "icp_plane_step_cloud")

    return _state_run(src, state, launch, True, max_iters, check_every, tol, trace)


def align_clouds(pred, gt, init=None, n_samples=20000, max_iters=50, trim=math.inf, with_scale=True, tol=1e-6,
                 check_every=5, index=None, metric="point", normals=16, point_weight=0.0, _trace=None):
    """Trimmed point-to-point ICP of the cloud `pred` onto the cloud `gt` (f32[N,3] device tensors): the Sim3 T with
    T(pred) ~ gt.  The arguments, the returned dict and the stop rule are align_meshes' (mesh_align._icp_args, _icp_run).

    `metric`: "point" - what follows; "plane" - the point-to-plane metric (DESIGN.md "Point-to-plane ICP"): one fused
    launch per iteration moves the sample, finds the nearest neighbours (the same scan, the same bits) and accumulates
    n . (q - c) with the neighbour's normal n, and a second one solves for a small Sim3 and composes it onto T.
    `normals`: a k - cloud_normals(gt, k) once before the loop - or gt's normals f32[N,3] themselves; a pair whose
    neighbour has a zero or non-finite normal does not count.  The metric constrains nothing ALONG a surface: where few
    normals face some direction (normal_spread near 0) the sample slides, and `point_weight` > 0 (0.05 is a mild tie;
    "plane" only) adds the three point residuals with that weight, under which a pair without a normal counts too.  The
    dict then gains point_rmse (the RMSE of the distances; `rmse` is that of the minimised residual) and normal_spread,
    both of the last iteration.  `init` is rounded to f32 there, as in align_meshes.

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
    plane, point_weight = _metric_arg(what, metric, point_weight)
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
    if plane:
        return _align_clouds_plane(what, src, gt, init, trims, with_scale, tol, max_iters, check_every, index, normals,
                                   point_weight, _trace)
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


def _direction(queries, points, index, threshold, max_dist, scan=None):
    """The figures of one direction as 0-d f64 device tensors: mean, median, rmse over the valid queries within
    max_dist, the share of the valid queries within threshold, the valid queries beyond max_dist, the valid queries.
    `scan`: the (dist2, nearest) of _distance2 for these arguments, when the caller holds it."""
    dev = queries.device
    dist2 = (_distance2(queries, points, index) if scan is None else scan)[0]
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


def compare_clouds(pred, gt, threshold=0.05, voxel=None, max_dist=None, align=None, align_kw=None, index=None,
                   normals=None, observed=None):
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
    align_clouds(pred, gt, **align_kw) (a local method: pass align_kw=dict(init=...) beyond a modest offset;
    align_kw=dict(metric="plane", point_weight=0.05) is the point-to-plane metric with a mild point tie).  With
    alignment the dict gains `alignment`: T (8 floats), rmse and iterations (None for a given Sim3).

    `index`: None - plain scans, every pair is measured; True - a CloudIndex of each cloud is built; a CloudIndex of
    `gt` (without `voxel`, which makes a new tensor) - that one and a new one of pred.  The dict is the same, value for
    value.

    `normals`: None, or k - cloud_normals(., k) of both clouds after thinning and alignment, and the dict gains
    normal_consistency_accuracy / normal_consistency_completion (the mean of |n_query . n_nearest| over a direction's
    pairs within `max_dist` whose two normals are non-zero; NaN without one), normal_consistency (their mean) and
    n_normal_pairs (the pairs of both directions).

    `observed`: None - every ground-truth point counts; a dict with `poses` (n Sim3s, world from camera), `K` (3,3),
    `hw` and optionally `near`, `far`, `tol`, `rel_tol`, `radius`, `point_size`, `max_radius` (cloud_view.
    observed_cloud_points) and `frame` - only the ground-truth points that some camera sees, the thinned ground-truth
    cloud itself the occluder, enter completion, recall, fscore, chamfer and the completion half of the normal
    consistency (DESIGN.md "Cloud views"); n_gt counts them.  `frame`: "gt" (default) - the poses lie in the ground
    truth's frame; "pred" - in pred's, and the alignment transform moves them first.  `point_size` defaults to
    2 `voxel` (after thinning the spacing is about one voxel and a cell's diagonal is below two); without `voxel`,
    `point_size` and `radius` it raises.  The dict gains gt_observed_share (of the valid ground-truth points) and
    n_gt_observed; ValueError when no point is observed (one more host read).  Accuracy and precision do not change."""
    what = "compare_clouds"
    if normals is not None:
        normals = _k_arg(normals, what, "normals")
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
    gt_all, seen = gt, None
    if observed is not None:
        from .cloud_view import _observed_cloud

        seen = _observed_cloud(what, gt, observed, T, voxel)
        n_all = _valid(gt).sum()
        gt = gt[seen].contiguous()
        n_obs, n_all = int(gt.shape[0]), int(n_all)                              # a host read
        if n_obs == 0:
            raise ValueError(f"{what}: no ground-truth point is observed by the given cameras")
    if normals is None:
        figures = _direction(pred, gt_all, g_index, threshold, limit) + _direction(gt, pred, p_index, threshold, limit)
        consistency = []
    else:
        # the normals' own k-NN is always indexed: the same bits as the plain scan, and not quadratic
        n_pred_, n_gt_ = (cloud_normals(c, normals, index=ix if ix is not None else True)[0]
                          for c, ix in ((pred, p_index), (gt_all, g_index)))
        acc_scan, comp_scan = _distance2(pred, gt_all, g_index), _distance2(gt, pred, p_index)
        figures = (_direction(pred, gt_all, g_index, threshold, limit, acc_scan)
                   + _direction(gt, pred, p_index, threshold, limit, comp_scan))
        consistency = (_normal_consistency(acc_scan, n_pred_, n_gt_, limit)
                       + _normal_consistency(comp_scan, n_gt_ if seen is None else n_gt_[seen], n_pred_, limit))
    (acc, acc_med, acc_rms, prec, acc_out, n_pred, comp, comp_med, comp_rms, rec, comp_out,
     n_gt, *consistency) = torch.stack(figures + consistency).tolist()       # the one host read of the figures
    if n_pred == 0 or n_gt == 0:
        raise ValueError(f"{what}: a cloud has no valid point ({int(n_pred)} in pred, {int(n_gt)} in gt)")
    out = dict(accuracy=acc, accuracy_median=acc_med, accuracy_rmse=acc_rms, completion=comp,
               completion_median=comp_med, completion_rmse=comp_rms, precision=prec, recall=rec,
               **_fscore_chamfer(prec, rec, acc, comp), n_pred=int(n_pred), n_gt=int(n_gt), threshold=threshold, voxel=None if voxel is None else float(voxel),
               max_dist=None if max_dist is None else limit, accuracy_outliers=int(acc_out),
               completion_outliers=int(comp_out))
    if alignment is not None:
        out["alignment"] = alignment
    if observed is not None:
        out.update(gt_observed_share=n_obs / n_all, n_gt_observed=n_obs)
    if normals is not None:
        nc_acc, pairs_acc, nc_comp, pairs_comp = consistency
        out.update(normal_consistency_accuracy=nc_acc, normal_consistency_completion=nc_comp,
                   normal_consistency=0.5 * (nc_acc + nc_comp), n_normal_pairs=int(pairs_acc + pairs_comp))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# k nearest neighbours, normals, outliers (csrc/cloud_knn.hip; the statement is tests/cloud_knn_numpy.py)
# ----------------------------------------------------------------------------------------------------------------------
MAX_K = _m.header_constants()["MSLAM_CLOUD_KNN_MAX_K"]


def _k_arg(k, what, name="k"):
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"{what}: {name} must be an integer in [1, {MAX_K}], got {k!r}")
    return int(k)


def _knn2(queries, points, k, index=None, sort_queries=True, exclude=None, levels=2):
    """(dist2 f64[n,k], neighbors i32[n,k]) of the checked arguments; `exclude`: None or i32[n] on the device."""
    n, N = int(queries.shape[0]), int(points.shape[0])

    def scan(q, ex, dist2, neighbors):
        _m.check(_m.lib().mslam_cloud_knn(_m.ptr(q), n, _m.ptr(points), N, k, _m.ptr(ex), *_index_ops(index, levels), 0,
                                          _m.ptr(dist2), _m.ptr(neighbors), _m.stream_ptr()), "cloud_knn")

    return _sorted_scan(queries, index, sort_queries, ((torch.float64, (k,)), (torch.int32, (k,))), scan, (exclude,))


def _self(points):
    return torch.arange(int(points.shape[0]), dtype=torch.int32, device=points.device)


def cloud_knn(queries, points, k, index=None, sort_queries=True, exclude=None):
    """The k nearest neighbours, 1 <= k <= 32, of the queries f32[n,3] in the cloud `points` f32[N,3] -> (distance
    f64[n,k], neighbors i32[n,k]) device tensors.  Row i holds the k smallest valid points under the total order
    (squared distance, index), ascending - the squared distance is cloud_distance's f64 sum - so a tie goes to the
    lower index; slots beyond the points that qualify hold +inf and -1, and so does the row of a query with a non-finite
    coordinate.  `exclude`: None; i32[n], the point with index exclude[i] is left out of row i (an entry outside [0, N)
    excludes nothing); "self" - `queries` is `points` and every point is left out of its own row.  Exclusion is by
    index: a duplicate of the query at another index stays a neighbour, at distance 0.  `index`, `sort_queries`: as in
    cloud_distance; the same bits in every form, and k = 1 without `exclude` is cloud_distance (DESIGN.md "Point
    clouds")."""
    what = "cloud_knn"
    k = _k_arg(k, what)
    same = queries is points or (torch.is_tensor(queries) and torch.is_tensor(points)
                                 and queries.shape == points.shape and queries.data_ptr() == points.data_ptr())
    queries = _points_arg(queries, "queries", what)
    index = _index_arg(CloudIndex, index, what, points)
    points = _points_arg(points, "points", what)
    if queries.device != points.device:
        raise ValueError(f"{what}: queries and points are on different devices")
    if isinstance(exclude, str):
        if exclude != "self" or not same:
            raise ValueError(f"{what}: exclude='self' needs queries to be the points tensor itself")
        exclude = _self(points)
    elif exclude is not None:
        if not torch.is_tensor(exclude) or tuple(exclude.shape) != (int(queries.shape[0]),):
            raise ValueError(f"{what}: exclude must be None, 'self' or an i32[{int(queries.shape[0])}] device tensor")
        _m.require_dtype(exclude, torch.int32, "exclude")
        _m.ptr(exclude)
        if exclude.device != points.device:
            raise ValueError(f"{what}: exclude and points are on different devices")
        exclude = exclude.contiguous()
    dist2, neighbors = _knn2(queries, points, k, index, sort_queries, exclude)
    return torch.sqrt(dist2), neighbors


def _normals(points, neighbors, k, viewpoint, what):
    """mslam_cloud_normals of the checked points and their neighbour rows -> (normals, curvature, count)."""
    N, dev = int(points.shape[0]), points.device
    vp, stride = None, 0
    if viewpoint is not None:
        vp = viewpoint if torch.is_tensor(viewpoint) else torch.as_tensor(np.asarray(viewpoint, np.float32))
        vp = vp.detach().to(device=dev, dtype=torch.float32).contiguous()
        if tuple(vp.shape) == (N, 3) and N != 1:
            stride = 3
        elif vp.numel() == 3:
            vp = vp.reshape(3)
        else:
            raise ValueError(f"{what}: viewpoint must be 3 numbers or ({N},3), got {tuple(vp.shape)}")
    normals = torch.empty((N, 3), dtype=torch.float32, device=dev)
    curvature = torch.empty(N, dtype=torch.float32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    _m.check(_m.lib().mslam_cloud_normals(_m.ptr(points), N, _m.ptr(neighbors), k, _m.ptr(vp), stride, _m.ptr(normals),
                                          _m.ptr(curvature), _m.ptr(count), 0, _m.stream_ptr()), "cloud_normals")
    return normals, curvature, count


def cloud_normals(points, k=16, viewpoint=None, index=True):
    """A normal per point of the cloud `points` f32[N,3] from its k nearest neighbours in the cloud, itself included
    (cloud_knn without exclusion) -> (normals f32[N,3], curvature f32[N], count i32[N]) device tensors.  The normal is
    the unit eigenvector of the smallest eigenvalue of the neighbourhood's covariance (f64, cyclic Jacobi), the
    curvature the surface variation l_min / (l0 + l1 + l2), the count the neighbours found.  Fewer than 3 neighbours,
    coincident or collinear ones (the middle eigenvalue <= 2^-40 of the largest) and an invalid point: the normal is
    (0, 0, 0) and the curvature NaN.  `viewpoint`: 3 numbers, or f32[N,3] with one per point - the normal is turned
    towards it (not when exactly perpendicular); None - turned so that its largest component is positive.  `index`:
    None, True or a CloudIndex of the tensor; the same bits (DESIGN.md "Point clouds")."""
    what = "cloud_normals"
    k = _k_arg(k, what)
    index = _index_arg(CloudIndex, index, what, points)
    points = _points_arg(points, "points", what)
    neighbors = _knn2(points, points, k, index)[1]
    return _normals(points, neighbors, k, viewpoint, what)


def cloud_outliers(points, k=16, std_ratio=2.0, radius=None, min_neighbors=None, index=True):
    """Which points of the cloud `points` f32[N,3] to keep -> (keep bool[N] device tensor, dict).

    The statistical rule (Open3D's and PCL's; `std_ratio` None: off): mean_i is the mean distance from point i to its k
    nearest neighbours other than itself (cloud_knn with exclude="self"; the sum in list order over the m_i found,
    divided by m_i; a valid point with m_i >= 1), mu and sigma the mean and the SAMPLE standard deviation (divisor
    M - 1; 0 when M < 2) of the mean_i over those M points, in f64 on the device; a point is kept when mean_i <= mu +
    std_ratio * sigma.  The radius rule (`radius` and `min_neighbors` <= 32 together): a point is kept when its
    min_neighbors-th neighbour lies within `radius` (squared distance <= radius^2 in f64).  With both, both must hold;
    an invalid point is never kept.  The dict: mu, sigma, threshold (NaN without the statistical rule), kept, n_valid -
    one host read - and mean_distance f64[N] (a device tensor; NaN where undefined; None without the rule)."""
    what = "cloud_outliers"
    if (radius is None) != (min_neighbors is None):
        raise ValueError(f"{what}: radius and min_neighbors go together")
    if std_ratio is None and radius is None:
        raise ValueError(f"{what}: no rule: give std_ratio, or radius and min_neighbors")
    if std_ratio is not None and not float(std_ratio) >= 0.0:
        raise ValueError(f"{what}: std_ratio must be >= 0, got {std_ratio}")
    if radius is not None and not float(radius) >= 0.0:
        raise ValueError(f"{what}: radius must be >= 0, got {radius}")
    index = _index_arg(CloudIndex, index, what, points)
    points = _points_arg(points, "points", what)
    N, dev = int(points.shape[0]), points.device
    ok = _valid(points)
    keep = ok.clone()
    nan = torch.full((), math.nan, dtype=torch.float64, device=dev)
    mu = sigma = thr = nan
    mean = None
    if std_ratio is not None:
        k = _k_arg(k, what)
        dist2, nb = _knn2(points, points, k, index, exclude=_self(points))
        d, has = torch.sqrt(dist2), nb >= 0
        total = torch.zeros(N, dtype=torch.float64, device=dev)
        for j in range(k):                                                   # the sum in list order
            total = total + torch.where(has[:, j], d[:, j], torch.zeros_like(total))
        m = has.sum(1)
        scored = ok & (m >= 1)
        mean = torch.where(scored, total / m.to(torch.float64), nan)
        M = scored.sum().to(torch.float64)
        zero = torch.zeros_like(total)
        mu = torch.where(scored, mean, zero).sum() / M
        dev2 = torch.where(scored, (mean - mu) * (mean - mu), zero).sum()
        sigma = torch.where(M >= 2.0, torch.sqrt(dev2 / (M - 1.0)), torch.zeros_like(mu))
        thr = mu + float(std_ratio) * sigma
        keep &= scored & (mean <= thr)
    if radius is not None:
        mn = _k_arg(min_neighbors, what, "min_neighbors")
        r2 = _knn2(points, points, mn, index, exclude=_self(points))[0][:, mn - 1]
        keep &= r2 <= float(radius) * float(radius)
    mu_, sigma_, thr_, kept, n_valid = torch.stack(
        [mu, sigma, thr, keep.sum().to(torch.float64), ok.sum().to(torch.float64)]).tolist()      # the host read
    return keep, dict(mu=mu_, sigma=sigma_, threshold=thr_, kept=int(kept), n_valid=int(n_valid), mean_distance=mean)


def filter_cloud(points, colors=None, **outlier_kw):
    """The cloud without the points cloud_outliers(points, **outlier_kw) drops, in the original order -> (points
    f32[M,3], colors u8[M,3] or None, kept_indices i64[M])."""
    keep = cloud_outliers(points, **outlier_kw)[0]
    if colors is not None:
        colors = _colors_arg(colors, int(points.shape[0]), "filter_cloud")
    idx = torch.nonzero(keep).reshape(-1)
    return points[idx].contiguous(), None if colors is None else colors[idx].contiguous(), idx


def _normal_consistency(scan, n_query, n_points, max_dist):
    """[mean of |n_query . n_nearest| over the pairs within max_dist whose two normals are non-zero (NaN without one),
    the pairs] as 0-d f64 device tensors, from the (dist2, nearest) of one direction."""
    dist2, nearest = scan
    j = nearest.clamp_min(0).long()
    a, b = n_query.to(torch.float64), n_points.to(torch.float64)[j] if int(n_points.shape[0]) else torch.zeros_like(
        n_query, dtype=torch.float64)
    pair = (nearest >= 0) & (torch.sqrt(dist2) <= max_dist) & (a != 0.0).any(1) & (b != 0.0).any(1)
    dot = torch.abs((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2])
    pairs = pair.sum().to(torch.float64)
    return [torch.where(pair, dot, torch.zeros_like(dot)).sum() / pairs, pairs]
