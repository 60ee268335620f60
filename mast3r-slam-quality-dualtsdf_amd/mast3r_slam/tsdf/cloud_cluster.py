"""Density clusters of a point cloud on the device: how many points lie within a radius of a point, DBSCAN labels, and
the filter that drops whole clusters - the small dense blobs hanging in the air ("floaters") that have neighbours enough
to pass the point-wise rules of cloud_outliers.

No counterpart in the reference.  The kernels are csrc/cloud_cluster.hip (DESIGN.md "Cloud clusters"); the numpy
statement of the same definitions is tests/cloud_cluster_numpy.py.  A cloud is points f32[N,3]; a point is valid when
its three coordinates are finite.  The squared distance is cloud_distance's f64 sum, "within" means <= radius^2, and a
point counts itself and its duplicates.
"""
import math

import torch

import mslam_hip as _m

from ._mesh_args import _points_arg
from .cloud import CloudIndex, _colors_arg, _valid
from .mesh_index import _index_arg, _index_ops, _sorted_scan


def _radius_count(queries, points, eps2, index=None, sort_queries=True, levels=2):
    """count i32[n] of the checked arguments."""
    n, N = int(queries.shape[0]), int(points.shape[0])

    def scan(q, count):
        _m.check(_m.lib().mslam_cloud_radius_count(_m.ptr(q), n, _m.ptr(points), N, eps2, *_index_ops(index, levels), 0,
                                                   _m.ptr(count), _m.stream_ptr()), "cloud_radius_count")

    return _sorted_scan(queries, index, sort_queries, ((torch.int32, ()),), scan)[0]


def cloud_radius_count(queries, points, radius, index=None, sort_queries=True):
    """How many valid points of the cloud `points` f32[N,3] lie within `radius` of each of the queries f32[n,3] ->
    count i32[n], a device tensor: the points with squared distance <= float(radius)^2 in f64, the squared distance
    cloud_distance's sum.  A point of the cloud counts itself and its duplicates; the count is not capped; 0 for a query
    with a non-finite coordinate.  `radius` is finite and >= 0.  `index`, `sort_queries`: as in cloud_distance - None
    is the plain scan, with an index tiles and groups whose boxes lie beyond the radius are not scanned; the same bytes
    in every form (DESIGN.md "Cloud clusters")."""
    what = "cloud_radius_count"
    if not (float(radius) >= 0.0 and math.isfinite(float(radius))):
        raise ValueError(f"{what}: radius must be finite and >= 0, got {radius}")
    queries = _points_arg(queries, "queries", what)
    index = _index_arg(CloudIndex, index, what, points)
    points = _points_arg(points, "points", what)
    if queries.device != points.device:
        raise ValueError(f"{what}: queries and points are on different devices")
    return _radius_count(queries, points, float(radius) * float(radius), index, sort_queries)


def _link(points, eps2, core, index):
    """The link launch, the flatten and the labels of the checked arguments -> (label_root i32[N], is_root bool[N]).
    With an index the rows follow its order, so a block's queries are its home tiles."""
    N, dev = int(points.shape[0]), points.device
    L, st = _m.lib(), _m.stream_ptr()
    parent = torch.empty(N, dtype=torch.int32, device=dev)
    rows_anchor = torch.empty(N, dtype=torch.int32, device=dev)
    dist2 = torch.empty(N, dtype=torch.float64, device=dev)
    _m.check(L.mslam_cloud_cluster_init(N, _m.ptr(parent), st), "cloud_cluster_init")
    rows = None if index is None else index.order
    _m.check(L.mslam_cloud_cluster_link(_m.ptr(points), N, _m.ptr(rows), N, eps2, _m.ptr(core), *_index_ops(index), 0,
                                        _m.ptr(parent), _m.ptr(rows_anchor), _m.ptr(dist2), st), "cloud_cluster_link")
    # the order names every point once: the rows back in point order
    anchor = rows_anchor if rows is None else torch.empty_like(rows_anchor).index_copy_(0, rows.long(), rows_anchor)
    _m.check(L.mslam_cloud_cluster_flatten(N, _m.ptr(parent), st), "cloud_cluster_flatten")
    label_root = torch.empty(N, dtype=torch.int32, device=dev)
    is_root = torch.empty(N, dtype=torch.uint8, device=dev)
    _m.check(L.mslam_cloud_cluster_labels(_m.ptr(parent), _m.ptr(core), _m.ptr(anchor), N, _m.ptr(label_root),
                                          _m.ptr(is_root), st), "cloud_cluster_labels")
    return label_root, is_root.bool()


def _cluster_args(what, eps, min_points):
    if not (float(eps) > 0.0 and math.isfinite(float(eps))):
        raise ValueError(f"{what}: eps must be positive and finite, got {eps}")
    if isinstance(min_points, bool) or int(min_points) != min_points or int(min_points) < 1:
        raise ValueError(f"{what}: min_points must be an integer >= 1, got {min_points!r}")
    return float(eps) * float(eps), int(min_points)


def cloud_clusters(points, eps, min_points=10, index=True):
    """DBSCAN of the cloud `points` f32[N,3] -> (labels i32[N], info), device tensors.

    A point is a CORE point when it is valid and at least `min_points` valid points of the cloud, itself and its
    duplicates included, lie within `eps` of it (cloud_radius_count).  A cluster is a connected component of the graph
    on the core points with an edge between two within `eps`; a path through a point that is not core joins nothing.
    A valid point that is not core but has a core point within `eps` is a BORDER point and belongs to the cluster of its
    anchor, the core point smallest under the total order (squared distance, index).  Textbook DBSCAN hands a border
    point to whichever cluster reaches it first, which depends on the order of the visit; here the labels are a
    function of the cloud alone, the same bytes on every call and with every `index`.  Every other point, and every
    invalid one, is noise: label -1.  Clusters are numbered 0..C-1 in ascending order of their smallest point index.

    `eps` is positive and finite, `min_points` an integer >= 1 with no upper limit.  `index`: None, True or a
    CloudIndex of the tensor.  info: n_clusters, n_noise, n_core (Python ints, one host read), sizes i32[C] (core and
    border members), core bool[N] and count i32[N] (device tensors).  An empty cloud and a cloud without a valid point
    give labels of -1 and no cluster."""
    what = "cloud_clusters"
    eps2, min_points = _cluster_args(what, eps, min_points)
    index = _index_arg(CloudIndex, index, what, points)
    points = _points_arg(points, "points", what)
    N, dev = int(points.shape[0]), points.device
    if N == 0:
        empty = torch.zeros(0, dtype=torch.int32, device=dev)
        return empty, dict(n_clusters=0, n_noise=0, n_core=0, sizes=empty.clone(), core=empty.bool(),
                           count=empty.clone())
    count = _radius_count(points, points, eps2, index)
    core = _valid(points) & (count >= min_points)
    label_root, is_root = _link(points, eps2, core.to(torch.uint8), index)
    dense = (torch.cumsum(is_root, 0) - 1).to(torch.int32)              # cluster id, valid at the roots
    member = label_root >= 0
    labels = torch.where(member, dense[label_root.clamp_min(0).long()], -1).to(torch.int32)
    n_clusters, n_noise, n_core = torch.stack([is_root.sum(), (~member).sum(), core.sum()]).tolist()   # the host read
    # integer adds into the cluster's slot, noise into a slot past the end
    sizes = torch.zeros(n_clusters + 1, dtype=torch.int32, device=dev)
    sizes.scatter_add_(0, torch.where(member, labels, n_clusters).long(), torch.ones(N, dtype=torch.int32, device=dev))
    return labels, dict(n_clusters=n_clusters, n_noise=n_noise, n_core=n_core, sizes=sizes[:n_clusters].contiguous(),
                        core=core, count=count)


def filter_cloud_clusters(points, colors=None, eps=None, min_points=10, min_cluster_points=0, keep_largest=None,
                          keep_noise=False, index=True):
    """The cloud without the clusters that are too small, in the original order -> (points f32[M,3], colors u8[M,3] or
    None, kept_indices i64[M]).  cloud_clusters(points, eps, min_points, index) first; then filter_mesh's rule: the
    clusters with at least `min_cluster_points` members (core and border) stay, and of those only the `keep_largest`
    largest when that is given, ties going to the lower label (a stable descending sort).  Noise leaves the cloud unless
    `keep_noise`, which keeps the valid points of label -1; an invalid point is never kept."""
    what = "filter_cloud_clusters"
    if eps is None:
        raise ValueError(f"{what}: eps must be given")
    if keep_largest is not None and int(keep_largest) < 0:
        raise ValueError(f"{what}: keep_largest must be >= 0")
    _points_arg(points, "points", what)
    if colors is not None:
        colors = _colors_arg(colors, int(points.shape[0]), what)
    labels, info = cloud_clusters(points, eps, min_points, index)
    sizes, dev = info["sizes"], labels.device
    keep = sizes >= int(min_cluster_points)
    if keep_largest is not None:
        # stable descending sort: among equal sizes the lower label comes first
        order = torch.sort(torch.where(keep, sizes, -1), stable=True, descending=True)[1][:int(keep_largest)]
        top = torch.zeros_like(keep)
        top[order] = True
        keep = keep & top
    keep = torch.cat([keep, torch.zeros(1, dtype=torch.bool, device=dev)])          # the slot of label -1
    kept = keep[torch.where(labels >= 0, labels, int(sizes.shape[0])).long()]
    if keep_noise:
        kept = kept | ((labels < 0) & _valid(points))
    idx = torch.nonzero(kept).reshape(-1)
    return points[idx].contiguous(), None if colors is None else colors[idx].contiguous(), idx
