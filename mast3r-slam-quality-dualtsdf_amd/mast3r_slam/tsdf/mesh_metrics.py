"""Mesh quality on the device: face areas, an area-weighted stratified surface sampler, the exact distance from points
to a triangle mesh, and the accuracy / completion / precision / recall / F-score / Chamfer figures between two meshes.

No counterpart in the reference.  The kernels are csrc/mesh_distance.hip (DESIGN.md "Mesh quality"); the numpy
statement of the same definitions is tests/meshdist_numpy.py.  A face is valid when its indices lie in [0, V) and its
cross product is not exactly zero; an invalid face has area 0, is never sampled and is never the nearest face.  The two
meshes of a comparison must lie in one frame; compare_meshes(align=...) moves the first into the second's frame first
(mesh_align.py, DESIGN.md "Mesh alignment"), and compare_meshes(observed=...) scores completion and recall over the part
of the second that given cameras see (mesh_raycast.py, DESIGN.md "Mesh ray casting").
"""
import torch

import mslam_hip as _m

from ._mesh_args import _areas, _mesh_arg, _pair, _points_arg, _sample
from .mesh_align import _alignment_arg, align_meshes, transform_mesh
from .mesh_index import _NEAREST, MeshIndex, _index_arg, _index_ops, _sorted_scan


def face_areas(vertices, faces, _validate=True):
    """area f64[F] = 0.5 |(b - a) x (c - a)| of the faces i32[F,3] over vertices f32[V,3] (device tensors), in f64."""
    vertices, faces, V, F = _mesh_arg(vertices, faces, _validate, "face_areas")
    return _areas(vertices, faces, V, F)


def sample_mesh(vertices, faces, n, seed=0, _validate=True):
    """n points on the mesh, area-weighted -> (points f32[n,3], face i32[n]) device tensors.  Stratified: sample i sits
    at (i + 0.5) / n of the cumulative area, so every face gets its share of the samples to within one, in face order;
    the place inside the face comes from a stateless hash of (seed, i).  The same inputs give the same bits.  Raises
    ValueError when n < 1 or the mesh has no area."""
    vertices, faces, V, F = _mesh_arg(vertices, faces, _validate, "sample_mesh")
    return _sample(vertices, faces, V, F, n, seed, "sample_mesh")[:2]


def _distance2(points, vertices, faces, V, F, skip, index=None, sort_queries=True):
    """(dist2 f64[n], nearest i32[n]).  `index`: a MeshIndex of this mesh - the scan runs over its tiles, and with
    `sort_queries` on the points in the order of their Morton keys, the results scattered back."""
    L, n = _m.lib(), int(points.shape[0])
    ws_bytes = int(L.mslam_mesh_distance_workspace_bytes(F)) if index is None and skip and F else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=points.device) if ws_bytes else None

    def scan(pts, dist2, nearest):
        if index is not None:
            _m.check(L.mslam_mesh_distance_indexed(_m.ptr(pts), n, _m.ptr(vertices), _m.ptr(faces), F, V,
                                                   *_index_ops(index), 0, _m.ptr(dist2), _m.ptr(nearest),
                                                   _m.stream_ptr()), "mesh_distance_indexed")
        else:
            _m.check(L.mslam_mesh_distance(_m.ptr(pts), n, _m.ptr(vertices), _m.ptr(faces), F, V, 1 if ws_bytes else 0,
                                           _m.ptr(ws), ws_bytes, _m.ptr(dist2), _m.ptr(nearest), _m.stream_ptr()),
                     "mesh_distance")

    return _sorted_scan(points, index, sort_queries, _NEAREST, scan)


def _fscore_chamfer(precision, recall, accuracy, completion):
    """The two figures compare_meshes and compare_clouds derive from the other four, as dict entries: the harmonic mean
    of precision and recall (0 when both are 0) and the mean of accuracy and completion."""
    return dict(fscore=2.0 * precision * recall / (precision + recall) if precision + recall > 0.0 else 0.0,
                chamfer=0.5 * (accuracy + completion))


def mesh_distance(points, vertices, faces, skip=True, _validate=True, index=None, sort_queries=True):
    """Exact distance from points f32[n,3] to the mesh -> (distance f64[n], nearest i32[n]) device tensors: the distance
    to the closest point of the closest valid face and the lowest index of a face at that distance; +inf and -1 when
    the mesh has no valid face.  `skip`: tiles of faces whose bounding box lies beyond a point block's current best are
    not scanned; the output is the same bit for bit (DESIGN.md "Mesh quality").  `index`: None - that path; True - a
    MeshIndex of the mesh is built first; a MeshIndex built for these tensors - the scan runs over its Morton-ordered
    tiles and group boxes, and with `sort_queries` the points are scanned in the order of their Morton keys and the
    results scattered back; the same bits again, for faces in any order (DESIGN.md "Mesh index")."""
    points = _points_arg(points, "points", "mesh_distance")
    index = _index_arg(MeshIndex, index, "mesh_distance", vertices, faces)
    vertices, faces, V, F = _mesh_arg(vertices, faces, _validate, "mesh_distance")
    if points.device != vertices.device:
        raise ValueError("mesh_distance: points and mesh are on different devices")
    dist2, nearest = _distance2(points, vertices, faces, V, F, bool(skip), index, sort_queries)
    return torch.sqrt(dist2), nearest


def compare_meshes(pred, gt, n_samples=200_000, threshold=0.05, seed=0, skip=True, _validate_pred=True, align=None,
                   align_kw=None, observed=None, index=None):
    """Quality of the mesh `pred` against the ground truth `gt`, both (vertices f32[V,3], faces i32[F,3]) device tensors
    or the tuples extract_mesh returns (normals and colours are ignored), in one frame.  n_samples points are drawn on
    each (sample_mesh with `seed` on pred, `seed + 1` on gt) and measured against the other (mesh_distance).  Returns
    Python numbers: accuracy / accuracy_median (pred samples to gt, mean and median), completion / completion_median
    (gt samples to pred), precision / recall (share of pred / gt samples within `threshold`), fscore (their harmonic
    mean, 0 when both are 0), chamfer = (accuracy + completion) / 2, n_samples, threshold, pred_area, gt_area.  The
    means are f64 sums.  Host reads: the index range of each mesh, each total area, and the figures at the end.

    `align`: None - the meshes are taken as they are; a Sim3 ([t(3), q(xyzw), s], 8 numbers) - pred is moved by it first
    (transform_mesh); "icp" - pred is moved by align_meshes(pred, gt, **align_kw) first (a local method: pass
    align_kw=dict(init=...) for more than a modest offset; dict(metric="plane") is the point-to-plane metric).  With alignment the dict gains `alignment`: T (a list of 8
    floats), rmse and iterations (None for a given Sim3).

    `observed`: None - every ground-truth sample counts; a dict with `poses` (n Sim3s, world from camera), `K` (3,3),
    `hw` and optionally `near`, `far`, `tol` (observed_points) and `frame` - only the ground-truth samples that some
    camera sees, occlusion against the ground-truth mesh included, enter completion, completion_median, recall, fscore
    and chamfer (DESIGN.md "Mesh ray casting").  `frame`: "gt" (default) - the poses lie in the ground truth's frame;
    "pred" - in pred's, and the alignment transform moves them first.  The dict gains gt_observed_share and
    n_gt_observed; ValueError when no sample is observed.  Accuracy and precision do not change.

    `index`: None, True or a MeshIndex of `gt` (DESIGN.md "Mesh index"): the alignment, the distances to gt and the
    observed-part cull run over it, so their speed does not depend on the order of gt's faces.  The dict is the same,
    value for value."""
    n = int(n_samples)
    index = _index_arg(MeshIndex, index, "compare_meshes", *_pair(gt, "gt"))
    threshold = float(threshold)
    T, alignment = _alignment_arg("compare_meshes", align, align_kw,
                                  lambda **kw: align_meshes(_pair(pred, "pred"), gt, index=index, **kw))
    if T is not None:
        pvert, pfaces = _pair(pred, "pred")
        pred = (transform_mesh(pvert, T), pfaces)
    pv, pf, pV, pF = _mesh_arg(*_pair(pred, "pred"), _validate_pred, "compare_meshes")
    gv, gf, gV, gF = _mesh_arg(*_pair(gt, "gt"), True, "compare_meshes")
    p_pts, _, p_area = _sample(pv, pf, pV, pF, n, seed, "compare_meshes (pred)")
    g_pts, _, g_area = _sample(gv, gf, gV, gF, n, int(seed) + 1, "compare_meshes (gt)")
    n_obs = n
    if observed is not None:
        seen = _observed_samples(g_pts, _pair(gt, "gt") if index is not None else (gv, gf), observed,
                                 T, bool(skip), index)
        g_pts = g_pts[seen]
        n_obs = int(g_pts.shape[0])                                               # a host read
        if n_obs == 0:
            raise ValueError("compare_meshes: no ground-truth sample is observed by the given cameras")
    out = []
    for pts, m, (v, f, V, F), ix in ((p_pts, n, (gv, gf, gV, gF), index), (g_pts, n_obs, (pv, pf, pV, pF), None)):
        d = torch.sqrt(_distance2(pts, v, f, V, F, bool(skip), ix)[0])
        s = torch.sort(d)[0]
        out += [d.sum() / m, 0.5 * (s[(m - 1) // 2] + s[m // 2]), (d <= threshold).sum().to(torch.float64) / m]
    acc, acc_med, prec, comp, comp_med, rec = torch.stack(out).tolist()          # the one host read of the figures
    out = dict(accuracy=acc, accuracy_median=acc_med, completion=comp, completion_median=comp_med, precision=prec,
               recall=rec, **_fscore_chamfer(prec, rec, acc, comp), n_samples=n, threshold=threshold, pred_area=p_area,
               gt_area=g_area)
    if alignment is not None:
        out["alignment"] = alignment
    if observed is not None:
        out.update(gt_observed_share=n_obs / n, n_gt_observed=n_obs)
    return out


def _observed_samples(g_pts, gt, observed, T, skip, index=None):
    """bool[n]: the ground-truth samples the cameras of `observed` see; T: the alignment transform or None."""
    from ._view_args import _poses_arg, compose_sim3
    from .mesh_raycast import observed_points

    spec = dict(observed)
    unknown = set(spec) - {"poses", "K", "hw", "near", "far", "tol", "frame"}
    if unknown or not {"poses", "K", "hw"} <= set(spec):
        raise ValueError(f"compare_meshes: observed needs poses, K and hw (and takes near, far, tol, frame); got "
                         f"{sorted(spec)}")
    frame = spec.pop("frame", "gt")
    if frame not in ("gt", "pred"):
        raise ValueError(f"compare_meshes: observed['frame'] must be 'gt' or 'pred', got {frame!r}")
    poses = _poses_arg(spec.pop("poses"), "compare_meshes")
    if frame == "pred" and T is not None:
        poses = compose_sim3(T, poses)
    return observed_points(g_pts, gt, poses, spec.pop("K"), spec.pop("hw"), skip=skip, index=index, **spec)
