"""Mesh alignment on the device: the closed-form similarity (Sim3) between corresponding points and trimmed
point-to-mesh ICP, so that a monocular map - defined only up to a similarity - can be scored against a ground-truth mesh
that lies in another frame.

No counterpart in the reference.  The kernels are csrc/mesh_align.hip (DESIGN.md "Mesh alignment"); the numpy statement
of the same definitions is tests/meshalign_numpy.py.  A Sim3 is lietorch's [t(3), q(xyzw), s] and acts as s R(q) p + t.
"""
import math

import numpy as np
import torch

import mslam_hip as _m

from ._mesh_args import _mesh_arg, _pair, _points_arg, _sample, _sim3_arg
from .mesh_index import MeshIndex, _index_arg, _index_ops

STATE_BYTES, LOG_DOUBLES, OK, DEGENERATE = (_m.header_constants()["MSLAM_MESH_ALIGN_" + k] for k in (
    "STATE_BYTES", "LOG_DOUBLES", "OK", "DEGENERATE"))


def _read_state(state):
    """(T f64[8], T32 f32[8], status i32[1]) device tensors of a state block."""
    dev = state.device
    T64 = torch.empty(8, dtype=torch.float64, device=dev)
    T32 = torch.empty(8, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _m.check(_m.lib().mslam_mesh_align_read(_m.ptr(state), _m.ptr(T64), _m.ptr(T32), _m.ptr(status), _m.stream_ptr()),
             "mesh_align_read")
    return T64, T32, status


def fit_sim3(src, dst, weights=None, with_scale=True):
    """The similarity that moves the points src f32[n,3] onto dst f32[n,3] (device tensors) in the weighted least-squares
    sense (Umeyama; the rotation by Horn's quaternion method, always a proper rotation, defined for coplanar points)
    -> (T f64[8], T32 f32[8]) device tensors in lietorch layout.  `weights` f32[n] >= 0, a pair of weight 0 does not
    count; `with_scale=False` fixes the scale at 1.  Raises ValueError when the problem is degenerate: fewer than 3
    pairs that count, no spread among the source points, or no positive scale.  One host read: the status."""
    src = _points_arg(src, "src", "fit_sim3")
    dst = _points_arg(dst, "dst", "fit_sim3")
    if src.shape != dst.shape:
        raise ValueError(f"fit_sim3: src {tuple(src.shape)} and dst {tuple(dst.shape)} differ in shape")
    if src.device != dst.device:
        raise ValueError("fit_sim3: src and dst are on different devices")
    n, dev = int(src.shape[0]), src.device
    if weights is not None:
        if not torch.is_tensor(weights):
            raise TypeError("fit_sim3: weights must be a device tensor")
        if tuple(weights.shape) != (n,):
            raise ValueError(f"fit_sim3: weights must be ({n},), got {tuple(weights.shape)}")
        _m.require_dtype(weights, torch.float32, "weights")
        _m.ptr(weights)
        if weights.device != dev:
            raise ValueError("fit_sim3: weights are on another device")
        weights = weights.contiguous()
    L = _m.lib()
    ws_bytes = int(L.mslam_mesh_align_workspace_bytes(n, 0, 0))
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    state = torch.empty(STATE_BYTES, dtype=torch.uint8, device=dev)
    log = torch.empty(LOG_DOUBLES, dtype=torch.float64, device=dev)
    _m.check(L.mslam_mesh_align_fit_pairs(_m.ptr(src), _m.ptr(dst), _m.ptr(weights), n, 1 if with_scale else 0,
                                          _m.ptr(ws), ws_bytes, _m.ptr(state), _m.ptr(log), _m.stream_ptr()),
             "mesh_align_fit_pairs")
    T64, T32, status = _read_state(state)
    if int(status) != OK:
        raise ValueError(f"fit_sim3: degenerate problem ({n} pairs): fewer than 3 pairs that count, no spread among "
                         "the source points, or no positive scale")
    return T64, T32


# not merged with cloud.transform_cloud: that one is an elementwise f64 sum in a stated order, this one a matmul, they
# round differently and tests pin the bits of each
def transform_mesh(vertices, T, normals=None):
    """The vertices f32[V,3] moved by the Sim3 T (s R v + t, in f64, stored f32) and, when given, the normals rotated
    (R n): torch ops on the vertices' device.  Returns the vertices, or (vertices, normals)."""
    if not torch.is_tensor(vertices):
        raise TypeError("transform_mesh: vertices must be a tensor")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"transform_mesh: vertices must be (V,3), got {tuple(vertices.shape)}")
    T = _sim3_arg(T, "transform_mesh", vertices.device, torch.float64)
    x, y, z, w = T[3:7] / torch.linalg.vector_norm(T[3:7])
    R = torch.stack([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w),
                     2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w),
                     2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]).reshape(3, 3)
    moved = (T[7] * (vertices.to(torch.float64) @ R.T) + T[:3]).to(vertices.dtype)
    if normals is None:
        return moved
    return moved, (normals.to(torch.float64) @ R.T).to(normals.dtype)


def _icp_args(what, max_iters, check_every, tol, trim):
    """(max_iters, check_every, trims) of align_meshes' and align_clouds' loop arguments, checked; trims: one float
    per iteration."""
    max_iters, check_every = int(max_iters), int(check_every)
    if max_iters < 1 or check_every < 1:
        raise ValueError(f"{what}: max_iters and check_every must be >= 1, got {max_iters} and {check_every}")
    if not float(tol) >= 0.0:
        raise ValueError(f"{what}: tol must be >= 0, got {tol}")
    trims = [float(t) for t in trim] if isinstance(trim, (list, tuple, np.ndarray)) else [float(trim)] * max_iters
    if len(trims) != max_iters:
        raise ValueError(f"{what}: a trim sequence needs one value per iteration ({max_iters}), got {len(trims)}")
    if not all(t >= 0.0 for t in trims):
        raise ValueError(f"{what}: trim must be >= 0 (+inf keeps every pair)")
    return max_iters, check_every, trims


def _icp_run(step, log, max_iters, check_every, tol):
    """The ICP loop and its stop rule -> (iterations, converged, history).  step(it) runs iteration `it` and leaves its
    (inliers, rmse, scale, status) in log[it, :4], a tensor of max_iters rows.  The log is read every `check_every`
    iterations and after the last; at a read the loop stops when the latest status is not OK, or, from the second
    iteration on, when the RMSE of the last two iterations differs by at most `tol` relative.  So `iterations` is a
    multiple of check_every or max_iters, and history (numpy f64[iterations, 4]) is the log up to there."""
    converged, hist, it = False, None, 0
    for it in range(max_iters):
        step(it)
        if (it + 1) % check_every == 0 or it + 1 == max_iters:
            hist = log[:it + 1, :4].cpu().numpy()                      # the one host read of this stretch
            if hist[it, 3] != OK:
                break
            if it >= 1 and abs(hist[it, 1] - hist[it - 1, 1]) <= float(tol) * hist[it - 1, 1]:
                converged = True
                break
    return it + 1, converged, hist


PLANE_LOG_DOUBLES = _m.header_constants()["MSLAM_ICP_PLANE_LOG_DOUBLES"]


def _metric_arg(what, metric, point_weight):
    """(plane, point_weight) of align_meshes' and align_clouds' `metric` and `point_weight`, checked."""
    if metric not in ("point", "plane"):
        raise ValueError(f"{what}: metric must be 'point' or 'plane', got {metric!r}")
    w = float(point_weight)
    if not (w >= 0.0 and math.isfinite(w)):
        raise ValueError(f"{what}: point_weight must be finite and >= 0, got {point_weight}")
    if metric == "point" and w != 0.0:
        raise ValueError(f"{what}: point_weight goes with metric='plane' only")
    return metric == "plane", w


def _icp_setup(dev, ws_bytes, T0, boxed=None):
    """(ws, state) of a loop over a state block: the workspace, and the state set to T0 f32[8] (None: the identity).
    `boxed`: the (vertices, faces, F, V) of a target mesh scanned without an index - the boxes of its tiles are built at
    the head of the workspace."""
    L, st = _m.lib(), _m.stream_ptr()
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    state = torch.empty(STATE_BYTES, dtype=torch.uint8, device=dev)
    if boxed is None:
        _m.check(L.mslam_mesh_align_init_indexed(_m.ptr(T0), _m.ptr(state), st), "mesh_align_init_indexed")
    else:
        gv, gf, gF, gV = boxed
        _m.check(L.mslam_mesh_align_init(_m.ptr(T0), _m.ptr(gv), _m.ptr(gf), gF, gV, _m.ptr(ws), ws_bytes,
                                         _m.ptr(state), st), "mesh_align_init")
    return ws, state


def _state_run(src, state, launch, plane, max_iters, check_every, tol, trace):
    """The loop of both metrics over an initialised state block (csrc/mesh_align.hip, csrc/icp_plane.hip) -> the dict
    align_meshes and align_clouds return.  launch(it, nearest, moved, dist2, closest, log_row) runs the step of
    iteration `it`; `closest` is 0 unless the plane metric is traced.  `plane`: the log rows are the plane metric's, and
    beside _icp_run's reads there is one more at the end, the last row's point rmse and normal_spread."""
    n, dev = int(src.shape[0]), src.device
    log = torch.zeros((max_iters, PLANE_LOG_DOUBLES if plane else LOG_DOUBLES), dtype=torch.float64, device=dev)
    nearest = torch.full((n,), -1, dtype=torch.int32, device=dev)
    moved = torch.empty((n, 3), dtype=torch.float32, device=dev)
    dist2 = torch.empty(n, dtype=torch.float64, device=dev)

    def step(it):
        if trace is None or not plane:
            launch(it, nearest, moved, dist2, 0, _m.ptr(log[it]))
            if trace is not None:
                trace.append(dict(moved=moved.clone(), dist2=dist2.clone(), nearest=nearest.clone(),
                                  log=log[it].clone()))
            return
        T_before = _read_state(state)[0]
        closest = torch.empty((n, 3), dtype=torch.float64, device=dev)
        launch(it, nearest, moved, dist2, _m.ptr(closest), _m.ptr(log[it]))
        T, _, status = _read_state(state)
        trace.append(dict(T_before=T_before, moved=moved.clone(), dist2=dist2.clone(), nearest=nearest.clone(),
                          closest=closest, log=log[it].clone(), T=T, status=status))

    iterations, converged, hist = _icp_run(step, log, max_iters, check_every, tol)
    res = dict(T=_read_state(state)[0], iterations=iterations, converged=converged, rmse=float(hist[-1, 1]),
               inliers=int(hist[-1, 0]), history=hist)
    if plane:
        res["point_rmse"], res["normal_spread"] = log[iterations - 1, 4:6].tolist()
    return res


def _alignment_arg(what, align, align_kw, icp):
    """compare_meshes' and compare_clouds' `align` -> (T, alignment): (None, None) for None; a Sim3 itself; for "icp"
    the T of icp(**align_kw), align_meshes or align_clouds bound to the pair.  alignment: the dict the figures gain."""
    if not isinstance(align, str):
        if align_kw:
            raise ValueError(f"{what}: align_kw goes with align='icp' only")
        if align is None:
            return None, None
        T = _sim3_arg(align, what, None, torch.float64)
        return T, dict(rmse=None, iterations=None, T=T.tolist())
    if align != "icp":
        raise ValueError(f"{what}: align must be None, a Sim3 or 'icp', got {align!r}")
    res = icp(**(align_kw or {}))
    return res["T"], dict(rmse=res["rmse"], iterations=res["iterations"], T=res["T"].tolist())


def align_meshes(pred, gt, init=None, n_samples=20000, max_iters=50, trim=math.inf, with_scale=True, seed=0, tol=1e-6,
                 check_every=5, index=None, metric="point", point_weight=0.0, _trace=None):
    """Trimmed point-to-mesh ICP of the mesh `pred` onto the mesh `gt` (both (vertices f32[V,3], faces i32[F,3]) device
    tensors or extract_mesh tuples): the Sim3 T with T(pred) ~ gt.

    n_samples points are drawn on pred (sample_mesh with `seed`) once.  Every iteration moves them by the current T,
    finds the exact closest point of gt for each (the culled scan of mesh_distance, warm-started from the last
    iteration's faces; gt's tile boxes are built once), keeps the pairs within `trim` (in gt's units; +inf keeps all;
    a sequence gives one value per iteration) and replaces T by the closed-form similarity of the original samples onto
    their closest points (`with_scale=False`: scale 1).  Nothing is read back except the log, once every `check_every`
    iterations; the loop stops when the RMSE of two successive iterations differs by at most `tol` relative, when an
    iteration is degenerate (fewer than 3 pairs within `trim`), or after `max_iters`.

    `index`: None, True or a MeshIndex of `gt`: the scan runs over its Morton-ordered tiles and group boxes instead of
    the tiles of gt's face order, warm start unchanged; same transform and log, bit for bit (DESIGN.md "Mesh index").

    `metric`: "point" - the above; "plane" - the point-to-plane metric with a Gauss-Newton solve (DESIGN.md
    "Point-to-plane ICP"): each pair contributes n . (q - c), n the plane of the nearest face, and the solve composes a
    small Sim3 onto T; on planar scenes it needs a tenth of the iterations.  It constrains nothing ALONG a surface, so a
    scene whose faces leave a direction free slides; `point_weight` > 0 (0.05 is a mild tie; "plane" only) adds the
    three point residuals q - c with that weight.  The dict then gains point_rmse (the RMSE of |q - c|; `rmse` is that
    of the minimised residual) and normal_spread (the smallest eigenvalue of the summed n n^T - with point_weight, plus
    point_weight I - over the pairs; near 0: some translation is free), both of the last iteration.

    ICP is a LOCAL method: it needs `init` (a Sim3, default the identity) for anything beyond a modest offset.  On a
    partial room, a numpy prototype recovered 8 degrees / 15 cm / scale 0.9 and failed at 15 degrees / 0.3 m / scale
    0.8, where the samples slid along a wall.  SlamSystem.align_trajectory gives an `init` from camera centres.

    Returns a dict: T (f64[8] device tensor), iterations (the steps run), converged, rmse and inliers (of the last
    iteration: the pairs within trim under the T that iteration started from, and their RMSE), history (numpy
    f64[iterations, 4]: inliers, rmse, scale after the solve, status)."""
    what = "align_meshes"
    max_iters, check_every, trims = _icp_args(what, max_iters, check_every, tol, trim)
    plane, point_weight = _metric_arg(what, metric, point_weight)
    index = _index_arg(MeshIndex, index, what, *_pair(gt, "gt"))
    pv, pf, pV, pF = _mesh_arg(*_pair(pred, "pred"), True, what)
    gv, gf, gV, gF = _mesh_arg(*_pair(gt, "gt"), True, what)
    if pv.device != gv.device:
        raise ValueError(f"{what}: pred and gt are on different devices")
    dev = pv.device
    src = _sample(pv, pf, pV, pF, n_samples, seed, what)[0]
    n = int(src.shape[0])
    T0 = None if init is None else _sim3_arg(init, what, dev, torch.float32)
    L, st = _m.lib(), _m.stream_ptr()
    boxed = gF if index is None else 0
    ws_bytes = int(L.mslam_icp_plane_workspace_bytes(n, boxed) if plane
                   else L.mslam_mesh_align_workspace_bytes(n, boxed, 0))
    ws, state = _icp_setup(dev, ws_bytes, T0, (gv, gf, gF, gV) if index is None else None)
    # mslam_{mesh_align_step, icp_plane_step_mesh}[_indexed]: the sample and the mesh, with an index its three operands,
    # then the metric's own arguments, then what every step takes
    name = ("icp_plane_step_mesh" if plane else "mesh_align_step") + ("" if index is None else "_indexed")
    step_fn = getattr(L, "mslam_" + name)
    target = (_m.ptr(src), n, _m.ptr(gv), _m.ptr(gf), gF, gV) + (() if index is None else _index_ops(index)[:3])
    scale = 1 if with_scale else 0

    def launch(it, nearest, moved, dist2, closest, log_row):
        metric = (trims[it], point_weight, scale) if plane else (trims[it], scale, 0)       # 0: no skip counts
        _m.check(step_fn(*target, *metric, _m.ptr(ws), ws_bytes, _m.ptr(state), _m.ptr(nearest), _m.ptr(moved),
                         _m.ptr(dist2), closest, log_row, st), name)

    return _state_run(src, state, launch, plane, max_iters, check_every, tol, _trace)
