"""GPU tests (-m gpu) of how the nine entry points that take a spatial index - (order, index, index_bytes, levels), or
(order, index, index_bytes) for the two mesh ICP steps - answer degenerate calls: `levels` out of range, an order
without its index, no queries, an empty target.  The checks are one host helper (md_index_arg of csrc/mesh_tri.h), but
every entry point keeps it where its checks stood, so the answers differ per entry point: TABLE is what the library gave
before the helper existed, and it is what it must give.  The size refusals of index_bytes are pinned by each entry
point's own test file.  Every output lies in a guarded buffer; a refused call leaves its fill pattern."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mesh_support import FAR, NEAR, Operands  # noqa: E402
from mesh_support import _build as _build_mesh  # noqa: E402
from test_cloud_gpu import _build as _build_cloud  # noqa: E402
from test_cloud_gpu import cloud, queries  # noqa: E402

pytestmark = pytest.mark.gpu

N_TARGET = 129       # two tiles, one element in the second
N_QUERIES = 70       # one block, a partial second wave
EINVAL = -1
OK = (0, "")
LEVELS = (EINVAL, "levels must be")
NEEDS = (EINVAL, "an order needs its index")
NULL = (EINVAL, "null pointer")
# (return code, fragment of mslam_last_error) per entry point and cell; None: the cell does not exist there
#                                  levels 0 and 3,    an order and a null index, the target of
#                                  70 and 0 queries   129 and 70 q.   129 and 0 q.   0 elements
TABLE = {
    "cloud_distance":              (LEVELS,           NEEDS,          OK,            OK),
    "cloud_knn":                   (LEVELS,           NEEDS,          OK,            OK),
    "cloud_radius_count":          (LEVELS,           NEEDS,          NEEDS,         OK),
    "cloud_cluster_link":          (LEVELS,           NEEDS,          NEEDS,         OK),
    "icp_plane_step_cloud":        (LEVELS,           NEEDS,          NEEDS,         OK),
    "mesh_distance_indexed":       (LEVELS,           NULL,           OK,            None),
    "mesh_raycast_indexed":        (LEVELS,           NULL,           OK,            None),
    "mesh_align_step_indexed":     (None,             NULL,           NULL,          None),
    "icp_plane_step_mesh_indexed": (None,             NULL,           NULL,          None),
}
K = 3


def _lib():
    import mslam_hip as _m

    return _m, _m.lib(), _m.stream_ptr()


@pytest.fixture(scope="module")
def env(device):
    rng = np.random.default_rng(129)
    V = rng.uniform(0.0, 1.0, (3 * N_TARGET, 3)).astype(np.float32)
    normals = rng.normal(size=(N_TARGET, 3)).astype(np.float32)
    Q = queries("random")[:N_QUERIES]
    return dict(cloud=_build_cloud(device, cloud(N_TARGET, "random")), Q=Q,
                rays=(Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32),
                normals=torch.from_numpy(normals).to(device),
                mesh=_build_mesh(device, V, np.arange(3 * N_TARGET, dtype=np.int32).reshape(-1, 3)))


def _call(device, env, entry, n, full, with_index, levels):
    """One raw call of `entry`: n queries (samples, rays), the target of 129 elements (`full`) or of none, the target's
    order, its index or NULL, `levels` -> (rc, message, the Operands, the outputs by name, the tensors that a refused
    call must leave alone, each with the copy taken before the call)."""
    _m, L, st = _lib()
    mh = _m.header_constants()
    ops = Operands(device)
    on_cloud = entry in ("cloud_distance", "cloud_knn", "cloud_radius_count", "cloud_cluster_link",
                         "icp_plane_step_cloud")
    ix = env["cloud" if on_cloud else "mesh"]
    # never NULL; with an empty target it is not followed
    index = (_m.ptr(ix["o"]), _m.ptr(ix["ws"]) if with_index else 0, ix["ws"].numel())
    q = ops.put((env["rays"] if entry == "mesh_raycast_indexed" else env["Q"])[:n], np.float32)
    if on_cloud:
        p, nrm, N = (ix["p"], env["normals"], ix["N"]) if full else (None, None, 0)
    else:
        assert full
        mesh = (_m.ptr(ix["v"]), _m.ptr(ix["f"]), ix["nf"], ix["nv"])
    out, kept = {}, {}
    if "step" in entry:                                                          # the three ICP steps
        plane = entry.startswith("icp_plane")
        state = torch.empty(mh["MSLAM_MESH_ALIGN_STATE_BYTES"], dtype=torch.uint8, device=device)
        _m.check(L.mslam_mesh_align_init_indexed(0, _m.ptr(state), st), "mesh_align_init_indexed")
        ws_bytes = int(L.mslam_icp_plane_workspace_bytes(n, 0) if plane else L.mslam_mesh_align_workspace_bytes(n, 0, 0))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        kept["state"] = (state, state.clone())
        out = dict(nearest=ops.out(torch.int32, (n,)), moved=ops.out(torch.float32, (n, 3)),
                   dist2=ops.out(torch.float64, (n,)),
                   log_row=ops.out(torch.float64, (mh["MSLAM_ICP_PLANE_LOG_DOUBLES" if plane
                                                       else "MSLAM_MESH_ALIGN_LOG_DOUBLES"],)))
        tail = (_m.ptr(ws), ws_bytes, _m.ptr(state), _m.ptr(out["nearest"]), _m.ptr(out["moved"]), _m.ptr(out["dist2"]),
                0, _m.ptr(out["log_row"]), st)
    if entry == "cloud_distance":
        out = dict(dist2=ops.out(torch.float64, (n,)), nearest=ops.out(torch.int32, (n,)))
        rc = L.mslam_cloud_distance(_m.ptr(q), n, _m.ptr(p), N, *index, levels, 0, _m.ptr(out["dist2"]),
                                    _m.ptr(out["nearest"]), st)
    elif entry == "cloud_knn":
        out = dict(dist2=ops.out(torch.float64, (n, K)), nearest=ops.out(torch.int32, (n, K)))
        rc = L.mslam_cloud_knn(_m.ptr(q), n, _m.ptr(p), N, K, 0, *index, levels, 0, _m.ptr(out["dist2"]),
                               _m.ptr(out["nearest"]), st)
    elif entry == "cloud_radius_count":
        out = dict(count=ops.out(torch.int32, (n,)))
        rc = L.mslam_cloud_radius_count(_m.ptr(q), n, _m.ptr(p), N, 0.01, *index, levels, 0, _m.ptr(out["count"]), st)
    elif entry == "cloud_cluster_link":                                          # self NULL: row i is point i
        core = torch.ones(N, dtype=torch.uint8, device=device)
        parent = torch.arange(N, dtype=torch.int32, device=device)
        kept["parent"] = (parent, parent.clone())
        out = dict(nearest=ops.out(torch.int32, (n,)), dist2=ops.out(torch.float64, (n,)))
        rc = L.mslam_cloud_cluster_link(_m.ptr(p), N, 0, n, 0.01, _m.ptr(core), *index, levels, 0,
                                        _m.ptr(parent), _m.ptr(out["nearest"]), _m.ptr(out["dist2"]), st)
    elif entry == "icp_plane_step_cloud":
        rc = L.mslam_icp_plane_step_cloud(_m.ptr(q), n, _m.ptr(p), _m.ptr(nrm), N, *index, levels, np.inf, 0.0, 1, *tail)
    elif entry == "mesh_distance_indexed":
        out = dict(dist2=ops.out(torch.float64, (n,)), nearest=ops.out(torch.int32, (n,)))
        rc = L.mslam_mesh_distance_indexed(_m.ptr(q), n, *mesh, *index, levels, 0, _m.ptr(out["dist2"]),
                                           _m.ptr(out["nearest"]), st)
    elif entry == "mesh_raycast_indexed":
        pose = ops.put([0, 0, 0, 0, 0, 0, 1, 1], np.float32)
        out = dict(range=ops.out(torch.float32, (n,)), normal=ops.out(torch.float32, (n, 3)),
                   hit=ops.out(torch.uint8, (n,)), face=ops.out(torch.int32, (n,)), t64=ops.out(torch.float64, (n,)))
        rc = L.mslam_mesh_raycast_indexed(_m.ptr(q), 1, n, _m.ptr(pose), *mesh, NEAR, FAR, *index, levels, 0,
                                          *(_m.ptr(t) for t in out.values()), st)
    elif entry == "mesh_align_step_indexed":
        rc = L.mslam_mesh_align_step_indexed(_m.ptr(q), n, *mesh, *index, np.inf, 1, 0, *tail)
    else:
        assert entry == "icp_plane_step_mesh_indexed"
        rc = L.mslam_icp_plane_step_mesh_indexed(_m.ptr(q), n, *mesh, *index, np.inf, 0.0, 1, *tail)
    message = L.mslam_last_error().decode() if rc else ""
    return rc, message, ops, out, list(kept.values())


def _cells(entry):
    """(label, n, full, with_index, levels, expected) of the cells of `entry`."""
    by_levels, null_index, null_index_q0, empty = TABLE[entry]
    cells = []
    if by_levels is not None:
        cells += [(f"levels {lv}, {n} queries", n, True, True, lv, by_levels) for lv in (0, 3) for n in (N_QUERIES, 0)]
    cells += [(f"null index, {N_QUERIES} queries", N_QUERIES, True, False, 2, null_index),
              ("null index, 0 queries", 0, True, False, 2, null_index_q0)]
    if empty is not None:
        cells += [(f"null index, empty target, {n} queries", n, False, False, 2, empty) for n in (N_QUERIES, 0)]
    return cells


@pytest.mark.parametrize("entry", list(TABLE))
def test_degenerate_calls(device, env, entry):
    wrong = []
    for label, n, full, with_index, levels, (want_rc, want_text) in _cells(entry):
        rc, message, ops, out, kept = _call(device, env, entry, n, full, with_index, levels)
        torch.cuda.synchronize()
        print(f"{entry} | {label}: rc {rc} {message!r}")
        if rc != want_rc or want_text not in message:
            wrong.append((label, rc, message))
        if rc:                                                                    # refused: nothing written
            for name in ops.outputs:
                assert bool((ops.all[name].raw == ops.all[name].pat).all()), (label, name)
            for t, before in kept:
                assert torch.equal(t, before), label
            continue
        ops.check()
        if not full and n:                                                        # the answers of an empty target
            for name, t in out.items():
                if name == "nearest":
                    assert bool((t == -1).all()), label
                elif name == "dist2":
                    assert bool(torch.isinf(t).all()) and bool((t > 0).all()), label
                elif name == "count":
                    assert bool((t == 0).all()), label
    env["cloud"]["ops"].check()
    env["mesh"]["ops"].check()
    assert not wrong, wrong
