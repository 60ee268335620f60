"""GPU tests (-m gpu) of decimate_mesh (csrc/mesh_decimate.hip, DESIGN.md "Mesh decimation") and of the decimate_*
arguments of the mesh extraction, against the numpy statement tests/decimate_numpy.py.

Everything is compared byte for byte: collapse decisions compare f64 costs, so a cost that differs in its last bit shows
up as different faces.  The state is f64 on the f32 input, every sum is sequential in the statement's order, every
operation is rounded on its own (-ffp-contract=off), and nothing goes through a library function other than sqrt and
the division, both correctly rounded."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimate_numpy as Q  # noqa: E402
import simplify_numpy as S  # noqa: E402
import smooth_numpy as T  # noqa: E402
from mesh_support import VS, Operands, _host, _room, _same, _vol  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(mesh, device):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in mesh)


def _bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()))


def _check(mesh, device, what, mesh_d=None, want=None, **kw):
    """decimate_mesh on the device against the statement: every tensor, the map, the rounds and the classes."""
    from mast3r_slam.tsdf import decimate_mesh

    mesh_d = _dev(mesh, device) if mesh_d is None else mesh_d
    out = decimate_mesh(mesh_d, return_map=True, return_info=True, **kw)
    want = Q.decimate(mesh, return_map=True, return_info=True, **kw) if want is None else want
    assert len(out) == len(mesh) + 2
    for k in range(len(mesh)):
        assert out[k].is_cuda and out[k].is_contiguous()
        _bytes(out[k].cpu().numpy(), want[k], f"{what} tensor {k}")
    _bytes(out[-2].cpu().numpy(), want[-2], what + " vertex_map")
    info, winfo = out[-1], want[-1]
    assert info["rounds"] == winfo["rounds"], what
    _bytes(info["collapses"].numpy(), winfo["collapses"], what + " collapses")
    assert info["max_cost"] == winfo["max_cost"], (what, info["max_cost"], winfo["max_cost"])
    _bytes(info["removable"].cpu().numpy(), winfo["removable"], what + " removable")
    _bytes(info["boundary"].cpu().numpy(), winfo["boundary"], what + " boundary")
    plain = decimate_mesh(mesh_d, **kw)
    assert len(plain) == len(mesh) and all(torch.equal(a, b) for a, b in zip(plain, out))
    return out


def _with_attributes(V, F, colors):
    rng = np.random.default_rng(len(V))
    N = rng.normal(size=V.shape)
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)
    return (V, N, F) + ((rng.uniform(0, 1, V.shape).astype(np.float32),) if colors else ())


HAND = dict({k: (np.array(v[0], np.float32).reshape(-1, 3), np.array(v[1], np.int32).reshape(-1, 3))
             for k, v in T.HAND.items()}, flat_fan=Q.disc(1), disc=Q.disc(2), disc3=Q.disc(3), notched=Q.notched_fan())


@pytest.mark.parametrize("colors", [False, True])
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_meshes(device, name, colors):
    mesh = _with_attributes(*HAND[name], colors)
    nf = len(mesh[2])
    _check(mesh, device, f"{name} to 0", target_faces=0)
    _check(mesh, device, f"{name} by two", target_faces=max(nf - 2, 0))
    _check(mesh, device, f"{name} ratio", ratio=0.5)
    _check(mesh, device, f"{name} error", max_error=0.05)
    same = _check(mesh, device, f"{name} nothing to do", target_faces=nf + 1)
    assert same[-1]["rounds"] == 0


@pytest.mark.parametrize("name", ["sphere2", "torus", "box", "plate"])
def test_fixtures_at_their_targets(device, name):
    mesh = Q.fixture(name)
    ref = Q.fixture_reference(name)
    out = _check(mesh, device, name, want=ref[:4] + (dict(ref[4]),), target_faces=Q.TARGETS[name])
    assert Q.TARGETS[name] - 1 <= out[2].shape[0] <= Q.TARGETS[name]


def test_sphere_by_error_and_cap(device):
    mesh = Q.fixture("sphere2")
    mesh_d = _dev(mesh, device)
    faces = [int(_check(mesh, device, f"sphere2 {e}", mesh_d=mesh_d, max_error=e * VS)[2].shape[0])
             for e in (0.02, 0.05, 0.1)]
    assert faces[0] > faces[1] > faces[2]
    _check(mesh, device, "sphere2 error and target", mesh_d=mesh_d, max_error=0.1 * VS, target_faces=2000)
    cap = T.sphere_cap()
    out = _check(cap, device, "cap", ratio=0.25)
    assert int(out[-1]["boundary"].sum()) == 88


def _grid(V, seed, flat=False):
    """A grid_patch cut to exactly V vertices (the faces that use a dropped vertex go with it), with colours."""
    ny = 16 if V % 16 == 0 else 19 if V % 19 == 0 else 17
    P, N, F, C = S.grid_patch(-(-V // ny), ny, seed)
    if flat:
        P = P.copy()
        P[:, 2] = 1.0
    return P[:V], N[:V], np.ascontiguousarray(F[(F < V).all(1)]), C[:V]


@pytest.mark.parametrize("V", [255, 256, 257, 513])
def test_grids_at_block_edges(device, V):
    """One lane per vertex in blocks of 256: the last block full, one short, one over, and a third block of one."""
    mesh = _grid(V, seed=V)
    nf = len(mesh[2])
    assert len(mesh[0]) == V and nf > V
    out = _check(mesh, device, f"grid {V} target", target_faces=nf // 3)
    assert out[-1]["rounds"] > 3
    _check(mesh, device, f"grid {V} ratio", ratio=0.6)
    _check(mesh, device, f"grid {V} error", max_error=0.05)
    _check(_grid(V, seed=V, flat=True)[:3], device, f"flat grid {V}, every cost zero", target_faces=nf // 4)


def test_views_repeat_calls_and_empty(device):
    """Non-contiguous inputs, the same bytes on every call, inputs left as they were, and empty meshes."""
    from mast3r_slam.tsdf import decimate_mesh

    mesh = _grid(257, seed=2)
    V, F = len(mesh[0]), len(mesh[2])
    wide = torch.zeros((V, 5), dtype=torch.float32, device=device)
    wide[:, 1:4] = torch.from_numpy(mesh[0]).to(device)
    every_other = torch.zeros((2 * V, 3), dtype=torch.float32, device=device)
    every_other[::2] = torch.from_numpy(mesh[1]).to(device)
    faces_t = torch.from_numpy(np.ascontiguousarray(mesh[2].T)).to(device).T
    views = (wide[:, 1:4], every_other[::2], faces_t, torch.from_numpy(mesh[3]).to(device))
    assert not any(v.is_contiguous() for v in views[:3])
    before = [v.clone() for v in views]
    first = _check(mesh, device, "views", mesh_d=views, ratio=0.3)
    for v, b in zip(views, before):
        assert torch.equal(v, b)
    for _ in range(3):
        again = decimate_mesh(views, ratio=0.3, return_map=True)
        assert all(torch.equal(a, b) for a, b in zip(again, first[:5]))
    assert decimate_mesh(views, target_faces=F) is views and decimate_mesh(views, ratio=1.0) is views
    empty = tuple(torch.zeros((0, 3), dtype=d, device=device) for d in (torch.float32, torch.float32, torch.int32))
    assert decimate_mesh(empty, 10) is empty
    out = decimate_mesh(empty, ratio=0.5, return_map=True, return_info=True)
    assert out[3].shape == (0,) and out[4]["rounds"] == 0 and out[4]["removable"].shape == (0,)
    no_faces = _dev(mesh[:2], device) + (empty[2],)
    out = decimate_mesh(no_faces, max_error=0.1, return_map=True, return_info=True)
    assert all(a is b for a, b in zip(out, no_faces)) and torch.equal(out[3].cpu(), torch.arange(V, dtype=torch.int32))
    assert not out[4]["removable"].any() and not out[4]["boundary"].any()


def test_validation(device):
    from mast3r_slam.tsdf import decimate_mesh

    mesh = _with_attributes(*HAND["disc"], True)
    mesh_d = _dev(mesh, device)
    for bad in (np.nan, np.inf, -np.inf):
        V = mesh[0].copy()
        V[2, 1] = bad
        with pytest.raises(ValueError, match=r"decimate_mesh: vertex coordinates span \[.*\] and are not all finite"):
            decimate_mesh(_dev((V,) + mesh[1:], device), 4)
    for face, span in (([0, 1, 13], r"\[0, 13\]"), ([0, -1, 2], r"\[-1, 12\]")):
        F = mesh[2].copy()
        F[0] = face
        with pytest.raises(ValueError, match=r"decimate_mesh: face indices span " + span + r", outside \[0, 13\)"):
            decimate_mesh(_dev(mesh[:2] + (F,) + mesh[3:], device), 4)
    with pytest.raises(ValueError, match="one of target_faces, ratio and max_error is needed"):
        decimate_mesh(mesh_d)
    with pytest.raises(ValueError, match="target_faces must be >= 0"):
        decimate_mesh(mesh_d, -2)
    with pytest.raises(ValueError, match=r"ratio must be in \(0, 1\]"):
        decimate_mesh(mesh_d, ratio=1.01)
    with pytest.raises(ValueError, match="max_error must be finite and >= 0"):
        decimate_mesh(mesh_d, max_error=float("nan"))
    with pytest.raises(ValueError, match="mesh must hold 3 or 4 tensors"):
        decimate_mesh(mesh_d[:2], 4)
    with pytest.raises(ValueError, match=r"normals must be \(13,3\)"):
        decimate_mesh((mesh_d[0], mesh_d[1][:3], mesh_d[2]), 4)


# ----------------------------------------------------------------------------------------------------------------------
# the C entry points, operands in guarded allocations
# ----------------------------------------------------------------------------------------------------------------------
def _raw_round(device, P, F, gate, rnd):
    """state -> candidates -> rank (torch) -> two spreads -> apply -> finish through the C entry points; every operand of
    every launch in a guarded allocation."""
    import mslam_hip as _m

    L, st = _m.lib(), _m.stream_ptr()
    ops = Operands(device)
    nv, nf = len(P), len(F)
    v32 = ops.put(P, np.float32)
    f = ops.put(np.reshape(F, (-1, 3)), np.int32)
    keys = torch.empty(6 * nf, dtype=torch.int64, device=device)
    _m.check(L.mslam_mesh_smooth_edges(_m.ptr(f), nf, nv, _m.ptr(keys), st), "edges")
    ukeys, cnt = torch.unique_consecutive(torch.sort(keys)[0], return_counts=True)
    ne = int(ukeys.shape[0])
    row_start = ops.put(torch.searchsorted(ukeys, torch.arange(nv + 1, device=device) * nv).cpu().numpy(), np.int64)
    nbr = ops.put((ukeys % max(nv, 1)).cpu().numpy(), np.int32)
    mult = ops.put(cnt.cpu().numpy(), np.int32)
    pairs = torch.empty(3 * nf, dtype=torch.int64, device=device)
    _m.check(L.mslam_mesh_vertex_faces(_m.ptr(f), nf, nv, _m.ptr(pairs), st), "faces")
    sorted_pairs = ops.put(torch.sort(pairs)[0].cpu().numpy(), np.int64)
    pstart = ops.put(torch.searchsorted(sorted_pairs, torch.arange(nv + 1, device=device) * nf).cpu().numpy(), np.int64)
    state = ops.out(torch.float64, (nv, 11))
    _m.check(L.mslam_mesh_decimate_state(_m.ptr(v32), _m.ptr(f), nf, nv, _m.ptr(sorted_pairs), _m.ptr(pstart),
                                         _m.ptr(state), st), "state")
    best, cost = ops.out(torch.int32, (nv,)), ops.out(torch.float64, (nv,))
    key, vclass = ops.out(torch.int64, (nv,)), ops.out(torch.uint8, (nv,))
    _m.check(L.mslam_mesh_decimate_candidates(_m.ptr(v32), _m.ptr(f), nf, nv, _m.ptr(row_start), _m.ptr(nbr),
                                              _m.ptr(mult), ne, _m.ptr(sorted_pairs), _m.ptr(pstart), _m.ptr(state),
                                              gate, rnd, _m.ptr(best), _m.ptr(cost), _m.ptr(key), _m.ptr(vclass), st),
             "candidates")
    ops.check()
    by_key = torch.sort(key)[1]
    order = by_key[torch.sort(cost[by_key], stable=True)[1]]
    rank_t = torch.empty(nv, dtype=torch.int32, device=device)
    rank_t[order] = torch.arange(nv, dtype=torch.int32, device=device)
    rank = ops.put(torch.where(best >= 0, rank_t, Q.NO_RANK).cpu().numpy(), np.int32)
    m1, m2 = ops.out(torch.int32, (nv,)), ops.out(torch.int32, (nv,))
    for src, dst in ((rank, m1), (m1, m2)):
        _m.check(L.mslam_mesh_decimate_spread(_m.ptr(src), _m.ptr(row_start), _m.ptr(nbr), nv, ne, _m.ptr(dst), st),
                 "spread")
    selected = ops.put(((best >= 0) & (m2 == rank)).cpu().numpy(), np.uint8)
    state_before = state.cpu().numpy()
    work = ops.put(np.reshape(F, (-1, 3)), np.int32)
    parent = ops.put(np.arange(nv), np.int32)
    _m.check(L.mslam_mesh_decimate_apply(_m.ptr(work), nf, nv, _m.ptr(selected), _m.ptr(best), _m.ptr(state),
                                         _m.ptr(parent), st), "apply")
    keep_face, end = ops.out(torch.int32, (nf,)), ops.out(torch.int32, (nv,))
    referenced = ops.put(np.zeros(nv), np.int32)
    _m.check(L.mslam_mesh_decimate_finish(_m.ptr(work), nf, nv, _m.ptr(parent), 1, _m.ptr(keep_face),
                                          _m.ptr(referenced), _m.ptr(end), st), "finish")
    ops.check()
    assert np.array_equal(f.cpu().numpy(), np.reshape(F, (-1, 3))) and np.array_equal(v32.cpu().numpy(), P)
    host = lambda t: t.cpu().numpy()
    return dict(state=state_before, state_after=host(state), best=host(best), cost=host(cost), key=host(key),
                vclass=host(vclass), rank=host(rank), m2=host(m2), selected=host(selected).astype(bool),
                faces=host(work), parent=host(parent), keep_face=host(keep_face), referenced=host(referenced),
                end=host(end))


@pytest.mark.parametrize("gate", [-1.0, 0.01])
def test_entry_points(device, gate):
    """One round on a mesh with faces Python would reject: an index past V, a negative one, a repeated one.  They are
    skipped, never followed, and the rest is the statement's; nothing outside the outputs is written and every output is
    written."""
    P, _, F, _ = _grid(257, seed=5)
    F = F.copy()
    F[3], F[40], F[77] = [0, 1, 257], [5, -1, 6], [9, 9, 10]
    F[100] = [2 ** 31 - 1, 0, 1]
    assert int((~T.counting(F, 257)).sum()) == 4
    rnd = 3
    got = _raw_round(device, P, F, gate, rnd)
    p = P.astype(np.float64)
    cur = F.astype(np.int64)
    S0 = Q.initial_state(p, cur)
    _bytes(got["state"], S0, "state")
    tab = Q.candidates(p, cur, S0, None if gate < 0 else gate)
    _bytes(got["best"], tab["best"].astype(np.int32), "best")
    _bytes(got["cost"], tab["cost"], "cost")
    cand = tab["best"] >= 0
    assert cand.sum() > 50 and (cand.sum() < tab["removable"].sum()) == (gate >= 0)    # the gate refuses some, not all
    want_key = np.where(cand, (Q.hash32(np.arange(257), rnd).astype(np.int64) << 31) | np.arange(257),
                        np.iinfo(np.int64).max)
    _bytes(got["key"], want_key, "key")
    import mslam_hip

    C = mslam_hip.header_constants()
    deg = np.diff(tab["row_start"])
    want_class = np.where(deg == 0, C["MSLAM_MESH_DECIMATE_ISOLATED"],
                          np.where(tab["boundary"], C["MSLAM_MESH_DECIMATE_BOUNDARY"],
                                   np.where(tab["removable"], C["MSLAM_MESH_DECIMATE_REMOVABLE"],
                                            C["MSLAM_MESH_DECIMATE_OTHER"]))).astype(np.uint8)
    _bytes(got["vclass"], want_class, "vclass")
    sel, rank = Q.select(tab, rnd, 10 ** 9)
    _bytes(got["rank"], rank.astype(np.int32), "rank")
    assert np.array_equal(np.nonzero(got["selected"])[0], np.sort(sel)) and len(sel) > 3
    v = tab["best"][sel]
    S1 = S0.copy()
    S1[v] = S1[v] + S1[sel]
    _bytes(got["state_after"], S1, "state after apply")
    step = np.arange(257)
    step[sel] = v
    ok = ((F >= 0) & (F < 257))
    want_faces = np.where(ok, step[np.where(ok, F, 0)], F).astype(np.int32)
    _bytes(got["faces"], want_faces, "faces after apply")
    _bytes(got["parent"], step.astype(np.int32), "parent")
    _bytes(got["end"], step.astype(np.int32), "end")
    live = T.counting(want_faces, 257)
    _bytes(got["keep_face"], live.astype(np.int32), "keep_face")
    assert int(live.sum()) == int(T.counting(F, 257).sum()) - 2 * len(sel)
    used = np.zeros(257, np.int32)
    used[want_faces[live].reshape(-1)] = 1
    _bytes(got["referenced"], used, "referenced")


def test_entry_points_refuse(device):
    import mslam_hip as _m

    L, st = _m.lib(), _m.stream_ptr()
    einval = _m.header_constants()["MSLAM_EINVAL"]
    r = torch.zeros(4, dtype=torch.int32, device=device)
    rs = torch.zeros(5, dtype=torch.int64, device=device)
    assert L.mslam_mesh_decimate_spread(_m.ptr(r), _m.ptr(rs), 0, 4, 0, _m.ptr(r), st) == einval      # in place
    assert L.mslam_mesh_decimate_spread(_m.ptr(r), _m.ptr(rs), 0, -1, 0, _m.ptr(r.clone()), st) == einval
    assert L.mslam_mesh_decimate_spread(0, 0, 0, 0, 0, 0, st) == 0                                    # V = 0
    assert L.mslam_mesh_decimate_state(0, 0, 0, 0, 0, 0, 0, st) == 0
    assert L.mslam_mesh_decimate_finish(0, 0, 0, 0, 0, 0, 0, 0, st) == 0
    assert L.mslam_mesh_decimate_apply(0, 0, 0, 0, 0, 0, 0, st) == 0
    x = torch.zeros((4, 11), dtype=torch.float64, device=device)
    c = torch.zeros(4, dtype=torch.float64, device=device)
    k = torch.zeros(4, dtype=torch.int64, device=device)
    v = torch.zeros((4, 3), dtype=torch.float32, device=device)
    for bad in (dict(gate=float("nan")), dict(rnd=-1), dict(best=0)):
        rc = L.mslam_mesh_decimate_candidates(_m.ptr(v), 0, 0, 4, _m.ptr(rs), 0, 0, 0, 0, _m.ptr(rs), _m.ptr(x),
                                              bad.get("gate", -1.0), bad.get("rnd", 0), bad.get("best", _m.ptr(r)),
                                              _m.ptr(c), _m.ptr(k), 0, st)
        assert rc == einval, bad
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# product path
# ----------------------------------------------------------------------------------------------------------------------
def test_room(device):
    """The room mesh at ratio 0.2: invariants only, no statement run."""
    from mast3r_slam.tsdf import (decimate_mesh, mesh_boundaries, mesh_components, mesh_from_voxels, simplify_mesh)

    vol = _vol(device, 1 << 20)
    for pw, conf, org in _room():
        vol.integrate(pw, conf, org)
    plain = vol.extract_mesh()
    V, F = plain[0].shape[0], plain[2].shape[0]
    _same(plain, vol.extract_mesh(decimate_faces=0, decimate_ratio=None, decimate_error=0.0))
    with pytest.raises(TypeError, match="unexpected keyword argument 'decimate_face'"):
        vol.extract_mesh(decimate_face=100)
    with pytest.raises(ValueError, match=r"decimate_mesh: ratio must be in \(0, 1\]"):
        vol.extract_mesh(decimate_ratio=2.0)
    out = decimate_mesh(plain, ratio=0.2, return_map=True, return_info=True)
    oV, oN, oF, vmap, info = out
    target = int(np.floor(0.2 * F))
    print(f"room: {V} / {F} -> {oV.shape[0]} / {oF.shape[0]} in {info['rounds']} rounds, target {target}, largest "
          f"accepted cost {info['max_cost']:.3e}")
    assert target - 1 <= oF.shape[0] <= target                      # the room's interior is large enough to reach a fifth
    assert 2 * int(info["collapses"].sum()) == F - oF.shape[0] and info["collapses"].numel() == info["rounds"]
    hV, hN, hF, hmap = _host((oV, oN, oF, vmap))
    pV, pN, pF = _host(plain)
    kept = np.nonzero(hmap[np.arange(V)] >= 0)[0]
    src = np.full(len(hV), -1)
    fixed = kept[(pV[kept].view(np.uint32) == hV[hmap[kept]].view(np.uint32)).all(1)]
    src[hmap[fixed][::-1]] = fixed[::-1]
    assert (src >= 0).all() and (np.diff(src) > 0).all()                     # a subset, in order
    assert hV.tobytes() == pV[src].tobytes() and hN.tobytes() == pN[src].tobytes()
    assert T.counting(hF, len(hV)).all() and len(np.unique(np.sort(hF, 1), axis=0)) == len(hF)
    assert len(np.unique(hF)) == len(hV)
    # the rims: the same loops over the same vertices, dart by dart (the subset keeps the order, so the names agree)
    b0 = {k: v.cpu().numpy() for k, v in mesh_boundaries(plain[2], V).items()}
    b1 = {k: v.cpu().numpy() for k, v in mesh_boundaries(oF, oV.shape[0]).items()}
    assert int(b0["n_boundary_edges"]) == int(b1["n_boundary_edges"]) > 0 and int(b0["n_open"]) == int(b1["n_open"])
    assert np.array_equal(b0["loop_id"], src[b1["loop_id"]]) and np.array_equal(b0["loop_length"], b1["loop_length"])
    assert sorted(zip(b0["dart_tail"].tolist(), b0["dart_head"].tolist())) == \
        sorted(zip(src[b1["dart_tail"]].tolist(), src[b1["dart_head"]].tolist()))
    assert len(np.unique(pF)) == V                                   # extraction leaves no vertex unused
    assert mesh_components(oF, oV.shape[0])[2].shape[0] == mesh_components(plain[2], V)[2].shape[0]
    # the chain: last of all, after the clustering, and the same through the voxel arrays
    _same(vol.extract_mesh(decimate_ratio=0.2), out[:3])
    n = F // 3
    _same(vol.extract_mesh(decimate_faces=n), decimate_mesh(plain, n))
    c = 2 * VS
    both = vol.extract_mesh(simplify_cell=c, decimate_ratio=0.5, decimate_error=0.2 * VS)
    _same(both, decimate_mesh(simplify_mesh(plain, c), ratio=0.5, max_error=0.2 * VS))
    keys, t, w = vol.voxels()
    _same(mesh_from_voxels(keys, t, w, VS, vol.min_weight, device=device, decimate_faces=n),
          decimate_mesh(plain, n))
    _same(mesh_from_voxels(keys, t, w, VS, vol.min_weight, device=device), plain)


def test_color_volume(device):
    import color_numpy
    from mast3r_slam.tsdf import decimate_mesh

    vol = _vol(device, color=True)
    for pw, conf, org in _room():
        vol.integrate(pw, conf, org, colors=color_numpy.texture(pw).astype(np.float32))
    cmesh = vol.extract_mesh(colors=True)
    out = vol.extract_mesh(colors=True, decimate_ratio=0.3)
    assert len(out) == 4 and out[2].shape[0] <= int(0.3 * cmesh[2].shape[0])
    _same(out, decimate_mesh(cmesh, ratio=0.3))
    _same(vol.extract_mesh(colors=True, decimate_faces=0), cmesh)


def test_slam_system_decimated_ply(device, tmp_path, monkeypatch):
    """The run of test_slam_system_mesh_and_ply."""
    from mast3r_slam import evaluate
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from mast3r_slam.tsdf import decimate_mesh
    from test_slam_system_gpu import RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    assert tcfg["mesh_decimate_faces"] == 0 and tcfg["mesh_decimate_error"] == 0.0
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    try:
        system.run(_frames(list(range(0, 60, 3)), device))
        plain = system.extract_mesh()
        n = plain[2].shape[0] // 4
        small = system.extract_mesh(decimate_faces=n)
        sizes = evaluate.save_tsdf_mesh(tmp_path, "small.ply", system, decimate_faces=n)
        evaluate.save_tsdf_mesh(tmp_path, "plain.ply", system)
        evaluate.save_tsdf_mesh(tmp_path, "zero.ply", system, decimate_faces=0, decimate_error=0.0)
        system.tsdf_manager.cfg["mesh_decimate_faces"] = n                 # the config default of the system
        _same(system.extract_mesh(), small)
        _same(system.extract_mesh(decimate_faces=0), plain)
        system.tsdf_manager.cfg["mesh_decimate_faces"] = 0
        system.tsdf_manager.cfg["mesh_decimate_error"] = 0.1               # in voxel sizes
        by_error = system.extract_mesh()
        vs = float(system.tsdf_manager.volume.voxel_size)
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    _same(small, decimate_mesh(plain, n))
    _same(by_error, decimate_mesh(plain, max_error=0.1 * vs))
    V, N, F = _host(small)
    assert sizes == (len(V), len(F)) and n - 1 <= len(F) <= n
    lv, lf = evaluate.load_mesh(tmp_path / "small.ply")
    assert lv.dtype == np.float32 and np.array_equal(lv, V) and np.array_equal(lf, F)
    assert (tmp_path / "zero.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
