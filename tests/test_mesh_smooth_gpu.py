"""GPU tests (-m gpu) of smooth_mesh and vertex_normals (csrc/mesh_smooth.hip, DESIGN.md "Mesh smoothing") and of the
smooth_* arguments of the mesh extraction, against the numpy statement tests/smooth_numpy.py.

Everything is compared byte for byte: the state is f64 from the f32 input to one final rounding, every sum is sequential
in the statement's order, nothing goes through a solver or a library function other than sqrt and the division, both
correctly rounded."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_numpy as S  # noqa: E402
import smooth_numpy as T  # noqa: E402
from mesh_support import VS, Operands, _host, _room, _same, _vol  # noqa: E402

pytestmark = pytest.mark.gpu

ROOM_MIN_WEIGHT = 40.0              # where the room's mesh has small components (tests/test_mesh_components_gpu.py)
ROOM_MIN_FACES = 5
SCHEDULES = [(1, 0.0), (2, 0.0), (10, 0.0), (1, -0.53), (2, -0.53), (10, -0.53)]      # both parities of the exchange


def _dev(mesh, device):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in mesh)


def _bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()))


def _check(mesh, device, iterations, what, mesh_d=None, **kw):
    """smooth_mesh on the device against the statement: vertices, normals, the classes; the rest passed through."""
    from mast3r_slam.tsdf import smooth_mesh

    mesh_d = _dev(mesh, device) if mesh_d is None else mesh_d
    out = smooth_mesh(mesh_d, iterations, return_info=True, **kw)
    want = T.smooth(mesh, iterations, return_info=True, **kw)
    assert len(out) == len(mesh) + 1
    for a in out[:2]:
        assert a.is_cuda and a.is_contiguous()
    assert all(a is b for a, b in zip(out[2:-1], mesh_d[2:]))
    _bytes(out[0].cpu().numpy(), want[0], what + " vertices")
    _bytes(out[1].cpu().numpy(), want[1], what + " normals")
    info = out[-1]
    _bytes(info["boundary_vertex"].cpu().numpy(), want[-1]["boundary_vertex"], what + " boundary_vertex")
    _bytes(info["degree"].cpu().numpy(), want[-1]["degree"], what + " degree")
    assert int(info["n_edges"]) == want[-1]["n_edges"], what
    plain = smooth_mesh(mesh_d, iterations, **kw)
    assert len(plain) == len(mesh) and torch.equal(plain[0], out[0]) and torch.equal(plain[1], out[1])
    return out


@pytest.mark.parametrize("colors", [False, True])
@pytest.mark.parametrize("name", sorted(T.HAND))
def test_hand_meshes(device, name, colors):
    mesh = T.hand_mesh(name, colors)
    for mode in T.MODES:
        for iterations, mu in ((1, 0.0), (2, -0.53), (3, -0.53)):
            _check(mesh, device, iterations, f"{name} {mode} {iterations}", lam=0.5, mu=mu, boundary=mode)
    _check(mesh, device, 2, f"{name} keep", normals="keep")


@pytest.mark.parametrize("name", ["sphere2", "torus", "box"])
def test_analytic_shapes(device, name):
    mesh = S.shape_mesh(name)
    mesh_d = _dev(mesh, device)
    for iterations, mu in SCHEDULES:
        _check(mesh, device, iterations, f"{name} {iterations} mu={mu}", mesh_d=mesh_d, mu=mu)


def test_noisy_sphere_and_cap(device):
    _, noisy, _, _ = T.noisy_sphere()
    _check(noisy, device, 10, "noisy sphere")
    cap = T.sphere_cap()
    for mode in T.MODES:
        out = _check(cap, device, 10, f"cap {mode}", boundary=mode)
        assert int(out[-1]["boundary_vertex"].sum()) == 88


def _grid(V, seed):
    """A grid_patch cut to exactly V vertices (the faces that use a dropped vertex go with it), with colours."""
    ny = 16 if V % 16 == 0 else 19 if V % 19 == 0 else 17
    P, N, F, C = S.grid_patch(-(-V // ny), ny, seed)
    return P[:V], N[:V], np.ascontiguousarray(F[(F < V).all(1)]), C[:V]


@pytest.mark.parametrize("V", [255, 256, 257, 513])
def test_grids_at_block_edges(device, V):
    """One lane per vertex in blocks of 256: the last block full, one short, one over, and a third block of one."""
    mesh = _grid(V, seed=V)
    assert len(mesh[0]) == V and len(mesh[2]) > V
    for mode in T.MODES:
        _check(mesh, device, 3, f"grid {V} {mode}", boundary=mode)
    _check(mesh[:3], device, 2, f"grid {V} without colours", mu=0.0)


def test_views_and_repeat_calls(device):
    """Non-contiguous inputs, the tensors that pass through, and the same bytes on every call."""
    from mast3r_slam.tsdf import smooth_mesh

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
    first = _check(mesh, device, 3, "views", mesh_d=views)
    assert first[2] is faces_t and first[3] is views[3]
    for v, b in zip(views, before):
        assert torch.equal(v, b)
    for _ in range(3):
        again = smooth_mesh(views, 3)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    off = smooth_mesh(views, 0)
    assert off is views
    rng = np.random.default_rng(1)
    shuffled = mesh[:2] + (mesh[2][rng.permutation(F)],) + mesh[3:]
    moved = smooth_mesh(_dev(shuffled, device), 3)
    assert torch.equal(moved[0], first[0]) and torch.equal(moved[1], first[1])


def test_vertex_normals(device):
    from mast3r_slam.tsdf import smooth_mesh, vertex_normals

    V, N, F = T.hand_mesh("tetrahedron")
    assert torch.equal(smooth_mesh(_dev((V, N, F), device), 0, return_info=True)[0], torch.from_numpy(V).to(device))
    for name in ("sphere2", "box"):
        V, N, F = S.shape_mesh(name)
        got = vertex_normals(*_dev((V, F), device))
        _bytes(got.cpu().numpy(), T.vertex_normals(V, F), name)
        assert float((got.cpu().double().numpy() * N).sum(1).min()) > 0.0
    V, N, F = T.hand_mesh("repeated_index")
    _bytes(vertex_normals(*_dev((V, F), device)).cpu().numpy(), T.vertex_normals(V, F), "repeated index")
    both = np.array([[0, 1, 2], [0, 2, 1]], np.int32)
    _bytes(vertex_normals(*_dev((V, both), device)).cpu().numpy(), np.zeros((4, 3), np.float32), "cancelling faces")
    none = vertex_normals(torch.zeros((0, 3), device=device), torch.zeros((0, 3), dtype=torch.int32, device=device))
    assert none.shape == (0, 3)
    no_faces = vertex_normals(torch.ones((5, 3), device=device), torch.zeros((0, 3), dtype=torch.int32, device=device))
    assert no_faces.shape == (5, 3) and not no_faces.any()
    with pytest.raises(ValueError, match=r"vertex_normals: face indices span \[0, 4\], outside \[0, 4\)"):
        vertex_normals(*_dev((V, np.array([[0, 1, 4]], np.int32)), device))


# ----------------------------------------------------------------------------------------------------------------------
# the C entry points, operands in guarded allocations
# ----------------------------------------------------------------------------------------------------------------------
def _raw(device, P, N, F, factor, mode, stride):
    """edges -> table (torch) -> one step -> faces -> normals of the stepped positions, through the C entry points."""
    import mslam_hip as _m

    L, st = _m.lib(), _m.stream_ptr()
    ops = Operands(device)
    nv, nf = len(P), len(F)
    f = ops.put(np.reshape(F, (-1, 3)), np.int32)
    keys = ops.out(torch.int64, (6 * nf,))
    _m.check(L.mslam_mesh_smooth_edges(_m.ptr(f), nf, nv, _m.ptr(keys), st), "edges")
    ukeys, cnt = torch.unique_consecutive(torch.sort(keys)[0], return_counts=True)
    row_start = ops.put(torch.searchsorted(ukeys, torch.arange(nv + 1, device=device) * nv).cpu().numpy(), np.int64)
    nbr = ops.put((ukeys % max(nv, 1)).cpu().numpy(), np.int32)
    mult = ops.put(cnt.cpu().numpy(), np.int32)
    x = np.zeros((nv, stride))
    x[:, :3] = P
    x_in, x_out = ops.put(x, np.float64), ops.out(torch.float64, (nv, stride))
    vclass = ops.out(torch.uint8, (nv,))
    _m.check(L.mslam_mesh_smooth_step(_m.ptr(x_in), _m.ptr(x_out), stride, _m.ptr(row_start), _m.ptr(nbr), _m.ptr(mult),
                                      nv, int(ukeys.shape[0]), factor, mode, _m.ptr(vclass), st), "step")
    pairs = ops.out(torch.int64, (3 * nf,))
    _m.check(L.mslam_mesh_vertex_faces(_m.ptr(f), nf, nv, _m.ptr(pairs), st), "faces")
    sorted_pairs = ops.put(torch.sort(pairs)[0].cpu().numpy(), np.int64)
    pstart = ops.put(torch.searchsorted(sorted_pairs, torch.arange(nv + 1, device=device) * nf).cpu().numpy(), np.int64)
    stepped = x_out[:, :3].to(torch.float32).cpu().numpy() if nv else np.zeros((0, 3), np.float32)
    v32, n_in = ops.put(stepped, np.float32), ops.put(N, np.float32)
    n_out = ops.out(torch.float32, (nv, 3))
    _m.check(L.mslam_mesh_vertex_normals(_m.ptr(v32), _m.ptr(f), nf, nv, _m.ptr(sorted_pairs), _m.ptr(pstart),
                                         _m.ptr(n_in), _m.ptr(n_out), st), "normals")
    ops.check()
    assert np.array_equal(f.cpu().numpy(), np.reshape(F, (-1, 3))) and np.array_equal(x_in.cpu().numpy(), x)
    assert np.array_equal(n_in.cpu().numpy(), N)
    return dict(keys=keys.cpu().numpy(), x=x_out.cpu().numpy(), vclass=vclass.cpu().numpy(), pairs=pairs.cpu().numpy(),
                normals=n_out.cpu().numpy(), stepped=stepped)


@pytest.mark.parametrize("stride", [3, 4])
def test_entry_points(device, stride):
    """A mesh with faces Python would reject: an index past V, a negative one, a repeated one.  They are skipped, never
    followed, and the rest is the statement's; nothing outside the outputs is written and every output is written."""
    P, N, F, _ = _grid(257, seed=5)
    F = F.copy()
    F[3], F[40], F[77] = [0, 1, 257], [5, -1, 6], [9, 9, 10]
    F[100] = [2 ** 31 - 1, 0, 1]
    ok = T.counting(F, 257)
    assert int((~ok).sum()) == 4
    from mast3r_slam.tsdf.mesh_smooth import _MODES

    assert sorted(_MODES) == sorted(T.MODES)
    for mode in T.MODES:
        got = _raw(device, P, N, F, 0.5, _MODES[mode], stride)
        k = got["keys"].reshape(-1, 6)
        assert (k[~ok] == np.iinfo(np.int64).max).all() and (k[ok] < 257 * 257).all() and (k[ok] >= 0).all()
        a, b, c = (F[ok][:, j].astype(np.int64) for j in range(3))
        assert np.array_equal(k[ok], np.stack([a * 257 + b, b * 257 + a, b * 257 + c, c * 257 + b, c * 257 + a,
                                               a * 257 + c], 1))
        pr = got["pairs"].reshape(-1, 3)
        assert (pr[~ok] == np.iinfo(np.int64).max).all()
        assert np.array_equal(pr[ok], F[ok].astype(np.int64) * len(F) + np.nonzero(ok)[0][:, None])
        want = T.step(P.astype(np.float64), 0.5, T.adjacency(F, 257), mode)
        _bytes(got["x"][:, :3], want, f"step {mode}")
        assert stride == 3 or not got["x"][:, 3].any()
        _bytes(got["vclass"], T.classify(F, 257)[0], "classes")
        _bytes(got["normals"], T.vertex_normals(got["stepped"], F, N), "normals")


def test_entry_points_empty(device):
    import mslam_hip as _m
    from mast3r_slam.tsdf.mesh_smooth import _STRIDE

    assert _STRIDE in (3, 4)
    P, N, F, _ = _grid(255, seed=6)
    none_f, none_v = np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32)
    got = _raw(device, P, N, none_f, 0.5, 0, 4)                      # F = 0: every vertex isolated, every normal kept
    _bytes(got["x"][:, :3], P.astype(np.float64), "F = 0")
    assert (got["vclass"] == T.ISOLATED).all() and np.array_equal(got["normals"], N)
    got = _raw(device, none_v, none_v, none_f, 0.5, 0, 3)            # V = 0
    assert got["x"].shape == (0, 3)
    got = _raw(device, none_v, none_v, np.array([[0, 1, 2]], np.int32), 0.5, 0, 3)       # V = 0 with a face: skipped
    assert (got["keys"] == np.iinfo(np.int64).max).all() and (got["pairs"] == np.iinfo(np.int64).max).all()
    L = _m.lib()
    x = torch.zeros((4, 4), dtype=torch.float64, device=device)
    rs = torch.zeros(5, dtype=torch.int64, device=device)
    for bad in (dict(stride=5), dict(mode=3), dict(factor=float("nan")), dict(out=x)):
        rc = L.mslam_mesh_smooth_step(_m.ptr(x), _m.ptr(bad.get("out", x.clone())), bad.get("stride", 4), _m.ptr(rs), 0,
                                      0, 4, 0, bad.get("factor", 0.5), bad.get("mode", 0), 0, _m.stream_ptr())
        assert rc == _m.header_constants()["MSLAM_EINVAL"], bad


# ----------------------------------------------------------------------------------------------------------------------
# call behaviour
# ----------------------------------------------------------------------------------------------------------------------
def test_validation(device):
    from mast3r_slam.tsdf import smooth_mesh

    mesh = T.hand_mesh("two_triangles", True)
    mesh_d = _dev(mesh, device)
    for off in (None, 0, -3):
        assert smooth_mesh(mesh_d, off) is mesh_d
    for bad in (1.5, 2.0, "3"):
        with pytest.raises(ValueError, match="smooth_mesh: iterations must be an integer"):
            smooth_mesh(mesh_d, bad)
    for kw in (dict(lam=float("nan")), dict(lam=float("inf")), dict(mu=float("-inf")), dict(mu=float("nan"))):
        with pytest.raises(ValueError, match="smooth_mesh: lam and mu must be finite"):
            smooth_mesh(mesh_d, 1, **kw)
    with pytest.raises(ValueError, match="boundary must be 'fixed', 'curve' or 'free', got 'pinned'"):
        smooth_mesh(mesh_d, 1, boundary="pinned")
    with pytest.raises(ValueError, match="normals must be 'recompute' or 'keep', got 'flat'"):
        smooth_mesh(mesh_d, 1, normals="flat")
    for bad in (np.nan, np.inf, -np.inf):
        V = mesh[0].copy()
        V[2, 1] = bad
        with pytest.raises(ValueError, match=r"smooth_mesh: vertex coordinates span \[.*\] and are not all finite"):
            smooth_mesh(_dev((V,) + mesh[1:], device), 1)
    for face, span in (([0, 1, 4], r"\[0, 4\]"), ([0, -1, 2], r"\[-1, 3\]")):
        F = mesh[2].copy()
        F[0] = face
        with pytest.raises(ValueError, match=r"smooth_mesh: face indices span " + span + r", outside \[0, 4\)"):
            smooth_mesh(_dev(mesh[:2] + (F,) + mesh[3:], device), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        smooth_mesh(tuple(torch.from_numpy(a) for a in mesh), 1)
    with pytest.raises(ValueError, match="mesh must hold 3 or 4 tensors"):
        smooth_mesh(mesh_d[:2], 1)
    with pytest.raises(ValueError, match=r"normals must be \(4,3\)"):
        smooth_mesh((mesh_d[0], mesh_d[1][:3], mesh_d[2]), 1)
    empty = tuple(torch.zeros((0, 3), dtype=d, device=device) for d in (torch.float32, torch.float32, torch.int32))
    assert smooth_mesh(empty, 2) is empty
    no_faces = mesh_d[:2] + (empty[2],)
    out = smooth_mesh(no_faces, 2, return_info=True)
    assert all(a is b for a, b in zip(out, no_faces)) and not out[3]["boundary_vertex"].any() and int(out[3]["n_edges"]) == 0


def test_quality_through_the_products_metric(device):
    from mast3r_slam.tsdf import compare_meshes, smooth_mesh

    clean, noisy, _, _ = T.noisy_sphere()
    clean_d, noisy_d = _dev(clean, device), _dev(noisy, device)
    before = compare_meshes(noisy_d, clean_d, n_samples=4000, threshold=VS, seed=1)
    after = compare_meshes(smooth_mesh(noisy_d, 10), clean_d, n_samples=4000, threshold=VS, seed=1)
    print(f"noisy sphere against the clean one: accuracy {before['accuracy']:.5f} -> {after['accuracy']:.5f}, "
          f"completion {before['completion']:.5f} -> {after['completion']:.5f}")
    assert after["accuracy"] < before["accuracy"]


# ----------------------------------------------------------------------------------------------------------------------
# product path
# ----------------------------------------------------------------------------------------------------------------------
def test_room(device):
    from mast3r_slam.tsdf import filter_mesh, mesh_from_voxels, simplify_mesh, smooth_mesh

    c = 2 * VS
    vol = _vol(device, 1 << 20)
    for pw, conf, org in _room():
        vol.integrate(pw, conf, org)
    plain = vol.extract_mesh()
    _same(plain, vol.extract_mesh(smooth_iterations=0))
    for k in (1, 4):
        _same(vol.extract_mesh(smooth_iterations=k), smooth_mesh(plain, k))
    _same(vol.extract_mesh(smooth_iterations=2, smooth_lambda=0.4, smooth_mu=0.0, smooth_boundary="curve"),
          smooth_mesh(plain, 2, lam=0.4, mu=0.0, boundary="curve"))
    _check(_host(plain), device, 4, "room", mesh_d=plain)
    raw = vol.extract_mesh(min_weight=ROOM_MIN_WEIGHT)
    filt = filter_mesh(raw, min_faces=ROOM_MIN_FACES)
    assert filt[2].shape[0] < raw[2].shape[0]
    both = vol.extract_mesh(min_weight=ROOM_MIN_WEIGHT, min_component_faces=ROOM_MIN_FACES, smooth_iterations=3,
                            simplify_cell=c)
    _same(both, simplify_mesh(smooth_mesh(filt, 3), c))
    assert not torch.equal(both[0], simplify_mesh(filt, c)[0])
    keys, t, w = vol.voxels()
    _same(both, mesh_from_voxels(keys, t, w, VS, ROOM_MIN_WEIGHT, device=device, min_component_faces=ROOM_MIN_FACES,
                                 smooth_iterations=3, simplify_cell=c))


def test_color_volume(device):
    import color_numpy
    from mast3r_slam.tsdf import smooth_mesh

    vol = _vol(device, color=True)
    for pw, conf, org in _room():
        vol.integrate(pw, conf, org, colors=color_numpy.texture(pw).astype(np.float32))
    cmesh = vol.extract_mesh(colors=True)
    out = vol.extract_mesh(colors=True, smooth_iterations=2)
    assert len(out) == 4
    _same(out, smooth_mesh(cmesh, 2))
    assert torch.equal(out[3], cmesh[3]) and torch.equal(out[2], cmesh[2]) and not torch.equal(out[0], cmesh[0])


def test_slam_system_smoothed_ply(device, tmp_path, monkeypatch):
    """The run of test_slam_system_mesh_and_ply."""
    from mast3r_slam import evaluate
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from mast3r_slam.tsdf import smooth_mesh
    from test_slam_system_gpu import RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    assert tcfg["mesh_smooth_iterations"] == 0
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    try:
        system.run(_frames(list(range(0, 60, 3)), device))
        plain = system.extract_mesh()
        smoothed = system.extract_mesh(smooth_iterations=5)
        sizes = evaluate.save_tsdf_mesh(tmp_path, "smoothed.ply", system, smooth_iterations=5)
        evaluate.save_tsdf_mesh(tmp_path, "plain.ply", system)
        evaluate.save_tsdf_mesh(tmp_path, "zero.ply", system, smooth_iterations=0)
        system.tsdf_manager.cfg["mesh_smooth_iterations"] = 5              # the config default of the system
        _same(system.extract_mesh(), smoothed)
        _same(system.extract_mesh(smooth_iterations=0), plain)
        _same(system.extract_mesh(smooth_boundary="free", smooth_mu=0.0), smooth_mesh(plain, 5, mu=0.0, boundary="free"))
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    _same(smoothed, smooth_mesh(plain, 5))
    V, N, F = _host(smoothed)
    assert sizes == (len(V), len(F)) and len(F) == plain[2].shape[0] and not np.array_equal(V, plain[0].cpu().numpy())
    lv, lf = evaluate.load_mesh(tmp_path / "smoothed.ply")
    assert lv.dtype == np.float32 and np.array_equal(lv, V) and np.array_equal(lf, F)
    assert (tmp_path / "zero.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
