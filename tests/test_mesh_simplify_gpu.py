"""GPU tests (-m gpu) of simplify_mesh (csrc/mesh_simplify.hip, DESIGN.md "Mesh simplification") and of the simplify_cell
/ simplify_position arguments of the mesh extraction, against the numpy statement tests/simplify_numpy.py.

What is compared how: faces and the vertex map are integers and must be equal.  Normals, colours and mean-mode positions
are sequential f64 sums in the statement's order and must be bit-equal.  Quadric positions go through an eigen-solver
(Jacobi on the device, eigh in numpy), both f64 with the used directions' conditioning capped at 1e3, so only the final
f32 rounding can differ: 1 ulp (np.spacing) per coordinate.  A vertex renumbering reorders the sums: positions within
1 ulp there too."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M  # noqa: E402
import simplify_numpy as S  # noqa: E402
from mesh_support import VS, _host, _room, _same, _vol  # noqa: E402

pytestmark = pytest.mark.gpu

ROOM_MIN_WEIGHT = 40.0              # where the room's mesh has small components (tests/test_mesh_components_gpu.py)
ROOM_MIN_FACES = 5
GRID = (71, 73)                     # 5183 vertices, 10080 faces: no multiple of 64 or 256


def _dev(mesh, device):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in mesh)


def _ulps(got, want):
    """Largest |got - want| in units of want's f32 spacing."""
    if got.size == 0:
        return 0.0
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want))).max())


def _check(got, want, position, colors, what=""):
    """got: the host copy of simplify_mesh(..., return_map=True); want: the statement's."""
    assert len(got) == len(want) == 4 + bool(colors)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, what
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[-1], want[-1]), what
    assert np.array_equal(got[1], want[1]), what
    if colors:
        assert np.array_equal(got[3], want[3]), what
    ulps = _ulps(got[0], want[0])
    if ulps > 0:
        print(f"{what} {position}: positions differ by up to {ulps:.3g} ulp")
    assert ulps <= (0.0 if position == "mean" else 1.0), (what, ulps)
    return ulps


def _simplify(mesh_d, c, position, **kw):
    from mast3r_slam.tsdf import simplify_mesh

    out = simplify_mesh(mesh_d, c, position=position, return_map=True, **kw)
    for a in out:
        assert a.is_cuda and a.is_contiguous()
    return _host(out)


@pytest.mark.parametrize("position", ["mean", "quadric"])
@pytest.mark.parametrize("colors", [False, True])
@pytest.mark.parametrize("name", sorted(S.HAND))
def test_hand_built_meshes(device, name, colors, position):
    h = S.HAND[name]
    mesh = S.hand_mesh(name, colors)
    got = _simplify(_dev(mesh, device), h["cell"], position)
    assert got[2].tolist() == h["out_faces"] and got[-1].tolist() == h["vertex_map"]
    _check(got, S.simplify(mesh, h["cell"], position, return_map=True), position, colors, name)
    if "fallback" in h and position == "quadric":                    # the fallback is the mean's value, bit for bit
        fb = np.array(h["fallback"])
        assert np.array_equal(got[0][fb], _simplify(_dev(mesh, device), h["cell"], "mean")[0][fb])
    _check(_simplify(_dev(mesh, device), h["cell"], position, _two_pass=True), got, "mean", colors, name + " two-pass")


def _closed(mesh, euler):
    V, F = mesh[0], mesh[2]
    cnt, consistent = M.edge_use(F)
    assert (cnt == 2).all() and consistent and M.euler(V, F) == euler
    assert np.array_equal(np.unique(F), np.arange(len(V)))


@pytest.mark.parametrize("position", ["mean", "quadric"])
@pytest.mark.parametrize("name,voxels", [("sphere2", 2), ("torus", 2), ("box", 2), ("sphere2", 3)])
def test_analytic_shapes(device, name, voxels, position):
    from mast3r_slam.tsdf import mesh_from_voxels

    c = voxels * VS
    k, t, w = S.shape_voxels(name)
    mesh_d = mesh_from_voxels(k, t, w, VS, 0.5, device=device)
    mesh = _host(mesh_d)
    assert (len(mesh[0]), len(mesh[2])) == S.SHAPES[name][3:5]
    want = S.simplify(mesh, c, position, return_map=True, return_info=True)
    if position == "quadric":                                        # the precondition of the 1-ulp comparison
        lam = want[-1]["eig"]
        assert np.abs(lam / lam[:, 2:3] / S.EIG_REL - 1.0).min() > 1e-6
    got = _simplify(mesh_d, c, position)
    _check(got, want[:-1], position, False, f"{name} c={voxels} voxels")
    _closed(got, S.SHAPES[name][7])
    if voxels == 2:
        assert (len(got[0]), len(got[2])) == S.SHAPES[name][5:7]
    assert (got[-1] >= 0).all()
    # the same through the extraction's own argument
    _same(mesh_from_voxels(k, t, w, VS, 0.5, device=device, simplify_cell=c, simplify_position=position),
          _dev(got[:3], device))


@pytest.fixture(scope="module")
def grid():
    return S.grid_patch(*GRID, seed=7)


@pytest.mark.parametrize("cell,position,colors", [(0.25, "quadric", True), (0.25, "mean", False), (9.0, "quadric", True),
                                                  (9.0, "mean", True), (17.0, "quadric", False), (17.0, "mean", True)])
def test_grid_cluster_sizes(device, grid, cell, position, colors):
    """Vertices are 1 apart with jitter 0.2.  c = 0.25: every cluster is one vertex and every face survives; c = 9 / 17:
    clusters of up to 81 / 289 vertices, beyond one wave / one block of threads' worth of elements."""
    mesh = grid if colors else grid[:3]
    want = S.simplify(mesh, cell, position, return_map=True, return_info=True)
    sizes = np.bincount(want[-1]["cluster"])
    if cell == 0.25:
        assert sizes.max() == 1 and len(want[2]) == len(mesh[2])
    else:
        assert sizes.max() > (64 if cell == 9.0 else 256) and 0 < len(want[2]) < len(mesh[2])
    _check(_simplify(_dev(mesh, device), cell, position), want[:-1], position, colors, f"grid c={cell}")


def test_empty_results(device, grid):
    from mast3r_slam.tsdf import simplify_mesh

    for mesh in (grid, grid[:3]):
        for position in ("mean", "quadric"):
            assert np.bincount(S.simplify(mesh, 200.0, position, return_info=True)[-1]["cluster"]).tolist() == [len(mesh[0])]
            out = simplify_mesh(_dev(mesh, device), 200.0, position=position, return_map=True)      # one cell holds it all
            assert len(out) == len(mesh) + 1
            assert all(a.shape == (0, 3) and a.is_cuda for a in out[:-1]) and out[2].dtype == torch.int32
            assert out[-1].dtype == torch.int32 and (out[-1] == -1).all() and out[-1].shape == (len(mesh[0]),)
    none = tuple(torch.zeros((0, 3), dtype=d, device=device) for d in (torch.float32, torch.float32, torch.int32))
    for mesh in (none, _dev(grid[:2], device) + (none[2],)):            # V = 0; F = 0
        out = simplify_mesh(mesh, 1.0, return_map=True)
        assert all(a.shape == (0, 3) for a in out[:3]) and out[3].shape == (mesh[0].shape[0],) and (out[3] == -1).all()
    same = simplify_mesh(none, 0.0)
    assert all(a is b for a, b in zip(same, none))


def _padded(n, dtype, device, pad=64):
    fill = -77 if dtype in (torch.int32, torch.int64) else 1234.5
    full = torch.full((n + 2 * pad,), fill, dtype=dtype, device=device)
    return full, full[pad:pad + n], fill


@pytest.mark.parametrize("packed", [1, 0])
def test_entry_points_stay_inside_their_buffers(device, grid, packed):
    """The four entry points called directly, every output in a buffer with 64 sentinel words on either side."""
    import mslam_hip as _m

    L, st = _m.lib(), _m.stream_ptr()
    verts, normals, faces, colors = _dev(grid, device)
    V, F, c = len(grid[0]), len(grid[2]), 2.5
    bufs = []

    def out(n, dtype):
        full, view, fill = _padded(n, dtype, device)
        bufs.append((full, n, fill))
        return view

    keys = out(V, torch.int64)
    _m.check(L.mslam_mesh_simplify_keys(_m.ptr(verts), V, c, _m.ptr(keys), st), "keys")
    sorted_keys, vorder = torch.sort(keys, stable=True)
    head = torch.ones(V, dtype=torch.bool, device=device)
    head[1:] = sorted_keys[1:] != sorted_keys[:-1]
    cid = torch.cumsum(head, 0) - 1
    C = int(cid[-1]) + 1
    cluster = torch.empty(V, dtype=torch.int32, device=device)
    cluster[vorder] = cid.to(torch.int32)
    ids = torch.arange(C + 1, device=device)
    vstart = torch.searchsorted(cid, ids)
    tri, key_lo, key_hi, pairs = out(3 * F, torch.int32), out(F, torch.int64), out(F, torch.int64), out(3 * F, torch.int64)
    _m.check(L.mslam_mesh_simplify_faces(_m.ptr(faces), F, V, _m.ptr(cluster), C, packed, _m.ptr(tri), _m.ptr(key_hi),
                                         _m.ptr(key_lo), _m.ptr(pairs), st), "faces")
    if packed:
        assert (key_hi == -77).all()                                 # not written in this mode
        forder = torch.sort(key_lo, stable=True)[1]
    else:
        first = torch.sort(key_lo, stable=True)[1]
        forder = first[torch.sort(key_hi[first], stable=True)[1]]
    sorted_pairs = torch.sort(pairs)[0]
    pstart = torch.searchsorted(sorted_pairs, ids * F)
    pos, nrm, col, fb = (out(3 * C, torch.float32), out(3 * C, torch.float32), out(3 * C, torch.float32),
                         out(C, torch.int32))
    _m.check(L.mslam_mesh_simplify_solve(_m.ptr(verts), _m.ptr(normals), _m.ptr(colors), _m.ptr(faces), F, V, c,
                                         _m.ptr(sorted_keys), _m.ptr(vorder), _m.ptr(vstart), _m.ptr(sorted_pairs),
                                         _m.ptr(pstart), C, 1, _m.ptr(pos), _m.ptr(nrm), _m.ptr(col), _m.ptr(fb), st),
             "solve")
    sorted_tri, keep, ref = out(3 * F, torch.int32), out(F, torch.int32), out(C, torch.int32)
    ref.zero_()
    _m.check(L.mslam_mesh_simplify_mark(_m.ptr(tri), _m.ptr(forder), F, C, _m.ptr(sorted_tri), _m.ptr(keep), _m.ptr(ref),
                                        st), "mark")
    torch.cuda.synchronize()
    for full, n, fill in bufs:
        assert (full[:64] == fill).all() and (full[64 + n:] == fill).all()
    # and what they hold is the statement's
    want = S.simplify(grid, c, "quadric", return_map=True, return_info=True)
    info = want[-1]
    assert np.array_equal(cluster.cpu().numpy(), info["cluster"])
    used = ref.cpu().numpy().astype(bool)
    assert np.array_equal(used, info["referenced"]) and int(keep.sum()) == len(want[2])
    assert np.array_equal(fb.cpu().numpy().astype(bool)[used], info["fallback"])
    assert _ulps(pos.cpu().numpy().reshape(-1, 3)[used], want[0]) <= 1.0
    assert np.array_equal(nrm.cpu().numpy().reshape(-1, 3)[used], want[1])
    assert np.array_equal(col.cpu().numpy().reshape(-1, 3)[used], want[3])
    remap = np.cumsum(used) - 1
    assert np.array_equal(remap[sorted_tri.cpu().numpy().reshape(-1, 3)[keep.cpu().numpy().astype(bool)]], want[2])


@pytest.mark.parametrize("position", ["mean", "quadric"])
def test_invariance(device, grid, position):
    c = 2.5
    rng = np.random.default_rng(5)
    first = _simplify(_dev(grid, device), c, position)
    assert 0 < len(first[2]) < len(grid[2])
    for _ in range(4):                                               # five calls in all
        for a, b in zip(_simplify(_dev(grid, device), c, position), first):
            assert np.array_equal(a, b)
    shuffled = grid[:2] + (grid[2][rng.permutation(len(grid[2]))],) + grid[3:]
    for a, b in zip(_simplify(_dev(shuffled, device), c, position), first):
        assert np.array_equal(a, b)
    perm = rng.permutation(len(grid[0]))
    moved = _simplify(_dev(S.renumber(grid, perm), device), c, position)
    assert np.array_equal(moved[2], first[2]) and np.array_equal(moved[-1][perm], first[-1])
    assert _ulps(moved[0], first[0]) <= 1.0


def test_validation(device):
    """cell_size None or <= 0 means "off" (the input itself, tests/test_mesh_simplify_cpu.py); the sizes that are neither
    off nor usable are NaN and the infinities, -inf included: they raise."""
    from mast3r_slam.tsdf import simplify_mesh

    mesh = S.hand_mesh("fan_duplicate", True)

    def with_vertex(value):
        V = mesh[0].copy()
        V[2, 1] = value
        return _dev((V,) + mesh[1:], device)

    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match=r"vertex coordinates span \[.*\] and are not all finite"):
            simplify_mesh(with_vertex(bad), 1.0)
    with pytest.raises(ValueError, match=r"cells span \[0, 1048576\] at cell_size 1.0, outside \[-1048576, 1048576\)"):
        simplify_mesh(with_vertex(float(1 << 20)), 1.0)
    with pytest.raises(ValueError, match=r"cells span \[-1048577, 1\]"):
        simplify_mesh(with_vertex(-float((1 << 20) + 1)), 1.0)
    ok = simplify_mesh(with_vertex(float((1 << 20) - 1)), 1.0)      # the last cell of the range, and the first
    assert ok[2].shape[0] == 2
    assert simplify_mesh(with_vertex(-float(1 << 20)), 1.0)[2].shape[0] == 2
    with pytest.raises(ValueError, match=r"cells span"):             # cells far smaller than the coordinates
        simplify_mesh(_dev(mesh, device), 1e-7)
    for face, span in (([0, 1, 4], r"\[0, 4\]"), ([0, -1, 2], r"\[-1, 3\]")):
        F = mesh[2].copy()
        F[0] = face
        with pytest.raises(ValueError, match=r"face indices span " + span + r", outside \[0, 4\)"):
            simplify_mesh(_dev(mesh[:2] + (F,) + mesh[3:], device), 1.0)
    for bad in (float("nan"), float("inf"), float("-inf")):          # not "off" and not a size
        with pytest.raises(ValueError, match="cell_size must be finite"):
            simplify_mesh(_dev(mesh, device), bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        simplify_mesh(tuple(torch.from_numpy(a) for a in mesh), 1.0)


@pytest.mark.parametrize("name", ["sphere2", "box"])
def test_quality_through_the_products_metric(device, name):
    from mast3r_slam.tsdf import compare_meshes, mesh_distance, mesh_from_voxels, sample_mesh, simplify_mesh

    c = 2 * VS
    bound = np.sqrt(3.0) * c
    mesh = mesh_from_voxels(*S.shape_voxels(name), VS, 0.5, device=device)
    worst = {}
    for position in ("mean", "quadric"):
        out = simplify_mesh(mesh, c, position=position)
        pts = sample_mesh(out[0], out[2], 2000, seed=1)[0]
        worst[position] = float(mesh_distance(pts, mesh[0], mesh[2])[0].max())
        m = compare_meshes(out, mesh, n_samples=2000, threshold=bound, seed=1)
        print(f"{name} {position}: out->in max {worst[position]:.4f} mean {m['accuracy']:.4f}, in->out mean "
              f"{m['completion']:.4f}")
        assert worst[position] <= bound and m["accuracy"] <= bound and m["precision"] == 1.0
    assert worst["quadric"] < worst["mean"]


# ----------------------------------------------------------------------------------------------------------------------
# product path
# ----------------------------------------------------------------------------------------------------------------------
def test_room(device):
    from mast3r_slam.tsdf import filter_mesh, mesh_from_voxels, simplify_mesh
    from mast3r_slam.tsdf import global_volume as G

    c = 2 * VS
    big = _vol(device, 1 << 22)
    shards = [_vol(device, 1 << 19, shard_id=r, num_shards=2) for r in range(2)]
    for pw, conf, org in _room():
        big.integrate(pw, conf, org)
        for s in shards:
            s.integrate(pw, conf, org, return_fused=False)
    plain = big.extract_mesh()
    _same(plain, G._extract(big._table, big.capacity, big.voxel_size, big.min_weight, 0.0, big.device))     # as today
    _same(plain, big.extract_mesh(simplify_cell=0.0))
    for position in ("quadric", "mean"):
        simp = big.extract_mesh(simplify_cell=c, simplify_position=position)
        assert 0 < simp[2].shape[0] < plain[2].shape[0]
        _same(simp, simplify_mesh(plain, c, position=position))
        got = _host(simplify_mesh(plain, c, position=position, return_map=True))
        _check(got, S.simplify(_host(plain), c, position, return_map=True), position, False, "room")
        assert np.array_equal(np.unique(got[2]), np.arange(len(got[0])))
    print(f"room: V={plain[0].shape[0]} F={plain[2].shape[0]} -> V'={simp[0].shape[0]} F'={simp[2].shape[0]}")
    # filter first, then simplify
    raw = big.extract_mesh(min_weight=ROOM_MIN_WEIGHT)
    filt = filter_mesh(raw, min_faces=ROOM_MIN_FACES)
    assert filt[2].shape[0] < raw[2].shape[0]
    both = big.extract_mesh(min_weight=ROOM_MIN_WEIGHT, min_component_faces=ROOM_MIN_FACES, simplify_cell=c)
    _same(both, simplify_mesh(filt, c))
    # the union of two voxel shards
    parts = [s.voxels() for s in shards]
    keys, t, w = (np.concatenate([p[j] for p in parts]) for j in range(3))
    _same(both, mesh_from_voxels(keys, t, w, VS, ROOM_MIN_WEIGHT, device=device, min_component_faces=ROOM_MIN_FACES,
                                 simplify_cell=c))


def test_color_volume(device):
    import color_numpy
    from mast3r_slam.tsdf import simplify_mesh

    c = 2 * VS
    vol = _vol(device, color=True)
    for pw, conf, org in _room():
        vol.integrate(pw, conf, org, colors=color_numpy.texture(pw).astype(np.float32))
    cmesh = vol.extract_mesh(colors=True)
    simp = vol.extract_mesh(colors=True, simplify_cell=c)
    assert len(cmesh) == 4 and len(simp) == 4 and simp[3].shape == simp[0].shape
    assert 0 < simp[0].shape[0] < cmesh[0].shape[0]
    assert float(simp[3].min()) >= 0.0 and float(simp[3].max()) <= 1.0
    _same(simp, simplify_mesh(cmesh, c))
    _check(_simplify(cmesh, c, "quadric"), S.simplify(_host(cmesh), c, return_map=True), "quadric", True, "colour room")
    _same(simp[:3], vol.extract_mesh(simplify_cell=c))


def test_slam_system_simplified_ply(device, tmp_path, monkeypatch):
    """The run of test_slam_system_mesh_and_ply."""
    from mast3r_slam import evaluate
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from mast3r_slam.tsdf import simplify_mesh
    from test_slam_system_gpu import RoomModel, _frames

    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    assert tcfg["mesh_simplify_voxels"] == 0.0
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    try:
        system.run(_frames(list(range(0, 60, 3)), device))
        vs = float(system.tsdf_manager.volume.voxel_size)
        plain = system.extract_mesh()
        simp = system.extract_mesh(simplify_cell=2 * vs)
        sizes = evaluate.save_tsdf_mesh(tmp_path, "simplified.ply", system, simplify_cell=2 * vs)
        evaluate.save_tsdf_mesh(tmp_path, "plain.ply", system)
        evaluate.save_tsdf_mesh(tmp_path, "zero.ply", system, simplify_cell=0.0)
        system.tsdf_manager.cfg["mesh_simplify_voxels"] = 2.0               # the config default of the system
        _same(system.extract_mesh(), simp)
        _same(system.extract_mesh(simplify_cell=0.0), plain)
        _same(system.extract_mesh(simplify_position="mean"), simplify_mesh(plain, 2 * vs, position="mean"))
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    _same(simp, simplify_mesh(plain, 2 * vs))
    V, N, F = _host(simp)
    assert sizes == (len(V), len(F)) and 0 < len(F) < plain[2].shape[0]
    lv, lf = evaluate.load_mesh(tmp_path / "simplified.ply")
    assert lv.dtype == np.float32 and np.array_equal(lv, V) and np.array_equal(lf, F)
    assert (tmp_path / "zero.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
