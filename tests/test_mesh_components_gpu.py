"""GPU tests (-m gpu) of mesh_components / filter_mesh (csrc/mesh_components.hip, DESIGN.md "Mesh components") and of
the min_component_faces / keep_largest arguments of the mesh extraction: hand-built meshes and triangle strips against
the numpy statement (tests/cc_numpy.py), analytic shapes that must come apart into themselves, the three-keyframe room
of tests/test_tsdf_mesh_gpu.py, a colour volume, and the product path through SlamSystem.  Everything is integer or a
gather: every comparison is exact.

The room at the volume's default min_weight is ONE component (checked on the CPU with mc_numpy + cc_numpy: 6430 faces,
1 component, also at min_weight 0.05 ... 15), so the room cases extract at min_weight = 40, where thinly observed
voxels drop out and the mesh has 6 components of 5634, 6, 4, 2, 2, 2 faces; min_faces = 5 drops four and keeps two."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cc_numpy as C  # noqa: E402
import mc_numpy as M  # noqa: E402
from mesh_support import VS, _host, _room, _same, _vol  # noqa: E402

pytestmark = pytest.mark.gpu

ROOM_MIN_WEIGHT = 40.0
ROOM_MIN_FACES = 5


def _components(device, faces, V):
    from mast3r_slam.tsdf import mesh_components

    out = mesh_components(torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(device), V)
    for a in out:
        assert a.is_cuda and a.dtype == torch.int32
    return _host(out)


def _roots(vertex_component):
    """Smallest vertex index of each vertex's component, from the dense ids."""
    vc = np.asarray(vertex_component, np.int64)
    if len(vc) == 0:
        return vc
    first = np.full(int(vc.max()) + 1, len(vc), np.int64)
    np.minimum.at(first, vc, np.arange(len(vc)))
    return first[vc]


def _equal_components(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


def _mesh_of(device, V, faces, colors=False):
    """A device mesh tuple over V vertices whose per-vertex rows name their vertex."""
    v = torch.arange(3 * V, dtype=torch.float32, device=device).reshape(V, 3)
    f = torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(device)
    return (v, -v, f) + ((v + 0.5,) if colors else ())


@pytest.mark.parametrize("name", sorted(C.HAND))
def test_hand_built_meshes(device, name):
    from mast3r_slam.tsdf import filter_mesh

    faces, V, root, cfaces, cverts = C.HAND[name]
    got = _components(device, faces, V)
    _equal_components(got, C.components(faces, V))
    assert _roots(got[0]).tolist() == root and got[2].tolist() == cfaces and got[3].tolist() == cverts
    for colors in (False, True):
        mesh = _mesh_of(device, V, faces, colors)
        assert all(a is b for a, b in zip(filter_mesh(mesh), mesh))              # off: the input tensors themselves
        for kw in (dict(min_faces=1), dict(min_faces=2), dict(keep_largest=1), dict(min_faces=1, keep_largest=0)):
            out = filter_mesh(mesh, **kw)
            want = C.filter_mesh(_host(mesh), **kw)
            assert len(out) == len(mesh)
            for a, b in zip(_host(out), want):
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (name, kw)
    if name == "unreferenced":                                                  # vertex 2 goes with min_faces = 1
        out = _host(filter_mesh(_mesh_of(device, V, faces), min_faces=1))
        assert np.array_equal(out[0][:, 0], 3.0 * np.array([0, 1, 3, 4, 5, 6], np.float32))
        assert out[2].tolist() == [[0, 1, 2], [3, 4, 5]]


def test_index_range_is_validated(device):
    from mast3r_slam.tsdf import filter_mesh, mesh_components

    bad = torch.tensor([[0, 1, 3]], dtype=torch.int32, device=device)
    with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
        mesh_components(bad, 3)
    with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
        filter_mesh(_mesh_of(device, 3, [[0, -1, 2]]), min_faces=1)


@pytest.mark.parametrize("numbering", ["reversed", "permuted"])
def test_strip(device, numbering):
    """5 000 faces: no multiple of 256, 20 blocks, 79 waves.  Reversed indices make every link point up the strip, the
    deepest parent chains there are; a fixed random permutation makes them point everywhere."""
    n_f, n_v = 5000, 5002
    rng = np.random.default_rng(11)
    relabel = np.arange(n_v)[::-1] if numbering == "reversed" else rng.permutation(n_v)
    faces = relabel[C.strip(n_f)].astype(np.int32)
    first = _components(device, faces, n_v)
    _equal_components(first, C.components(faces, n_v))
    assert (_roots(first[0]) == 0).all() and first[2].tolist() == [n_f] and first[3].tolist() == [n_v]
    for _ in range(4):                                                          # five calls in all
        _equal_components(_components(device, faces, n_v), first)
    perm = rng.permutation(n_f)
    shuffled = _components(device, faces[perm], n_v)
    assert np.array_equal(shuffled[0], first[0]) and np.array_equal(shuffled[1], first[1][perm])
    # cut in two: labels and counts on both sides of the cut
    cut = np.concatenate([C.strip(n_f)[:2000], C.strip(n_f)[2002:]])
    cut = relabel[cut].astype(np.int32)
    _equal_components(_components(device, cut, n_v), C.components(cut, n_v))


def test_count_forms_agree(device):
    """The wave-aggregated and the one-atomic-per-element counts are the same integers, with runs that end inside a
    wave, at a wave's end and at a block's end."""
    import mslam_hip as _m

    rng = np.random.default_rng(3)
    n_v = 3 * 64 * 5 + 17
    root = np.repeat(np.arange(0, n_v, 7), 7)[:n_v]                             # runs of 7: every wave holds run ends
    root[640:1000] = 640                                                        # and one run over whole waves
    faces = np.concatenate([np.stack([np.arange(n_v)] * 3, 1),                   # first vertices in order: runs of 7
                            np.stack([rng.permutation(n_v)] * 3, 1)[:300]]).astype(np.int32)      # and in no order
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(device)
    f_d, r_d = t(faces), t(root)
    out = []
    for aggregate in (0, 1):
        c = torch.full((2, n_v), -7, dtype=torch.int32, device=device)
        _m.check(_m.lib().mslam_mesh_cc_count(_m.ptr(f_d), len(faces), n_v, _m.ptr(r_d), _m.ptr(c[0]), _m.ptr(c[1]),
                                              aggregate, _m.stream_ptr()), "mesh_cc_count")
        out.append(_host(c))
    assert np.array_equal(out[0], out[1])
    assert np.array_equal(out[0][1], np.bincount(root, minlength=n_v))
    assert np.array_equal(out[0][0], np.bincount(root[faces[:, 0]], minlength=n_v))


# ----------------------------------------------------------------------------------------------------------------------
# analytic shapes: three spheres and a torus in one voxel set
# ----------------------------------------------------------------------------------------------------------------------
SHAPES = [("sphere", (0.0, 0.0, 0.0), 0.2, 2), ("sphere", (0.75, 0.004, -0.007), 0.13, 2),
          ("sphere", (0.3, -0.9, 0.1), 0.31, 2), ("torus", (0.01, 0.9, 0.0), (0.3, 0.1), 0)]


def _shape_voxels(i):
    kind, c, r, _ = SHAPES[i]
    c = np.array(c)
    if kind == "torus":
        ext = np.array([r[0] + r[1], r[0] + r[1], r[1]])
        return M.sample_sdf(M.torus_sdf(c, *r), c - ext, c + ext, VS, 3 * VS)
    return M.sample_sdf(M.sphere_sdf(c, r), c - r, c + r, VS, 3 * VS)


def _union(parts):
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))


def test_analytic_shapes_come_apart(device):
    from mast3r_slam.tsdf import filter_mesh, mesh_from_voxels

    parts = [_shape_voxels(i) for i in range(4)]
    for i in range(4):                                  # at least 3 empty voxels between any two: bounding boxes of keys
        for j in range(i):
            gap = np.maximum(parts[i][0].min(0) - parts[j][0].max(0), parts[j][0].min(0) - parts[i][0].max(0)).max()
            assert gap >= 4, (i, j, gap)
    alone = [mesh_from_voxels(*p, VS, 0.5, device=device) for p in parts]
    n_alone = [int(m[2].shape[0]) for m in alone]
    assert len(set(n_alone)) == 4
    k, t, w = _union(parts)
    vol = _vol(device, 1 << 17)
    vol.load_voxels(k, t, w)
    mesh = vol.extract_mesh(min_weight=0.5)
    V, N, F = _host(mesh)
    vc, fc, cf, cv = _components(device, F, len(V))
    assert len(cf) == 4
    centres = np.array([s[1] for s in SHAPES])
    for c in range(4):                                  # which shape: the one whose centre the component surrounds
        i = int(np.argmin(np.linalg.norm(centres - V[vc == c].astype(np.float64).mean(0), axis=1)))
        assert cf[c] == n_alone[i] and cv[c] == alone[i][0].shape[0], (c, i)
        sub = F[fc == c]
        cnt, consistent = M.edge_use(sub)
        assert (cnt == 2).all() and consistent
        assert M.euler(np.zeros((int(cv[c]), 3)), sub) == SHAPES[i][3]
    order = np.argsort(n_alone)
    small, large = int(order[0]), int(order[-1])
    assert SHAPES[small][0] == "sphere"
    for min_faces in (n_alone[small] + 1, n_alone[order[1]]):           # both ends of the interval
        got = vol.extract_mesh(min_weight=0.5, min_component_faces=min_faces)
        _same(got, mesh_from_voxels(*_union([p for i, p in enumerate(parts) if i != small]), VS, 0.5, device=device))
        _same(got, filter_mesh(mesh, min_faces=min_faces))
    _same(vol.extract_mesh(min_weight=0.5, min_component_faces=n_alone[small]), mesh)       # nothing below: all stay
    _same(vol.extract_mesh(min_weight=0.5, keep_largest=1), alone[large])
    _same(mesh_from_voxels(k, t, w, VS, 0.5, device=device, keep_largest=1), alone[large])
    two = vol.extract_mesh(min_weight=0.5, min_component_faces=n_alone[small] + 1, keep_largest=2)
    _same(two, mesh_from_voxels(*_union([parts[i] for i in order[2:]]), VS, 0.5, device=device))


# ----------------------------------------------------------------------------------------------------------------------
# the three-keyframe room
# ----------------------------------------------------------------------------------------------------------------------
def _unique_is_arange(mesh):
    V, _, F = _host(mesh)[:3]
    assert np.array_equal(np.unique(F), np.arange(len(V)))


def test_room(device):
    from mast3r_slam.tsdf import filter_mesh, mesh_from_voxels

    data = _room()
    big = _vol(device, 1 << 22)
    small = _vol(device, 1 << 14)
    shards = [_vol(device, 1 << 19, shard_id=r, num_shards=2) for r in range(2)]
    for pw, conf, org in data:
        small.maintain(reserve=len(pw) * 10)
        big.integrate(pw, conf, org)
        small.integrate(pw, conf, org)
        for s in shards:
            s.integrate(pw, conf, org, return_fused=False)
    assert 1 << 14 < small.capacity < big.capacity
    mesh = big.extract_mesh(min_weight=ROOM_MIN_WEIGHT)
    V, N, F = _host(mesh)
    got = _components(device, F, len(V))
    want = C.components(F, len(V))
    _equal_components(got, want)
    cf = want[2]
    print(f"room at min_weight {ROOM_MIN_WEIGHT}: V={len(V)} F={len(F)} components={len(cf)} faces={np.sort(cf)[::-1][:12]}")
    assert len(cf) > 1
    assert (cf < ROOM_MIN_FACES).any() and (cf >= ROOM_MIN_FACES).any()          # some dropped, some kept
    filt = big.extract_mesh(min_weight=ROOM_MIN_WEIGHT, min_component_faces=ROOM_MIN_FACES)
    ref = C.filter_mesh((V, N, F), min_faces=ROOM_MIN_FACES)
    assert 0 < filt[2].shape[0] < len(F)
    for a, b in zip(_host(filt), ref):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    _unique_is_arange(filt)
    _same(filt, filter_mesh(mesh, min_faces=ROOM_MIN_FACES))
    _same(filt, big.extract_mesh(min_weight=ROOM_MIN_WEIGHT, min_component_faces=ROOM_MIN_FACES))      # repeated call
    for k in (1, 2):
        top = big.extract_mesh(min_weight=ROOM_MIN_WEIGHT, keep_largest=k)
        for a, b in zip(_host(top), C.filter_mesh((V, N, F), keep_largest=k)):
            assert np.array_equal(a, b)
        _unique_is_arange(top)
    # the default threshold: the mesh as extracted, and one component
    plain = big.extract_mesh()
    assert len(_components(device, _host(plain)[2], plain[0].shape[0])[2]) == 1
    _same(plain, big.extract_mesh(min_component_faces=ROOM_MIN_FACES))
    # grown and rehashed table, and the union of two voxel shards
    _same(filt, small.extract_mesh(min_weight=ROOM_MIN_WEIGHT, min_component_faces=ROOM_MIN_FACES))
    parts = [s.voxels() for s in shards]
    keys, t, w = (np.concatenate([p[j] for p in parts]) for j in range(3))
    _same(filt, mesh_from_voxels(keys, t, w, VS, ROOM_MIN_WEIGHT, device=device, min_component_faces=ROOM_MIN_FACES))


def test_color_volume(device):
    from mast3r_slam.tsdf import global_volume as G

    import color_numpy

    vol = _vol(device, color=True)
    for pw, conf, org in _room():
        vol.integrate(pw, conf, org, colors=color_numpy.texture(pw).astype(np.float32))
    cmesh = vol.extract_mesh(min_weight=ROOM_MIN_WEIGHT, colors=True)
    filt = vol.extract_mesh(min_weight=ROOM_MIN_WEIGHT, colors=True, min_component_faces=ROOM_MIN_FACES)
    assert len(cmesh) == 4 and len(filt) == 4
    V, N, F, col = _host(cmesh)
    vc, fc, cf, _ = C.components(F, len(V))
    kv = (cf >= ROOM_MIN_FACES)[vc]
    assert 0 < kv.sum() < len(V)
    fv, fn, ff, fcol = _host(filt)
    assert np.array_equal(fcol, col[kv]) and np.array_equal(fv, V[kv]) and np.array_equal(fn, N[kv])
    _same(filt[:3], vol.extract_mesh(min_weight=ROOM_MIN_WEIGHT, min_component_faces=ROOM_MIN_FACES))
    # without the new arguments: what _extract (and sample_color) return, nothing else
    direct = G._extract(vol._table, vol.capacity, vol.voxel_size, vol.min_weight, 0.0, vol.device)
    _same(vol.extract_mesh(), direct)
    plain = vol.extract_mesh(colors=True)
    _same(plain[:3], direct)
    assert torch.equal(plain[3], vol.sample_color(direct[0])[0])


# ----------------------------------------------------------------------------------------------------------------------
# product path
# ----------------------------------------------------------------------------------------------------------------------
def test_slam_system_filtered_ply(device, tmp_path, monkeypatch):
    """The run of test_slam_system_mesh_and_ply.  Its mesh is one component at the default min_weight and at most
    others; at min_weight = 12 it has 11, of 5860, 14, 8, 8, 6, 4, 4, 2, 2, 2, 2 faces (measured with cc_numpy), so the
    mesh is taken there and n = 5 drops six of them."""
    from mast3r_slam import evaluate
    from mast3r_slam.config import config
    from mast3r_slam.slam_system import SlamSystem
    from test_slam_system_gpu import RoomModel, _frames

    n, mw = 5, 12.0
    monkeypatch.setitem(config["tracking"], "match_frac_thresh", 0.72)
    tcfg = dict(config["tsdf_global"], enabled=True, pre_icp_iters=0, max_iterations=0, hash_capacity=1 << 18)
    torch.manual_seed(0)
    system = SlamSystem(RoomModel(device), device, frame_group=2, tsdf_global_cfg=tcfg, backend="thread")
    try:
        system.run(_frames(list(range(0, 60, 3)), device))
        plain = system.extract_mesh(min_weight=mw)
        filt = system.extract_mesh(min_weight=mw, min_component_faces=n)
        sizes = evaluate.save_tsdf_mesh(tmp_path, "filtered.ply", system, min_weight=mw, min_component_faces=n)
        evaluate.save_tsdf_mesh(tmp_path, "plain.ply", system, min_weight=mw)
        evaluate.save_tsdf_mesh(tmp_path, "zero.ply", system, min_weight=mw, min_component_faces=0)
        system.tsdf_manager.cfg["mesh_min_component_faces"] = n              # the config default of the system
        _same(system.extract_mesh(min_weight=mw), filt)
        _same(system.extract_mesh(min_weight=mw, min_component_faces=0), plain)
    finally:
        system.shutdown()
    torch.cuda.synchronize()
    V, N, F = _host(filt)
    cf = C.components(_host(plain)[2], plain[0].shape[0])[2]
    print(f"slam mesh: F={plain[2].shape[0]} components={len(cf)} faces={np.sort(cf)[::-1][:12]} -> F'={len(F)}")
    assert sizes == (len(V), len(F)) and 100 < len(F) == int(cf[cf >= n].sum()) < plain[2].shape[0]
    for a, b in zip(_host(filt), C.filter_mesh(_host(plain), min_faces=n)):
        assert np.array_equal(a, b)
    lines, vert, faces = M.parse_ply(tmp_path / "filtered.ply")
    assert len(vert) == len(V) and np.array_equal(faces, F)
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), V)
    assert (tmp_path / "zero.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
