"""The definition of mesh decimation (tests/decimate_numpy.py, DESIGN.md "Mesh decimation") judged on its own, without a
device: the four analytic fixtures at the face counts that clustering reaches, what it keeps on flat and thin geometry
where clustering cannot, the error gate, open rims, hand meshes, the tie-break and the selection's three hops.
tests/test_mesh_decimate_gpu.py then holds the kernels to it bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimate_numpy as Q  # noqa: E402
import meshdist_numpy as D  # noqa: E402
import simplify_numpy as S  # noqa: E402
import smooth_numpy as T  # noqa: E402

RADIUS = 0.1                        # beyond every distance measured here; out_to_in is exact within it
CURVED_BAR = 2.5                    # decimation's out->in over clustering's on the curved fixtures (measured: 1.99, 1.05)


def _vertex_dist(points, mesh):
    """Exact distance f64[n] from every point to the mesh (brute force over all faces)."""
    a, b, c, valid = D.triangles(mesh[0], mesh[2])
    a, b, c = a[valid], b[valid], c[valid]
    p = np.asarray(points, np.float64)
    pi, fi = np.divmod(np.arange(len(p) * len(a)), len(a))
    return np.sqrt(D.tri_dist2(p[pi], a[fi], b[fi], c[fi]).reshape(len(p), len(a)).min(1))


def _one_sided(src, dst):
    """The largest distance found from `src` to `dst`: over 2000 area-weighted samples and over every vertex `src` uses."""
    used = np.unique(src[2])
    return max(float(S.out_to_in(src, dst, RADIUS).max()), float(_vertex_dist(src[0][used], dst).max()))


def _subset_in_order(out, mesh, vmap):
    """src i64[V']: the input vertex every output vertex is, bit for bit, with its normal (and colour), in input order;
    found among the vertices the map sends there (the fixtures have no two vertices at one position)."""
    src = np.full(len(out[0]), -1)
    for w in np.nonzero(vmap >= 0)[0]:
        if mesh[0][w].tobytes() == out[0][vmap[w]].tobytes():
            assert src[vmap[w]] < 0
            src[vmap[w]] = w
    assert (src >= 0).all() and (np.diff(src) > 0).all()
    for k in [0, 1] + ([3] if len(mesh) == 4 else []):
        assert out[k].dtype == np.float32 and out[k].tobytes() == mesh[k][src].tobytes()
    assert (vmap[src] == np.arange(len(src))).all()
    return src


@pytest.mark.parametrize("name", ["sphere2", "torus", "box", "plate"])
def test_fixtures_at_their_targets(name):
    mesh = Q.fixture(name)
    target = Q.TARGETS[name]
    V, N, F, vmap, info = Q.fixture_reference(name)
    print(f"{name}: {len(mesh[0])} / {len(mesh[2])} -> {len(V)} / {len(F)} in {info['rounds']} rounds, "
          f"largest accepted cost {info['max_cost']:.3e}")
    assert target - 1 <= len(F) <= target
    assert Q.topology(mesh[2], len(mesh[0])) == (True, True, Q.EULER[name])
    assert Q.topology(F, len(V)) == (True, True, Q.EULER[name])
    assert len(np.unique(F)) == len(V) and len(np.unique(F, axis=0)) == len(F)
    src = _subset_in_order((V, N, F), mesh, vmap)
    # the map composes: following the traced collapses from any vertex ends where the map says
    end = np.arange(len(mesh[0]))
    for r in info["trace"]:
        step = np.arange(len(end))
        step[r["u"]] = r["v"]
        end = step[end]
    assert (vmap >= 0).all() and np.array_equal(src[vmap], end)
    assert int(info["collapses"].sum()) * 2 == len(mesh[2]) - len(F) and len(info["collapses"]) == info["rounds"]
    assert info["removable"].all() and not info["boundary"].any()


@pytest.mark.parametrize("name", ["box", "plate"])
def test_flat_and_thin_geometry_is_exact_where_clustering_is_not(name):
    """Flat sides need zero-cost collapses only: both one-sided distances stay at rounding level.  Clustering at the same
    face count cuts the edges off the box and squeezes the 1.3-voxel plate: more than 0.01 m."""
    mesh = Q.fixture(name)
    out = Q.fixture_reference(name)[:3]
    cl = S.simplify(mesh, 2 * S.VS)
    assert len(cl[2]) == Q.TARGETS[name]
    ours = (_one_sided(out, mesh), _one_sided(mesh, out))
    theirs = (_one_sided(cl, mesh), _one_sided(mesh, cl))
    print(f"{name}: decimation out->in {ours[0]:.3e} in->out {ours[1]:.3e}; clustering at {len(cl[2])} faces "
          f"{theirs[0]:.5f} / {theirs[1]:.5f}")
    assert max(ours) <= 1e-6
    assert max(theirs) > 0.01


@pytest.mark.parametrize("name", ["sphere2", "torus"])
def test_curved_shapes_against_clustering(name):
    """Subset placement is no better than clustering on curved shapes; it must not be much worse."""
    mesh = Q.fixture(name)
    out = Q.fixture_reference(name)[:3]
    cl = S.shape_reference(name, 2, "quadric")[:3]
    assert len(cl[2]) == Q.TARGETS[name]
    ours, theirs = float(S.out_to_in(out, mesh, RADIUS).max()), float(S.out_to_in(cl, mesh, RADIUS).max())
    print(f"{name}: max out->in {ours:.5f} against clustering's {theirs:.5f}: {ours / theirs:.3f} x")
    assert ours <= CURVED_BAR * theirs


def test_max_error_on_the_sphere():
    mesh = Q.fixture("sphere2")
    counts = []
    for e in (0.02, 0.05, 0.1):
        V, N, F, info = Q.decimate(mesh, max_error=e * S.VS, return_info=True, trace=True)
        far = float(S.out_to_in((V, N, F), mesh, RADIUS).max())
        print(f"sphere2 max_error {e} VS: {len(F)} faces in {info['rounds']} rounds, max out->in {far / S.VS:.3f} VS")
        counts.append(len(F))
        e2 = np.float64(e * S.VS) * np.float64(e * S.VS)
        assert info["trace"]
        for r in info["trace"]:
            assert (r["cost"] <= e2 * r["area"]).all()
        assert info["max_cost"] == max(float(r["cost"].max()) for r in info["trace"])
        assert Q.topology(F, len(V)) == (True, True, 2)
    assert counts[0] > counts[1] > counts[2] and counts[0] < len(mesh[2])


def test_open_cap_keeps_its_rim():
    V, N, F = T.sphere_cap()
    vclass, _, _ = T.classify(F, len(V))
    rim = np.nonzero(vclass == T.BOUNDARY)[0]
    assert len(rim) == 88
    oV, oN, oF, vmap, info = Q.decimate((V, N, F), ratio=0.25, return_map=True, return_info=True)
    assert np.array_equal(info["boundary"], vclass == T.BOUNDARY) and not info["removable"][rim].any()
    assert len(oF) < len(F) // 2
    assert (vmap[rim] >= 0).all() and oV[vmap[rim]].tobytes() == V[rim].tobytes()

    def rim_edges(faces, nv, names):
        row_start, nbr, mult = T.adjacency(faces, nv)
        rows = np.repeat(np.arange(nv), np.diff(row_start))
        return sorted((int(names[a]), int(names[b])) for a, b in zip(rows[mult == 1], nbr[mult == 1]))

    back = np.full(len(oV), -1)
    back[vmap[vmap >= 0]] = np.nonzero(vmap >= 0)[0]                 # any input vertex of the chain ...
    back[vmap[rim]] = rim                                            # ... the rim vertex itself on the rim
    assert rim_edges(oF, len(oV), back) == rim_edges(F, len(V), np.arange(len(V)))


def _flat(V, F):
    """(vertices, normals +z, faces) of a flat hand mesh."""
    return V, np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (len(V), 1)), F


def test_hand_meshes():
    tet = T.hand_mesh("tetrahedron")
    out = Q.decimate(tet, 0, return_map=True, return_info=True)      # every vertex is removable, no link condition holds
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out[:3], tet)) and out[4]["rounds"] == 0
    assert out[4]["removable"].all() and np.array_equal(out[3], np.arange(4))
    fan = _flat(*Q.disc(1))                                          # the centre goes into rim vertex 1, the lowest v
    oV, oN, oF, vmap, info = Q.decimate(fan, 0, return_map=True, return_info=True)
    assert info["removable"].tolist() == [True] + [False] * 6 and info["boundary"].tolist() == [False] + [True] * 6
    assert info["collapses"].tolist() == [1] and info["max_cost"] == 0.0
    assert oV.tobytes() == fan[0][1:].tobytes() and vmap.tolist() == [0, 0, 1, 2, 3, 4, 5]
    assert oF.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5]]
    disc = _flat(*Q.disc(2))                                         # the centre and the inner ring are interior
    assert Q.topology(disc[2], len(disc[0]))[1]
    oV, oN, oF, vmap, info = Q.decimate(disc, 0, return_map=True, return_info=True)
    assert info["removable"][:7].all() and info["boundary"][7:].all() and not info["removable"][7:].any()
    assert info["rounds"] >= 1 and 2 * int(info["collapses"].sum()) == len(disc[2]) - len(oF) >= 10
    assert oV[vmap[7:]].tobytes() == disc[0][7:].tobytes() and (vmap >= 0).all() and Q.topology(oF, len(oV))[1]
    one = Q.decimate(disc, len(disc[2]) - 2)                         # one collapse is all that is asked for
    assert len(one[2]) == len(disc[2]) - 2 and len(one[0]) == len(disc[0]) - 1
    for name in ("bow_tie", "three_on_an_edge", "triangle", "two_triangles", "duplicated_face"):
        mesh = T.hand_mesh(name, colors=True)
        out = Q.decimate(mesh, 0, return_info=True)
        # the face given twice passes for a closed surface, but its vertices have one common neighbour, not two
        assert out[4]["rounds"] == 0 and out[4]["removable"].any() == (name == "duplicated_face"), name
        assert all(a.tobytes() == b.tobytes() for a, b in zip(out[:4], mesh)), name
    # a repeated-index face and an isolated vertex: neither counts; once something is asked for they are dropped
    mesh = T.hand_mesh("repeated_index")
    out = Q.decimate(mesh, 0, return_map=True)
    assert out[2].tolist() == [[0, 1, 2]] and out[0].tobytes() == mesh[0][:3].tobytes() and out[3].tolist() == [0, 1, 2, -1]
    mesh = T.hand_mesh("isolated_vertex")
    out = Q.decimate(mesh, 0, return_map=True)
    assert len(out[0]) == 4 and out[3].tolist() == [0, 1, 2, 3, -1] and np.array_equal(out[2], mesh[2])
    # target_faces >= F: the input itself
    for target in (len(disc[2]), len(disc[2]) + 5):
        same = Q.decimate(disc, target, return_map=True)
        assert all(a is b for a, b in zip(same[:3], disc)) and np.array_equal(same[3], np.arange(len(disc[0])))
    assert all(a is b for a, b in zip(Q.decimate(disc, ratio=1.0), disc))


def test_flip_test_refuses_a_collapse():
    """decimate_numpy.notched_fan: coplanar faces around vertex 0 whose rim is not convex, so that 0 -> 1 and 0 -> 2 turn
    a face over while 0 -> 3 does not; every cost is zero, so only the flip test can tell them apart."""
    mesh = _flat(*Q.notched_fan())
    p = mesh[0].astype(np.float64)
    for f in mesh[2]:                                                # a valid flat mesh: every face counter-clockwise
        assert np.cross(p[f[1]] - p[f[0]], p[f[2]] - p[f[0]])[2] > 0
    cur = mesh[2].astype(np.int64)
    tab = Q.candidates(p, cur, Q.initial_state(p, cur), None)
    assert tab["removable"][0]

    def flips(u, v):
        faces = cur[(cur == u).any(1) & ~(cur == v).any(1)]
        new = np.where(faces == u, v, faces)
        return bool((np.cross(p[new[:, 1]] - p[new[:, 0]], p[new[:, 2]] - p[new[:, 0]])[:, 2] <= 0).any())

    assert flips(0, 1) and flips(0, 2) and not flips(0, 3)           # worked out by hand in notched_fan's terms
    # every cost is zero, so best(0) is the lowest valid v; 1 and 2 have two common neighbours with 0 like any rim
    # vertex of a fan, so it is the flip test alone that refused them
    assert int(tab["best"][0]) == 3 and tab["cost"][0] == 0.0
    out = Q.decimate(mesh, 0)
    o = out[0].astype(np.float64)
    assert (np.cross(o[out[2][:, 1]] - o[out[2][:, 0]], o[out[2][:, 2]] - o[out[2][:, 0]])[:, 2] > 0).all()


def _flat_grid(nx, ny, seed):
    P, N, F, C = S.grid_patch(nx, ny, seed)
    P = P.copy()
    P[:, 2] = 1.0                                                    # in-plane jitter only: every cost is exactly zero
    return P, N, F, C


def test_hashed_ties_keep_the_rounds_short():
    mesh = _flat_grid(24, 24, seed=3)
    target = len(mesh[2]) // 4
    hashed = Q.decimate(mesh, target, return_info=True)
    by_index = Q.decimate(mesh, target, return_info=True, tie="index")
    print(f"flat 24 x 24 grid to {target} faces: {hashed[-1]['rounds']} rounds with hashed ties, "
          f"{by_index[-1]['rounds']} with index ties")
    assert hashed[-1]["max_cost"] == 0.0 and by_index[-1]["max_cost"] == 0.0
    assert target - 1 <= len(hashed[2]) <= target and target - 1 <= len(by_index[2]) <= target
    assert 3 * hashed[-1]["rounds"] <= by_index[-1]["rounds"]


@pytest.mark.parametrize("name", ["sphere2", "box", "plate", "torus"])
def test_selected_vertices_are_three_hops_apart(name):
    nv = len(Q.fixture(name)[0])
    trace = Q.fixture_reference(name)[-1]["trace"]
    assert len(trace) > 20
    for r in trace:
        assert len(r["u"]) and Q.hops_apart(r["faces"], nv, r["u"])
        assert not np.isin(r["v"], r["u"]).any() and len(np.unique(r["v"])) == len(r["v"])
    assert not Q.hops_apart(trace[0]["faces"], nv, trace[0]["faces"][0, :2])       # the check itself: two neighbours


def test_hash_is_the_documented_mix():
    assert int(Q.hash32(0, 0)) == 0 and len(set(Q.hash32(np.arange(1000), 5).tolist())) == 1000
    x = (1 * 0x9E3779B1 + 3 * 0x85EBCA77) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(Q.hash32(1, 3)) == x and int(Q.hash32(2 ** 31 - 1, 200)) < 2 ** 32


def test_argument_errors():
    mesh = T.hand_mesh("tetrahedron")
    with pytest.raises(ValueError, match="one of target_faces, ratio and max_error"):
        Q.decimate(mesh)


def test_keywords_exist_without_a_device(tmp_path):
    import inspect

    import torch

    import mslam_hip
    from mast3r_slam import evaluate, tsdf
    from mast3r_slam.config import config

    assert config["tsdf_global"]["mesh_decimate_faces"] == 0 and config["tsdf_global"]["mesh_decimate_error"] == 0.0
    declared = mslam_hip.exported_symbols()
    for s in ("state", "candidates", "spread", "apply", "finish"):
        assert "mslam_mesh_decimate_" + s in declared and hasattr(mslam_hip.lib(), "mslam_mesh_decimate_" + s), s
    assert mslam_hip.header_constants()["MSLAM_MESH_DECIMATE_STATE"] == 11
    # the three arguments of the five export functions, and the shape of their signatures: test_mesh_chain_cpu.py
    assert inspect.signature(tsdf.decimate_mesh).parameters["target_faces"].default is None
    mesh = (torch.zeros(3, 3), torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32))
    for kw, msg in ((dict(), "one of target_faces, ratio and max_error is needed"),
                    (dict(target_faces=-1), "target_faces must be >= 0"),
                    (dict(target_faces=1.5), "target_faces must be an integer"),
                    (dict(ratio=0.0), r"ratio must be in \(0, 1\]"), (dict(ratio=1.5), r"ratio must be in \(0, 1\]"),
                    (dict(ratio=float("nan")), r"ratio must be in \(0, 1\]"),
                    (dict(max_error=-1e-3), "max_error must be finite and >= 0"),
                    (dict(max_error=float("nan")), "max_error must be finite and >= 0"),
                    (dict(max_error=float("inf")), "max_error must be finite and >= 0")):
        with pytest.raises(ValueError, match="decimate_mesh: " + msg):
            tsdf.decimate_mesh(mesh, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsdf.decimate_mesh(mesh, 1)

    class Source:
        def extract_mesh(self, **kw):
            self.kw = kw
            raise LookupError

    src = Source()
    for given, passed in ((dict(decimate_faces=500), dict(decimate_faces=500)), (dict(decimate_faces=0), {}),
                          (dict(decimate_ratio=0.2), dict(decimate_ratio=0.2)),
                          (dict(decimate_error=0.01, simplify_cell=0.06),
                           dict(simplify_cell=0.06, simplify_position="quadric", decimate_error=0.01)),
                          (dict(decimate_faces=None, decimate_ratio=None, decimate_error=None), {})):
        with pytest.raises(LookupError):
            evaluate.save_tsdf_mesh(tmp_path, "mesh.ply", src, **given)
        assert src.kw == dict(min_weight=None, level=0.0, **passed), given
    with pytest.raises(TypeError, match="unexpected keyword argument 'decimate_face'"):
        evaluate.save_tsdf_mesh(tmp_path, "mesh.ply", src, decimate_face=500)


def test_manager_and_system_pass_the_arguments_on():
    import types

    from mast3r_slam import tsdf
    from mast3r_slam.slam_system import SlamSystem

    calls = []
    volume = types.SimpleNamespace(voxel_size=0.03, extract_mesh=lambda **kw: calls.append(kw) or "mesh")
    manager = types.SimpleNamespace(volume=volume, cfg={})
    manager.extract_mesh = lambda **kw: tsdf.TSDFGlobalManager.extract_mesh(manager, **kw)
    base = dict(min_weight=None, level=0.0)
    for given, passed in (({}, {}), (dict(decimate_faces=0, decimate_error=0.0), {}),
                          (dict(decimate_faces=300), dict(colors=False, decimate_faces=300)),
                          (dict(decimate_ratio=0.5, decimate_error=0.002),
                           dict(colors=False, decimate_ratio=0.5, decimate_error=0.002))):
        assert manager.extract_mesh(**given) == "mesh" and calls.pop() == dict(base, **passed), given
    system = types.SimpleNamespace(tsdf_manager=manager, drain=lambda: None)
    for cfg, given, passed in (({}, {}, {}),
                               (dict(mesh_decimate_faces=1000), {}, dict(colors=False, decimate_faces=1000)),
                               (dict(mesh_decimate_faces=1000), dict(decimate_faces=0), {}),
                               (dict(mesh_decimate_error=0.5), {}, dict(colors=False, decimate_error=0.5 * 0.03)),
                               (dict(mesh_decimate_error=0.5), dict(decimate_error=0.0, decimate_ratio=0.1),
                                dict(colors=False, decimate_ratio=0.1))):
        manager.cfg = cfg
        assert SlamSystem.extract_mesh(system, **given) == "mesh" and calls.pop() == dict(base, **passed), (cfg, given)
