"""GPU tests (-m gpu) of the bow-tie mode of mesh_boundaries and fill_holes (bowties=True; csrc/mesh_holes.hip, DESIGN.md
"Mesh holes") and of the fill_bowties argument of the mesh extraction, against the numpy statement tests/bowtie_numpy.py.

Everything is compared byte for byte, as in test_mesh_holes_gpu.py: the pairing is combinatorial, and what follows it is
the plain mode's arithmetic."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bowtie_numpy as BT  # noqa: E402
import holes_numpy as H  # noqa: E402
from mesh_support import VS, _host, _room, _same, _vol  # noqa: E402

pytestmark = pytest.mark.gpu

INFO = ("loop_id", "loop_head", "loop_length", "dart", "dart_tail", "dart_head", "dart_loop", "loop_perimeter",
        "loop_filled")
PLAIN_KEYS = {"loop_id", "loop_length", "dart", "dart_tail", "dart_head", "dart_loop", "n_boundary_edges", "n_open"}


def _dev(mesh, device):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in mesh)


def _bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()))


def _views(mesh, device):
    """The mesh as non-contiguous device views: columns 1:4 of a wider tensor, every other row, a transposed copy."""
    V = len(mesh[0])
    wide = torch.zeros((V, 5), dtype=torch.float32, device=device)
    wide[:, 1:4] = torch.from_numpy(mesh[0]).to(device)
    every_other = torch.zeros((2 * V, 3), dtype=torch.float32, device=device)
    every_other[::2] = torch.from_numpy(mesh[1]).to(device)
    faces_t = torch.from_numpy(np.ascontiguousarray(mesh[2].T)).to(device).T
    out = (wide[:, 1:4], every_other[::2], faces_t)
    if len(mesh) == 4:
        cols = torch.zeros((V, 6), dtype=torch.float32, device=device)
        cols[:, ::2] = torch.from_numpy(mesh[3]).to(device)
        out += (cols[:, ::2],)
    return out


def _check_info(info, want, what, keys=INFO):
    for k in keys:
        _bytes(info[k].cpu().numpy(), want[k], f"{what} {k}")
    for k in ("n_boundary_edges", "n_open"):
        assert int(info[k]) == want[k], (what, k, int(info[k]), want[k])


def _check(mesh, device, max_edges, what, mesh_d=None, want=None, colours=True):
    """fill_holes and mesh_boundaries in bow-tie mode against the statement, every tensor and every info entry byte for
    byte; `colours`: once more without the colours."""
    from mast3r_slam.tsdf import fill_holes, mesh_boundaries

    mesh_d = _dev(mesh, device) if mesh_d is None else mesh_d
    want = BT.fill(mesh, max_edges, return_info=True) if want is None else want
    out = fill_holes(mesh_d, max_edges, return_info=True, bowties=True)
    assert len(out) == len(mesh) + 1 and set(out[-1]) == set(want[-1])
    for k in range(len(mesh)):
        _bytes(out[k].cpu().numpy(), want[k], f"{what} tensor {k}")
    _check_info(out[-1], want[-1], what)
    if not want[-1]["loop_filled"].any():
        assert all(a is b for a, b in zip(out[:-1], mesh_d))
    plain = fill_holes(mesh_d, max_edges, bowties=True)
    assert len(plain) == len(mesh) and all(torch.equal(a, b) for a, b in zip(plain, out))
    nv = len(mesh[0])
    _check_info(mesh_boundaries(mesh_d[2], nv, mesh_d[0], bowties=True), want[-1], what + " boundaries", INFO[:-1])
    bare = mesh_boundaries(mesh_d[2], nv, bowties=True)
    assert "loop_perimeter" not in bare and "loop_head" in bare
    _check_info(bare, want[-1], what + " boundaries without vertices", INFO[:-2])
    if colours and len(mesh) == 4:
        short = fill_holes(mesh_d[:3], max_edges, return_info=True, bowties=True)
        assert len(short) == 4
        for k in range(3):
            _bytes(short[k].cpu().numpy(), want[k], f"{what} without colours, tensor {k}")
        _check_info(short[-1], want[-1], what + " without colours")
    return out


def _lengths(out):
    return sorted(out[-1]["loop_length"].tolist())


@pytest.mark.parametrize("colors", [False, True])
@pytest.mark.parametrize("name", H.HAND)
def test_hand_meshes(device, name, colors):
    mesh = H.hand_mesh(name, colors)
    want = BT.fill(mesh, 16, return_info=True)
    out = _check(mesh, device, 16, name, want=want)
    _check(mesh, device, 16, name + " views", mesh_d=_views(mesh, device), want=want)
    if name == "bow_tie":
        assert _lengths(out) == [3, 3] and int(out[-1]["n_open"]) == 0
    if name == "three_on_an_edge":
        assert _lengths(out) == [] and int(out[-1]["n_open"]) == 6


def test_two_loops_with_the_same_smallest_vertex(device):
    """Two triangles that share their smallest vertex: the same loop_id, told apart by loop_head."""
    V = H.hand_mesh("bow_tie", True)[0]
    mesh = H.with_attributes(V[[2, 1, 0, 3, 4]], [[2, 1, 0], [0, 4, 3]])
    out = _check(mesh, device, 16, "mirrored bow-tie")
    assert out[-1]["loop_id"].tolist() == [0, 0] and out[-1]["loop_head"].tolist() == [2, 4]
    assert sorted(out[-1]["dart_loop"].tolist()) == [0, 0, 0, 1, 1, 1]


GRIDS = {
    "two diagonal": (lambda: H.grid(4, 4, [(1, 1), (2, 2)]), [4, 4, 16], 2),
    "three diagonal": (lambda: H.grid(5, 5, [(1, 1), (2, 2), (3, 3)], jitter=0.05), [4, 4, 4, 20], 3),
    "four around one": (lambda: H.grid(5, 5, [(1, 2), (2, 1), (2, 3), (3, 2)]), [4, 12, 20], 1),    # 4: an island's rim
    "corner": (lambda: H.grid(3, 3, [(0, 0), (1, 1)]), [4, 12], 1),
    "three gaps about a vertex": (lambda: BT.gapped_fan(6, [0, 2, 4]), [3, 3, 3, 6], 3),
    "two sheets": (BT.two_sheets, [8, 8], 0),
}


@pytest.mark.parametrize("name", list(GRIDS))
def test_grids(device, name):
    make, lengths, n_filled = GRIDS[name]
    mesh = make()
    out = _check(mesh, device, 16, name)
    assert _lengths(out) == lengths and int(out[-1]["n_open"]) == 0
    assert int(out[-1]["loop_filled"].sum()) == n_filled
    _check(mesh, device, 16, name + " views", mesh_d=_views(mesh, device), colours=False)


def test_bad_winding(device):
    """One flipped face: the rotation is bounded and crosses an edge only when it and its reverse occur exactly once, so
    the call returns what the statement says."""
    out = _check(BT.bad_winding(), device, 16, "bad winding")
    assert _lengths(out) == [4, 4] and int(out[-1]["n_open"]) == 16


@pytest.mark.parametrize("n", [3, 33, 70])
def test_welded_rings(device, n):
    """B = 4 n darts, no power of two; the loops of 33 lie within a wave, those of 70 cross one and the 64-dart round of
    the doubling."""
    out = _check(BT.welded_rings(n), device, 80, f"welded rings {n}")
    assert _lengths(out) == [n] * 4 and int(out[-1]["n_open"]) == 0
    assert out[-1]["loop_id"].tolist()[:2] == [0, 0]


@pytest.mark.parametrize("a", [8, 9, 17])
def test_long_figure_of_eight(device, a):
    """One closed fan walk of 8 a darts (64, 72, 136) that is cut into two loops of 4 a at its only repeated vertex."""
    out = _check(BT.diagonal_squares(a), device, 80, f"diagonal squares {a}", colours=False)
    assert _lengths(out) == [4 * a, 4 * a, 4 * (2 * a + 2)] and int(out[-1]["n_open"]) == 0
    assert int(out[-1]["loop_filled"].sum()) == 2


@pytest.mark.parametrize("B", [255, 256, 257])
def test_dart_counts_at_block_edges(device, B):
    mesh = H.join(H.strip(B - 24), H.grid(4, 4, [(1, 1), (2, 2)]))
    out = _check(mesh, device, 16, f"B = {B}", colours=False)
    assert int(out[-1]["n_boundary_edges"]) == B and _lengths(out) == [4, 4, 16, B - 24]
    assert int(out[-1]["loop_filled"].sum()) == 2


def test_more_loops_than_a_block(device):
    mesh = BT.hole_pairs(17)
    out = _check(mesh, device, 4, "17 x 17 pairs of holes", colours=False)
    assert out[-1]["loop_id"].shape[0] == 579 and int(out[-1]["loop_filled"].sum()) == 578
    assert int(out[-1]["n_open"]) == 0 and out[2].shape[0] == len(mesh[2]) + 4 * 578


def test_long_fan(device):
    """600 faces about one vertex with two gaps: one lane rotates through 299 faces to find its successor."""
    out = _check(BT.gapped_fan(600, [0, 300]), device, 16, "fan of 600", colours=False)
    assert _lengths(out) == [3, 3, 600] and int(out[-1]["n_open"]) == 0


@pytest.mark.parametrize("name", ["two diagonal", "three gaps about a vertex", "sphere"])
def test_face_order_and_corner_rotation(device, name):
    mesh = _sphere(0)[0] if name == "sphere" else GRIDS[name][0]()
    cap = 64 if name == "sphere" else 16
    a = _check(mesh, device, cap, name, want=_sphere(0)[1] if name == "sphere" else None, colours=False)
    b = _check(BT.reordered(mesh, 7), device, cap, name + " reordered", colours=False)
    nf = len(mesh[2])
    assert a[0].shape[0] > len(mesh[0])
    for k in range(len(mesh)):
        if k != 2:
            assert torch.equal(a[k], b[k])
    assert torch.equal(a[2][nf:], b[2][nf:])
    for k in ("loop_id", "loop_head", "loop_length", "loop_filled", "loop_perimeter"):
        _bytes(a[-1][k].cpu().numpy(), b[-1][k].cpu().numpy(), k)


@functools.lru_cache(maxsize=None)
def _sphere(seed):
    mesh = H.sphere_mesh(seed, 200)
    return mesh, BT.fill(mesh, 64, return_info=True)


@pytest.mark.parametrize("seed,n_loops", [(0, 52), (1, 58)])
def test_spheres(device, seed, n_loops):
    mesh, want = _sphere(seed)
    out = _check(mesh, device, 64, f"sphere {seed}", want=want)
    assert out[-1]["loop_id"].shape[0] == n_loops and int(out[-1]["n_open"]) == 0


def test_off_means_off(device):
    from mast3r_slam.tsdf import fill_holes, mesh_boundaries

    mesh = _sphere(0)[0]
    mesh_d = _dev(mesh, device)
    a, b = fill_holes(mesh_d, 16, return_info=True), fill_holes(mesh_d, 16, return_info=True, bowties=False)
    assert all(torch.equal(x, y) for x, y in zip(a[:-1], b[:-1]))
    assert set(a[-1]) == set(b[-1]) == PLAIN_KEYS | {"loop_perimeter", "loop_filled"}
    assert all(torch.equal(a[-1][k], b[-1][k]) for k in a[-1])
    want = H.fill(mesh, 16, return_info=True)
    for k in range(3):
        _bytes(b[k].cpu().numpy(), want[k], f"plain tensor {k}")
    nv = len(mesh[0])
    a, b = mesh_boundaries(mesh_d[2], nv), mesh_boundaries(mesh_d[2], nv, bowties=False)
    assert set(a) == set(b) == PLAIN_KEYS and all(torch.equal(a[k], b[k]) for k in a)
    assert int(b["n_open"]) == 72
    for off in (None, 0, -3):
        assert fill_holes(mesh_d, off, bowties=True) is mesh_d


def test_edge_cases(device):
    from mast3r_slam.tsdf import fill_holes, mesh_boundaries

    none_v = np.zeros((0, 3), np.float32)
    none_f = np.zeros((0, 3), np.int32)
    V, N, _, C = H.grid(2, 2)
    for mesh in ((V, N, none_f, C), (none_v, none_v, none_f), (none_v, none_v, none_f, none_v)):
        out = _check(mesh, device, 16, "empty")
        assert int(out[-1]["n_boundary_edges"]) == 0 and out[-1]["loop_filled"].shape == (0,)
        assert out[-1]["loop_head"].shape == (0,) and out[-1]["loop_head"].dtype == torch.int32
    b = mesh_boundaries(torch.zeros((0, 3), dtype=torch.int32, device=device), 0, bowties=True)
    assert b["loop_id"].shape == (0,) and b["loop_head"].shape == (0,) and int(b["n_open"]) == 0
    tet = H.hand_mesh("tetrahedron", True)
    out = _check(tet, device, 16, "tetrahedron")
    assert int(out[-1]["n_boundary_edges"]) == 0 and int(out[-1]["n_open"]) == 0
    mesh_d = _dev(tet, device)
    assert all(a is b for a, b in zip(fill_holes(mesh_d, 16, bowties=True), mesh_d))


def test_validation(device):
    """A `bowties` that is not a bool is refused before anything else is looked at."""
    from mast3r_slam.tsdf import TSDFVolume, fill_holes, mesh_boundaries

    mesh = H.grid(3, 3, [(1, 1)])
    mesh_d = _dev(mesh, device)
    host = tuple(torch.from_numpy(a) for a in mesh)
    for bad in (1, 0, None, "yes", 1.0):
        for m in (mesh_d, host):
            with pytest.raises(ValueError, match="fill_holes: bowties must be a bool"):
                fill_holes(m, 16, bowties=bad)
            with pytest.raises(ValueError, match="mesh_boundaries: bowties must be a bool"):
                mesh_boundaries(m[2], 16, bowties=bad)
    with pytest.raises(ValueError, match="fill_holes: bowties must be a bool"):
        fill_holes(mesh_d, 0, bowties="yes")
    assert fill_holes(mesh_d, 16, bowties=np.True_)[0].shape[0] == 17
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fill_holes(host, 16, bowties=True)
    F = mesh[2].copy()
    F[0] = [0, 1, 16]
    with pytest.raises(ValueError, match=r"fill_holes: face indices span \[0, 16\], outside \[0, 16\)"):
        fill_holes(_dev(mesh[:2] + (F,) + mesh[3:], device), 16, bowties=True)
    with pytest.raises(ValueError, match=r"mesh_boundaries: face indices span \[0, 16\], outside \[0, 16\)"):
        mesh_boundaries(torch.from_numpy(F).to(device), 16, bowties=True)
    vol = TSDFVolume(0.03, 0.09, 100.0, 0.5, capacity=1 << 10, device=device)
    with pytest.raises(ValueError, match="TSDFVolume.extract_mesh: fill_bowties must be a bool"):
        vol.extract_mesh(fill_holes=16, fill_bowties=1)


def test_repeat_calls(device):
    from mast3r_slam.tsdf import fill_holes

    mesh_d = _dev(_sphere(1)[0], device)
    before = [t.clone() for t in mesh_d]
    first = fill_holes(mesh_d, 64, return_info=True, bowties=True)
    for _ in range(3):
        again = fill_holes(mesh_d, 64, return_info=True, bowties=True)
        assert all(torch.equal(a, b) for a, b in zip(again[:-1], first[:-1]))
        assert all(torch.equal(again[-1][k], first[-1][k]) for k in first[-1])
    assert all(torch.equal(a, b) for a, b in zip(mesh_d, before))


# ----------------------------------------------------------------------------------------------------------------------
# product path
# ----------------------------------------------------------------------------------------------------------------------
def test_sphere_volume(device):
    """extract_mesh(fill_holes=64, fill_bowties=True) of a volume loaded with the seed-0 sphere without 200 voxels: every
    boundary dart is on a loop, the chain order is filter -> fill -> smooth -> simplify, the defaults are untouched."""
    from mast3r_slam.tsdf import (TSDFVolume, fill_holes, mesh_boundaries, mesh_from_voxels, simplify_mesh,
                                  smooth_mesh)

    keys, t, w = H.sphere_voxels(0, 200)
    vol = TSDFVolume(0.03, 0.09, 100.0, 0.5, capacity=1 << 15, device=device)
    vol.load_voxels(keys, t, w)
    plain = vol.extract_mesh()
    mesh, want = _sphere(0)
    for got, ref in zip(_host(plain), mesh):
        _bytes(got, ref, "extraction")
    assert vol.extract_mesh(fill_bowties=True)[0].shape == plain[0].shape
    _same(plain, vol.extract_mesh(fill_bowties=True))
    _same(plain, vol.extract_mesh(fill_holes=0, fill_bowties=True))
    _same(vol.extract_mesh(fill_holes=64), fill_holes(plain, 64))
    _same(vol.extract_mesh(fill_holes=64, fill_bowties=False), fill_holes(plain, 64))
    b = mesh_boundaries(plain[2], plain[0].shape[0], bowties=True)
    assert int(b["n_open"]) == 0 and int(b["n_boundary_edges"]) == 598
    assert int(mesh_boundaries(plain[2], plain[0].shape[0])["n_open"]) == 72
    filled = vol.extract_mesh(fill_holes=64, fill_bowties=True)
    _same(filled, fill_holes(plain, 64, bowties=True))
    for got, ref in zip(_host(filled), want[:3]):
        _bytes(got, ref, "filled")
    assert filled[2].shape[0] == plain[2].shape[0] + 309
    assert int(mesh_boundaries(filled[2], filled[0].shape[0], bowties=True)["n_boundary_edges"]) == 289
    _same(filled, mesh_from_voxels(keys, t, w, 0.03, 0.5, device=device, fill_holes=64, fill_bowties=True))
    c = 2 * 0.03
    chain = vol.extract_mesh(fill_holes=64, fill_bowties=True, smooth_iterations=2, simplify_cell=c)
    _same(chain, simplify_mesh(smooth_mesh(fill_holes(plain, 64, bowties=True), 2), c))
    assert not torch.equal(chain[0], simplify_mesh(fill_holes(smooth_mesh(plain, 2), 64, bowties=True), c)[0])
    _same(chain, mesh_from_voxels(keys, t, w, 0.03, 0.5, device=device, fill_holes=64, fill_bowties=True,
                                  smooth_iterations=2, simplify_cell=c))


ROOM_MIN_WEIGHT = 40.0              # where the room's surface is thin: most boundary darts lie on rims that meet


def test_room(device):
    from mast3r_slam import synthetic
    from mast3r_slam.tsdf import compare_meshes, fill_holes

    vol = _vol(device, 1 << 20)
    for pw, conf, org in _room():
        vol.integrate(pw, conf, org)
    plain = vol.extract_mesh(min_weight=ROOM_MIN_WEIGHT)
    filled = vol.extract_mesh(min_weight=ROOM_MIN_WEIGHT, fill_holes=16, fill_bowties=True)
    out = _check(_host(plain), device, 16, "room", mesh_d=plain, colours=False)
    _same(filled, out[:3])
    info = out[-1]
    without = fill_holes(plain, 16, return_info=True)
    assert int(info["n_open"]) <= int(without[-1]["n_open"])
    assert int(info["n_boundary_edges"]) == int(without[-1]["n_boundary_edges"])
    gv, gf = synthetic.room_mesh()
    gt = (torch.from_numpy(gv.astype(np.float32)).to(device), torch.from_numpy(gf.astype(np.int32)).to(device))
    before = compare_meshes(plain, gt, n_samples=20000, threshold=VS, seed=1)
    after = compare_meshes(filled, gt, n_samples=20000, threshold=VS, seed=1)
    plain_after = compare_meshes(without[:3], gt, n_samples=20000, threshold=VS, seed=1)
    for name, i, m in (("plain", without[-1], plain_after), ("bow-ties", info, after)):
        print(f"room, min_weight {ROOM_MIN_WEIGHT}, {name}: F = {plain[2].shape[0]}, {i['loop_id'].shape[0]} loops "
              f"(longest {int(i['loop_length'].max())}), {int(i['loop_filled'].sum())} filled, {int(i['n_open'])} open "
              f"darts of {int(i['n_boundary_edges'])}; accuracy {before['accuracy']:.5f} -> {m['accuracy']:.5f}, "
              f"completion {before['completion']:.5f} -> {m['completion']:.5f}, recall {before['recall']:.5f} -> "
              f"{m['recall']:.5f}, F-score {before['fscore']:.5f} -> {m['fscore']:.5f}")
    assert after["recall"] >= before["recall"]
    assert after["accuracy"] <= before["accuracy"] + VS


# ----------------------------------------------------------------------------------------------------------------------
# the C entry points of the pairing, operands in guarded allocations
# ----------------------------------------------------------------------------------------------------------------------
def _raw(device, mesh, spoil=None, variants=False):
    """dkeys .. loop_assign through the C entry points.  `spoil`: a function that changes the numpy copy of the fan
    successors before they are claimed.  `variants`: the loops are found three more times, without a flag, without a flag
    and the loop_id and loop_head outputs, and with the flag but without those outputs: got["variants"]."""
    import mslam_hip as _m
    from mast3r_slam.tsdf.mesh_holes import _darts, _rounds
    from mesh_support import Operands

    L, st = _m.lib(), _m.stream_ptr()
    ops = Operands(device)
    F = np.reshape(mesh[2], (-1, 3))
    nv, nf = len(mesh[0]), len(F)
    i32, i64 = torch.int32, torch.int64
    put = lambda t, dt: ops.put(t.cpu().numpy(), dt)
    f = ops.put(F, np.int32)
    dart, tail, head = (put(t, np.int32) for t in _darts(f, nv, nf))
    B = int(dart.shape[0])
    keys = ops.out(i64, (3 * nf,))
    _m.check(L.mslam_mesh_holes_dkeys(_m.ptr(f), nf, nv, _m.ptr(keys), st), "dkeys")
    skeys, order = torch.sort(keys, stable=True)
    skeys, order = put(skeys, np.int64), put(order, np.int64)
    fan = ops.out(i32, (B,))
    _m.check(L.mslam_mesh_holes_fan(_m.ptr(f), nf, nv, _m.ptr(dart), _m.ptr(head), B, _m.ptr(skeys), _m.ptr(order),
                                    _m.ptr(fan), st), "fan")
    rotated = fan.cpu().numpy()
    if spoil is not None:
        s = rotated.copy()
        spoil(s)
        fan = ops.put(s, np.int32)
    dart_key = put(keys[dart.long()], np.int64)
    sorted_fan, sorted_dart_key = put(torch.sort(fan)[0], np.int32), put(torch.sort(dart_key)[0], np.int64)
    pairs = lambda: ops.out(i32, (B, 2))

    def double(state):
        buf = [state, pairs(), pairs()]
        cur = 0
        for _ in range(max(_rounds(B), 2)):                           # at least two: both spare buffers are written
            nxt = 1 if cur != 1 else 2
            _m.check(L.mslam_mesh_holes_double(_m.ptr(buf[cur]), _m.ptr(buf[nxt]), B, st), "double")
            cur = nxt
        return buf[cur]

    state = pairs()
    _m.check(L.mslam_mesh_holes_claim(_m.ptr(fan), _m.ptr(sorted_fan), _m.ptr(dart_key), _m.ptr(sorted_dart_key), B,
                                      _m.ptr(state), st), "claim")
    labelled = double(state)
    rank = [pairs(), pairs()]
    _m.check(L.mslam_mesh_holes_rank_init(_m.ptr(state), _m.ptr(labelled), B, _m.ptr(rank[0]), st), "rank_init")
    rounds = _rounds(B) + (_rounds(B) & 1)                           # even: the result is in rank[0], both are written
    for r in range(rounds):
        _m.check(L.mslam_mesh_holes_rank_double(_m.ptr(rank[r & 1]), _m.ptr(rank[~r & 1]), B, st), "rank_double")
    walk_keys = ops.out(i64, (B,))
    _m.check(L.mslam_mesh_holes_walk_keys(_m.ptr(labelled), _m.ptr(rank[0]), B, _m.ptr(walk_keys), st), "walk_keys")
    swalk, walk_order = torch.sort(walk_keys)
    swalk, walk_order = put(swalk, np.int64), put(walk_order, np.int64)
    pair_keys = ops.out(i64, (B,))
    _m.check(L.mslam_mesh_holes_pair_keys(_m.ptr(labelled), _m.ptr(head), _m.ptr(swalk), _m.ptr(walk_order), B, nv,
                                          _m.ptr(pair_keys), st), "pair_keys")
    spair, pair_order = torch.sort(pair_keys, stable=True)
    spair, pair_order = put(spair, np.int64), put(pair_order, np.int64)
    paired = pairs()
    _m.check(L.mslam_mesh_holes_repair(_m.ptr(spair), _m.ptr(pair_order), _m.ptr(walk_order), _m.ptr(state), B,
                                       _m.ptr(paired), st), "repair")
    labelled2 = double(paired)
    tail_keys = ops.out(i64, (B,))
    _m.check(L.mslam_mesh_holes_tail_keys(_m.ptr(labelled2), _m.ptr(tail), B, nv, _m.ptr(tail_keys), st), "tail_keys")
    stail = put(torch.sort(tail_keys)[0], np.int64)
    flag = ops.put(np.zeros(B, np.uint8), np.uint8)
    _m.check(L.mslam_mesh_holes_tail_flag(_m.ptr(stail), B, nv, _m.ptr(flag), st), "tail_flag")
    h = lambda t: t.cpu().numpy()

    def find(flag, names=True):
        """loop_labels .. loop_assign; `flag` and, with names=False, the loop_id and loop_head outputs may be None."""
        lab = ops.out(i32, (B + 1,))
        _m.check(L.mslam_mesh_holes_loop_labels(_m.ptr(labelled2), _m.ptr(flag), B, _m.ptr(lab), st), "loop_labels")
        runs, counts = torch.unique_consecutive(torch.sort(lab)[0], return_counts=True)
        loop_name, length = put(runs[:-1], np.int32), counts[:-1].cpu().numpy()
        nl = int(loop_name.shape[0])
        dart_loop, start = ops.out(i32, (B,)), ops.out(i32, (nl,))
        loop_id, loop_head = (ops.out(i32, (nl,)), ops.out(i32, (nl,))) if names else (None, None)
        _m.check(L.mslam_mesh_holes_loop_assign(_m.ptr(labelled2), _m.ptr(paired), _m.ptr(flag), _m.ptr(tail),
                                                _m.ptr(head), B, _m.ptr(loop_name), nl, _m.ptr(dart_loop),
                                                _m.ptr(start), _m.ptr(loop_id), _m.ptr(loop_head), st), "loop_assign")
        out = dict(lab=h(lab), dart_loop=h(dart_loop), start=h(start), loop_length=length, n_open=int(counts[-1]) - 1)
        if names:
            out.update(loop_id=h(loop_id), loop_head=h(loop_head))
        return out

    got = find(flag)
    if variants:
        got["variants"] = dict(null_flag=find(None), null_flag_no_names=find(None, False), no_names=find(flag, False))
    ops.check()
    assert np.array_equal(f.cpu().numpy(), F)
    got.update(keys=h(keys), rotated=rotated, fan=h(state)[:, 0], name=h(state)[:, 1], nxt=h(paired)[:, 0],
               flag=h(flag))
    return got


def _raw_against(got, tr):
    assert np.array_equal(got["fan"], tr["fan"]) and np.array_equal(got["name"], tr["name"])
    assert np.array_equal(got["nxt"], tr["nxt"]) and np.array_equal(got["dart_loop"], tr["dart_loop"])
    assert got["start"].tolist() == [w[0] for w in tr["walks"]]
    assert got["loop_length"].tolist() == [len(w) for w in tr["walks"]]
    assert np.array_equal(got["loop_id"], tr["loop_id"]) and np.array_equal(got["loop_head"], tr["loop_head"])
    assert got["n_open"] == int((tr["dart_loop"] < 0).sum())


def _bad_faces():
    """hole_pairs(3) with four faces Python would reject in place of faces that touch neither a hole nor the rim."""
    P, N, F, C = BT.hole_pairs(3)
    F = F.copy()
    bad = ([0, 1, len(P)], [5, -1, 6], [9, 9, 10], [2 ** 31 - 1, 0, 1])
    inner = [(4 * i + 3, 4 * j + 1) for i, j in ((0, 0), (1, 1), (1, 2), (0, 2))]    # cells away from every hole
    for (a, b), face in zip(inner, bad):
        v = a * 13 + b
        row = np.nonzero((F == [v, v + 13, v + 14]).all(1))[0]
        assert len(row) == 1
        F[row[0]] = face
    assert int((~H.counting(F, len(P))).sum()) == 4
    return P, N, F, C


@pytest.mark.parametrize("name", ["bad faces", "bad winding", "three gaps", "sphere"])
def test_entry_points(device, name):
    """The pairing through its entry points: faces that do not count are skipped and never followed, nothing outside
    the outputs is written, every output is written, and every stage is the statement's."""
    mesh = {"bad faces": _bad_faces, "bad winding": BT.bad_winding, "three gaps": lambda: BT.gapped_fan(6, [0, 2, 4]),
            "sphere": lambda: _sphere(1)[0]}[name]()
    nv = len(mesh[0])
    got = _raw(device, mesh)
    ok = np.repeat(H.counting(mesh[2], nv), 3)
    assert (got["keys"][~ok] == np.iinfo(np.int64).max).all() and (got["keys"][ok] < nv * nv).all()
    tr = BT.trace(mesh[2], nv)
    _raw_against(got, tr)
    assert np.array_equal(got["rotated"], got["fan"])                 # nobody claims another's successor
    if name == "bad faces":
        assert sorted(got["loop_length"].tolist()) == [3] * 4 + [4] * 18 + [48] and got["n_open"] == 0
    assert not got["flag"].any()


def test_entry_points_with_broken_successors(device):
    """Successors out of range, and one claimed twice: they are nobody's, their walks are open, the rest is untouched."""
    mesh = BT.hole_pairs(3)
    nv = len(mesh[0])
    tr = BT.trace(mesh[2], nv)
    B = len(tr["dart"])
    w = tr["closed"]
    assert len(w) >= 5

    def spoil(s):
        s[w[1][0]] = B + 5
        s[w[2][1]] = -7
        s[w[3][0]] = 2 ** 31 - 1
        s[w[4][0]] = s[w[4][2]]                                      # two darts claim one successor: neither has it

    got = _raw(device, mesh, spoil)
    fan = tr["fan"].copy()
    fan[[w[1][0], w[2][1], w[3][0], w[4][0], w[4][2]]] = -1
    assert np.array_equal(got["fan"], fan)
    broken = np.zeros(B, bool)
    for k in (1, 2, 3, 4):
        broken[w[k]] = True
    assert (got["dart_loop"][broken] == -1).all() and (got["nxt"][broken] == -1).all()
    assert got["n_open"] == int(broken.sum())
    keep = [l for l, walk in enumerate(tr["walks"]) if not broken[walk[0]]]
    assert got["loop_length"].tolist() == [len(tr["walks"][l]) for l in keep]
    assert got["start"].tolist() == [tr["walks"][l][0] for l in keep]
    assert np.array_equal(got["nxt"][~broken], tr["nxt"][~broken])


def test_null_flag_is_a_zero_flag(device):
    """Where both are defined (labels that are dart names), loop_labels and loop_assign without a flag are those with an
    all-zero flag, and the loop_id and loop_head outputs may be left out; _raw checks the guards and the outputs."""
    mesh = BT.hole_pairs(3)
    got = _raw(device, mesh, variants=True)
    assert not got["flag"].any() and len(got["start"]) >= 5
    _raw_against(got, BT.trace(mesh[2], len(mesh[0])))
    for name, other in got["variants"].items():
        assert set(other) == {"lab", "dart_loop", "start", "loop_length", "n_open"} | (
            {"loop_id", "loop_head"} if name == "null_flag" else set()), name
        for k, v in other.items():
            assert np.array_equal(v, got[k]), (name, k)


def test_entry_points_reject_bad_arguments(device):
    import mslam_hip as _m

    L, st = _m.lib(), _m.stream_ptr()
    einval = _m.header_constants()["MSLAM_EINVAL"]
    s = torch.zeros((4, 2), dtype=torch.int32, device=device)
    k = torch.zeros(4, dtype=torch.int64, device=device)
    assert L.mslam_mesh_holes_rank_double(_m.ptr(s), _m.ptr(s), 4, st) == einval
    assert L.mslam_mesh_holes_rank_double(_m.ptr(s), _m.ptr(s.clone()), -1, st) == einval
    assert L.mslam_mesh_holes_repair(_m.ptr(k), _m.ptr(k), _m.ptr(k), _m.ptr(s), 4, _m.ptr(s), st) == einval
    assert L.mslam_mesh_holes_dkeys(0, 3, 3, 0, st) == einval
    assert L.mslam_mesh_holes_tail_flag(_m.ptr(k), 4, 0, _m.ptr(s), st) == einval
    assert L.mslam_mesh_holes_fan(0, 0, 0, 0, 0, 0, 0, 0, 0, st) == 0      # nothing to do
