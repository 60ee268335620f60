"""GPU tests (-m gpu) of mesh_boundaries and fill_holes (csrc/mesh_holes.hip, DESIGN.md "Mesh holes") and of the
fill_holes argument of the mesh extraction, against the numpy statement tests/holes_numpy.py.

Everything is compared byte for byte: all arithmetic is f64 on the f32 input, every sum is sequential in the statement's
walk order, nothing goes through a library function other than sqrt and the division, both correctly rounded."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import holes_numpy as H  # noqa: E402
import mc_numpy as M  # noqa: E402
from mesh_support import VS, Operands, _host, _room, _same, _vol  # noqa: E402

pytestmark = pytest.mark.gpu

INFO = ("loop_id", "loop_length", "dart", "dart_tail", "dart_head", "dart_loop", "loop_perimeter", "loop_filled")


def _dev(mesh, device):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in mesh)


def _bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()))


def _views(mesh, device):
    """The mesh as non-contiguous device views: columns 1:4 of a wider tensor, every other row, a transposed copy."""
    V, F = len(mesh[0]), len(mesh[2])
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
        assert int(info[k]) == want[k], (what, k)


def _check(mesh, device, max_edges, what, mesh_d=None, want=None):
    """fill_holes and mesh_boundaries on the device against the statement, every tensor byte for byte."""
    from mast3r_slam.tsdf import fill_holes, mesh_boundaries

    mesh_d = _dev(mesh, device) if mesh_d is None else mesh_d
    want = H.fill(mesh, max_edges, return_info=True) if want is None else want
    out = fill_holes(mesh_d, max_edges, return_info=True)
    assert len(out) == len(mesh) + 1
    for k in range(len(mesh)):
        _bytes(out[k].cpu().numpy(), want[k], f"{what} tensor {k}")
    _check_info(out[-1], want[-1], what)
    if not want[-1]["loop_filled"].any():
        assert all(a is b for a, b in zip(out[:-1], mesh_d))
    plain = fill_holes(mesh_d, max_edges)
    assert len(plain) == len(mesh) and all(torch.equal(a, b) for a, b in zip(plain, out))
    nv = len(mesh[0])
    _check_info(mesh_boundaries(mesh_d[2], nv, mesh_d[0]), want[-1], what + " boundaries", INFO[:-1])
    bare = mesh_boundaries(mesh_d[2], nv)
    assert "loop_perimeter" not in bare
    _check_info(bare, want[-1], what + " boundaries without vertices", INFO[:-2])
    return out


@pytest.mark.parametrize("colors", [False, True])
@pytest.mark.parametrize("name", H.HAND)
def test_hand_meshes(device, name, colors):
    mesh = H.hand_mesh(name, colors)
    want = H.fill(mesh, 16, return_info=True)
    _check(mesh, device, 16, name, want=want)
    _check(mesh, device, 16, name + " views", mesh_d=_views(mesh, device), want=want)


def test_grid_and_folded_loops(device):
    mesh = H.grid(5, 5, [(2, 2)])
    out = _check(mesh, device, 16, "grid")
    assert out[-1]["loop_filled"].tolist() == [False, True] and out[0][36].tolist() == [2.5, 2.5, 0.0]
    assert out[-1]["loop_length"].tolist() == [20, 4]
    _check(mesh[:3], device, 16, "grid without colours")
    _check(mesh, device, 16, "grid views", mesh_d=_views(mesh, device))
    out = _check(H.folded_ring(), device, 16, "folded ring")
    assert not out[-1]["loop_filled"].any()
    V, N, F, C = H.ring(5)
    V = V.copy()
    V[:5] = [[1, 0, 0], [-1, 0, 0], [-2, -1, 0], [0, 3, 0], [2, -2, 0]]         # one product is exactly zero
    out = _check((V, N, F, C), device, 16, "degenerate fan face")
    assert not out[-1]["loop_filled"].any()
    jittered = H.grid(8, 7, [(1, 1), (3, 2), (5, 5), (6, 1)], jitter=0.2, seed=4)
    out = _check(jittered, device, 16, "jittered grid")
    assert out[-1]["loop_filled"].tolist() == [False] + [True] * 4


@functools.lru_cache(maxsize=None)
def _sphere(seed):
    mesh = H.sphere_mesh(seed)
    return mesh, H.fill(mesh, 16, return_info=True)


@pytest.mark.parametrize("seed,n_loops,n_open", [(2, 16, 0), (0, 18, 6), (3, 16, 14)])
def test_spheres(device, seed, n_loops, n_open):
    mesh, want = _sphere(seed)
    out = _check(mesh, device, 16, f"sphere {seed}", want=want)
    assert out[-1]["loop_id"].shape[0] == n_loops and int(out[-1]["n_open"]) == n_open


def test_empty_meshes(device):
    from mast3r_slam.tsdf import fill_holes, mesh_boundaries

    none_v = np.zeros((0, 3), np.float32)
    none_f = np.zeros((0, 3), np.int32)
    V, N, _, C = H.grid(2, 2)
    for mesh in ((V, N, none_f, C), (none_v, none_v, none_f), (none_v, none_v, none_f, none_v)):
        out = _check(mesh, device, 16, "empty")
        assert int(out[-1]["n_boundary_edges"]) == 0 and out[-1]["loop_filled"].shape == (0,)
        mesh_d = _dev(mesh, device)
        assert all(a is b for a, b in zip(fill_holes(mesh_d, 16), mesh_d))
    b = mesh_boundaries(torch.zeros((0, 3), dtype=torch.int32, device=device), 0)
    assert b["loop_id"].shape == (0,) and b["dart"].dtype == torch.int32 and int(b["n_open"]) == 0


@pytest.mark.parametrize("n", [3, 4, 63, 64, 65, 257])
def test_rings_across_the_doubling_rounds(device, n):
    """B = 2 n darts in two loops of n: n = 64 is a loop that 6 rounds cover exactly, 63 and 65 lie on either side; the
    cap is inclusive."""
    mesh = H.ring(n)
    out = _check(mesh, device, n, f"ring {n}")
    assert out[-1]["loop_length"].tolist() == [n, n] and out[-1]["loop_filled"].tolist() == [True, False]
    assert out[0].shape[0] == 2 * n + 1 and out[2].shape[0] == 3 * n
    below = _check(mesh[:3], device, n - 1, f"ring {n} capped")
    assert not below[-1]["loop_filled"].any()


@pytest.mark.parametrize("B", [255, 256, 257, 513])
def test_dart_counts_at_block_edges(device, B):
    """One lane per boundary dart in blocks of 256: the last block one short, full, one over, and a third block of one."""
    mesh = H.join(H.strip(B - 6), H.ring(3))
    out = _check(mesh, device, 16, f"B = {B}")
    assert int(out[-1]["n_boundary_edges"]) == B and out[-1]["loop_length"].tolist() == [B - 6, 3, 3]
    assert out[-1]["loop_filled"].tolist() == [False, True, False]


def test_more_loops_than_a_block(device):
    removed = [(i, j) for i in range(1, 35, 2) for j in range(1, 35, 2)]
    mesh = H.grid(35, 35, removed, jitter=0.15, seed=9)
    out = _check(mesh, device, 4, "289 holes")
    assert out[-1]["loop_filled"].tolist() == [False] + [True] * 289
    assert out[0].shape[0] == 36 * 36 + 289 and out[2].shape[0] == len(mesh[2]) + 4 * 289


def test_loop_id_in_the_last_face_and_face_order(device):
    mesh = H.grid(6, 5, [(2, 2), (4, 1)], jitter=0.1, seed=2)
    tr = H.trace(mesh[2], len(mesh[0]))
    first_dart_face = int(tr["dart"][tr["walks"][1][0]]) // 3
    order = [f for f in range(len(mesh[2])) if f != first_dart_face] + [first_dart_face]
    moved = mesh[:2] + (np.ascontiguousarray(mesh[2][order]),) + mesh[3:]
    a = _check(mesh, device, 16, "grid")
    b = _check(moved, device, 16, "grid, the loop id's dart in the last face")
    assert int(b[-1]["dart"][-1]) // 3 == len(mesh[2]) - 1 and int(b[-1]["dart_tail"][-1]) == int(b[-1]["loop_id"][1])
    nf = len(mesh[2])
    perm = np.random.default_rng(3).permutation(nf)
    c = _check(mesh[:2] + (np.ascontiguousarray(mesh[2][perm]),) + mesh[3:], device, 16, "grid, faces shuffled")
    for other in (b, c):
        for k in (0, 1, 3):
            assert torch.equal(a[k], other[k])
        assert torch.equal(a[2][nf:], other[2][nf:])
        for k in ("loop_id", "loop_length", "loop_filled", "loop_perimeter"):
            assert torch.equal(a[-1][k], other[-1][k])


def test_repeat_calls(device):
    from mast3r_slam.tsdf import fill_holes

    mesh, want = _sphere(2)
    mesh_d = _dev(mesh, device)
    before = [t.clone() for t in mesh_d]
    first = fill_holes(mesh_d, 16, return_info=True)
    for _ in range(3):
        again = fill_holes(mesh_d, 16, return_info=True)
        assert all(torch.equal(a, b) for a, b in zip(again[:-1], first[:-1]))
        assert all(torch.equal(again[-1][k], first[-1][k]) for k in first[-1])
    assert all(torch.equal(a, b) for a, b in zip(mesh_d, before))
    for off in (None, 0, -3):
        assert fill_holes(mesh_d, off) is mesh_d


# ----------------------------------------------------------------------------------------------------------------------
# the C entry points, operands in guarded allocations
# ----------------------------------------------------------------------------------------------------------------------
def _raw(device, mesh, max_edges, spoil=None):
    """The whole sequence through the C entry points.  `spoil`: a function that changes the numpy copy of the linked
    state (the successors) before the walks."""
    import mslam_hip as _m
    from mast3r_slam.tsdf.mesh_holes import _rounds

    L, st = _m.lib(), _m.stream_ptr()
    ops = Operands(device)
    P, _, F, C = mesh
    nv, nf = len(P), len(F)
    i32, i64 = torch.int32, torch.int64
    put = lambda t, dt: ops.put(t.cpu().numpy(), dt)
    v, f, c = ops.put(P, np.float32), ops.put(np.reshape(F, (-1, 3)), np.int32), ops.put(C, np.float32)
    keys = ops.out(i64, (3 * nf,))
    _m.check(L.mslam_mesh_holes_keys(_m.ptr(f), nf, nv, _m.ptr(keys), st), "keys")
    skeys, order = torch.sort(keys, stable=True)
    skeys, order = put(skeys, np.int64), put(order, np.int64)
    flag = ops.out(torch.uint8, (3 * nf,))
    _m.check(L.mslam_mesh_holes_mark(_m.ptr(skeys), _m.ptr(order), 3 * nf, _m.ptr(flag), st), "mark")
    dart = put(torch.nonzero(flag).reshape(-1), np.int32)
    B = int(dart.shape[0])
    tail, head = ops.out(i32, (B,)), ops.out(i32, (B,))
    _m.check(L.mslam_mesh_holes_darts(_m.ptr(f), nf, nv, _m.ptr(dart), B, _m.ptr(tail), _m.ptr(head), st), "darts")
    sorted_tail, tail_order = torch.sort(tail, stable=True)
    sorted_tail, tail_order, sorted_head = put(sorted_tail, np.int32), put(tail_order, np.int64), put(torch.sort(head)[0],
                                                                                                    np.int32)
    state = ops.out(i32, (B, 2))
    _m.check(L.mslam_mesh_holes_link(_m.ptr(tail), _m.ptr(head), _m.ptr(sorted_tail), _m.ptr(tail_order),
                                     _m.ptr(sorted_head), B, nv, _m.ptr(state), st), "link")
    buf = [state, ops.out(i32, (B, 2)), ops.out(i32, (B, 2))]
    cur = 0
    for _ in range(max(_rounds(B), 2) if B else 0):                 # at least two: both spare buffers are written
        nxt = 1 if cur != 1 else 2
        _m.check(L.mslam_mesh_holes_double(_m.ptr(buf[cur]), _m.ptr(buf[nxt]), B, st), "double")
        cur = nxt
    lab = ops.out(i32, (B + 1,))
    _m.check(L.mslam_mesh_holes_loop_labels(_m.ptr(buf[cur]), 0, B, _m.ptr(lab), st), "labels")
    runs, counts = torch.unique_consecutive(torch.sort(lab)[0], return_counts=True)
    loop_id, length = put(runs[:-1], np.int32), put(counts[:-1], np.int32)
    nl = int(loop_id.shape[0])
    dart_loop, start = ops.out(i32, (B,)), ops.out(i32, (nl,))
    _m.check(L.mslam_mesh_holes_loop_assign(_m.ptr(buf[cur]), _m.ptr(state), 0, 0, 0, B, _m.ptr(loop_id), nl,
                                            _m.ptr(dart_loop), _m.ptr(start), 0, 0, st), "assign")
    walked = state
    if spoil is not None:
        s = state.cpu().numpy().copy()
        spoil(s)
        walked = ops.put(s, np.int32)
    per, cen, fil = ops.out(torch.float64, (nl,)), ops.out(torch.float64, (nl, 3)), ops.out(torch.uint8, (nl,))
    _m.check(L.mslam_mesh_holes_measure(_m.ptr(v), _m.ptr(f), nf, nv, _m.ptr(dart), _m.ptr(tail), _m.ptr(head),
                                        _m.ptr(walked), B, _m.ptr(start), _m.ptr(length), nl, max_edges, 1, _m.ptr(per),
                                        _m.ptr(cen), _m.ptr(fil), st), "measure")
    fl = fil.to(i64)
    fn = fl * length
    vend, fend = torch.cumsum(fl, 0), torch.cumsum(fn, 0)
    new_v, new_f = (int(vend[-1]), int(fend[-1])) if nl else (0, 0)
    vbase, fbase = put(vend - fl, np.int64), put(fend - fn, np.int64)
    ov, on, oc = (ops.out(torch.float32, (nv + new_v, 3)) for _ in range(3))
    of = ops.out(i32, (nf + new_f, 3))
    for o, src in ((ov, v), (on, v), (oc, c)):
        o[:nv] = src
    of[:nf] = 0
    _m.check(L.mslam_mesh_holes_emit(_m.ptr(v), _m.ptr(c), _m.ptr(tail), _m.ptr(head), _m.ptr(walked), B, _m.ptr(start),
                                     _m.ptr(length), _m.ptr(fil), _m.ptr(vbase), _m.ptr(fbase), nl, nv, nf, new_v, new_f,
                                     _m.ptr(cen), _m.ptr(ov), _m.ptr(on), _m.ptr(oc), _m.ptr(of), st), "emit")
    ops.check()
    assert np.array_equal(f.cpu().numpy(), np.reshape(F, (-1, 3))) and np.array_equal(v.cpu().numpy(), P)
    h = lambda t: t.cpu().numpy()
    return dict(keys=h(keys), flag=h(flag), dart=h(dart), dart_tail=h(tail), dart_head=h(head), state=h(state),
                dart_loop=h(dart_loop), loop_id=h(loop_id), loop_length=h(length), start=h(start),
                loop_perimeter=h(per), loop_filled=h(fil).astype(bool), new_vertices=h(ov)[nv:], new_normals=h(on)[nv:],
                new_colors=h(oc)[nv:], new_faces=h(of)[nf:])


def _bad_mesh():
    """A jittered grid with four holes and four faces Python would reject: an index past V, a negative one, a repeated
    one, INT32_MAX.  They do not count, so each leaves a three-edge hole of its own: the first face of four inner cells
    that touch neither a hole, nor the rim, nor each other."""
    P, N, F, C = H.grid(8, 7, [(1, 1), (3, 2), (5, 5), (6, 1)], jitter=0.2, seed=4)
    F = F.copy()
    bad = ([0, 1, len(P)], [5, -1, 6], [9, 9, 10], [2 ** 31 - 1, 0, 1])
    for (i, j), face in zip(((1, 3), (3, 4), (5, 3), (1, 5)), bad):
        v = i * 8 + j
        row = np.nonzero((F == [v, v + 8, v + 9]).all(1))[0]
        assert len(row) == 1
        F[row[0]] = face
    assert int((~H.counting(F, len(P))).sum()) == 4
    return P, N, F, C


def test_entry_points(device):
    """Faces that do not count are skipped, never followed, and the rest is the statement's; nothing outside the outputs
    is written and every output is written."""
    mesh = _bad_mesh()
    P, N, F, C = mesh
    nv, nf = len(P), len(F)
    want = H.fill(mesh, 16, return_info=True)
    info = want[-1]
    assert info["loop_filled"].tolist() == [False] + [True] * 8 and sorted(info["loop_length"].tolist()) == [3] * 4 + [
        4] * 4 + [30]
    got = _raw(device, mesh, 16)
    ok = np.repeat(H.counting(F, nv), 3)
    assert (got["keys"][~ok] == np.iinfo(np.int64).max).all() and (got["keys"][ok] < nv * nv).all()
    assert not got["flag"][~ok].any() and int(got["flag"].sum()) == info["n_boundary_edges"]
    for k in INFO:
        _bytes(got[k], info[k], k)
    tr = H.trace(F, nv)
    assert np.array_equal(got["state"][:, 0], tr["nxt"]) and np.array_equal(got["state"][:, 1], tr["tail"])
    assert np.array_equal(got["start"], [w[0] for w in tr["walks"]])
    _bytes(got["new_vertices"], want[0][nv:], "vertices")
    _bytes(got["new_normals"], want[1][nv:], "normals")
    _bytes(got["new_colors"], want[3][nv:], "colours")
    _bytes(got["new_faces"], want[2][nf:], "faces")


def test_entry_points_with_broken_successors(device):
    """Successors outside [0, B), and one that leaves its loop: the walks stop there, those loops are not fillable, the
    others are the statement's."""
    mesh = _bad_mesh()
    nv = len(mesh[0])
    tr = H.trace(mesh[2], nv)
    want = H.fill(mesh, 16, return_info=True)[-1]
    B = len(tr["dart"])
    walks = tr["walks"]
    assert len(walks) >= 5 and want["loop_filled"][1:5].all()

    def spoil(s):
        s[walks[1][1], 0] = B + 5
        s[walks[2][0], 0] = -7
        s[walks[3][2], 0] = 2 ** 31 - 1
        s[walks[4][1], 0] = walks[1][0]                              # into another loop: the walk does not close

    got = _raw(device, mesh, 16, spoil)
    filled = want["loop_filled"].copy()
    filled[1:5] = False
    assert np.array_equal(got["loop_filled"], filled)
    assert np.isnan(got["loop_perimeter"][1:5]).all()
    keep = np.ones(len(filled), bool)
    keep[1:5] = False
    _bytes(got["loop_perimeter"][keep], want["loop_perimeter"][keep], "perimeter of the other loops")
    assert len(got["new_vertices"]) == int(filled.sum())


def test_entry_points_empty(device):
    import mslam_hip as _m

    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    P, N, _, C = H.grid(3, 3)
    got = _raw(device, (P, N, none_f, C), 16)                       # F = 0
    assert got["dart"].shape == (0,) and got["loop_id"].shape == (0,) and got["new_faces"].shape == (0, 3)
    got = _raw(device, (none_v, none_v, none_f, none_v), 16)        # V = 0
    assert got["dart"].shape == (0,)
    got = _raw(device, (none_v, none_v, np.array([[0, 1, 2]], np.int32), none_v), 16)    # V = 0 with a face: skipped
    assert (got["keys"] == np.iinfo(np.int64).max).all() and not got["flag"].any()
    L = _m.lib()
    s = torch.zeros((4, 2), dtype=torch.int32, device=device)
    einval = _m.header_constants()["MSLAM_EINVAL"]
    assert L.mslam_mesh_holes_double(_m.ptr(s), _m.ptr(s), 4, _m.stream_ptr()) == einval
    assert L.mslam_mesh_holes_double(_m.ptr(s), _m.ptr(s.clone()), -1, _m.stream_ptr()) == einval
    assert L.mslam_mesh_holes_keys(0, 3, 3, 0, _m.stream_ptr()) == einval
    k = torch.zeros(5, dtype=torch.int32, device=device)
    for B in (4, -1):                                                # a null `labelled`, and a negative count
        state = 0 if B > 0 else _m.ptr(s)
        assert L.mslam_mesh_holes_loop_labels(state, 0, B, _m.ptr(k), _m.stream_ptr()) == einval
        assert L.mslam_mesh_holes_loop_assign(state, _m.ptr(s), 0, 0, 0, B, _m.ptr(k), 1, _m.ptr(k), _m.ptr(k), 0, 0,
                                              _m.stream_ptr()) == einval


def _open_octahedron():
    """An octahedron whose vertices are numbered so that one face is (3, 4, 5), without that face: B = 3, and the id of
    the only loop, vertex 3, is not below B.  Plain mode's labels are vertices; only bow-tie mode's are dart names."""
    P = np.array([[-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    F = []
    for sx, sy, sz in np.ndindex(2, 2, 2):                          # 1: the positive end of the axis
        f = [3 * sx, 1 + 3 * sy, 2 + 3 * sz]
        F.append(f if (sx + sy + sz) % 2 else f[::-1])              # wound outwards
    assert F[-1] == [3, 4, 5]
    return H.with_attributes(P, F[:-1])


def test_loop_id_not_below_the_dart_count(device):
    mesh = _open_octahedron()
    want = H.fill(mesh, 16, return_info=True)
    info = want[-1]
    assert info["n_boundary_edges"] == 3 and info["n_open"] == 0 and info["loop_filled"].tolist() == [True]
    assert info["loop_id"].tolist() == [3] and info["loop_length"].tolist() == [3]
    out = _check(mesh, device, 16, "open octahedron", want=want)
    assert out[2].shape[0] == 10 and out[-1]["dart_loop"].tolist() == [0, 0, 0]


# ----------------------------------------------------------------------------------------------------------------------
# call behaviour
# ----------------------------------------------------------------------------------------------------------------------
def test_validation(device):
    from mast3r_slam.tsdf import fill_holes, mesh_boundaries

    mesh = H.grid(3, 3, [(1, 1)])
    mesh_d = _dev(mesh, device)
    for off in (None, 0, -3):
        assert fill_holes(mesh_d, off) is mesh_d
    for bad in (1.5, 2.0, "3"):
        with pytest.raises(ValueError, match="fill_holes: max_edges must be an integer"):
            fill_holes(mesh_d, bad)
    for bad in (np.nan, np.inf, -np.inf):
        V = mesh[0].copy()
        V[2, 1] = bad
        with pytest.raises(ValueError, match=r"fill_holes: vertex coordinates span \[.*\] and are not all finite"):
            fill_holes(_dev((V,) + mesh[1:], device), 16)
    for face, span in (([0, 1, 16], r"\[0, 16\]"), ([0, -1, 2], r"\[-1, 15\]")):
        F = mesh[2].copy()
        F[0] = face
        with pytest.raises(ValueError, match=r"fill_holes: face indices span " + span + r", outside \[0, 16\)"):
            fill_holes(_dev(mesh[:2] + (F,) + mesh[3:], device), 16)
        with pytest.raises(ValueError, match=r"mesh_boundaries: face indices span " + span + r", outside \[0, 16\)"):
            mesh_boundaries(torch.from_numpy(F).to(device), 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fill_holes(tuple(torch.from_numpy(a) for a in mesh), 16)
    with pytest.raises(ValueError, match="mesh must hold 3 or 4 tensors"):
        fill_holes(mesh_d[:2], 16)
    with pytest.raises(ValueError, match=r"normals must be \(16,3\)"):
        fill_holes((mesh_d[0], mesh_d[1][:3], mesh_d[2]), 16)
    with pytest.raises(ValueError, match="vertices has 16 rows, num_vertices is 15"):
        mesh_boundaries(mesh_d[2], 15, mesh_d[0])
    huge = fill_holes(mesh_d, 2 ** 40, return_info=True)            # any integer is a cap
    assert huge[-1]["loop_filled"].tolist() == [False, True]


# ----------------------------------------------------------------------------------------------------------------------
# product path
# ----------------------------------------------------------------------------------------------------------------------
def test_sphere_volume(device):
    """extract_mesh(fill_holes=16) of a volume loaded with the seed-2 sphere: the chain order filter -> fill -> smooth ->
    simplify, watertight, and the default untouched."""
    from mast3r_slam.tsdf import TSDFVolume, fill_holes, mesh_boundaries, mesh_from_voxels, simplify_mesh, smooth_mesh

    keys, t, w = H.sphere_voxels(2)
    vol = TSDFVolume(0.03, 0.09, 100.0, 0.5, capacity=1 << 15, device=device)
    vol.load_voxels(keys, t, w)
    plain = vol.extract_mesh()
    mesh, want = _sphere(2)
    for got, ref in zip(_host(plain), mesh):
        _bytes(got, ref, "extraction")
    _same(plain, vol.extract_mesh(fill_holes=0))
    _same(plain, vol.extract_mesh(fill_holes=None))
    filled = vol.extract_mesh(fill_holes=16)
    _same(filled, fill_holes(plain, 16))
    for got, ref in zip(_host(filled), want[:3]):
        _bytes(got, ref, "filled")
    b = mesh_boundaries(filled[2], filled[0].shape[0])
    assert int(b["n_boundary_edges"]) == 0 and int(b["n_open"]) == 0 and b["loop_id"].shape[0] == 0
    V, _, F = _host(filled)
    cnt, consistent = M.edge_use(F)
    assert consistent and (cnt == 2).all() and M.euler(V, F) == 2
    c = 2 * 0.03
    chain = vol.extract_mesh(fill_holes=16, smooth_iterations=2, simplify_cell=c)
    _same(chain, simplify_mesh(smooth_mesh(fill_holes(plain, 16), 2), c))
    assert not torch.equal(chain[0], simplify_mesh(fill_holes(smooth_mesh(plain, 2), 16), c)[0])
    _same(chain, mesh_from_voxels(keys, t, w, 0.03, 0.5, device=device, fill_holes=16, smooth_iterations=2,
                                  simplify_cell=c))
    # the smoothing moves the new vertices: they are interior now
    smoothed = vol.extract_mesh(fill_holes=16, smooth_iterations=2)
    nv = plain[0].shape[0]
    assert smoothed[0].shape[0] == nv + 16 and not torch.equal(smoothed[0][nv:], filled[0][nv:])


ROOM_MIN_WEIGHT = 40.0              # where the room's surface is thin: small components and small holes


@pytest.mark.parametrize("min_weight", [None, ROOM_MIN_WEIGHT])
def test_room(device, min_weight):
    from mast3r_slam import synthetic
    from mast3r_slam.tsdf import compare_meshes, fill_holes

    vol = _vol(device, 1 << 20)
    for pw, conf, org in _room():
        vol.integrate(pw, conf, org)
    plain = vol.extract_mesh(min_weight=min_weight)
    _same(plain, vol.extract_mesh(min_weight=min_weight, fill_holes=0))
    filled = vol.extract_mesh(min_weight=min_weight, fill_holes=16)
    out = _check(_host(plain), device, 16, "room", mesh_d=plain)
    _same(filled, out[:3])
    info = out[-1]
    assert torch.equal(filled[0][:plain[0].shape[0]], plain[0]) and torch.equal(filled[2][:plain[2].shape[0]], plain[2])
    gv, gf = synthetic.room_mesh()
    gt = (torch.from_numpy(gv.astype(np.float32)).to(device), torch.from_numpy(gf.astype(np.int32)).to(device))
    before = compare_meshes(plain, gt, n_samples=20000, threshold=VS, seed=1)
    after = compare_meshes(filled, gt, n_samples=20000, threshold=VS, seed=1)
    print(f"room, min_weight {min_weight}: F = {plain[2].shape[0]}, {info['loop_id'].shape[0]} loops (longest "
          f"{int(info['loop_length'].max())}), {int(info['loop_filled'].sum())} filled, {int(info['n_open'])} open darts of "
          f"{int(info['n_boundary_edges'])}; completion {before['completion']:.5f} -> {after['completion']:.5f}, recall "
          f"{before['recall']:.5f} -> {after['recall']:.5f}, accuracy {before['accuracy']:.5f} -> {after['accuracy']:.5f}")
    assert after["recall"] >= before["recall"]
    assert after["accuracy"] <= before["accuracy"] + VS
