"""Mesh decimation on the device: round-based half-edge collapse with plane quadrics (Garland & Heckbert, "Surface
simplification using quadric error metrics") to a target face count, a ratio or an error.

No counterpart in the reference.  The kernels are csrc/mesh_decimate.hip (DESIGN.md "Mesh decimation"); the numpy
statement of the same definitions is tests/decimate_numpy.py.  torch sorts and scans, the kernels do the rest: the
tables of every round are mesh_smooth's, the gather at the end is mesh_ops' mslam_mesh_cc_emit.  Works on any welded mesh,
not only on what extract_mesh returns.
"""
import math
import operator

import torch

import mslam_hip as _m

from ._mesh_args import _check_face_range, _check_finite, _faces_arg, _mesh_tuple_arg, _ranges
from .mesh_ops import _compact
from .mesh_smooth import _face_table, _neighbour_table

_C = _m.header_constants()
_STATE = _C["MSLAM_MESH_DECIMATE_STATE"]
_BOUNDARY, _REMOVABLE = _C["MSLAM_MESH_DECIMATE_BOUNDARY"], _C["MSLAM_MESH_DECIMATE_REMOVABLE"]
_NO_RANK = (1 << 31) - 1


def _decimate_args(target_faces, ratio, max_error, what="decimate_mesh"):
    """(target_faces or None, ratio or None, max_error or None) checked; all None: ValueError."""
    if target_faces is not None:
        try:
            target_faces = operator.index(target_faces)
        except TypeError:
            raise ValueError(f"{what}: target_faces must be an integer, got {target_faces!r}") from None
        if target_faces < 0:
            raise ValueError(f"{what}: target_faces must be >= 0, got {target_faces}")
    if ratio is not None:
        ratio = float(ratio)
        if not (ratio > 0.0 and ratio <= 1.0):
            raise ValueError(f"{what}: ratio must be in (0, 1], got {ratio}")
    if max_error is not None:
        max_error = float(max_error)
        if not (max_error >= 0.0) or math.isinf(max_error):
            raise ValueError(f"{what}: max_error must be finite and >= 0, got {max_error}")
    if target_faces is None and ratio is None and max_error is None:
        raise ValueError(f"{what}: one of target_faces, ratio and max_error is needed")
    return target_faces, ratio, max_error


class _Round:
    """The tables of one round on the working faces, and its candidates."""

    def __init__(self, verts, cur, V, F, state, gate, rnd, want_class):
        dev = verts.device
        self.row_start, self.nbr, self.mult, self.E = _neighbour_table(cur, V, F)
        sorted_pairs, pair_start = _face_table(cur, V, F)
        self.best = torch.empty(V, dtype=torch.int32, device=dev)
        self.cost = torch.empty(V, dtype=torch.float64, device=dev)
        self.key = torch.empty(V, dtype=torch.int64, device=dev)
        self.vclass = torch.empty(V, dtype=torch.uint8, device=dev) if want_class else None
        _m.check(_m.lib().mslam_mesh_decimate_candidates(
            _m.ptr(verts), _m.ptr(cur), F, V, _m.ptr(self.row_start), _m.ptr(self.nbr), _m.ptr(self.mult), self.E,
            _m.ptr(sorted_pairs), _m.ptr(pair_start), _m.ptr(state), gate, rnd, _m.ptr(self.best), _m.ptr(self.cost),
            _m.ptr(self.key), _m.ptr(self.vclass), _m.stream_ptr()), "mesh_decimate_candidates")

    def select(self, V):
        """selected bool[V]: the candidates whose rank under (cost, hash, u) is the lowest within two hops."""
        dev = self.best.device
        by_key = torch.sort(self.key)[1]                                    # the keys of candidates are distinct
        order = by_key[torch.sort(self.cost[by_key], stable=True)[1]]
        rank = torch.empty(V, dtype=torch.int32, device=dev)
        rank[order] = torch.arange(V, dtype=torch.int32, device=dev)
        rank = torch.where(self.best >= 0, rank, _NO_RANK).contiguous()
        m1, m2 = torch.empty_like(rank), torch.empty_like(rank)
        for src, dst in ((rank, m1), (m1, m2)):
            _m.check(_m.lib().mslam_mesh_decimate_spread(_m.ptr(src), _m.ptr(self.row_start), _m.ptr(self.nbr), V,
                                                         self.E, _m.ptr(dst), _m.stream_ptr()), "mesh_decimate_spread")
        return (self.best >= 0) & (m2 == rank), rank


def decimate_mesh(mesh, target_faces=None, ratio=None, max_error=None, return_map=False, return_info=False,
                  _validate=True):
    """Decimates `mesh` = (vertices f32[V,3], normals f32[V,3], faces i32[F,3][, colors f32[V,3]]), the tuple
    extract_mesh / filter_mesh / simplify_mesh use, by half-edge collapses chosen by plane quadrics; the result has the
    same arity.  DESIGN.md "Mesh decimation" has the definitions; in short:

    - a collapse u -> v merges the vertex u into a neighbour v: every output vertex is an input vertex, with the input's
      bits in position, normal and colour, and vertices and faces keep their order;
    - every vertex carries the area-weighted plane quadric of its input faces; the cost of u -> v is the summed quadric
      of both at the position of v.  Only interior, manifold vertices are removed (boundary vertices and rims stay as
      they are), and only where the link condition holds and no face of u flips or loses its area;
    - each round ranks every vertex's best collapse by (cost, a hash, index), applies those that are the lowest within
      two hops, all at once, and rebuilds the tables.  It stops at the target or when a round finds nothing.

    `target_faces`: stop at this many faces; `ratio` in (0, 1]: at floor(ratio * F); each collapse removes two faces, so
    a reachable target is met to within one face.  `max_error` (world units): a collapse is allowed only while cost <=
    max_error^2 * (area_u + area_v), which bounds the area-weighted RMS distance from the kept position to the planes
    that the two vertices have accumulated.  It is NOT a Hausdorff bound: the distance between the surfaces can be
    larger (DESIGN.md has measured figures).  Alone, it decimates as far as the bound allows; with a target, both hold.

    All arithmetic is f64 in fixed order: the same bits on every call.  A target at or above the number of counting
    faces: nothing to do, the input tuple itself.  Otherwise faces that repeat an index and vertices that no face uses
    are dropped.  `return_map`: also vertex_map i32[V], the output vertex each input vertex was merged into, -1 where
    that vertex is not used by any face.  `return_info`: also a dict: rounds, collapses i64[rounds] (per round),
    max_cost (the largest accepted cost), removable and boundary bool[V] (the classes of the input's vertices).  Raises
    ValueError when none of the three is given, for a negative target_faces, a ratio outside (0, 1], a negative or
    non-finite max_error, a non-finite coordinate or a face index outside [0, V).  Host reads: the validation ranges
    with the number of counting faces, per round the table size and the number of collapses, and the output sizes."""
    mesh = tuple(mesh)
    verts, normals, faces_in, colors, per_vertex = _mesh_tuple_arg(mesh, "decimate_mesh", check=False)
    target_faces, ratio, max_error = _decimate_args(target_faces, ratio, max_error)
    _mesh_tuple_arg(mesh, "decimate_mesh", on_device=True)
    faces, V, F = _faces_arg(faces_in, verts.shape[0], False, "decimate_mesh")
    _m.ptr(faces)
    dev = verts.device
    i32 = dict(dtype=torch.int32, device=dev)

    def result(out, vertex_map, rounds=0, collapses=(), max_cost=0.0, vclass=None):
        if return_map:
            out = out + (vertex_map,)
        if return_info:
            vclass = torch.full((V,), _C["MSLAM_MESH_DECIMATE_ISOLATED"], dtype=torch.uint8, device=dev) \
                if vclass is None else vclass
            out = out + (dict(rounds=rounds, collapses=torch.tensor(list(collapses), dtype=torch.int64),
                              max_cost=float(max_cost), removable=vclass == _REMOVABLE, boundary=vclass == _BOUNDARY),)
        return out

    if V == 0 or F == 0:                                    # no face: nothing to remove
        return result(mesh, torch.arange(V, **i32))
    verts = verts.contiguous()
    if V * F >= 1 << 62:
        raise ValueError(f"decimate_mesh: {V} vertices x {F} faces overflow the pair keys")
    counting = ((faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])).sum()
    if _validate:                                           # one host read, the number of counting faces with it
        vlo, vhi, flo, fhi, finite, counting = _ranges(verts, faces, counting)
        _check_finite("decimate_mesh", vlo, vhi, finite)
        _check_face_range("decimate_mesh", flo, fhi, V)
    n_live = int(counting)                                  # indices are in range, so this is smooth_numpy.counting
    target = target_faces if target_faces is not None else math.floor(ratio * n_live) if ratio is not None else 0
    gate = -1.0 if max_error is None else max_error * max_error
    if target >= n_live and not return_info:                # nothing to do
        return result(mesh, torch.arange(V, **i32))
    L, stream = _m.lib(), _m.stream_ptr()
    cur = faces.clone()
    sorted_pairs, pair_start = _face_table(cur, V, F)
    state = torch.empty((V, _STATE), dtype=torch.float64, device=dev)
    _m.check(L.mslam_mesh_decimate_state(_m.ptr(verts), _m.ptr(cur), F, V, _m.ptr(sorted_pairs), _m.ptr(pair_start),
                                         _m.ptr(state), stream), "mesh_decimate_state")
    if target >= n_live:                                    # nothing to do but the classes
        return result(mesh, torch.arange(V, **i32), vclass=_Round(verts, cur, V, F, state, gate, 0, True).vclass)
    parent = torch.arange(V, **i32)
    collapses, vclass = [], None
    max_cost = torch.zeros((), dtype=torch.float64, device=dev)
    while n_live > target:
        rnd = len(collapses)
        tab = _Round(verts, cur, V, F, state, gate, rnd, return_info and rnd == 0)
        vclass = tab.vclass if rnd == 0 else vclass
        selected, rank = tab.select(V)
        n_sel = int(selected.sum())                         # the round's host read
        need = (n_live - target + 1) // 2
        if n_sel == 0:
            break
        if n_sel > need:                                    # the last round: the `need` lowest ranks
            bound = torch.sort(torch.where(selected, rank, _NO_RANK))[0][need - 1]
            selected = selected & (rank <= bound)
            n_sel = need
        max_cost = torch.maximum(max_cost, torch.where(selected, tab.cost, 0.0).max())
        _m.check(L.mslam_mesh_decimate_apply(_m.ptr(cur), F, V, _m.ptr(selected.to(torch.uint8)), _m.ptr(tab.best),
                                             _m.ptr(state), _m.ptr(parent), stream), "mesh_decimate_apply")
        collapses.append(n_sel)
        n_live -= 2 * n_sel                                 # a valid collapse removes the two faces on its edge
    flags = torch.zeros(V + F, **i32)
    end = torch.empty(V, **i32)
    _m.check(L.mslam_mesh_decimate_finish(_m.ptr(cur), F, V, _m.ptr(parent), len(collapses), _m.ptr(flags[V:]),
                                          _m.ptr(flags), _m.ptr(end), stream), "mesh_decimate_finish")
    out, out_faces, base, _ = _compact([t.contiguous() for t in per_vertex], cur, flags, V, F)
    vertex_map = None
    if return_map:
        e = end.long()
        vertex_map = torch.where(flags[:V][e] > 0, base[:V][e], -1).to(torch.int32)
    return result((out[0], out[1], out_faces, *out[2:]), vertex_map, len(collapses), collapses, max_cost, vclass)
