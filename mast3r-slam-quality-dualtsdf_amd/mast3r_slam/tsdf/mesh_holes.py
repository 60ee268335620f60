"""Mesh holes on the device: the boundary loops of any welded mesh, and a centroid fan over the small, well-behaved ones.

No counterpart in the reference.  The kernels are csrc/mesh_holes.hip (DESIGN.md "Mesh holes"); the numpy statement of
the same definitions is tests/holes_numpy.py.  torch sorts and scans, the kernels do the rest.  Works on any welded mesh,
not only on what extract_mesh returns.  `bowties=True` pairs the boundary darts across the hole they bound, so that holes
which meet in a vertex are loops of their own (_pair, _tail_flag; tests/bowtie_numpy.py); it adds no host read.  Both
modes share one tracer: _trace, with _double and _loops.
"""
import operator

import torch

import mslam_hip as _m

from ._mesh_args import (_bool_arg, _check_face_range, _check_finite, _faces_arg, _mesh_arg, _mesh_tuple_arg,
                         _ranges)

_I32_MAX = (1 << 31) - 1


def _darts(faces, V, F):
    """(dart, tail, head) i32[B] of the boundary darts in ascending dart id.  One host read: B."""
    dev = faces.device
    L, stream = _m.lib(), _m.stream_ptr()
    keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
    _m.check(L.mslam_mesh_holes_keys(_m.ptr(faces), F, V, _m.ptr(keys), stream), "mesh_holes_keys")
    skeys, order = torch.sort(keys, stable=True)
    flag = torch.empty(3 * F, dtype=torch.uint8, device=dev)
    _m.check(L.mslam_mesh_holes_mark(_m.ptr(skeys), _m.ptr(order), 3 * F, _m.ptr(flag), stream), "mesh_holes_mark")
    dart = torch.nonzero(flag).reshape(-1).to(torch.int32)
    B = int(dart.shape[0])
    tail, head = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    _m.check(L.mslam_mesh_holes_darts(_m.ptr(faces), F, V, _m.ptr(dart), B, _m.ptr(tail), _m.ptr(head), stream),
             "mesh_holes_darts")
    return dart, tail, head


def _link(tail, head, V):
    """state i32[B,2]: per dart (next or -1, its tail)."""
    B = int(tail.shape[0])
    sorted_tail, tail_order = torch.sort(tail, stable=True)
    sorted_head = torch.sort(head)[0]
    state = torch.empty((B, 2), dtype=torch.int32, device=tail.device)
    _m.check(_m.lib().mslam_mesh_holes_link(_m.ptr(tail), _m.ptr(head), _m.ptr(sorted_tail), _m.ptr(tail_order),
                                            _m.ptr(sorted_head), B, V, _m.ptr(state), _m.stream_ptr()),
             "mesh_holes_link")
    return state


def _rounds(B):
    return (B - 1).bit_length() + 1                         # ceil(log2 B) + 1


def _double(state, rounds, entry="mesh_holes_double"):
    """`rounds` rounds of the pointer doubling `entry` (the labels' minimum, or mesh_holes_rank_double's sum of steps),
    between two spare buffers; `state` is left as it is."""
    B = int(state.shape[0])
    fn = getattr(_m.lib(), "mslam_" + entry)
    buf = [state, torch.empty_like(state), torch.empty_like(state)]
    cur = 0
    for _ in range(rounds):
        nxt = 1 if cur != 1 else 2
        _m.check(fn(_m.ptr(buf[cur]), _m.ptr(buf[nxt]), B, _m.stream_ptr()), entry)
        cur = nxt
    return buf[cur]


def _loops(state, labelled, flag=None, tail=None, head=None):
    """The loops among the cycles of `state`'s successors, `labelled` = _double(state): (loop_id i32[L], loop_head i32[L]
    or None, length i32[L], dart_loop i32[B], start i32[L], n_open i64[]).  One host read: L.  Plain mode: a cycle's
    label is its smallest tail and its loop's id.  Bow-tie mode passes `flag` (_tail_flag: the cycles that stay open),
    `tail` and `head`: a label is a dart's name, and loop_id and loop_head are the tail and the head of that dart."""
    B, dev = int(state.shape[0]), state.device
    L, stream = _m.lib(), _m.stream_ptr()
    keys = torch.empty(B + 1, dtype=torch.int32, device=dev)
    _m.check(L.mslam_mesh_holes_loop_labels(_m.ptr(labelled), _m.ptr(flag), B, _m.ptr(keys), stream),
             "mesh_holes_loop_labels")
    runs, counts = torch.unique_consecutive(torch.sort(keys)[0], return_counts=True)
    loop_name, length = runs[:-1].contiguous(), counts[:-1].to(torch.int32)       # the last run: the open darts, and one
    nl = int(loop_name.shape[0])
    dart_loop = torch.empty(B, dtype=torch.int32, device=dev)
    named = flag is not None
    unset = lambda: torch.full((nl,), -1, dtype=torch.int32, device=dev)
    start = unset()
    loop_id, loop_head = (unset(), unset()) if named else (None, None)
    _m.check(L.mslam_mesh_holes_loop_assign(_m.ptr(labelled), _m.ptr(state), _m.ptr(flag), _m.ptr(tail), _m.ptr(head),
                                            B, _m.ptr(loop_name), nl, _m.ptr(dart_loop), _m.ptr(start), _m.ptr(loop_id),
                                            _m.ptr(loop_head), stream), "mesh_holes_loop_assign")
    return loop_id if named else loop_name, loop_head, length, dart_loop, start, counts[-1] - 1


def _pair(faces, V, F, dart, tail, head):
    """Bow-tie mode's state i32[B,2]: per dart (next or -1, its name).  No host read."""
    dev, B = faces.device, int(dart.shape[0])
    L, stream = _m.lib(), _m.stream_ptr()
    i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)
    pairs = lambda: torch.empty((B, 2), dtype=torch.int32, device=dev)
    keys = i64(3 * F)
    _m.check(L.mslam_mesh_holes_dkeys(_m.ptr(faces), F, V, _m.ptr(keys), stream), "mesh_holes_dkeys")
    skeys, order = torch.sort(keys, stable=True)
    fan = torch.empty(B, dtype=torch.int32, device=dev)
    _m.check(L.mslam_mesh_holes_fan(_m.ptr(faces), F, V, _m.ptr(dart), _m.ptr(head), B, _m.ptr(skeys), _m.ptr(order),
                                    _m.ptr(fan), stream), "mesh_holes_fan")
    dart_key = keys[dart.long()]
    sorted_fan, sorted_dart_key = torch.sort(fan)[0], torch.sort(dart_key)[0]
    state = pairs()
    _m.check(L.mslam_mesh_holes_claim(_m.ptr(fan), _m.ptr(sorted_fan), _m.ptr(dart_key), _m.ptr(sorted_dart_key), B,
                                      _m.ptr(state), stream), "mesh_holes_claim")
    rounds = _rounds(B)
    labelled = _double(state, rounds)                       # the closed walks of fan, labelled by their smallest name
    rank = pairs()
    _m.check(L.mslam_mesh_holes_rank_init(_m.ptr(state), _m.ptr(labelled), B, _m.ptr(rank), stream),
             "mesh_holes_rank_init")
    rank = _double(rank, rounds, "mesh_holes_rank_double")  # (successor, steps)
    walk_keys = i64(B)
    _m.check(L.mslam_mesh_holes_walk_keys(_m.ptr(labelled), _m.ptr(rank), B, _m.ptr(walk_keys), stream),
             "mesh_holes_walk_keys")
    walk_keys, walk_order = torch.sort(walk_keys)           # distinct below INT64_MAX
    pair_keys = i64(B)
    _m.check(L.mslam_mesh_holes_pair_keys(_m.ptr(labelled), _m.ptr(head), _m.ptr(walk_keys), _m.ptr(walk_order), B, V,
                                          _m.ptr(pair_keys), stream), "mesh_holes_pair_keys")
    pair_keys, pair_order = torch.sort(pair_keys, stable=True)
    paired = pairs()
    _m.check(L.mslam_mesh_holes_repair(_m.ptr(pair_keys), _m.ptr(pair_order), _m.ptr(walk_order), _m.ptr(state), B,
                                       _m.ptr(paired), stream), "mesh_holes_repair")
    return paired


def _tail_flag(labelled, tail, V):
    """flag u8[B], by label: 1 for the cycles of bow-tie mode's next on which a vertex is a tail twice; they stay open."""
    B, dev = int(tail.shape[0]), tail.device
    L, stream = _m.lib(), _m.stream_ptr()
    tail_keys = torch.empty(B, dtype=torch.int64, device=dev)
    _m.check(L.mslam_mesh_holes_tail_keys(_m.ptr(labelled), _m.ptr(tail), B, V, _m.ptr(tail_keys), stream),
             "mesh_holes_tail_keys")
    tail_keys = torch.sort(tail_keys)[0]
    flag = torch.zeros(B, dtype=torch.uint8, device=dev)
    _m.check(L.mslam_mesh_holes_tail_flag(_m.ptr(tail_keys), B, V, _m.ptr(flag), stream), "mesh_holes_tail_flag")
    return flag


def _trace(faces, V, F, bowties=False):
    """The boundary of a mesh whose face indices lie in [0, V): dict of device tensors; in bow-tie mode `state` holds that
    mode's next and the dict has loop_head too.  Two host reads."""
    dev = faces.device
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    dart, tail, head = _darts(faces, V, F) if F and V else (i32(0), i32(0), i32(0))
    B = int(dart.shape[0])
    if B == 0:
        state, n_open = torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
        loop_id, loop_head, length, dart_loop, start = (i32(0) for _ in range(5))
    else:
        state = _pair(faces, V, F, dart, tail, head) if bowties else _link(tail, head, V)
        labelled = _double(state, _rounds(B))
        named = (_tail_flag(labelled, tail, V), tail, head) if bowties else ()
        loop_id, loop_head, length, dart_loop, start, n_open = _loops(state, labelled, *named)
    tr = dict(dart=dart, tail=tail, head=head, state=state, loop_id=loop_id, length=length, dart_loop=dart_loop,
              start=start, n_open=n_open)
    if bowties:
        tr["loop_head"] = loop_head
    return tr


def _measure(verts, faces, V, F, tr, max_edges, all_perimeters):
    """(perimeter f64[L], centre f64[L,3], fillable u8[L])."""
    nl, dev = int(tr["loop_id"].shape[0]), faces.device
    perimeter = torch.empty(nl, dtype=torch.float64, device=dev)
    centre = torch.empty((nl, 3), dtype=torch.float64, device=dev)
    fillable = torch.empty(nl, dtype=torch.uint8, device=dev)
    _m.check(_m.lib().mslam_mesh_holes_measure(_m.ptr(verts), _m.ptr(faces), F, V, _m.ptr(tr["dart"]),
                                               _m.ptr(tr["tail"]), _m.ptr(tr["head"]), _m.ptr(tr["state"]),
                                               int(tr["dart"].shape[0]), _m.ptr(tr["start"]), _m.ptr(tr["length"]), nl,
                                               min(int(max_edges), _I32_MAX), int(bool(all_perimeters)),
                                               _m.ptr(perimeter), _m.ptr(centre), _m.ptr(fillable), _m.stream_ptr()),
             "mesh_holes_measure")
    return perimeter, centre, fillable


def _info(tr, perimeter=None, filled=None):
    out = dict(loop_id=tr["loop_id"], loop_length=tr["length"], dart=tr["dart"], dart_tail=tr["tail"],
               dart_head=tr["head"], dart_loop=tr["dart_loop"],
               n_boundary_edges=torch.tensor(int(tr["dart"].shape[0]), dtype=torch.int64, device=tr["dart"].device),
               n_open=tr["n_open"])
    if "loop_head" in tr:
        out["loop_head"] = tr["loop_head"]
    if perimeter is not None:
        out["loop_perimeter"] = perimeter
    if filled is not None:
        out["loop_filled"] = filled
    return out


def mesh_boundaries(faces, num_vertices, vertices=None, bowties=False, _validate=True):
    """The boundary of any welded mesh (faces i32[F,3] device tensor over `num_vertices` vertices) as a dict of device
    tensors.  DESIGN.md "Mesh holes" has the definitions; in short: a boundary dart is a directed edge of a counting face
    (indices pairwise different), in the face's winding, whose undirected edge lies on exactly one counting face; its id
    is 3 face + corner.  A vertex is simple when exactly one boundary dart leaves it and one enters it; darts are chained
    through simple vertices; a closed chain is a loop, named by its smallest vertex.

      loop_id i32[L] ascending, loop_length i32[L]; dart, dart_tail, dart_head i32[B] in ascending dart id; dart_loop
      i32[B], the number of the dart's loop or -1 for an OPEN dart (bow-tie rims and chains that run into a vertex that is
      not simple); n_boundary_edges (B) and n_open, 0-d i64; with `vertices` f32[V,3] also loop_perimeter f64[L], the sum of
      the edge lengths in walk order (from the loop id along the winding) in f64.

    `bowties=True`: darts are paired across the hole they bound instead (DESIGN.md "Mesh holes", bow-tie mode): the
    successor of u -> v is found by rotating about v from the dart's face across interior edges, and a closed walk that
    visits a vertex several times is cut there, so the rims of holes that meet in a vertex are loops of their own.  OPEN
    are then only darts at non-manifold or inconsistently wound edges and cycles whose visits of two vertices
    interleave.  A loop is named by (its smallest vertex, the head of the dart leaving it); loops are numbered by
    ascending name, loop_id can repeat, and the dict also has loop_head i32[L].  No further host reads.

    L == 0 and n_open == 0: the mesh is watertight.  The result does not depend on the order of the faces.  Raises
    ValueError for a face index outside [0, V) or a `bowties` that is not a bool.  Host reads: the index range, B and
    L."""
    what = "mesh_boundaries"
    bowties = _bool_arg(bowties, "bowties", what)
    if vertices is not None:
        verts, faces, V, F = _mesh_arg(vertices, faces, _validate, what)
        if V != int(num_vertices):
            raise ValueError(f"{what}: vertices has {V} rows, num_vertices is {int(num_vertices)}")
    else:
        faces, V, F = _faces_arg(faces, num_vertices, _validate, what)
        _m.ptr(faces)
    tr = _trace(faces, V, F, bowties)
    perimeter = None
    if vertices is not None:
        perimeter = _measure(verts, faces, V, F, tr, 0, True)[0]
    return _info(tr, perimeter)


def fill_holes(mesh, max_edges, return_info=False, bowties=False, _validate=True):
    """Closes the small holes of `mesh` = (vertices f32[V,3], normals f32[V,3], faces i32[F,3][, colors f32[V,3]]), the
    tuple extract_mesh / filter_mesh / smooth_mesh / simplify_mesh use; the result has the same arity.  DESIGN.md "Mesh
    holes" has the definitions; in short:

    - the boundary loops are those of mesh_boundaries; the centre of a loop is the f64 mean of its vertices in walk order;
    - a loop of n edges is filled when 3 <= n <= `max_edges` and every fan face (head, tail, centre) of its darts turns
      the way of the dart's own face (the f64 product of the two face normals is > 0).  That tells a hole from the outer
      rim of a patch, whose fan would cover the patch a second time, flipped, and refuses folded loops;
    - a filled loop appends one vertex (the centre rounded to f32; normal: the normalised sum of the fan faces' normals;
      colour: the mean of the loop's colours) and n faces (head, tail, centre), wound like the faces across the edges.

    The first V rows of the vertex tensors and the first F faces are the input's bits; then the new vertices by ascending
    loop id, then the new faces by loop id and walk order.  The result does not depend on the order of the faces, and on
    the vertex numbering only through the order of the sums.  Open darts are never filled.  When no loop is filled the
    input tuple itself is returned.

    `bowties=True`: the loops are those of mesh_boundaries(bowties=True), so holes that meet in a vertex are closed too;
    new vertices and faces then follow in the order of the loops' names.  No further host reads.

    `max_edges` None or <= 0: off, the input tuple itself.  `return_info`: also the dict of mesh_boundaries (with
    loop_perimeter) plus loop_filled bool[L].  Raises ValueError for a `max_edges` that is not an integer, a `bowties`
    that is not a bool, a non-finite coordinate or a face index outside [0, V), before any kernel follows an index.
    Host reads: the validation ranges, B, L and the new sizes."""
    what = "fill_holes"
    bowties = _bool_arg(bowties, "bowties", what)
    mesh = tuple(mesh)
    verts_in, nrm_in, faces_in, colors, _ = _mesh_tuple_arg(mesh, what, check=False)
    if max_edges is not None:
        try:
            max_edges = operator.index(max_edges)
        except TypeError:
            raise ValueError(f"{what}: max_edges must be an integer, got {max_edges!r}") from None
    off = max_edges is None or max_edges <= 0
    if off and not return_info:
        return mesh
    _mesh_tuple_arg(mesh, what, on_device=True)
    faces, V, F = _faces_arg(faces_in, verts_in.shape[0], False, what)
    _m.ptr(faces)
    verts = verts_in.contiguous()
    if _validate and V and F:                               # one host read
        vlo, vhi, flo, fhi, finite = _ranges(verts, faces)
        _check_finite(what, vlo, vhi, finite)
        _check_face_range(what, flo, fhi, V)
    dev = verts.device
    tr = _trace(faces, V, F, bowties)
    nl = int(tr["loop_id"].shape[0])
    perimeter, centre, fillable = _measure(verts, faces, V, F, tr, 0 if off else max_edges, return_info)
    out, filled = mesh, fillable.bool()
    if nl and not off:
        fl = fillable.to(torch.int64)
        fn = fl * tr["length"]
        vend, fend = torch.cumsum(fl, 0), torch.cumsum(fn, 0)
        new_v, new_f = (int(x) for x in torch.stack([vend[-1], fend[-1]]).cpu())         # one host read
        if V + new_v > _I32_MAX or 3 * (F + new_f) > _I32_MAX:
            raise ValueError(f"{what}: {V + new_v} vertices / {F + new_f} faces are outside the int32 index range")
        if new_v:
            grown = lambda t, k: torch.cat([t, torch.empty((k, 3), dtype=t.dtype, device=dev)])
            out_v, out_n, out_f = grown(verts, new_v), grown(nrm_in, new_v), grown(faces, new_f)
            col = None if colors is None else colors.contiguous()
            out_c = None if colors is None else grown(col, new_v)
            vbase, fbase = vend - fl, fend - fn             # exclusive scans
            _m.check(_m.lib().mslam_mesh_holes_emit(
                _m.ptr(verts), _m.ptr(col), _m.ptr(tr["tail"]), _m.ptr(tr["head"]), _m.ptr(tr["state"]),
                int(tr["dart"].shape[0]), _m.ptr(tr["start"]), _m.ptr(tr["length"]), _m.ptr(fillable),
                _m.ptr(vbase), _m.ptr(fbase), nl, V, F, new_v, new_f, _m.ptr(centre), _m.ptr(out_v),
                _m.ptr(out_n), _m.ptr(out_c), _m.ptr(out_f), _m.stream_ptr()), "mesh_holes_emit")
            out = (out_v, out_n, out_f) + (() if colors is None else (out_c,))
    if return_info:
        out = out + (_info(tr, perimeter, filled),)
    return out
