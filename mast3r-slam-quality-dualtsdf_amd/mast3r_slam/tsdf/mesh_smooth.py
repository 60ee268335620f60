"""Mesh smoothing on the device: Taubin's lambda|mu filter with uniform weights (Taubin, "A signal processing approach
to fair surface design") over a per-vertex neighbour table, and vertex normals from the winding over a per-vertex face
table.

No counterpart in the reference.  The kernels are csrc/mesh_smooth.hip (DESIGN.md "Mesh smoothing"); the numpy statement
of the same definitions is tests/smooth_numpy.py.  torch sorts and scans, the kernels do the rest.  Works on any welded
mesh, not only on what extract_mesh returns.
"""
import math
import operator

import torch

import mslam_hip as _m

from ._mesh_args import _check_face_range, _check_finite, _faces_arg, _mesh_arg, _mesh_tuple_arg, _ranges

_C = _m.header_constants()
_MODES = {k: _C["MSLAM_MESH_SMOOTH_" + k.upper()] for k in ("fixed", "curve", "free")}
_BOUNDARY = _C["MSLAM_MESH_SMOOTH_BOUNDARY"]
_STRIDE = 3                             # doubles per vertex of the f64 state: packed; 4 measured slower


def _neighbour_table(faces, V, F):
    """(row_start i64[V+1], nbr i32[E'], mult i32[E'], E'): row v = the neighbours of v, each once, ascending, and how
    many counting faces hold each edge.  E' counts one entry past the rows when a face does not count; the rows end at
    row_start[V].  One host read, in unique_consecutive: the number of distinct keys."""
    dev = faces.device
    keys = torch.empty(6 * F, dtype=torch.int64, device=dev)
    _m.check(_m.lib().mslam_mesh_smooth_edges(_m.ptr(faces), F, V, _m.ptr(keys), _m.stream_ptr()), "mesh_smooth_edges")
    ukeys, mult = torch.unique_consecutive(torch.sort(keys)[0], return_counts=True)
    row_start = torch.searchsorted(ukeys, torch.arange(V + 1, dtype=torch.int64, device=dev) * V)
    return row_start, (ukeys % V).to(torch.int32), mult.to(torch.int32), int(ukeys.shape[0])


def _face_table(faces, V, F):
    """(sorted_pairs i64[3F], pair_start i64[V+1]): the counting faces of every vertex in ascending face index."""
    pairs = torch.empty(3 * F, dtype=torch.int64, device=faces.device)
    _m.check(_m.lib().mslam_mesh_vertex_faces(_m.ptr(faces), F, V, _m.ptr(pairs), _m.stream_ptr()), "mesh_vertex_faces")
    sorted_pairs = torch.sort(pairs)[0]
    ids = torch.arange(V + 1, dtype=torch.int64, device=faces.device)
    return sorted_pairs, torch.searchsorted(sorted_pairs, ids * F)


def _normals(verts, faces, V, F, normals_in, what):
    if V * F >= 1 << 62:
        raise ValueError(f"{what}: {V} vertices x {F} faces overflow the pair keys")
    out = torch.empty((V, 3), dtype=torch.float32, device=verts.device)
    sorted_pairs, pair_start = _face_table(faces, V, F)
    _m.check(_m.lib().mslam_mesh_vertex_normals(_m.ptr(verts), _m.ptr(faces), F, V, _m.ptr(sorted_pairs),
                                                _m.ptr(pair_start), _m.ptr(normals_in), _m.ptr(out), _m.stream_ptr()),
             "mesh_vertex_normals")
    return out


def vertex_normals(vertices, faces, _validate=True):
    """Unit normals f32[V,3] of any welded mesh (vertices f32[V,3], faces i32[F,3], device tensors; what
    evaluate.load_mesh returns, moved to the device): per vertex the normalised sum, over its faces in ascending face
    index, of (b - a) x (c - a) in f64.  Area-weighted, and it follows the winding: counter-clockwise seen from free
    space gives normals into free space, as extract_mesh's are.  A face with an index outside [0, V) raises ValueError;
    one with a repeated index is ignored.  Zero where the sum is zero or not finite and where no face uses the vertex."""
    verts, faces, V, F = _mesh_arg(vertices, faces, _validate, "vertex_normals")
    if V == 0:
        return torch.empty((0, 3), dtype=torch.float32, device=verts.device)
    return _normals(verts, faces, V, F, None, "vertex_normals")


def smooth_mesh(mesh, iterations, lam=0.5, mu=-0.53, boundary="fixed", normals="recompute", return_info=False,
                _validate=True):
    """Smooths `mesh` = (vertices f32[V,3], normals f32[V,3], faces i32[F,3][, colors f32[V,3]]), the tuple extract_mesh
    / filter_mesh / simplify_mesh use, by `iterations` Taubin iterations; the result has the same arity.  DESIGN.md "Mesh
    smoothing" has the definitions; in short:

    - a face counts when its indices are pairwise different (area plays no part); N(v) are the vertices that share an
      edge of a counting face with v; an edge on exactly one counting face is a boundary edge, a vertex with one a
      boundary vertex;
    - one step with factor f moves every vertex at once, from the previous state: x' = x + f * (mean of N(v) - x); one
      iteration is a step with `lam`, then one with `mu` (negative, a little larger in size: it undoes the shrinkage of
      the first).  `mu` = 0: the `lam` step alone, plain Laplacian smoothing, which shrinks;
    - boundary="fixed" (default): boundary vertices keep their input bits; "curve": a boundary vertex averages over the
      neighbours behind its boundary edges only, so the rim is smoothed as a curve; "free": no distinction.  Vertices
      that no counting face uses keep their input bits in every mode;
    - normals="recompute" (default): vertex_normals of the output positions (the input normal where no counting face
      uses the vertex); "keep": the input normals.

    Faces, colours, V, F and both orders are unchanged (faces and colours are the input tensors themselves), so a
    canonical mesh stays canonical.  The state is f64 from the f32 input to one final rounding and every sum runs in
    ascending index: the same bits on every call, whatever the order of the faces.  The result DOES depend on the vertex
    numbering in its last bits, because the neighbour sums run in index order (tests/smooth_numpy.py bounds it).

    `iterations` None or <= 0: off, the input tuple itself.  `return_info`: also a dict of device tensors, boundary_vertex
    bool[V], degree i32[V] (|N(v)|) and n_edges (the number of undirected edges).  Raises ValueError for an `iterations`
    that is not an integer, a `lam` or `mu` that is not finite, an unknown `boundary` or `normals`, a non-finite
    coordinate or a face index outside [0, V).  Host reads: the validation ranges and the number of directed edges."""
    mesh = tuple(mesh)
    verts, nrm_in, faces_in, colors, _ = _mesh_tuple_arg(mesh, "smooth_mesh", check=False)
    if iterations is not None:
        try:
            iterations = operator.index(iterations)
        except TypeError:
            raise ValueError(f"smooth_mesh: iterations must be an integer, got {iterations!r}") from None
    lam, mu = float(lam), float(mu)
    if not (math.isfinite(lam) and math.isfinite(mu)):
        raise ValueError(f"smooth_mesh: lam and mu must be finite, got {lam} and {mu}")
    if boundary not in _MODES:
        raise ValueError(f"smooth_mesh: boundary must be 'fixed', 'curve' or 'free', got {boundary!r}")
    if normals not in ("recompute", "keep"):
        raise ValueError(f"smooth_mesh: normals must be 'recompute' or 'keep', got {normals!r}")
    off = iterations is None or iterations <= 0
    if off and not return_info:
        return mesh
    _mesh_tuple_arg(mesh, "smooth_mesh", on_device=True)
    faces, V, F = _faces_arg(faces_in, verts.shape[0], False, "smooth_mesh")
    _m.ptr(faces)
    dev = verts.device
    if V == 0 or F == 0:                                    # no face, so nothing has a neighbour
        info = dict(boundary_vertex=torch.zeros(V, dtype=torch.bool, device=dev),
                    degree=torch.zeros(V, dtype=torch.int32, device=dev),
                    n_edges=torch.zeros((), dtype=torch.int64, device=dev))
        return mesh + ((info,) if return_info else ())
    verts = verts.contiguous()
    if _validate:                                           # one host read
        vlo, vhi, flo, fhi, finite = _ranges(verts, faces)
        _check_finite("smooth_mesh", vlo, vhi, finite)
        _check_face_range("smooth_mesh", flo, fhi, V)
    L, stream = _m.lib(), _m.stream_ptr()
    row_start, nbr, mult, E = _neighbour_table(faces, V, F)
    vclass = torch.empty(V, dtype=torch.uint8, device=dev) if return_info else None
    state = [torch.zeros((V, _STRIDE), dtype=torch.float64, device=dev) for _ in range(2)]
    state[0][:, :3] = verts                                 # f32 -> f64 is exact
    cur = 0
    steps = [] if off else ([lam] if mu == 0.0 else [lam, mu]) * iterations
    if off:                                                 # the classes alone: a step of factor 0 into the spare state
        steps = [0.0]
    for i, f in enumerate(steps):
        _m.check(L.mslam_mesh_smooth_step(_m.ptr(state[cur]), _m.ptr(state[1 - cur]), _STRIDE, _m.ptr(row_start),
                                          _m.ptr(nbr), _m.ptr(mult), V, E, f, _MODES[boundary],
                                          _m.ptr(vclass) if i == 0 else 0, stream), "mesh_smooth_step")
        cur = 1 - cur
    if off:
        out = mesh
    else:
        out_verts = state[cur][:, :3].to(torch.float32).contiguous()       # one rounding, to nearest even
        out_nrm = nrm_in
        if normals == "recompute":
            out_nrm = _normals(out_verts, faces, V, F, nrm_in.contiguous(), "smooth_mesh")
        out = (out_verts, out_nrm, faces_in) + mesh[3:]
    if return_info:
        info = dict(boundary_vertex=vclass == _BOUNDARY, degree=(row_start[1:] - row_start[:-1]).to(torch.int32),
                    n_edges=row_start[V] // 2)
        out = out + (info,)
    return out
