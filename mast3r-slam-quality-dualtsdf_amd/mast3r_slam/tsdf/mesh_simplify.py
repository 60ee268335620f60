"""Mesh simplification on the device: vertices clustered on a uniform grid, each cluster's vertex placed by the plane
quadrics of the faces that touch its cell (Lindstrom, "Out-of-core simplification of large polygonal models").

No counterpart in the reference.  The kernels are csrc/mesh_simplify.hip (DESIGN.md "Mesh simplification"); the numpy
statement of the same definitions is tests/simplify_numpy.py.  torch sorts and scans, the kernels do the rest, and the
gather at the end is mesh_ops' mslam_mesh_cc_emit.  Works on any welded mesh, not only on what extract_mesh returns.
"""
import math

import torch

import mslam_hip as _m

from ._mesh_args import _check_face_range, _check_finite, _faces_arg, _mesh_tuple_arg, _ranges
from .mesh_ops import _compact

_KEY_LIMIT = 1 << 20                    # cell keys per axis lie in [-2^20, 2^20): the voxel hash's 21-bit signed range


def _validate_ranges(verts, faces, V, c):
    """One host read: the coordinate range (finite, cells within the key range) and the face index range."""
    vlo, vhi, flo, fhi, finite = _ranges(verts, faces)
    _check_finite("simplify_mesh", vlo, vhi, finite)
    klo, khi = vlo / c, vhi / c
    if not (klo >= -_KEY_LIMIT and math.floor(khi) < _KEY_LIMIT):
        raise ValueError(f"simplify_mesh: cells span [{math.floor(klo) if math.isfinite(klo) else klo}, "
                         f"{math.floor(khi) if math.isfinite(khi) else khi}] at cell_size {c}, outside "
                         f"[{-_KEY_LIMIT}, {_KEY_LIMIT})")
    _check_face_range("simplify_mesh", flo, fhi, V)


def simplify_mesh(mesh, cell_size, position="quadric", return_map=False, _validate=True, _two_pass=False):
    """Simplifies `mesh` = (vertices f32[V,3], normals f32[V,3], faces i32[F,3][, colors f32[V,3]]), the tuple
    extract_mesh / filter_mesh use, by clustering its vertices on a grid of `cell_size` (world units); the result has the
    same arity.  DESIGN.md "Mesh simplification" has the definitions; in short:

    - a vertex lies in cell floor(p / cell_size); the occupied cells, in lexicographic (x, y, z) order, are the clusters;
    - a face whose vertices lie in three different clusters survives, rotated so that its smallest cluster is first
      (orientation kept); survivors are sorted, equal triples are kept once.  Two faces of opposite orientation are
      different triples and both stay; a zero-area face survives like any other;
    - the output vertices are the clusters a kept face uses, in cluster order: a canonical mesh stays canonical, and the
      result does not depend on the order of the input faces;
    - position="mean": the mean of the cluster's vertices; "quadric" (default): the minimiser of the summed plane
      quadrics of the faces touching the cell, moved from the mean only along directions whose eigenvalue exceeds 1e-3
      of the largest, and replaced by the mean when it leaves the cell.  Normals are the normalised sum, colours the
      mean, of the cluster's vertices.

    Every output vertex lies in its cell's closed box (up to the final f32 rounding), so every point of an output face is
    within sqrt(3) * cell_size of the corresponding point of the input face it came from: the one-sided distance
    output -> input is at most sqrt(3) * cell_size.  The other direction has NO such bound: sheets closer than a cell
    merge and features thinner than a cell collapse.  All arithmetic is f64 in fixed order: the same bits on every call.

    `cell_size` None or <= 0: off, the input tensors themselves.  `return_map`: also vertex_map i32[V], the output vertex
    of each input vertex, -1 where its cluster is not used by any kept face.  Raises ValueError for a cell_size that is
    not finite, a non-finite coordinate, a cell outside the 21-bit key range or a face index outside [0, V).  Host reads:
    the validation ranges, the number of clusters, the output sizes.  `_two_pass` forces the face sort that meshes of
    1.6 M clusters and more take (two stable passes instead of one packed key); the result is the same."""
    mesh = tuple(mesh)
    verts, normals, faces, colors, per_vertex = _mesh_tuple_arg(mesh, "simplify_mesh", check=False)
    if position not in ("quadric", "mean"):
        raise ValueError(f"simplify_mesh: position must be 'quadric' or 'mean', got {position!r}")
    c = None if cell_size is None else float(cell_size)
    if c is not None and not math.isfinite(c):
        raise ValueError(f"simplify_mesh: cell_size must be finite, got {c}")
    if c is None or c <= 0.0:
        if not return_map:
            return mesh
        return mesh + (torch.arange(int(verts.shape[0]), dtype=torch.int32, device=verts.device),)
    _mesh_tuple_arg(mesh, "simplify_mesh", on_device=True)
    faces, V, F = _faces_arg(faces, verts.shape[0], False, "simplify_mesh")
    _m.ptr(faces)
    dev = verts.device
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)

    def result(out, out_faces, vertex_map):
        return (out[0], out[1], out_faces, *out[2:]) + ((vertex_map,) if return_map else ())

    if V == 0 or F == 0:                                    # no face, so no cluster is used
        return result([torch.empty((0, 3), dtype=torch.float32, device=dev) for _ in per_vertex],
                      torch.empty((0, 3), **i32), torch.full((V,), -1, **i32))
    verts, normals = verts.contiguous(), normals.contiguous()
    colors = colors.contiguous() if colors is not None else None
    if _validate:
        _validate_ranges(verts, faces, V, c)
    L, stream = _m.lib(), _m.stream_ptr()
    # clusters: stable sort of the cell keys, heads of the runs, one cumsum
    keys = torch.empty(V, **i64)
    _m.check(L.mslam_mesh_simplify_keys(_m.ptr(verts), V, c, _m.ptr(keys), stream), "mesh_simplify_keys")
    sorted_keys, vorder = torch.sort(keys, stable=True)
    head = torch.ones(V, dtype=torch.bool, device=dev)
    head[1:] = sorted_keys[1:] != sorted_keys[:-1]
    cid = torch.cumsum(head, 0) - 1
    C = int(cid[-1]) + 1
    if C * F >= 1 << 62:
        raise ValueError(f"simplify_mesh: {C} clusters x {F} faces overflow the pair keys")
    cluster = torch.empty(V, **i32)
    cluster[vorder] = cid.to(torch.int32)
    ids = torch.arange(C + 1, **i64)
    vstart = torch.searchsorted(cid, ids)
    # faces: rotated triples and their sort keys, (cluster, face) pairs
    packed = not _two_pass and C ** 3 < 1 << 62
    tri = torch.empty((F, 3), **i32)
    key_lo = torch.empty(F, **i64)
    key_hi = None if packed else torch.empty(F, **i64)
    pairs = torch.empty(3 * F, **i64)
    _m.check(L.mslam_mesh_simplify_faces(_m.ptr(faces), F, V, _m.ptr(cluster), C, int(packed), _m.ptr(tri),
                                         _m.ptr(key_hi), _m.ptr(key_lo), _m.ptr(pairs), stream), "mesh_simplify_faces")
    if packed:
        forder = torch.sort(key_lo, stable=True)[1]
    else:                                                   # two stable passes: (t1, t2), then t0
        first = torch.sort(key_lo, stable=True)[1]
        forder = first[torch.sort(key_hi[first], stable=True)[1]]
    out = [torch.empty((C, 3), dtype=torch.float32, device=dev) for _ in per_vertex]
    quadric = position == "quadric"
    sorted_pairs = pstart = None
    if quadric:
        sorted_pairs = torch.sort(pairs)[0]
        pstart = torch.searchsorted(sorted_pairs, ids * F)
    _m.check(L.mslam_mesh_simplify_solve(_m.ptr(verts), _m.ptr(normals), _m.ptr(colors), _m.ptr(faces), F, V, c,
                                         _m.ptr(sorted_keys), _m.ptr(vorder), _m.ptr(vstart), _m.ptr(sorted_pairs),
                                         _m.ptr(pstart), C, int(quadric), _m.ptr(out[0]), _m.ptr(out[1]),
                                         _m.ptr(out[2]) if colors is not None else 0, 0, stream), "mesh_simplify_solve")
    # kept faces and the clusters they use
    flags = torch.zeros(C + F, **i32)
    sorted_tri = torch.empty((F, 3), **i32)
    _m.check(L.mslam_mesh_simplify_mark(_m.ptr(tri), _m.ptr(forder), F, C, _m.ptr(sorted_tri), _m.ptr(flags[C:]),
                                        _m.ptr(flags), stream), "mesh_simplify_mark")
    res, out_faces, base, _ = _compact(out, sorted_tri, flags, C, F)
    vertex_map = None
    if return_map:
        cl = cluster.long()
        vertex_map = torch.where(flags[:C][cl] > 0, base[:C][cl], -1).to(torch.int32)
    return result(res, out_faces, vertex_map)
