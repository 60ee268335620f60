"""Numpy statement of the mesh index (DESIGN.md "Mesh index"; the kernels are csrc/mesh_index.hip and md_box_kernel of
csrc/mesh_tri.h): the Morton keys of faces and of query points, the face order, the boxes of the tiles of 128 faces in
that order and of the groups of 32 tiles, and the scans over the permuted tiles with their tie rule by ORIGINAL face
index.  Everything is f64 on the f32 inputs, and the operation order written here is the kernel's."""
import numpy as np

import meshdist_numpy as D
import raycast_numpy as R

TILE = 128         # kMdTile of csrc/mesh_tri.h: faces per tile
GROUP = 32         # kMdGroup: tiles per group
BITS = 21          # kMiBits of csrc/mesh_index.hip: bits per axis of a key
NONE = np.iinfo(np.int64).max


def bounds(vertices):
    """f32[6] = lo.xyz, hi.xyz of the vertices (zeros without one): what the caller hands to the key kernel."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    return np.concatenate([v.min(0), v.max(0)]) if len(v) else np.zeros(6, np.float32)


def spread(x):
    """bits 0..20 of x (uint64) moved to every third bit"""
    x = x & np.uint64(0x1fffff)
    for shift, mask in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f),
                        (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(shift))) & np.uint64(mask)
    return x


def morton(c, bnd):
    """int64[n]: per axis floor((c - lo) / (hi - lo) * 2^21) clamped to [0, 2^21) by fmax then fmin (a NaN is cell 0),
    interleaved with x highest."""
    c = np.asarray(c, np.float64).reshape(-1, 3)
    b = np.asarray(bnd, np.float32).astype(np.float64)
    key = np.zeros(len(c), np.uint64)
    with np.errstate(all="ignore"):
        for d in range(3):
            u = (c[:, d] - b[d]) / (b[3 + d] - b[d]) * float(1 << BITS)
            q = np.fmin(np.fmax(np.floor(u), 0.0), float((1 << BITS) - 1))
            key |= spread(q.astype(np.uint64)) << np.uint64(2 - d)
    return key.astype(np.int64)


def face_keys(vertices, faces, bnd=None):
    """int64[F]: the Morton code of the centroid ((a + b) + c) / 3 of each valid face, INT64_MAX for an invalid one."""
    a, b, c, valid = D.triangles(vertices, faces)
    with np.errstate(all="ignore"):
        keys = morton(((a + b) + c) / 3.0, bounds(vertices) if bnd is None else bnd)
    return np.where(valid, keys, NONE)


def point_keys(points, bnd):
    return morton(np.asarray(points, np.float32).astype(np.float64), bnd)


def order_of(keys):
    """int32[F]: the stable sort of the keys."""
    return np.argsort(keys, kind="stable").astype(np.int32)


def boxes(vertices, faces, order):
    """(tile f64[ntiles,6], group f64[ngroups,6]): lo.xyz, hi.xyz over the corners of the valid faces order[128 t + k]
    of tile t, an entry of `order` outside [0, F) skipped; then over the tiles 32 g .. 32 g + 31 of group g.  An empty
    tile or group is (+inf, -inf)."""
    a, b, c, valid = D.triangles(vertices, faces)
    nf = len(valid)
    order = np.asarray(order, np.int64)
    ntiles = (nf + TILE - 1) // TILE
    ngroups = (ntiles + GROUP - 1) // GROUP
    tile = np.tile(np.array([np.inf] * 3 + [-np.inf] * 3), (ntiles, 1))
    for t in range(ntiles):
        o = order[TILE * t:TILE * (t + 1)]
        o = o[(o >= 0) & (o < nf)]
        o = o[valid[o]]
        if len(o):
            pts = np.concatenate([a[o], b[o], c[o]])
            with np.errstate(all="ignore"):
                tile[t, :3], tile[t, 3:] = np.fmin.reduce(pts, 0), np.fmax.reduce(pts, 0)
    group = np.tile(np.array([np.inf] * 3 + [-np.inf] * 3), (ngroups, 1))
    for g in range(ngroups):
        part = tile[GROUP * g:GROUP * (g + 1)]
        group[g, :3], group[g, 3:] = np.fmin.reduce(part[:, :3], 0), np.fmax.reduce(part[:, 3:], 0)
    return tile, group


def closest_in_order(points, vertices, faces, order, tie="index"):
    """(dist2, nearest) of a scan that visits the faces in `order`.  tie "index": d < best or (d == best and f < best_f)
    on the original index f, the rule of the indexed scan; "first": strict <, the first face met wins - what a
    permuted scan would do without the rule."""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    a, b, c, valid = D.triangles(vertices, faces)
    best = np.full(len(p), np.inf)
    nearest = np.full(len(p), -1, np.int32)
    for f in np.asarray(order, np.int64):
        if not (0 <= f < len(valid)) or not valid[f]:
            continue
        d = D.tri_dist2(p, a[f], b[f], c[f])
        better = d < best
        if tie == "index":
            better |= (d == best) & (f < nearest)
        best = np.where(better, d, best)
        nearest = np.where(better, np.int32(f), nearest)
    return best, nearest


def cast_in_order(o, d, vertices, faces, order, near, far, tie="index"):
    """(t64, face) of a cast that visits the faces in `order`, with the same two tie rules on t: one face at a time
    through raycast_numpy.cast, so the arithmetic is that statement's."""
    nf = len(np.asarray(faces).reshape(-1, 3))
    best = np.full(len(d), np.inf)
    face = np.full(len(d), -1, np.int32)
    F = np.asarray(faces, np.int32).reshape(-1, 3)
    for f in np.asarray(order, np.int64):
        if not 0 <= f < nf:
            continue
        t, hit = R.cast(o, d, vertices, F[f:f + 1], near, far)
        got = hit >= 0
        better = got & (t < best)
        if tie == "index":
            better |= got & (t == best) & (f < face)
        best = np.where(better, t, best)
        face = np.where(better, np.int32(f), face)
    return best, face
