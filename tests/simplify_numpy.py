"""Numpy statement of mast3r_slam.tsdf.simplify_mesh (csrc/mesh_simplify.hip, DESIGN.md "Mesh simplification"): vertex
clustering on a uniform grid with quadric placement (Lindstrom, "Out-of-core simplification of large polygonal models").
Everything is f64 on the f32 inputs, every sum is sequential in the order the kernels use (np.add.at visits its operands
in order: ascending vertex index within a cluster, ascending face index within a cluster), and a * b + c is two
roundings.  The eigen-decomposition is np.linalg.eigh; the kernel's is a cyclic Jacobi, so quadric positions agree to
the final f32 rounding, everything else exactly.

  cell      k = floor(p / c) per axis; x0 = (k + 0.5) c is the cell's centre.
  cluster   the distinct cells that hold a vertex, numbered in ascending packed key (mc_numpy.pack: lexicographic x,y,z).
  faces     a face whose vertices lie in three different clusters survives as (cl a, cl b, cl c) rotated so that the
            smallest id is first; the survivors are sorted lexicographically and equal triples are kept once.  Opposite
            orientations are different triples: both stay.
  vertices  the clusters a kept face references, in cluster order.
  mean      m = (sum of (p - x0)) / n.
  quadric   over the valid faces (meshdist_numpy.triangles' rule) that touch the cluster, once per face:
            n = (b - a) x (c - a), u = n / |n|, w = |n| / 2, d = -u . (a - x0), A += w u u^T, b += w d u;
            r = -b - A m; x = m + sum over eigenpairs with lambda_i > 1e-3 lambda_max of e_i (e_i . r) / lambda_i;
            x = m when lambda_max <= 0, when any |x_j| > c / 2 or when x is not finite.
  normal    the sum of the cluster's normals, normalised (zero when the sum is zero); colour: sum / n."""
import functools

import numpy as np

import mc_numpy as M
import meshdist_numpy as D
from mc_numpy import pack

EIG_REL = 1.0e-3


def _cells(vertices, c):
    p = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    k = np.floor(p / np.float64(c)).astype(np.int64)
    return p, k


def clusters(vertices, c):
    """(cluster i64[V], cell i64[C,3]): the cluster of every vertex and the cell key of every cluster."""
    p, k = _cells(vertices, c)
    if len(p) == 0:
        return np.zeros(0, np.int64), np.zeros((0, 3), np.int64)
    pk = pack(k)
    order = np.argsort(pk, kind="stable")
    head = np.concatenate([[True], pk[order][1:] != pk[order][:-1]])
    cl = np.empty(len(p), np.int64)
    cl[order] = np.cumsum(head) - 1
    return cl, k[order][head]


def cluster_faces(faces, cl, num_clusters):
    """Sorted, de-duplicated surviving triples i64[F',3] in cluster ids."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(cl))).all(1)
    t = cl[np.where(ok[:, None], f, 0)] if len(cl) else np.zeros((len(f), 3), np.int64)
    ok &= (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    t = t[ok]
    if len(t) == 0:
        return np.zeros((0, 3), np.int64)
    first = np.argmin(t, 1)
    t = np.stack([t[np.arange(len(t)), (first + j) % 3] for j in range(3)], 1)
    return np.unique(t, axis=0)                                      # lexicographic, each triple once


def _seq_sum(index, values, n):
    """out[i] = values[j0] + values[j1] + ... over the j with index[j] == i, in ascending j, starting from 0.0."""
    out = np.zeros((n,) + values.shape[1:])
    np.add.at(out, index, values)
    return out


def quadrics(p, faces, cl, x0):
    """(A f64[C,6] as xx, xy, xz, yy, yz, zz; b f64[C,3]) summed over each cluster's faces in ascending face index."""
    C = len(x0)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    in_range = ((f >= 0) & (f < len(p))).all(1)
    f = f[in_range]                                                  # order kept: ascending face index
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    e1, e2 = b - a, c - a
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    valid = (n != 0.0).any(1)
    f, a, n = f[valid], a[valid], n[valid]
    ln = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    u = n / ln[:, None]
    wu = (0.5 * ln)[:, None] * u
    t = cl[f]
    # one contribution per distinct cluster of the face, face-major: ascending face index within every cluster
    use = np.stack([np.ones(len(f), bool), t[:, 1] != t[:, 0], (t[:, 2] != t[:, 0]) & (t[:, 2] != t[:, 1])], 1)
    rel = a[:, None, :] - x0[t]                                      # [F,3 slots,3]
    d = -(u[:, None, 0] * rel[:, :, 0] + u[:, None, 1] * rel[:, :, 1] + u[:, None, 2] * rel[:, :, 2])
    A6 = np.stack([wu[:, 0] * u[:, 0], wu[:, 0] * u[:, 1], wu[:, 0] * u[:, 2], wu[:, 1] * u[:, 1], wu[:, 1] * u[:, 2],
                   wu[:, 2] * u[:, 2]], 1)
    A6 = np.broadcast_to(A6[:, None, :], (len(f), 3, 6))
    b3 = wu[:, None, :] * d[:, :, None]
    return _seq_sum(t[use], A6[use], C), _seq_sum(t[use], b3[use], C)


def solve(A6, b, m, c):
    """(x f64[C,3], fallback bool[C], eigenvalues f64[C,3] ascending)."""
    C = len(m)
    A = np.empty((C, 3, 3))
    for (i, j), k in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(6)):
        A[:, i, j] = A[:, j, i] = A6[:, k]
    r = np.stack([-b[:, i] - (A[:, i, 0] * m[:, 0] + A[:, i, 1] * m[:, 1] + A[:, i, 2] * m[:, 2]) for i in range(3)], 1)
    lam, E = np.linalg.eigh(A) if C else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    lmax = lam[:, 2] if C else np.zeros(0)
    x = m.copy()
    with np.errstate(all="ignore"):
        for i in range(3):
            e = E[:, :, i]
            step = e * ((e * r).sum(1) / lam[:, i])[:, None]
            x = x + np.where((lam[:, i] > EIG_REL * lmax)[:, None], step, 0.0)
        fallback = ~(lmax > 0.0) | (np.abs(x) > 0.5 * c).any(1) | ~np.isfinite(x).all(1)
    return np.where(fallback[:, None], m, x), fallback, lam


def simplify(mesh, cell_size, position="quadric", return_map=False, return_info=False):
    """mesh = (vertices f32[V,3], normals f32[V,3], faces i32[F,3][, colors f32[V,3]]) -> the same arity (+ vertex_map
    i32[V]) (+ a dict of per-cluster intermediates)."""
    assert position in ("quadric", "mean")
    V, N, F = mesh[:3]
    c = np.float64(cell_size)
    p, _ = _cells(V, c)
    cl, cell = clusters(V, c)
    C = len(cell)
    x0 = (cell.astype(np.float64) + 0.5) * c
    tri = cluster_faces(F, cl, C)
    ref = np.zeros(C, bool)
    ref[tri.reshape(-1)] = True
    remap = np.cumsum(ref) - 1
    cnt = np.bincount(cl, minlength=C).astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        m = _seq_sum(cl, p - x0[cl], C) / cnt
        fallback, lam = np.ones(C, bool), np.zeros((C, 3))
        x = m
        if position == "quadric":
            A6, b = quadrics(p, F, cl, x0)
            x, fallback, lam = solve(A6, b, m, c)
        s = _seq_sum(cl, np.asarray(N, np.float32).astype(np.float64).reshape(-1, 3), C)
        ln = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2])
        nrm = np.where(ln[:, None] > 0.0, s / np.where(ln > 0.0, ln, 1.0)[:, None], 0.0)
    out = ((x0 + x)[ref].astype(np.float32), nrm[ref].astype(np.float32), remap[tri].astype(np.int32).reshape(-1, 3))
    if len(mesh) == 4:
        col = _seq_sum(cl, np.asarray(mesh[3], np.float32).astype(np.float64).reshape(-1, 3), C) / cnt
        out += (col[ref].astype(np.float32),)
    if return_map:
        out += (np.where(ref[cl], remap[cl], -1).astype(np.int32),)
    if return_info:
        out += (dict(cluster=cl, cell=cell[ref], x0=x0[ref], fallback=fallback[ref], eig=lam[ref], referenced=ref),)
    return out


def out_to_in(simplified, original, radius, n=2000, seed=1):
    """Distances f64[n] from n area-weighted samples of `simplified` (meshdist_numpy.sample) to the mesh `original`:
    exact wherever the distance is <= radius, +inf where no face of `original` comes that close.  Only faces whose box,
    grown by `radius`, holds the sample are measured (meshdist_numpy.tri_dist2 on the flat list of such pairs)."""
    cdf = np.cumsum(D.face_areas(simplified[0], simplified[2]))
    pts = D.sample(simplified[0], simplified[2], cdf, n, seed=seed)[0].astype(np.float64)
    a, b, c, valid = D.triangles(original[0], original[2])
    a, b, c = a[valid], b[valid], c[valid]
    lo, hi = np.minimum(np.minimum(a, b), c) - radius, np.maximum(np.maximum(a, b), c) + radius
    best = np.full(n, np.inf)
    for s in range(0, n, 250):
        p = pts[s:s + 250]
        pi, fi = np.nonzero(((p[:, None, :] >= lo[None]) & (p[:, None, :] <= hi[None])).all(2))
        d2 = D.tri_dist2(p[pi], a[fi], b[fi], c[fi])
        np.minimum.at(best, s + pi, d2)
    d = np.sqrt(best)
    return np.where(d <= radius, d, np.inf)


def box_sdf(centre, half):
    centre, half = np.asarray(centre, np.float64), np.asarray(half, np.float64)

    def f(P):
        q = np.abs(P - centre) - half
        return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(1), 0.0)
    return f


# analytic fixtures: marching-cubes meshes (mc_numpy.extract, voxel size VS, band 3 VS, min_weight 0.5) of three closed
# shapes, with what the statement gives at c = 2 VS: name -> (sdf, lo, hi, V, F, V', F', Euler number)
VS = 0.03
_BOX_C, _BOX_H = np.array([0.012, 0.02, -0.01]), np.array([0.2, 0.14, 0.17])
SHAPES = {
    "sphere2": (M.sphere_sdf((0.3, -0.2, 0.1), 0.31), np.array([0.3, -0.2, 0.1]) - 0.31, np.array([0.3, -0.2, 0.1]) + 0.31,
                2006, 4008, 394, 784, 2),
    "torus": (M.torus_sdf((0.01, 0.0, 0.0), 0.3, 0.1), (-0.45, -0.45, -0.15), (0.45, 0.45, 0.15), 1784, 3568, 356, 712, 0),
    "box": (box_sdf(_BOX_C, _BOX_H), _BOX_C - _BOX_H, _BOX_C + _BOX_H, 718, 1432, 185, 366, 2),
}


@functools.lru_cache(maxsize=None)
def shape_voxels(name):
    sdf, lo, hi = SHAPES[name][:3]
    return M.sample_sdf(sdf, lo, hi, VS, 3 * VS)


@functools.lru_cache(maxsize=None)
def shape_mesh(name):
    return M.extract(*shape_voxels(name), VS, 0.5)


@functools.lru_cache(maxsize=None)
def shape_reference(name, voxels_per_cell, position):
    """simplify(shape_mesh(name), voxels_per_cell * VS, position) with the vertex map and the intermediates, once."""
    return simplify(shape_mesh(name), voxels_per_cell * VS, position, return_map=True, return_info=True)


def renumber(mesh, perm):
    """The same mesh with vertex v renamed perm[v]."""
    inv = np.argsort(perm)
    V, N, F = mesh[:3]
    return (V[inv], N[inv], np.asarray(perm)[F].astype(np.int32)) + tuple(c[inv] for c in mesh[3:])


def grid_patch(nx, ny, seed, jitter=0.2, spacing=1.0):
    """A planar nx x ny grid in z ~ 1 with in-plane and out-of-plane jitter, every coordinate positive, two faces per quad:
    (vertices f32[nx ny,3], normals f32[nx ny,3], faces i32[2 (nx-1)(ny-1),3], colors f32[nx ny,3])."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    P = np.stack([i, j, np.zeros_like(i)], -1).reshape(-1, 3).astype(np.float64)
    P = (P + 1.0 + rng.uniform(-jitter, jitter, P.shape)) * spacing
    v = (i * ny + j)[:-1, :-1].reshape(-1)
    faces = np.concatenate([np.stack([v, v + ny, v + ny + 1], 1), np.stack([v, v + ny + 1, v + 1], 1)])
    nrm = rng.normal(size=P.shape) * 0.2 + np.array([0.0, 0.0, 1.0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return P.astype(np.float32), nrm.astype(np.float32), faces.astype(np.int32), rng.uniform(0, 1, P.shape).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# hand-built meshes: name -> dict(vertices, faces, cell, out_faces, vertex_map[, positions | mean_positions][, fallback]),
# written out by hand.  `positions` hold in both modes (exactly for the mean, to rounding for the quadric),
# `mean_positions` for the mean only; `fallback`: the clusters whose quadric position is their mean, bit for bit.
# Clusters are numbered by ascending (x, y, z) cell.
# ----------------------------------------------------------------------------------------------------------------------
_TRI = [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]]           # cells (0,0,0), (1,0,0), (0,1,0): clusters 0, 2, 1
_G4 = [0.25, 0.75, 1.25, 1.75]
_PATCH_V = [[x, y, 0.25] for x in _G4 for y in _G4]                    # vertex 4 i + j
_PATCH_F = [t for i in range(3) for j in range(3)
            for t in ([4 * i + j, 4 * i + j + 4, 4 * i + j + 5], [4 * i + j, 4 * i + j + 5, 4 * i + j + 1])]

HAND = {
    # vertices 2 and 3 share cell (0,1,0): both faces become (0, 2, 1) and one is kept
    "fan_duplicate": dict(vertices=_TRI + [[0.625, 1.375, 0.5]], faces=[[0, 1, 2], [0, 1, 3]], cell=1.0,
                          out_faces=[[0, 2, 1]], vertex_map=[0, 2, 1, 1]),
    # the second face has two vertices in cell (0,1,0): collapsed
    "collapsed": dict(vertices=_TRI + [[0.625, 1.375, 0.5]], faces=[[0, 1, 2], [0, 2, 3]], cell=1.0,
                      out_faces=[[0, 2, 1]], vertex_map=[0, 2, 1, 1]),
    # the same triangle in both orientations: two different triples, both stay, sorted
    "opposite_pair": dict(vertices=_TRI, faces=[[0, 1, 2], [0, 2, 1]], cell=1.0, out_faces=[[0, 1, 2], [0, 2, 1]],
                          vertex_map=[0, 2, 1]),
    # vertex 3 in cell (0,0,1) = cluster 1 belongs to no face: the clusters behind it move up
    "unreferenced": dict(vertices=_TRI + [[0.5, 0.5, 1.5]], faces=[[0, 1, 2]], cell=1.0, out_faces=[[0, 2, 1]],
                         vertex_map=[0, 2, 1, -1]),
    # c = 0.5.  -0.5 = -1 c lies in cell -1; -0.125 lies in cell -1 by floor (truncation would say 0), so vertices 0 and
    # 3 share cell (-1,0,0).  Cells (-1,-1,1), (-1,0,0), (1,0,0) are clusters 0, 1, 2; both faces become (0, 1, 2).
    "boundary_negative": dict(vertices=[[-0.5, 0.0, 0.0], [0.5, 0.0, 0.0], [-0.25, -0.25, 0.5], [-0.125, 0.0, 0.0]],
                              faces=[[0, 1, 2], [3, 1, 2]], cell=0.5, out_faces=[[0, 1, 2]], vertex_map=[1, 2, 0, 1],
                              mean_positions=[[-0.25, -0.25, 0.5], [-0.3125, 0.0, 0.0], [0.5, 0.0, 0.0]]),
    # three collinear vertices in three cells: the face survives, no quadric, every cluster at its mean
    "zero_area": dict(vertices=[[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5]], faces=[[0, 1, 2]], cell=1.0,
                      out_faces=[[0, 1, 2]], vertex_map=[0, 1, 2],
                      positions=[[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5]], fallback=[True, True, True]),
    # a 4 x 4 grid in the plane z = 0.25, four vertices per cell; only the central quad's two faces span three cells.
    # The plane is the only constraint: the quadric moves nothing, x == mean to rounding.
    "planar_patch": dict(vertices=_PATCH_V, faces=_PATCH_F, cell=1.0, out_faces=[[0, 2, 3], [0, 3, 1]],
                         vertex_map=[0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3],
                         positions=[[0.5, 0.5, 0.25], [0.5, 1.5, 0.25], [1.5, 0.5, 0.25], [1.5, 1.5, 0.25]]),
    # two steep planes through vertices 0 and 1 of cell (0,0,0) meet in the ridge x = 0.5, z = 2, 1.5 above the cell's
    # centre: outside the box, so cluster 0 falls back to its mean (0.5, 0.5, 0.125)
    "tent": dict(vertices=[[0.25, 0.5, 0.125], [0.75, 0.5, 0.125], [0.5, 0.25, 2.0], [0.5, 1.25, 2.0]],
                 faces=[[0, 2, 3], [1, 3, 2]], cell=1.0, out_faces=[[0, 1, 2], [0, 2, 1]], vertex_map=[0, 0, 1, 2],
                 positions=[[0.5, 0.5, 0.125], [0.5, 0.25, 2.0], [0.5, 1.25, 2.0]], fallback=[True, False, False]),
}


def hand_mesh(name, colors=False):
    h = HAND[name]
    V = np.array(h["vertices"], np.float32).reshape(-1, 3)
    rng = np.random.default_rng(len(V))
    N = rng.normal(size=V.shape)
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)
    F = np.array(h["faces"], np.int32).reshape(-1, 3)
    return (V, N, F) + ((rng.uniform(0, 1, V.shape).astype(np.float32),) if colors else ())
