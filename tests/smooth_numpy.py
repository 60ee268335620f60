"""Numpy statement of mast3r_slam.tsdf.smooth_mesh and vertex_normals (csrc/mesh_smooth.hip, DESIGN.md "Mesh smoothing"):
Taubin's lambda|mu filter with uniform weights (Taubin, "A signal processing approach to fair surface design") and
area-weighted vertex normals from the winding.  The state is f64 from the f32 input to one final rounding, every sum is
sequential in the order the kernels use and every operation is rounded on its own, so the kernels' output equals this
one bit for bit.

  counting   a face counts when its three indices lie in [0, V) and are pairwise different; area plays no part.
  N(v)       the vertices that share an edge of a counting face with v, each once, ascending.
  m(v, u)    the number of counting faces that hold the undirected edge {v, u}; m = 1: a boundary edge.
  class      isolated: N(v) empty (the same as: no counting face uses v); boundary: some m(v, u) = 1; else interior.
  step(f)    S = 0.0 + x[u0] + x[u1] + ... over u in N(v) ascending, n = |N(v)|, x' = x + f * (S / n - x), all vertices at
             once from the previous state.  "fixed": boundary vertices are copied; "curve": a boundary vertex takes S and
             n over its neighbours with m = 1 only; "free": no distinction.  Isolated vertices are copied in every mode.
  iteration  step(lam), then step(mu); mu == 0: step(lam) alone.
  normals    s = the sum over the vertex's counting faces, in ascending face index, of (b - a) x (c - a) on the OUTPUT f32
             positions in f64; l = sqrt(sx sx + sy sy + sz sz); s / l when 0 < l < inf, else zero; the input normal for a
             vertex without a counting face.

Summation order.  S depends on the vertex numbering in its last bits.  One step with valence n and neighbours within R
of the origin: a sequential sum of n terms errs by at most (n - 1) u n R (u = 2^-53), the three further operations add
a few u R, so two numberings differ by at most about 2 (n + 3) u R per step and, the steps being averages of factor at
most max(1, |1 - 2 f|) <= 2.06 at the defaults, by RENUMBER_BOUND after all of them: far below the final f32 rounding,
which therefore differs by at most one f32 spacing, and only where the f64 value lies that close to a rounding tie."""
import numpy as np

U64 = 2.0 ** -53
MODES = ("fixed", "curve", "free")
INTERIOR, BOUNDARY, ISOLATED = 0, 1, 2


def counting(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def adjacency(faces, V):
    """(row_start i64[V+1], nbr i64[E], mult i64[E]): row v = nbr[row_start[v]:row_start[v+1]], ascending."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[counting(f, V)]
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    keys = np.concatenate([a * V + b, b * V + a, b * V + c, c * V + b, c * V + a, a * V + c])
    keys, mult = np.unique(keys, return_counts=True)
    row_start = np.searchsorted(keys, np.arange(V + 1, dtype=np.int64) * V)
    return row_start.astype(np.int64), (keys % max(V, 1)).astype(np.int64), mult.astype(np.int64)


def classify(faces, V):
    """(vclass u8[V], degree i32[V], n_edges): INTERIOR / BOUNDARY / ISOLATED, |N(v)|, the number of undirected edges."""
    row_start, nbr, mult = adjacency(faces, V)
    degree = np.diff(row_start)
    rim = np.zeros(V, np.int64)
    np.add.at(rim, np.repeat(np.arange(V), degree), (mult == 1).astype(np.int64))
    vclass = np.where(degree == 0, ISOLATED, np.where(rim > 0, BOUNDARY, INTERIOR)).astype(np.uint8)
    return vclass, degree.astype(np.int32), len(nbr) // 2


def _row_sums(x, row_start, nbr, use):
    """(S f64[V,3], n i64[V]): per row the sequential sum 0.0 + x[u0] + x[u1] + ... over its entries with use[j], in
    order.  Pass k adds the k-th used entry of every row that has one: one addition per row and pass, in row order."""
    V = len(x)
    S, n = np.zeros((V, 3)), np.zeros(V, np.int64)
    rows = np.repeat(np.arange(V), np.diff(row_start))[use]
    cols = nbr[use]
    if len(rows) == 0:
        return S, n
    first = np.searchsorted(rows, np.arange(V))                      # rows is ascending
    rank = np.arange(len(rows)) - first[rows]
    n = np.bincount(rows, minlength=V)
    for k in range(int(rank.max()) + 1):
        sel = rank == k
        S[rows[sel]] = S[rows[sel]] + x[cols[sel]]
    return S, n


def step(x, factor, adj, mode):
    row_start, nbr, mult = adj
    Sa, na = _row_sums(x, row_start, nbr, np.ones(len(nbr), bool))
    Sb, nb = _row_sums(x, row_start, nbr, mult == 1)
    isolated, boundary = na == 0, nb > 0
    along = boundary & (mode == "curve")
    moves = ~isolated & ~(boundary & (mode == "fixed"))
    S = np.where(along[:, None], Sb, Sa)
    n = np.where(along, nb, na).astype(np.float64)
    with np.errstate(all="ignore"):
        new = x + np.float64(factor) * (S / n[:, None] - x)
    return np.where(moves[:, None], new, x)


def smooth_positions(vertices, faces, iterations, lam=0.5, mu=-0.53, boundary="fixed"):
    """f32[V,3] after `iterations` iterations; the f64 state is rounded once, at the end."""
    assert boundary in MODES
    x = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    adj = adjacency(faces, len(x))
    for _ in range(int(iterations)):
        x = step(x, lam, adj, boundary)
        if mu != 0.0:
            x = step(x, mu, adj, boundary)
    return x.astype(np.float32)


def vertex_normals(vertices, faces, normals_in=None):
    p = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    V = len(p)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[counting(f, V)]                                            # order kept: ascending face index
    a = p[f[:, 0]]
    e1, e2 = p[f[:, 1]] - a, p[f[:, 2]] - a
    with np.errstate(all="ignore"):
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        s = np.zeros((V, 3))
        np.add.at(s, f.reshape(-1), np.repeat(n, 3, axis=0))         # face-major: ascending face index per vertex
        ln = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2])
        unit = (ln > 0.0) & (ln < np.inf)
        out = np.where(unit[:, None], s / np.where(unit, ln, 1.0)[:, None], 0.0).astype(np.float32)
    used = np.zeros(V, bool)
    used[f.reshape(-1)] = True
    keep = np.zeros((V, 3), np.float32) if normals_in is None else np.asarray(normals_in, np.float32).reshape(-1, 3)
    return np.where(used[:, None], out, keep)


def smooth(mesh, iterations, lam=0.5, mu=-0.53, boundary="fixed", normals="recompute", return_info=False):
    """mesh = (vertices f32[V,3], normals f32[V,3], faces i32[F,3][, colors f32[V,3]]) -> the same arity (+ a dict with
    boundary_vertex bool[V], degree i32[V], n_edges)."""
    assert normals in ("recompute", "keep")
    V, N, F = mesh[:3]
    if iterations is None or iterations <= 0:
        out = tuple(mesh)
    else:
        P = smooth_positions(V, F, iterations, lam, mu, boundary)
        out = (P, vertex_normals(P, F, N) if normals == "recompute" else N, F) + tuple(mesh[3:])
    if return_info:
        vclass, degree, n_edges = classify(F, len(V))
        out += (dict(boundary_vertex=vclass == BOUNDARY, degree=degree, n_edges=n_edges),)
    return out


def renumber_bound(iterations, max_valence, radius, lam=0.5, mu=-0.53):
    """RENUMBER_BOUND of the module docstring: the largest difference, in f64 before the final rounding, between the
    results of two vertex numberings of one mesh whose coordinates stay within `radius` of the origin."""
    per_step = 2.0 * (max_valence + 3) * U64 * radius
    steps = [lam] + ([mu] if mu != 0.0 else [])
    total = 0.0
    for _ in range(int(iterations)):
        for f in steps:
            total = total * max(1.0, abs(1.0 - 2.0 * f)) + per_step * max(1.0, abs(f))
    return total


# ----------------------------------------------------------------------------------------------------------------------
# hand meshes: name -> (vertices, faces).  What each is about stands in tests/test_mesh_smooth_cpu.py.
# ----------------------------------------------------------------------------------------------------------------------
_TET = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
FAN_VALENCE = 300


def _fan():
    t = 2.0 * np.pi * np.arange(FAN_VALENCE) / FAN_VALENCE
    rim = np.stack([np.cos(t), np.sin(t), 0.1 * np.cos(5 * t)], 1)
    V = np.concatenate([[[0.05, -0.03, 0.4]], rim])
    i = np.arange(FAN_VALENCE)
    return V, np.stack([np.zeros_like(i), 1 + i, 1 + (i + 1) % FAN_VALENCE], 1)


HAND = {
    "triangle": ([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5]], [[0, 1, 2]]),
    "two_triangles": ([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [0.0, 1.0, 0.0], [1.0, 1.0, 0.5]], [[0, 1, 2], [1, 3, 2]]),
    "tetrahedron": (_TET, [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]),
    # two triangles that meet in vertex 2 alone
    "bow_tie": ([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.5, 0.25], [0.0, 1.0, 0.0], [1.0, 1.0, 0.5]],
                [[0, 1, 2], [2, 4, 3]]),
    # three faces on the edge {0, 1}: m = 3, interior; their outer edges are boundary edges
    "three_on_an_edge": ([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.5], [-0.5, 0.75, 0.5], [-0.5, -0.75, 0.25]],
                         [[0, 1, 2], [0, 1, 3], [0, 1, 4]]),
    # the same face twice: every edge has m = 2, nothing is boundary
    "duplicated_face": ([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5]], [[0, 1, 2], [0, 1, 2]]),
    # the second face repeats an index and is ignored: vertex 3 is isolated
    "repeated_index": ([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5], [2.0, 2.0, 2.0]], [[0, 1, 2], [0, 3, 3]]),
    "isolated_vertex": (_TET + [[5.0, 5.0, 5.0]], [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]),
    "fan": _fan(),
}


def hand_mesh(name, colors=False):
    V, F = HAND[name]
    V = np.array(V, np.float32).reshape(-1, 3)
    rng = np.random.default_rng(len(V))
    N = rng.normal(size=V.shape)
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)
    F = np.array(F, np.int32).reshape(-1, 3)
    return (V, N, F) + ((rng.uniform(0, 1, V.shape).astype(np.float32),) if colors else ())


def noisy_sphere(sigma_voxels=0.3, seed=7):
    """(clean mesh, noisy mesh, centre, radius): sphere2 with radial Gaussian noise of sigma_voxels voxels."""
    import simplify_numpy as S

    V, N, F = S.shape_mesh("sphere2")
    c, r = np.array([0.3, -0.2, 0.1]), 0.31
    d = V.astype(np.float64) - c
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    noise = np.random.default_rng(seed).normal(0.0, sigma_voxels * S.VS, len(V))
    return (V, N, F), ((V.astype(np.float64) + noise[:, None] * u).astype(np.float32), N, F), c, r


def sphere_cap():
    """sphere2 with only the faces whose vertices all have z > c_z + 0.05: an open cap; the other vertices stay, unused."""
    import simplify_numpy as S

    V, N, F = S.shape_mesh("sphere2")
    keep = (V[F][:, :, 2] > 0.1 + 0.05).all(1)
    return V, N, np.ascontiguousarray(F[keep])
