"""Numpy statement of mast3r_slam.tsdf.decimate_mesh (csrc/mesh_decimate.hip, DESIGN.md "Mesh decimation"): round-based
half-edge collapse with plane quadrics (Garland & Heckbert, "Surface simplification using quadric error metrics").  A
removed vertex u is merged into a neighbour v, so every output vertex is an input vertex with its input bits.  All
arithmetic is f64 on the f32 input, every sum is sequential in the order the kernels use and every operation is rounded
on its own, so the kernels' decisions, and with them the output, equal this one bit for bit.

  counting   smooth_numpy.counting on the CURRENT faces: indices in [0, V), pairwise different.  N(v), m(v, w) and the
             face list of a vertex are smooth_numpy's, on the current counting faces.
  plane      of an input face (a, b, c): n = (b - a) x (c - a), l = sqrt((nx nx + ny ny) + nz nz); it contributes only
             when 0 < l < inf.  k = n / l, A = 0.5 l, d = -((kx ax + ky ay) + kz az), g = (kx, ky, kz, d).
  state      S[v] f64[11], once, from the input: entries 0..9 the quadric in the order xx xy xz xd yy yz yd zz zd dd,
             entry ij = (A g_i) g_j; entry 10 = A.  S[v] = 0.0 + the entries of its counting faces that contribute, in
             ascending face index.
  removable  u has a neighbour, every edge at u has m = 2, and the number of its faces equals |N(u)|.
  cost(u, v) Q = S[u] + S[v] entry by entry, (x, y, z) = position of v,
             r0 = ((Qxx x + Qxy y) + Qxz z) + Qxd, r1 = ((Qxy x + Qyy y) + Qyz z) + Qyd,
             r2 = ((Qxz x + Qyz y) + Qzz z) + Qzd, r3 = ((Qxd x + Qyd y) + Qzd z) + Qdd,
             c = ((r0 x + r1 y) + r2 z) + r3; cost = c when c > 0, else 0.0.
  valid      u -> v, v in N(u), is valid when u is removable and
             link   exactly two vertices lie in both N(u) and N(v), and neither of the two has three neighbours or fewer
                    and as many faces as neighbours (a closed fan of three faces loses one and would be left as two
                    faces back to back, as in a tetrahedron; a rim vertex may get down to one face);
             flip   every face (a, b, c) of u that does not hold v, with o = (b - a) x (c - a) and o' the same on the face
                    with u replaced by v (corner order kept), has (o'x ox + o'y oy) + o'z oz > 0: the new face has area and
                    has not turned over (a face of u without area therefore blocks u);
             gate   with max_error given: cost <= (max_error * max_error) * (S[u][10] + S[v][10]).
  best(u)    the valid v of lowest (cost, v); u is a candidate when it has one.
  hash32     x = (u * 0x9E3779B1 + round * 0x85EBCA77) mod 2^32, then x ^= x >> 16, x *= 0x85EBCA6B, x ^= x >> 13,
             x *= 0xC2B2AE35, x ^= x >> 16, all mod 2^32 (the finaliser of MurmurHash3).  round counts from 0.
  rank       the position of a candidate under (cost, hash32(u, round), u); 2^31 - 1 for every other vertex.
  selected   m1[w] = min of rank over w and N(w), m2[u] = min of m1 over u and N(u); a candidate is selected when
             m2[u] == rank[u]: it is the lowest within two hops, so two selected vertices are at least three hops apart.
             With need = ceil((F_live - target) / 2) and more than need selected, the need lowest ranks stay.
  apply      per selected u, v = best(u): S[v] = S[v] + S[u] entry by entry, parent[u] = v, and every face corner u
             becomes v.  Exactly the two faces on the edge {u, v} stop counting.
  stop       before a round when F_live <= target; after a round that selected nothing.  target = target_faces, else
             floor(ratio * F_counting), else 0; target >= F_counting: nothing is done and the input is the result.
  emit       the vertices that a counting face uses, in their order, with their normals and colours; the counting faces
             in their order, re-indexed.  vertex_map[w] = the output index of the end of w's parent chain, -1 when no
             counting face uses that vertex."""
import functools

import numpy as np

import smooth_numpy as T

NO_RANK = 2 ** 31 - 1
_M32 = np.uint64(0xFFFFFFFF)
# (i, j) of the ten quadric entries over g = (kx, ky, kz, d)
ENTRIES = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))


def hash32(u, rnd):
    x = (np.asarray(u, np.uint64) * np.uint64(0x9E3779B1) + np.uint64(rnd) * np.uint64(0x85EBCA77)) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & _M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & _M32
    return x ^ (x >> np.uint64(16))


def _cross(a, b, c):
    e1, e2 = b - a, c - a
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)


def initial_state(p, faces):
    """S f64[V,11] from the f64 positions and the input faces."""
    V = len(p)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[T.counting(f, V)]                                          # order kept: ascending face index
    a = p[f[:, 0]]
    n = _cross(a, p[f[:, 1]], p[f[:, 2]])
    with np.errstate(all="ignore"):
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = (ln > 0.0) & (ln < np.inf)
        f, a, n, ln = f[ok], a[ok], n[ok], ln[ok]
        k = n / ln[:, None]
        area = 0.5 * ln
        d = -((k[:, 0] * a[:, 0] + k[:, 1] * a[:, 1]) + k[:, 2] * a[:, 2])
        g = np.concatenate([k, d[:, None]], 1)
        w = area[:, None] * g
        rows = np.stack([w[:, i] * g[:, j] for i, j in ENTRIES] + [area], 1)
    S = np.zeros((V, 11))
    np.add.at(S, f.reshape(-1), np.repeat(rows, 3, axis=0))          # face-major: ascending face index per vertex
    return S


def costs(S, p, u, v):
    Q = S[u] + S[v]
    x, y, z = p[v, 0], p[v, 1], p[v, 2]
    xx, xy, xz, xd, yy, yz, yd, zz, zd, dd = (Q[:, i] for i in range(10))
    r0 = ((xx * x + xy * y) + xz * z) + xd
    r1 = ((xy * x + yy * y) + yz * z) + yd
    r2 = ((xz * x + yz * y) + zz * z) + zd
    r3 = ((xd * x + yd * y) + zd * z) + dd
    c = ((r0 * x + r1 * y) + r2 * z) + r3
    return np.where(c > 0.0, c, 0.0)


def _expand(counts):
    """(owner, offset) of sum(counts) slots: slot s belongs to owner[s] and is its offset[s]-th."""
    owner = np.repeat(np.arange(len(counts)), counts)
    first = np.cumsum(counts) - counts
    return owner, np.arange(len(owner)) - first[owner]


def candidates(p, cur, S, e2):
    """One round's tables and best collapses on the current faces `cur` i64[F,3] ->
    dict(row_start, nbr, rows, removable bool[V], boundary bool[V], best i64[V] (-1: none), cost f64[V] (inf: none))."""
    V = len(p)
    row_start, nbr, mult = T.adjacency(cur, V)
    deg = np.diff(row_start)
    rows = np.repeat(np.arange(V), deg)
    live = T.counting(cur, V)
    lf = cur[live]
    nfaces = np.bincount(lf.reshape(-1), minlength=V)
    odd = np.bincount(rows, mult != 2, minlength=V)
    rim = np.bincount(rows, mult == 1, minlength=V)
    removable = (deg > 0) & (odd == 0) & (nfaces == deg)
    best, cost = np.full(V, -1, np.int64), np.full(V, np.inf)
    out = dict(row_start=row_start, nbr=nbr, rows=rows, removable=removable, boundary=rim > 0, best=best, cost=cost)
    e = np.nonzero(removable[rows])[0]
    if len(e) == 0:
        return out
    u, v = rows[e], nbr[e]
    c = costs(S, p, u, v)
    valid = np.ones(len(e), bool)
    if e2 is not None:
        valid &= c <= np.float64(e2) * (S[u, 10] + S[v, 10])
    # link: the w of N(u) that are in N(v) too
    keys = rows * V + nbr                                            # ascending
    own, off = _expand(deg[u])
    w = nbr[row_start[u[own]] + off]
    q = v[own] * V + w
    pos = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
    both = keys[pos] == q
    valid &= np.bincount(own, both, minlength=len(e)) == 2
    valid &= np.bincount(own, both & (deg[w] <= 3) & (nfaces[w] == deg[w]), minlength=len(e)) == 0
    # flip: the faces of u, from the (vertex, face) pairs in ascending order
    vf = np.sort(lf.reshape(-1) * len(cur) + np.repeat(np.nonzero(live)[0], 3))
    fstart = np.searchsorted(vf, np.arange(V) * len(cur))
    own, off = _expand(nfaces[u])
    tri = cur[vf[fstart[u[own]] + off] % len(cur)]
    uu, vv = u[own][:, None], v[own][:, None]
    new = np.where(tri == uu, vv, tri)
    o = _cross(p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]])
    n = _cross(p[new[:, 0]], p[new[:, 1]], p[new[:, 2]])
    dot = (n[:, 0] * o[:, 0] + n[:, 1] * o[:, 1]) + n[:, 2] * o[:, 2]
    blocks = ~(tri == vv).any(1) & ~(dot > 0.0)
    valid &= np.bincount(own, blocks, minlength=len(e)) == 0
    u, v, c = u[valid], v[valid], c[valid]
    order = np.lexsort((v, c, u))                                    # by u, then (cost, v)
    u, v, c = u[order], v[order], c[order]
    first = np.concatenate([[True], u[1:] != u[:-1]]) if len(u) else np.zeros(0, bool)
    best[u[first]], cost[u[first]] = v[first], c[first]
    return out


def select(tab, rnd, need, tie="hash"):
    """(selected vertices ascending by rank, rank i64[V])."""
    V = len(tab["best"])
    cand = np.nonzero(tab["best"] >= 0)[0]
    h = hash32(cand, rnd) if tie == "hash" else np.zeros(len(cand), np.uint64)
    order = np.lexsort((cand, h, tab["cost"][cand]))
    rank = np.full(V, NO_RANK, np.int64)
    rank[cand[order]] = np.arange(len(cand))
    m1 = rank.copy()
    np.minimum.at(m1, tab["rows"], rank[tab["nbr"]])
    m2 = m1.copy()
    np.minimum.at(m2, tab["rows"], m1[tab["nbr"]])
    sel = cand[order][(m2 == rank)[cand[order]]]
    return sel[:max(int(need), 0)], rank


def resolve_target(n_counting, target_faces, ratio, max_error):
    if target_faces is None and ratio is None and max_error is None:
        raise ValueError("decimate: one of target_faces, ratio and max_error is needed")
    if target_faces is not None:
        return int(target_faces)
    if ratio is not None:
        return int(np.floor(np.float64(ratio) * n_counting))
    return 0


def decimate(mesh, target_faces=None, ratio=None, max_error=None, return_map=False, return_info=False, tie="hash",
             trace=False):
    """mesh = (vertices f32[V,3], normals f32[V,3], faces i32[F,3][, colors f32[V,3]]) -> the same arity (+ vertex_map
    i32[V]) (+ dict(rounds, collapses i64[rounds], max_cost, removable bool[V], boundary bool[V]; with `trace` also
    `trace`: per round dict(faces, u, v, cost, area))).  `tie` = "index" drops the hash from the rank: for the test of
    the tie-break only, the kernels have no such mode."""
    P, N, F = mesh[:3]
    V = len(P)
    p = np.asarray(P, np.float32).astype(np.float64).reshape(-1, 3)
    cur = np.asarray(F, np.int64).reshape(-1, 3).copy()
    n_live = int(T.counting(cur, V).sum())
    target = resolve_target(n_live, target_faces, ratio, max_error)
    e2 = None if max_error is None else float(max_error) * float(max_error)
    S = initial_state(p, cur)
    parent = np.arange(V)
    collapses, rounds_trace, max_cost = [], [], 0.0
    first = candidates(p, cur, S, e2) if return_info else None
    done = target >= n_live
    while not done and n_live > target:
        rnd = len(collapses)
        tab = candidates(p, cur, S, e2) if rnd or first is None else first
        u, _ = select(tab, rnd, (n_live - target + 1) // 2, tie)
        if len(u) == 0:
            break
        v = tab["best"][u]
        if trace:
            rounds_trace.append(dict(faces=cur.copy(), u=u, v=v, cost=tab["cost"][u], area=S[u, 10] + S[v, 10]))
        max_cost = max(max_cost, float(tab["cost"][u].max()))
        S[v] = S[v] + S[u]
        parent[u] = v
        step = np.arange(V)
        step[u] = v
        cur = step[cur]
        collapses.append(len(u))
        n_live = int(T.counting(cur, V).sum())
    if done:
        out = tuple(mesh)
        vmap = np.arange(V, dtype=np.int32)
    else:
        live = T.counting(cur, V)
        used = np.zeros(V, bool)
        used[cur[live].reshape(-1)] = True
        index = np.cumsum(used) - 1
        end = parent.copy()
        while (parent[end] != end).any():
            end = parent[end]
        out = (P[used], N[used], index[cur[live]].astype(np.int32).reshape(-1, 3)) + tuple(c[used] for c in mesh[3:])
        vmap = np.where(used[end], index[end], -1).astype(np.int32)
    if return_map:
        out += (vmap,)
    if return_info:
        info = dict(rounds=len(collapses), collapses=np.array(collapses, np.int64), max_cost=max_cost,
                    removable=first["removable"], boundary=first["boundary"])
        if trace:
            info["trace"] = rounds_trace
        out += (info,)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# fixtures and checks
# ----------------------------------------------------------------------------------------------------------------------
PLATE = ((0.012, 0.02, -0.01), (0.2, 0.14, 0.02))                    # simplify_numpy.box_sdf: 1.3 voxels thick
TARGETS = {"sphere2": 784, "torus": 712, "box": 366, "plate": 146}  # what clustering reaches at two voxels per cell
EULER = {"sphere2": 2, "torus": 0, "box": 2, "plate": 2}


@functools.lru_cache(maxsize=None)
def fixture(name):
    import mc_numpy as M
    import simplify_numpy as S

    if name != "plate":
        return S.shape_mesh(name)
    c, h = np.array(PLATE[0]), np.array(PLATE[1])
    return M.extract(*M.sample_sdf(S.box_sdf(c, h), c - h, c + h, S.VS, 3 * S.VS), S.VS, 0.5)


@functools.lru_cache(maxsize=None)
def fixture_reference(name):
    """decimate(fixture(name), TARGETS[name]) with the map and the traced info, once."""
    return decimate(fixture(name), TARGETS[name], return_map=True, return_info=True, trace=True)


def disc(rings, n=6):
    """(vertices f32, faces i32): a flat fan of n faces around vertex 0 with rings - 1 rings of quads around it, every
    face counter-clockwise.  The last ring is the rim; everything inside is interior, and every cost is zero."""
    V, F = [[0.0, 0.0, 0.0]], []
    for r in range(1, rings + 1):
        t = 2 * np.pi * (np.arange(n) + 0.5 * r) / n
        V += [[r * np.cos(a), r * np.sin(a), 0.0] for a in t]
    F += [[0, 1 + i, 1 + (i + 1) % n] for i in range(n)]
    for r in range(1, rings):
        a0, b0 = 1 + (r - 1) * n, 1 + r * n
        for i in range(n):
            j = (i + 1) % n
            F += [[a0 + i, b0 + i, a0 + j], [a0 + j, b0 + i, b0 + j]]
    return np.array(V, np.float32), np.array(F, np.int32)


def notched_fan():
    """(vertices f32, faces i32): a flat fan around vertex 0 inside a ring that makes the fan's rim interior: three pairs
    of coplanar quads.  The rim is not convex: vertex 3 is pulled in past the centre, so moving 0 onto 1 or 2 turns the
    faces next to 3 over, while moving it onto 3 itself is fine.  Every cost is zero: only the flip test tells them apart."""
    rim = [[1.0, 0.0], [0.5, 0.9], [-0.1, -0.05], [-1.0, 0.0], [-0.5, -0.9], [0.5, -0.9]]
    outer = [[2.0 * x, 2.0 * y] if i != 2 else [-0.6, 1.2] for i, (x, y) in enumerate(rim)]
    V = [[0.1, -0.3, 0.0]] + [[x, y, 0.0] for x, y in rim] + [[x, y, 0.0] for x, y in outer]
    F = [[0, 1 + i, 1 + (i + 1) % 6] for i in range(6)]
    for i in range(6):
        F += [[1 + i, 7 + i, 1 + (i + 1) % 6], [1 + (i + 1) % 6, 7 + i, 7 + (i + 1) % 6]]
    return np.array(V, np.float32), np.array(F, np.int32)


def topology(faces, V):
    """(closed, consistently wound, Euler number V_used - E + F) of the counting faces."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[T.counting(f, V)]
    d = np.concatenate([f[:, 0] * V + f[:, 1], f[:, 1] * V + f[:, 2], f[:, 2] * V + f[:, 0]])
    und = np.minimum(d // V, d % V) * V + np.maximum(d // V, d % V)
    _, cnt = np.unique(und, return_counts=True)
    consistent = len(np.unique(d)) == len(d)                         # no directed edge twice
    return bool((cnt == 2).all()), bool(consistent), len(np.unique(f)) - len(cnt) + len(f)


def hops_apart(faces, V, sel):
    """True when no two of the vertices `sel` are within two hops of each other on the counting faces."""
    row_start, nbr, _ = T.adjacency(faces, V)
    rows = np.repeat(np.arange(V), np.diff(row_start))
    mark = np.zeros(V, np.int64)
    mark[sel] = 1
    np.add.at(mark, rows, mark[nbr].copy())                          # selected vertices in each closed neighbourhood
    return bool((mark <= 1).all())                                   # two within two hops share a closed neighbourhood
