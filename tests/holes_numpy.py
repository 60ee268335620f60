"""Numpy statement of mast3r_slam.tsdf.mesh_boundaries and fill_holes (csrc/mesh_holes.hip, DESIGN.md "Mesh holes"): the
boundary loops of a welded triangle mesh, and the closing of the small, well-behaved ones with a centroid fan.  Every
sum is sequential in walk order and every operation is rounded on its own, so the kernels' output equals this one bit
for bit.  The loops are walked one dart at a time with plain Python loops.

  counting   a face counts when its three indices lie in [0, V) and are pairwise different (as in smooth_numpy).
  m(a, b)    the number of counting faces on the undirected edge {a, b}.
  dart       a directed edge a -> b of a counting face, in the face's winding, with m(a, b) = 1: a boundary dart.  a is
             its tail, b its head, 3 face + corner its id (corner 0: f0 -> f1, 1: f1 -> f2, 2: f2 -> f0).  B darts.
  simple     a vertex that exactly one boundary dart leaves and exactly one enters.
  next(d)    the boundary dart whose tail is head(d) when head(d) is simple, else none: a partial injection, whose
             components are cycles or paths.
  loop       a cycle of next; its id is its smallest vertex; loops are numbered by ascending id.  Every other boundary
             dart is OPEN (bow-tie rims, chains into a non-simple vertex): counted, flagged with loop -1, never filled.
  walk       starts at the dart whose tail is the loop id and follows next.
  perimeter  0.0 + l0 + l1 + ... in walk order, l = sqrt((dx dx + dy dy) + dz dz) of head - tail in f64.
  centre     c64 = (0.0 + p[t0] + p[t1] + ...) / n over the tails in walk order, in f64; c = c64 rounded to f32 once.
  fan face   of a dart a -> b: (b, a, centre), the winding of the face across the edge.
  fillable   3 <= n <= max_edges and, for every dart, dot(cross(p[a] - p[b], c64 - p[b]), cross(q1 - q0, q2 - q0)) > 0,
             q the corners of the dart's own face in its order, cross(u, v) = (u1 v2 - u2 v1, u2 v0 - u0 v2,
             u0 v1 - u1 v0), dot(u, v) = (u0 v0 + u1 v1) + u2 v2, in f64, each operation rounded on its own.
  appended   per filled loop one vertex and n faces.  Position c.  Normal: s = 0.0 + the fan faces' (y - x) x (z - x)
             (x, y, z = head, tail, centre: the face's own order) on the f32 positions in f64, in walk order;
             l = sqrt((sx sx + sy sy) + sz sz); s / l when 0 < l < inf, else zero.  Colour: (0.0 + col[t0] + ...) / n in
             f64, rounded once.
  layout     input rows first (their bits), then the new vertices by ascending loop id, then the new faces by loop id and
             walk order.  Independent of the face order; dependent on the vertex numbering through the sum order only.
"""
import numpy as np

import smooth_numpy as T

counting = T.counting


def boundary_darts(faces, V):
    """(dart i64[B] ascending, tail i64[B], head i64[B])."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = np.repeat(counting(f, V), 3)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)                # row-major: position = 3 face + corner
    key = np.minimum(a, b) * max(V, 1) + np.maximum(a, b)
    _, inv, cnt = np.unique(key[ok], return_inverse=True, return_counts=True)
    single = np.zeros(len(a), bool)
    single[np.nonzero(ok)[0]] = cnt[inv.reshape(-1)] == 1
    d = np.nonzero(single)[0]
    return d.astype(np.int64), a[d], b[d]


def trace(faces, V):
    """The loops, by plain walking -> dict with dart, tail, head i64[B]; nxt (index into the darts, -1 = none) i64[B];
    loop_id i64[L] ascending; walks: per loop the dart indices in walk order; dart_loop i64[B] (-1 = open)."""
    dart, tail, head = boundary_darts(faces, V)
    B = len(dart)
    leaves, enters, by_tail = {}, {}, {}
    for i in range(B):
        leaves[int(tail[i])] = leaves.get(int(tail[i]), 0) + 1
        enters[int(head[i])] = enters.get(int(head[i]), 0) + 1
        by_tail[int(tail[i])] = i
    nxt = np.full(B, -1, np.int64)
    for i in range(B):
        h = int(head[i])
        if leaves.get(h, 0) == 1 and enters.get(h, 0) == 1:
            nxt[i] = by_tail[h]
    state = np.zeros(B, np.int64)                                    # 0 unseen, 1 on a cycle, 2 open
    cycles = []
    for i in range(B):
        if state[i]:
            continue
        path, j = [i], int(nxt[i])
        while j >= 0 and j != i:                                     # next is injective: back to i, or off the end
            path.append(j)
            j = int(nxt[j])
        state[path] = 1 if j == i else 2
        if j == i:
            cycles.append(path)
    walks = []
    for path in cycles:
        k = int(np.argmin(tail[path]))
        walks.append(path[k:] + path[:k])
    walks.sort(key=lambda w: int(tail[w[0]]))
    dart_loop = np.full(B, -1, np.int64)
    for l, w in enumerate(walks):
        dart_loop[w] = l
    return dict(dart=dart, tail=tail, head=head, nxt=nxt, walks=walks, dart_loop=dart_loop,
                loop_id=np.array([tail[w[0]] for w in walks], np.int64))


def _cross(u, v):
    return np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def perimeter(p, tr, walk):
    s = np.float64(0.0)
    for i in walk:
        d = p[tr["head"][i]] - p[tr["tail"][i]]
        s = s + np.sqrt(_dot(d, d))
    return s


def centre(p, tr, walk):
    s = np.zeros(3)
    for i in walk:
        s = s + p[tr["tail"][i]]
    return s / np.float64(len(walk))


def fan_products(p, faces, tr, walk):
    """The fillable test's product of every dart of the loop, in walk order."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    c64 = centre(p, tr, walk)
    out = []
    with np.errstate(all="ignore"):
        for i in walk:
            a, b = p[tr["tail"][i]], p[tr["head"][i]]
            q = p[f[tr["dart"][i] // 3]]
            out.append(_dot(_cross(a - b, c64 - b), _cross(q[1] - q[0], q[2] - q[0])))
    return np.array(out)


def boundaries(faces, num_vertices, vertices=None):
    """The dict of mesh_boundaries, numpy arrays in its dtypes."""
    tr = trace(faces, num_vertices)
    i32 = lambda a: np.asarray(a, np.int64).astype(np.int32).reshape(-1)
    out = dict(loop_id=i32(tr["loop_id"]), loop_length=i32([len(w) for w in tr["walks"]]), dart=i32(tr["dart"]),
               dart_tail=i32(tr["tail"]), dart_head=i32(tr["head"]), dart_loop=i32(tr["dart_loop"]),
               n_boundary_edges=len(tr["dart"]), n_open=int((tr["dart_loop"] < 0).sum()))
    if vertices is not None:
        p = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
        with np.errstate(all="ignore"):
            out["loop_perimeter"] = np.array([perimeter(p, tr, w) for w in tr["walks"]], np.float64).reshape(-1)
    return out


def fill(mesh, max_edges, return_info=False):
    """mesh = (vertices f32[V,3], normals f32[V,3], faces i32[F,3][, colors f32[V,3]]) -> the same arity (+ the dict of
    boundaries() with loop_filled bool[L])."""
    if max_edges is None or max_edges <= 0:
        return tuple(mesh)
    V32, N32, F = mesh[:3]
    col = mesh[3] if len(mesh) == 4 else None
    nv = len(V32)
    p = np.asarray(V32, np.float32).astype(np.float64).reshape(-1, 3)
    tr = trace(F, nv)
    filled, new_v, new_n, new_c, new_f = [], [], [], [], []
    with np.errstate(all="ignore"):
        for w in tr["walks"]:
            n = len(w)
            ok = 3 <= n <= max_edges and bool((fan_products(p, F, tr, w) > 0).all())
            filled.append(ok)
            if not ok:
                continue
            k = nv + len(new_v)
            c32 = centre(p, tr, w).astype(np.float32)
            c = c32.astype(np.float64)
            s = np.zeros(3)
            for i in w:
                x, y = p[tr["head"][i]], p[tr["tail"][i]]
                s = s + _cross(y - x, c - x)
                new_f.append([tr["head"][i], tr["tail"][i], k])
            ln = np.sqrt(_dot(s, s))
            new_v.append(c32)
            new_n.append((s / ln).astype(np.float32) if 0.0 < ln < np.inf else np.zeros(3, np.float32))
            if col is not None:
                cs = np.zeros(3)
                for i in w:
                    cs = cs + np.asarray(col, np.float32)[tr["tail"][i]].astype(np.float64)
                new_c.append((cs / np.float64(n)).astype(np.float32))
    cat = lambda a, b, dt: np.concatenate([np.asarray(a, dt).reshape(-1, 3), np.asarray(b, dt).reshape(-1, 3)])
    out = (cat(V32, new_v, np.float32), cat(N32, new_n, np.float32), cat(F, new_f, np.int32))
    if col is not None:
        out += (cat(col, new_c, np.float32),)
    if return_info:
        info = boundaries(F, nv, V32)
        info["loop_filled"] = np.array(filled, bool).reshape(-1)
        out += (info,)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# meshes.  The hand meshes are smooth_numpy.HAND's; what each is about stands in tests/test_mesh_holes_cpu.py.
# ----------------------------------------------------------------------------------------------------------------------
HAND = ("tetrahedron", "triangle", "two_triangles", "bow_tie", "three_on_an_edge", "duplicated_face", "repeated_index")
hand_mesh = T.hand_mesh


def with_attributes(V, F, colors=True, seed=0):
    """(V f32, unit normals f32, F i32[, colours f32]) with random attributes."""
    V = np.asarray(V, np.float32).reshape(-1, 3)
    rng = np.random.default_rng(seed + len(V))
    N = rng.normal(size=V.shape)
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)
    F = np.asarray(F, np.int32).reshape(-1, 3)
    return (V, N, F) + ((rng.uniform(0, 1, V.shape).astype(np.float32),) if colors else ())


def grid(nx, ny, removed=(), jitter=0.0, seed=0, colors=True):
    """A planar grid of nx x ny cells in z = 0 (vertex (i, j) = i (ny + 1) + j at (i, j, 0)), two faces per cell, wound
    counter-clockwise seen from +z; the cells of `removed` = [(i, j), ...] are left out.  `jitter`: uniform noise of that
    size on every coordinate."""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    V = np.stack([i, j, np.zeros_like(i)], -1).reshape(-1, 3).astype(np.float64)
    if jitter:
        V = V + np.random.default_rng(seed).uniform(-jitter, jitter, V.shape)
    gone = set(map(tuple, removed))
    F = []
    for a in range(nx):
        for b in range(ny):
            if (a, b) in gone:
                continue
            v = a * (ny + 1) + b
            F += [[v, v + ny + 1, v + ny + 2], [v, v + ny + 2, v + 1]]
    return with_attributes(V, F, colors, seed)


def ring(n, colors=True, seed=0):
    """A planar annulus strip: n inner vertices (0 .. n-1, radius 1) and n outer ones (radius 2), 2 n faces wound
    counter-clockwise seen from +z.  The inner loop (id 0, n edges) is a hole, the outer one (id n) the rim."""
    t = 2.0 * np.pi * np.arange(n) / n
    rng = np.random.default_rng(seed + n)
    z = 0.05 * rng.uniform(-1, 1, 2 * n)
    V = np.concatenate([np.stack([np.cos(t), np.sin(t)], 1), 2.0 * np.stack([np.cos(t), np.sin(t)], 1)])
    V = np.concatenate([V, z[:, None]], 1)
    i = np.arange(n)
    k = (i + 1) % n
    F = np.concatenate([np.stack([i, n + i, n + k], 1), np.stack([i, n + k, k], 1)])
    return with_attributes(V, F, colors, seed)


def strip(B, colors=True, seed=0):
    """A triangle strip with exactly B boundary darts (B >= 3): B - 2 faces over B vertices, one rim loop of B edges."""
    v = np.arange(B)
    V = np.stack([v // 2, v % 2, np.zeros_like(v)], 1).astype(np.float64)
    F = [[k, k + 1, k + 2] if k % 2 == 0 else [k + 1, k, k + 2] for k in range(B - 2)]
    return with_attributes(V, F, colors, seed)


def sphere_voxels(seed, n_removed=40):
    """The sphere fixture: (keys, tsdf, weight) with the weight of n_removed voxels set to 0."""
    import mc_numpy as M

    keys, t, w = M.sample_sdf(M.sphere_sdf([0.3, -0.2, 0.1], 0.31), [-0.2, -0.7, -0.4], [0.8, 0.3, 0.6], 0.03, 0.09)
    w = w.copy()
    w[np.random.default_rng(seed).choice(len(w), n_removed, replace=False)] = 0.0
    return keys, t, w


def sphere_mesh(seed, n_removed=40):
    import mc_numpy as M

    return M.extract(*sphere_voxels(seed, n_removed), 0.03, 0.5)


def join(*meshes):
    """Disjoint union: the vertices of each mesh after those of the ones before it."""
    off, parts = 0, []
    for m in meshes:
        parts.append(m[:2] + (m[2] + np.int32(off),) + m[3:])
        off += len(m[0])
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(len(parts[0])))


def folded_ring(n=8, r=-0.5):
    """ring(n) with inner vertex 1 pulled through the centre to radius r on its ray: exactly one dart of the inner loop
    then has a fan face that turns against its own face (tests/test_mesh_holes_cpu.py asserts the count)."""
    V, N, F, C = ring(n)
    V = V.copy()
    t = 2.0 * np.pi / n
    V[1, :2] = np.float32(r) * np.array([np.cos(t), np.sin(t)], np.float32)
    return V, N, F, C
