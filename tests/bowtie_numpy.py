"""Numpy statement of the bow-tie mode of mast3r_slam.tsdf.mesh_boundaries and fill_holes (bowties=True; DESIGN.md "Mesh
holes", csrc/mesh_holes.hip): boundary darts are paired across the hole they bound, so that the rims of holes that meet
in a vertex close.  Counting face, m(a, b), boundary dart, dart id, walk, centre, fan test, appended rows and layout are
holes_numpy's; only next and the naming of loops differ.  Dicts and plain loops throughout.

  fan(d)     d = u -> v on face f.  Within f, u -> v is followed by v -> w.  If v -> w is a boundary dart it is fan(d).
             Otherwise the rotation crosses to the one counting face that holds the directed edge w -> v and goes on with
             that face's edge after w -> v.  It stops with no successor when w -> v or v -> w does not occur exactly once
             among the directed edges of counting faces, or after more steps than directed edges leave v.  A successor
             claimed by more than one dart is nobody's.
  closed     the cycles of fan.  A dart on no cycle is OPEN.
  name       the position of a dart in the order of all boundary darts by (tail, head).  A closed walk starts at its dart
             of smallest name; rank counts from there.
  next       per closed walk and vertex v, the walk's darts with head v by ascending rank, d_0 .. d_{k-1}:
             next(d_m) = fan(d_{m-1 mod k}).
  loop       a cycle of next on which no vertex is a tail twice; any other cycle is OPEN, all of it.  A loop is named by
             its dart of smallest name, loops are numbered by ascending name, the walk starts at that dart.  loop_id is
             that dart's tail (the loop's smallest vertex), loop_head its head.
"""
import numpy as np

import holes_numpy as H

from holes_numpy import (HAND, boundary_darts, centre, counting, fan_products, folded_ring, grid,  # noqa: F401
                         hand_mesh, join, perimeter, ring, sphere_mesh, sphere_voxels, strip, with_attributes)


def directed_edges(faces, V):
    """{(a, b): [dart ids 3 face + corner of the counting faces' directed edges a -> b]}."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    slots = {}
    for fi in np.nonzero(counting(f, V))[0]:
        for c in range(3):
            slots.setdefault((int(f[fi, c]), int(f[fi, (c + 1) % 3])), []).append(3 * int(fi) + c)
    return slots


def fan_successors(faces, V, dart, head):
    """fan i64[B]: the index of the successor among the boundary darts, -1 = none."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    slots = directed_edges(f, V)
    leaving = {}
    for (a, _), s in slots.items():
        leaving[a] = leaving.get(a, 0) + len(s)
    index = {int(d): i for i, d in enumerate(dart)}
    B = len(dart)
    fan = np.full(B, -1, np.int64)
    for i in range(B):
        v, s, steps = int(head[i]), int(dart[i]), 0
        while True:
            fi, c = divmod(s, 3)
            c1 = (c + 1) % 3
            w = int(f[fi, (c1 + 1) % 3])                             # the edge after s in its face is v -> w
            steps += 1
            if steps > leaving.get(v, 0):
                break
            if 3 * fi + c1 in index:
                fan[i] = index[3 * fi + c1]
                break
            if len(slots.get((w, v), ())) != 1 or len(slots.get((v, w), ())) != 1:
                break
            s = slots[(w, v)][0]
    claims = {}
    for i in range(B):
        claims[int(fan[i])] = claims.get(int(fan[i]), 0) + 1
    for i in range(B):
        if fan[i] >= 0 and claims[int(fan[i])] > 1:
            fan[i] = -1
    return fan


def cycles_of(nxt):
    """The cycles of a partial injection, each as the list of its elements from an arbitrary one along nxt."""
    n = len(nxt)
    seen = np.zeros(n, bool)
    out = []
    for i in range(n):
        if seen[i]:
            continue
        path, j = [i], int(nxt[i])
        while j >= 0 and j != i and not seen[j]:
            path.append(j)
            j = int(nxt[j])
        seen[path] = True
        if j == i:
            out.append(path)
    return out


def _from_smallest(path, name):
    k = int(np.argmin(name[path]))
    return path[k:] + path[:k]


def names(tail, head):
    """name i64[B]: the rank of (tail, head) among all boundary darts."""
    order = sorted(range(len(tail)), key=lambda i: (int(tail[i]), int(head[i])))
    name = np.zeros(len(tail), np.int64)
    name[order] = np.arange(len(tail))
    return name


def trace(faces, V):
    """dict as holes_numpy.trace's, plus fan i64[B], name i64[B], closed: the closed walks of fan from their dart of
    smallest name, and loop_head i64[L]."""
    dart, tail, head = boundary_darts(faces, V)
    B = len(dart)
    fan = fan_successors(faces, V, dart, head)
    name = names(tail, head)
    closed = [_from_smallest(p, name) for p in cycles_of(fan)]
    nxt = np.full(B, -1, np.int64)
    for walk in closed:
        visits = {}
        for d in walk:                                               # ascending rank
            visits.setdefault(int(head[d]), []).append(d)
        for ds in visits.values():
            for m in range(len(ds)):
                nxt[ds[m]] = fan[ds[m - 1]]
    walks = []
    for path in cycles_of(nxt):
        tails = [int(tail[d]) for d in path]
        if len(set(tails)) == len(tails):
            walks.append(_from_smallest(path, name))
    walks.sort(key=lambda w: int(name[w[0]]))
    dart_loop = np.full(B, -1, np.int64)
    for l, w in enumerate(walks):
        dart_loop[w] = l
    return dict(dart=dart, tail=tail, head=head, fan=fan, name=name, closed=closed, nxt=nxt, walks=walks,
                dart_loop=dart_loop, loop_id=np.array([tail[w[0]] for w in walks], np.int64),
                loop_head=np.array([head[w[0]] for w in walks], np.int64))


def boundaries(faces, num_vertices, vertices=None):
    """The dict of mesh_boundaries(bowties=True), numpy arrays in its dtypes."""
    tr = trace(faces, num_vertices)
    i32 = lambda a: np.asarray(a, np.int64).astype(np.int32).reshape(-1)
    out = dict(loop_id=i32(tr["loop_id"]), loop_head=i32(tr["loop_head"]), loop_length=i32([len(w) for w in tr["walks"]]),
               dart=i32(tr["dart"]), dart_tail=i32(tr["tail"]), dart_head=i32(tr["head"]), dart_loop=i32(tr["dart_loop"]),
               n_boundary_edges=len(tr["dart"]), n_open=int((tr["dart_loop"] < 0).sum()))
    if vertices is not None:
        p = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
        with np.errstate(all="ignore"):
            out["loop_perimeter"] = np.array([perimeter(p, tr, w) for w in tr["walks"]], np.float64).reshape(-1)
    return out


def fill(mesh, max_edges, return_info=False):
    """holes_numpy.fill over this module's loops."""
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
                s = s + H._cross(y - x, c - x)
                new_f.append([tr["head"][i], tr["tail"][i], k])
            ln = np.sqrt(H._dot(s, s))
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
# meshes with holes that meet in a vertex, beside holes_numpy's
# ----------------------------------------------------------------------------------------------------------------------
def weld(mesh, keep, gone):
    """`mesh` with every use of vertex `gone` replaced by `keep`; `gone` stays as an unused row."""
    F = mesh[2].copy()
    F[F == gone] = keep
    return mesh[:2] + (F,) + mesh[3:]


def moved(mesh, offset):
    return ((mesh[0] + np.asarray(offset, np.float32)).astype(np.float32),) + mesh[1:]


def gapped_fan(n, gaps, colors=True, seed=0):
    """A fan of n faces (0, i, i + 1) around vertex 0 inside ring(n)'s annulus, without the faces of `gaps`: every gap
    is a three-edge hole, and all of them meet in vertex 0."""
    R = ring(n, colors, seed)
    V = np.concatenate([np.zeros((1, 3), np.float32), R[0]])
    i = np.array([g for g in range(n) if g not in set(gaps)])
    fan = np.stack([np.zeros_like(i), 1 + i, 1 + (i + 1) % n], 1)
    return with_attributes(V, np.concatenate([fan, R[2] + 1]), colors, seed)


def welded_rings(n, colors=True):
    """Two ring(n), the second moved aside, sharing the first one's inner vertex 0: two sheets that meet in a vertex."""
    both = join(ring(n, colors), moved(ring(n, colors, seed=1), [5.0, 0.0, 0.0]))
    return weld(both, 0, 2 * n)


def two_sheets(colors=True):
    """Two 2 x 2 grids with one corner in common and nothing else."""
    both = join(grid(2, 2, colors=colors), moved(grid(2, 2, colors=colors, seed=1), [2.0, 2.0, 1.0]))
    return weld(both, 8, 9)


def diagonal_squares(a, colors=True):
    """A grid with two holes of a x a cells that touch in a corner: one closed fan walk of 8 a darts, two loops of 4 a."""
    cells = [(1 + i, 1 + j) for i in range(a) for j in range(a)]
    return grid(2 * a + 2, 2 * a + 2, cells + [(a + i, a + j) for i, j in cells], colors=colors)


def hole_pairs(n, jitter=0.1, seed=5):
    """n x n blocks of 4 x 4 cells, each with the two diagonal holes of grid(4, 4, [(1, 1), (2, 2)])."""
    removed = [(4 * i + c, 4 * j + c) for i in range(n) for j in range(n) for c in (1, 2)]
    return grid(4 * n, 4 * n, removed, jitter=jitter, seed=seed)


def bad_winding():
    """grid(4, 4, [(1, 1), (2, 2)]) with the first two indices of face 5 swapped."""
    V, N, F, C = grid(4, 4, [(1, 1), (2, 2)])
    F = F.copy()
    F[5, [0, 1]] = F[5, [1, 0]]
    return V, N, F, C


def reordered(mesh, seed=0):
    """The same mesh with its faces permuted and the corners of every face rotated."""
    rng = np.random.default_rng(seed)
    F = mesh[2][rng.permutation(len(mesh[2]))]
    shift = rng.integers(0, 3, len(F))
    F = np.stack([F[np.arange(len(F)), (k + shift) % 3] for k in range(3)], 1).astype(np.int32)
    return mesh[:2] + (np.ascontiguousarray(F),) + mesh[3:]


def stack_cycles(tr):
    """An independent cut of the closed fan walks: walk each with a stack and pop a cycle whenever a vertex repeats.
    -> the set of cycles, each a frozenset of dart indices."""
    out = set()
    for walk in tr["closed"]:
        stack = []                                                   # (tail vertex, dart)
        for d in walk:
            stack.append((int(tr["tail"][d]), d))
            h = int(tr["head"][d])
            at = [k for k, (t, _) in enumerate(stack) if t == h]
            if at:
                out.add(frozenset(x for _, x in stack[at[-1]:]))
                del stack[at[-1]:]
        assert not stack
    return out
