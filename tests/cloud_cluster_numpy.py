"""Numpy statement of the radius count and the density clusters of a point cloud (DESIGN.md "Cloud clusters"; the
kernels are csrc/cloud_cluster.hip, the Python layer mast3r_slam/tsdf/cloud_cluster.py).  Everything about distances
is f64 on the f32 inputs in cloud_numpy.dist2_matrix's order; everything else is integer work.

THE DEFINITION.  d2(i, j) = (dx dx + dy dy) + dz dz of the f64 differences of the f32 coordinates, uncontracted.  It is
BIT-SYMMETRIC: a difference and its negation have the same square, so d2(i, j) and d2(j, i) are the same bits
(`pairs_within` asserts it on every diagonal block it forms).  "Within" means d2 <= eps2, eps2 an f64 taken as it is.
  count    count[q] = the valid points of the cloud within eps2 of query q; a point of the cloud counts itself and its
           duplicates (sklearn's and Open3D's convention); 0 for a query with a non-finite coordinate.
  core     core[i] = valid[i] and count[i] >= min_points.
  cluster  a connected component of the graph on the core points with an edge where d2 <= eps2; its root is its
           smallest point index.  A path through a point that is not core joins nothing.
  border   a valid point that is not core with a core point within eps2 belongs to the cluster of its ANCHOR, the core
           point smallest under the total order (d2, index).  Textbook DBSCAN gives a border point to whichever cluster
           reaches it first, which depends on the order of the visit; this rule does not, so the labels are a function
           of the cloud alone.
  noise    every other point, and every invalid point: label -1.
  labels   clusters are numbered 0..C-1 in ascending order of their root (as mesh_components numbers its components);
           sizes i32[C] counts core and border members.
The same bytes on every call and in every form of the scan.

Beside the statement stand the WRONG forms its tests must tell from it: a strict <, a fused sum
(cloud_numpy.dist2_fused), clusters joined through border points, a border point given to the first core met."""
import numpy as np

import cc_numpy
import cloud_numpy as C


def radius_count(queries, points, eps2, chunk=256):
    """count i32[n]; eps2: one f64, or a sequence - then i32[len(eps2), n] from one pass over the distances."""
    q, p = C.f32(queries), C.f32(points)
    many = np.ndim(eps2) > 0
    e = np.atleast_1d(np.asarray(eps2, np.float64))
    out = np.zeros((len(e), len(q)), np.int32)
    ok_p, ok_q = C.valid(p), C.valid(q)
    if len(q) and ok_p.any():
        for s in range(0, len(q), chunk):
            d = C.dist2_matrix(q[s:s + chunk], p)
            with np.errstate(all="ignore"):
                for k, ek in enumerate(e):
                    within = (d <= ek) & ok_p[None, :] & ok_q[s:s + chunk, None]
                    out[k, s:s + chunk] = within.sum(1)
    return out if many else out[0]


def pairs_within(points, eps2, rows=None, chunk=256):
    """(i, j, d2) of every ordered pair of VALID points with d2(i, j) <= eps2, the pair (i, i) included, i over `rows`
    (default: every point; entries outside [0, N) are skipped), sorted by (i, j).  Asserts the bit-symmetry of d2 on
    every block of rows against itself."""
    p = C.f32(points)
    N = len(p)
    ok = C.valid(p)
    rows = np.arange(N) if rows is None else np.unique(np.asarray(rows, np.int64))
    rows = rows[(rows >= 0) & (rows < N)]
    rows = rows[ok[rows]]
    I, J, D = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0)]
    for s in range(0, len(rows), chunk):
        r = rows[s:s + chunk]
        d = C.dist2_matrix(p[r], p)
        own = d[:, r]
        assert own.tobytes() == np.ascontiguousarray(own.T).tobytes()        # d2(i, j) and d2(j, i): the same bits
        with np.errstate(all="ignore"):
            a, b = np.nonzero((d <= eps2) & ok[None, :])
        I.append(r[a]), J.append(b), D.append(d[a, b])
    return np.concatenate(I), np.concatenate(J), np.concatenate(D)


def link(points, eps2, core, self=None, pairs=None):
    """The statement of mslam_cloud_cluster_link followed by the flatten, for the rows `self` (None: every point) ->
    (root i32[N], anchor i32[n], anchor_dist2 f64[n]).  root: parent after flatten - the smallest index of the tree of
    every point, where a core row i has united (i, j) for every core j < i within eps2; a point no row united stays its
    own root.  `pairs`: pairs_within(points, eps2) when the caller holds it."""
    p = C.f32(points)
    N = len(p)
    core = np.asarray(core).astype(bool).reshape(N)
    rows = np.arange(N, dtype=np.int64) if self is None else np.asarray(self, np.int64)
    inside = (rows >= 0) & (rows < N)
    i, j, d = pairs_within(p, eps2, rows) if pairs is None else pairs
    present = np.zeros(N, bool)
    present[rows[inside]] = True
    m = present[i] & core[i] & core[j] & (j < i)
    root = cc_numpy.labels(np.stack([i[m], j[m], j[m]], 1), N).astype(np.int32)
    # the best core point of every point that is not core, under (d2, index)
    best_j, best_d = np.full(N, -1, np.int32), np.full(N, np.inf)
    m = ~core[i] & core[j]
    bi, bj, bd = i[m], j[m], d[m]
    o = np.lexsort((bj, bd, bi))
    bi, bj, bd = bi[o], bj[o], bd[o]
    first = np.r_[True, bi[1:] != bi[:-1]] if len(bi) else np.zeros(0, bool)
    best_j[bi[first]], best_d[bi[first]] = bj[first], bd[first]
    ok = C.valid(p)
    v = np.where(inside, rows, 0)
    is_core = inside & core[v] & ok[v] if N else np.zeros(len(rows), bool)
    live = inside & ok[v] if N else np.zeros(len(rows), bool)
    anchor = np.where(is_core, v, np.where(live, best_j[v] if N else -1, -1)).astype(np.int32)
    dist2 = np.where(is_core, 0.0, np.where(live, best_d[v] if N else np.inf, np.inf))
    return root, anchor, dist2


def clusters(points, eps2, min_points, pairs=None):
    """dict: count i32[N], core bool[N], root i32[N], anchor i32[N], anchor_dist2 f64[N], labels i32[N], sizes i32[C],
    n_clusters, n_noise, n_core."""
    p = C.f32(points)
    N = len(p)
    pairs = pairs_within(p, eps2) if pairs is None else pairs
    count = np.bincount(pairs[0], minlength=N).astype(np.int32)
    core = C.valid(p) & (count >= int(min_points))
    root, anchor, dist2 = link(p, eps2, core, pairs=pairs)
    label_root = np.where(anchor >= 0, root[np.maximum(anchor, 0)] if N else -1, -1)
    is_root = core & (root == np.arange(N))
    dense = np.cumsum(is_root) - 1
    labels = np.where(label_root >= 0, dense[np.maximum(label_root, 0)] if N else -1, -1).astype(np.int32)
    n_c = int(is_root.sum())
    sizes = np.bincount(labels[labels >= 0], minlength=n_c).astype(np.int32)
    return dict(count=count, core=core, root=root, anchor=anchor, anchor_dist2=dist2, labels=labels, sizes=sizes,
                n_clusters=n_c, n_noise=int((labels < 0).sum()), n_core=int(core.sum()))


def keep_points(points, labels, sizes, min_cluster_points=0, keep_largest=None, keep_noise=False):
    """bool[N], filter_mesh's rule on the clusters: those with at least min_cluster_points members, then the
    keep_largest largest of them, ties to the lower label; keep_noise: the VALID points of label -1 stay too.  An
    invalid point is never kept."""
    keep = cc_numpy.keep_mask(sizes, min_cluster_points, keep_largest)
    labels = np.asarray(labels, np.int64)
    out = (labels >= 0) & np.r_[keep, False][labels]
    if keep_noise:
        out |= (labels < 0) & C.valid(points)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the wrong forms
# ----------------------------------------------------------------------------------------------------------------------
def clusters_textbook(points, eps2, min_points, visit=None):
    """THE WRONG FORM: textbook DBSCAN, the points visited in the order `visit` (default ascending): a border point goes
    to the first cluster that reaches it.  labels i32[N] in the order the clusters are found."""
    p = C.f32(points)
    N = len(p)
    i, j, _ = pairs_within(p, eps2)
    nb = [j[i == v] for v in range(N)]
    core = C.valid(p) & (np.bincount(i, minlength=N) >= min_points)
    labels = np.full(N, -1, np.int32)
    c = 0
    for v in (range(N) if visit is None else visit):
        if labels[v] >= 0 or not core[v]:
            continue
        labels[v] = c
        stack = [v]
        while stack:
            u = stack.pop()
            for w in nb[u]:
                if labels[w] < 0:
                    labels[w] = c
                    if core[w]:
                        stack.append(w)
        c += 1
    return labels


def clusters_through_border(points, eps2, min_points):
    """THE WRONG FORM: every point with a core point within eps2 joins the graph, so two core groups that share a
    border point become one cluster.  labels i32[N]."""
    p = C.f32(points)
    N = len(p)
    i, j, _ = pairs_within(p, eps2)
    core = C.valid(p) & (np.bincount(i, minlength=N) >= min_points)
    m = core[i] | core[j]
    root = cc_numpy.labels(np.stack([i[m], j[m], j[m]], 1), N)
    member = np.zeros(N, bool)
    member[i[m]] = True
    is_root = member & (root == np.arange(N))
    dense = np.cumsum(is_root) - 1
    return np.where(member, dense[root], -1).astype(np.int32)


def same_partition(a, b):
    """Two label vectors describe the same partition: the same noise set and a one-to-one renaming of the rest."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = np.unique(np.stack([a[a >= 0], b[b >= 0]], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))
