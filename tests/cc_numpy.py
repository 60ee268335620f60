"""Plain-numpy union-find over a triangle mesh: the test-side statement of mast3r_slam.tsdf.mesh_components and
filter_mesh (csrc/mesh_components.hip, DESIGN.md "Mesh components").  Same definitions: a component's label is its
smallest vertex index, dense ids number the components in the order of that index, a face belongs to the component of
its first vertex, a vertex no face uses is a component of its own with zero faces.  Everything is integer: the device
result must equal it exactly."""
import numpy as np


def labels(faces, num_vertices):
    """root i64[V]: the smallest vertex index of each vertex's component.  Union-find in rounds: compress every path to
    its root, hook the larger root of every edge whose ends still differ below the smaller one, until no edge differs."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    parent = np.arange(int(num_vertices), dtype=np.int64)
    a = np.concatenate([f[:, 0], f[:, 0]])
    b = np.concatenate([f[:, 1], f[:, 2]])
    while True:
        while True:                                   # parent[v] <= v: the jumps end at the roots
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
        ra, rb = parent[a], parent[b]
        m = ra != rb
        if not m.any():
            return parent
        np.minimum.at(parent, np.maximum(ra, rb)[m], np.minimum(ra, rb)[m])


def components(faces, num_vertices):
    """(vertex_component i32[V], face_component i32[F], component_faces i32[C], component_vertices i32[C])."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = int(num_vertices)
    root = labels(f, V)
    is_root = root == np.arange(V)
    dense = np.cumsum(is_root) - 1
    vc = dense[root]
    fc = vc[f[:, 0]]
    C = int(is_root.sum())
    return (vc.astype(np.int32), fc.astype(np.int32), np.bincount(fc, minlength=C).astype(np.int32),
            np.bincount(vc, minlength=C).astype(np.int32))


def keep_mask(component_faces, min_faces=0, keep_largest=None):
    """bool[C]: components with at least min_faces faces; keep_largest=k: then only the k with the most faces, ties to
    the lower component id."""
    cf = np.asarray(component_faces, np.int64)
    keep = cf >= int(min_faces)
    if keep_largest is not None:
        ids = np.nonzero(keep)[0]
        order = ids[np.argsort(-cf[ids], kind="stable")][:int(keep_largest)]
        keep = np.zeros(len(cf), bool)
        keep[order] = True
    return keep


def filter_mesh(mesh, min_faces=0, keep_largest=None):
    """mesh = (vertices, normals, faces[, colors]) numpy arrays -> the same arity: kept vertices in their original order,
    kept faces re-indexed."""
    V, N, F = mesh[:3]
    if int(min_faces) <= 0 and keep_largest is None:
        return tuple(mesh)
    vc, fc, cf, _ = components(F, len(V))
    keep = keep_mask(cf, min_faces, keep_largest)
    kv, kf = keep[vc], keep[fc]
    remap = np.cumsum(kv) - 1
    out_f = remap[np.asarray(F, np.int64)[kf]].astype(np.int32).reshape(-1, 3)
    return (V[kv], N[kv], out_f) + tuple(c[kv] for c in mesh[3:])


def strip(n_faces):
    """Triangle strip of n_faces faces over n_faces + 2 vertices: face i = (i, i + 1, i + 2)."""
    i = np.arange(int(n_faces), dtype=np.int32)
    return np.stack([i, i + 1, i + 2], 1)


# hand-built meshes: name -> (faces, V, root, component_faces, component_vertices), the answers written out by hand
HAND = {
    "empty": (np.zeros((0, 3), np.int32), 0, [], [], []),
    "one_triangle": (np.array([[0, 1, 2]], np.int32), 3, [0, 0, 0], [1], [3]),
    "shared_vertex": (np.array([[4, 3, 2], [2, 1, 0]], np.int32), 5, [0, 0, 0, 0, 0], [2], [5]),
    "disjoint": (np.array([[0, 2, 4], [5, 3, 1]], np.int32), 6, [0, 1, 0, 1, 0, 1], [1, 1], [3, 3]),
    "unreferenced": (np.array([[0, 1, 3], [4, 5, 6]], np.int32), 7, [0, 0, 2, 0, 4, 4, 4], [1, 0, 1], [3, 1, 3]),
}
