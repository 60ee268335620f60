"""Pure-numpy marching cubes over a sparse voxel set: the test-side statement of TSDFVolume.extract_mesh
(csrc/tsdf_mesh.hip, DESIGN.md "Mesh extraction").  Same case tables (tools/gen_mc_tables.py), same sample points, same
validity / inside rules, same vertex and face order, same f64 formulae - so the device result must match it to within
f32 rounding of identical f64 values.  Also: analytic SDF sampling and mesh checks (manifold, Euler, winding)."""
import os
import sys

import numpy as np

_TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)

import gen_mc_tables as _g  # noqa: E402

_BIAS = 1 << 20
EDGE_TABLE, TRI_TABLE, TRI_COUNT = _g.build_tables()
_CORNER_OFF = np.array([_g.corner_pos(c) for c in range(8)], np.int64)
_EDGE_CORNER = np.array(_g.EDGE_CORNER, np.int64)
_EDGE_AXIS = np.array(_g.EDGE_AXIS, np.int64)
_TRI = np.full((256, 3 * 5), -1, np.int64)
for _c in range(256):
    _f = [e for t in TRI_TABLE[_c] for e in t]
    _TRI[_c, :len(_f)] = _f
_NTRI = np.array(TRI_COUNT, np.int64)
_EYE = np.eye(3, dtype=np.int64)


def pack(keys):
    k = np.asarray(keys, np.int64) + _BIAS
    return (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]


def extract(keys, tsdf, weight, voxel_size, min_weight, level=0.0):
    """keys i64[n,3] (unique), tsdf f64[n], weight f64[n] -> (vertices f32[V,3], normals f32[V,3], faces i32[F,3])."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    tsdf = np.asarray(tsdf, np.float64).reshape(-1)
    weight = np.asarray(weight, np.float64).reshape(-1)
    ok = weight >= min_weight
    keys, val = keys[ok], tsdf[ok]
    pk = pack(keys)
    o = np.argsort(pk, kind="stable")
    keys, val, pk = keys[o], val[o], pk[o]
    n = len(pk)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    if n == 0:
        return empty

    def find(k):
        """sorted position of each key of k (m,3), -1 when absent"""
        q = pack(k)
        p = np.minimum(np.searchsorted(pk, q), n - 1)
        return np.where(pk[p] == q, p, -1)

    vs = float(voxel_size)
    lv = float(level)
    # cubes: corners k + {0,1}^3, all valid
    cidx = np.stack([find(keys + _CORNER_OFF[c]) for c in range(8)], 1)          # [n,8]
    full = (cidx >= 0).all(1)
    case = np.zeros(n, np.int64)
    for c in range(8):
        case |= np.where(full, (val[np.maximum(cidx[:, c], 0)] < lv).astype(np.int64) << c, 0)
    ntri = np.where(full, _NTRI[case], 0)
    # referenced edges: (owner position, axis)
    ref = np.zeros((n, 3), bool)
    cubes = np.nonzero(ntri)[0]
    for c in cubes:
        for e in set(_TRI[case[c], :3 * ntri[c]].tolist()):
            ref[cidx[c, _EDGE_CORNER[e]], _EDGE_AXIS[e]] = True
    vid = np.cumsum(ref.reshape(-1)).reshape(n, 3) - 1
    own, ax = np.nonzero(ref)                                                     # row-major: owner, then axis
    V = len(own)
    if V == 0:
        return empty
    ka = keys[own]
    kb = ka + _EYE[ax]
    va = val[own]
    vb = val[find(kb)]
    t = (lv - va) / (vb - va)
    a = (ka.astype(np.float64) + 0.5) * vs
    b = (kb.astype(np.float64) + 0.5) * vs
    p = a + t[:, None] * (b - a)

    def grad(k, v):
        g = np.zeros((len(k), 3))
        for d in range(3):
            ip, im = find(k + _EYE[d]), find(k - _EYE[d])
            vp, vm = val[np.maximum(ip, 0)], val[np.maximum(im, 0)]
            g[:, d] = np.where((ip >= 0) & (im >= 0), (vp - vm) / (2.0 * vs),
                               np.where(ip >= 0, (vp - v) / vs, np.where(im >= 0, (v - vm) / vs, 0.0)))
        return g

    ga, gb = grad(ka, va), grad(kb, vb)
    g = ga + t[:, None] * (gb - ga)
    ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    nrm = np.where(ln[:, None] > 0, g / np.where(ln > 0, ln, 1.0)[:, None], 0.0)
    faces = []
    for c in cubes:
        for j in range(ntri[c]):
            tri = []
            for e in _TRI[case[c], 3 * j:3 * j + 3]:
                tri.append(vid[cidx[c, _EDGE_CORNER[e]], _EDGE_AXIS[e]])
            faces.append(tri)
    return p.astype(np.float32), nrm.astype(np.float32), np.array(faces, np.int32).reshape(-1, 3)


# ----------------------------------------------------------------------------------------------------------------------
# analytic inputs and mesh checks
# ----------------------------------------------------------------------------------------------------------------------
def sample_sdf(sdf, lo, hi, voxel_size, band):
    """Voxels of the cells [k vs, (k+1) vs) whose centre lies within `band` of the surface, with the SDF value there
    (weight 1): keys i64[n,3] (lexicographic), tsdf f64[n], weight f64[n]."""
    lo_k = np.floor(np.asarray(lo) / voxel_size).astype(np.int64) - 1
    hi_k = np.ceil(np.asarray(hi) / voxel_size).astype(np.int64) + 1
    ax = [np.arange(lo_k[d], hi_k[d] + 1) for d in range(3)]
    K = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    P = (K.astype(np.float64) + 0.5) * voxel_size
    v = sdf(P)
    m = np.abs(v) <= band
    return K[m], v[m], np.ones(int(m.sum()))


def sphere_sdf(c, r):
    c = np.asarray(c, np.float64)
    return lambda P: np.linalg.norm(P - c, axis=1) - r


def torus_sdf(c, R, r):
    c = np.asarray(c, np.float64)

    def f(P):
        q = P - c
        return np.sqrt((np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2) - R) ** 2 + q[:, 2] ** 2) - r
    return f


def edge_use(faces):
    """{undirected edge: number of faces}, and whether every directed edge occurs at most once (consistent winding)."""
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und = np.sort(d, 1)
    _, cnt = np.unique(und, axis=0, return_counts=True)
    _, dcnt = np.unique(d, axis=0, return_counts=True)
    return cnt, bool((dcnt == 1).all())


def euler(vertices, faces):
    f = np.asarray(faces, np.int64)
    d = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    E = len(np.unique(d, axis=0))
    return len(vertices) - E + len(f)


def face_normals(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


def parse_ply(path):
    """Minimal binary little-endian PLY reader for what evaluate.save_mesh writes -> (header lines, vertex record array,
    faces i32[F,3])."""
    _types = {"float": "<f4", "double": "<f8", "uchar": "u1", "int": "<i4", "uint": "<u4", "short": "<i2",
              "ushort": "<u2", "char": "i1"}
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").strip().split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elems, cur = [], None
    for ln in lines[2:-1]:
        tok = ln.split()
        if tok[0] == "element":
            cur = [tok[1], int(tok[2]), []]
            elems.append(cur)
        elif tok[0] == "property":
            cur[2].append(tok[1:])
    off = end
    vert, faces = None, None
    for name, count, props in elems:
        if name == "vertex":
            dt = np.dtype([(p[1], _types[p[0]]) for p in props])
            vert = np.frombuffer(data, dt, count, off)
            off += dt.itemsize * count
        elif name == "face":
            assert props == [["list", "uchar", "int", "vertex_indices"]]
            dt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
            rec = np.frombuffer(data, dt, count, off)
            assert (rec["n"] == 3).all()
            faces = rec["i"].astype(np.int32).reshape(-1, 3)
            off += dt.itemsize * count
    assert off == len(data), "trailing bytes after the last element"
    return lines, vert, faces
