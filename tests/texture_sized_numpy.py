"""Numpy statement of the sized atlas of the mesh textures (DESIGN.md "Mesh textures: sized atlas"; the kernels are in
csrc/mesh_texture.hip, the Python is mast3r_slam/tsdf/mesh_texture.py): the classes, the resolution of a face, the
stable rank by class, the band packing, owner / face_cell, the bake and the shade from a sized atlas.  Everything inside
a cell is texture_numpy's, with the face's own R in the place of the atlas's: the view rule, the bilinear sample, the
edge functions and the ray cast are imported from there and from raycast_numpy, unchanged.  Everything is f64 on the f32
inputs, and the operation order written here is the kernels'."""
import math

import numpy as np

import raycast_numpy as RC
import texture_numpy as TX

CLASSES = (4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256)
NC = len(CLASSES)
_R = np.array(CLASSES, np.int64)


def floor_and_cap(texels=8, max_texels=256):
    """(floor, cap): the indices of the smallest class >= texels and of the largest class <= max_texels."""
    if int(texels) != texels or texels < 4:
        raise ValueError(f"texels must be an integer >= 4, got {texels!r}")
    if texels > CLASSES[-1]:
        raise ValueError(f"texels must not exceed the largest class {CLASSES[-1]}, got {texels!r}")
    lo = int(np.flatnonzero(_R >= texels)[0])
    le = np.flatnonzero(_R <= max_texels)
    if len(le) == 0 or int(le[-1]) < lo:
        raise ValueError(f"max_texels {max_texels!r} is below the floor class {CLASSES[lo]}")
    return lo, int(le[-1])


def edge_lengths(vertices, faces):
    """(e f64[F,3] of the edges ab, bc, ca, in_range bool[F]): e = sqrt((dx dx + dy dy) + dz dz) of the f32 corners in
    f64; zeros for a face with an index outside [0, V)."""
    a, b, c, ok = TX._corners(vertices, faces)
    out = []
    with np.errstate(all="ignore"):
        for p, q in ((a, b), (b, c), (c, a)):
            d = q - p
            out.append(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))
    return np.stack(out, 1).reshape(-1, 3), ok


def need_of(density, L):
    """need = ceil(density L + 3.5) in f64 (may be inf)."""
    with np.errstate(all="ignore"):
        return np.ceil(np.float64(density) * np.asarray(L, np.float64) + 3.5)


def class_of_need(need, lo, cap):
    """(cls i32, clamped bool) of `need` f64: the smallest class >= max(need, floor), capped at class `cap`; clamped
    where need exceeds the cap's R."""
    need = np.asarray(need, np.float64)
    cls = np.searchsorted(_R.astype(np.float64), need, side="left")        # the first class with R >= need; NC: none
    cls = np.minimum(np.maximum(cls, lo), cap)
    return cls.astype(np.int32), need > float(CLASSES[cap])


def face_classes(vertices, faces, density, texels=8, max_texels=256):
    """(cls i32[F] - the index into CLASSES of every face's R_f -, clamped bool[F]).  L = max(max(e_ab, e_bc), e_ca); a
    face with an index out of range or an edge that is not finite gets the floor class and is not clamped."""
    if not (density > 0.0 and math.isfinite(density)):
        raise ValueError(f"density must be a positive number, got {density!r}")
    lo, cap = floor_and_cap(texels, max_texels)
    e, ok = edge_lengths(vertices, faces)
    ok = ok & np.isfinite(e).all(1)
    L = np.maximum(np.maximum(e[:, 0], e[:, 1]), e[:, 2]) if len(e) else np.zeros(0)
    cls, clamped = class_of_need(need_of(density, np.where(ok, L, 0.0)), lo, cap)
    return np.where(ok, cls, lo).astype(np.int32), clamped & ok


def stable_rank(cls):
    """(rank i32[F], order i32[F], counts i32[NC]): rank = the number of faces with a smaller index in the same class;
    order lists the faces class by class, largest R first, each class by rising face index."""
    cls = np.asarray(cls, np.int32).reshape(-1)
    counts = np.bincount(cls, minlength=NC).astype(np.int32)
    rank = np.zeros(len(cls), np.int32)
    order = []
    for c in range(NC - 1, -1, -1):
        idx = np.flatnonzero(cls == c)
        rank[idx] = np.arange(len(idx), dtype=np.int32)
        order.append(idx)
    return rank, np.concatenate(order).astype(np.int32) if len(cls) else np.zeros(0, np.int32), counts


def sized_layout(counts):
    """(H, W, bands i32[NC,6]) of the per-class face counts: a row of `bands` is (R, cols, rows, y0, base, count) of the
    class, base its first position in `order`.  cells = (count + 1) >> 1, A = sum cells (R + 1) R, W = max(ceil(sqrt(A)),
    R_top + 1), bands from the largest class in use down, cols = W // (R + 1), rows = ceil(cells / cols)."""
    counts = [int(c) for c in counts]
    if len(counts) != NC or min(counts) < 0:
        raise ValueError(f"sized_layout takes {NC} non-negative counts, got {counts}")
    cells = [(c + 1) >> 1 for c in counts]
    A = sum(q * (R + 1) * R for q, R in zip(cells, CLASSES))
    used = [R for R, c in zip(CLASSES, counts) if c]
    W = 0
    if used:
        W = math.isqrt(A)
        W += 1 if W * W < A else 0
        W = max(W, used[-1] + 1)
    bands = np.zeros((NC, 6), np.int64)
    y0 = base = 0
    for c in range(NC - 1, -1, -1):
        R = CLASSES[c]
        cols = W // (R + 1)
        rows = -(-cells[c] // cols) if cells[c] else 0
        bands[c] = (R, cols, rows, y0, base, counts[c])
        y0 += rows * R
        base += counts[c]
    H = y0
    if H * W >= 1 << 31 or 3 * base >= 1 << 31:
        raise ValueError(f"an atlas of {H}x{W} texels / {base} faces is outside the int32 index range")
    return H, W, bands.astype(np.int32)


def face_cells(cls, rank, bands):
    """face_cell i32[F,4] = (x0, y0, R_f, half): face f is half k & 1 of cell q = k >> 1 of its class's band, k its
    rank; the cell lies at ((q % cols)(R + 1), y0_c + (q // cols) R)."""
    cls, k = np.asarray(cls, np.int64), np.asarray(rank, np.int64)
    b = np.asarray(bands, np.int64)[cls].reshape(-1, 6)
    R, cols, yb = b[:, 0], np.maximum(b[:, 1], 1), b[:, 3]
    q = k >> 1
    return np.stack([(q % cols) * (R + 1), yb + (q // cols) * R, R, k & 1], 1).astype(np.int32).reshape(-1, 4)


def texel_owner(H, W, bands, order):
    """owner i32[H,W]: the band of a texel from its row, the cell from (x // (R + 1), (y - y0) // R), the half from
    i + j > R - 1, the face order[base + 2 q + half]; -1 right of the band's last column, in a cell past the band's last
    and in the absent half of an odd class's last cell."""
    owner = np.full((H, W), -1, np.int32)
    order = np.asarray(order, np.int64)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for R, cols, rows, y0, base, count in np.asarray(bands, np.int64):
        if count == 0:
            continue
        inb = (y >= y0) & (y < y0 + rows * R)
        cx, cy = x // (R + 1), (y - y0) // R
        i, j = x - cx * (R + 1), (y - y0) - cy * R
        k = 2 * (cy * cols + cx) + (i + j > R - 1)
        ok = inb & (cx < cols) & (k < count)
        owner[ok] = order[base + k[ok]]
    return owner


def texel_local(owner, face_cell):
    """(li, lj, R i64[H,W]) of every texel from its owner's face_cell alone, as the sized kernels recover them: i = x - x0,
    j = y - y0, mirrored (R - i, R - 1 - j) for half 1.  A texel without an owner has (0, 0, 4)."""
    H, W = owner.shape
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    own = owner >= 0
    fc = np.asarray(face_cell, np.int64).reshape(-1, 4)
    cell = fc[np.where(own, owner, 0)] if len(fc) else np.zeros((H, W, 4), np.int64)
    R = np.where(own, cell[..., 2], 4)
    i, j = x - cell[..., 0], y - cell[..., 1]
    half = cell[..., 3] == 1
    li, lj = np.where(half, R - i, i), np.where(half, R - 1 - j, j)
    return np.where(own, li, 0), np.where(own, lj, 0), R


def layout(vertices, faces, density, texels=8, max_texels=256):
    """dict(cls, clamped, rank, order, counts, H, W, bands, face_cell, owner) of a mesh."""
    cls, clamped = face_classes(vertices, faces, density, texels, max_texels)
    rank, order, counts = stable_rank(cls)
    H, W, bands = sized_layout(counts)
    fc = face_cells(cls, rank, bands)
    return dict(cls=cls, clamped=clamped, rank=rank, order=order, counts=counts, H=H, W=W, bands=bands, face_cell=fc,
                owner=texel_owner(H, W, bands, order), face_texels=_R[cls].astype(np.int32))


def atlas_xy(face_cell, f, beta, gamma):
    """texture_numpy.atlas_xy with the face's own cell: local (m + beta s, m + gamma s), s = R_f - 3.5, mirrored for half
    1, plus the cell's origin -> (x, y, cell i64[n,4])."""
    cell = np.asarray(face_cell, np.int64).reshape(-1, 4)[np.asarray(f, np.int64)]
    R = cell[:, 2]
    s = TX.span(R)
    lx, ly = TX.M + beta * s, TX.M + gamma * s
    half = cell[:, 3] == 1
    lx, ly = np.where(half, R - lx, lx), np.where(half, (R - 1) - ly, ly)
    return cell[:, 0] + lx, cell[:, 1] + ly, cell


def face_uv(face_cell):
    """f64[F,3,2]: the atlas coordinates of the corners a, b, c of every face."""
    F = len(np.reshape(face_cell, (-1, 4)))
    out = np.zeros((F, 3, 2))
    for k, (b, g) in enumerate(((0.0, 0.0), (1.0, 0.0), (0.0, 1.0))):
        if F:
            out[:, k, 0], out[:, k, 1] = atlas_xy(face_cell, np.arange(F), np.full(F, b), np.full(F, g))[:2]
    return out


def texel_points(vertices, faces, lay):
    """texture_numpy.texel_points on the sized layout `lay`: the same dict, per texel, flattened row-major."""
    F = len(np.reshape(faces, (-1, 3)))
    owner = lay["owner"].reshape(-1)
    li, lj, R = (t.reshape(-1) for t in texel_local(lay["owner"], lay["face_cell"]))
    a, b, c, in_range = TX._corners(vertices, faces)
    g = np.where(owner >= 0, owner, 0)
    ok = (owner >= 0) & (in_range[g] if F else False)
    al, be, ga = TX.texel_bary(li, lj, R)
    if F == 0:
        z = np.zeros((len(owner), 3))
        return dict(owner=owner, ok=ok, alpha=al, beta=be, gamma=ga, p=z, n=z)
    A, B, C = a[g], b[g], c[g]
    with np.errstate(all="ignore"):                                   # a vertex that is not finite
        p = (al[:, None] * A + be[:, None] * B) + ga[:, None] * C
        e1, e2 = B - A, C - A
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        n = n /np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]
    return dict(owner=owner, ok=ok, alpha=al, beta=be, gamma=ga, p=p, n=n)


def bake(vertices, faces, images, poses, K, density, texels=8, max_texels=256, near=0.05, far=10.0, tol=0.01,
         cos_min=0.1, fallback=None, default_color=0.5, trace=False):
    """texture_numpy.bake on the sized atlas -> dict(atlas, views, owner, sums, face_cell, order, ...layout) and, with
    `trace`, per view the lists dir, r, cos, uv, t64 and sums_after."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    images = np.asarray(images, np.float32)
    poses = np.asarray(poses, np.float32).reshape(-1, 8)
    F = len(faces)
    lay = layout(vertices, faces, density, texels, max_texels)
    H, W = lay["H"], lay["W"]
    if len(poses) and (images.ndim != 4 or images.shape[1] < 2 or images.shape[2] < 2):
        raise ValueError("images must be (K,h,w,3) with h, w >= 2")
    tp = texel_points(vertices, faces, lay)
    n = H * W
    sums = np.zeros((n, 4))
    views = np.zeros(n, np.int32)
    tr = dict(dir=[], r=[], cos=[], uv=[], t64=[], sums_after=[])
    for k, pose in enumerate(poses):
        dirs, r, cos, uv = TX.view_rays(tp, pose, K, images.shape[1:3], near, far, cos_min)
        o = pose[:3].astype(np.float64)
        t64 = np.full(n, np.inf)
        idx = np.flatnonzero(cos > 0.0)
        if len(idx):
            t64[idx] = RC.cast(o, dirs[idx].astype(np.float64), vertices, faces, 0.0, np.inf)[0]
        seen = (cos > 0.0) & (t64 >= r - tol)
        sc = float(pose.astype(np.float64)[7])
        with np.errstate(all="ignore"):
            wgt = np.where(seen, (cos * (sc / r)) * (sc / r), 0.0)
        col = TX.bilinear(images[k], uv[:, 0], uv[:, 1])
        i = np.flatnonzero(seen)
        sums[i, 0] += wgt[i]
        sums[i, 1:] += wgt[i, None] * col[i]
        views[i] += 1
        for key, val in zip(("dir", "r", "cos", "uv", "t64", "sums_after"), (dirs, r, cos, uv, t64, sums.copy())):
            tr[key].append(val)
    if fallback is not None:
        col = np.asarray(fallback, np.float32).astype(np.float64).reshape(-1, 3)
        fi = faces.astype(np.int64)[np.where(tp["owner"] >= 0, tp["owner"], 0)] if F else np.zeros((n, 3), np.int64)
        fi = np.where(tp["ok"][:, None], fi, 0)
        fb = ((tp["alpha"][:, None] * col[fi[:, 0]] + tp["beta"][:, None] * col[fi[:, 1]]) +
              tp["gamma"][:, None] * col[fi[:, 2]]) if len(col) else np.zeros((n, 3))
        fb = np.where(tp["ok"][:, None], fb, float(default_color))
    else:
        fb = np.full((n, 3), float(default_color))
    with np.errstate(all="ignore"):
        atlas = np.where((sums[:, 0] > 0.0)[:, None], sums[:, 1:] / sums[:, :1], fb)
    atlas = np.where((tp["owner"] >= 0)[:, None], atlas, 0.0).astype(np.float32)
    out = dict(lay, atlas=atlas.reshape(H, W, 3), views=views.reshape(H, W), sums=sums, num_faces=F,
               density=float(density))
    return dict(out, **tr) if trace else out


def sample_atlas(atlas, face_cell, f, beta, gamma):
    """texture_numpy.sample_atlas with the face's own cell: the four integer corners clamped into it."""
    at = np.asarray(atlas, np.float32).astype(np.float64)
    x, y, cell = atlas_xy(face_cell, f, beta, gamma)
    cx0, cy0, R = cell[:, 0], cell[:, 1], cell[:, 2]
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf)[:, None], (y - yf)[:, None]
    xi = np.clip(xf, cx0 - 1.0, cx0 + R + 1.0).astype(np.int64)
    yi = np.clip(yf, cy0 - 1.0, cy0 + R - 1 + 1.0).astype(np.int64)
    x0, x1 = np.clip(xi, cx0, cx0 + R), np.clip(xi + 1, cx0, cx0 + R)
    y0, y1 = np.clip(yi, cy0, cy0 + R - 1), np.clip(yi + 1, cy0, cy0 + R - 1)
    top = at[y0, x0] + fx * (at[y0, x1] - at[y0, x0])
    bot = at[y1, x0] + fx * (at[y1, x1] - at[y1, x0])
    return top + fy * (bot - top)


def shade_texture(pose, rays, vertices, faces, face, atlas, face_cell):
    """rgb f32[n,3]: the sized atlas sampled at beta = V / det, gamma = W / det of the hit face; 0 on a miss."""
    U, V, W, det, ok = TX.edge_functions(pose, rays, vertices, faces, face)
    with np.errstate(all="ignore"):
        beta, gamma = np.where(ok, V / det, 0.0), np.where(ok, W / det, 0.0)
    good = ok & np.isfinite(beta) & np.isfinite(gamma)
    if len(np.reshape(face_cell, (-1, 4))) == 0:
        return np.zeros((len(U), 3), np.float32)
    rgb = sample_atlas(atlas, face_cell, np.where(good, face, 0), np.where(good, beta, 0.0), np.where(good, gamma, 0.0))
    return np.where(good[:, None], rgb, 0.0).astype(np.float32)


# ---- the mixed checker room: the scene of the test that cannot pass without the sized atlas ---------------------------
MIXED_GRID = (16, 12)            # squares along y and z on the +x wall
MIXED_DENSITY = 9.0
MIXED_TEXELS = 8


def mixed_scene():
    """texture_numpy.checker_scene() with the +x wall (faces 2, 3) replaced by a 16 x 12 grid of squares of 0.25 m, two
    triangles each, wound as the quad they replace: 394 faces, 10 of 5 to 7.2 m and 384 of 0.35 m.  The grid's vertices
    are appended to the eight corners."""
    scene = dict(TX.checker_scene())
    V, F = scene["V"], scene["F"]
    ny, nz = MIXED_GRID
    a, b, c, d = (V[k].astype(np.float64) for k in (F[2][0], F[2][1], F[2][2], F[3][2]))    # the quad a, b, c, d
    assert np.array_equal(F[3][:2], F[2][[0, 2]])
    # a -> b runs along z, b -> c (= a -> d) along y
    gy, gz = np.arange(ny + 1) / ny, np.arange(nz + 1) / nz
    grid = a[None, None] + gz[None, :, None] * (b - a)[None, None] + gy[:, None, None] * (d - a)[None, None]
    base = len(V)
    vid = lambda iy, iz: base + iy * (nz + 1) + iz
    tris = []
    for iy in range(ny):
        for iz in range(nz):
            qa, qb, qc, qd = vid(iy, iz), vid(iy, iz + 1), vid(iy + 1, iz + 1), vid(iy + 1, iz)
            tris += [(qa, qb, qc), (qa, qc, qd)]
    scene["V"] = np.concatenate([V, grid.reshape(-1, 3).astype(np.float32)])
    scene["F"] = np.concatenate([F[:2], np.array(tris, np.int32), F[4:]]).astype(np.int32)
    scene.pop("colors")
    return scene


def owned(tex):
    return int((tex["owner"] >= 0).sum())


def uniform_texels_for(F, budget):
    """The smallest uniform `texels` whose owned texel count F R (R + 1) / 2 is not below `budget`."""
    R = 4
    while F * R * (R + 1) // 2 < budget:
        R += 1
    return R


def mixed_views(scene, tex):
    """(rgb f32[6,h,w,3], hit bool[6,h,w]) of the scene's mesh from its six poses, shaded by the statement from the
    dict of bake() (sized, with a face_cell) or of texture_numpy.bake() (uniform)."""
    h, w = scene["hw"]
    rgb, hit = [], []
    for pose in scene["poses"]:
        out = RC.render(pose, scene["rays"], scene["V"], scene["F"], 0.05, 10.0)
        if "face_cell" in tex:
            c = shade_texture(pose, scene["rays"], scene["V"], scene["F"], out[3], tex["atlas"], tex["face_cell"])
        else:
            c = TX.shade_texture(pose, scene["rays"], scene["V"], scene["F"], out[3], tex["atlas"], tex["texels"],
                                 tex["cols"])
        rgb.append(c.reshape(h, w, 3)), hit.append(out[2].reshape(h, w).astype(bool))
    return np.stack(rgb), np.stack(hit)


def mixed_statement():
    """The CPU statement on the mixed checker room -> (scene, sized texture dict, (rgb, hit) with it, uniform texture
    dict at the smallest texels with no fewer owned texels, (rgb, hit) with it).  Callers cache it."""
    scene = mixed_scene()
    args = (scene["V"], scene["F"], scene["images"], scene["poses"], scene["K"])
    sized = bake(*args, density=MIXED_DENSITY, texels=MIXED_TEXELS)
    uni = TX.bake(*args, R=uniform_texels_for(len(scene["F"]), owned(sized)))
    return scene, sized, mixed_views(scene, sized), uni, mixed_views(scene, uni)
