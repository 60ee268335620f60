"""Numpy statement of the mesh textures (DESIGN.md "Mesh textures"; the kernels are csrc/mesh_texture.hip, the Python
is mast3r_slam/tsdf/mesh_texture.py): the per-face atlas layout, the bake of keyframe images into it, and the shading
of a ray cast from vertex colours or from the atlas.  Everything is f64 on the f32 inputs, and the operation order
written here is the kernels': no sum is reassociated and a * b + c is two roundings."""
import numpy as np

import raycast_numpy as RC

M = 0.5                  # the local coordinate of barycentric 0: half a texel inside the cell


def span(R):
    """s: the local distance between barycentric 0 and 1."""
    return R - 3.5


def layout(F, R):
    """(cols, rows, H, W) of the atlas of F faces with R texels: a pure function of (F, R)."""
    F, R = int(F), int(R)
    if R < 4:
        raise ValueError(f"texels must be >= 4, got {R}")
    n_cells = (F + 1) >> 1
    cols = int(np.ceil(np.sqrt(n_cells)))
    while cols * cols < n_cells:
        cols += 1
    while cols > 0 and (cols - 1) * (cols - 1) >= n_cells:
        cols -= 1
    rows = (n_cells + cols - 1) // cols if cols else 0
    H, W = rows * R, cols * (R + 1)
    if H * W >= 1 << 31 or 3 * F >= 1 << 31:
        raise ValueError(f"an atlas of {H}x{W} texels / {F} faces is outside the int32 index range")
    return cols, rows, H, W


def texel_owner(F, R):
    """(owner i32[H,W], li i32[H,W], lj i32[H,W]): the face that owns each texel (-1: none) and the texel's local
    coordinates in that face's half-0 frame (half 1 through the mirror (i, j) -> (R - i, R - 1 - j))."""
    cols, rows, H, W = layout(F, R)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cx, cy = x // (R + 1), y // R
    c = cy * cols + cx
    i, j = x - cx * (R + 1), y - cy * R
    half = (i + j > R - 1).astype(np.int64)
    f = 2 * c + half
    owner = np.where((c < ((F + 1) >> 1)) & (f < F), f, -1).astype(np.int32)
    li = np.where(half == 1, R - i, i).astype(np.int32)
    lj = np.where(half == 1, R - 1 - j, j).astype(np.int32)
    return owner, li, lj


def texel_bary(li, lj, R):
    """(alpha, beta, gamma) f64 of an owned texel: beta = (i - m) / s, gamma = (j - m) / s, alpha = (1 - beta) - gamma,
    the negative ones set to 0 and the three divided by their sum (alpha + beta) + gamma."""
    s = span(R)
    beta = (li.astype(np.float64) - M) / s
    gamma = (lj.astype(np.float64) - M) / s
    alpha = (1.0 - beta) - gamma
    alpha, beta, gamma = (np.where(t < 0.0, 0.0, t) for t in (alpha, beta, gamma))
    tot = (alpha + beta) + gamma
    return alpha / tot, beta / tot, gamma / tot


def atlas_xy(f, beta, gamma, R, cols):
    """Atlas coordinates f64 (x, y), texel centres at integers, of the point with barycentrics (., beta, gamma) of face
    f: local (m + beta s, m + gamma s) for half 0, its mirror (R - x, (R - 1) - y) for half 1, plus the cell's origin."""
    f = np.asarray(f, np.int64)
    s = span(R)
    lx, ly = M + beta * s, M + gamma * s
    half = (f & 1) == 1
    lx, ly = np.where(half, R - lx, lx), np.where(half, (R - 1) - ly, ly)
    c = f >> 1
    return (c % cols) * (R + 1) + lx, (c // cols) * R + ly


def face_uv(F, R):
    """f64[F,3,2]: the atlas coordinates of the corners a, b, c of every face (MeshTexture.uv() rounds them to f32)."""
    cols = layout(F, R)[0]
    f = np.arange(F)
    out = np.zeros((F, 3, 2))
    for k, (b, g) in enumerate(((0.0, 0.0), (1.0, 0.0), (0.0, 1.0))):
        out[:, k, 0], out[:, k, 1] = atlas_xy(f, np.full(F, b), np.full(F, g), R, max(cols, 1))
    return out


def _corners(vertices, faces):
    """(a, b, c f64[F,3], in_range bool[F]); the corners of a face with an index outside [0, V) are zeros."""
    V = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    Fi = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((Fi >= 0) & (Fi < len(V))).all(1)
    g = np.where(ok[:, None], Fi, 0)
    if len(V) == 0:
        z = np.zeros((len(Fi), 3))
        return z, z, z, ok & False
    a, b, c = (np.where(ok[:, None], V[g[:, k]], 0.0) for k in range(3))
    return a, b, c, ok


def texel_points(vertices, faces, R):
    """Per texel of the atlas, flattened row-major: dict(owner, ok, alpha, beta, gamma, p f64[n,3], n f64[n,3]).  `ok`:
    the texel has an owner whose indices are in range.  p = (alpha a + beta b) + gamma c; n = (b - a) x (c - a) over its
    length sqrt((nx nx + ny ny) + nz nz) (zero or non-finite for a face that no view sees)."""
    F = len(np.reshape(faces, (-1, 3)))
    owner, li, lj = (t.reshape(-1) for t in texel_owner(F, R))
    a, b, c, in_range = _corners(vertices, faces)
    g = np.where(owner >= 0, owner, 0)
    ok = (owner >= 0) & (in_range[g] if F else False)
    al, be, ga = texel_bary(li, lj, R)
    if F == 0:
        z = np.zeros((len(owner), 3))
        return dict(owner=owner, ok=ok, alpha=al, beta=be, gamma=ga, p=z, n=z)
    A, B, C = a[g], b[g], c[g]
    p = (al[:, None] * A + be[:, None] * B) + ga[:, None] * C
    e1, e2 = B - A, C - A
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    with np.errstate(all="ignore"):
        n = n / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]
    return dict(owner=owner, ok=ok, alpha=al, beta=be, gamma=ga, p=p, n=n)


def view_rays(tp, pose, K, hw, near, far, cos_min):
    """One view of the view rule on the texels `tp` of texel_points -> (dir f32[n,3], r f64[n], cos f64[n], uv
    f64[n,2]).  A texel takes part geometrically when its camera-frame z > 0, -0.5 <= u < w - 0.5, -0.5 <= v < h - 0.5,
    near <= r <= far and cos = -(n . v) / r is >= cos_min and > 0 (back faces never qualify); every other texel has
    dir = 0, r = 0, cos = 0, uv = 0.  The operations are raycast_numpy.view_rays'."""
    p8 = np.asarray(pose, np.float32).astype(np.float64).reshape(8)
    K = np.asarray(K, np.float64).reshape(3, 3)
    h, w = hw
    v = tp["p"] - p8[:3]
    n = tp["n"]
    X = RC.rotate(np.array([-p8[3], -p8[4], -p8[5], p8[6]]), v)
    r = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    with np.errstate(all="ignore"):
        u = K[0, 0] * X[:, 0] / X[:, 2] + K[0, 2]
        vv = K[1, 1] * X[:, 1] / X[:, 2] + K[1, 2]
        cos = -((n[:, 0] * v[:, 0] + n[:, 1] * v[:, 1]) + n[:, 2] * v[:, 2]) / r
        dirs = (v / r[:, None]).astype(np.float32)
        take = (tp["ok"] & np.isfinite(n).all(1) & (X[:, 2] > 0.0) & (u >= -0.5) & (u < w - 0.5) & (vv >= -0.5) &
                (vv < h - 0.5) & (r >= near) & (r <= far) & (cos >= cos_min) & (cos > 0.0))
    z = np.zeros_like(r)
    return (np.where(take[:, None], dirs, np.float32(0.0)), np.where(take, r, z), np.where(take, cos, z),
            np.stack([np.where(take, u, z), np.where(take, vv, z)], 1))


def bilinear(image, u, v):
    """f64[n,C]: the bilinear sample of image f32[h,w,C] at (u, v), pixel centres at integers: uc = clamp(u, 0, w - 1),
    x0 = min(floor(uc), w - 2), fx = uc - x0, the same in v; a + f (b - a) along x, then along y."""
    img = np.asarray(image, np.float32).astype(np.float64)
    h, w = img.shape[:2]
    uc, vc = np.minimum(np.maximum(u, 0.0), w - 1.0), np.minimum(np.maximum(v, 0.0), h - 1.0)
    x0 = np.minimum(np.floor(uc), w - 2.0).astype(np.int64)
    y0 = np.minimum(np.floor(vc), h - 2.0).astype(np.int64)
    fx, fy = (uc - x0)[:, None], (vc - y0)[:, None]
    top = img[y0, x0] + fx * (img[y0, x0 + 1] - img[y0, x0])
    bot = img[y0 + 1, x0] + fx * (img[y0 + 1, x0 + 1] - img[y0 + 1, x0])
    return top + fy * (bot - top)


def bake(vertices, faces, images, poses, K, R=8, near=0.05, far=10.0, tol=0.01, cos_min=0.1, fallback=None,
         default_color=0.5, trace=False):
    """dict(atlas f32[H,W,3], views i32[H,W], owner i32[H,W], sums f64[H W,4]) and, with `trace`, per view the lists
    dir, r, cos, uv, t64.  The views are added in index order: S0 += wgt, Sc += wgt I_c with wgt = (cos (sc / r))
    (sc / r)."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    images = np.asarray(images, np.float32)
    poses = np.asarray(poses, np.float32).reshape(-1, 8)
    F = len(faces)
    cols, rows, H, W = layout(F, R)
    if len(poses) and (images.ndim != 4 or images.shape[1] < 2 or images.shape[2] < 2):
        raise ValueError("images must be (K,h,w,3) with h, w >= 2")
    tp = texel_points(vertices, faces, R)
    n = H * W
    sums = np.zeros((n, 4))
    views = np.zeros(n, np.int32)
    tr = dict(dir=[], r=[], cos=[], uv=[], t64=[])
    for k, pose in enumerate(poses):
        hw = images.shape[1:3]
        dirs, r, cos, uv = view_rays(tp, pose, K, hw, near, far, cos_min)
        o = pose[:3].astype(np.float64)
        t64 = np.full(n, np.inf)
        idx = np.flatnonzero(cos > 0.0)
        if len(idx):
            t64[idx] = RC.cast(o, dirs[idx].astype(np.float64), vertices, faces, 0.0, np.inf)[0]
        seen = (cos > 0.0) & (t64 >= r - tol)
        sc = float(pose.astype(np.float64)[7])
        with np.errstate(all="ignore"):
            wgt = np.where(seen, (cos * (sc / r)) * (sc / r), 0.0)
        col = bilinear(images[k], uv[:, 0], uv[:, 1])
        i = np.flatnonzero(seen)
        sums[i, 0] += wgt[i]
        sums[i, 1:] += wgt[i, None] * col[i]
        views[i] += 1
        for key, val in zip(("dir", "r", "cos", "uv", "t64"), (dirs, r, cos, uv, t64)):
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
    out = dict(atlas=atlas.reshape(H, W, 3), views=views.reshape(H, W), owner=tp["owner"].reshape(H, W), sums=sums,
               texels=int(R), cols=cols, rows=rows, num_faces=F)
    return dict(out, **tr) if trace else out


def edge_functions(pose, rays, vertices, faces, face):
    """(U, V, W, det f64[n], ok bool[n]) of the rays against the one face `face` i32[n] each hit (ok: face in [0, F) with
    its indices in range): steps 1-4 of DESIGN.md "Mesh ray casting", raycast_numpy.cast's operations."""
    o, d, _ = RC.directions(pose, rays)
    a, b, c, in_range = _corners(vertices, faces)
    face = np.asarray(face, np.int64).reshape(-1)
    F = len(a)
    inside = (face >= 0) & (face < F)
    g = np.where(inside, face, 0)
    ok = inside & (in_range[g] if F else False)
    if F == 0:
        z = np.zeros(len(d))
        return z, z, z, z, ok
    ad = np.abs(d)
    kz = np.where(ad[:, 1] > ad[:, 0], 1, 0)
    kz = np.where(ad[:, 2] > RC._take(ad, kz), 2, kz)
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    with np.errstate(all="ignore"):
        dz = RC._take(d, kz)
        kx, ky = np.where(dz < 0.0, ky, kx), np.where(dz < 0.0, kx, ky)
        Sx, Sy = RC._take(d, kx) / dz, RC._take(d, ky) / dz
        x, y = [], []
        for v in (a[g], b[g], c[g]):
            q = v - o
            x.append(RC._take(q, kx) - Sx * RC._take(q, kz))
            y.append(RC._take(q, ky) - Sy * RC._take(q, kz))
        U = x[2] * y[1] - y[2] * x[1]
        V = x[0] * y[2] - y[0] * x[2]
        W = x[1] * y[0] - y[1] * x[0]
        det = (U + V) + W
    return U, V, W, det, ok


def shade_colors(pose, rays, vertices, faces, face, colors):
    """rgb f32[n,3] = ((U ca + V cb) + W cc) / det on a hit, 0 on a miss."""
    U, V, W, det, ok = edge_functions(pose, rays, vertices, faces, face)
    col = np.asarray(colors, np.float32).astype(np.float64).reshape(-1, 3)
    fi = np.asarray(faces, np.int64).reshape(-1, 3)
    fi = np.where(ok[:, None], fi[np.where(ok, face, 0)], 0) if len(fi) else np.zeros((len(U), 3), np.int64)
    with np.errstate(all="ignore"):
        rgb = ((U[:, None] * col[fi[:, 0]] + V[:, None] * col[fi[:, 1]]) + W[:, None] * col[fi[:, 2]]) / det[:, None]
    return np.where(ok[:, None], rgb, 0.0).astype(np.float32)


def sample_atlas(atlas, f, beta, gamma, R, cols):
    """f64[n,3]: the bilinear sample of atlas f32[H,W,3] at the atlas coordinates of (beta, gamma) on face f; the four
    integer corners are clamped into the face's cell (a guard: inside the closed triangle they lie in it)."""
    at = np.asarray(atlas, np.float32).astype(np.float64)
    x, y = atlas_xy(f, beta, gamma, R, cols)
    c = np.asarray(f, np.int64) >> 1
    cx0, cy0 = (c % cols) * (R + 1), (c // cols) * R
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf)[:, None], (y - yf)[:, None]
    xi = np.clip(xf, cx0 - 1.0, cx0 + R + 1.0).astype(np.int64)      # the doubles first: the conversion is defined
    yi = np.clip(yf, cy0 - 1.0, cy0 + R - 1 + 1.0).astype(np.int64)
    x0, x1 = np.clip(xi, cx0, cx0 + R), np.clip(xi + 1, cx0, cx0 + R)
    y0, y1 = np.clip(yi, cy0, cy0 + R - 1), np.clip(yi + 1, cy0, cy0 + R - 1)
    top = at[y0, x0] + fx * (at[y0, x1] - at[y0, x0])
    bot = at[y1, x0] + fx * (at[y1, x1] - at[y1, x0])
    return top + fy * (bot - top)


def shade_texture(pose, rays, vertices, faces, face, atlas, R, cols):
    """rgb f32[n,3]: the atlas sampled at beta = V / det, gamma = W / det of the hit face; 0 on a miss."""
    U, V, W, det, ok = edge_functions(pose, rays, vertices, faces, face)
    with np.errstate(all="ignore"):
        beta, gamma = np.where(ok, V / det, 0.0), np.where(ok, W / det, 0.0)
    good = ok & np.isfinite(beta) & np.isfinite(gamma)
    rgb = sample_atlas(atlas, np.where(good, face, 0), np.where(good, beta, 0.0), np.where(good, gamma, 0.0), R, cols)
    return np.where(good[:, None], rgb, 0.0).astype(np.float32)


def parse_obj(text):
    """(v f64[V,3], vt f64[T,2], vn f64[N,3], faces i64[F,3,k]) of the OBJ text save_textured_mesh writes; the face
    entries are 0-based (v, vt[, vn])."""
    v, vt, vn, fc, mtl, use = [], [], [], [], None, None
    for ln in text.splitlines():
        w = ln.split()
        if not w or w[0].startswith("#"):
            continue
        if w[0] == "v":
            v.append([float(t) for t in w[1:4]])
        elif w[0] == "vt":
            vt.append([float(t) for t in w[1:3]])
        elif w[0] == "vn":
            vn.append([float(t) for t in w[1:4]])
        elif w[0] == "f":
            fc.append([[int(t) - 1 for t in e.split("/")] for e in w[1:4]])
        elif w[0] == "mtllib":
            mtl = w[1]
        elif w[0] == "usemtl":
            use = w[1]
    k = len(fc[0][0]) if fc else 2
    return (np.array(v, np.float64).reshape(-1, 3), np.array(vt, np.float64).reshape(-1, 2),
            np.array(vn, np.float64).reshape(-1, 3), np.array(fc, np.int64).reshape(-1, 3, k), mtl, use)


# ---- the checker room: the scene of the test that cannot pass without textures ----------------------------------------
CHECKER_PERIOD = 0.5
CHECKER_VIEWS = (0, 160, 330, 500, 670, 840)
CHECKER_HW = (96, 128)
CHECKER_TEXELS = 64
_BRIGHT, _DARK = np.array([0.9, 0.85, 0.2]), np.array([0.1, 0.15, 0.7])


def checker(P, axis):
    """f64[n,3]: the world-space checker of period 0.5 m on the wall whose normal is `axis` (int[n]) at the points P:
    the parity of the sum of floor(coordinate / period) over the two in-plane coordinates."""
    cell = np.floor(np.asarray(P, np.float64) / CHECKER_PERIOD)
    cell[np.arange(len(cell)), axis] = 0.0
    odd = (cell.sum(1) % 2.0) == 1.0
    return np.where(odd[:, None], _BRIGHT, _DARK)


def checker_scene():
    """dict of the checker room: V, F (synthetic.room_mesh, 12 faces), poses f32[6,8] (synthetic.camera_pose), K, hw,
    rays f32[h,w,3] (unit pinhole rays), images f32[6,h,w,3] rendered analytically - synthetic.ray_box_depth along each
    ray, the checker at the point hit - and colors f32[8,3], the checker at the eight corners (as a point of a z wall)."""
    from mast3r_slam import synthetic

    V, F = synthetic.room_mesh()
    h, w = CHECKER_HW
    K = synthetic.intrinsics(h, w).astype(np.float64)
    d = synthetic.pixel_rays(h, w, K)
    rays = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    poses = np.stack([synthetic.camera_pose(k) for k in CHECKER_VIEWS]).astype(np.float32)
    images = []
    for pose in poses:
        o, dw, _ = RC.directions(pose, rays)
        P = o + synthetic.ray_box_depth(o, dw)[:, None] * dw
        axis = np.argmin(np.abs(np.abs(P) - synthetic.ROOM_HALF), 1)
        images.append(checker(P, axis).reshape(h, w, 3))
    colors = checker(V.astype(np.float64), np.full(len(V), 2)).astype(np.float32)
    return dict(V=V, F=F, poses=poses, K=K, hw=(h, w), rays=rays, images=np.stack(images).astype(np.float32),
                colors=colors)


def checker_views(scene, colors=None, texture=None):
    """(rgb f32[6,h,w,3], hit bool[6,h,w]) of the scene's mesh from its six poses, shaded by the statement from vertex
    colours or from the dict of bake()."""
    h, w = scene["hw"]
    rgb, hit = [], []
    for pose in scene["poses"]:
        out = RC.render(pose, scene["rays"], scene["V"], scene["F"], 0.05, 10.0)
        if colors is not None:
            c = shade_colors(pose, scene["rays"], scene["V"], scene["F"], out[3], colors)
        else:
            c = shade_texture(pose, scene["rays"], scene["V"], scene["F"], out[3], texture["atlas"], texture["texels"],
                              texture["cols"])
        rgb.append(c.reshape(h, w, 3)), hit.append(out[2].reshape(h, w).astype(bool))
    return np.stack(rgb), np.stack(hit)


def checker_statement():
    """The CPU statement on the checker room -> (scene, texture dict, rgb and hit with the texture, rgb and hit with the
    vertex colours).  A few seconds of numpy; callers cache it."""
    scene = checker_scene()
    tex = bake(scene["V"], scene["F"], scene["images"], scene["poses"], scene["K"], R=CHECKER_TEXELS)
    return scene, tex, checker_views(scene, texture=tex), checker_views(scene, colors=scene["colors"])
