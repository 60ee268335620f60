"""Mesh textures on the device: keyframe images baked into a per-face atlas (bake_texture -> MeshTexture), and colour
views of a mesh from its vertex colours or its texture (render_mesh_color), which tsdf.image_metrics scores against
images as it scores the TSDF's colour views.

No counterpart in the reference.  The kernels are csrc/mesh_texture.hip (DESIGN.md "Mesh textures"); the numpy statement
of the same definitions is tests/texture_numpy.py.  With `density=` the atlas is the sized one (DESIGN.md "Mesh textures:
sized atlas", tests/texture_sized_numpy.py): a resolution per face from its longest edge, packed in one band per class.  The occlusion test is the ray cast of mesh_raycast, called exactly
as observed_points calls it.  There is no CPU path and no uncalibrated path: a texel is projected, and the ray-image
camera model has no projection."""
import ctypes
import math

import numpy as np
import torch

import mslam_hip as _m

from ._mesh_args import _pair
from ._view_args import _eye, _K_arg, _poses_arg, _range_arg
from .global_volume import _render_args
from .mesh_raycast import _Caster


def atlas_layout(num_faces, texels):
    """(cols, rows, H, W) of the atlas of `num_faces` faces with `texels` = R >= 4: face f is half f & 1 of cell f >> 1,
    a cell is R + 1 wide and R high, cols = ceil(sqrt(cells)), rows = ceil(cells / cols).  A pure function of (F, R)."""
    F, R = int(num_faces), int(texels)
    if R != texels or R < 4:
        raise ValueError(f"bake_texture: texels must be an integer >= 4, got {texels!r}")
    cells = (F + 1) >> 1
    cols = math.isqrt(cells)
    cols += 1 if cols * cols < cells else 0
    rows = (cells + cols - 1) // cols if cols else 0
    H, W = rows * R, cols * (R + 1)
    if F < 0 or H * W >= 1 << 31 or 3 * F >= 1 << 31:
        raise ValueError(f"bake_texture: an atlas of {H}x{W} texels for {F} faces is outside the int32 index range")
    return cols, rows, H, W


atlas_classes = (4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256)      # R of the sized atlas; each step is <= 1.5x


def _floor_and_cap(texels, max_texels, what="bake_texture"):
    """The indices into atlas_classes of the smallest class >= texels and of the largest class <= max_texels."""
    if int(texels) != texels or texels < 4:
        raise ValueError(f"{what}: texels must be an integer >= 4, got {texels!r}")
    lo = [c for c, R in enumerate(atlas_classes) if R >= texels]
    if not lo:
        raise ValueError(f"{what}: with density, texels must not exceed the largest class {atlas_classes[-1]}, got "
                         f"{texels!r}")
    le = [c for c, R in enumerate(atlas_classes) if R <= max_texels]
    if not le or le[-1] < lo[0]:
        raise ValueError(f"{what}: max_texels {max_texels!r} is below the floor class {atlas_classes[lo[0]]}")
    return lo[0], le[-1]


def sized_layout(counts):
    """(H, W, bands) of the sized atlas, a pure function of the 13 per-class face counts: `bands` has a row (R, cols,
    rows, y0, base, count) per class of atlas_classes.  cells = (count + 1) >> 1, A = sum cells (R + 1) R,
    W = max(ceil(sqrt(A)), R_top + 1) for the largest class in use; the bands run from that class down, cols =
    W // (R + 1), rows = ceil(cells / cols), y0 the rows of texels above, base the faces of the classes above (the band's
    first position in `order`).  Cell q of a band lies at ((q % cols)(R + 1), y0 + (q // cols) R)."""
    counts = [int(c) for c in counts]
    if len(counts) != len(atlas_classes) or min(counts) < 0:
        raise ValueError(f"sized_layout: {len(atlas_classes)} non-negative counts expected, got {counts}")
    cells = [(c + 1) >> 1 for c in counts]
    area = sum(q * (R + 1) * R for q, R in zip(cells, atlas_classes))
    used = [R for R, c in zip(atlas_classes, counts) if c]
    W = 0
    if used:
        W = math.isqrt(area)
        W = max(W + (1 if W * W < area else 0), used[-1] + 1)
    bands, y0, base = [None] * len(counts), 0, 0
    for c in range(len(counts) - 1, -1, -1):
        R = atlas_classes[c]
        cols = W // (R + 1)
        rows = -(-cells[c] // cols) if cells[c] else 0
        bands[c] = (R, cols, rows, y0, base, counts[c])
        y0, base = y0 + rows * R, base + counts[c]
    if y0 * W >= 1 << 31 or 3 * base >= 1 << 31:
        raise ValueError(f"bake_texture: an atlas of {y0}x{W} texels for {base} faces is outside the int32 index range")
    return y0, W, bands


class MeshTexture:
    """A per-face texture atlas: atlas f32[H,W,3] in [0,1], views i32[H,W] (the views that took part in each texel),
    owner i32[H,W] (the face a texel belongs to, -1 for none), texels, cols, rows, num_faces.  A sized atlas
    (bake_texture(density=...)) also carries face_cell i32[F,4] = (x0, y0, R_f, half), face_texels i32[F] = R_f, counts
    (the 13 per-class face counts, the argument of sized_layout), clamped (the faces that needed more than max_texels)
    and density; its texels is the floor class and its cols, rows are 0."""

    def __init__(self, atlas, views, owner, texels, cols, rows, num_faces, face_cell=None, face_texels=None, counts=None,
                 clamped=0, density=None):
        self.atlas, self.views, self.owner = atlas, views, owner
        self.texels, self.cols, self.rows, self.num_faces = int(texels), int(cols), int(rows), int(num_faces)
        self.face_cell, self.face_texels, self.counts = face_cell, face_texels, counts
        self.clamped, self.density = int(clamped), density

    @property
    def sized(self):
        return self.face_cell is not None

    def uv(self):
        """f32[F,3,2] on the atlas's device: the atlas coordinates (x, y), texel centres at integers, of the corners a, b,
        c of every face - local (m + beta s, m + gamma s) with m = 0.5, s = texels - 3.5 for an even face, the mirror
        (R - x, R - 1 - y) for an odd one, plus the cell's origin; computed in f64.  A sized atlas: the same with the
        face's own R_f, half and origin from face_cell."""
        if self.sized:
            cell = self.face_cell.to(torch.int64)
            x0, y0, Rf, odd = cell[:, 0].double(), cell[:, 1].double(), cell[:, 2].double(), cell[:, 3] == 1
            s = Rf - 3.5
            out = []
            for beta, gamma in ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0)):
                lx, ly = 0.5 + beta * s, 0.5 + gamma * s
                out.append(torch.stack((x0 + torch.where(odd, Rf - lx, lx), y0 + torch.where(odd, (Rf - 1) - ly, ly)), -1))
            return torch.stack(out, 1).float()
        R, F = self.texels, self.num_faces
        f = torch.arange(F, dtype=torch.int64, device=self.atlas.device)
        c, odd = f >> 1, (f & 1).bool()
        x0 = ((c % max(self.cols, 1)) * (R + 1)).double()
        y0 = (torch.div(c, max(self.cols, 1), rounding_mode="floor") * R).double()
        s = R - 3.5
        out = []
        for beta, gamma in ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0)):
            lx, ly = 0.5 + beta * s, 0.5 + gamma * s
            lx, mx, ly, my = (x0.new_tensor(t) for t in (lx, R - lx, ly, (R - 1) - ly))       # f64 scalars
            out.append(torch.stack((x0 + torch.where(odd, mx, lx), y0 + torch.where(odd, my, ly)), -1))
        return torch.stack(out, 1).float() if F else torch.zeros((0, 3, 2), dtype=torch.float32, device=f.device)


def _colors_arg(colors, V, device, what, name="colors"):
    if not torch.is_tensor(colors):
        raise TypeError(f"{what}: {name} must be a device tensor")
    if colors.dim() != 2 or tuple(colors.shape) != (V, 3):
        raise ValueError(f"{what}: {name} must be ({V},3), got {tuple(colors.shape)}")
    _m.require_dtype(colors, torch.float32, name)
    _m.ptr(colors)
    if colors.device != device:
        raise ValueError(f"{what}: {name} and the mesh are on different devices")
    return colors.contiguous()


class _Baker:
    """The launches of one bake, one method per kernel, over the texels of one atlas; the raw-entry tests and
    tools/mesh_texture_time.py walk the same methods that bake_texture walks."""

    def __init__(self, caster, texels):
        self.c, self.R = caster, int(texels)
        self.cols, self.rows, self.H, self.W = atlas_layout(caster.F, texels)
        self.n, dev = self.H * self.W, caster.device
        self.atlas_args = (caster.F, self.R, self.cols, self.rows)
        self.dir = torch.empty((self.n, 3), dtype=torch.float32, device=dev)
        self.r = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.cos = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.uv = torch.empty((self.n, 2), dtype=torch.float64, device=dev)
        self.sums = torch.zeros((self.n, 4), dtype=torch.float64, device=dev)
        self.views = torch.zeros(self.n, dtype=torch.int32, device=dev)

    def layout(self):
        owner = torch.empty(self.n, dtype=torch.int32, device=self.c.device)
        _m.check(_m.lib().mslam_mesh_texture_layout(*self.atlas_args, _m.ptr(owner), _m.stream_ptr()),
                 "mesh_texture_layout")
        return owner.view(self.H, self.W)

    def rays(self, pose, K4, hw, near, far, cos_min):
        c = self.c
        _m.check(_m.lib().mslam_mesh_texture_rays(_m.ptr(c.v), _m.ptr(c.f), c.F, c.V, self.R, self.cols, self.rows,
                                                  _m.ptr(pose), *K4, int(hw[0]), int(hw[1]), float(near), float(far),
                                                  float(cos_min), _m.ptr(self.dir), _m.ptr(self.r), _m.ptr(self.cos),
                                                  _m.ptr(self.uv), _m.stream_ptr()), "mesh_texture_rays")

    def cast(self, pose):
        """The occlusion rays of the last `rays` from the pose's origin, as observed_points casts them -> t64."""
        if self.n == 0:
            return torch.empty(0, dtype=torch.float64, device=self.c.device)
        return self.c.cast(self.dir, 1, self.n, _eye(pose), 0.0, float("inf"), t64=True)[4]

    def accumulate(self, t64, image, pose, tol):
        h, w = int(image.shape[0]), int(image.shape[1])
        _m.check(_m.lib().mslam_mesh_texture_accumulate(_m.ptr(t64), _m.ptr(self.r), _m.ptr(self.cos), _m.ptr(self.uv),
                                                        _m.ptr(image), h, w, _m.ptr(pose), float(tol), self.n,
                                                        _m.ptr(self.sums), _m.ptr(self.views), _m.stream_ptr()),
                 "mesh_texture_accumulate")

    def resolve(self, colors, default_color):
        c = self.c
        atlas = torch.empty((self.n, 3), dtype=torch.float32, device=c.device)
        _m.check(_m.lib().mslam_mesh_texture_resolve(_m.ptr(c.f), c.F, c.V, self.R, self.cols, self.rows,
                                                     _m.ptr(self.sums), _m.ptr(colors), float(default_color),
                                                     _m.ptr(atlas), _m.stream_ptr()), "mesh_texture_resolve")
        return atlas.view(self.H, self.W, 3)


class _SizedBaker(_Baker):
    """The launches of one bake into a sized atlas: classes, rank, one host read of the counts, layout, and the sized
    forms of rays and resolve; cast and accumulate are _Baker's, which never see the layout."""

    def __init__(self, caster, density, texels, max_texels):
        density = float(density)
        if not (density > 0.0 and math.isfinite(density)):
            raise ValueError(f"bake_texture: density must be a positive number, got {density!r}")
        self.c, self.density = caster, density
        self.lo, self.cap = _floor_and_cap(texels, max_texels)
        self.R = atlas_classes[self.lo]

    def classes(self):
        c, dev = self.c, self.c.device
        self.cls = torch.empty(c.F, dtype=torch.int32, device=dev)
        self.over = torch.empty(c.F, dtype=torch.int32, device=dev)
        _m.check(_m.lib().mslam_mesh_texture_classes(_m.ptr(c.v), _m.ptr(c.f), c.F, c.V, self.density, self.lo, self.cap,
                                                     _m.ptr(self.cls), _m.ptr(self.over), _m.stream_ptr()),
                 "mesh_texture_classes")

    def ranks(self):
        c, dev, L = self.c, self.c.device, _m.lib()
        ints = int(L.mslam_mesh_texture_rank_table_ints(c.F))
        table = torch.empty(ints, dtype=torch.int32, device=dev)
        self.rank = torch.empty(c.F, dtype=torch.int32, device=dev)
        self.order = torch.empty(c.F, dtype=torch.int32, device=dev)
        self.counts14 = torch.empty(len(atlas_classes) + 1, dtype=torch.int32, device=dev)
        _m.check(L.mslam_mesh_texture_rank(_m.ptr(self.cls), _m.ptr(self.over), c.F, _m.ptr(table), ints,
                                           _m.ptr(self.rank), _m.ptr(self.order), _m.ptr(self.counts14), _m.stream_ptr()),
                 "mesh_texture_rank")

    def read_counts(self):
        """The one host read of the bake: the 13 class counts and the clamped count; then the packing and the texel
        buffers."""
        got = self.counts14.cpu().tolist()
        self.counts, self.clamped = tuple(got[:-1]), got[-1]
        self.H, self.W, self.bands = sized_layout(self.counts)
        self.n, dev = self.H * self.W, self.c.device
        self.dir = torch.empty((self.n, 3), dtype=torch.float32, device=dev)
        self.r = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.cos = torch.empty(self.n, dtype=torch.float64, device=dev)
        self.uv = torch.empty((self.n, 2), dtype=torch.float64, device=dev)
        self.sums = torch.zeros((self.n, 4), dtype=torch.float64, device=dev)
        self.views = torch.zeros(self.n, dtype=torch.int32, device=dev)

    def layout(self):
        c, dev = self.c, self.c.device
        self.owner = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.face_cell = torch.empty((c.F, 4), dtype=torch.int32, device=dev)
        bands = (ctypes.c_int32 * (6 * len(atlas_classes)))(*[v for row in self.bands for v in row])   # host memory
        _m.check(_m.lib().mslam_mesh_texture_layout_sized(ctypes.addressof(bands), c.F, self.H, self.W, _m.ptr(self.cls),
                                                          _m.ptr(self.rank), _m.ptr(self.order), _m.ptr(self.owner),
                                                          _m.ptr(self.face_cell), _m.stream_ptr()),
                 "mesh_texture_layout_sized")
        return self.owner.view(self.H, self.W)

    def rays(self, pose, K4, hw, near, far, cos_min):
        c = self.c
        _m.check(_m.lib().mslam_mesh_texture_rays_sized(_m.ptr(c.v), _m.ptr(c.f), c.F, c.V, _m.ptr(self.owner),
                                                        _m.ptr(self.face_cell), self.H, self.W, _m.ptr(pose), *K4,
                                                        int(hw[0]), int(hw[1]), float(near), float(far), float(cos_min),
                                                        _m.ptr(self.dir), _m.ptr(self.r), _m.ptr(self.cos),
                                                        _m.ptr(self.uv), _m.stream_ptr()), "mesh_texture_rays_sized")

    def resolve(self, colors, default_color):
        c = self.c
        atlas = torch.empty((self.n, 3), dtype=torch.float32, device=c.device)
        _m.check(_m.lib().mslam_mesh_texture_resolve_sized(_m.ptr(c.f), c.F, c.V, _m.ptr(self.owner),
                                                           _m.ptr(self.face_cell), self.H, self.W, _m.ptr(self.sums),
                                                           _m.ptr(colors), float(default_color), _m.ptr(atlas),
                                                           _m.stream_ptr()), "mesh_texture_resolve_sized")
        return atlas.view(self.H, self.W, 3)

    def texture(self, atlas, owner):
        R = torch.tensor(atlas_classes, dtype=torch.int32, device=self.c.device)
        return MeshTexture(atlas, self.views.view(self.H, self.W), owner, self.R, 0, 0, self.c.F,
                           face_cell=self.face_cell, face_texels=R[self.cls.long()], counts=self.counts,
                           clamped=self.clamped, density=self.density)


def bake_texture(mesh, images, poses, K, texels=8, near=0.05, far=10.0, tol=0.01, cos_min=0.1, fallback=None,
                 default_color=0.5, skip=True, index=None, validate=True, density=None, max_texels=256):
    """Bakes camera images into a per-face texture atlas of a mesh -> MeshTexture (DESIGN.md "Mesh textures").
    `mesh`: (vertices f32[V,3], faces i32[F,3]) device tensors or an extract_mesh tuple.  `images` f32[K,h,w,3] in
    [0,1] (h, w >= 2), `poses` Sim3 [K,8] [t, q, s], world from camera, rounded to f32, and one pinhole `K` (3,3), pixel
    centres at integers.  K = 0 views is legal: every texel then comes from the fallback.

    Every texel of the atlas stands for a point p of its face (atlas_layout; `texels` = R: each face gets R (R + 1) / 2
    texels).  View k takes part in it when, all in f64: p's camera-frame z > 0; -0.5 <= u < w - 0.5, -0.5 <= v < h - 0.5;
    near <= r = |p - t| <= far; cos = -(n . (p - t)) / r >= cos_min (and > 0) for the face's unit normal n; and the ray
    from t towards p misses the mesh or first hits it at t64 >= r - tol (the cast of observed_points; `skip`, `index` as
    there).  The texel is the mean of the bilinear samples of those images, weighted by cos (s / r)^2, the views added in
    index order: bit-identical from call to call.  A texel no view takes part in is the `fallback`: vertex colours
    f32[V,3] interpolated at p (True: the colours of a 4-tensor extract_mesh tuple), or `default_color`.

    With a `density` > 0, in texels per world unit, the atlas is the sized one (DESIGN.md "Mesh textures: sized atlas"):
    face f gets R_f, the smallest of atlas_classes >= ceil(density L + 3.5) for its longest edge L, so that L spans at
    least density L texels; at least the smallest class >= `texels`, at most the largest class <= `max_texels` (the faces
    that needed more are counted in MeshTexture.clamped).  The cells of a class lie in one band (sized_layout); inside
    a cell nothing changes.  One host read, of the per-class face counts."""
    what = "bake_texture"
    if density is not None:
        density = float(density)
        if not (density > 0.0 and math.isfinite(density)):
            raise ValueError(f"{what}: density must be a positive number, got {density!r}")
        _floor_and_cap(texels, max_texels, what)
    mesh = tuple(mesh)
    vertices, faces = _pair(mesh, "mesh")
    caster = _Caster(vertices, faces, validate, bool(skip), what, index)
    dev = caster.device
    if fallback is True:
        if len(mesh) != 4 or mesh[3] is None:
            raise ValueError(f"{what}: fallback=True needs an extract_mesh tuple with colours")
        fallback = mesh[3]
    colors = None if fallback is None or fallback is False else _colors_arg(fallback, caster.V, dev, what, "fallback")
    poses = _poses_arg(poses, what).to(torch.float32)
    n_views = int(poses.shape[0])
    if not torch.is_tensor(images):
        images = torch.as_tensor(np.asarray(images, np.float32))
    if images.dim() != 4 or images.shape[3] != 3 or not images.is_floating_point():
        raise ValueError(f"{what}: images must be float (K,h,w,3), got {tuple(images.shape)} {images.dtype}")
    if int(images.shape[0]) != n_views:
        raise ValueError(f"{what}: {int(images.shape[0])} images but {n_views} poses")
    h, w = int(images.shape[1]), int(images.shape[2])
    if n_views and (h < 2 or w < 2):
        raise ValueError(f"{what}: images must be at least 2x2, got {h}x{w}")
    if n_views and images.device != dev:
        if images.is_cuda:
            raise ValueError(f"{what}: images and the mesh are on different devices")
        images = images.to(dev)
    K4 = _K_arg(K, what)
    near, far = _range_arg(near, far, what, strict=False)
    if not float(tol) == float(tol) or not float(cos_min) == float(cos_min):
        raise ValueError(f"{what}: tol and cos_min must be numbers")
    with torch.cuda.device(dev):
        if density is None:
            bk = _Baker(caster, texels)
        else:
            bk = _SizedBaker(caster, density, texels, max_texels)
            bk.classes()
            bk.ranks()
            bk.read_counts()
        owner = bk.layout()
        pd = poses.to(dev)
        for k in range(n_views):
            bk.rays(pd[k], K4, (h, w), near, far, cos_min)
            t64 = bk.cast(pd[k])
            bk.accumulate(t64, images[k].detach().to(torch.float32).contiguous(), pd[k], tol)
        atlas = bk.resolve(colors, default_color)
    if density is not None:
        return bk.texture(atlas, owner)
    return MeshTexture(atlas, bk.views.view(bk.H, bk.W), owner, bk.R, bk.cols, bk.rows, caster.F)


def render_mesh_color(mesh, pose, colors=None, texture=None, rays=None, K=None, hw=None, near=0.05, far=10.0, skip=True,
                      validate=True, index=None):
    """A colour view of a triangle mesh -> (range f32[h,w], normals f32[h,w,3], hit bool[h,w], rgb f32[h,w,3]): the
    first three are render_mesh's, bit for bit, with its arguments; rgb is 0 on a miss.  Exactly one of `colors`
    f32[V,3] (vertex colours, interpolated by the hit's barycentrics) and `texture` (a MeshTexture of this mesh, sampled
    bilinearly at the hit's atlas coordinates) is given; True for `colors` takes them from a 4-tensor extract_mesh tuple.
    The barycentrics are (U, V, W) / ((U + V) + W) of the edge functions of the face hit, recomputed as the cast
    computes them (DESIGN.md "Mesh textures")."""
    what = "render_mesh_color"
    mesh = tuple(mesh)
    if (colors is None) == (texture is None):
        raise ValueError(f"{what}: give exactly one of colors and texture")
    vertices, faces = _pair(mesh, "mesh")
    caster = _Caster(vertices, faces, validate, bool(skip), what, index)
    dev = caster.device
    if colors is True:
        if len(mesh) != 4 or mesh[3] is None:
            raise ValueError(f"{what}: colors=True needs an extract_mesh tuple with colours")
        colors = mesh[3]
    if colors is not None:
        colors = _colors_arg(colors, caster.V, dev, what)
        atlas, layout = None, (0, 0, 0)
    else:
        if not isinstance(texture, MeshTexture):
            raise TypeError(f"{what}: texture must be a MeshTexture")
        if texture.num_faces != caster.F:
            raise ValueError(f"{what}: the texture was baked for {texture.num_faces} faces, the mesh has {caster.F}")
        if texture.atlas.device != dev:
            raise ValueError(f"{what}: texture and the mesh are on different devices")
        _m.require_dtype(texture.atlas, torch.float32, "texture.atlas")
        if texture.sized:
            H, W, _ = sized_layout(texture.counts)
            if sum(texture.counts) != caster.F or tuple(texture.atlas.shape) != (H, W, 3):
                raise ValueError(f"{what}: the texture's atlas {tuple(texture.atlas.shape)} is not the sized layout of "
                                 f"its {sum(texture.counts)} faces by class, {H}x{W}")
            face_cell = texture.face_cell
            if not torch.is_tensor(face_cell) or tuple(face_cell.shape) != (caster.F, 4):
                raise ValueError(f"{what}: texture.face_cell must be ({caster.F},4)")
            _m.require_dtype(face_cell, torch.int32, "texture.face_cell")
            if face_cell.device != dev:
                raise ValueError(f"{what}: texture.face_cell and the mesh are on different devices")
            atlas, layout, face_cell = texture.atlas.contiguous(), (H, W), face_cell.contiguous()
        else:
            cols, rows, H, W = atlas_layout(caster.F, texture.texels)
            if (texture.cols, texture.rows) != (cols, rows) or tuple(texture.atlas.shape) != (H, W, 3):
                raise ValueError(f"{what}: the texture's atlas {tuple(texture.atlas.shape)} is not the layout of "
                                 f"{caster.F} faces with {texture.texels} texels")
            atlas, layout = texture.atlas.contiguous(), (texture.texels, cols, rows)
    pose, rays, _ = _render_args(pose, rays, K, hw, near, far, 1.0, 1.0, dev)
    h, w = int(rays.shape[0]), int(rays.shape[1])
    with torch.cuda.device(dev):
        rng, nrm, hit, fc, _ = caster.cast(rays, h, w, pose, near, far, face=True)
        rgb = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        if texture is not None and texture.sized:
            _m.check(_m.lib().mslam_mesh_shade_sized(_m.ptr(fc), _m.ptr(rays), h, w, _m.ptr(pose), _m.ptr(caster.v),
                                                     _m.ptr(caster.f), caster.F, caster.V, _m.ptr(atlas),
                                                     _m.ptr(face_cell), *layout, _m.ptr(rgb), _m.stream_ptr()),
                     "mesh_shade_sized")
            return rng.view(h, w), nrm.view(h, w, 3), hit.view(h, w).bool(), rgb
        _m.check(_m.lib().mslam_mesh_shade(_m.ptr(fc), _m.ptr(rays), h, w, _m.ptr(pose), _m.ptr(caster.v),
                                           _m.ptr(caster.f), caster.F, caster.V, _m.ptr(colors), _m.ptr(atlas), *layout,
                                           _m.ptr(rgb), _m.stream_ptr()), "mesh_shade")
    return rng.view(h, w), nrm.view(h, w, 3), hit.view(h, w).bool(), rgb
