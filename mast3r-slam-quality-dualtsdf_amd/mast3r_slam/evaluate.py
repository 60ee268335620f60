"""Mirror of the reference's output writers, mast3r_slam/evaluate.py: TUM-format trajectory, coloured
point cloud (binary little-endian PLY, with or without the quality attributes) and keyframe images — the formats the
reference's `scripts/eval_*.sh` / `evo_ape` consume.  Same function names and arguments.

The reference writes PLY through `plyfile` and images / grid upsampling through `cv2`; neither is installed here, so
* `save_ply*` emit the file `plyfile`'s `PlyData([PlyElement.describe(arr, "vertex")], text=False)` is documented to
  produce (header lines + packed records) — byte parity with plyfile itself is **unpinned**;
* `save_keyframes` writes PNG through PIL (same RGB content; cv2's BGR swap is its own file convention);
* the quality grids are upsampled with cv2.resize's published INTER_LINEAR / INTER_NEAREST sampling rules — **unpinned**.
`save_traj` is pinned against the reference function (tests/golden/evaluate_traj.npz)."""
import pathlib

import numpy as np
import torch

from mast3r_slam.config import config
from mast3r_slam.geometry import constrain_points_to_ray
from mast3r_slam.lietorch_utils import as_SE3


def prepare_savedir(args, dataset):
    """evaluate.py:14-20."""
    save_dir = pathlib.Path("logs")
    if args.save_as != "default":
        save_dir = save_dir / args.save_as
    save_dir.mkdir(exist_ok=True, parents=True)
    seq_name = dataset.dataset_path.stem
    return save_dir, seq_name


def save_traj(logdir, logfile, timestamps, frames, intrinsics=None):
    """evaluate.py:23-45: one line per keyframe, `t x y z qx qy qz qw` (python float repr of the float32 values)."""
    logdir = pathlib.Path(logdir)
    logdir.mkdir(exist_ok=True, parents=True)
    logfile = logdir / logfile
    with open(logfile, "w") as f:
        for i in range(len(frames)):
            keyframe = frames[i]
            t = timestamps[keyframe.frame_id]
            if intrinsics is None:
                T_WC = as_SE3(keyframe.T_WC)
            else:
                T_WC = intrinsics.refine_pose_with_calibration(keyframe)
            x, y, z, qx, qy, qz, qw = T_WC.data.cpu().numpy().reshape(-1)
            f.write(f"{t} {x} {y} {z} {qx} {qy} {qz} {qw}\n")


def _world_points(keyframe):
    if config["use_calib"]:
        X_canon = constrain_points_to_ray(keyframe.img_shape.flatten()[:2], keyframe.X_canon[None], keyframe.K)
        keyframe.X_canon = X_canon.squeeze(0)
    pW = keyframe.T_WC.act(keyframe.X_canon).cpu().numpy().reshape(-1, 3)
    color = (keyframe.uimg.cpu().numpy() * 255).astype(np.uint8).reshape(-1, 3)
    return pW, color


def save_reconstruction(savedir, filename, keyframes, c_conf_threshold):
    """evaluate.py:48-71."""
    savedir = pathlib.Path(savedir)
    savedir.mkdir(exist_ok=True, parents=True)
    pointclouds, colors = [], []
    for i in range(len(keyframes)):
        keyframe = keyframes[i]
        pW, color = _world_points(keyframe)
        valid = keyframe.get_average_conf().cpu().numpy().astype(np.float32).reshape(-1) > c_conf_threshold
        pointclouds.append(pW[valid])
        colors.append(color[valid])
    save_ply(savedir / filename, np.concatenate(pointclouds, axis=0), np.concatenate(colors, axis=0))


def save_keyframes(savedir, timestamps, keyframes):
    """evaluate.py:74-87 (PIL instead of cv2.imwrite)."""
    import PIL.Image

    savedir = pathlib.Path(savedir)
    savedir.mkdir(exist_ok=True, parents=True)
    for i in range(len(keyframes)):
        keyframe = keyframes[i]
        t = timestamps[keyframe.frame_id]
        PIL.Image.fromarray((keyframe.uimg.cpu().numpy() * 255).astype(np.uint8)).save(str(savedir / f"{t}.png"))


_PLY_TYPES = {"f4": "float", "u1": "uchar", "f8": "double", "i4": "int", "u4": "uint", "i2": "short", "u2": "ushort", "i1": "char"}


def _write_ply(filename, pcd):
    """Binary little-endian PLY with one `vertex` element described by the structured array `pcd`."""
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(pcd)}"]
    for name in pcd.dtype.names:
        header.append(f"property {_PLY_TYPES[pcd.dtype[name].str[1:]]} {name}")
    header.append("end_header")
    with open(filename, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(pcd.astype(pcd.dtype.newbyteorder("<")).tobytes())


def save_ply(filename, points, colors):
    """evaluate.py:90-106."""
    colors = colors.astype(np.uint8)
    pcd = np.empty(len(points), dtype=[("x", "f4"), ("y", "f4"), ("z", "f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    pcd["x"], pcd["y"], pcd["z"] = points.T
    pcd["red"], pcd["green"], pcd["blue"] = colors.T
    _write_ply(filename, pcd)


def save_cloud(filename, points, colors=None, normals=None):
    """A point cloud (SlamSystem.keyframe_cloud's tensors, or numpy arrays) as binary little-endian PLY: x, y, z float
    [, nx, ny, nz float][, red, green, blue uchar] per vertex, the layout load_ply_points reads."""
    host = lambda a, dtype: np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype)
    points = host(points, np.float32).reshape(-1, 3)
    fields = [("x", "f4"), ("y", "f4"), ("z", "f4")]
    if normals is not None:
        normals = host(normals, np.float32).reshape(-1, 3)
        fields += [("nx", "f4"), ("ny", "f4"), ("nz", "f4")]
    if colors is not None:
        colors = host(colors, np.uint8).reshape(-1, 3)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    for name, a in (("normals", normals), ("colors", colors)):
        if a is not None and len(a) != len(points):
            raise ValueError(f"save_cloud: {name} must be ({len(points)},3), got {a.shape}")
    pcd = np.empty(len(points), dtype=fields)
    pcd["x"], pcd["y"], pcd["z"] = points.T
    if normals is not None:
        pcd["nx"], pcd["ny"], pcd["nz"] = normals.T
    if colors is not None:
        pcd["red"], pcd["green"], pcd["blue"] = colors.T
    _write_ply(filename, pcd)


def save_mesh(filename, vertices, faces, normals=None, colors=None):
    """Triangle mesh as binary little-endian PLY: `element vertex` (x, y, z [, nx, ny, nz] float [, red, green, blue]
    uchar = rint(255 c) of `colors` in [0, 1]) and `element face` (`property list uchar int vertex_indices`).  Arrays may
    be numpy or device tensors."""
    def host(a, dtype):
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        return a.astype(dtype).reshape(-1, 3)

    v = host(vertices, np.float32)
    f = host(faces, np.int32)
    cols = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        cols += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    n_float = len(cols)
    if colors is not None:
        cols += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vert = np.empty(len(v), dtype=cols)
    vert["x"], vert["y"], vert["z"] = v.T
    if normals is not None:
        n = host(normals, np.float32)
        vert["nx"], vert["ny"], vert["nz"] = n.T
    if colors is not None:
        c = np.clip(np.rint(255.0 * host(colors, np.float64)), 0, 255).astype(np.uint8)
        if len(c) != len(v):
            raise ValueError(f"save_mesh: {len(c)} colours for {len(v)} vertices")
        vert["red"], vert["green"], vert["blue"] = c.T
    face = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    face["n"], face["i"] = 3, f
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    header += [f"property float {name}" for name, _ in cols[:n_float]]
    header += [f"property uchar {name}" for name, _ in cols[n_float:]]
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(filename, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())


_PLY_SIZES = {"char": 1, "uchar": 1, "int8": 1, "uint8": 1, "short": 2, "ushort": 2, "int16": 2, "uint16": 2, "int": 4,
              "uint": 4, "int32": 4, "uint32": 4, "float": 4, "float32": 4, "double": 8, "float64": 8}


def load_mesh(filename):
    """Reads a triangle mesh from the binary little-endian PLY that save_mesh writes -> (vertices f32[V,3], faces
    i32[F,3]) numpy.  The vertex element needs float x, y, z; its other properties are skipped by their declared sizes.
    The face element is one `property list uchar int|uint` of three indices per face.  ASCII or big-endian files, list
    properties on vertices and faces that are no triangles raise ValueError."""
    with open(filename, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"load_mesh: {filename} is not a PLY file")
    lines = data[:end].decode("ascii", "replace").split("\n")
    body = end + len(b"end_header\n")
    if not any(ln.split() == ["format", "binary_little_endian", "1.0"] for ln in lines):
        raise ValueError(f"load_mesh: {filename} is not binary_little_endian 1.0 (ASCII and big-endian are not read)")
    elements = []                                        # [name, count, [property words]]
    for ln in lines:
        w = ln.split()
        if w[:1] == ["element"]:
            elements.append([w[1], int(w[2]), []])
        elif w[:1] == ["property"]:
            if not elements:
                raise ValueError("load_mesh: property before any element")
            elements[-1][2].append(w[1:])
    if [e[0] for e in elements[:2]] != ["vertex", "face"]:
        raise ValueError("load_mesh: expected a vertex element followed by a face element")
    (_, n_v, vprops), (_, n_f, fprops) = elements[:2]
    fields = []
    for w in vprops:
        if w[0] == "list" or w[0] not in _PLY_SIZES:
            raise ValueError(f"load_mesh: unsupported vertex property '{' '.join(w)}'")
        is_xyz = w[1] in ("x", "y", "z")
        if is_xyz and w[0] not in ("float", "float32"):
            raise ValueError(f"load_mesh: vertex {w[1]} must be float, got {w[0]}")
        fields.append((w[1], "<f4" if is_xyz else f"V{_PLY_SIZES[w[0]]}"))
    if not {"x", "y", "z"} <= {name for name, _ in fields}:
        raise ValueError("load_mesh: the vertex element has no float x, y, z")
    if len(fprops) != 1 or fprops[0][:2] != ["list", "uchar"] or fprops[0][2] not in ("int", "uint", "int32", "uint32"):
        raise ValueError("load_mesh: the face element must be one `property list uchar int|uint`")
    vdt = np.dtype(fields)
    fdt = np.dtype([("n", "u1"), ("i", "<u4" if fprops[0][2].startswith("u") else "<i4", (3,))])
    if len(data) < body + n_v * vdt.itemsize:
        raise ValueError("load_mesh: the file ends inside the vertex element")
    vert = np.frombuffer(data, vdt, n_v, body)
    body += n_v * vdt.itemsize
    counts = np.frombuffer(data, "u1", len(data) - body, body)[::fdt.itemsize][:n_f]
    if len(data) < body + n_f * fdt.itemsize or (counts != 3).any():
        raise ValueError("load_mesh: only triangle faces are read")
    face = np.frombuffer(data, fdt, n_f, body)
    vertices = np.stack([vert["x"], vert["y"], vert["z"]], 1).astype(np.float32).reshape(-1, 3)
    return vertices, face["i"].astype(np.int32).reshape(-1, 3)


def load_ply_points(filename):
    """Reads the points of a binary little-endian PLY with a vertex element - what save_ply and save_mesh write, or a
    laser scan - with or without faces -> (points f32[N,3], colors u8[N,3] or None) numpy.  The vertex element must
    come first and needs float x, y, z; `colors` are its uchar red, green, blue when all three are present; its other
    properties are skipped by their declared sizes, and every element after it is left unread.  With load_mesh's
    refusals: files that are no PLY, ASCII or big-endian files, list properties on vertices, x, y, z of another type,
    and files that end inside the vertex element raise ValueError."""
    what = "load_ply_points"
    with open(filename, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{what}: {filename} is not a PLY file")
    lines = data[:end].decode("ascii", "replace").split("\n")
    body = end + len(b"end_header\n")
    if not any(ln.split() == ["format", "binary_little_endian", "1.0"] for ln in lines):
        raise ValueError(f"{what}: {filename} is not binary_little_endian 1.0 (ASCII and big-endian are not read)")
    elements = []                                        # [name, count, [property words]]
    for ln in lines:
        w = ln.split()
        if w[:1] == ["element"]:
            elements.append([w[1], int(w[2]), []])
        elif w[:1] == ["property"]:
            if not elements:
                raise ValueError(f"{what}: property before any element")
            elements[-1][2].append(w[1:])
    if not elements or elements[0][0] != "vertex":
        raise ValueError(f"{what}: expected a vertex element first")
    _, n_v, vprops = elements[0]
    fields = []
    for w in vprops:
        if w[0] == "list" or w[0] not in _PLY_SIZES:
            raise ValueError(f"{what}: unsupported vertex property '{' '.join(w)}'")
        is_xyz = w[1] in ("x", "y", "z")
        if is_xyz and w[0] not in ("float", "float32"):
            raise ValueError(f"{what}: vertex {w[1]} must be float, got {w[0]}")
        is_rgb = w[1] in ("red", "green", "blue") and w[0] in ("uchar", "uint8")
        fields.append((w[1], "<f4" if is_xyz else "u1" if is_rgb else f"V{_PLY_SIZES[w[0]]}"))
    if not {"x", "y", "z"} <= {name for name, _ in fields}:
        raise ValueError(f"{what}: the vertex element has no float x, y, z")
    vdt = np.dtype(fields)
    if len(data) < body + n_v * vdt.itemsize:
        raise ValueError(f"{what}: the file ends inside the vertex element")
    vert = np.frombuffer(data, vdt, n_v, body)
    points = np.stack([vert["x"], vert["y"], vert["z"]], 1).astype(np.float32).reshape(-1, 3)
    colors = None
    if all(vdt.fields.get(c, (None,))[0] == np.dtype("u1") for c in ("red", "green", "blue")):
        colors = np.stack([vert["red"], vert["green"], vert["blue"]], 1).astype(np.uint8).reshape(-1, 3)
    return points, colors


def save_cloud_metrics(savedir, filename, metrics):
    """The dict of tsdf.compare_clouds / SlamSystem.evaluate_cloud as JSON with sorted keys, in the form of
    save_mesh_metrics.  Returns the path."""
    return save_mesh_metrics(savedir, filename, metrics)


def save_plane_metrics(savedir, filename, figures):
    """The dict of tsdf.plane_figures / SlamSystem.evaluate_planarity as JSON with sorted keys, in the form of
    save_mesh_metrics.  Returns the path."""
    return save_mesh_metrics(savedir, filename, figures)


def trajectory_ate(est_xyz, gt_xyz, with_scale=True, device="cuda:0"):
    """Absolute trajectory error of the positions est_xyz (K x 3) against gt_xyz (K x 3), numpy arrays or tensors, after
    the best similarity (tsdf.fit_sim3 on `device`; `with_scale=False`: the best rigid motion) -> (rmse, T): the root
    mean square of |T(est_k) - gt_k| in f64 as a Python float and T as numpy f64[8] [t(3), q(xyzw), s]."""
    from mast3r_slam.tsdf import fit_sim3, transform_mesh

    est = torch.as_tensor(est_xyz, dtype=torch.float32).to(device).reshape(-1, 3)
    gt = torch.as_tensor(gt_xyz, dtype=torch.float32).to(device).reshape(-1, 3)
    T = fit_sim3(est, gt, with_scale=with_scale)[0]
    r = transform_mesh(est.double(), T) - gt.double()
    return float(torch.sqrt((r * r).sum(1).mean())), T.cpu().numpy()


def save_mesh_metrics(savedir, filename, metrics):
    """The dict of tsdf.compare_meshes / SlamSystem.evaluate_mesh as JSON with sorted keys.  Returns the path."""
    import json

    savedir = pathlib.Path(savedir)
    savedir.mkdir(exist_ok=True, parents=True)
    path = savedir / filename
    with open(path, "w") as f:
        json.dump(dict(metrics), f, indent=1, sort_keys=True)
        f.write("\n")
    return path


def save_render_metrics(savedir, filename, metrics):
    """The dict of SlamSystem.evaluate_render (psnr, ssim, shares, per_view lists) as JSON with sorted keys, in the form
    of save_mesh_metrics; a NaN or an infinity is written as Python's json writes it (NaN, Infinity).  Returns the
    path."""
    return save_mesh_metrics(savedir, filename, metrics)


def save_tsdf_mesh(savedir, filename, source, min_weight=None, level=0.0, colors=False, **chain):
    """The global TSDF's triangle mesh (marching cubes) as PLY with normals, beside save_reconstruction's point cloud.
    `source`: a SlamSystem, a TSDFGlobalManager or a TSDFVolume.  `colors=True` (a volume with tsdf_global.color): the
    vertices carry the fused colour as red / green / blue.  `chain`: the options of the export chain
    (tsdf/mesh_chain.py); an option that is off is not handed on.  Returns (V, F)."""
    from mast3r_slam.tsdf.mesh_chain import chain_options

    kw = chain_options(chain, "save_tsdf_mesh")
    savedir = pathlib.Path(savedir)
    savedir.mkdir(exist_ok=True, parents=True)
    if colors:
        v, n, f, c = source.extract_mesh(min_weight=min_weight, level=level, colors=True, **kw)
        save_mesh(savedir / filename, v, f, normals=n, colors=c)
    else:
        v, n, f = source.extract_mesh(min_weight=min_weight, level=level, **kw)
        save_mesh(savedir / filename, v, f, normals=n)
    return int(v.shape[0]), int(f.shape[0])


def save_color_view(savedir, filename, rgb, hit):
    """A rendered colour view (TSDFVolume.render(colors=True)[3], in [0, 1]) as 8-bit RGB PNG, rint(255 c), black on a
    miss.  Arrays may be numpy or device tensors.  Returns the path."""
    from PIL import Image

    def host(a):
        return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)

    savedir = pathlib.Path(savedir)
    savedir.mkdir(exist_ok=True, parents=True)
    m = host(hit).astype(bool)
    c = host(rgb).astype(np.float64)
    if c.shape != m.shape + (3,):
        raise ValueError(f"save_color_view: rgb {c.shape} does not match hit {m.shape}")
    img = np.where(m[..., None], np.clip(np.rint(255.0 * c), 0, 255), 0).astype(np.uint8)
    path = savedir / filename
    Image.fromarray(img).save(path)
    return path


def save_textured_mesh(savedir, stem, vertices, faces, texture, normals=None):
    """A textured mesh (tsdf.bake_texture's MeshTexture) as three files: `<stem>.obj` - `v` with %.9g, `vn` with
    `normals`, three `vt` per face (corner k of face f is entry 3 f + k + 1) and `f a/ta[/na]`; `<stem>.mtl` - one
    material whose map_Kd is `<stem>.png`; `<stem>.png` - the atlas as 8-bit RGB, rint(255 c), written as save_color_view
    writes.  The atlas coordinates (x, y) of texture.uv(), texel centres at integers, become
    vt = ((x + 0.5) / W, 1 - (y + 0.5) / H).  Arrays may be numpy or device tensors.  Returns the three paths."""
    from PIL import Image

    def host(a, dtype):
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        return a.astype(dtype)

    savedir = pathlib.Path(savedir)
    savedir.mkdir(exist_ok=True, parents=True)
    v, f = host(vertices, np.float32).reshape(-1, 3), host(faces, np.int64).reshape(-1, 3)
    atlas = host(texture.atlas, np.float64)
    H, W = atlas.shape[:2]
    if H * W == 0:
        raise ValueError("save_textured_mesh: the texture's atlas is empty (a mesh without faces)")
    uv = host(texture.uv(), np.float64).reshape(-1, 2)
    if len(uv) != 3 * len(f):
        raise ValueError(f"save_textured_mesh: the texture holds {len(uv) // 3} faces, the mesh {len(f)}")
    n = None if normals is None else host(normals, np.float32).reshape(-1, 3)
    if n is not None and len(n) != len(v):
        raise ValueError(f"save_textured_mesh: {len(n)} normals for {len(v)} vertices")
    obj, mtl, png = (savedir / f"{stem}.{ext}" for ext in ("obj", "mtl", "png"))
    lines = [f"mtllib {stem}.mtl", "usemtl atlas"]
    lines += ["v %.9g %.9g %.9g" % tuple(float(c) for c in p) for p in v]
    if n is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(float(c) for c in p) for p in n]
    lines += ["vt %.9g %.9g" % ((x + 0.5) / W, 1.0 - (y + 0.5) / H) for x, y in uv]
    for k, (a, b, c) in enumerate(f + 1):
        t = 3 * k + 1
        lines.append(f"f {a}/{t}/{a} {b}/{t + 1}/{b} {c}/{t + 2}/{c}" if n is not None else
                     f"f {a}/{t} {b}/{t + 1} {c}/{t + 2}")
    with open(obj, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    with open(mtl, "w") as fh:
        fh.write(f"newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {stem}.png\n")
    Image.fromarray(np.clip(np.rint(255.0 * atlas), 0, 255).astype(np.uint8).reshape(H, W, 3)).save(png)
    return obj, mtl, png


def save_depth_view(savedir, filename, range_or_depth, normals, hit, pose=None):
    """A rendered view (TSDFVolume.render) as two images beside `filename`'s stem: `<stem>_depth.png`, 16-bit grey,
    the given range or depth in millimetres (rounded, clipped to 65535; 0 = miss), and `<stem>_normal.png`, 8-bit RGB of
    0.5 * (n_cam + 1) (0 on a miss).  `normals` are camera-frame, or world-frame (as render returns them) together with
    the view's `pose` (8,) [t, q, s], whose rotation is then undone.  Arrays may be numpy or device tensors.  Returns the
    two paths."""
    from PIL import Image

    def host(a):
        return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)

    savedir = pathlib.Path(savedir)
    savedir.mkdir(exist_ok=True, parents=True)
    stem = pathlib.Path(filename).stem
    m = host(hit).astype(bool)
    d = np.where(m, host(range_or_depth).astype(np.float64), 0.0)
    mm = np.clip(np.rint(d * 1000.0), 0, 65535).astype(np.uint16)
    n = host(normals).astype(np.float64)
    if pose is not None:          # n_cam = R^T n_world: rotate with the conjugate quaternion
        q = host(getattr(pose, "data", pose)).astype(np.float64).reshape(8)[3:7]
        qv, qw = -q[:3], q[3]
        u = 2.0 * np.cross(qv, n)
        n = n + qw * u + np.cross(qv, u)
    n = np.where(m[..., None], 0.5 * (n + 1.0), 0.0)
    rgb = np.clip(np.rint(n * 255.0), 0, 255).astype(np.uint8)
    depth_path, normal_path = savedir / f"{stem}_depth.png", savedir / f"{stem}_normal.png"
    Image.fromarray(mm).save(depth_path)          # uint16 array -> mode I;16
    Image.fromarray(rgb).save(normal_path)
    return depth_path, normal_path


def _resize_grid(g, H, W, mode):
    """cv2.resize(g, (W, H), INTER_NEAREST | INTER_LINEAR) for a 2-D float32 grid: nearest takes src = floor(dst * scale),
    linear samples at (dst + 0.5) * scale - 0.5 with the border replicated."""
    gh, gw = g.shape
    sy, sx = gh / H, gw / W
    if mode == "nearest":
        iy = np.minimum(np.floor(np.arange(H) * sy).astype(np.int64), gh - 1)
        ix = np.minimum(np.floor(np.arange(W) * sx).astype(np.int64), gw - 1)
        return g[iy][:, ix]
    fy = (np.arange(H, dtype=np.float32) + 0.5) * np.float32(sy) - 0.5
    fx = (np.arange(W, dtype=np.float32) + 0.5) * np.float32(sx) - 0.5
    y0, x0 = np.floor(fy).astype(np.int64), np.floor(fx).astype(np.int64)
    wy, wx = (fy - y0).astype(np.float32), (fx - x0).astype(np.float32)
    y0c, y1c = np.clip(y0, 0, gh - 1), np.clip(y0 + 1, 0, gh - 1)
    x0c, x1c = np.clip(x0, 0, gw - 1), np.clip(x0 + 1, 0, gw - 1)
    top = g[y0c][:, x0c] * (1 - wx) + g[y0c][:, x1c] * wx
    bot = g[y1c][:, x0c] * (1 - wx) + g[y1c][:, x1c] * wx
    return (top * (1 - wy)[:, None] + bot * wy[:, None]).astype(np.float32)


def save_ply_with_quality(savedir, filename, keyframes, c_conf_threshold, quality_service, patch_size=16):
    """evaluate.py:108-186: the reconstruction with the per-patch quality grids (r, delta_cov, u, class_id, priority)
    upsampled to the image and attached to every vertex."""
    savedir = pathlib.Path(savedir)
    savedir.mkdir(exist_ok=True, parents=True)
    cols = {k: [] for k in ("points", "colors", "r", "delta_cov", "u", "class_id", "priority")}
    for i in range(len(keyframes)):
        kf = keyframes[i]
        pW, col = _world_points(kf)
        valid = kf.get_average_conf().cpu().numpy().astype(np.float32).reshape(-1) > c_conf_threshold
        H, W = int(kf.img_shape.flatten()[0]), int(kf.img_shape.flatten()[1])
        res = quality_service.get(kf.frame_id) if quality_service is not None else None
        if res is not None:
            def up(g, mode):
                gnp = g.detach().cpu().numpy() if torch.is_tensor(g) else np.asarray(g)
                return _resize_grid(gnp.astype(np.float32).reshape(gnp.shape[-2], gnp.shape[-1]), H, W, mode).reshape(-1)
            cid = res["class_id"].float() if torch.is_tensor(res["class_id"]) else np.asarray(res["class_id"]).astype(np.float32)
            q = dict(delta_cov=up(res["delta_cov"], "linear"), r=up(res["r"], "linear"), u=up(res["u"], "linear"),
                     class_id=up(cid, "nearest").astype(np.uint8), priority=up(res["priority"], "linear"))
        else:
            n = H * W
            q = dict(delta_cov=np.zeros(n, np.float32), r=np.zeros(n, np.float32), u=np.zeros(n, np.float32),
                     class_id=np.zeros(n, np.uint8), priority=np.zeros(n, np.float32))
        cols["points"].append(pW[valid])
        cols["colors"].append(col[valid])
        for k, v in q.items():
            cols[k].append(v[valid])
    points, colors = np.concatenate(cols["points"], 0), np.concatenate(cols["colors"], 0)
    pcd = np.empty(points.shape[0], dtype=[("x", "f4"), ("y", "f4"), ("z", "f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                                           ("r", "f4"), ("delta_cov", "f4"), ("u", "f4"), ("class_id", "u1"), ("priority", "f4")])
    pcd["x"], pcd["y"], pcd["z"] = points.T
    pcd["red"], pcd["green"], pcd["blue"] = colors.T
    for k in ("r", "delta_cov", "u", "priority"):
        pcd[k] = np.concatenate(cols[k], 0).astype(np.float32)
    pcd["class_id"] = np.concatenate(cols["class_id"], 0).astype(np.uint8)
    _write_ply(savedir / filename, pcd)
