"""CPU tests of the colour outputs: evaluate.save_mesh with vertex colours, evaluate.save_color_view, the colour gather
from a keyframe image that is smaller than the pointmap, and the header / library side of the mslam_tsdf_color_* entry
points."""
import os
import subprocess

import numpy as np
import pytest
import torch

import mslam_hip
from mast3r_slam import evaluate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COLOR_SYMBOLS = ["mslam_tsdf_color_bytes", "mslam_tsdf_color_init", "mslam_tsdf_integrate_color",
                 "mslam_tsdf_color_rehash", "mslam_tsdf_color_dump", "mslam_tsdf_color_load", "mslam_tsdf_color_sample"]

_PLY = {"float": "<f4", "uchar": "u1", "int": "<i4"}


def read_ply(path):
    """Header-driven reader of the meshes save_mesh writes: (vertex structured array, faces i32[F,3], header lines)."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elems, cur = [], None
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            cur = (w[1], int(w[2]), [])
            elems.append(cur)
        elif w[:1] == ["property"] and w[1] != "list":
            cur[2].append((w[2], _PLY[w[1]]))
        elif w[:2] == ["property", "list"]:
            assert w[2:] == ["uchar", "int", "vertex_indices"]
    (vn, nv, vprops), (fn, nf, _) = elems
    assert vn == "vertex" and fn == "face"
    vert = np.frombuffer(raw, dtype=vprops, count=nv, offset=end)
    face = np.frombuffer(raw, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nf, offset=end + vert.nbytes)
    assert end + vert.nbytes + face.nbytes == len(raw) and (face["n"] == 3).all()
    return vert, face["i"], lines


def _mesh(seed=0, nv=50, nf=80):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(nv, 3)).astype(np.float32)
    n = rng.normal(size=(nv, 3)).astype(np.float32)
    f = rng.integers(0, nv, (nf, 3)).astype(np.int32)
    c = rng.uniform(0, 1, (nv, 3)).astype(np.float32)
    c[0], c[1], c[2] = (0.0, 1.0, 0.5), (1.5, -0.5, 127.5 / 255.0), (1.0 / 255.0, 254.6 / 255.0, 0.2)
    return v, n, f, c


@pytest.mark.parametrize("with_normals", [True, False])
def test_save_mesh_with_colors_round_trips(tmp_path, with_normals):
    v, n, f, c = _mesh()
    path = tmp_path / "m.ply"
    evaluate.save_mesh(path, torch.from_numpy(v), f, normals=n if with_normals else None, colors=torch.from_numpy(c))
    vert, faces, lines = read_ply(path)
    names = ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + ["red", "green", "blue"]
    assert list(vert.dtype.names) == names                      # colours after the normals
    assert all(vert.dtype[k] == np.uint8 for k in ("red", "green", "blue"))
    assert np.array_equal(np.stack([vert[k] for k in "xyz"], 1), v) and np.array_equal(faces, f)
    if with_normals:
        assert np.array_equal(np.stack([vert[k] for k in ("nx", "ny", "nz")], 1), n)
    want = np.clip(np.rint(255.0 * c.astype(np.float64)), 0, 255).astype(np.uint8)
    assert np.array_equal(np.stack([vert[k] for k in ("red", "green", "blue")], 1), want)
    assert tuple(want[0]) == (0, 255, 128) and tuple(want[1][:2]) == (255, 0)
    with pytest.raises(ValueError):
        evaluate.save_mesh(path, v, f, colors=c[:-1])


def test_save_mesh_without_colors_is_unchanged(tmp_path):
    """The bytes of the mesh files as they were before vertex colours existed, written out by hand."""
    v, n, f, _ = _mesh(1)
    for normals in (n, None):
        path = tmp_path / "m.ply"
        evaluate.save_mesh(path, v, f, normals=normals)
        props = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals is not None else [])
        header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
        header += [f"property float {p}" for p in props]
        header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
        body = np.concatenate((v, normals), 1) if normals is not None else v
        faces = b"".join(b"\x03" + row.astype("<i4").tobytes() for row in f)
        assert open(path, "rb").read() == ("\n".join(header) + "\n").encode("ascii") + body.astype("<f4").tobytes() + faces
        evaluate.save_mesh(tmp_path / "n.ply", v, f, normals=normals, colors=None)
        assert open(tmp_path / "n.ply", "rb").read() == open(path, "rb").read()


def test_save_color_view(tmp_path):
    from PIL import Image

    rng = np.random.default_rng(2)
    rgb = rng.uniform(0, 1, (9, 13, 3)).astype(np.float32)
    rgb[0, 0] = (1.2, -0.1, 0.5)
    hit = rng.uniform(size=(9, 13)) > 0.4
    hit[0, 0] = True
    path = evaluate.save_color_view(tmp_path / "views", "c.png", torch.from_numpy(rgb), torch.from_numpy(hit))
    img = Image.open(path)
    assert img.mode == "RGB"
    a = np.asarray(img)
    assert a.shape == (9, 13, 3) and a.dtype == np.uint8
    assert not a[~hit].any()                                   # black on a miss
    want = np.clip(np.rint(255.0 * rgb.astype(np.float64)), 0, 255).astype(np.uint8)
    assert np.array_equal(a[hit], want[hit]) and tuple(a[0, 0]) == (255, 0, 128)
    with pytest.raises(ValueError):
        evaluate.save_color_view(tmp_path, "d.png", rgb[:, :5], hit)


def test_gather_uimg_scales_rows_and_columns():
    """create_frame subsamples uimg when dataset.img_downsample > 1: the pointmap pixel (r, c) of an (H, W) map reads
    uimg[r * h // H, c * w // W]."""
    from mast3r_slam.tsdf.global_manager import gather_uimg

    H, W = 12, 20
    g = torch.Generator().manual_seed(0)
    full = torch.rand(H, W, 3, generator=g)
    choice = torch.randperm(H * W, generator=g)[:150]
    assert torch.equal(gather_uimg(full, choice, (H, W)), full.reshape(-1, 3)[choice])
    assert torch.equal(gather_uimg(full, choice, torch.tensor([H, W])), full.reshape(-1, 3)[choice])
    for ds in (2, 3):
        small = full[::ds, ::ds]                                # frame.py: uimg[::ds, ::ds]
        h, w = small.shape[:2]
        r, c = choice // W, choice % W
        got = gather_uimg(small, choice, (H, W))
        assert got.shape == (150, 3) and torch.equal(got, small[r * h // H, c * w // W])
        if H % ds == 0 and W % ds == 0:                         # then that is the subsampled pixel's own source block
            assert torch.equal(got, full[(r // ds) * ds, (c // ds) * ds])


def test_color_config_is_off_by_default():
    from mast3r_slam.config import config

    assert config["tsdf_global"]["color"] is False


def test_header_declares_and_library_exports_color_symbols():
    declared = mslam_hip.exported_symbols()
    for s in COLOR_SYMBOLS:
        assert s in declared, s
    sig = mslam_hip.parse_header(open(os.path.join(ROOT, "include", "mslam_hip.h")).read())
    import ctypes

    vp, u64, i, d, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_double, ctypes.c_size_t
    assert sig["mslam_tsdf_color_bytes"] == (sz, [u64])
    assert sig["mslam_tsdf_integrate_color"] == (i, [vp, u64, vp, vp, vp, vp, vp, i, d, d, d, vp])
    assert sig["mslam_tsdf_color_sample"] == (i, [vp, u64, vp, vp, i, i, d, d, d, d, vp, vp, vp])
    lib = os.path.join(ROOT, "mast3r-slam-quality-dualtsdf_amd", "libmslam_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in COLOR_SYMBOLS:
        assert s in exported, s
    L = mslam_hip.lib()
    assert L.mslam_tsdf_color_bytes(1 << 10) == 32 << 10 and L.mslam_tsdf_color_bytes(1000) == 0
