"""What the GPU tests of the mesh, TSDF-mesh, render and colour group share: the kernels' tile constants, the fused
room, host copies and byte comparisons, the raw C entry points of the plain distance and cast, and guarded operands.
A plain module like kernel_refs.py (whose Guarded and check_guards it uses); no test module of the group imports from
another."""
import itertools

import numpy as np
import torch

import meshindex_numpy
import render_numpy
from kernel_refs import Guarded, check_guards
from mast3r_slam import synthetic

T = 128            # kMdTile of csrc/mesh_tri.h: triangles per LDS tile and per box
G = 32             # kMdGroup: tiles per group box of a mesh index
BLOCK = 256        # kMdBlock: points or rays per block
VS = 0.03          # voxel size of the test volumes
NEAR, FAR = 0.05, 10.0
CAST_KEYS = ("range", "normal", "hit", "face", "t64")


def _dev(device, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(device)


def _host(tensors):
    return tuple(a.cpu().numpy() for a in tensors)


def _same(a, b):
    for x, y in zip(_host(a), _host(b)):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)


def _same_bytes(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def _vol(device, capacity=1 << 20, **kw):
    from mast3r_slam.tsdf import TSDFVolume

    return TSDFVolume(VS, 0.12, 100.0, 1.0e-3, capacity=capacity, device=device, **kw)


def _room(n_kf=3, n_pts=20000, h=192, w=256):
    out = []
    for kf in range(n_kf):
        T_wc = synthetic.camera_pose(kf * 10)
        X = synthetic.render_pointmap(T_wc, h, w).reshape(-1, 3)
        rng = np.random.default_rng(kf)
        sel = rng.permutation(X.shape[0])[:n_pts]
        out.append((synthetic.sim3_act(T_wc, X[sel]).astype(np.float32), rng.uniform(0.1, 8.0, len(sel)),
                    T_wc[:3].astype(np.float32)))
    return out


def _rays(h, w):
    return render_numpy.unit_rays(h, w, synthetic.intrinsics(h, w))


def _pose(t, rotvec, s=1.0):
    return np.concatenate((t, synthetic.quat_from_rotvec(np.asarray(rotvec, np.float64)), [s])).astype(np.float32)


# a pose off the trajectory with a generic rotation and a scale, one of the trajectory that was not fused, one outside
# the room looking away
POSES = {
    "generic": _pose(synthetic.camera_pose(12)[:3] + [0.1, -0.05, 0.08], [0.2, 0.3, 0.25], 1.25),
    "unfused": synthetic.camera_pose(15).astype(np.float32),
    "outside": _pose([0.0, 0.0, 5.0], [0.0, 0.0, 0.0]),
}


def color_checks(rgb, hit, truth, full_image, label):
    """Checks (a) and (b) of the colour view: `rgb` f[h,w,3] the rendered colours, `truth` f[h,w,3] the texture at the hit
    points, `full_image` f[h,w,3] the texture image of the whole frame (for the mirror images).  Returns (max, mean)
    absolute error over the hit pixels."""
    err = np.abs(rgb - truth)[hit]
    mean = float(err.mean())
    const = float(np.abs(truth[hit] - truth[hit].mean(0, keepdims=True)).mean())   # the best constant image
    print(f"{label}: {int(hit.sum())} hit pixels, max error {err.max():.4f}, mean error {mean:.5f}, best constant image "
          f"{const:.4f} (per channel {np.abs(truth[hit] - truth[hit].mean(0)).mean(0).round(3).tolist()})")
    assert mean < const, (mean, const)
    for p in itertools.permutations(range(3)):
        if p != (0, 1, 2):
            other = float(np.abs(rgb - truth[..., list(p)])[hit].mean())
            assert mean < other, ("channel permutation", p, mean, other)
    for name, img in (("left-right", full_image[:, ::-1]), ("up-down", full_image[::-1])):
        other = float(np.abs(rgb - img)[hit].mean())
        assert mean < other, (name, mean, other)
    return float(err.max()), mean


class Operands:
    """Device copies of the inputs and the outputs of one call, each inside a guarded allocation (kernel_refs.Guarded)."""

    def __init__(self, device):
        self.device, self.all, self.outputs = device, {}, []

    def _add(self, g, output):
        name = str(len(self.all))
        self.all[name] = g
        if output and g.n:
            self.outputs.append(name)
        return g.t

    def put(self, a, dtype):
        a = np.ascontiguousarray(a, dtype)
        return self._add(Guarded(self.device, torch.from_numpy(a).dtype, src=torch.from_numpy(a)), False)

    def out(self, dtype, shape):
        return self._add(Guarded(self.device, dtype, shape), True)

    def check(self):
        """Every guard is intact and every output is written in full."""
        check_guards(self.all, self.outputs, "operands")


def _raw_distance(device, P, V, F, skip):
    """mslam_mesh_distance through the C entry point -> (dist2, nearest, share of (wave, tile) scans skipped)."""
    import mslam_hip as _m

    L = _m.lib()
    p, v, f = _dev(device, P, np.float32), _dev(device, V, np.float32), _dev(device, F, np.int32)
    n, nf = len(P), len(F)
    d2 = torch.empty(n, dtype=torch.float64, device=device)
    nearest = torch.empty(n, dtype=torch.int32, device=device)
    nblk = (n + BLOCK - 1) // BLOCK
    box = int(L.mslam_mesh_distance_workspace_bytes(nf))
    assert box == 48 * ((nf + T - 1) // T)
    ws = torch.zeros(box + 16 * nblk, dtype=torch.uint8, device=device) if skip else None
    _m.check(L.mslam_mesh_distance(_m.ptr(p), n, _m.ptr(v), _m.ptr(f), nf, len(V), 2 if skip else 0, _m.ptr(ws),
                                   ws.numel() if skip else 0, _m.ptr(d2), _m.ptr(nearest), _m.stream_ptr()),
             "mesh_distance")
    share = 0.0
    if skip and nf:
        waves = (n + 63) // 64                    # the waves that hold a point
        counts = ws[box:].view(torch.int32).cpu().numpy().reshape(nblk, 4).reshape(-1)[:waves]
        share = float(counts.sum()) / (waves * ((nf + T - 1) // T))
    return d2.cpu().numpy(), nearest.cpu().numpy(), share


def _raw_cast(device, rays, h, w, pose, V, F, skip, near=NEAR, far=FAR, face=True, t64=True, guarded=False):
    """mslam_mesh_raycast_boxes + mslam_mesh_raycast through the C entry points -> dict of numpy arrays."""
    import mslam_hip as _m

    L, st = _m.lib(), _m.stream_ptr()
    r, p = _dev(device, np.reshape(rays, (-1, 3)), np.float32), _dev(device, pose, np.float32)
    v, f = _dev(device, np.reshape(V, (-1, 3)), np.float32), _dev(device, np.reshape(F, (-1, 3)), np.int32)
    n, nf = h * w, len(f)
    assert len(r) == n
    wb = int(L.mslam_mesh_raycast_workspace_bytes(nf))
    assert wb == 48 * ((nf + T - 1) // T)
    ws = None
    if skip and nf:
        ws = torch.empty(wb, dtype=torch.uint8, device=device)
        _m.check(L.mslam_mesh_raycast_boxes(_m.ptr(v), _m.ptr(f), nf, len(v), _m.ptr(ws), wb, st), "mesh_raycast_boxes")
    shapes = dict(range=(torch.float32, (n,)), normal=(torch.float32, (n, 3)), hit=(torch.uint8, (n,)),
                  face=(torch.int32, (n,)), t64=(torch.float64, (n,)))
    out = {k: Guarded(device, *shapes[k]) for k in CAST_KEYS if (k != "face" or face) and (k != "t64" or t64)}
    arg = lambda k: _m.ptr(out[k].t) if k in out else 0
    ws_before = ws.clone() if ws is not None else None
    _m.check(L.mslam_mesh_raycast(_m.ptr(r), h, w, _m.ptr(p), _m.ptr(v), _m.ptr(f), nf, len(v), near, far,
                                  1 if skip else 0, _m.ptr(ws), wb if ws is not None else 0, arg("range"),
                                  arg("normal"), arg("hit"), arg("face"), arg("t64"), st), "mesh_raycast")
    if guarded:
        check_guards(out, list(out), "mesh_raycast")
        assert ws is None or torch.equal(ws, ws_before)                  # the cast only reads the boxes
    return {k: g.t.cpu().numpy() for k, g in out.items()}


def _build(device, V, F, order=None):
    """mslam_mesh_index_keys, a stable torch.sort and mslam_mesh_index_boxes through the C entry points -> dict with
    the device operands (v, f, order, ws) and numpy copies of keys, order, tile and group boxes.  `order`: put this one
    in the place of the sorted one."""
    import mslam_hip as _m

    L, st = _m.lib(), _m.stream_ptr()
    ops = Operands(device)
    V, F = np.reshape(V, (-1, 3)), np.reshape(F, (-1, 3))
    nv, nf = len(V), len(F)
    v, f = ops.put(V, np.float32), ops.put(F, np.int32)
    bnd = ops.put(meshindex_numpy.bounds(V), np.float32)
    if nv:
        assert torch.equal(bnd, torch.cat((v.amin(0), v.amax(0))))
    keys = ops.out(torch.int64, (nf,))
    _m.check(L.mslam_mesh_index_keys(_m.ptr(v), nv, _m.ptr(f), nf, _m.ptr(bnd), _m.ptr(keys), st), "mesh_index_keys")
    srt = torch.sort(keys, stable=True)[1].to(torch.int32).cpu().numpy() if order is None else order
    o = ops.put(srt, np.int32)
    ntiles = (nf + T - 1) // T
    ngroups = (ntiles + G - 1) // G
    need = int(L.mslam_mesh_index_bytes(nf))
    assert need == 48 * (ntiles + ngroups)
    ws = ops.out(torch.float64, (need // 8,)).view(torch.uint8)
    _m.check(L.mslam_mesh_index_boxes(_m.ptr(v), _m.ptr(f), nf, nv, _m.ptr(o), _m.ptr(ws), ws.numel(), st),
             "mesh_index_boxes")
    ops.check()
    box = ws[:need].cpu().numpy().view(np.float64).reshape(-1, 6)
    return dict(ops=ops, V=V, F=F, v=v, f=f, nv=nv, nf=nf, o=o, ws=ws, bnd=bnd, keys=keys.cpu().numpy(), order=srt,
                tile=box[:ntiles], group=box[ntiles:])


def _indexed_cast(device, ix, rays, h, w, pose, levels, near, far):
    """mslam_mesh_raycast_indexed over the index `ix` of _build -> (dict of numpy arrays as _raw_cast, the per-wave skip
    counts i32[4 * blocks]); guards checked."""
    import mslam_hip as _m

    L = _m.lib()
    ops = Operands(device)
    n = h * w
    r, p = ops.put(np.reshape(rays, (-1, 3)), np.float32), ops.put(pose, np.float32)
    shapes = dict(range=(torch.float32, (n,)), normal=(torch.float32, (n, 3)), hit=(torch.uint8, (n,)),
                  face=(torch.int32, (n,)), t64=(torch.float64, (n,)))
    out = {k: ops.out(*shapes[k]) for k in CAST_KEYS}
    blocks = int(L.mslam_mesh_raycast_blocks(h, w))
    assert blocks == ((n + BLOCK - 1) // BLOCK if h == 1 else ((w + 15) // 16) * ((h + 15) // 16))
    counts = ops.out(torch.int32, (4 * blocks,))
    _m.check(L.mslam_mesh_raycast_indexed(_m.ptr(r), h, w, _m.ptr(p), _m.ptr(ix["v"]), _m.ptr(ix["f"]), ix["nf"],
                                          ix["nv"], near, far, _m.ptr(ix["o"]), _m.ptr(ix["ws"]), ix["ws"].numel(),
                                          levels, _m.ptr(counts), *(_m.ptr(out[k]) for k in CAST_KEYS),
                                          _m.stream_ptr()), "mesh_raycast_indexed")
    ops.check()
    ix["ops"].check()
    return {k: t.cpu().numpy() for k, t in out.items()}, counts.cpu()
