"""The camera arguments of the view functions, each convention stated once (DESIGN.md "Cameras and views"): poses,
intrinsics, image size and range as every function that renders or projects takes them, and the f64 camera arithmetic
that runs in torch.  global_volume and mesh_raycast re-export the public names.  A pose is a Sim3 [t, q = x y z w, s],
world from camera; pixel centres lie at integers."""
import numpy as np
import torch


def _pose_arg(pose, what, device):
    """f32[8] on `device` from a tensor, an array, a sequence, a (1,8) batch of one or a lietorch Sim3."""
    if isinstance(pose, np.ndarray):
        pose = torch.from_numpy(np.ascontiguousarray(pose))
    pose = getattr(pose, "data", pose)        # a lietorch Sim3 carries its (1,8) tensor in .data
    pose = torch.as_tensor(pose)
    if pose.numel() != 8:
        raise ValueError(f"{what}: pose must hold 8 values [t, q, s], got shape {tuple(pose.shape)}")
    return pose.detach().to(device=device, dtype=torch.float32).reshape(8).contiguous()


def _poses_arg(poses, what):
    """[n,8] on the host, from a tensor, an array or a sequence of Sim3s (lietorch Sim3s included)."""
    if not torch.is_tensor(poses) and not isinstance(poses, np.ndarray):
        poses = [p if isinstance(p, np.ndarray) else getattr(p, "data", p) for p in poses]
        poses = torch.stack([torch.as_tensor(p).detach().reshape(8).to("cpu", torch.float64) for p in poses]) \
            if len(poses) else torch.zeros((0, 8), dtype=torch.float64)
    poses = torch.as_tensor(poses).detach().to("cpu")
    if poses.numel() % 8 != 0:
        raise ValueError(f"{what}: poses must be (n,8) Sim3s [t, q, s], got shape {tuple(poses.shape)}")
    return poses.reshape(-1, 8)


def _K_arg(K, what):
    """(fx, fy, cx, cy) as Python floats of a finite (3,3) pinhole matrix."""
    K = np.asarray(torch.as_tensor(K).detach().cpu(), np.float64)
    if K.shape != (3, 3) or not np.isfinite(K).all():
        raise ValueError(f"{what}: K must be a finite (3,3) pinhole matrix, got shape {K.shape}")
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def _hw_arg(hw, what):
    """(h, w) as ints, both >= 1."""
    if hw is None or len(hw) != 2 or min(int(x) for x in hw) < 1:
        raise ValueError(f"{what}: hw must be (h, w) with h, w >= 1, got {hw!r}")
    return int(hw[0]), int(hw[1])


def _range_arg(near, far, what, strict):
    """(near, far) as floats.  `strict`: far > near with a finite span, what a march needs, which divides by the span;
    otherwise near <= far.  A NaN fails either."""
    near, far = float(near), float(far)
    if strict:
        if not far > near or not np.isfinite(far - near):
            raise ValueError(f"{what}: far must be greater than near, got {near} and {far}")
    elif not near <= far:
        raise ValueError(f"{what}: near must not exceed far, got {near} and {far}")
    return near, far


def _eye(pose):
    """The pose's origin with no rotation and scale 1: the camera of a cast whose rays are world directions already."""
    return torch.cat((pose[:3], pose.new_tensor([0.0, 0.0, 0.0, 1.0, 1.0]))).contiguous()


def rotate(q, r):
    """R(q) r for one quaternion q[4] = x y z w and vectors r[...,3], f64 tensors: (r + w u) + q x u, u = 2 q x r, in
    the grouping of the kernels (csrc/view.h view_rotate).  The conjugate, camera from world, is q with its vector part
    negated."""
    u0 = 2.0 * (q[1] * r[..., 2] - q[2] * r[..., 1])
    u1 = 2.0 * (q[2] * r[..., 0] - q[0] * r[..., 2])
    u2 = 2.0 * (q[0] * r[..., 1] - q[1] * r[..., 0])
    return torch.stack(((r[..., 0] + q[3] * u0) + (q[1] * u2 - q[2] * u1),
                        (r[..., 1] + q[3] * u1) + (q[2] * u0 - q[0] * u2),
                        (r[..., 2] + q[3] * u2) + (q[0] * u1 - q[1] * u0)), -1)


def pinhole_rays(K, hw, device="cuda"):
    """Unit camera-frame rays f32[h,w,3] of a pinhole camera: ((u - cx) / fx, (v - cy) / fy, 1) normalised, pixel
    centres at integer (u, v) (synthetic.pixel_rays)."""
    h, w = (int(x) for x in hw)
    K = torch.as_tensor(K).detach().to(device="cpu", dtype=torch.float64).reshape(3, 3)
    u = torch.arange(w, dtype=torch.float64).view(1, w).expand(h, w)
    v = torch.arange(h, dtype=torch.float64).view(h, 1).expand(h, w)
    r = torch.stack(((u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], torch.ones(h, w, dtype=torch.float64)), -1)
    return (r / r.norm(dim=-1, keepdim=True)).to(device=device, dtype=torch.float32).contiguous()


def hit_points(pose, rays, rng):
    """World points f32[h,w,3] of a view's range image: o + (double)range * s * d in f64, d the ray directions as the
    render kernel forms them (`rotate` on the f32 pose and rays), rounded to f32 once."""
    p = pose.double()
    return (p[:3] + (rng.double() * p[7]).unsqueeze(-1) * rotate(p[3:7], rays.double())).float().contiguous()


def compose_sim3(T, poses):
    """T o pose for poses f64[n,8] and one Sim3 T (8 numbers), in f64 on the host: the cameras of a map moved into the
    frame an alignment leads to."""
    T = torch.as_tensor(T, dtype=torch.float64).detach().to("cpu").reshape(8)
    p = poses.to(torch.float64)
    a, b = T[3:7], p[:, 3:7]
    q = torch.stack((a[3] * b[:, 0] + a[0] * b[:, 3] + a[1] * b[:, 2] - a[2] * b[:, 1],
                     a[3] * b[:, 1] - a[0] * b[:, 2] + a[1] * b[:, 3] + a[2] * b[:, 0],
                     a[3] * b[:, 2] + a[0] * b[:, 1] - a[1] * b[:, 0] + a[2] * b[:, 3],
                     a[3] * b[:, 3] - a[0] * b[:, 0] - a[1] * b[:, 1] - a[2] * b[:, 2]), -1)
    return torch.cat((T[7] * rotate(a, p[:, :3]) + T[:3], q, (T[7] * p[:, 7]).unsqueeze(-1)), -1)
