"""Mirror of mast3r_slam/tsdf/global_volume.py (TSDFVolume, lines 15-140) on a GPU voxel hash.

Same constructor and method names (`integrate`, `query`, `stats`); the python dict
`_voxels[(ix,iy,iz)] -> (tsdf, weight)` becomes an open-addressing table in HBM
(libmslam_hip.so: csrc/tsdf_global.hip).  Inputs may be numpy arrays (as the reference's callers
pass, global_manager.py:101-106) or device tensors; they are moved to the device once.
The per-voxel replay makes results independent of thread scheduling and equal to the reference's
sequential loop; integer keys are bit-exact.  Thread safety: calls are stream-ordered; the
reference's RLock (global_volume.py:30) has no equivalent because there is no host-side state.
"""
import numpy as np
import torch

import mslam_hip as _m

from ._view_args import _hw_arg, _K_arg, _pose_arg, _range_arg, hit_points, pinhole_rays  # noqa: F401 (re-exported)
from .mesh_chain import chain_options, run_chain


_KEY_BIAS = 1 << 20


def voxel_shard(keys, num_shards):
    """Owner rank of integer voxel keys (n,3): host restatement of the device rule in
    csrc/tsdf_global.hip (pack 3x21-bit biased key, murmur3 finaliser, bits 40.. mod num_shards).
    Used by the multi-rank tests and by callers that route queries to the owning rank."""
    k = np.asarray(keys, np.int64) + _KEY_BIAS
    key = (k[:, 0].astype(np.uint64) << np.uint64(42)) | (k[:, 1].astype(np.uint64) << np.uint64(21)) | k[:, 2].astype(np.uint64)
    with np.errstate(over="ignore"):
        key ^= key >> np.uint64(33); key *= np.uint64(0xff51afd7ed558ccd)
        key ^= key >> np.uint64(33); key *= np.uint64(0xc4ceb9fe1a85ec53)
        key ^= key >> np.uint64(33)
    return ((key >> np.uint64(40)) % np.uint64(num_shards)).astype(np.int64)


class TSDFVolume:
    def __init__(self, voxel_size, truncation, max_weight=100.0, min_weight=1.0e-3, capacity=1 << 22,
                 device="cuda", shard_id=0, num_shards=1, group=None, channel=None, color=False):
        self.voxel_size = float(voxel_size)
        self.truncation = float(truncation)
        self.max_weight = float(max_weight)
        self.min_weight = float(min_weight)
        self.capacity = int(capacity)
        self.device = torch.device(device)
        # Voxel sharding (north_star; the reference keeps one dict): this table holds the voxels whose key hashes to
        # `shard_id` of `num_shards` (csrc/tsdf_global.hip: mix64(key) >> 40 mod num_shards).  With num_shards > 1 the
        # methods below are COLLECTIVE over `group`: every rank calls them with the same arguments (integrate keeps only
        # its own voxels of the replicated point list; query all-reduces the owners' look-ups).  `channel`
        # (mast3r_slam/shard.py) is set when one driver rank calls and the others mirror it: the driver announces.
        self.shard_id, self.num_shards = int(shard_id), int(num_shards)
        self.channel = channel
        self.group = channel.group if channel is not None else group
        L = _m.lib()
        nbytes = L.mslam_tsdf_table_bytes(self.capacity)
        if nbytes == 0:
            raise RuntimeError("TSDFVolume: capacity must be a power of two")
        self._table = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._ws = None
        _m.check(L.mslam_tsdf_table_init(_m.ptr(self._table), nbytes, self.capacity, _m.stream_ptr()), "tsdf_table_init")
        # Colour (DESIGN.md "Colour"): a second buffer addressed by the table's slot index, four integer sums per slot.
        # Off: nothing is allocated and nothing below touches it.
        self.color = bool(color)
        if self.color and channel is not None:
            raise ValueError("TSDFVolume: color=True is not supported with a channel-driven shard (the fuse op carries "
                             "no colours); use the SPMD form (group=) or one table")
        self._color = self._new_color(self.capacity) if self.color else None

    @property
    def _driver(self):
        return self.channel is not None and self.channel.is_driver and self.num_shards > 1

    @property
    def _collective(self):
        return self.num_shards > 1 and (self.group is not None or self.channel is not None)

    def _all_reduce(self, t):
        import torch.distributed as dist

        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t

    # ------------------------------------------------------------------
    def _dev(self, a, dtype):
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(np.ascontiguousarray(a))
        return a.to(device=self.device, dtype=dtype).contiguous()

    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self._ws

    def _new_color(self, capacity):
        L = _m.lib()
        nbytes = L.mslam_tsdf_color_bytes(capacity)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        _m.check(L.mslam_tsdf_color_init(_m.ptr(buf), nbytes, capacity, _m.stream_ptr()), "tsdf_color_init")
        return buf

    def _header(self):
        out = (np.zeros(8, np.uint32))
        _m.check(_m.lib().mslam_tsdf_header(_m.ptr(self._table), self.capacity, out.ctypes.data, _m.stream_ptr()),
                 "tsdf_header")
        return out

    def maintain(self, max_load=0.5, reserve=0):
        """The reference's dict never fills up; the table does.  One small D2H read (stream sync): raises if samples
        were dropped (table full / coordinate out of the 21-bit key range) and doubles + rehashes the table when more
        than `max_load` of the slots would be taken after `reserve` further insertions (the caller's bound on what it
        integrates before the next call: the table cannot grow in the middle of an integrate).  The synchronous
        pipeline calls it once per backend solve (TSDFGlobalManager.on_after_backend_solve).  Returns (voxels, capacity)."""
        if self._driver:
            from mast3r_slam import shard as sh

            with self.channel.lock:
                self.channel.announce(sh.OP_TSDF_MAINTAIN, [int(reserve)])
        h = self._header()
        if h[1]:
            raise RuntimeError(f"TSDFVolume: samples were dropped (overflow code {int(h[1])}, {int(h[0])} voxels in "
                               f"{self.capacity} slots); raise tsdf_global.hash_capacity")
        while int(h[0]) + int(reserve) > max_load * self.capacity:
            L = _m.lib()
            new_cap = self.capacity * 2
            nbytes = L.mslam_tsdf_table_bytes(new_cap)
            new = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _m.check(L.mslam_tsdf_table_init(_m.ptr(new), nbytes, new_cap, _m.stream_ptr()), "tsdf_table_init")
            _m.check(L.mslam_tsdf_rehash(_m.ptr(self._table), self.capacity, _m.ptr(new), new_cap, _m.stream_ptr()),
                     "tsdf_rehash")
            if self.color:
                new_color = self._new_color(new_cap)
                _m.check(L.mslam_tsdf_color_rehash(_m.ptr(self._table), self.capacity, _m.ptr(self._color), _m.ptr(new),
                                                   new_cap, _m.ptr(new_color), _m.stream_ptr()), "tsdf_color_rehash")
                self._color = new_color
            self._table, self.capacity = new, new_cap
            h = self._header()
            if h[1]:
                raise RuntimeError("TSDFVolume: rehash overflow")
        return int(h[0]), self.capacity

    # ------------------------------------------------------------------
    def integrate(self, points_world, confidences, cam_origin, step_scale=0.5, return_fused=True, colors=None):
        """global_volume.py:35-72.  Returns the number of fused points (needs one stream sync; pass
        return_fused=False inside a pipeline to stay asynchronous).  `colors` f32[n,3] in [0, 1] (needs color=True):
        the points' colours are fused into the voxels the same samples touch, after the TSDF integrate and on the same
        stream; the TSDF itself is the same with and without them."""
        pts = self._dev(points_world, torch.float32).reshape(-1, 3)
        n = pts.shape[0]
        rgb = None
        if colors is not None:
            if not self.color:
                raise ValueError("TSDFVolume.integrate: colors= needs a volume built with color=True")
            rgb = self._dev(colors, torch.float32)
            if rgb.dim() < 1 or rgb.shape[-1] != 3 or rgb.numel() != 3 * n:
                raise ValueError(f"TSDFVolume.integrate: colors must be ({n},3), got {tuple(rgb.shape)}")
            rgb = rgb.reshape(-1, 3)
        if n == 0:
            return 0
        conf = self._dev(confidences, torch.float64).reshape(-1)
        org = self._dev(cam_origin, torch.float32).reshape(3)
        if self._driver:       # the point list is replicated (1.3 MB per 40 000 points), every rank keeps its own voxels
            from mast3r_slam import shard as sh

            pk = torch.empty((n + 1, 4), dtype=torch.float64, device=self.device)
            pk[:n, :3], pk[:n, 3], pk[n, :3], pk[n, 3] = pts, conf, org, 0.0     # f32 -> f64 -> f32 is exact
            with self.channel.lock:
                self.channel.announce(sh.OP_TSDF_FUSE, [n])
                self.channel.bcast(pk)
        L = _m.lib()
        ws = self._workspace(L.mslam_tsdf_integrate_workspace_bytes(n, self.voxel_size, self.truncation, step_scale))
        rc = L.mslam_tsdf_integrate(
            _m.ptr(self._table), self.capacity, _m.ptr(pts), _m.ptr(conf), _m.ptr(org), n, self.voxel_size,
            self.truncation, self.max_weight, float(step_scale), self.shard_id, self.num_shards, _m.ptr(ws),
            ws.numel(), _m.stream_ptr())
        _m.check(rc, "tsdf_integrate")
        if rgb is not None:
            rc = L.mslam_tsdf_integrate_color(_m.ptr(self._table), self.capacity, _m.ptr(self._color), _m.ptr(pts),
                                              _m.ptr(conf), _m.ptr(rgb), _m.ptr(org), n, self.voxel_size,
                                              self.truncation, float(step_scale), _m.stream_ptr())
            _m.check(rc, "tsdf_integrate_color")
        if not return_fused:
            return None
        h = self._header()
        if h[1]:
            raise RuntimeError(f"TSDFVolume: voxel table overflow (code {h[1]}); raise capacity (now {self.capacity})")
        if self.num_shards > 1 and self.shard_id != 0:     # the fused-point count is kept by shard 0 (every point once)
            return None
        return int(h[4])

    def query(self, point_world):
        """global_volume.py:93-105 for one point: (tsdf or None, unit gradient (3,) f64 or None)."""
        v, g, st = self.query_batch(np.asarray(point_world, np.float32).reshape(1, 3))
        st = int(st[0])
        if st == 0:
            return None, None
        return float(v[0]), (g[0].cpu().numpy() if st == 2 else None)

    def query_batch(self, points):
        """Vectorised form: (value f64[n], grad f64[n,3], status u8[n]) device tensors;
        status 0 = (None, None), 1 = (value, None), 2 = (value, gradient)."""
        pts = self._dev(points, torch.float32).reshape(-1, 3)
        n = pts.shape[0]
        val = torch.zeros(n, dtype=torch.float64, device=self.device)
        grad = torch.zeros((n, 3), dtype=torch.float64, device=self.device)
        st = torch.zeros(n, dtype=torch.uint8, device=self.device)
        if self._collective:      # owner-computes: every rank looks up what it holds, the sum is the whole answer
            if self._driver:
                from mast3r_slam import shard as sh

                with self.channel.lock:
                    self.channel.announce(sh.OP_TSDF_QUERY, [n])
                    self.channel.bcast(pts)
            lk = self.lookup7(pts)
            rc = _m.lib().mslam_tsdf_query_lookup(_m.ptr(lk), n, self.voxel_size, self.min_weight, _m.ptr(val), _m.ptr(grad),
                                                  _m.ptr(st), _m.stream_ptr())
            _m.check(rc, "tsdf_query_lookup")
            return val, grad, st
        rc = _m.lib().mslam_tsdf_query(_m.ptr(self._table), self.capacity, _m.ptr(pts), n, self.voxel_size,
                                       self.min_weight, _m.ptr(val), _m.ptr(grad), _m.ptr(st), _m.stream_ptr())
        _m.check(rc, "tsdf_query")
        return val, grad, st

    def lookup7(self, pts, pose=None):
        """(state, weight, tsdf) f64[n,7,3] of the seven voxels a query of each point reads, summed over the shards (a voxel
        has one owner: the sum is exact).  `pose` (8,) f32: pts are camera-frame points, moved with it first."""
        n = pts.shape[0]
        lk = torch.zeros((n, 7, 3), dtype=torch.float64, device=self.device)
        rc = _m.lib().mslam_tsdf_lookup7(_m.ptr(self._table), self.capacity, _m.ptr(pts), n, _m.ptr(pose), self.voxel_size,
                                         _m.ptr(lk), _m.stream_ptr())
        _m.check(rc, "tsdf_lookup7")
        return self._all_reduce(lk) if self._collective else lk

    def voxels(self):
        """Dict contents as sorted arrays: keys i64[n,3] (lexicographic), tsdf f64[n], weight f64[n].  Sharded +
        collective: the union over the shards, on every rank (test / export helper: host-side gather)."""
        if self._collective:
            import torch.distributed as dist

            if self._driver:
                from mast3r_slam import shard as sh

                with self.channel.lock:
                    self.channel.announce(sh.OP_TSDF_VOXELS, [])
            mine = self._local_voxels()
            parts = [None] * dist.get_world_size(self.group)
            dist.all_gather_object(parts, mine, group=self.group)
            keys = np.concatenate([p[0] for p in parts]); t = np.concatenate([p[1] for p in parts])
            w = np.concatenate([p[2] for p in parts])
            o = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
            return keys[o], t[o], w[o]
        return self._local_voxels()

    def _local_voxels(self):
        n = int(self._header()[0])
        keys = torch.zeros((max(n, 1), 3), dtype=torch.int64, device=self.device)
        t = torch.zeros(max(n, 1), dtype=torch.float64, device=self.device)
        w = torch.zeros(max(n, 1), dtype=torch.float64, device=self.device)
        rc = _m.lib().mslam_tsdf_dump(_m.ptr(self._table), self.capacity, _m.ptr(keys), _m.ptr(t), _m.ptr(w),
                                      max(n, 1), _m.stream_ptr())
        _m.check(rc, "tsdf_dump")
        m = int(self._header()[5])
        keys, t, w = keys[:m].cpu().numpy(), t[:m].cpu().numpy(), w[:m].cpu().numpy()
        o = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
        return keys[o], t[o], w[o]

    def voxel_color_sums(self):
        """(keys i64[n,3], sums u64[n,4]) in voxels()'s order: the integer colour sums (sum_w in units of 2^-20, sum_w *
        r8, sum_w * g8, sum_w * b8) of every voxel.  Sharded + collective: the union over the shards, on every rank."""
        if not self.color:
            raise ValueError("TSDFVolume: this volume was built with color=False")
        if self._collective:
            import torch.distributed as dist

            mine = self._local_color_sums()
            parts = [None] * dist.get_world_size(self.group)
            dist.all_gather_object(parts, mine, group=self.group)
            keys = np.concatenate([p[0] for p in parts]); sums = np.concatenate([p[1] for p in parts])
            o = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
            return keys[o], sums[o]
        return self._local_color_sums()

    def _local_color_sums(self):
        keys = self._local_voxels()[0]
        n = len(keys)
        sums = torch.zeros((n, 4), dtype=torch.int64, device=self.device)     # the u64 words, bit for bit
        k = self._dev(keys, torch.int64).reshape(-1, 3)
        _m.check(_m.lib().mslam_tsdf_color_dump(_m.ptr(self._table), self.capacity, _m.ptr(self._color), _m.ptr(k), n,
                                                _m.ptr(sums), _m.stream_ptr()), "tsdf_color_dump")
        return keys, sums.cpu().numpy().view(np.uint64)

    def voxel_colors(self):
        """(keys i64[n,3], rgb f64[n,3] in [0, 1], sum_w u64[n]) in voxels()'s order: c = sum_wc / (255 sum_w), zero
        where sum_w == 0 (a voxel that was loaded or fused without colours)."""
        keys, sums = self.voxel_color_sums()
        sw = sums[:, 0]
        den = 255.0 * np.where(sw > 0, sw, 1).astype(np.float64)
        return keys, sums[:, 1:].astype(np.float64) / den[:, None], sw

    def sample_color(self, points, default_color=(0.5, 0.5, 0.5)):
        """Trilinear colour at world points (...,3) -> (rgb f32[...,3], count u8[...]) device tensors, on the lattice of
        the mesh and the views; a corner voxel without colour contributes `default_color`, `count` is the number of
        coloured corners.  The table is only read.  Sharded volumes: the union of the shards is sampled (collective)."""
        if not self.color:
            raise ValueError("TSDFVolume.sample_color needs a volume built with color=True")
        pts = self._dev(points, torch.float32)
        if pts.dim() < 1 or pts.shape[-1] != 3:
            raise ValueError(f"sample_color: points must be (...,3), got {tuple(pts.shape)}")
        if self.num_shards > 1:
            return self._union().sample_color(pts, default_color)
        image_w = int(pts.shape[1]) if pts.dim() == 3 else 0
        return _sample_color(self._table, self.capacity, self._color, pts, image_w, self.voxel_size, default_color)

    def _union(self):
        """A one-table copy of a sharded volume (with its colours), for the operations whose samples span owners."""
        keys, t, w = self.voxels()
        return _loaded(keys, t, w, self.voxel_size, self.min_weight, self.device,
                       self.voxel_color_sums()[1] if self.color else None)

    # ------------------------------------------------------------------
    def load_voxels(self, keys, tsdf, weight, colors=None):
        """Inserts distinct voxels keys i64[n,3], tsdf f64[n], weight f64[n] as averaged voxels (a table that was built
        elsewhere, e.g. the union of voxel shards).  Local to this table; raises when the table overflowed.  `colors`
        u64[n,4] (needs color=True): the voxels' colour sums as voxel_color_sums() returns them."""
        k = self._dev(keys, torch.int64).reshape(-1, 3)
        t = self._dev(tsdf, torch.float64).reshape(-1)
        w = self._dev(weight, torch.float64).reshape(-1)
        n = k.shape[0]
        if t.shape[0] != n or w.shape[0] != n:
            raise ValueError("load_voxels: keys, tsdf and weight must have the same length")
        c = None
        if colors is not None:
            if not self.color:
                raise ValueError("TSDFVolume.load_voxels: colors= needs a volume built with color=True")
            if isinstance(colors, np.ndarray):
                colors = torch.from_numpy(np.ascontiguousarray(colors).view(np.int64) if colors.dtype == np.uint64
                                          else np.ascontiguousarray(colors))
            c = colors.to(device=self.device, dtype=torch.int64).contiguous()
            if c.numel() != 4 * n:
                raise ValueError(f"load_voxels: colors must be ({n},4), got {tuple(c.shape)}")
        if n == 0:
            return
        _m.check(_m.lib().mslam_tsdf_load(_m.ptr(self._table), self.capacity, _m.ptr(k), _m.ptr(t), _m.ptr(w), n,
                                          _m.stream_ptr()), "tsdf_load")
        h = self._header()
        if h[1]:
            raise RuntimeError(f"TSDFVolume.load_voxels: table overflow (code {int(h[1])}, {n} voxels into "
                               f"{self.capacity} slots)")
        if c is not None:
            _m.check(_m.lib().mslam_tsdf_color_load(_m.ptr(self._table), self.capacity, _m.ptr(self._color), _m.ptr(k),
                                                    _m.ptr(c), n, _m.stream_ptr()), "tsdf_color_load")

    def extract_mesh(self, min_weight=None, level=0.0, colors=False, default_color=(0.5, 0.5, 0.5), **chain):
        """Marching cubes over the fused volume -> (vertices f32[V,3], normals f32[V,3], faces i32[F,3]) device tensors in
        canonical order (DESIGN.md "Mesh extraction").  Corners are voxel centres with weight >= min_weight (default
        self.min_weight), inside = tsdf < level, normals point to free space, faces are counter-clockwise seen from
        there.  The table is only read.  One host read (the output sizes).  Sharded volumes: cubes span owners, so the
        union of the shards (voxels(), collective) is meshed on every rank.  `colors=True` (needs color=True): a fourth
        tensor f32[V,3] in [0, 1], the colour sampled at each f32 vertex position (sample_color).  `chain`: the options
        of the export chain, which then runs on the result (mesh_chain); the defaults leave the mesh as extracted."""
        chain = chain_options(chain, "TSDFVolume.extract_mesh")
        mw = self.min_weight if min_weight is None else float(min_weight)
        if colors and not self.color:
            raise ValueError("TSDFVolume.extract_mesh: colors=True needs a volume built with color=True")
        if self.num_shards > 1:
            if colors:
                return self._union().extract_mesh(min_weight=mw, level=level, colors=True, default_color=default_color,
                                                  **chain)
            keys, t, w = self.voxels()
            return mesh_from_voxels(keys, t, w, self.voxel_size, mw, level, device=self.device, **chain)
        mesh = _extract(self._table, self.capacity, self.voxel_size, mw, float(level), self.device)
        if colors:
            mesh = mesh + (_sample_color(self._table, self.capacity, self._color, mesh[0], 0, self.voxel_size,
                                         default_color)[0],)
        return run_chain(mesh, chain)

    def render(self, pose, rays=None, K=None, hw=None, near=0.05, far=10.0, min_weight=None, level=0.0, step=None,
               skip=True, colors=False, default_color=(0.5, 0.5, 0.5)):
        """Ray cast of the fused volume from a camera -> (range f32[h,w], normals f32[h,w,3], hit bool[h,w]) device
        tensors (DESIGN.md "View rendering").  `pose`: Sim3 (8,) [t, q, s], world from camera.  Either `rays` f32[h,w,3],
        unit, camera frame (the project's ray model for an uncalibrated camera), or a pinhole `K` (3,3) with `hw` =
        (h, w).  `range` is the distance along the unit ray in camera units (range * rays = the camera-frame pointmap;
        0 on a miss); normals are in the world frame and point to free space.  Samples every `step` (default half a
        voxel) between `near` and `far`, world units; a hit is the first crossing from >= level to < level between two
        valid samples.  `skip=False` marches through empty space sample by sample (same output, for checks and timing).
        The table is only read.  Sharded volumes: samples span owners, so the union of the shards (voxels(), collective)
        is rendered on every rank.  `colors=True` (needs color=True): a fourth tensor f32[h,w,3] in [0, 1], the colour
        sampled (sample_color) at the hit point recomputed from the f32 range output, o + (double)range * s * d; zero on
        a miss.  The march does not change."""
        mw = self.min_weight if min_weight is None else float(min_weight)
        if colors and not self.color:
            raise ValueError("TSDFVolume.render: colors=True needs a volume built with color=True")
        pose, rays, step = _render_args(pose, rays, K, hw, near, far, step, self.voxel_size, self.device)
        if self.num_shards > 1:
            if colors:
                return self._union().render(pose, rays=rays, near=near, far=far, min_weight=mw, level=level, step=step,
                                            skip=skip, colors=True, default_color=default_color)
            keys, t, w = self.voxels()
            return render_from_voxels(keys, t, w, self.voxel_size, mw, pose, rays, near=near, far=far, level=level,
                                      step=step, skip=skip, device=self.device)
        view = _render(self._table, self.capacity, self.voxel_size, mw, float(level), pose, rays, float(near),
                       float(far), step, bool(skip), self.device)
        if not colors:
            return view
        rng, _, hit = view
        pts = hit_points(pose, rays, rng)
        rgb = _sample_color(self._table, self.capacity, self._color, pts, int(pts.shape[1]), self.voxel_size,
                            default_color)[0]
        return view + (rgb * hit.unsqueeze(-1),)

    def stats(self):
        """global_volume.py:136-140."""
        keys, t, w = self.voxels()
        return {"valid_voxels": int((w >= self.min_weight).sum()), "total_voxels": int(len(w))}


def _extract(table, capacity, voxel_size, min_weight, level, device):
    L = _m.lib()
    stream = _m.stream_ptr()
    sk = torch.empty(capacity, dtype=torch.int64, device=device)
    _m.check(L.mslam_tsdf_mesh_keys(_m.ptr(table), capacity, min_weight, _m.ptr(sk), stream), "tsdf_mesh_keys")
    sk, order = torch.sort(sk)       # packed-key order = lexicographic (x, y, z): the canonical voxel order
    order = order.contiguous()
    wsb = L.mslam_tsdf_mesh_workspace_bytes(capacity)
    ws = torch.empty(wsb, dtype=torch.uint8, device=device)
    counts = torch.empty((2, capacity), dtype=torch.int32, device=device)
    _m.check(L.mslam_tsdf_mesh_count(_m.ptr(table), capacity, min_weight, level, _m.ptr(sk), _m.ptr(order),
                                     _m.ptr(counts), _m.ptr(ws), wsb, stream), "tsdf_mesh_count")
    # one device-wide scan over both rows (a scan along dim 1 of the (2, capacity) tensor runs one block per row here:
    # 50x slower): the face row then carries V in front of every entry
    incl = torch.cumsum(counts.view(-1), dim=0).view(2, capacity)
    V, VF = (int(x) for x in incl[:, -1].cpu())
    F = VF - V
    verts = torch.empty((V, 3), dtype=torch.float32, device=device)
    normals = torch.empty((V, 3), dtype=torch.float32, device=device)
    faces = torch.empty((F, 3), dtype=torch.int32, device=device)
    if V == 0 and F == 0:
        return verts, normals, faces
    if V >= 1 << 31:
        raise RuntimeError(f"extract_mesh: {V} vertices exceed the int32 face indices")
    base = incl - counts
    base[1] -= incl[0, -1]
    _m.check(L.mslam_tsdf_mesh_emit(_m.ptr(table), capacity, float(voxel_size), min_weight, level, _m.ptr(sk),
                                    _m.ptr(order), _m.ptr(base[0]), _m.ptr(base[1]), _m.ptr(ws), wsb, _m.ptr(verts),
                                    _m.ptr(normals), _m.ptr(faces), V, F, stream), "tsdf_mesh_emit")
    return verts, normals, faces


def _sample_color(table, capacity, color, pts, image_w, voxel_size, default_color):
    dc = [float(x) for x in default_color]
    if len(dc) != 3:
        raise ValueError("default_color must hold 3 values")
    shape = tuple(pts.shape[:-1])
    pts = pts.reshape(-1, 3).contiguous()
    n = pts.shape[0]
    if n >= 1 << 31:
        raise ValueError("sample_color: too many points")
    rgb = torch.empty((n, 3), dtype=torch.float32, device=pts.device)
    cnt = torch.empty(n, dtype=torch.uint8, device=pts.device)
    _m.check(_m.lib().mslam_tsdf_color_sample(_m.ptr(table), capacity, _m.ptr(color), _m.ptr(pts), n, image_w,
                                              float(voxel_size), dc[0], dc[1], dc[2], _m.ptr(rgb), _m.ptr(cnt),
                                              _m.stream_ptr()), "tsdf_color_sample")
    return rgb.reshape(shape + (3,)), cnt.reshape(shape)


def _render_args(pose, rays, K, hw, near, far, step, voxel_size, device):
    """Checked (pose f32[8], rays f32[h,w,3], step) on `device`."""
    pose = _pose_arg(pose, "render", device)
    if (rays is None) == (K is None):
        raise ValueError("render: give either rays (h,w,3) or K with hw")
    if rays is None:
        hw = _hw_arg(hw, "render")
        _K_arg(K, "render")
        rays = pinhole_rays(K, hw, device)
    else:
        if isinstance(rays, np.ndarray):
            rays = torch.from_numpy(np.ascontiguousarray(rays))
        if rays.dim() != 3 or rays.shape[-1] != 3 or rays.shape[0] < 1 or rays.shape[1] < 1:
            raise ValueError(f"render: rays must be (h,w,3), got {tuple(rays.shape)}")
        if hw is not None and tuple(int(x) for x in hw) != tuple(rays.shape[:2]):
            raise ValueError("render: hw does not match rays")
        rays = rays.detach().to(device=device, dtype=torch.float32).contiguous()
    step = 0.5 * float(voxel_size) if step is None else float(step)
    if not step > 0.0:
        raise ValueError("render: step must be positive")
    _range_arg(near, far, "render", strict=True)
    return pose, rays, step


def _render(table, capacity, voxel_size, min_weight, level, pose, rays, near, far, step, skip, device):
    L = _m.lib()
    stream = _m.stream_ptr()
    h, w = int(rays.shape[0]), int(rays.shape[1])
    wsb = L.mslam_tsdf_render_workspace_bytes(capacity)
    ws = torch.empty(wsb, dtype=torch.uint8, device=device)
    _m.check(L.mslam_tsdf_render_blocks(_m.ptr(table), capacity, min_weight, _m.ptr(ws), wsb, stream),
             "tsdf_render_blocks")
    rng = torch.empty((h, w), dtype=torch.float32, device=device)
    nrm = torch.empty((h, w, 3), dtype=torch.float32, device=device)
    hit = torch.empty((h, w), dtype=torch.uint8, device=device)
    _m.check(L.mslam_tsdf_render(_m.ptr(table), capacity, _m.ptr(rays), h, w, _m.ptr(pose), float(voxel_size),
                                 min_weight, level, near, far, step, int(skip), _m.ptr(ws), wsb, _m.ptr(rng),
                                 _m.ptr(nrm), _m.ptr(hit), stream), "tsdf_render")
    return rng, nrm, hit.bool()


def _loaded(keys, tsdf, weight, voxel_size, min_weight, device, colors=None):
    """A temporary table of at least 2n slots that holds the given voxels (and their colour sums)."""
    n = int(len(keys))
    cap = 1024
    while cap < 2 * n:
        cap *= 2
    vol = TSDFVolume(voxel_size, 1.0, min_weight=min_weight, capacity=cap, device=device, color=colors is not None)
    vol.load_voxels(keys, tsdf, weight, colors=colors)
    return vol


def render_from_voxels(keys, tsdf, weight, voxel_size, min_weight, pose, rays, near=0.05, far=10.0, level=0.0,
                       step=None, skip=True, device="cuda", colors=None, default_color=(0.5, 0.5, 0.5)):
    """View of a voxel set given as arrays (keys i64[n,3] distinct, tsdf f64[n], weight f64[n]; numpy or device): loads
    a temporary table of at least 2n slots and renders from it (TSDFVolume.render semantics).  `colors` u64[n,4]: the
    voxels' colour sums (voxel_color_sums()); the view then carries the colour image as a fourth tensor."""
    vol = _loaded(keys, tsdf, weight, voxel_size, min_weight, device, colors)
    return vol.render(pose, rays=rays, near=near, far=far, min_weight=min_weight, level=level, step=step, skip=skip,
                      colors=colors is not None, default_color=default_color)


def mesh_from_voxels(keys, tsdf, weight, voxel_size, min_weight, level=0.0, device="cuda", colors=None,
                     default_color=(0.5, 0.5, 0.5), **chain):
    """Mesh of a voxel set given as arrays (keys i64[n,3] distinct, tsdf f64[n], weight f64[n]; numpy or device): loads
    a temporary table of at least 2n slots and extracts from it (TSDFVolume.extract_mesh semantics, the export chain of
    mesh_chain included).  `colors` u64[n,4]: the voxels' colour sums (voxel_color_sums()); the mesh then carries vertex
    colours as a fourth tensor."""
    vol = _loaded(keys, tsdf, weight, voxel_size, min_weight, device, colors)
    return vol.extract_mesh(min_weight=min_weight, level=level, colors=colors is not None, default_color=default_color,
                            **chain)
