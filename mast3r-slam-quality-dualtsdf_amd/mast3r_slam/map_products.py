"""The map products of a run - meshes, clouds, views and their scores against ground truth - as a base class of SlamSystem
that uses nothing of it but `keyframes`, `tsdf_manager`, `K`, `device` and `drain()`.  A keyframe's camera comes from
the helpers at the top (DESIGN.md "Cameras and views")."""
import torch

from mast3r_slam.config import config


def _sim3(T):
    """f64[8] on the host of one Sim3: a tensor, an array, a sequence or a lietorch Sim3."""
    return torch.as_tensor(getattr(T, "data", T)).detach().double().cpu().reshape(8)


class MapProducts:
    # ---- the keyframes' cameras ------------------------------------------------------------------------------------
    @staticmethod
    def _keyframe_hw(kf):
        """(h, w) of a keyframe's pointmap."""
        h, w = (int(x) for x in kf.img_shape.reshape(-1)[:2].tolist())
        return h, w

    def _keyframe_poses(self):
        """The keyframes' T_WC [n,8], in keyframe order (n >= 1)."""
        return torch.stack([self.keyframes[i].T_WC.data.detach().reshape(8) for i in range(len(self.keyframes))])

    def _keyframe_view(self, kf):
        """The camera arguments of a view through a keyframe: dict(K=, hw=) when the system is calibrated, otherwise
        dict(rays=), the canonical pointmap normalised to unit length - the ray model of an uncalibrated camera."""
        h, w = self._keyframe_hw(kf)
        if config["use_calib"] and self.K is not None:
            return dict(K=self.K, hw=(h, w))
        X = kf.X_canon.detach().reshape(h, w, 3).float()
        return dict(rays=X / X.norm(dim=-1, keepdim=True).clamp_min(1.0e-12))

    def _keyframe_image(self, kf, what, i):
        """The keyframe's `uimg` f32[h,w,3] at the pointmap's size, read by the colour fusion's rule
        (tsdf.global_manager.gather_uimg); `what` and `i` name the caller and the keyframe when it has none."""
        from mast3r_slam.tsdf.global_manager import gather_uimg

        if kf.uimg is None:
            raise ValueError(f"{what}: keyframe {i} has no uimg")
        h, w = self._keyframe_hw(kf)
        pixels = torch.arange(h * w, device=self.device)
        return gather_uimg(kf.uimg.detach(), pixels, (h, w)).reshape(h, w, 3)

    def _keyframe_pinholes(self, what, gt_K, asked):
        """(K, the keyframes' poses [n,8], (h, w) of the newest keyframe) for the views that need a projection; K is
        `gt_K` or else the system's calibration.  Raises without a pinhole and without a keyframe."""
        K = gt_K if gt_K is not None else self.K
        if K is None:
            raise ValueError(f"{what}: {asked} needs a pinhole camera, gt_K or the system's calibration: the ray-image "
                             "camera model has no projection")
        if len(self.keyframes) == 0:
            raise RuntimeError(f"{what}: {asked} needs at least one keyframe")
        return K, self._keyframe_poses(), self._keyframe_hw(self.keyframes[len(self.keyframes) - 1])

    # ---- meshes, clouds, views -------------------------------------------------------------------------------------
    def extract_mesh(self, min_weight=None, level=0.0, colors=False, **chain):
        """Triangle mesh of the global TSDF at this point of the run: (vertices f32[V,3], normals f32[V,3], faces i32[F,3])
        device tensors (TSDFVolume.extract_mesh).  Drains the backend first, so every fusion it has issued is ordered
        before the read.  `colors=True` (tsdf_global.color on): vertex colours f32[V,3] as a fourth tensor.  `chain`: the
        options of the export chain (tsdf/mesh_chain.py); one that is absent or None takes tsdf_global's value
        (mesh_chain.CONFIG), anything else, an explicit 0 included, stays as given."""
        if self.tsdf_manager is None:
            raise RuntimeError("SlamSystem.extract_mesh: the global TSDF is disabled (tsdf_global.enabled = False)")
        from mast3r_slam.tsdf.mesh_chain import config_defaults

        chain = config_defaults(chain, self.tsdf_manager.cfg, self.tsdf_manager.volume.voxel_size)
        self.drain()
        return self.tsdf_manager.extract_mesh(min_weight=min_weight, level=level, colors=colors, **chain)

    def align_trajectory(self, gt_positions):
        """The Sim3 that moves the map's frame onto a ground truth's, from camera centres: tsdf.fit_sim3 of the keyframes'
        centres (the translations of their T_WC, in keyframe order) onto gt_positions (K x 3, numpy or tensor, one row
        per keyframe) -> f64[8] device tensor in lietorch layout.  An `init` for evaluate_mesh(align="icp").  Drains the
        backend first, so the poses are the ones it has solved."""
        from mast3r_slam.tsdf import fit_sim3

        self.drain()
        n = len(self.keyframes)
        gt = torch.as_tensor(gt_positions, dtype=torch.float32).to(self.device).reshape(-1, 3)
        if gt.shape[0] != n:
            raise ValueError(f"SlamSystem.align_trajectory: {n} keyframes but {gt.shape[0]} ground-truth positions")
        centres = [self.keyframes[i].T_WC.data.reshape(8)[:3] for i in range(n)]
        est = torch.stack(centres).to(device=self.device, dtype=torch.float32) if n else gt.new_zeros((0, 3))
        return fit_sim3(est, gt)[0]

    def _alignment_kw(self, what, align, init, gt_positions, align_kw):
        """The align / align_kw keywords of compare_meshes and compare_clouds from evaluate_mesh's and evaluate_cloud's
        arguments: with align="icp", `init` joins align_kw, "trajectory" as self.align_trajectory(gt_positions)."""
        if not isinstance(align, str):
            if init is not None or align_kw:
                raise ValueError(f"{what}: init and align_kw go with align='icp' only")
            return {} if align is None else dict(align=align)
        align_kw = dict(align_kw or {})
        if isinstance(init, str):
            if init != "trajectory" or gt_positions is None:
                raise ValueError(f"{what}: init='trajectory' needs gt_positions")
            init = self.align_trajectory(gt_positions)
        if init is not None:
            align_kw["init"] = init
        return dict(align=align, align_kw=align_kw)

    def evaluate_mesh(self, gt_vertices, gt_faces, n_samples=200_000, threshold=None, align=None, init=None,
                      gt_positions=None, align_kw=None, observed=False, gt_K=None, index=None, **extract_kw):
        """Quality of the global TSDF's mesh at this point of the run against a ground-truth mesh (gt_vertices f32[V,3],
        gt_faces i32[F,3]; numpy arrays or device tensors): the dict of tsdf.compare_meshes,
        accuracy / completion / precision / recall / fscore / chamfer (DESIGN.md "Mesh quality").  The mesh is
        self.extract_mesh(**extract_kw), so the backend is drained first and the config's clean-up default applies.
        `threshold` defaults to tsdf_global.mesh_eval_threshold.

        `align=None`: the ground truth lies in the map's frame.  A Sim3 or "icp": compare_meshes(align=...) moves the
        mesh into the ground truth's frame first (DESIGN.md "Mesh alignment"); `init` is where ICP starts - a Sim3, or
        "trajectory" with `gt_positions` (K x 3, one row per keyframe) for self.align_trajectory(gt_positions);
        `align_kw`: further arguments of tsdf.align_meshes, dict(metric="plane", point_weight=0.05) among them (DESIGN.md
        "Point-to-plane ICP").

        `observed=True`: only the part of the ground truth that some keyframe sees enters completion, recall, fscore and
        chamfer (compare_meshes(observed=...), DESIGN.md "Mesh ray casting"): the cameras are the keyframes' T_WC, moved
        by the alignment, with the pinhole `gt_K` (3,3) or else the system's calibration at the keyframes' image size.
        Without either it raises: the ray-image camera model has no projection.

        `index`: None, True or a tsdf.MeshIndex of the ground-truth tensors (DESIGN.md "Mesh index").  True builds one
        here, and the alignment, the scoring against the ground truth and the observed-part cull all use it, so that
        their speed does not depend on the order of the ground truth's faces.  The figures do not change."""
        if self.tsdf_manager is None:
            raise RuntimeError("SlamSystem.evaluate_mesh: the global TSDF is disabled (tsdf_global.enabled = False)")
        from mast3r_slam.tsdf import compare_meshes

        if threshold is None:
            threshold = float(self.tsdf_manager.cfg.get("mesh_eval_threshold", 0.05))
        kw = self._alignment_kw("SlamSystem.evaluate_mesh", align, init, gt_positions, align_kw)
        mesh = self.extract_mesh(**extract_kw)
        dev = mesh[0].device
        gt_vertices = torch.as_tensor(gt_vertices, dtype=torch.float32).to(dev)
        gt_faces = torch.as_tensor(gt_faces, dtype=torch.int32).to(dev)
        if observed:
            K, poses, hw = self._keyframe_pinholes("SlamSystem.evaluate_mesh", gt_K, "observed=True")
            kw["observed"] = dict(poses=poses, K=K, hw=hw, frame="pred")
        if index is not None and index is not False:
            kw["index"] = index
        return compare_meshes(mesh, (gt_vertices, gt_faces), n_samples=n_samples, threshold=threshold,
                              _validate_pred=False, **kw)

    def keyframe_cloud(self, conf_threshold=None, voxel=None, colors=True, outliers=None, normals=None, clusters=None,
                       smooth=None):
        """The map as a point cloud at this point of the run, on the device: what evaluate.save_reconstruction gathers -
        for every keyframe the world points T_WC.act(X_canon) (with calibration: X_canon constrained to the pixel rays
        first) of the pixels whose average confidence is > `conf_threshold` (default tracking.C_conf of the config), in
        keyframe order -> (points f32[N,3], colors u8[N,3] or None).  `voxel`: the cloud is then thinned by
        tsdf.downsample_cloud on that grid (centroids and mean colours, in key order).  `colors=False`: no colours.
        Drains the backend first, so the poses are the ones it has solved.  `outliers`: a dict of keyword arguments for
        tsdf.cloud_outliers, applied after `voxel`; the points it drops leave the cloud.  `normals`: k - a third return
        value, tsdf.cloud_normals(points, k) turned towards the camera centre of the keyframe each point came from
        (after thinning: the keyframe of the cell's lowest-index member).  `clusters`: a dict of keyword arguments for
        tsdf.filter_cloud_clusters (eps, min_points, min_cluster_points, keep_largest, keep_noise), applied after
        `voxel` and `outliers` and before `normals`: whole clusters leave the cloud - the small dense blobs in the air
        that have neighbours enough for the point-wise rules.  `smooth`: a dict of keyword arguments for
        tsdf.smooth_cloud (radius, which is required; iterations, min_points, strength, edge_angle), applied after
        `voxel`, `outliers` and `clusters` and before `normals`: the points that are left move onto the local planes of
        the cloud, their colours and order stay.  With all four None the pair is what it was."""
        from mast3r_slam.geometry import constrain_points_to_ray

        self.drain()
        if conf_threshold is None:
            conf_threshold = float(config["tracking"]["C_conf"])
        pts, cols, source = [], [], []
        for i in range(len(self.keyframes)):
            kf = self.keyframes[i]
            X = kf.X_canon
            if config["use_calib"]:
                X = constrain_points_to_ray(kf.img_shape.flatten()[:2], X[None], kf.K).squeeze(0)
            pW = kf.T_WC.act(X).reshape(-1, 3).to(device=self.device, dtype=torch.float32)
            keep = kf.get_average_conf().to(device=self.device, dtype=torch.float32).reshape(-1) > conf_threshold
            pts.append(pW[keep])
            if normals is not None:
                source.append((i, kf.T_WC.data.reshape(8)[:3].to(device=self.device, dtype=torch.float32)))
            if colors:
                cols.append((kf.uimg * 255).to(torch.uint8).reshape(-1, 3).to(self.device)[keep])
        points = torch.cat(pts).contiguous() if pts else torch.zeros((0, 3), dtype=torch.float32, device=self.device)
        color = (torch.cat(cols).contiguous() if cols else torch.zeros((0, 3), dtype=torch.uint8,
                                                                        device=self.device)) if colors else None
        if outliers is None and normals is None and clusters is None and smooth is None:
            if voxel is not None:
                from mast3r_slam.tsdf import downsample_cloud

                points, color, _ = downsample_cloud(points, voxel, color)
            return points, color
        from mast3r_slam.tsdf import (cloud_normals, downsample_cloud, filter_cloud, filter_cloud_clusters,
                                      smooth_cloud)

        # the keyframe of every point, carried through the thinning and the filter
        kf_of = (torch.cat([torch.full((int(p.shape[0]),), i, dtype=torch.int64, device=self.device)
                            for p, (i, _) in zip(pts, source)]) if source else
                 torch.zeros(0, dtype=torch.int64, device=self.device))
        if voxel is not None:
            points, color, _, first = downsample_cloud(points, voxel, color, return_first=True)
            if normals is not None:
                kf_of = kf_of[first.long()]
        if outliers is not None:
            points, color, kept = filter_cloud(points, color, **dict(outliers))
            if normals is not None:
                kf_of = kf_of[kept]
        if clusters is not None:
            points, color, kept = filter_cloud_clusters(points, color, **dict(clusters))
            if normals is not None:
                kf_of = kf_of[kept]
        if smooth is not None:
            if "radius" not in smooth:
                raise ValueError("SlamSystem.keyframe_cloud: smooth needs a radius")
            points, color, _ = smooth_cloud(points, colors=color, **dict(smooth))
        if normals is None:
            return points, color
        centres = (torch.stack([c for _, c in source]) if source else
                   torch.zeros((0, 3), dtype=torch.float32, device=self.device))
        viewpoint = centres[kf_of].contiguous() if int(points.shape[0]) else None
        return points, color, cloud_normals(points, normals, viewpoint=viewpoint)[0]

    def evaluate_cloud(self, gt_points, threshold=None, voxel=None, align=None, init=None, gt_positions=None,
                       align_kw=None, index=None, conf_threshold=None, outliers=None, normals=None, observed=False,
                       gt_K=None, clusters=None, smooth=None):
        """Quality of the map's point cloud (self.keyframe_cloud(conf_threshold)) against a ground-truth cloud gt_points
        f32[N,3] (a numpy array or a device tensor; a laser scan needs no faces): the dict of tsdf.compare_clouds
        (DESIGN.md "Point clouds").  `threshold` and `voxel` default to the global TSDF's voxel size (the config's when
        the global TSDF is off): both clouds are thinned on the map's own grid and a point counts as right within one
        cell; voxel=0 scores the raw clouds.  `align`, `init` ("trajectory" with `gt_positions` for
        self.align_trajectory), `align_kw` and `index` (None or True) as in evaluate_mesh, with tsdf.align_clouds in the
        place of align_meshes.  `outliers`: a dict for tsdf.cloud_outliers, applied to the map's raw cloud first
        (keyframe_cloud), `clusters` a dict for tsdf.filter_cloud_clusters, applied after it, and `smooth` a dict for
        tsdf.smooth_cloud, applied last; `normals`: k, for compare_clouds' normal-consistency figures.

        `observed=True`: only the part of the ground truth that some keyframe sees, the thinned ground-truth cloud itself
        the occluder, enters completion, recall, fscore and chamfer (compare_clouds(observed=...), DESIGN.md "Cloud
        views"): the cameras are the keyframes' T_WC, moved by the alignment, with the pinhole `gt_K` (3,3) or else the
        system's calibration at the keyframes' image size.  Without either it raises: the ray-image camera model has no
        projection.  A dict instead of True overrides entries of compare_clouds' `observed` (point_size, tol, ...)."""
        from mast3r_slam.tsdf import compare_clouds

        vs = float(self.tsdf_manager.volume.voxel_size if self.tsdf_manager is not None
                   else config["tsdf_global"]["voxel_size"])
        threshold = vs if threshold is None else float(threshold)
        voxel = vs if voxel is None else float(voxel)
        kw = self._alignment_kw("SlamSystem.evaluate_cloud", align, init, gt_positions, align_kw)
        points, _ = self.keyframe_cloud(conf_threshold, colors=False, outliers=outliers, clusters=clusters,
                                        smooth=smooth)
        gt = torch.as_tensor(gt_points, dtype=torch.float32).to(points.device).reshape(-1, 3).contiguous()
        if index is not None and index is not False:
            kw["index"] = index
        if normals is not None:
            kw["normals"] = normals
        if observed is not False and observed is not None:
            K, poses, hw = self._keyframe_pinholes("SlamSystem.evaluate_cloud", gt_K, "observed=True")
            kw["observed"] = dict(dict(poses=poses, K=K, hw=hw, frame="pred"),
                                  **(observed if isinstance(observed, dict) else {}))
        return compare_clouds(points, gt, threshold=threshold, voxel=voxel if voxel > 0.0 else None, **kw)

    def cloud_planes(self, conf_threshold=None, voxel=None, outliers=None, smooth=None, **planes_kw):
        """The planes of the map's point cloud: tsdf.cloud_planes on self.keyframe_cloud(conf_threshold, voxel,
        outliers=outliers, smooth=smooth) -> (points f32[N,3], the dict of tsdf.cloud_planes).  `tol` defaults to the global TSDF's
        voxel size (the config's when the global TSDF is off); every other keyword is cloud_planes' (DESIGN.md "Cloud
        planes")."""
        from mast3r_slam.tsdf import cloud_planes

        points, _ = self.keyframe_cloud(conf_threshold, voxel, colors=False, outliers=outliers, smooth=smooth)
        if "tol" not in planes_kw:
            planes_kw["tol"] = float(self.tsdf_manager.volume.voxel_size if self.tsdf_manager is not None
                                     else config["tsdf_global"]["voxel_size"])
        return points, cloud_planes(points, **planes_kw)

    def evaluate_planarity(self, conf_threshold=None, voxel=None, outliers=None, **planes_kw):
        """Quality figures of the map that need no ground truth: tsdf.plane_figures of self.cloud_planes(...) - the
        share of the cloud that lies on planes, the rmse of those points about their planes, the number of planes, and
        how far the planes stand from parallel or square to each other, in degrees.  Python floats."""
        from mast3r_slam.tsdf import plane_figures

        points, result = self.cloud_planes(conf_threshold, voxel, outliers, **planes_kw)
        return plane_figures(result, points)

    def evaluate_cloud_depth(self, gt_points, point_size=None, align=None, near=0.05, far=10.0, gt_K=None):
        """ "Depth L1" against a laser scan: for every keyframe, the view of the global TSDF (TSDFVolume.render) against
        the z-buffer splat of the ground-truth cloud gt_points f32[N,3] (tsdf.render_cloud; a numpy array or a device
        tensor) from the same camera through the same pinhole - `gt_K` (3,3) or else the system's calibration; without
        either it raises, a splat needs a projection.  `point_size`: the world-unit diameter of a ground-truth point,
        default twice the TSDF's voxel size (times the alignment's scale).  `align`, `near`, `far` and the returned
        dict - depth_l1, depth_l1_median, both_hit_share, n_pixels - as in evaluate_depth, with the same handling of
        scale.  Drains the backend first."""
        what = "SlamSystem.evaluate_cloud_depth"
        if self.tsdf_manager is None:
            raise RuntimeError(f"{what}: the global TSDF is disabled (tsdf_global.enabled = False)")
        from mast3r_slam.tsdf import render_cloud

        self.drain()
        K = self._keyframe_pinholes(what, gt_K, "a cloud view")[0]
        gt = torch.as_tensor(gt_points, dtype=torch.float32).to(self.device).reshape(-1, 3).contiguous()
        if point_size is None:       # in ground-truth units: the map's voxel times the alignment's scale
            a_scale = 1.0 if align is None else float(_sim3(align)[7])
            point_size = 2.0 * float(self.tsdf_manager.volume.voxel_size) * a_scale

        def render_gt(i, moved, view):
            return render_cloud(gt, moved, near=near, far=far, point_size=point_size, **view)

        return self._depth_l1(render_gt, align, near, far, lambda kf: dict(K=K, hw=self._keyframe_hw(kf)))

    def render_cloud_view(self, pose=None, **kw):
        """The map's own cloud seen from a camera: tsdf.render_cloud of self.keyframe_cloud() with its colours ->
        (range f32[h,w], index i32[h,w], hit bool[h,w], rgb u8[h,w,3]).  `pose=None`: the newest keyframe's pose.
        `kw`: render_cloud's K, hw, near, far, radius, point_size, max_radius, and keyframe_cloud's conf_threshold and
        voxel; K and hw default to the system's calibration and the newest keyframe's image size, and without a pinhole
        it raises."""
        what = "SlamSystem.render_cloud_view"
        from mast3r_slam.tsdf import render_cloud

        cloud_kw = {k: kw.pop(k) for k in ("conf_threshold", "voxel") if k in kw}
        points, colors = self.keyframe_cloud(**cloud_kw)                     # drains the backend
        K, poses, hw = self._keyframe_pinholes(what, kw.pop("K", None), "a cloud view")
        pose = poses[-1] if pose is None else torch.as_tensor(getattr(pose, "data", pose)).reshape(-1)    # one view
        return render_cloud(points, pose, K, kw.pop("hw", None) or hw, colors=colors, **kw)

    def evaluate_depth(self, gt_vertices, gt_faces, align=None, near=0.05, far=10.0, index=None):
        """The "Depth L1" figure of dense-SLAM evaluations: for every keyframe, the view of the global TSDF
        (TSDFVolume.render) against the view of a ground-truth mesh (tsdf.render_mesh; gt_vertices f32[V,3], gt_faces
        i32[F,3], numpy arrays or device tensors) from the same camera through the same rays - the system's intrinsics
        when it is calibrated, otherwise the keyframe's canonical pointmap normalised to unit length (render_view).
        `align`: None - the ground truth lies in the map's frame; a Sim3 - it moves the keyframe's pose into the ground
        truth's frame for the mesh view.  `near`, `far`: ground-truth units.  Returns Python numbers: depth_l1 and
        depth_l1_median, mean and median of |range_map - range_gt| times the moved pose's scale (ground-truth units)
        over the pixels hit in both views (NaN without one), both_hit_share and n_pixels.  Drains the backend first.
        `index`: None, True or a tsdf.MeshIndex of the ground-truth tensors: one index serves every keyframe's view of the
        ground truth (DESIGN.md "Mesh index"); the figures do not change."""
        if self.tsdf_manager is None:
            raise RuntimeError("SlamSystem.evaluate_depth: the global TSDF is disabled (tsdf_global.enabled = False)")
        from mast3r_slam.tsdf import render_mesh
        from mast3r_slam.tsdf.mesh_index import MeshIndex, _index_arg

        self.drain()
        if len(self.keyframes) == 0:
            raise RuntimeError("SlamSystem.evaluate_depth: no keyframe yet")
        gt = (torch.as_tensor(gt_vertices, dtype=torch.float32).to(self.device),
              torch.as_tensor(gt_faces, dtype=torch.int32).to(self.device))
        index = _index_arg(MeshIndex, index, "SlamSystem.evaluate_depth", *gt)

        def render_gt(i, moved, view):
            return render_mesh(gt, moved, near=near, far=far, validate=i == 0, index=index, **view)

        return self._depth_l1(render_gt, align, near, far, self._keyframe_view)

    def _depth_l1(self, render_gt, align, near, far, view_of):
        """The keyframe loop of evaluate_depth and evaluate_cloud_depth (backend drained): for every keyframe the view
        of the global TSDF through `view_of(kf)` against `render_gt(i, moved pose, view)` -> (range, _, hit) of the
        ground truth, the pose moved by `align` (None or a Sim3) for the ground truth and near / far divided by its
        scale for the map -> the dict evaluate_depth documents."""
        from mast3r_slam.tsdf._view_args import compose_sim3

        T = None if align is None else _sim3(align)
        a_scale = 1.0 if T is None else float(T[7])
        diffs, n_pixels = [], 0
        for i in range(len(self.keyframes)):
            kf = self.keyframes[i]
            view = view_of(kf)
            pose = kf.T_WC.data.detach().reshape(8)
            moved = pose.double().cpu() if T is None else compose_sim3(T, pose.double().cpu().reshape(1, 8))[0]
            r_map, _, hit_map = self.tsdf_manager.render(pose, near=near / a_scale, far=far / a_scale, **view)[:3]
            r_gt, _, hit_gt = render_gt(i, moved, view)[:3]
            both = hit_map & hit_gt
            diffs.append((r_map.double() - r_gt.double()).abs()[both] * float(moved[7]))
            n_pixels += int(hit_map.numel())
        d = torch.sort(torch.cat(diffs))[0]
        m = int(d.numel())
        l1, med = (float("nan"),) * 2 if m == 0 else torch.stack((d.sum() / m, 0.5 * (d[(m - 1) // 2] + d[m // 2]))).tolist()
        return dict(depth_l1=l1, depth_l1_median=med, both_hit_share=m / n_pixels, n_pixels=n_pixels)

    def evaluate_render(self, images=None, poses=None, rays=None, K=None, near=0.05, far=10.0, chunk=8):
        """The photometric figures of dense-SLAM evaluations: PSNR and SSIM of the colour views of the global TSDF
        against camera images (tsdf.image_metrics, DESIGN.md "Render quality").  Needs tsdf_global.color.

        Without `images`, the training views: every keyframe's pose, through the rays evaluate_depth uses (the
        system's intrinsics when it is calibrated, otherwise the keyframe's canonical pointmap normalised to unit
        length), against the keyframe's `uimg`; where uimg is smaller than the pointmap (dataset.img_downsample > 1) it is
        read by the colour fusion's rule, uimg[r h // H, c w // W] (tsdf.global_manager.gather_uimg), so a training view
        is compared with exactly what was fused.  With `images` f32[M,h,w,3] in [0,1], held-out views: `poses` Sim3
        [M,8] in the map's frame and a pinhole `K` (3,3; the images' shape) or `rays` f32[h,w,3] / [M,h,w,3].

        The mask of a view is its hit image: a pixel enters the squared error when its ray hit the surface, a window
        enters SSIM when all its 121 pixels did.  Views are rendered `chunk` at a time and scored by one launch per
        chunk.  Returns Python numbers: psnr / ssim, the means over the views that have a pixel / a window (NaN without
        one), psnr_min / ssim_min, hit_share and window_share (of all pixels of all views), n_views, and per_view: lists
        of psnr, ssim, n_pixels, n_windows.  Drains the backend first."""
        what = "SlamSystem.evaluate_render"
        if self.tsdf_manager is None:
            raise RuntimeError(f"{what}: the global TSDF is disabled (tsdf_global.enabled = False)")
        if not self.tsdf_manager.volume.color:
            raise RuntimeError(f"{what}: the global TSDF carries no colour (tsdf_global.color = False)")

        def render(pose, r):
            out = self.tsdf_manager.render(pose, near=near, far=far, colors=True, **r)
            return out[3], out[2]

        return self._score_views(what, render, images, poses, rays, K, chunk, True)

    def _score_views(self, what, render, images, poses, rays, K, chunk, need_keyframe):
        """The view loop of evaluate_render and evaluate_mesh_render: the training views (images None) or the held-out
        views, `render(pose, rays-or-K arguments)` -> (rgb f32[h,w,3], hit bool[h,w]) for each, `chunk` views scored by
        one image_metrics launch -> the dict evaluate_render documents.  Drains the backend first."""
        from mast3r_slam.tsdf import image_metrics
        from mast3r_slam.tsdf._view_args import _poses_arg

        self.drain()
        if images is None:
            if poses is not None or rays is not None or K is not None:
                raise ValueError(f"{what}: poses, rays and K go with images")
            n_views = len(self.keyframes)
            if n_views == 0:
                raise RuntimeError(f"{what}: no keyframe yet")
        else:
            images = torch.as_tensor(images)
            if images.dim() != 4 or images.shape[3] != 3 or not images.is_floating_point():
                raise ValueError(f"{what}: images must be float (M,h,w,3), got {tuple(images.shape)} {images.dtype}")
            n_views, h, w = (int(x) for x in images.shape[:3])
            if need_keyframe and len(self.keyframes) == 0:
                raise RuntimeError(f"{what}: no keyframe yet")
            if poses is None or (rays is None) == (K is None):
                raise ValueError(f"{what}: images need poses and either K or rays")
            poses = _poses_arg(poses, what)
            if poses.shape[0] != n_views:
                raise ValueError(f"{what}: {n_views} images but {poses.shape[0]} poses")
            if rays is not None:
                rays = torch.as_tensor(rays).to(self.device)
                if tuple(rays.shape) not in ((h, w, 3), (n_views, h, w, 3)):
                    raise ValueError(f"{what}: rays must be {(h, w, 3)} or {(n_views, h, w, 3)}, got {tuple(rays.shape)}")

        def view(i):
            """(pose, render arguments, target f32[h,w,3] on the device) of view i."""
            if images is not None:
                r = dict(K=K, hw=(h, w)) if rays is None else dict(rays=rays if rays.dim() == 3 else rays[i])
                return poses[i], r, images[i].to(device=self.device, dtype=torch.float32)
            kf = self.keyframes[i]
            return kf.T_WC.data.detach().reshape(8), self._keyframe_view(kf), self._keyframe_image(kf, what, i)

        per = dict(psnr=[], ssim=[], n_pixels=[], n_windows=[])
        total = 0
        for start in range(0, n_views, max(int(chunk), 1)):
            rgb, hit, tgt = [], [], []
            for i in range(start, min(start + max(int(chunk), 1), n_views)):
                pose, r, target = view(i)
                view_rgb, view_hit = render(pose, r)
                if view_rgb.shape != target.shape:
                    raise ValueError(f"{what}: view {i} renders {tuple(view_rgb.shape)} against an image of "
                                     f"{tuple(target.shape)}")
                rgb.append(view_rgb), hit.append(view_hit), tgt.append(target)
            if any(x.shape != rgb[0].shape for x in rgb):
                raise ValueError(f"{what}: the views {start}.. differ in shape; score them with chunk=1")
            m = image_metrics(torch.stack(rgb), torch.stack(tgt), mask=torch.stack(hit))     # one launch, one host read
            for v in torch.stack((m["psnr"], m["ssim"], m["n_pixels"].double(), m["n_windows"].double()), 1).tolist():
                per["psnr"].append(v[0]), per["ssim"].append(v[1])
                per["n_pixels"].append(int(v[2])), per["n_windows"].append(int(v[3]))
            total += len(rgb) * int(rgb[0].shape[0]) * int(rgb[0].shape[1])
        ps = [p for p, k in zip(per["psnr"], per["n_pixels"]) if k > 0]
        ss = [s for s, k in zip(per["ssim"], per["n_windows"]) if k > 0]
        nan = float("nan")
        return dict(psnr=sum(ps) / len(ps) if ps else nan, ssim=sum(ss) / len(ss) if ss else nan,
                    psnr_min=min(ps) if ps else nan, ssim_min=min(ss) if ss else nan,
                    hit_share=sum(per["n_pixels"]) / total, window_share=sum(per["n_windows"]) / total,
                    n_views=n_views, per_view=per)

    def bake_texture(self, mesh=None, K=None, **kw):
        """A texture atlas for a mesh of the map from the keyframes' images: tsdf.bake_texture (DESIGN.md "Mesh
        textures"; `kw`: its further arguments) with the keyframes' T_WC as poses and their `uimg`, read at the
        pointmap's size by the colour fusion's rule (tsdf.global_manager.gather_uimg), as images -> MeshTexture.
        `mesh=None`: self.extract_mesh(colors=...) with the configured chain, with colours where the volume carries them.
        `K` (3,3) or else the system's calibration; with neither it raises, as evaluate_mesh(observed=True) does: a
        texel is projected, and the ray-image camera model has no projection.  The occlusion casts run over a mesh
        index built here unless `index=` says otherwise (the same atlas bit for bit).  Drains the backend first."""
        what = "SlamSystem.bake_texture"
        from mast3r_slam.tsdf import bake_texture

        self.drain()
        K = K if K is not None else self.K
        if K is None:
            raise ValueError(f"{what}: needs a pinhole camera, K or the system's calibration: the ray-image camera "
                             "model has no projection")
        if mesh is None:
            if self.tsdf_manager is None:
                raise RuntimeError(f"{what}: the global TSDF is disabled (tsdf_global.enabled = False); give a mesh")
            mesh = self.extract_mesh(colors=bool(self.tsdf_manager.volume.color))
        n_kf = len(self.keyframes)
        if n_kf == 0:
            raise RuntimeError(f"{what}: no keyframe yet")
        images = [self._keyframe_image(self.keyframes[i], what, i).float() for i in range(n_kf)]
        if any(x.shape != images[0].shape for x in images):
            raise ValueError(f"{what}: the keyframes differ in image size")
        poses = self._keyframe_poses()
        kw.setdefault("index", True)          # the same bytes; a decimated mesh's casts are 3x faster over an index
        if kw.get("density") is None:         # absent or None: the configured one, as mesh_chain.config_defaults does
            mgr = self.tsdf_manager
            cfg = mgr.cfg if mgr is not None else config["tsdf_global"]
            voxel = mgr.volume.voxel_size if mgr is not None else cfg["voxel_size"]
            per_voxel = float(cfg.get("mesh_texture_density", 0.0))
            kw["density"] = per_voxel / float(voxel) if per_voxel > 0.0 else None
        return bake_texture(mesh, torch.stack(images), poses, K, **kw)

    def evaluate_mesh_render(self, mesh, colors=None, texture=None, images=None, poses=None, rays=None, K=None,
                             near=0.05, far=10.0, chunk=8):
        """evaluate_render for a triangle mesh of the map: PSNR and SSIM of its colour views (tsdf.render_mesh_color,
        from vertex `colors` f32[V,3] - True: those of a 4-tensor extract_mesh tuple - or from a `texture` of
        bake_texture; exactly one of the two) against camera images, so that an exported mesh is scored by the figures
        that score the TSDF.  `mesh`: (vertices, faces) device tensors or an extract_mesh tuple.  The training views,
        the held-out views (`images`, `poses`, `rays` / `K`), the mask - the hit image - and the returned dict are
        evaluate_render's.  Drains the backend first."""
        what = "SlamSystem.evaluate_mesh_render"
        from mast3r_slam.tsdf import build_mesh_index, render_mesh_color

        if (colors is None) == (texture is None):
            raise ValueError(f"{what}: give exactly one of colors and texture")
        mesh = tuple(mesh)
        index = build_mesh_index(mesh)                           # validated here; one index serves every view

        def render(pose, r):
            out = render_mesh_color(mesh, pose, colors=colors, texture=texture, near=near, far=far, index=index,
                                    validate=False, **r)
            return out[3], out[2]

        return self._score_views(what, render, images, poses, rays, K, chunk, False)

    def render_view(self, pose=None, rays=None, K=None, hw=None, **kw):
        """Depth / normal view of the global TSDF at this point of the run: (range f32[h,w], normals f32[h,w,3],
        hit bool[h,w]) device tensors (TSDFVolume.render; `kw`: near, far, min_weight, level, step, skip, and - with
        tsdf_global.color on - colors=True for the colour image f32[h,w,3] as a fourth tensor).  Drains the
        backend first, like extract_mesh.  `pose=None`: the newest keyframe's pose.  Without `rays` and `K` the view uses
        the system's intrinsics when it is calibrated and otherwise the newest keyframe's canonical pointmap normalised
        to unit length - the ray model of an uncalibrated camera - so the view lies pixel for pixel over that keyframe."""
        if self.tsdf_manager is None:
            raise RuntimeError("SlamSystem.render_view: the global TSDF is disabled (tsdf_global.enabled = False)")
        self.drain()
        kf = self.keyframes.last_keyframe()
        if kf is None and (pose is None or (rays is None and K is None)):
            raise RuntimeError("SlamSystem.render_view: no keyframe yet; give pose and rays (or K with hw)")
        if pose is None:
            pose = kf.T_WC.data
        view = dict(rays=rays, K=K, hw=hw)
        if rays is None and K is None:
            view.update(self._keyframe_view(kf))
        return self.tsdf_manager.render(pose, **view, **kw)
