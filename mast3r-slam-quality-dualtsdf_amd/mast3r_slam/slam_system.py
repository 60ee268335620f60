"""the reference's process model as ONE process.

main.py runs the tracking frontend (main.py:325-446) and the backend (run_backend, main.py:73-163; relocalization,
main.py:28-71) as two processes that share keyframes through CUDA-IPC buffers, manager locks and 10 ms polling.
`SlamSystem` is the same state machine (Mode.INIT / TRACKING / RELOC, the same calls in the same order) in one
process.  `backend="inline"` (default) has the semantics of the reference's `single_thread: True` evaluation configs
(the backend task of a keyframe is finished before the next frame is tracked, main.py:391-395) and is deterministic;
`backend="thread"` runs the backend on its own host thread and HIP stream beside the tracking loop, as the reference's
second process does: the symmetric edge inference (most of a backend task) overlaps tracking, while everything that
reads or writes keyframe pointmaps / poses (the tracking step on one side; global GN + TSDF hook on the other) runs in
critical sections that hand the data over between the two streams with events instead of locks + polling + IPC copies.
Two more things the split made impossible:

* **frame groups** (`frame_group` = B > 1): the encoder runs B frames ahead on its own stream and the two-view
  forward of the next B frames against the current keyframe is ONE batch call
  (mast3r_utils.mast3r_asymmetric_inference_group).  Matching and tracking stay strictly per frame, in order.  The
  group decode speculates that the keyframe stays: when a frame of the group becomes a keyframe (or tracking falls
  into RELOC) the rest of the group is decoded again against the new keyframe.  Rows of a batch are computed exactly as
  a batch of one, so the trajectory is bit-identical to B = 1 (tests/test_slam_system_gpu.py).
* the keyframe store is whatever the caller passes: `KeyframeStore` (unbounded) or the `SharedKeyframes` mirror.

Retrieval (retrieval_database.py, ASMK) is not available offline; `retriever` is any object with the reference's
`update(frame, add_after_query, k, min_thresh) -> [keyframe ids]`.  The default stand-in proposes no loop-closure edges
and offers the most recent keyframes as relocalisation candidates."""
import contextlib
import os
import queue
import threading
import time

import torch

from lietorch_hip import Sim3
from mast3r_slam import mast3r_utils as mu
from mast3r_slam.config import config
from mast3r_slam.frame import KeyframeStore, Mode
from mast3r_slam.global_opt import FactorGraph
from mast3r_slam.tracker import FrameTracker


class RecentKeyframes:
    """Stand-in for RetrievalDatabase.update: no loop-closure proposals for the graph (add_after_query=True), the
    last `k` keyframes as relocalisation candidates (add_after_query=False)."""

    def __init__(self, keyframes, k=1):
        self.keyframes, self.k = keyframes, k

    def update(self, frame, add_after_query=True, k=3, min_thresh=0.0):
        if add_after_query:
            return []
        n = len(self.keyframes)
        return list(range(max(0, n - self.k), n))[::-1]


class _BackendThread(threading.Thread):
    """One stage of run_backend (main.py:73-163) as a host thread with its own stream.  Tasks are (keyframe index, event
    the stage's stream waits for, payload of the previous stage); `fn(idx, payload)` does the stage's work and its return
    value travels to `next_stage` behind an event recorded on this stage's stream."""

    def __init__(self, system, fn, next_stage=None, priority=0):
        super().__init__(daemon=True)
        self.system, self.fn, self.next_stage, self.priority = system, fn, next_stage, int(priority)
        self.q, self.error = queue.Queue(), None
        self.start()

    def run(self):
        dev = self.system.device
        torch.cuda.set_device(dev)
        with torch.cuda.stream(torch.cuda.Stream(device=dev, priority=self.priority)):
            while True:
                task = self.q.get()
                try:
                    if task is None:
                        return
                    if self.error is None:
                        idx, ev, payload = task
                        stream = torch.cuda.current_stream(dev)
                        stream.wait_event(ev)              # what the task reads was produced on another stream
                        out = self.fn(idx, payload)
                        if self.next_stage is not None:
                            done = torch.cuda.Event()
                            done.record(stream)
                            self.next_stage.q.put((idx, done, out))
                except Exception as e:   # surfaced by drain()
                    self.error = e
                finally:
                    self.q.task_done()

    def drain(self):
        self.q.join()                    # every task of this stage has been handed on before it counts as done
        if self.error is not None:
            raise self.error
        if self.next_stage is not None:
            self.next_stage.drain()

    def stop(self):
        st = self
        while st is not None:
            st.q.put(None)
            st.join(timeout=5.0)
            st = st.next_stage


class SlamSystem:
    def __init__(self, model, device, K=None, keyframes=None, retriever=None, frame_group=1, tsdf_global_cfg=None,
                 encoder_group=None,
                 backend="inline", tsdf_refine_cfg=None, quality_service=None, shard_edges=False, decode_ahead=0,
                 shard_channel=None, pipeline=False, pipeline_depth=1, backend_priority=0, encoder_priority=0,
                 backend_stages=3, solve_priority=0):
        """`shard_channel` (mast3r_slam/shard.py): this process is the DRIVER rank of a session whose backend is sharded
        over the ranks of the channel's group - keyframe-pair inference + matching, the global GN (one all-reduce per
        iteration) and the global TSDF's voxels; the other ranks run BackendShard.serve()."""
        self.model, self.device, self.K = model, torch.device(device), K
        self.keyframes = KeyframeStore() if keyframes is None else keyframes
        self.tracker = FrameTracker(model, self.keyframes, device)
        self.tracker.quality_service = quality_service          # main.py:246
        self.shard_channel = shard_channel
        self.backend_priority = int(backend_priority)      # HIP stream priority of the backend thread's stream (-1 = high)
        self.pipeline = bool(pipeline)
        self.pipeline_depth = min(3, max(1, int(pipeline_depth)))     # FrameTracker keeps 4 solver states
        self.factor_graph = FactorGraph(model, self.keyframes, K, device, shard_edges=shard_edges or shard_channel is not None,
                                        channel=shard_channel)
        self.retriever = RecentKeyframes(self.keyframes) if retriever is None else retriever
        self.tsdf_manager = None
        if tsdf_global_cfg is not None and tsdf_global_cfg.get("enabled", False):   # main.py:78-88
            from mast3r_slam.tsdf import TSDFGlobalManager

            self.tsdf_manager = TSDFGlobalManager(self.keyframes, tsdf_global_cfg, config.get("use_calib", False), device,
                                                  channel=shard_channel)
            self.tsdf_manager.start()
        # the camera-side half of the dual TSDF (main.py:253-287): local block refinement of keyframes that left the
        # sliding window; scheduled and processed by the backend task (synchronous form of the refiner thread)
        self.tsdf_refiner = None
        if tsdf_refine_cfg is not None and tsdf_refine_cfg.get("enabled", False):
            from mast3r_slam.tsdf_refine import TSDFRefiner

            self.tsdf_refiner = TSDFRefiner(tsdf_refine_cfg, self.keyframes, quality_service, device)
            self.tsdf_refiner.edit_section = lambda: self._critical("refine")
            self.tsdf_refiner.start()
        assert backend in ("inline", "thread")
        self._lock = threading.RLock()
        self._bprof = bool(os.environ.get("MSLAM_BACKEND_PROFILE"))
        self._hand = {"main": None, "backend": None, "refine": None}   # event at the end of each party's last critical section
        self._commits = []                              # (solve job, event): optimised poses waiting to be written back
        self._backend_done = None                       # event behind the last backend task (threaded backend)
        # backend="thread", staged (default 3): the graph stage of keyframe k+1 (retrieval + symmetric inference +
        # matching: throughput-bound network launches) runs beside the solve stage of keyframe k (global GN: a dependent
        # chain of short kernels) and the fusion / refinement stage of keyframe k-1 (TSDF hook, local refinement: short
        # launches with host reads in between), each on a thread / stream of its own - the keyframe task's chain (64 ms
        # per keyframe at 60-120 keyframes, of which 27 ms network) was what bound the loop.
        # Every solve still sees exactly the edges of the tasks up to its own (the edge count travels with the task).
        # A sharded session keeps ONE backend thread: its collectives must be issued in one order on every rank.
        self._worker = None
        self._graph_done = None
        if backend == "thread":
            if int(backend_stages) >= 2 and shard_channel is None:
                post = None
                if int(backend_stages) >= 3:     # TSDF fusion + local refinement (host reads) behind the solve, on their own
                    post = _BackendThread(self, lambda idx, payload: self._backend_post(idx, payload), priority=solve_priority)
                solve = _BackendThread(self, lambda idx, n_edges: self._backend_solve(idx, n_edges, hand_on=post is not None),
                                       next_stage=post, priority=solve_priority)
                self._worker = _BackendThread(self, lambda idx, _: self._backend_graph(idx), next_stage=solve,
                                              priority=self.backend_priority)
            else:
                self._worker = _BackendThread(self, lambda idx, _: self._backend(idx), priority=self.backend_priority)
        self.mode = Mode.INIT
        self.last_T = None
        self.frame_group = max(1, int(frame_group))
        # the look-ahead encoder does not depend on any decision of the loop (every frame is encoded exactly once), so
        # its batch may be larger than the speculative decode group: nothing is ever encoded in vain
        self.encoder_group = self.frame_group if encoder_group is None else max(1, int(encoder_group))
        self.enc_stream = torch.cuda.Stream(device=self.device, priority=int(encoder_priority)) if self.frame_group > 1 else None
        self._enc_hi = 0
        self._kf_value, self._kf_slope = None, None      # keyframe-rule value of the last tracked frame, its decay per frame
        self._n_pending = 0                              # frames begun whose verdict is not read yet (pipelined run)
        # decode_ahead = k > 0: the NEXT group's pair decode is issued on a stream of its own as soon as at most k
        # already decoded frames are left in front of the current one, so that it runs beside the per-frame matching /
        # tracking of the current group instead of in front of the next group's first frame (more rows are decoded
        # in vain when the keyframe changes)
        self.decode_ahead = max(0, int(decode_ahead)) if self.frame_group > 1 else 0
        self.dec_stream = torch.cuda.Stream(device=self.device) if self.decode_ahead > 0 else None
        self.stats = dict(frames=0, keyframes=0, group_calls=0, decoded_rows=0, void_rows=0, relocalised=0)

    # ------------------------------------------------------------------ frontend (main.py:325-446)
    def run(self, frames, start=0, stop=None, release=False):
        """Track frames[start:stop] (Frame objects, frame.create_frame) in order; returns the per-frame results of
        step().  A sequence may be fed in several calls over the SAME list (the look-ahead state carries over).
        `release` drops the list's reference to a frame once it has been tracked (keyframes live on in the store), so
        that a long sequence does not keep every pointmap alive.

        `pipeline` (off by default, see below): in TRACKING mode the matching + pose solve of the next `pipeline_depth`
        frames are enqueued BEFORE frame f's verdict is read - on the premise "f is tracked and the keyframe stays" (true
        for ~88 % of the frames) - so the one host wait per frame no longer leaves the tracking stream without work.  When the premise fails (new keyframe, tracking
        lost, a solve that needed more than its first chunk of iterations) f+1 is rolled back (nothing of it has
        reached the keyframe store: FrameTracker keeps the fused keyframe in a shadow copy until the verdict is in) and
        begun again from f's real outcome.  Results are bit-identical to the frame-at-a-time loop.

        MEASURED (1 000-frame stream, same box, DESIGN.md "Round 3: the tracking loop"): the frontend's host work drops
        from 5.7 to 2.0-2.9 ms per frame, but the JOB gets slower (138 -> 133 frames/s at depth 1, 116-126 at depth 2 or with
        one hand-over section per iteration): a tracking stream that never runs dry takes the device away from the
        backend stream, the frontend finishes early and the backend drains its backlog alone - a single dependent
        chain of short kernels with a launch bubble behind each.  The frame-at-a-time loop interleaves the two by
        itself (the device works on the backend while the host reads a verdict), so it stays the default."""
        out = []
        stop = len(frames) if stop is None else min(stop, len(frames))
        self._enc_hi = max(self._enc_hi, start)
        if not self.pipeline:
            for i in range(start, stop):
                if self.frame_group > 1:
                    self._look_ahead(frames, i, stop)
                out.append(self.step(frames[i]))
                if release:
                    frames[i] = None
            return out
        i, pend = start, []                         # pend = [(index, handle)]: begun, verdict not read yet (oldest first)
        while i < stop or pend:
            # run ahead: up to `pipeline_depth` frames begun behind the one whose verdict is read next (the host then
            # has a frame's worth of enqueue time in hand when the device finishes a frame)
            while i < stop and self.mode == Mode.TRACKING and len(pend) <= self.pipeline_depth:
                # speculation that is rarely wrong: the value the keyframe rule compares with its threshold decays
                # steadily (see _speculative_window); when it says that a frame still in flight will replace the
                # keyframe, nothing more is begun (or decoded) behind it until that verdict is in
                self._n_pending = len(pend)
                if pend and not self._premise_holds(len(pend)):
                    break
                if self.frame_group > 1:
                    self._look_ahead(frames, i, stop)
                pend.append((i, self._begin(frames[i])))
                i += 1
            self._n_pending = 0
            if pend:
                k, h = pend.pop(0)
                with self._critical("main"):
                    self.tracker.track_resolve(h)
                    clean = h.kind == "ok" and not h.new_kf and not h.replayed
                    if pend and not clean:              # the premise of everything begun behind it failed: undo, newest first
                        for _, hh in reversed(pend):
                            self.tracker.rollback(hh)
                        self.stats["replayed_frames"] = self.stats.get("replayed_frames", 0) + len(pend)
                        i = pend[0][0]
                        pend = []
                    res, add_new_kf = self._end(h)
                if add_new_kf:
                    self._queue_backend(len(self.keyframes) - 1)
                if not pend:
                    self.last_T = h.frame.T_WC
                out.append(res)
                if release:
                    frames[k] = None
            elif i < stop and self.mode != Mode.TRACKING:      # INIT / RELOC: frame at a time
                if self.frame_group > 1:
                    self._look_ahead(frames, i, stop)
                out.append(self.step(frames[i]))
                if release:
                    frames[i] = None
                i += 1
        return out

    def _begin(self, frame):
        """First half of step() for a frame in TRACKING mode: everything enqueued, verdict not read."""
        self._wait_encoded(frame)
        self._wait_decoded(frame)
        if self.last_T is not None:
            frame.T_WC = Sim3(self.last_T.data.clone())
        with self._critical("main"):
            self._apply_commits()
            h = self.tracker.track_begin(frame)
        self.last_T = frame.T_WC                    # optimistic: the next frame starts from this one's solved pose
        return h

    def _end(self, h):
        """Second half (inside the hand-over section): the verdict's consequences -> (step()'s result dict, new_kf)."""
        frame = h.frame
        self.stats["frames"] += 1
        add_new_kf, _, try_reloc = self.tracker.track_finish(h)
        if try_reloc:
            self.mode = Mode.RELOC
        self._note_keyframe_rule(add_new_kf or try_reloc)
        if add_new_kf:
            self.keyframes.append(frame)
            self.stats["keyframes"] += 1
        return (dict(mode=Mode.TRACKING, new_kf=bool(add_new_kf), try_reloc=bool(try_reloc), pose=frame.T_WC.data.clone()),
                bool(add_new_kf))

    def finish(self):
        """End of the sequence (main.py:449-560): drain the backend, then the local refiner's final pass over the
        keyframes still inside its window."""
        self.drain()
        if self.tsdf_refiner is not None and len(self.keyframes) > 0:
            with self._critical("main"):
                self.tsdf_refiner.schedule_final_pass(len(self.keyframes) - 1)
                self.tsdf_refiner.process_queue()

    def step(self, frame):
        """One iteration of the main loop for an already created frame -> dict(mode, new_kf, try_reloc, pose) with
        `pose` = the frame's T_WC data as tracked (before any later backend update of a keyframe copy)."""
        self._wait_encoded(frame)
        self._wait_decoded(frame)
        if self.last_T is not None:                     # "last camera pose for the frame" (main.py:351-356)
            frame.T_WC = Sim3(self.last_T.data.clone())
        self.stats["frames"] += 1
        add_new_kf = try_reloc = False
        mode = self.mode
        if mode == Mode.RELOC and self._worker is not None:
            self._worker.drain()                        # relocalisation edits the factor graph: the backend must be idle
            self._adopt_backend_tensors()
        with self._critical("main"):
            self._apply_commits(wait=(mode == Mode.RELOC))
            if mode == Mode.INIT:                       # main.py:359-367
                X_init, C_init = mu.mast3r_inference_mono(self.model, frame)
                frame.update_pointmap(X_init, C_init)
                add_new_kf = True
                self.mode = Mode.TRACKING
            elif mode == Mode.TRACKING:                 # main.py:369-373
                h = self.tracker.track_begin(frame)
            elif mode == Mode.RELOC:                    # main.py:375-385
                self.tracker._shadow = None             # whatever comes next is tracked against the store's keyframe
                X, C = mu.mast3r_inference_mono(self.model, frame)
                frame.update_pointmap(X, C)
                if self._relocalization(frame):
                    self.mode = Mode.TRACKING
                    self.stats["relocalised"] += 1
            else:
                raise Exception("Invalid mode")
            if mode != Mode.TRACKING:
                self.last_T = frame.T_WC
                if add_new_kf:                          # main.py:387-395
                    self.keyframes.append(frame)
                    self.stats["keyframes"] += 1
        if mode == Mode.TRACKING:
            # the one host wait of a tracked frame happens OUTSIDE the hand-over section: the backend's solve stage can copy
            # keyframe data out (or write poses back) while this thread sleeps on the verdict
            self.tracker.track_resolve(h)
            with self._critical("main"):
                add_new_kf, _, try_reloc = self.tracker.track_finish(h)
                if try_reloc:
                    self.mode = Mode.RELOC
                self._note_keyframe_rule(add_new_kf or try_reloc)
                self.last_T = frame.T_WC
                if add_new_kf:                          # main.py:387-395
                    self.keyframes.append(frame)
                    self.stats["keyframes"] += 1
        if add_new_kf:
            self._queue_backend(len(self.keyframes) - 1)
        return dict(mode=mode, new_kf=bool(add_new_kf), try_reloc=bool(try_reloc), pose=frame.T_WC.data.clone())

    def drain(self):
        """Wait until every queued backend task has been issued and its poses are written back (backend="thread")."""
        if self._worker is not None:
            self._worker.drain()
            main = torch.cuda.current_stream(self.device)
            for ev in (self._backend_done, self._graph_done, self._hand["backend"], self._hand["refine"]):
                if ev is not None:           # the stages' last launches (the refiner's edits, the edge lists) lie
                    main.wait_event(ev)      # behind their last hand-over sections
            with self._critical("main"):
                self._apply_commits(wait=True)

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
        `align_kw`: further arguments of tsdf.align_meshes.

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
            K = gt_K if gt_K is not None else self.K
            n_kf = len(self.keyframes)
            if K is None:
                raise ValueError("SlamSystem.evaluate_mesh: observed=True needs a pinhole camera, gt_K or the system's "
                                 "calibration: the ray-image camera model has no projection")
            if n_kf == 0:
                raise RuntimeError("SlamSystem.evaluate_mesh: observed=True needs at least one keyframe")
            poses = torch.stack([self.keyframes[i].T_WC.data.reshape(8) for i in range(n_kf)])
            hw = tuple(int(x) for x in self.keyframes[n_kf - 1].img_shape.reshape(-1)[:2].tolist())
            kw["observed"] = dict(poses=poses, K=K, hw=hw, frame="pred")
        if index is not None and index is not False:
            kw["index"] = index
        return compare_meshes(mesh, (gt_vertices, gt_faces), n_samples=n_samples, threshold=threshold,
                              _validate_pred=False, **kw)

    def keyframe_cloud(self, conf_threshold=None, voxel=None, colors=True, outliers=None, normals=None):
        """The map as a point cloud at this point of the run, on the device: what evaluate.save_reconstruction gathers -
        for every keyframe the world points T_WC.act(X_canon) (with calibration: X_canon constrained to the pixel rays
        first) of the pixels whose average confidence is > `conf_threshold` (default tracking.C_conf of the config), in
        keyframe order -> (points f32[N,3], colors u8[N,3] or None).  `voxel`: the cloud is then thinned by
        tsdf.downsample_cloud on that grid (centroids and mean colours, in key order).  `colors=False`: no colours.
        Drains the backend first, so the poses are the ones it has solved.  `outliers`: a dict of keyword arguments for
        tsdf.cloud_outliers, applied after `voxel`; the points it drops leave the cloud.  `normals`: k - a third return
        value, tsdf.cloud_normals(points, k) turned towards the camera centre of the keyframe each point came from
        (after thinning: the keyframe of the cell's lowest-index member).  With both None the pair is what it was."""
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
        if outliers is None and normals is None:
            if voxel is not None:
                from mast3r_slam.tsdf import downsample_cloud

                points, color, _ = downsample_cloud(points, voxel, color)
            return points, color
        from mast3r_slam.tsdf import cloud_normals, downsample_cloud, filter_cloud

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
        if normals is None:
            return points, color
        centres = (torch.stack([c for _, c in source]) if source else
                   torch.zeros((0, 3), dtype=torch.float32, device=self.device))
        viewpoint = centres[kf_of].contiguous() if int(points.shape[0]) else None
        return points, color, cloud_normals(points, normals, viewpoint=viewpoint)[0]

    def evaluate_cloud(self, gt_points, threshold=None, voxel=None, align=None, init=None, gt_positions=None,
                       align_kw=None, index=None, conf_threshold=None, outliers=None, normals=None, observed=False,
                       gt_K=None):
        """Quality of the map's point cloud (self.keyframe_cloud(conf_threshold)) against a ground-truth cloud gt_points
        f32[N,3] (a numpy array or a device tensor; a laser scan needs no faces): the dict of tsdf.compare_clouds
        (DESIGN.md "Point clouds").  `threshold` and `voxel` default to the global TSDF's voxel size (the config's when
        the global TSDF is off): both clouds are thinned on the map's own grid and a point counts as right within one
        cell; voxel=0 scores the raw clouds.  `align`, `init` ("trajectory" with `gt_positions` for
        self.align_trajectory), `align_kw` and `index` (None or True) as in evaluate_mesh, with tsdf.align_clouds in the
        place of align_meshes.  `outliers`: a dict for tsdf.cloud_outliers, applied to the map's raw cloud first
        (keyframe_cloud); `normals`: k, for compare_clouds' normal-consistency figures.

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
        points, _ = self.keyframe_cloud(conf_threshold, colors=False, outliers=outliers)
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

    def _keyframe_pinholes(self, what, gt_K, asked):
        """(K, the keyframes' poses [n,8], (h, w) of the newest keyframe) for the cloud views; K is `gt_K` or else the
        system's calibration.  Raises without a pinhole and without a keyframe."""
        K = gt_K if gt_K is not None else self.K
        n_kf = len(self.keyframes)
        if K is None:
            raise ValueError(f"{what}: {asked} needs a pinhole camera, gt_K or the system's calibration: the ray-image "
                             "camera model has no projection")
        if n_kf == 0:
            raise RuntimeError(f"{what}: {asked} needs at least one keyframe")
        poses = torch.stack([self.keyframes[i].T_WC.data.reshape(8) for i in range(n_kf)])
        hw = tuple(int(x) for x in self.keyframes[n_kf - 1].img_shape.reshape(-1)[:2].tolist())
        return K, poses, hw

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
        from mast3r_slam.tsdf.mesh_raycast import compose_sim3

        self.drain()
        K, poses, _ = self._keyframe_pinholes(what, gt_K, "a cloud view")
        gt = torch.as_tensor(gt_points, dtype=torch.float32).to(self.device).reshape(-1, 3).contiguous()
        T = None if align is None else torch.as_tensor(getattr(align, "data", align)).detach().double().cpu().reshape(8)
        a_scale = 1.0 if T is None else float(T[7])
        if point_size is None:
            point_size = 2.0 * float(self.tsdf_manager.volume.voxel_size) * a_scale
        diffs, n_pixels = [], 0
        for i in range(len(self.keyframes)):
            kf = self.keyframes[i]
            hw = tuple(int(x) for x in kf.img_shape.reshape(-1)[:2].tolist())
            pose = kf.T_WC.data.detach().reshape(8)
            moved = pose.double().cpu() if T is None else compose_sim3(T, pose.double().cpu().reshape(1, 8))[0]
            r_map, _, hit_map = self.tsdf_manager.render(pose, near=near / a_scale, far=far / a_scale, K=K, hw=hw)[:3]
            r_gt, _, hit_gt = render_cloud(gt, moved, K, hw, near=near, far=far, point_size=point_size)
            both = hit_map & hit_gt
            diffs.append((r_map.double() - r_gt.double()).abs()[both] * float(moved[7]))
            n_pixels += hw[0] * hw[1]
        d = torch.sort(torch.cat(diffs))[0]
        m = int(d.numel())
        l1, med = (float("nan"),) * 2 if m == 0 else torch.stack((d.sum() / m, 0.5 * (d[(m - 1) // 2] + d[m // 2]))).tolist()
        return dict(depth_l1=l1, depth_l1_median=med, both_hit_share=m / n_pixels, n_pixels=n_pixels)

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
        from mast3r_slam.tsdf.mesh_raycast import compose_sim3

        self.drain()
        n_kf = len(self.keyframes)
        if n_kf == 0:
            raise RuntimeError("SlamSystem.evaluate_depth: no keyframe yet")
        gt = (torch.as_tensor(gt_vertices, dtype=torch.float32).to(self.device),
              torch.as_tensor(gt_faces, dtype=torch.int32).to(self.device))
        index = _index_arg(MeshIndex, index, "SlamSystem.evaluate_depth", *gt)
        T = None if align is None else torch.as_tensor(getattr(align, "data", align)).detach().double().cpu().reshape(8)
        a_scale = 1.0 if T is None else float(T[7])
        diffs, n_pixels = [], 0
        for i in range(n_kf):
            kf = self.keyframes[i]
            h, w = (int(x) for x in kf.img_shape.reshape(-1)[:2].tolist())
            pose = kf.T_WC.data.detach().reshape(8)
            if config["use_calib"] and self.K is not None:
                view = dict(K=self.K, hw=(h, w))
            else:
                X = kf.X_canon.detach().reshape(h, w, 3).float()
                view = dict(rays=X / X.norm(dim=-1, keepdim=True).clamp_min(1.0e-12))
            moved = pose.double().cpu() if T is None else compose_sim3(T, pose.double().cpu().reshape(1, 8))[0]
            r_map, _, hit_map = self.tsdf_manager.render(pose, near=near / a_scale, far=far / a_scale, **view)[:3]
            r_gt, _, hit_gt = render_mesh(gt, moved, near=near, far=far, validate=i == 0, index=index, **view)
            both = hit_map & hit_gt
            diffs.append((r_map.double() - r_gt.double()).abs()[both] * float(moved[7]))
            n_pixels += h * w
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
        from mast3r_slam.tsdf.global_manager import gather_uimg

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
            poses = torch.as_tensor(getattr(poses, "data", poses)).detach().reshape(-1, 8)
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
            H, W = (int(x) for x in kf.img_shape.reshape(-1)[:2].tolist())
            if config["use_calib"] and self.K is not None:
                r = dict(K=self.K, hw=(H, W))
            else:
                X = kf.X_canon.detach().reshape(H, W, 3).float()
                r = dict(rays=X / X.norm(dim=-1, keepdim=True).clamp_min(1.0e-12))
            if kf.uimg is None:
                raise ValueError(f"{what}: keyframe {i} has no uimg to compare with")
            pixels = torch.arange(H * W, device=self.device)
            return kf.T_WC.data.detach().reshape(8), r, gather_uimg(kf.uimg.detach(), pixels, (H, W)).reshape(H, W, 3)

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
        from mast3r_slam.tsdf.global_manager import gather_uimg

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
        images = []
        for i in range(n_kf):
            kf = self.keyframes[i]
            if kf.uimg is None:
                raise ValueError(f"{what}: keyframe {i} has no uimg to bake")
            H, W = (int(x) for x in kf.img_shape.reshape(-1)[:2].tolist())
            pixels = torch.arange(H * W, device=self.device)
            images.append(gather_uimg(kf.uimg.detach(), pixels, (H, W)).reshape(H, W, 3).float())
        if any(x.shape != images[0].shape for x in images):
            raise ValueError(f"{what}: the keyframes differ in image size")
        poses = torch.stack([self.keyframes[i].T_WC.data.detach().reshape(8) for i in range(n_kf)])
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
        if rays is None and K is None:
            h, w = (int(x) for x in kf.img_shape.reshape(-1)[:2].tolist())
            if config["use_calib"] and self.K is not None:
                K, hw = self.K, (h, w)
            else:
                X = kf.X_canon.detach().reshape(h, w, 3).float()
                rays = X / X.norm(dim=-1, keepdim=True).clamp_min(1.0e-12)
        return self.tsdf_manager.render(pose, rays=rays, K=K, hw=hw, **kw)

    def _adopt_backend_tensors(self):
        """Relocalisation (main.py:28-71) edits and solves the factor graph on the TRACKING stream, but its tensors were
        allocated and last written on the backend stream: the tracking stream first waits for everything the (now idle)
        backend thread has enqueued, and the caching allocator is told that these blocks are in use on this stream too."""
        main = torch.cuda.current_stream(self.device)
        for ev in (self._backend_done, self._graph_done):
            if ev is not None:
                main.wait_event(ev)
        fg = self.factor_graph
        for t in (fg.ii, fg.jj, fg.idx_ii2jj, fg.idx_jj2ii, fg.valid_match_j, fg.valid_match_i, fg.Q_ii2jj, fg.Q_jj2ii):
            if t.is_cuda and t.numel():
                t.record_stream(main)

    def _apply_commits(self, wait=False):
        """Threaded backend: the global GN runs on copies, outside the hand-over lock; its poses are written into the
        store HERE, by the tracking side on its own stream, once the solve has finished on the device (the reference's
        backend process writes them whenever it is done, main.py:145-164 - the frontend never waits for a solve).
        Always called inside a hand-over section (the backend calls it too, in front of the TSDF pose optimiser)."""
        while self._commits:
            job, ev = self._commits[0]
            if not wait and not ev.query():
                return
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            for t in job.values():      # allocated on the backend's stream, read here on this one: without the note the
                if torch.is_tensor(t) and t.is_cuda:   # caching allocator hands the block back to the backend the moment
                    t.record_stream(cur)               # the job is dropped, while this stream's copy is still queued
            self.factor_graph.commit_solve(job)
            self._commits.pop(0)

    def shutdown(self):
        if self._worker is not None:
            self._worker.drain()
            self._worker.stop()
            self._worker = None
        if self.tsdf_manager is not None:
            self.tsdf_manager.shutdown()

    @contextlib.contextmanager
    def _critical(self, me):
        """Section that reads or writes keyframe pointmaps / poses.  Inline backend: nothing to do.  Threaded backend:
        one party at a time (host lock; parties: "main" = tracking, "backend" = the solve stage, "refine" = the fusion /
        refinement stage), and the entering party's stream first waits for the events the OTHER parties recorded when they
        left their last sections, so data written on one stream is visible to the others."""
        if self._worker is None:
            yield
            return
        with self._lock:
            stream = torch.cuda.current_stream(self.device)
            for other, ev in self._hand.items():
                if other != me and ev is not None:
                    stream.wait_event(ev)
            try:
                yield
            finally:
                ev = torch.cuda.Event()
                ev.record(stream)
                self._hand[me] = ev

    def _queue_backend(self, idx):
        if self._worker is None:
            self._backend(idx)
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._worker.q.put((idx, ev, None))

    # ------------------------------------------------------------------ frame groups
    def _note_keyframe_rule(self, changed):
        """Bookkeeping for the size of the next speculative decode: the value the keyframe rule compares with its
        threshold (tracker.py:170-177) falls steadily while the camera moves away from the keyframe; its decay per frame
        says how many more frames the keyframe is likely to last."""
        v = self.tracker.last_kf_value
        if changed or v is None:
            self._kf_value = None
            return
        if self._kf_value is not None:
            d = max(self._kf_value - v, 0.0)
            self._kf_slope = d if self._kf_slope is None else 0.5 * self._kf_slope + 0.5 * d
        self._kf_value = v

    def _speculative_window(self, B, already=0):
        """Frames worth decoding against the current keyframe in one call: all B right behind a keyframe change, fewer
        when the keyframe rule is about to fire (rows decoded against a keyframe that is replaced are wasted; results do
        not depend on the grouping).  `already` = frames in front of the call that are decoded but not tracked yet
        (look-ahead calls): they use up part of what the keyframe is expected to last."""
        if self._kf_value is None or not self._kf_slope or self._kf_slope <= 0.0:
            return B if already == 0 else 0      # nothing known yet: no speculation beyond the current group
        left = (self._kf_value - config["tracking"]["match_frac_thresh"]) / self._kf_slope
        n = min(B, int(left) - already)
        return max(1, n) if already == 0 else max(0, n)

    def _premise_holds(self, in_flight):
        """Are the `in_flight` frames whose verdict is still out all predicted to leave the keyframe in place?  (The same
        prediction that sizes the group decode; unknown decay = right behind a keyframe change: no.)"""
        if self._kf_value is None or not self._kf_slope or self._kf_slope <= 0.0:
            return False
        left = (self._kf_value - config["tracking"]["match_frac_thresh"]) / self._kf_slope
        return in_flight <= int(left)

    def _wait_encoded(self, frame, stream=None, keep=False):
        ev = getattr(frame, "enc_event", None)
        if ev is not None:
            stream = torch.cuda.current_stream(self.device) if stream is None else stream
            stream.wait_event(ev)
            frame.feat.record_stream(stream)
            frame.pos.record_stream(stream)
            if not keep:
                frame.enc_event = None

    def _wait_decoded(self, frame):
        ev = getattr(frame, "dec_event", None)
        if ev is not None:
            main = torch.cuda.current_stream(self.device)
            main.wait_event(ev)
            stash = getattr(frame, "decoded", None)
            if stash is not None:
                for t in stash[1]:
                    t.record_stream(main)
            frame.dec_event = None

    def _look_ahead(self, frames, i, stop=None):
        B, n = self.frame_group, (len(frames) if stop is None else stop)
        EB = max(B, self.encoder_group)
        main = torch.cuda.current_stream(self.device)
        while self._enc_hi < min(n, i + EB + B):         # encoder: groups of EB, at least one decode group ahead of frame i
            grp = [frames[k] for k in range(self._enc_hi, min(n, self._enc_hi + EB))]
            self.enc_stream.wait_stream(main)            # the images were produced on the caller's stream
            with torch.cuda.stream(self.enc_stream):
                mu.encode_frames(self.model, grp)
                ev = torch.cuda.Event()
                ev.record()
            for f in grp:
                f.enc_event = ev
            self._enc_hi += len(grp)
        if self.mode != Mode.TRACKING:
            return
        keyframe = self.keyframes.last_keyframe()
        kid = int(keyframe.frame_id)

        def decoded(k):
            stash = getattr(frames[k], "decoded", None)
            return stash is not None and stash[0] == kid

        h = i - 1                                        # last frame of the run of frames decoded against this keyframe
        while h + 1 < n and decoded(h + 1):
            h += 1
        if h < i:
            lo = i                                       # the current frame itself is missing: it has to wait
        elif self.decode_ahead > 0 and h - i < self.decode_ahead and h + 1 < n:
            lo = h + 1                                   # few left: the next group, beside this one's tracking
        else:
            return
        # frames begun but not resolved yet (pipelined run) use up part of what the keyframe is expected to last, too
        window = [frames[k] for k in range(lo, min(n, lo + self._speculative_window(B, lo - i + self._n_pending)))]
        if not window and lo == i:
            window = [frames[i]]                         # the frame about to be tracked itself
        if not window:
            return
        for f in window:
            if getattr(f, "decoded", None) is not None:  # decoded against a keyframe that has been replaced since
                self.stats["void_rows"] += 1
        if self.dec_stream is None:
            for f in window:
                self._wait_encoded(f)
            mu.mast3r_asymmetric_inference_group(self.model, window, keyframe)
        else:
            self.dec_stream.wait_stream(main)            # the keyframe (and its features) exist on the tracking stream
            for f in window:
                self._wait_encoded(f, self.dec_stream, keep=True)
            with torch.cuda.stream(self.dec_stream):
                mu.mast3r_asymmetric_inference_group(self.model, window, keyframe)
                ev = torch.cuda.Event()
                ev.record()
            for f in window:
                f.dec_event = ev
        self.stats["group_calls"] += 1
        self.stats["decoded_rows"] += len(window)

    # ------------------------------------------------------------------ backend (main.py:73-163, 28-71)
    def _phase(self, name, t0):
        """MSLAM_BACKEND_PROFILE=1 (diagnostic): wall time per backend phase, each closed by a stream synchronise - what
        the keyframe task's dependent chain costs, phase by phase, beside a running frontend."""
        if not self._bprof:
            return t0
        torch.cuda.current_stream(self.device).synchronize()
        t1 = time.perf_counter()
        acc = self.stats.setdefault("backend_phase_s", {})
        acc[name] = acc.get(name, 0.0) + (t1 - t0)
        return t1

    def _backend(self, idx):
        """The body of run_backend's loop for the keyframe `idx` (graph construction, global GN, TSDF hook)."""
        self._backend_solve(idx, self._backend_graph(idx))

    def _backend_graph(self, idx):
        """First half of the keyframe task (main.py:118-143): retrieval, symmetric edge inference + matching, the new
        edges appended -> the number of edges the graph holds with this task's (the solve of this task uses those)."""
        t0 = time.perf_counter()
        kf_idx = []
        n_consec = 1
        for j in range(min(n_consec, idx)):
            kf_idx.append(idx - 1 - j)
        frame = self.keyframes[idx]
        retrieval_inds = self.retriever.update(frame, add_after_query=True, k=config["retrieval"]["k"],
                                               min_thresh=config["retrieval"]["min_thresh"])
        kf_idx += retrieval_inds
        kf_idx = set(kf_idx)
        kf_idx.discard(idx)
        kf_idx = list(kf_idx)
        frame_idx = [idx] * len(kf_idx)
        t0 = self._phase("retrieval", t0)
        if kf_idx:   # symmetric edge inference + matching: reads only the keyframes' (immutable) features
            self.factor_graph.add_factors(kf_idx, frame_idx, config["local_opt"]["min_match_frac"])
        self._phase("add_factors", t0)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.device))
        self._graph_done = done
        return self.factor_graph.n_edges

    def _backend_solve(self, idx, n_edges, hand_on=False):
        """Second half (main.py:145-163): global GN over the graph as it stood when this keyframe's edges had been added;
        then (or on the next stage's thread, `hand_on`) the TSDF hook and the local refinement (_backend_post)."""
        t0 = time.perf_counter()
        kind = "calib" if config["use_calib"] else "rays"
        if self._worker is None:     # inline: the reference's single_thread order, everything in sequence
            self._solve()
            t0 = self._phase("solve", t0)
            if self.tsdf_manager is not None:
                self.tsdf_manager.on_after_backend_solve(self.factor_graph)
            t0 = self._phase("tsdf", t0)
            self._refine(idx)
            self._phase("refine", t0)
            return None
        # threaded: the lock (and with it the tracking stream) is held only while keyframe data is copied out; the
        # solve and the fusions run on the copies; the poses are written back by the tracking side (_apply_commits)
        mgr = self.tsdf_manager
        with self._critical("backend"):
            t0 = self._phase("lock_wait", t0)
            job = self.factor_graph.prepare_solve(kind, n_edges=n_edges)
            if job is not None:
                self._chain_pending_poses(job)
            plan = mgr.plan(self.factor_graph) if mgr is not None else None
            t0 = self._phase("prepare+plan", t0)
        if job is not None:
            self.factor_graph.run_solve(job)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            with self._lock:
                self._commits.append((job, ev))
        self._phase("solve", t0)
        payload = (plan, job)
        if hand_on:
            return payload
        self._backend_post(idx, payload)
        return None

    def _backend_post(self, idx, payload):
        """The TSDF hook of the keyframe task (fusions at the poses its solve produced) and the local refinement
        (main.py:403-421).  With three backend stages this runs on a thread / stream of its own: both are chains of short
        launches with host reads in between, which would otherwise hold up the next solve."""
        t0 = time.perf_counter()
        plan, job = payload
        mgr = self.tsdf_manager
        cur = torch.cuda.current_stream(self.device)
        if plan is not None:
            for _, _, snap in plan["todo"]:        # copies taken on the solve stage's stream, read (and dropped) here
                for t in (snap or ()):
                    if torch.is_tensor(t) and t.is_cuda:
                        t.record_stream(cur)
            if job is not None:      # the fusions use the poses THIS solve produced, as the inline order does
                job["pose_data"].record_stream(cur)
                mgr.retarget(plan, job["unique_kf_idx_host"], job["pose_data"])
            if not mgr.has_pose_refinement(plan):
                mgr.execute(plan)            # fusions only: on the copies, outside the lock
            else:
                # the TSDF pose optimiser reads and writes keyframe poses in the store: inside the hand-over section,
                # behind this solve's own write-back (rare configuration: the tracking stream waits for the solve here)
                with self._critical("refine"):
                    self._apply_commits(wait=True)
                    mgr.execute(plan)
        t0 = self._phase("tsdf", t0)
        if self.tsdf_refiner is not None:
            # the refiner works on keyframes that have LEFT the sliding window (the tracking side reads and replaces only
            # the newest one): no section around the whole pass - an empty one orders this stream behind the other parties'
            # last writes (poses), and the refiner's in-place edit of a keyframe is a section of its own (edit_section)
            with self._critical("refine"):
                pass
            self._refine(idx)
            t0 = self._phase("refine", t0)
        done = torch.cuda.Event()
        done.record(cur)
        self._backend_done = done

    def _chain_pending_poses(self, job):
        """A solve whose result is still waiting in `_commits` (the tracking side writes it into the store when it gets
        there) has not reached the store this job's poses were copied from: take its poses - they were produced on
        this (the backend's) stream, so stream order makes them visible - for every keyframe both solves hold.  Called
        under the hand-over lock.  Without it solve N+1 restarts from pre-N poses and later overwrites N's result."""
        cur = {int(k): r for r, k in enumerate(job["unique_kf_idx_host"].tolist())}
        for prev, _ in self._commits:
            pin = prev["pin"]
            ids = prev["unique_kf_idx_host"].tolist()
            src = [r for r in range(pin, len(ids)) if int(ids[r]) in cur]
            if not src:
                continue
            dst = [cur[int(ids[r])] for r in src]
            dev = job["pose_data"].device
            job["pose_data"][torch.tensor(dst, device=dev)] = prev["pose_data"][torch.tensor(src, device=dev)]

    def _refine(self, idx):
        if self.tsdf_refiner is not None:      # main.py:403-421, after the backend task of the keyframe
            self.tsdf_refiner.registry.tick()
            self.tsdf_refiner.maybe_schedule_sliding_window(idx)
            self.stats["refine_blocks"] = self.stats.get("refine_blocks", 0) + self.tsdf_refiner.process_queue()

    def _solve(self):
        if config["use_calib"]:
            self.factor_graph.solve_GN_calib()
        else:
            self.factor_graph.solve_GN_rays()

    def _relocalization(self, frame):
        """main.py:28-71."""
        kf_idx = list(self.retriever.update(frame, add_after_query=False, k=config["retrieval"]["k"],
                                            min_thresh=config["retrieval"]["min_thresh"]))
        success = False
        if kf_idx:
            self.keyframes.append(frame)
            n_kf = len(self.keyframes)
            frame_idx = [n_kf - 1] * len(kf_idx)
            if self.factor_graph.add_factors(frame_idx, kf_idx, config["reloc"]["min_match_frac"],
                                             is_reloc=config["reloc"]["strict"]):
                self.retriever.update(frame, add_after_query=True, k=config["retrieval"]["k"],
                                      min_thresh=config["retrieval"]["min_thresh"])
                success = True
                kf = self.keyframes[n_kf - 1]
                kf.T_WC = Sim3(self.keyframes[kf_idx[0]].T_WC.data.clone())
                self.keyframes[n_kf - 1] = kf
                self.stats["keyframes"] += 1
            else:
                self.keyframes.pop_last()
        if success:
            self._solve()
        return success
