/*
 * mslam_hip.h — C ABI of libmslam_hip.so, the MI355X (gfx950) implementation of the per-frame
 * SLAM compute path of MASt3R-SLAM (dual-TSDF fork).
 *
 * Every entry point takes plain device pointers + sizes (no torch types) and a HIP stream
 * (`void* stream` is a hipStream_t; NULL = the null stream).  All pointers are DEVICE pointers
 * unless the parameter name ends in `_host`.  Every function returns 0 on success or a negative
 * MSLAM_E* code; mslam_last_error() returns a human-readable message for the calling thread.
 * Nothing here allocates device memory or synchronises the stream unless documented, so every
 * call can be captured into a hipGraph.
 *
 * Each declaration cites the reference interface it replaces (paths relative to the reference
 * repository root).  The Python binding a maintainer adds is shown in INTEGRATION.md.
 *
 * This header is also READ AT RUN TIME by mslam_hip.py, which takes every ctypes signature from it (there is no second
 * copy to keep in step).  So it holds plain C declarations only, one per `;`: `<ret> mslam_<name>(<params>);` with <ret>
 * one of int, size_t, const char*; a by-value parameter is named and of type int, float, double, size_t, long long,
 * int64_t, uint64_t or uint32_t; any parameter with a `*` is passed as an address.  Anything else (another scalar type, a
 * by-value struct, a function pointer, a typedef, a multi-line macro) makes the binding refuse to load.
 */
#ifndef MSLAM_HIP_H
#define MSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSLAM_OK 0
#define MSLAM_EINVAL (-1)    /* bad argument (shape / null pointer / unsupported size) */
#define MSLAM_EHIP (-2)      /* HIP runtime error (message in mslam_last_error) */
#define MSLAM_ENOMEM (-3)    /* workspace / table too small */
#define MSLAM_ENODEV (-4)    /* no gfx950 device */

const char* mslam_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int mslam_abi_version(void);
/* Returns 0 when a gfx950 device is present and usable, MSLAM_ENODEV otherwise. */
int mslam_device_check(void);

/* ------------------------------------------------------------------------------------------
 * Matching  (pybind `mast3r_slam_backends`, mast3r_slam/backend/src/gn.cpp:116-123)
 * ------------------------------------------------------------------------------------------ */

/* Replaces iter_proj(rays_img_with_grad, pts_3d_norm, p_init, max_iter, lambda_init, cost_thresh)
 *   binding   mast3r_slam/backend/src/gn.cpp:84-99
 *   launcher  mast3r_slam/backend/src/matching_kernels.cu:279-316
 *   kernel    mast3r_slam/backend/src/matching_kernels.cu:119-275
 * rays_img_with_grad f32[b,h,w,9], pts_3d_norm f32[b,n,3], p_init f32[b,n,2]
 *   -> p_new f32[b,n,2], converged u8[b,n] (torch.bool storage). */
int mslam_iter_proj(const float* rays_img_with_grad, const float* pts_3d_norm,
                    const float* p_init, float* p_new, uint8_t* converged, int b, int h, int w,
                    int n, int max_iter, float lambda_init, float cost_thresh, void* stream);

/* Replaces refine_matches(D11, D21, p1, radius, dilation_max)
 *   binding   mast3r_slam/backend/src/gn.cpp:101-114
 *   launcher  mast3r_slam/backend/src/matching_kernels.cu:84-116
 *   kernel    mast3r_slam/backend/src/matching_kernels.cu:25-81
 * D11 f16[b,h,w,fdim], D21 f16[b,n,fdim] (IEEE binary16 bits), p1 i64[b,n,2] -> p1_new i64[b,n,2]. */
int mslam_refine_matches(const uint16_t* D11, const uint16_t* D21, const int64_t* p1,
                         int64_t* p1_new, int b, int h, int w, int n, int fdim, int radius,
                         int dilation_max, void* stream);

/* Replaces prep_for_iter_proj + img_gradient (mast3r_slam/matching.py:25-49,
 * mast3r_slam/image.py:5-38) as ONE kernel: rays = normalize(X11), Scharr-like x/y gradients with
 * reflect padding, channel concat; pts_3d_norm = normalize(X21); p_init from idx_init (i64[b,n],
 * may be NULL = identity mapping).  X11,X21 f32[b,h,w,3]. */
int mslam_prep_iter_proj(const float* X11, const float* X21, const int64_t* idx_init,
                         float* rays_img_with_grad, float* pts_3d_norm, float* p_init, int b, int h,
                         int w, void* stream);

/* Replaces the occlusion test + pixel_to_lin of match_iterative_proj
 * (mast3r_slam/matching.py:68-76,87-90): p1 = trunc(p) ; valid &= |X11[p1]-X21| < dist_thresh.
 * p f32[b,n,2] -> p1 i64[b,n,2]; valid u8[b,n] in/out (converged flags in, valid_proj2 out). */
int mslam_match_occlusion(const float* X11, const float* X21, const float* p, int64_t* p1,
                          uint8_t* valid, int b, int h, int w, float dist_thresh, void* stream);

/* idx = u + w*v  (mast3r_slam/matching.py:13-15). p1 i64[b,n,2] -> idx i64[b,n]. */
int mslam_pixel_to_lin(const int64_t* p1, int64_t* idx, int b, int n, int w, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gauss-Newton backend  (pybind gauss_newton_{rays,calib,points}, gn.cpp:3-82;
 *                        host loops gn_kernels.cu:725-811, 1140-1228, 1546-1638)
 *
 * Shapes: Twc f32[P,8] ([t,q(xyzw),s], UPDATED IN PLACE for rows >= 1), Xs f32[P,HW,3],
 * Cs f32[P,HW,1], ii/jj i64[E] (global keyframe ids; the callee maps them to rows with
 * unique+searchsorted and pins the first unique id, gn_kernels.cu:161-170,1157),
 * idx_ii2jj i64[E,HW], valid_match u8[E,HW,1], Q f32[E,HW,1], K f32[3,3] (device), dx f32[P-1,7].
 * `workspace` is a caller-owned device buffer of >= mslam_gn_workspace_bytes(P,E,HW,E_local) bytes
 * (E_local = the edges this caller compacts and accumulates: E for the fused entry points, the size of
 * the rank's edge slice in the sharded loop).  No cap on P: the fp64 normal equations are a dense
 * (7(P-1))^2 matrix in the workspace, factored by a blocked LL^T on the f64 matrix cores.
 * The whole GN loop is enqueued on `stream` with NO host synchronisation: convergence
 * (||dx|| < delta_thresh, gn_kernels.cu:1219-1222) is a device-side flag that turns the remaining
 * iterations' kernels into no-ops.  LLT failure => dx = 0 (gn_kernels.cu:147-150).
 * ------------------------------------------------------------------------------------------ */
size_t mslam_gn_workspace_bytes(int num_poses, int num_edges, int num_points, int local_edges);

/* Replaces gauss_newton_rays (gn.cpp:28-52; ray_align_kernel gn_kernels.cu:813-1138). */
int mslam_gauss_newton_rays(float* Twc, const float* Xs, const float* Cs, const int64_t* ii,
                            const int64_t* jj, const int64_t* idx_ii2jj, const uint8_t* valid_match,
                            const float* Q, int num_poses, int num_points, int num_edges,
                            float sigma_ray, float sigma_dist, float C_thresh, float Q_thresh,
                            int max_iter, float delta_thresh, float* dx, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Replaces gauss_newton_calib (gn.cpp:54-82; calib_proj_kernel gn_kernels.cu:1231-1543). */
int mslam_gauss_newton_calib(float* Twc, const float* Xs, const float* Cs, const float* K,
                             const int64_t* ii, const int64_t* jj, const int64_t* idx_ii2jj,
                             const uint8_t* valid_match, const float* Q, int num_poses, int num_points,
                             int num_edges, int height, int width, int pixel_border, float z_eps,
                             float sigma_pixel, float sigma_depth, float C_thresh, float Q_thresh,
                             int max_iter, float delta_thresh, float* dx, void* workspace,
                             size_t workspace_bytes, void* stream);

/* Replaces gauss_newton_points (gn.cpp:3-26; point_align_kernel gn_kernels.cu:455-723). */
int mslam_gauss_newton_points(float* Twc, const float* Xs, const float* Cs, const int64_t* ii,
                              const int64_t* jj, const int64_t* idx_ii2jj, const uint8_t* valid_match,
                              const float* Q, int num_poses, int num_points, int num_edges,
                              float sigma_point, float C_thresh, float Q_thresh, int max_iter,
                              float delta_thresh, float* dx, void* workspace, size_t workspace_bytes,
                              void* stream);

/* The same loop opened up for the multi-GPU factor graph (global_opt.py:123-223): every rank calls
 * begin() with the FULL edge list, then compact() ONCE for ITS edge range (per-edge inputs are local
 * arrays of edge_count rows): the pose-independent part of the reference's edge kernels - the gather
 * Xi[idx] and the gates valid_match, Q > Q_thresh, C > C_thresh (gn_kernels.cu:905-925) - is resolved
 * into a dense stream in the workspace.  Per iteration: accumulate() streams it at the current poses
 * into the global, reference-layout buffers Hs f32[4,E,7,7] / gs f32[2,E,7] ([ii,ij,ji,jj] / [i,j],
 * gn_kernels.cu:1120-1133; slots of other ranks' edges stay zero), the caller all-reduces Hs and gs
 * (RCCL sum), then solve_retract(), which is bit-identical on every rank.
 * kind: 0 rays (sigma_a=ray, sigma_b=dist), 1 calib (pixel, depth), 2 points (point, -). */
int mslam_gn_begin(const int64_t* ii, const int64_t* jj, int num_poses, int num_edges, int num_points,
                   void* workspace, size_t workspace_bytes, void* stream);
int mslam_gn_compact(const float* Xs, const float* Cs, const int64_t* idx_ii2jj, const uint8_t* valid_match,
                     const float* Q, int num_poses, int num_points, int num_edges, int edge_begin,
                     int edge_count, float C_thresh, float Q_thresh, void* workspace, size_t workspace_bytes,
                     void* stream);
/* compact() for edge ranges whose per-edge inputs do not lie in ONE array: the factor graph keeps the forward and the
 * backward direction of its edges in two row-appendable buffers (global_opt.py:106-112 concatenates them for every
 * solve: O(edges) copies of [E, HW] arrays per keyframe); a rank's accumulate range of `range_count` edges is compacted
 * by one call per source array, each filling the slots [slot_begin, slot_begin + edge_count) of that range. */
int mslam_gn_compact_at(const float* Xs, const float* Cs, const int64_t* idx_ii2jj, const uint8_t* valid_match,
                        const float* Q, int num_poses, int num_points, int num_edges, int edge_begin, int edge_count,
                        int slot_begin, int range_count, float C_thresh, float Q_thresh, void* workspace,
                        size_t workspace_bytes, void* stream);
int mslam_gn_accumulate(int kind, const float* Twc, const float* K, int num_poses, int num_points,
                        int num_edges, int edge_begin, int edge_count, float sigma_a, float sigma_b,
                        int height, int width, int pixel_border, float z_eps, float* Hs, float* gs,
                        void* workspace, size_t workspace_bytes, void* stream);
int mslam_gn_solve_retract(const float* Hs, const float* gs, int num_poses, int num_edges,
                           int num_points, float* Twc, float* dx, float delta_thresh, void* workspace,
                           size_t workspace_bytes, void* stream);
/* status4 (device i32[4]) <- {done, iterations run, chol_fail, bits of last ||dx|| (f32)}.  chol_fail != 0: the
 * factorisation of the most recent solve_retract() failed (dx = 0, poses untouched); it stays until the next solve
 * that runs (a solve after `done` does not) and is 0 after one that succeeded and after begin(). */
int mslam_gn_status(int* status4, int num_poses, int num_edges, int num_points, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sim3 group ops (lietorch.Sim3 surface used by the hot path: act / inv / mul / exp / retr;
 * call sites tracker.py:150,232,247,264, geometry.py:45-52, global_manager.py:88-105;
 * maths restated in gn_kernels.cu:177-413).  Pose layout f32[n,8] = [t, q(xyzw), s]; xi f32[n,7]
 * = [tau, phi, sigma].  Forward only.
 * ------------------------------------------------------------------------------------------ */
/* Y[i] = T[pose(i)] . X[i]; pose(i) = i / pts_per_pose, or 0 when broadcast_pose. */
int mslam_sim3_act(const float* T, const float* X, float* Y, int num_poses, long long pts_per_pose,
                   int broadcast_pose, void* stream);
/* op 0: out = A^-1 ; 1: out = A*B ; 2: out = exp(A as xi) ; 3: out = exp(A as xi) * B (retr). */
int mslam_sim3_op(int op, const float* A, const float* B, float* out, int n, int bcast_a, int bcast_b,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * Global sparse TSDF (world-space half of the "dual TSDF"): GPU voxel hash replacing the python
 * dict of mast3r_slam/tsdf/global_volume.py.  `table` is a caller-owned device buffer of
 * mslam_tsdf_table_bytes(capacity) bytes (capacity = power of two slots); voxel keys are the
 * reference's integer triples floor(p / voxel_size) (global_volume.py:133-134), bit-exact.
 * ------------------------------------------------------------------------------------------ */
size_t mslam_tsdf_table_bytes(uint64_t capacity);
int mslam_tsdf_table_init(void* table, size_t table_bytes, uint64_t capacity, void* stream);

/* Replaces TSDFVolume.integrate (global_volume.py:35-72) + _update_voxel (:74-88).
 * points_world f32[n,3], conf f64[n], cam_origin f32[3] (all device).  Samples are replayed per
 * voxel in the reference's order, so results equal the sequential python loop, including the
 * first-touch and max_weight-saturation behaviour.  shard_id/num_shards: only voxels whose key
 * hashes to this shard are touched (multi-GPU: one table per rank, points replicated). */
size_t mslam_tsdf_integrate_workspace_bytes(int n_points, double voxel_size, double trunc, double step_scale);
int mslam_tsdf_integrate(void* table, uint64_t capacity, const float* points_world, const double* conf,
                         const float* cam_origin, int n_points, double voxel_size, double trunc,
                         double max_weight, double step_scale, int shard_id, int num_shards,
                         void* workspace, size_t workspace_bytes, void* stream);

/* out8_host <- {voxels, overflow flag, records of last integrate, voxels touched, points fused
 * (integrate's return value), dump cursor, capacity lo, capacity hi}.  SYNCHRONISES the stream. */
/* Growth of the voxel hash (the reference's dict is unbounded, global_volume.py:27): moves every voxel of `old_table`
 * into `new_table` (initialised by mslam_tsdf_table_init, capacity >= the old one) with value, weight and first-touch
 * state.  Call between integrate calls; the host side (TSDFVolume.maintain) does so when the load exceeds 1/2. */
int mslam_tsdf_rehash(void* old_table, uint64_t old_capacity, void* new_table, uint64_t new_capacity, void* stream);
int mslam_tsdf_header(void* table, uint64_t capacity, uint32_t* out8_host, void* stream);

/* Dict contents (TSDFVolume._voxels): keys i64[max_out,3], tsdf f64, weight f64, unordered. */
int mslam_tsdf_dump(void* table, uint64_t capacity, int64_t* keys, double* tsdf, double* weight,
                    uint32_t max_out, void* stream);

/* Replaces TSDFVolume.query + _estimate_gradient (global_volume.py:93-128) for n points:
 * status 0 = (None, None), 1 = (value, None), 2 = (value, unit gradient). */
int mslam_tsdf_query(void* table, uint64_t capacity, const float* points, int n, double voxel_size,
                     double min_weight, double* value, double* grad, uint8_t* status, void* stream);

/* Replaces one iteration of TSDFPoseOptimizer._optimize_single (tsdf_optimizer.py:77-86):
 * world = pose.act(points) (if points_in_camera_frame), residual/Jacobian/weights
 * (_build_linear_system :94-105, _sim3_jacobian :118-124), H,b (_accumulate_system :107-116, fp64),
 * and if update_pose: delta = solve(H + damping I, -b); pose <- exp(delta) * pose.
 * H_out f64[7,7], b_out f64[7], used_out i32 may be NULL.  workspace >= 64*36*8 bytes. */
int mslam_tsdf_pose_step(void* table, uint64_t capacity, const float* points, const float* conf, int n,
                         float* pose, int points_in_camera_frame, double voxel_size, double min_weight,
                         double lambda, double damping, int update_pose, double* H_out, double* b_out,
                         int* used_out, void* workspace, size_t workspace_bytes, void* stream);

/* Voxel-sharded volume (north_star: "TSDF voxel blocks shard across the 8 GPUs"; the reference's TSDFVolume is one
 * python dict, global_volume.py:15-31): a voxel lives in the table of exactly one rank, so a query / pose iteration is
 * owner-computes: every rank writes what ITS table holds for the seven voxels a query reads (centre, +x, -x, +y, -y,
 * +z, -z) of every point - out f64[n,7,3] = (state, weight, tsdf), zeros for voxels it does not own - the caller
 * all-reduces (sum) that array over the ranks, and the *_lookup entry points evaluate global_volume.py:93-128 /
 * tsdf_optimizer.py:77-124 on it: bit-identical to mslam_tsdf_query / mslam_tsdf_pose_step on one table holding
 * every voxel.  `pose` != NULL: points are camera-frame, moved with pose first (as mslam_tsdf_pose_step does). */
int mslam_tsdf_lookup7(void* table, uint64_t capacity, const float* points, int n, const float* pose,
                       double voxel_size, double* out, void* stream);
int mslam_tsdf_query_lookup(const double* lookup, int n, double voxel_size, double min_weight, double* value,
                            double* grad, uint8_t* status, void* stream);
int mslam_tsdf_pose_step_lookup(const double* lookup, const float* points, const float* conf, int n, float* pose,
                                int points_in_camera_frame, double voxel_size, double min_weight, double lambda,
                                double damping, int update_pose, double* H_out, double* b_out, int* used_out,
                                void* workspace, size_t workspace_bytes, void* stream);

/* Triangle mesh of the volume (marching cubes; no counterpart in the reference, DESIGN.md "Mesh extraction").  The table
 * is only read.  Sequence, all on one stream:
 *   mslam_tsdf_mesh_keys     sort_keys i64[capacity]: packed key of every voxel with weight >= min_weight, INT64_MAX
 *                            elsewhere; the caller sorts them ascending (values + their slot indices `order`);
 *   mslam_tsdf_mesh_count    counts i32[2][capacity]: vertices owned / triangles of the cube at each sorted position;
 *                            the caller forms their exclusive scans vbase, fbase (i64) and the totals V, F;
 *   mslam_tsdf_mesh_emit     vertices f32[V,3], normals f32[V,3], faces i32[F,3] in canonical order.
 * workspace >= mslam_tsdf_mesh_workspace_bytes(capacity), kept between count and emit. */
size_t mslam_tsdf_mesh_workspace_bytes(uint64_t capacity);
int mslam_tsdf_mesh_keys(void* table, uint64_t capacity, double min_weight, int64_t* sort_keys, void* stream);
int mslam_tsdf_mesh_count(void* table, uint64_t capacity, double min_weight, double level, const int64_t* sorted_keys,
                          const int64_t* order, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int mslam_tsdf_mesh_emit(void* table, uint64_t capacity, double voxel_size, double min_weight, double level,
                         const int64_t* sorted_keys, const int64_t* order, const int64_t* vbase, const int64_t* fbase,
                         void* workspace, size_t workspace_bytes, float* vertices, float* normals, int32_t* faces,
                         int64_t n_vertices, int64_t n_faces, void* stream);
/* Inserts n distinct voxels keys i64[n,3], tsdf f64[n], weight f64[n] into an initialised table as averaged voxels;
 * a full table or a key outside the 21-bit range sets the header's overflow flag (as integrate does). */
int mslam_tsdf_load(void* table, uint64_t capacity, const int64_t* keys, const double* tsdf, const double* weight,
                    int n, void* stream);

/* Connected components of a welded triangle mesh and the filter that drops whole components (no counterpart in the
 * reference, DESIGN.md "Mesh components").  faces i32[F,3] hold vertex indices in [0, V); the caller checks that range
 * (a face outside it is skipped, never followed).  Any welded mesh, not only the volume's.  Sequence, on one stream:
 *   mslam_mesh_cc_label   root i32[V]: the smallest vertex index of each vertex's component (lock-free union-find in
 *                         `root` itself; a parent is only ever replaced by a smaller value, so nothing can spin); exact
 *                         and bit-identical for any scheduling.  A vertex no face uses is its own component.
 *   mslam_mesh_cc_count   faces_at_root i32[V], verts_at_root i32[V] (either may be NULL): faces (by their first vertex)
 *                         and vertices of the component, at the root's index, zero elsewhere.  aggregate != 0: a run of
 *                         neighbouring lanes with one root adds once; 0: one atomic per element.  Same output.
 *   mslam_mesh_cc_select  keep_vertex i32[V], keep_face i32[F] <- keep_root u8[V] looked up at each element's root;
 *                         the caller forms their exclusive scans vbase, fbase (i64) and the totals V', F';
 *   mslam_mesh_cc_emit    kept vertices / normals / colours (colors and out_colors both NULL: none) f32[V',3] in their
 *                         original order, kept faces i32[F',3] with remapped indices.
 * No workspace: the union-find runs in `root`. */
int mslam_mesh_cc_label(const int32_t* faces, int num_faces, int num_vertices, int32_t* root, void* stream);
int mslam_mesh_cc_count(const int32_t* faces, int num_faces, int num_vertices, const int32_t* root,
                        int32_t* faces_at_root, int32_t* verts_at_root, int aggregate, void* stream);
int mslam_mesh_cc_select(const int32_t* faces, int num_faces, int num_vertices, const int32_t* root,
                         const uint8_t* keep_root, int32_t* keep_vertex, int32_t* keep_face, void* stream);
int mslam_mesh_cc_emit(const float* vertices, const float* normals, const float* colors, const int32_t* faces,
                       int num_faces, int num_vertices, const int32_t* keep_vertex, const int32_t* keep_face,
                       const int64_t* vbase, const int64_t* fbase, float* out_vertices, float* out_normals,
                       float* out_colors, int32_t* out_faces, int64_t n_out_vertices, int64_t n_out_faces,
                       void* stream);

/* Mesh simplification: vertices clustered on a uniform grid, each cluster's vertex placed by the plane quadrics of the
 * faces that touch its cell (no counterpart in the reference, DESIGN.md "Mesh simplification").  vertices / normals /
 * colors f32[V,3], faces i32[F,3]; every index read from memory is checked before it is followed and an element that
 * fails is skipped.  All arithmetic is f64 on the f32 inputs, every sum runs in one fixed order, nothing is atomic: the
 * same input gives the same bits.  Sequence, on one stream (C clusters, 3 F < 2^31, C F < 2^62):
 *   mslam_mesh_simplify_keys   keys i64[V]: the packed cell floor(p / cell_size) of each vertex, 21 bits per axis biased
 *                              by 2^20, x highest; INT64_MAX for a coordinate that is not finite or a cell outside
 *                              [-2^20, 2^20).  The caller sorts them (stable) -> sorted_keys, vertex_order; numbers the
 *                              distinct keys 0..C-1 -> cluster i32[V]; vertex_start i64[C+1]: the first sorted position
 *                              of each cluster, V at the end.
 *   mslam_mesh_simplify_faces  tri i32[F,3]: the face in cluster ids, rotated so that the smallest is first, -1 -1 -1
 *                              unless the three differ.  packed != 0 (needs C^3 < 2^62): key_lo i64[F] = (t0 C + t1) C +
 *                              t2, key_hi unused (may be NULL); 0: key_lo = t1 C + t2, key_hi = t0; INT64_MAX for a
 *                              collapsed face.  pairs i64[3 F]: cluster * F + face, once per distinct cluster of a face
 *                              whose indices are in range, INT64_MAX in the other slots.  The caller sorts the pairs ->
 *                              sorted_pairs, pair_start i64[C+1] (the first pair with key >= cluster * F), and the triple
 *                              keys -> face_order i64[F].
 *   mslam_mesh_simplify_solve  per cluster c: x0 = the cell's centre; m = mean of (p - x0) over its vertices in ascending
 *                              index; quadric != 0: A = sum w u u^T, b = sum w d u over its pairs' valid faces
 *                              (mslam_mesh_face_areas' rule) in ascending index, u the unit normal, w the area, d = -u .
 *                              (a - x0); x = m + sum over eigenpairs with lambda > 1e-3 lambda_max of e (e . (-b - A m)) /
 *                              lambda, or m when lambda_max <= 0, some |x_j| > cell_size / 2 or x is not finite.
 *                              out_vertices f32[C,3] = x0 + x; out_normals = the normalised sum of the normals (0 if
 *                              the sum is 0); out_colors = the mean colour (colors and out_colors both NULL: none);
 *                              out_fallback i32[C] (may be NULL) = 1 where x = m.
 *   mslam_mesh_simplify_mark   sorted_tri i32[F,3] = tri in face_order (0 0 0 for a collapsed face); keep_face i32[F] = 1
 *                              for a live face that differs from its predecessor; referenced i32[C] (zeroed by the
 *                              caller) = 1 at every cluster of a kept face.
 * The caller then scans the flags and calls mslam_mesh_cc_emit on (out_vertices, ..., sorted_tri). */
int mslam_mesh_simplify_keys(const float* vertices, int num_vertices, double cell_size, int64_t* keys, void* stream);
int mslam_mesh_simplify_faces(const int32_t* faces, int num_faces, int num_vertices, const int32_t* cluster,
                              int num_clusters, int packed, int32_t* tri, int64_t* key_hi, int64_t* key_lo,
                              int64_t* pairs, void* stream);
int mslam_mesh_simplify_solve(const float* vertices, const float* normals, const float* colors, const int32_t* faces,
                              int num_faces, int num_vertices, double cell_size, const int64_t* sorted_keys,
                              const int64_t* vertex_order, const int64_t* vertex_start, const int64_t* sorted_pairs,
                              const int64_t* pair_start, int num_clusters, int quadric, float* out_vertices,
                              float* out_normals, float* out_colors, int32_t* out_fallback, void* stream);
int mslam_mesh_simplify_mark(const int32_t* tri, const int64_t* face_order, int num_faces, int num_clusters,
                             int32_t* sorted_tri, int32_t* keep_face, int32_t* referenced, void* stream);

/* Mesh smoothing: Taubin lambda|mu steps over the vertex neighbour table, and vertex normals from the winding over the
 * vertex face table (no counterpart in the reference, DESIGN.md "Mesh smoothing").  faces i32[F,3]; a face COUNTS when
 * its three indices lie in [0, V) and are pairwise different (area plays no part).  Every index read from memory is
 * checked before it is followed and an element that fails is skipped.  The state is f64, every sum runs in one fixed
 * order, nothing is atomic: the same input gives the same bits.  Sequence, on one stream (3 F < 2^31, V F < 2^62):
 *   mslam_mesh_smooth_edges    keys i64[6 F]: per counting face the directed edge keys a V + b of its three edges in
 *                              both directions, INT64_MAX in all six slots of any other face.  The caller sorts them;
 *                              the E distinct keys below V V give nbr i32[E] = key mod V, mult i32[E] = how often the key
 *                              occurs (the counting faces on that edge) and row_start i64[V+1], the first key >= v V:
 *                              row v holds the neighbours of v, each once, in ascending index.
 *   mslam_mesh_smooth_step     one Jacobi step x_out = x_in + factor (S / n - x_in), each operation rounded on its own.
 *                              x_in, x_out f64[V,stride], stride 3, or 4 with both 32-byte aligned (x y z 0), never the
 *                              same buffer.  S = 0.0 + the positions of the row's neighbours in ascending index, n their
 *                              number.  A vertex with an edge of mult 1 is a boundary vertex: MSLAM_MESH_SMOOTH_FIXED
 *                              copies it, _CURVE sums only over its neighbours behind edges of mult 1, _FREE treats it
 *                              as any other.  A vertex with an empty row is copied.  vclass u8[V] (may be NULL) receives
 *                              MSLAM_MESH_SMOOTH_INTERIOR, _BOUNDARY or _ISOLATED.  num_edges: the length of nbr and
 *                              mult; rows are clipped to it.
 *   mslam_mesh_vertex_faces    pairs i64[3 F]: vertex F + face for the three vertices of a counting face, INT64_MAX in
 *                              the three slots of any other.  The caller sorts them -> sorted_pairs, and pair_start
 *                              i64[V+1], the first pair >= v F.
 *   mslam_mesh_vertex_normals  normals f32[V,3]: the sum over the vertex's counting faces, in ascending face index, of
 *                              (b - a) x (c - a) in f64 on the f32 vertices, divided by its length; zero when the sum is
 *                              zero or not finite; normals_in f32[V,3] (NULL: zero) for a vertex without a counting
 *                              face.  normals_in is only read and must not be `normals`. */
#define MSLAM_MESH_SMOOTH_FIXED 0
#define MSLAM_MESH_SMOOTH_CURVE 1
#define MSLAM_MESH_SMOOTH_FREE 2
#define MSLAM_MESH_SMOOTH_INTERIOR 0
#define MSLAM_MESH_SMOOTH_BOUNDARY 1
#define MSLAM_MESH_SMOOTH_ISOLATED 2
int mslam_mesh_smooth_edges(const int32_t* faces, int num_faces, int num_vertices, int64_t* keys, void* stream);
int mslam_mesh_smooth_step(const double* x_in, double* x_out, int stride, const int64_t* row_start, const int32_t* nbr,
                           const int32_t* mult, int num_vertices, int64_t num_edges, double factor, int boundary_mode,
                           uint8_t* vclass, void* stream);
int mslam_mesh_vertex_faces(const int32_t* faces, int num_faces, int num_vertices, int64_t* pairs, void* stream);
int mslam_mesh_vertex_normals(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                              const int64_t* sorted_pairs, const int64_t* pair_start, const float* normals_in,
                              float* normals, void* stream);

/* Mesh decimation: round-based half-edge collapse with plane quadrics to a target face count or error (no counterpart
 * in the reference, DESIGN.md "Mesh decimation", tests/decimate_numpy.py).  vertices f32[V,3] are only read: a removed
 * vertex is merged into a neighbour.  faces i32[F,3] is the caller's working copy; a face COUNTS as in the smoothing, and
 * the tables of a round are mslam_mesh_smooth_edges / mslam_mesh_vertex_faces on it.  state f64[V,MSLAM_MESH_DECIMATE_STATE]:
 * the quadric xx xy xz xd yy yz yd zz zd dd, then the area.  Every index read from memory is checked before it is
 * followed; all arithmetic is f64 on the f32 inputs, each operation rounded on its own, every sum in one fixed order,
 * nothing is atomic: the same input gives the same bits.  Sequence, on one stream (3 F < 2^31, V F < 2^62):
 *   mslam_mesh_decimate_state       once: state[v] = 0.0 + (A g_i) g_j and A over the counting faces of v in ascending
 *                                   face index, g = (k, -k . a), k the unit normal, A the area; a face whose cross
 *                                   product has no finite positive length adds nothing.
 *   mslam_mesh_decimate_candidates  per vertex u: vclass u8[V] (may be NULL) = _ISOLATED (no neighbour), _BOUNDARY (an
 *                                   edge of mult 1), _REMOVABLE (every edge of mult 2 and as many faces as neighbours)
 *                                   or _OTHER.  For a removable u, best i32[V] = the neighbour v of lowest (cost, v)
 *                                   among those that pass the link condition (exactly two common neighbours, neither a
 *                                   closed fan of three faces or fewer), the flip
 *                                   test (every face of u without v keeps a positive dot of its cross product with the
 *                                   one before) and, with gate >= 0, cost <= gate (area u + area v); cost f64[V] =
 *                                   max(0, h^T (Q_u + Q_v) h) at h = (x_v, 1).  -1 and +inf without one.  key i64[V] =
 *                                   hash32(u, round) 2^31 + u, INT64_MAX without one.  The caller ranks the candidates
 *                                   by (cost, key): rank i32[V], INT32_MAX for the others.
 *   mslam_mesh_decimate_spread      rank_out[v] = the minimum of rank_in over v and its neighbours; never in place.
 *                                   Twice: a candidate whose own rank comes back is selected.
 *   mslam_mesh_decimate_apply       per selected u (selected u8[V]), v = best[u]: every face corner u becomes v (in
 *                                   place), state[v] += state[u], parent[u] = v.  Selected vertices must be three hops
 *                                   apart, which the two spreads give.
 *   mslam_mesh_decimate_finish      keep_face i32[F] = the face counts; referenced i32[V] (zeroed by the caller) = 1 at
 *                                   the corners of a counting face; end i32[V] = the end of the parent chain, followed
 *                                   for at most max_steps links.
 * The caller then scans the flags and calls mslam_mesh_cc_emit on the input rows and the working faces. */
#define MSLAM_MESH_DECIMATE_STATE 11
#define MSLAM_MESH_DECIMATE_OTHER 0
#define MSLAM_MESH_DECIMATE_BOUNDARY 1
#define MSLAM_MESH_DECIMATE_ISOLATED 2
#define MSLAM_MESH_DECIMATE_REMOVABLE 3
int mslam_mesh_decimate_state(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                              const int64_t* sorted_pairs, const int64_t* pair_start, double* state, void* stream);
int mslam_mesh_decimate_candidates(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                                   const int64_t* row_start, const int32_t* nbr, const int32_t* mult, int64_t num_edges,
                                   const int64_t* sorted_pairs, const int64_t* pair_start, const double* state,
                                   double gate, int round, int32_t* best, double* cost, int64_t* key, uint8_t* vclass,
                                   void* stream);
int mslam_mesh_decimate_spread(const int32_t* rank_in, const int64_t* row_start, const int32_t* nbr, int num_vertices,
                               int64_t num_edges, int32_t* rank_out, void* stream);
int mslam_mesh_decimate_apply(int32_t* faces, int num_faces, int num_vertices, const uint8_t* selected,
                              const int32_t* best, double* state, int32_t* parent, void* stream);
int mslam_mesh_decimate_finish(const int32_t* faces, int num_faces, int num_vertices, const int32_t* parent,
                               int max_steps, int32_t* keep_face, int32_t* referenced, int32_t* end, void* stream);

/* Mesh holes: the boundary loops of a welded mesh, and a centroid fan over the small, well-behaved ones (no counterpart
 * in the reference, DESIGN.md "Mesh holes").  faces i32[F,3]; a face COUNTS as in the smoothing.  A boundary dart is a
 * directed edge of a counting face, in its winding, whose undirected edge lies on exactly one counting face; its id is
 * 3 face + corner, the edge from corner c to corner c + 1.  Every index read from memory is checked before it is
 * followed; all arithmetic is f64 on the f32 inputs, every sum runs in walk order, nothing is atomic: the same input gives
 * the same bits.  `state` is i32[B,2], 8-byte aligned: per boundary dart (successor or -1, smallest tail so far).
 * Sequence, on one stream (3 F < 2^31):
 *   mslam_mesh_holes_keys     keys i64[3 F]: slot 3 f + c holds min V + max of that edge of a counting face, INT64_MAX
 *                             in the three slots of any other face.  The caller sorts them, stable, with the permutation.
 *   mslam_mesh_holes_mark     flag u8[3 F]: flag[order[i]] = 1 when sorted slot i is a run of length 1 below INT64_MAX,
 *                             else 0.  The caller compacts the flagged slots, ascending: dart i32[B].
 *   mslam_mesh_holes_darts    tail, head i32[B] of every boundary dart; -1 for a dart or a vertex out of range.  The
 *                             caller sorts the tails (sorted_tail, tail_order i64[B]) and the heads (sorted_head).
 *   mslam_mesh_holes_link     state[d] = (next(d), tail[d]): next(d) is the dart whose tail is head(d) when head(d)
 *                             occurs exactly once in sorted_tail and once in sorted_head (a simple vertex), else -1.
 *   mslam_mesh_holes_double   one round of pointer doubling from state_in to state_out (never the same buffer):
 *                             (p, m) -> (p of p, min(m, m of p)); a dart whose p is -1 keeps its m.  After r rounds with
 *                             2^r >= B, p >= 0 exactly on the cycles of next, and m is the cycle's smallest vertex.
 *   mslam_mesh_holes_loop_labels  with flag NULL: keys i32[B+1]: m for a dart on a cycle, INT32_MAX for any other,
 *                             INT32_MAX in slot B.  The caller sorts them; the runs below the last give loop_id i32[L],
 *                             ascending, and length.
 *   mslam_mesh_holes_loop_assign  with own = the linked state, loop_name = loop_id, and flag, loop_id and loop_head
 *                             NULL: dart_loop i32[B]: the position of the dart's m in loop_id, -1 off the cycles;
 *                             start i32[L]: the dart of each loop whose tail is the loop id (the caller presets -1).
 *   mslam_mesh_holes_measure  one lane per loop, walking from start along next: perimeter f64[L] (NaN when not walked),
 *                             centre f64[L,3] (the f64 mean of the tails) and fillable u8[L]: 3 <= n <= max_edges and
 *                             every dart's fan face (head, tail, centre) turns the way of the dart's own face.  A loop
 *                             longer than max_edges is walked only when all_perimeters is set.
 *   mslam_mesh_holes_emit     one lane per fillable loop: row V + vertex_base[l] of out_vertices, out_normals and
 *                             out_colors (NULL with colors NULL), rows F + face_base[l] ... + n of out_faces.  Rows
 *                             below V and F are not touched: the caller copies the input there. */
int mslam_mesh_holes_keys(const int32_t* faces, int num_faces, int num_vertices, int64_t* keys, void* stream);
int mslam_mesh_holes_mark(const int64_t* sorted_keys, const int64_t* order, int64_t num_keys, uint8_t* flag,
                          void* stream);
int mslam_mesh_holes_darts(const int32_t* faces, int num_faces, int num_vertices, const int32_t* dart, int num_darts,
                           int32_t* tail, int32_t* head, void* stream);
int mslam_mesh_holes_link(const int32_t* tail, const int32_t* head, const int32_t* sorted_tail,
                          const int64_t* tail_order, const int32_t* sorted_head, int num_darts, int num_vertices,
                          int32_t* state, void* stream);
int mslam_mesh_holes_double(const int32_t* state_in, int32_t* state_out, int num_darts, void* stream);
int mslam_mesh_holes_loop_labels(const int32_t* labelled, const uint8_t* flag, int num_darts, int32_t* keys,
                                 void* stream);
int mslam_mesh_holes_loop_assign(const int32_t* labelled, const int32_t* own, const uint8_t* flag, const int32_t* tail,
                                 const int32_t* head, int num_darts, const int32_t* loop_name, int num_loops,
                                 int32_t* dart_loop, int32_t* start, int32_t* loop_id, int32_t* loop_head, void* stream);
int mslam_mesh_holes_measure(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                             const int32_t* dart, const int32_t* tail, const int32_t* head, const int32_t* state,
                             int num_darts, const int32_t* start, const int32_t* length, int num_loops, int max_edges,
                             int all_perimeters, double* perimeter, double* centre, uint8_t* fillable, void* stream);
int mslam_mesh_holes_emit(const float* vertices, const float* colors, const int32_t* tail, const int32_t* head,
                          const int32_t* state, int num_darts, const int32_t* start, const int32_t* length,
                          const uint8_t* fillable, const int64_t* vertex_base, const int64_t* face_base, int num_loops,
                          int num_vertices, int num_faces, int new_vertices, int new_faces, const double* centre,
                          float* out_vertices, float* out_normals, float* out_colors, int32_t* out_faces, void* stream);

/* Mesh holes, bow-tie mode (DESIGN.md "Mesh holes", tests/bowtie_numpy.py): boundary darts are paired across the hole
 * they bound, so that the rims of holes that meet in a vertex close.  Runs between mslam_mesh_holes_darts and
 * mslam_mesh_holes_measure in place of link and double, and ahead of loop_labels and loop_assign (declared above, here
 * with their flag); measure and emit read the paired state.  state, labelled, rank and paired are i32[B,2], 8-byte
 * aligned.  One lane per element, no atomics, every index read from memory is checked.
 *   mslam_mesh_holes_dkeys        keys i64[3 F]: slot 3 f + c holds tail V + head of that directed edge of a counting
 *                                 face, INT64_MAX in the three slots of any other face.  The caller sorts them, stable,
 *                                 with the permutation (sorted_keys, key_order), gathers dart_key i64[B] = keys[dart] and
 *                                 sorts that too: a dart's name is the position of its key there.
 *   mslam_mesh_holes_fan          fan i32[B]: for the dart u -> v on face f, the rotation about v from f across interior
 *                                 edges to the boundary dart that leaves v across the same hole, or -1.  An edge v -> w
 *                                 is crossed only when it and w -> v occur exactly once among the keys; at most as many
 *                                 steps as keys have the tail v.  The caller sorts fan (sorted_fan).
 *   mslam_mesh_holes_claim        state[d] = (fan[d] when it occurs exactly once in sorted_fan, else -1; name of d).
 *                                 mslam_mesh_holes_double on it gives labelled: p >= 0 exactly on the closed walks of
 *                                 fan, m the walk's smallest name.
 *   mslam_mesh_holes_rank_init    rank[d] = (fan[d], 1) on a closed walk, (-1, 1) when fan[d] is the walk's first dart
 *                                 (the one whose name is the label), (-1, 0) off the walks.
 *   mslam_mesh_holes_rank_double  one round of (p, c) -> (p of p, c + c of p), never in place (mslam_mesh_holes_double
 *                                 with a sum, saturating at B + 1, for the minimum): after r rounds with 2^r >= B, c is
 *                                 the number of steps to the walk's first dart, n for that dart itself.
 *   mslam_mesh_holes_walk_keys    keys i64[B]: label B + (B - c), INT64_MAX off the walks.  Sorted by the caller with
 *                                 the permutation (walk_order): by walk, then by rank.
 *   mslam_mesh_holes_pair_keys    keys i64[B], slot j for the dart walk_order[j]: head B + label, INT64_MAX off the
 *                                 walks.  Sorted by the caller, stable, with the permutation (pair_order): a run is the
 *                                 darts of one walk into one vertex, by ascending rank.
 *   mslam_mesh_holes_repair       paired[d_m] = (fan of d_(m-1 mod k), name of d_m) for the run d_0 .. d_(k-1) of the
 *                                 slot, its ends found by binary search; (-1, name) off the walks.  Every row is
 *                                 written.  mslam_mesh_holes_double on it gives the cycles of next and their labels.
 *   mslam_mesh_holes_tail_keys    keys i64[B]: label V + tail on a cycle of next, INT64_MAX elsewhere.  The caller sorts.
 *   mslam_mesh_holes_tail_flag    flag u8[B], zeroed by the caller: flag[label] = 1 when a sorted key equals the one
 *                                 before it: that cycle has a vertex as a tail twice and stays open.
 *   mslam_mesh_holes_loop_labels  with the flag: a dart whose m is outside [0, B) or flagged gets INT32_MAX too (only
 *                                 a flag makes m an index; without one it is not held against B).  The runs give
 *                                 loop_name i32[L], the smallest dart name of every loop, ascending, and the lengths.
 *   mslam_mesh_holes_loop_assign  with own = paired and the flag: dart_loop i32[B] as above; start, loop_id, loop_head
 *                                 i32[L]: the dart whose name (own[d] second entry) is the loop's, its tail and its
 *                                 head.  loop_id and loop_head may each be NULL; tail and head are read only for them. */
int mslam_mesh_holes_dkeys(const int32_t* faces, int num_faces, int num_vertices, int64_t* keys, void* stream);
int mslam_mesh_holes_fan(const int32_t* faces, int num_faces, int num_vertices, const int32_t* dart,
                         const int32_t* head, int num_darts, const int64_t* sorted_keys, const int64_t* key_order,
                         int32_t* fan, void* stream);
int mslam_mesh_holes_claim(const int32_t* fan, const int32_t* sorted_fan, const int64_t* dart_key,
                           const int64_t* sorted_dart_key, int num_darts, int32_t* state, void* stream);
int mslam_mesh_holes_rank_init(const int32_t* state, const int32_t* labelled, int num_darts, int32_t* rank,
                               void* stream);
int mslam_mesh_holes_rank_double(const int32_t* rank_in, int32_t* rank_out, int num_darts, void* stream);
int mslam_mesh_holes_walk_keys(const int32_t* labelled, const int32_t* rank, int num_darts, int64_t* keys,
                               void* stream);
int mslam_mesh_holes_pair_keys(const int32_t* labelled, const int32_t* head, const int64_t* sorted_walk_keys,
                               const int64_t* walk_order, int num_darts, int num_vertices, int64_t* keys, void* stream);
int mslam_mesh_holes_repair(const int64_t* sorted_pair_keys, const int64_t* pair_order, const int64_t* walk_order,
                            const int32_t* state, int num_darts, int32_t* paired, void* stream);
int mslam_mesh_holes_tail_keys(const int32_t* labelled, const int32_t* tail, int num_darts, int num_vertices,
                               int64_t* keys, void* stream);
int mslam_mesh_holes_tail_flag(const int64_t* sorted_keys, int num_darts, int num_vertices, uint8_t* flag,
                               void* stream);

/* Mesh quality: face areas, a surface sampler and the exact point-to-mesh distance (no counterpart in the reference,
 * DESIGN.md "Mesh quality").  vertices f32[V,3], faces i32[F,3]; every index is checked against [0, V) before use.  A
 * face is valid when its indices are in range and (b - a) x (c - a), in f64, is not exactly zero; an invalid face has
 * area 0, is never sampled and is never the nearest face.  All arithmetic is f64 on the f32 inputs.
 *   mslam_mesh_face_areas  area f64[F] = 0.5 |(b - a) x (c - a)|.
 *   mslam_mesh_sample      cdf f64[F]: inclusive cumulative area (formed by the caller), total = cdf[F-1] > 0.  Sample i
 *                          takes u = (i + 0.5) / n * total, the first face with cdf[f] > u (then back to the last valid
 *                          face at or before it), and barycentrics from a stateless hash of (seed, i): points f32[n,3],
 *                          face i32[n].  Stratified; the same bits on every call.
 *   mslam_mesh_distance    dist2 f64[n], nearest i32[n]: the smallest squared distance from each point to a valid face
 *                          (closest point by Voronoi regions) and the lowest index of a face that attains it; +inf and
 *                          -1 without a valid face.  skip = 0: every face is scanned; 1: tiles of 128 faces whose box
 *                          (written to the workspace first) lies beyond the current best are skipped, same output bit
 *                          for bit; 2: as 1, and i32[4 * ceil(n / 256)] behind the boxes receives, per wave, the number
 *                          of tiles it skipped (workspace_bytes must cover that too).  workspace >=
 *                          mslam_mesh_distance_workspace_bytes(F) for skip = 1; unused for skip = 0. */
int mslam_mesh_face_areas(const float* vertices, const int32_t* faces, int num_faces, int num_vertices, double* area,
                          void* stream);
int mslam_mesh_sample(const float* vertices, const int32_t* faces, int num_faces, int num_vertices, const double* cdf,
                      double total, int n, uint64_t seed, float* points, int32_t* face, void* stream);
size_t mslam_mesh_distance_workspace_bytes(int num_faces);
int mslam_mesh_distance(const float* points, int n, const float* vertices, const int32_t* faces, int num_faces,
                        int num_vertices, int skip, void* workspace, size_t workspace_bytes, double* dist2,
                        int32_t* nearest, void* stream);

/* Mesh alignment: the closed-form similarity between corresponding points and trimmed point-to-mesh ICP (no counterpart
 * in the reference, DESIGN.md "Mesh alignment").  All arithmetic is f64 on the f32 inputs; every sum is reduced in a
 * fixed order without atomics, so the same inputs give the same bits.
 *   state      a device block of MSLAM_MESH_ALIGN_STATE_BYTES: f64[8] Sim3 [t(3), q(xyzw), s] in lietorch layout, then
 *              an int32 status, MSLAM_MESH_ALIGN_OK or MSLAM_MESH_ALIGN_DEGENERATE (fewer than 3 pairs that count, no
 *              spread among the source points, or no positive finite scale: the Sim3 is then left as it was).
 *   log_row    f64[MSLAM_MESH_ALIGN_LOG_DOUBLES] on the device, written by every solve: the number of pairs that
 *              count, their RMSE under the transform the pairs were formed with (+inf without a pair), the scale after
 *              the solve, the status, then the 19 reduced sums about the origins (src[0]; T src[0] or dst[0]):
 *              count, sum w, sum w p (3), sum w c (3), sum w p c^T (9, row-major), sum w |p|^2, sum w dist2.
 *   workspace  mslam_mesh_align_workspace_bytes(n, F, count_skips): the target's tile boxes, one partial per block of
 *              256 points, and with count_skips one int32 per wave, the tiles it did not scan (as skip = 2 of
 *              mslam_mesh_distance), after them.  MSLAM_ENOMEM with the needed size in mslam_last_error when short.
 *   mslam_mesh_align_init       state <- T0 (device f32[8], quaternion normalised in f64; NULL: the identity), and the
 *                               boxes of the target mesh into the workspace, once per alignment.
 *   mslam_mesh_align_step       one ICP iteration on the stream: moved f32[n,3] = (float)(s R src + t) in f64 rounded
 *                               once; dist2 f64[n] / nearest i32[n] of `moved` against the mesh, bit for bit those of
 *                               mslam_mesh_distance; `nearest` is read first as a warm start (any value is safe: -1, out
 *                               of range and invalid faces are ignored) and overwritten; closest f64[n,3] (may be NULL)
 *                               the closest point on the nearest face, NaN without one.  A pair counts when it has a
 *                               face and dist2 <= trim^2 (trim >= 0 in target units, +inf keeps all).  Then the solve for
 *                               the total transform src -> closest replaces the state (with_scale = 0: scale 1).
 *                               n = 0 or F = 0: no pair, degenerate.
 *   mslam_mesh_align_fit_pairs  the same solve for explicit pairs src f32[n,3] -> dst f32[n,3], weights f32[n] >= 0 or
 *                               NULL (a pair of weight 0 does not count); the state is set to the identity first and
 *                               the logged RMSE is that of dst - src.
 *   mslam_mesh_align_read       device copies of the state: T64 f64[8], T32 f32[8], status i32[1]; each may be NULL. */
#define MSLAM_MESH_ALIGN_STATE_BYTES 72
#define MSLAM_MESH_ALIGN_LOG_DOUBLES 24
#define MSLAM_MESH_ALIGN_OK 0
#define MSLAM_MESH_ALIGN_DEGENERATE 1
size_t mslam_mesh_align_workspace_bytes(int n, int num_faces, int count_skips);
int mslam_mesh_align_init(const float* T0, const float* vertices, const int32_t* faces, int num_faces,
                          int num_vertices, void* workspace, size_t workspace_bytes, void* state, void* stream);
int mslam_mesh_align_step(const float* src, int n, const float* vertices, const int32_t* faces, int num_faces,
                          int num_vertices, double trim, int with_scale, int count_skips, void* workspace,
                          size_t workspace_bytes, void* state, int32_t* nearest, float* moved, double* dist2,
                          double* closest, double* log_row, void* stream);
int mslam_mesh_align_fit_pairs(const float* src, const float* dst, const float* weights, int n, int with_scale,
                               void* workspace, size_t workspace_bytes, void* state, double* log_row, void* stream);
int mslam_mesh_align_read(const void* state, double* T64, float* T32, int32_t* status, void* stream);

/* Depth / normal view of the volume by ray casting (no counterpart in the reference, DESIGN.md "View rendering").  The
 * table is only read.  Sequence, on one stream:
 *   mslam_tsdf_render_blocks  fills the workspace with the set of 8^3-voxel blocks that hold a voxel with weight >=
 *                             min_weight (what the march may not jump over); once per table state and min_weight;
 *   mslam_tsdf_render         one ray per pixel: rays f32[h*w,3] unit, camera frame, moved with pose8 (Sim3 [t,q,s] f32);
 *                             samples at near + k * step (world units) up to far; range f32[h*w] = distance along the
 *                             unit ray in camera units (world range / s; 0 on a miss), normal f32[h*w,3] world frame
 *                             towards free space (0 on a miss), hit u8[h*w].  skip = 0: brute-force march; != 0: jumps
 *                             over unmarked blocks, same output bit for bit.  h, w only shape the 8x8-pixel wave tiles.
 * workspace >= mslam_tsdf_render_workspace_bytes(capacity). */
size_t mslam_tsdf_render_workspace_bytes(uint64_t capacity);
int mslam_tsdf_render_blocks(void* table, uint64_t capacity, double min_weight, void* workspace, size_t workspace_bytes,
                             void* stream);
int mslam_tsdf_render(void* table, uint64_t capacity, const float* rays, int h, int w, const float* pose8,
                      double voxel_size, double min_weight, double level, double near, double far, double step, int skip,
                      const void* workspace, size_t workspace_bytes, float* range, float* normal, uint8_t* hit,
                      void* stream);

/* Ray casting against a triangle mesh (no counterpart in the reference, DESIGN.md "Mesh ray casting").  vertices
 * f32[V,3], faces i32[F,3], valid faces as for mslam_mesh_distance; nothing but the outputs is written.
 *   mslam_mesh_raycast_boxes  the boxes of the mesh's 128-face tiles into the workspace, once per mesh (many views
 *                             reuse them); workspace >= mslam_mesh_raycast_workspace_bytes(F).
 *   mslam_mesh_raycast        one ray per pixel: rays f32[h*w,3] in the camera frame, moved with pose8 (Sim3 [t,q,s]
 *                             f32) as mslam_tsdf_render does: origin t, direction d = R rays in f64, not renormalised.
 *                             The two-sided watertight test of Woop et al. in f64 finds, among the valid faces hit at
 *                             near <= t <= far (p = o + t d; far may be +inf), the smallest t and the lowest face index
 *                             at it: range f32[h*w] = t / s (0 on a miss), normal f32[h*w,3] the face's geometric
 *                             normal, unit, towards the origin (0 on a miss), hit u8[h*w], face i32[h*w] (-1 on a
 *                             miss; may be NULL), t64 f64[h*w] (+inf on a miss; may be NULL).  A ray with a zero or
 *                             non-finite direction misses.  h, w only shape the 8x8-pixel wave tiles; h = 1 is a plain
 *                             list of w rays.  skip = 0: every tile is scanned; != 0: tiles whose box the ray cannot
 *                             hit before its current best are skipped (the workspace of mslam_mesh_raycast_boxes is
 *                             read), same output bit for bit.  MSLAM_ENOMEM when the workspace is short. */
size_t mslam_mesh_raycast_workspace_bytes(int num_faces);
int mslam_mesh_raycast_boxes(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                             void* workspace, size_t workspace_bytes, void* stream);
int mslam_mesh_raycast(const float* rays, int h, int w, const float* pose8, const float* vertices,
                       const int32_t* faces, int num_faces, int num_vertices, double near, double far, int skip,
                       const void* workspace, size_t workspace_bytes, float* range, float* normal, uint8_t* hit,
                       int32_t* face, double* t64, void* stream);

/* Mesh index: Morton-ordered tiles with group boxes above them, so that the culled scans of mslam_mesh_distance,
 * mslam_mesh_align_step and mslam_mesh_raycast prune whatever order the caller's faces are in (no counterpart in the
 * reference, DESIGN.md "Mesh index").  The faces are never copied or permuted; all arithmetic is f64 on the f32 inputs in
 * one fixed order; no atomics.  Sequence, on one stream:
 *   mslam_mesh_index_keys     keys i64[F]: the 63-bit Morton code (x highest) of each face's centroid ((a + b) + c) / 3,
 *                             each axis floor((c - lo) / (hi - lo) * 2^21) clamped to [0, 2^21) (a NaN is cell 0) over
 *                             bounds f32[6] = lo.xyz, hi.xyz, the box of the mesh's vertices formed by the caller;
 *                             INT64_MAX for an invalid face (mslam_mesh_distance's rule).  The caller sorts the keys
 *                             (stable) -> order i32[F].
 *   mslam_mesh_index_point_keys  keys i64[n]: the same code of the points f32[n,3] themselves, the keys that sort
 *                             queries; a point outside the box lands in the nearest cell.
 *   mslam_mesh_index_boxes    into the workspace (>= mslam_mesh_index_bytes(F), MSLAM_ENOMEM with the needed size in
 *                             mslam_last_error when short): f64 boxes lo.xyz, hi.xyz of the tiles of 128 consecutive
 *                             faces in `order`, then of the groups of 32 tiles; (+inf, -inf) for an empty one.  An
 *                             entry of `order` outside [0, F) is skipped, not followed.
 * The _indexed entries below take `order` and that workspace (`index`, only read) and give the outputs of their plain
 * forms with skip = 0 bit for bit: a tie goes to the lowest ORIGINAL face index, whatever order the tiles are visited
 * in.  A face that `order` does not name is not seen.  levels: 1 - the tile boxes alone cull; 2 - a group whose box
 * fails the same test for the whole block is passed over first.  skip_counts (may be NULL): i32[4 * blocks], per wave
 * the tile scans it skipped, a skipped group counting as all of its tiles (blocks = ceil(n / 256) for points,
 * mslam_mesh_raycast_blocks(h, w) for rays).
 *   mslam_mesh_distance_indexed    as mslam_mesh_distance.
 *   mslam_mesh_raycast_indexed     as mslam_mesh_raycast.
 *   mslam_mesh_align_init_indexed  state <- T0 as mslam_mesh_align_init; the boxes are the index's.
 *   mslam_mesh_align_step_indexed  as mslam_mesh_align_step, warm start included; workspace >=
 *                                  mslam_mesh_align_workspace_bytes(n, 0, count_skips) (no boxes in it). */
size_t mslam_mesh_index_bytes(int num_faces);
int mslam_mesh_index_keys(const float* vertices, int num_vertices, const int32_t* faces, int num_faces,
                          const float* bounds, int64_t* keys, void* stream);
int mslam_mesh_index_point_keys(const float* points, int n, const float* bounds, int64_t* keys, void* stream);
int mslam_mesh_index_boxes(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                           const int32_t* order, void* workspace, size_t workspace_bytes, void* stream);
int mslam_mesh_distance_indexed(const float* points, int n, const float* vertices, const int32_t* faces, int num_faces,
                                int num_vertices, const int32_t* order, const void* index, size_t index_bytes,
                                int levels, int32_t* skip_counts, double* dist2, int32_t* nearest, void* stream);
int mslam_mesh_raycast_blocks(int h, int w);
int mslam_mesh_raycast_indexed(const float* rays, int h, int w, const float* pose8, const float* vertices,
                               const int32_t* faces, int num_faces, int num_vertices, double near, double far,
                               const int32_t* order, const void* index, size_t index_bytes, int levels,
                               int32_t* skip_counts, float* range, float* normal, uint8_t* hit, int32_t* face,
                               double* t64, void* stream);
int mslam_mesh_align_init_indexed(const float* T0, void* state, void* stream);
int mslam_mesh_align_step_indexed(const float* src, int n, const float* vertices, const int32_t* faces, int num_faces,
                                  int num_vertices, const int32_t* order, const void* index, size_t index_bytes,
                                  double trim, int with_scale, int count_skips, void* workspace, size_t workspace_bytes,
                                  void* state, int32_t* nearest, float* moved, double* dist2, double* closest,
                                  double* log_row, void* stream);

/* Point clouds: a cloud index, the exact nearest neighbour and the voxel downsample (no counterpart in the reference,
 * DESIGN.md "Point clouds"; the definition is tests/cloud_numpy.py).  points f32[N,3]; a point is valid when its three
 * coordinates are finite.  An invalid point is never a nearest neighbour and is never fused.  The points are never copied
 * or permuted; all arithmetic is f64 on the f32 inputs in one fixed order; no atomics.
 *   mslam_cloud_index_boxes   `order` i32[N] is the caller's stable sort of the points' Morton keys
 *                             (mslam_mesh_index_point_keys over the box of the VALID points, INT64_MAX put in for an
 *                             invalid point, so those come last).  Into the workspace (>= mslam_cloud_index_bytes(N),
 *                             MSLAM_ENOMEM with the needed size in mslam_last_error when short): f64 boxes lo.xyz, hi.xyz
 *                             of the tiles of 128 consecutive points in `order`, then of the groups of 32 tiles;
 *                             (+inf, -inf) for an empty one.  An entry of `order` outside [0, N) is skipped, not followed.
 *   mslam_cloud_distance      dist2 f64[n], nearest i32[n]: per query the smallest squared distance dx dx + dy dy + dz dz
 *                             (the f64 differences of the f32 inputs, in that order, uncontracted) to a valid point, and
 *                             the lowest ORIGINAL index of a point at it, whatever order the tiles are visited in; +inf
 *                             and -1 for a query with a non-finite coordinate and for a cloud without a valid point.
 *                             order == NULL: the plain scan, tiles of the input order, no culling (`index` is not
 *                             read).  Otherwise `index` is the workspace above (only read): a tile whose box cannot beat
 *                             the block's current bests is skipped, and with levels = 2 a whole group first; the same
 *                             bits.  A point that `order` does not name is not seen.  skip_counts (may be NULL):
 *                             i32[4 * ceil(n / 256)], per wave the tile scans it skipped, a skipped group counting as
 *                             all of its tiles.
 *   mslam_cloud_voxel_keys    keys i64[N]: the packed voxel key of the global TSDF for the cell size voxel_size,
 *                             floor(f32 coordinate / f32 voxel_size) per axis in [-2^20, 2^20), 21 bits each, x highest;
 *                             INT64_MAX for an invalid or out-of-range point.  (The one cell whose three indices are all
 *                             2^20 - 1 has that very bit pattern and counts as out of range.)
 *   mslam_cloud_voxel_reduce  the caller sorts the keys (stable) -> sorted_keys i64[N] and perm i64[N] (the original
 *                             index of each sorted slot), and lists the slots where a new key other than INT64_MAX
 *                             begins -> starts i64[M].  One entry per voxel, in key order: centroid f32[M,3], the f64 sum
 *                             of the members in sorted order (within a voxel: original index order) divided by the count
 *                             and rounded once; count i32[M]; first i32[M], the lowest original index; with colors
 *                             u8[N,3], color u8[M,3] = (2 sum + count) / (2 count) in integers (NULL together).  An
 *                             entry of perm outside [0, N) is skipped.  The same bits on every call. */
size_t mslam_cloud_index_bytes(int num_points);
int mslam_cloud_index_boxes(const float* points, int num_points, const int32_t* order, void* workspace,
                            size_t workspace_bytes, void* stream);
int mslam_cloud_distance(const float* queries, int n, const float* points, int num_points, const int32_t* order,
                         const void* index, size_t index_bytes, int levels, int32_t* skip_counts, double* dist2,
                         int32_t* nearest, void* stream);
int mslam_cloud_voxel_keys(const float* points, int num_points, double voxel_size, int64_t* keys, void* stream);
int mslam_cloud_voxel_reduce(const float* points, const uint8_t* colors, int num_points, const int64_t* sorted_keys,
                             const int64_t* perm, const int64_t* starts, int num_voxels, float* centroid,
                             int32_t* count, int32_t* first, uint8_t* color, void* stream);

/* Point clouds: the k nearest neighbours and normals (no counterpart in the reference, DESIGN.md "Point clouds"; the
 * definition is tests/cloud_knn_numpy.py; csrc/cloud_knn.hip).
 *   mslam_cloud_knn      dist2 f64[n,k], neighbors i32[n,k], 1 <= k <= MSLAM_CLOUD_KNN_MAX_K: row i holds the k smallest
 *                        valid points of the cloud under the total order (dist2, original index), ascending, dist2 the
 *                        sum of mslam_cloud_distance.  exclude (i32[n], may be NULL): the point with index exclude[i] is
 *                        left out of row i - by index, so a duplicate of it elsewhere stays, at distance 0; an entry
 *                        outside [0, N) excludes nothing.  Slots beyond the points that qualify hold (+inf, -1), and so
 *                        does the row of a query with a non-finite coordinate.  order, index, index_bytes, levels and
 *                        skip_counts as mslam_cloud_distance: the same bits in the three forms, and k = 1 without
 *                        exclude is mslam_cloud_distance's output.  `order` names no point twice.
 *   mslam_cloud_normals  one normal per point from row i of neighbors i32[N,k] (the k-NN of the cloud in itself without
 *                        exclude; entries outside [0, N) are no neighbours), all in f64: count i32[N] = m, the entries
 *                        that are neighbours (0 for an invalid point); the centroid (the sum in list order / m) and the
 *                        covariance (the six sums of products of the differences from it, in list order, each / m);
 *                        its eigenvectors by cyclic Jacobi; normals f32[N,3] the unit eigenvector of the smallest
 *                        eigenvalue, turned towards the viewpoint (viewpoints f32[3] with viewpoint_stride 0, f32[N,3]
 *                        with 3; exactly perpendicular: not turned) or, with viewpoints NULL, so that its component of
 *                        largest magnitude is positive; curvature f32[N] = max(l_min, 0) / (l0 + l1 + l2).  m < 3 or
 *                        a middle eigenvalue <= 2^-40 of the largest: normal (0, 0, 0) and curvature NaN.  moments
 *                        (may be NULL, for tests): f64[N, MSLAM_CLOUD_NORMALS_MOMENTS] - the centroid, the covariance
 *                        xx xy xz yy yz zz, the three eigenvalues in the order of their columns, and the oriented
 *                        normal before its rounding to f32. */
#define MSLAM_CLOUD_KNN_MAX_K 32
#define MSLAM_CLOUD_NORMALS_MOMENTS 15
int mslam_cloud_knn(const float* queries, int n, const float* points, int num_points, int k, const int32_t* exclude,
                    const int32_t* order, const void* index, size_t index_bytes, int levels, int32_t* skip_counts,
                    double* dist2, int32_t* neighbors, void* stream);
int mslam_cloud_normals(const float* points, int num_points, const int32_t* neighbors, int k, const float* viewpoints,
                        int viewpoint_stride, float* normals, float* curvature, int32_t* count, double* moments,
                        void* stream);

/* Cloud clusters: the points within a radius and density clustering, DBSCAN (no counterpart in the reference, DESIGN.md
 * "Cloud clusters"; the definition is tests/cloud_cluster_numpy.py; csrc/cloud_cluster.hip).  d2 is
 * mslam_cloud_distance's sum, the same bits for (i, j) and (j, i); "within" is d2 <= eps2, eps2 >= 0 an f64 taken as it
 * is (+inf: everything).  order, index, index_bytes, levels and skip_counts as mslam_cloud_distance: order NULL is the
 * plain scan; with an index a tile or group whose box lies beyond eps2 is not scanned; the same bytes in the three forms.
 *   mslam_cloud_radius_count     count i32[n]: the valid points of the cloud within eps2 of each query (a point of the
 *                                cloud counts itself and its duplicates; not capped); 0 for a query with a non-finite
 *                                coordinate.  No atomics.
 *   mslam_cloud_cluster_init     parent i32[N]: parent[v] = v.
 *   mslam_cloud_cluster_link     the cloud in itself; row q of n stands for point self[q] (self i32[n]; NULL: the
 *                                identity; an entry outside [0, N) is skipped, never followed).  core u8[N] (only read):
 *                                the caller's valid && count >= min_points.  parent i32[N], in and out, touched only
 *                                through atomics: a core row i unites (i, j) for every core j < i within eps2, in a
 *                                lock-free union-find with parent[v] <= v that never waits.  A row that is not core keeps
 *                                the core point smallest under the total order (d2, index) among those within eps2.
 *                                anchor i32[n] / anchor_dist2 f64[n]: (the row's own point, 0) for a core row, (that core
 *                                point, its d2) for a border row, (-1, +inf) for noise, an invalid point or a skipped row.
 *   mslam_cloud_cluster_flatten  parent[v] = its root, the smallest index of its tree, in a launch of its own; after the
 *                                link of every point that is the smallest core index of v's cluster (v itself for a
 *                                point that is not core), whatever order the atomics landed in.
 *   mslam_cloud_cluster_labels   with anchor i32[N] in point order: label_root i32[N] = root[anchor[i]], -1 where the
 *                                anchor is outside [0, N); is_cluster_root u8[N] = core[v] && root[v] == v.  Numbering
 *                                the roots and the sizes are the caller's integer work. */
int mslam_cloud_radius_count(const float* queries, int n, const float* points, int num_points, double eps2,
                             const int32_t* order, const void* index, size_t index_bytes, int levels,
                             int32_t* skip_counts, int32_t* count, void* stream);
int mslam_cloud_cluster_init(int num_points, int32_t* parent, void* stream);
int mslam_cloud_cluster_link(const float* points, int num_points, const int32_t* self, int n, double eps2,
                             const uint8_t* core, const int32_t* order, const void* index, size_t index_bytes,
                             int levels, int32_t* skip_counts, int32_t* parent, int32_t* anchor, double* anchor_dist2,
                             void* stream);
int mslam_cloud_cluster_flatten(int num_points, int32_t* parent, void* stream);
int mslam_cloud_cluster_labels(const int32_t* root, const uint8_t* core, const int32_t* anchor, int num_points,
                               int32_t* label_root, uint8_t* is_cluster_root, void* stream);

/* Cloud smoothing: one step of the moving-least-squares projection in its plane form (no counterpart in the reference,
 * DESIGN.md "Cloud smoothing"; the definition is tests/cloud_mls_numpy.py; csrc/cloud_mls.hip).  All f64 on the f32
 * inputs, one multiply or add at a time.  d2 is mslam_cloud_distance's sum; a valid point q of the cloud JOINS query p
 * when d2 <= h2 (h2 finite and > 0) and, with normals, passes the gate.  inv = 1 / h2, u = 1 - d2 inv, w = u u (a
 * neighbour at d2 == h2 counts with weight 0), r = q - p; per joining neighbour, in the order of the walk: S0 += w; wx =
 * w rx, S1x += wx, Sxx += wx rx, Sxy += wx ry, Sxz += wx rz; wy = w ry, S1y += wy, Syy += wy ry, Syz += wy rz; wz = w rz,
 * S1z += wz, Szz += wz rz; count += 1.  Then m = S1 / S0, C = S2 / S0 - m m^T entry by entry (zeros unless S0 > 0), its
 * eigenvectors by cyclic Jacobi, the unit eigenvector n of the smallest eigenvalue with its component of largest
 * magnitude positive, t = (nx mx + ny my) + nz mz and
 *   out_points     f32[n,3] = (float)(p + (strength t) n), strength in [0, 1].  A query STAYS - its input bits are
 *                  copied, NaN payloads included - when a coordinate is not finite, when count < min_points (>= 1),
 *                  when count < 3 or when the fit is degenerate (a middle eigenvalue <= 2^-40 of the largest).
 *                  out_points may alias neither queries nor points.
 *   out_normals    f32[n,3] = n, (0, 0, 0) for a query that stays;  out_curvature f32[n] = max(l_min, 0) / (l0 + l1 +
 *                  l2), NaN for a query that stays;  out_count i32[n] = count in every case (0 for an invalid query), not
 *                  capped.
 *   the gate       query_normals f32[n,3] and point_normals f32[N,3], both or neither (NULL may also stand for the one
 *                  that has no rows): neighbour j joins only when
 *                  fabs((ax bx + ay by) + az bz) >= cos_gate (in [0, 1]), a the query's normal and b point_normals[j].
 *                  A query whose normal is (0, 0, 0) or not finite is not gated; a neighbour's normal that is not
 *                  finite counts as (0, 0, 0), which fails every cos_gate > 0.
 *   moments        (may be NULL, for tests) f64[n, MSLAM_CLOUD_MLS_MOMENTS]: S0, S1 (3), S2 as xx xy xz yy yz zz, the
 *                  three diagonal entries after the sweeps, the signed unit normal before its rounding (zeros when the
 *                  query stays), t (0 when it stays) and one spare word, 0.
 * order, index, index_bytes, levels and skip_counts as mslam_cloud_radius_count.  THE ORDER OF THE SUMS IS THE WALK'S:
 * ascending point index with order NULL, order[0], order[1], ... with an index.  Levels 1 and 2 give the same bytes (a
 * skipped tile holds only points with d2 > h2, which add nothing); the plain and the indexed form differ by rounding,
 * since f64 sums depend on their order.  No atomics.  Bad arguments (a negative size, h2 not finite and > 0, min_points
 * < 1, strength or cos_gate outside [0, 1], one normal pointer without the other, a null output with n > 0) return
 * MSLAM_EINVAL and nothing is written; n == 0 returns MSLAM_OK after these checks; num_points == 0: every query stays. */
#define MSLAM_CLOUD_MLS_MOMENTS 18
int mslam_cloud_mls_step(const float* queries, int n, const float* points, int num_points, double h2, int min_points,
                         double strength, const float* query_normals, const float* point_normals, double cos_gate,
                         const int32_t* order, const void* index, size_t index_bytes, int levels, int32_t* skip_counts,
                         float* out_points, float* out_normals, float* out_curvature, int32_t* out_count,
                         double* moments, void* stream);

/* Cloud planes: which planes a cloud consists of, by sequential RANSAC (no counterpart in the reference, DESIGN.md
 * "Cloud planes"; the definition is tests/cloud_planes_numpy.py; csrc/cloud_planes.hip).  f64 on the f32 inputs, one
 * multiply or add at a time; integer counts; no float atomics; the same bytes on every call.  A point SUPPORTS the plane
 * (n, d) when |((nx px + ny py) + nz pz) + d| <= tol and, with normals f32[N,3] (may be NULL), its normal m is finite
 * and not zero and |(nx mx + ny my) + nz mz| >= cos_angle.  One round finds one plane; nothing is read back between
 * rounds.  state i32[MSLAM_CLOUD_PLANES_STATE]: M (the remaining list's length), planes_found, done, the chosen
 * hypothesis, its count, and whether the refit has stopped; every stage but the compaction returns at once when done is
 * set.  fit f64[MSLAM_CLOUD_PLANES_FIT]: the current plane (4), the origin (3, one spare), the
 * MSLAM_CLOUD_PLANES_SUMS sums of its supporters (count, q, q q^T as xx xy xz yy yz zz, r^2; q = p - origin), the
 * refit's candidate (4) and its scratch.  num_remaining: the length of the buffer `remaining`, an upper bound of M.
 *   mslam_cloud_planes_remaining  remaining i32[N]: the indices of the valid points (finite coordinates) with
 *                                 labels[i] < 0, ascending, by a stable scan; block_offsets i32[ceil(N / 256)] is its
 *                                 scratch.  state: M, and done when M < max(3, min_points).
 *   mslam_cloud_planes_draw       hypotheses f64[H,4], triples i32[H,3]: hypothesis h of `round` takes the points
 *                                 remaining[draw(seed, round, h, j)], j = 0, 1, 2, draw = mix(mix(mix(seed) ^ ((round <<
 *                                 32) | h)) ^ j) mod M with mix SplitMix64's finaliser; n = (p1 - p0) x (p2 - p0) over
 *                                 its length sqrt((nx nx + ny ny) + nz nz), d = -((nx p0x + ny p0y) + nz p0z).  A void
 *                                 hypothesis (two equal draws, a length not finite and > 0, M = 0) is four NaNs.
 *   mslam_cloud_planes_count      count i32[H]: the supporters of each hypothesis among the remaining points.
 *   mslam_cloud_planes_select     the largest count, the lowest h on ties, into state; a count below min_points (or
 *                                 below 1) sets done; else fit holds the hypothesis and its origin, the point
 *                                 triples[h][0].
 *   mslam_cloud_planes_refit      `iterations` times: a candidate from the sums of the plane's supporters (the
 *                                 eigenvector of the smallest eigenvalue of their covariance, d at the centroid)
 *                                 replaces the plane unless the fit is degenerate (fewer than 3 supporters, a middle
 *                                 eigenvalue <= 2^-40 of the largest) or the candidate has fewer supporters, which ends
 *                                 the refit.  partial f64[MSLAM_CLOUD_PLANES_SUMS ceil(num_remaining / 256)] is its
 *                                 scratch.  fit ends with the plane and the sums of its supporters.
 *   mslam_cloud_planes_label      the supporters of fit's plane get the label planes_found; planes
 *                                 f64[max_planes, MSLAM_CLOUD_PLANES_ROW] gains the row n (3), d, count, sum r^2, the
 *                                 centroid (3), the eigenvalues of the supporters' covariance (3), sqrt(sum r^2 / count); n and d negated
 *                                 together when the viewpoint f32[3] lies on the negative side or, with viewpoint NULL,
 *                                 when n's component of largest magnitude (lowest axis on ties) is negative; then
 *                                 planes_found grows by one.
 *   mslam_cloud_planes            the whole call: state and labels (-1) are initialised, then max_planes rounds are
 *                                 enqueued.  workspace: mslam_cloud_planes_workspace_bytes(N, H) bytes, 16-byte aligned.
 * Bad arguments (a null or misaligned pointer, H outside [1, MSLAM_CLOUD_PLANES_MAX_HYPOTHESES], max_planes outside
 * [1, MSLAM_CLOUD_PLANES_MAX_PLANES], tol not finite and > 0, cos_angle outside [0, 1], min_points < 1) return
 * MSLAM_EINVAL, a workspace that is too small MSLAM_ENOMEM, and nothing is written. */
#define MSLAM_CLOUD_PLANES_MAX_HYPOTHESES 1024
#define MSLAM_CLOUD_PLANES_MAX_PLANES 64
#define MSLAM_CLOUD_PLANES_STATE 8
#define MSLAM_CLOUD_PLANES_FIT 40
#define MSLAM_CLOUD_PLANES_SUMS 11
#define MSLAM_CLOUD_PLANES_ROW 13
int mslam_cloud_planes_remaining(const float* points, int num_points, const int32_t* labels, int min_points,
                                 int32_t* block_offsets, int32_t* remaining, int32_t* state, void* stream);
int mslam_cloud_planes_draw(const float* points, int num_points, const int32_t* remaining, int num_remaining,
                            const int32_t* state, uint64_t seed, int round, int num_hypotheses, double* hypotheses,
                            int32_t* triples, void* stream);
int mslam_cloud_planes_count(const float* points, const float* normals, int num_points, const int32_t* remaining,
                             int num_remaining, const int32_t* state, const double* hypotheses, int num_hypotheses,
                             double tol, double cos_angle, int32_t* count, void* stream);
int mslam_cloud_planes_select(const int32_t* count, int num_hypotheses, int min_points, const float* points,
                              int num_points, const double* hypotheses, const int32_t* triples, int32_t* state,
                              double* fit, void* stream);
int mslam_cloud_planes_refit(const float* points, const float* normals, int num_points, const int32_t* remaining,
                             int num_remaining, double tol, double cos_angle, int iterations, double* partial,
                             int32_t* state, double* fit, void* stream);
int mslam_cloud_planes_label(const float* points, const float* normals, int num_points, const int32_t* remaining,
                             int num_remaining, double tol, double cos_angle, const float* viewpoint, const double* fit,
                             int max_planes, int32_t* state, int32_t* labels, double* planes, void* stream);
size_t mslam_cloud_planes_workspace_bytes(int num_points, int num_hypotheses);
int mslam_cloud_planes(const float* points, const float* normals, int num_points, double tol, double cos_angle,
                       int max_planes, int min_points, int num_hypotheses, int refit_iterations, uint64_t seed,
                       const float* viewpoint, void* workspace, size_t workspace_bytes, int32_t* labels, double* planes,
                       int32_t* state, void* stream);

/* Point-to-plane ICP for clouds and meshes: one fused step and a Gauss-Newton solve on Sim3 per iteration (no
 * counterpart in the reference, DESIGN.md "Point-to-plane ICP"; the definition is tests/icp_plane_numpy.py;
 * csrc/icp_plane.hip).  The state block and its init and read are mslam_mesh_align_init / _init_indexed / _read; all
 * arithmetic is f64 on the f32 inputs; every sum is reduced in mslam_mesh_align_step's fixed order without atomics.
 * A step moves src f32[n,3] by the state (moved, rounded once to f32), finds each moved sample's nearest primitive
 * (dist2, nearest: the bits of mslam_cloud_distance / mslam_mesh_distance on `moved`; closest f64[n,3], may be NULL:
 * the nearest point, or the closest point of the nearest face, NaN without one), takes the target's normal there (the
 * given normals f32[N,3] of a cloud as they are; a face's ((b - a) x (c - a)) normalised in f64) and accumulates, about
 * o = moved[0] with a = q - o, e = q - c, the plane row r = n . e, J = [n, a x n, n . a] and, with point_weight > 0, the
 * three point rows r_d = e_d, J_d = [u_d, a x u_d, a_d] weighted by point_weight.  A pair counts when it has a
 * neighbour, dist2 <= trim^2 and a finite non-zero normal; with point_weight > 0 a pair without a normal counts with
 * its point rows alone.  The solve scales H = sum J^T J to unit diagonal, factors it by Cholesky, solves H xi = -g for
 * xi = (tau, omega, sigma) (with_scale = 0: without sigma) and composes x -> o + e^sigma R(omega) (x - o) + tau onto
 * the state.  MSLAM_MESH_ALIGN_DEGENERATE, the state left as it was: fewer pairs than unknowns, a zero or non-finite
 * diagonal entry, a pivot of the scaled matrix <= 2^-40, a non-finite xi or scale.
 *   log_row    f64[MSLAM_ICP_PLANE_LOG_DOUBLES]: the pairs that count, sqrt((sum r^2 + point_weight sum dist2) / sum w)
 *              (+inf without a pair), the scale after the solve, the status, the point rmse sqrt(sum dist2 / sum w),
 *              normal_spread - the smallest eigenvalue of H's 3 x 3 translation block over sum w, 0 when some
 *              translation is not constrained - then the MSLAM_ICP_PLANE_SUMS sums: count, sum w, sum r^2, sum dist2,
 *              g (7), the upper triangle of H row by row (28).
 *   workspace  mslam_icp_plane_workspace_bytes(n, F): F faces' tile boxes (mslam_mesh_align_init writes them; 0 for a
 *              cloud and for the indexed form) and one partial per block of 256 samples.
 *   mslam_icp_plane_step_cloud         order NULL: the plain scan; else `index` is mslam_cloud_index_boxes' workspace
 *                                      and levels as in mslam_cloud_distance.  The same bits in the three forms.
 *   mslam_icp_plane_step_mesh          `nearest` is read first as a warm start, as in mslam_mesh_align_step.
 *   mslam_icp_plane_step_mesh_indexed  over a mesh index, as mslam_mesh_align_step_indexed. */
#define MSLAM_ICP_PLANE_SUMS 39
#define MSLAM_ICP_PLANE_LOG_DOUBLES 45
size_t mslam_icp_plane_workspace_bytes(int n, int num_faces);
int mslam_icp_plane_step_cloud(const float* src, int n, const float* points, const float* normals, int num_points,
                               const int32_t* order, const void* index, size_t index_bytes, int levels, double trim,
                               double point_weight, int with_scale, void* workspace, size_t workspace_bytes,
                               void* state, int32_t* nearest, float* moved, double* dist2, double* closest,
                               double* log_row, void* stream);
int mslam_icp_plane_step_mesh(const float* src, int n, const float* vertices, const int32_t* faces, int num_faces,
                              int num_vertices, double trim, double point_weight, int with_scale, void* workspace,
                              size_t workspace_bytes, void* state, int32_t* nearest, float* moved, double* dist2,
                              double* closest, double* log_row, void* stream);
int mslam_icp_plane_step_mesh_indexed(const float* src, int n, const float* vertices, const int32_t* faces,
                                      int num_faces, int num_vertices, const int32_t* order, const void* index,
                                      size_t index_bytes, double trim, double point_weight, int with_scale,
                                      void* workspace, size_t workspace_bytes, void* state, int32_t* nearest,
                                      float* moved, double* dist2, double* closest, double* log_row, void* stream);

/* Cloud views: the z-buffer splat of a cloud into pinhole views and the observed part of a cloud (no counterpart in the
 * reference, DESIGN.md "Cloud views"; the definition is tests/cloudview_numpy.py; csrc/cloud_view.hip).  A view is a
 * pose f32[8] (Sim3 [t,q,s], world from camera), the pinhole fx, fy, cx, cy and an image of h x w, h w num_views < 2^31.
 * All in f64 on the f32 inputs: v = p - t, X = R(q)^T v, r = |v|, u = fx X0 / X2 + cx, v = fy X1 / X2 + cy; p is IN the
 * view when its coordinates are finite, X2 > 0, -0.5 <= u < w - 0.5, -0.5 <= v < h - 0.5 and near <= r <= far (world
 * units); its pixel is (floor(u + 0.5), floor(v + 0.5)).
 *   mslam_cloud_view_splat    zbuf u64[num_views,h,w], set to all ones (empty) here, on the stream, and then, per view,
 *                             lowered at every pixel of the square |dx|, |dy| <= rho around the pixel of every point in
 *                             view, clipped to the image, to the minimum of (bits of f32(r)) << 32 | index: the nearest
 *                             f32 range wins, then the lowest index; the same bytes on every call.  rho = radius, or with
 *                             point_size >= 0 (a world-unit diameter; negative: none) min(max_radius, max(radius,
 *                             floor(0.5 point_size max(fx, fy) / X2))), the min taken in f64.  0 <= radius <= max_radius
 *                             <= MSLAM_CLOUD_VIEW_MAX_RADIUS.  counters (NULL outside measurements): u64[2], the
 *                             footprint pixels visited and the atomics issued are ADDED to it.
 *   mslam_cloud_view_resolve  per pixel of zbuf: hit u8 (not empty), index i32 (-1 on a miss), range f32 = f32(f64(r32) /
 *                             s) for the view's scale s, so that range * ray is the camera-frame point (0 on a miss);
 *                             with colors u8[num_points,3], rgb u8[num_views,h,w,3], the winner's colour, 0 on a miss
 *                             (NULL together).
 *   mslam_cloud_view_visible  seen u8[num_queries]: set to 1 where, for some view, the query is in the view and its own
 *                             pixel is empty or f64(f32(r_query)) <= f64(r32 of the pixel) (1 + rel_tol) + tol.  `seen`
 *                             is the caller's: it is never cleared, and a query that is already marked is not looked at.
 * Bad arguments (a negative size, radius > max_radius, max_radius > 8, h w num_views >= 2^31, near > far, a negative
 * tolerance) return MSLAM_EINVAL and nothing is written. */
#define MSLAM_CLOUD_VIEW_MAX_RADIUS 8
int mslam_cloud_view_splat(const float* points, int num_points, const float* poses, int num_views, double fx, double fy,
                           double cx, double cy, int h, int w, double near, double far, int radius, double point_size,
                           int max_radius, uint64_t* zbuf, uint64_t* counters, void* stream);
int mslam_cloud_view_resolve(const uint64_t* zbuf, const float* poses, int num_views, int h, int w,
                             const uint8_t* colors, int num_points, float* range, int32_t* index, uint8_t* hit,
                             uint8_t* rgb, void* stream);
int mslam_cloud_view_visible(const float* queries, int num_queries, const uint64_t* zbuf, const float* poses,
                             int num_views, double fx, double fy, double cx, double cy, int h, int w, double near,
                             double far, double tol, double rel_tol, uint8_t* seen, void* stream);

/* Mesh textures: keyframe images baked into a per-face atlas, and the shading of a ray cast (no counterpart in the
 * reference, DESIGN.md "Mesh textures"; the definition is tests/texture_numpy.py).  The atlas is a pure function of
 * (F, texels = R >= 4): face f is half f & 1 of cell f >> 1, a cell is R + 1 texels wide and R high, the cells lie
 * row-major in `cols` columns and `rows` rows (cols * rows >= (F + 1) / 2), H = rows R, W = cols (R + 1), n = H W < 2^31.
 * All arithmetic is f64 on the f32 inputs in one fixed order; one thread per texel, no atomics; nothing but the outputs
 * is written.  A face with an index outside [0, V) is seen by no view and takes the default colour.
 *   mslam_mesh_texture_layout      owner i32[n]: the face that owns each texel, -1 for none.
 *   mslam_mesh_texture_rays        one view: pose8 f32[8] (Sim3 [t,q,s], world from camera), pinhole fx, fy, cx, cy, an
 *                                  image of h x w >= 2x2.  Per texel the point p of its face at the texel's clamped
 *                                  barycentrics, v = p - t, r = |v|, cos = -(n . v) / r for the face's unit normal n.
 *                                  Where z > 0, -0.5 <= u < w - 0.5, -0.5 <= v < h - 0.5, near <= r <= far and
 *                                  cos >= cos_min and > 0: dir f32[n,3] = v / r (the occlusion ray from t), r f64[n],
 *                                  cos f64[n], uv f64[n,2]; zeros everywhere else.
 *   mslam_mesh_texture_accumulate  one view, after mslam_mesh_raycast of `dir` from t (h = 1, identity rotation, near 0,
 *                                  far inf) gave t64: a texel with cos > 0 and t64 >= r - tol adds wgt = (cos (s / r))
 *                                  (s / r) and wgt times the bilinear sample of image f32[h,w,3] at uv into sums
 *                                  f64[n,4], and 1 into views i32[n].  The caller zeroes both before the first view.
 *   mslam_mesh_texture_resolve     atlas f32[n,3]: sums[1..3] / sums[0] where sums[0] > 0; otherwise the vertex colours
 *                                  colors f32[V,3] (may be NULL) at the texel's barycentrics, or default_color; 0
 *                                  without an owner.
 *   mslam_mesh_shade               rgb f32[h*w,3] of a ray cast: for every pixel with face[i] >= 0 the edge functions
 *                                  U, V, W of that face as mslam_mesh_raycast computes them (same rays, h, w, pose8) and
 *                                  det = (U + V) + W; with colors f32[V,3]: ((U ca + V cb) + W cc) / det; with an atlas
 *                                  f32[H,W,3] (and texels, cols, rows): its bilinear sample at the atlas coordinates of
 *                                  beta = V / det, gamma = W / det.  Exactly one of the two is given.  0 on a miss. */
int mslam_mesh_texture_layout(int num_faces, int texels, int cols, int rows, int32_t* owner, void* stream);
int mslam_mesh_texture_rays(const float* vertices, const int32_t* faces, int num_faces, int num_vertices, int texels,
                            int cols, int rows, const float* pose8, double fx, double fy, double cx, double cy, int h,
                            int w, double near, double far, double cos_min, float* dir, double* r, double* cos,
                            double* uv, void* stream);
int mslam_mesh_texture_accumulate(const double* t64, const double* r, const double* cos, const double* uv,
                                  const float* image, int h, int w, const float* pose8, double tol, int n, double* sums,
                                  int32_t* views, void* stream);
int mslam_mesh_texture_resolve(const int32_t* faces, int num_faces, int num_vertices, int texels, int cols, int rows,
                               const double* sums, const float* colors, double default_color, float* atlas,
                               void* stream);
int mslam_mesh_shade(const int32_t* face, const float* rays, int h, int w, const float* pose8, const float* vertices,
                     const int32_t* faces, int num_faces, int num_vertices, const float* colors, const float* atlas,
                     int texels, int cols, int rows, float* rgb, void* stream);

/* Mesh textures, the sized atlas (DESIGN.md "Mesh textures: sized atlas"; the definition is
 * tests/texture_sized_numpy.py).  Every face has its own R_f, one of the 13 classes 4, 6, 8, 12, 16, 24, ..., 192, 256
 * (class c has R = (c odd ? 6 : 4) << (c / 2)); the cells of a class lie in one band of the atlas.  Inside a cell
 * everything is the uniform atlas's with R_f for R.  256-thread blocks, integers and f64 in one fixed order, no atomics,
 * nothing but the outputs written, bit-identical from call to call.
 *   mslam_mesh_texture_classes        per face cls i32[F], the class index of R_f, and clamped i32[F] (0 / 1):
 *                                     L = max(max(e_ab, e_bc), e_ca), e = sqrt((dx dx + dy dy) + dz dz) in f64,
 *                                     need = ceil(density L + 3.5); the smallest class >= need, at least floor_class, at
 *                                     most cap_class; clamped where need exceeds the cap's R.  A face with an index
 *                                     outside [0, V) or an edge that is not finite: floor_class, not clamped.
 *   mslam_mesh_texture_rank_table_ints  the ints of `table` below: 14 (ceil(F / 256) + 1).
 *   mslam_mesh_texture_rank           the stable counting sort by class in three launches: rank i32[F] = the faces of a
 *                                     smaller index in the same class; order i32[F] = the faces class by class, largest
 *                                     R first, each by rising index; counts i32[14] = the 13 class counts and the
 *                                     number of clamped faces (also written for F = 0).  `table` is device scratch of
 *                                     the caller's.
 *   mslam_mesh_texture_layout_sized   bands: 13 rows (R, cols, rows, y0, base, count) of int32 in HOST memory, read
 *                                     before the call returns and checked against (F, H, W): bands from the largest
 *                                     class down, y0 and base the running sums of rows R and count.  owner i32[H W] and
 *                                     face_cell i32[F,4] = (x0, y0, R_f, half): face f is half k & 1 of cell k >> 1 of
 *                                     its band, k its rank; texels right of a band's last column, in unused cells and
 *                                     in the absent half of an odd class's last cell have owner -1.
 *   mslam_mesh_texture_rays_sized,
 *   mslam_mesh_texture_resolve_sized  mslam_mesh_texture_rays / _resolve on the texels of the sized atlas: the texel's
 *                                     face from owner, its local (i, j) = (x - x0, y - y0), mirrored (R - i, R - 1 - j)
 *                                     for half 1, from face_cell; an owner outside [0, F) counts as none.
 *                                     mslam_mesh_texture_accumulate serves both atlases.
 *   mslam_mesh_shade_sized            mslam_mesh_shade from a sized atlas f32[H,W,3]: the cell of the face hit from
 *                                     face_cell; a cell that does not lie inside the atlas shades as a miss. */
int mslam_mesh_texture_classes(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                               double density, int floor_class, int cap_class, int32_t* cls, int32_t* clamped,
                               void* stream);
size_t mslam_mesh_texture_rank_table_ints(int num_faces);
int mslam_mesh_texture_rank(const int32_t* cls, const int32_t* clamped, int num_faces, int32_t* table,
                            size_t table_ints, int32_t* rank, int32_t* order, int32_t* counts, void* stream);
int mslam_mesh_texture_layout_sized(const int32_t* bands, int num_faces, int H, int W, const int32_t* cls,
                                    const int32_t* rank, const int32_t* order, int32_t* owner, int32_t* face_cell,
                                    void* stream);
int mslam_mesh_texture_rays_sized(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                                  const int32_t* owner, const int32_t* face_cell, int H, int W, const float* pose8,
                                  double fx, double fy, double cx, double cy, int h, int w, double near, double far,
                                  double cos_min, float* dir, double* r, double* cos, double* uv, void* stream);
int mslam_mesh_texture_resolve_sized(const int32_t* faces, int num_faces, int num_vertices, const int32_t* owner,
                                     const int32_t* face_cell, int H, int W, const double* sums, const float* colors,
                                     double default_color, float* atlas, void* stream);
int mslam_mesh_shade_sized(const int32_t* face, const float* rays, int h, int w, const float* pose8,
                           const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                           const float* atlas, const int32_t* face_cell, int H, int W, float* rgb, void* stream);

/* Colour of the volume (no counterpart in the reference, DESIGN.md "Colour").  `color` is a second caller-owned device
 * buffer of mslam_tsdf_color_bytes(capacity) bytes, addressed by the slot index of `table`: four u64 words per slot,
 * sum_w (units of 2^-20), sum_w * r8, sum_w * g8, sum_w * b8 with 8-bit colours.  The sums are integers: the fused
 * colour is bit-identical for any order of arrival, capacity and shard count.
 *   mslam_tsdf_integrate_color  after mslam_tsdf_integrate of the same points (so the voxels exist): walks the same
 *                               samples with the same weights, rgb f32[n,3] in [0,1]; a sample whose voxel is not in
 *                               this table is skipped.  The table is only read.
 *   mslam_tsdf_color_rehash     after mslam_tsdf_rehash: every old slot finds its key in the new table and moves its words.
 *   mslam_tsdf_color_dump       sums u64[n,4] of the voxels keys i64[n,3] (zeros for a voxel that is not in the table).
 *   mslam_tsdf_color_load       counterpart of mslam_tsdf_load (call it after that): stores sums u64[n,4] at keys i64[n,3].
 *   mslam_tsdf_color_sample     trilinear colour at world points f32[n,3] on the lattice of the mesh and the views
 *                               (g = p / vs - 0.5, corner c = dx + 2 dy + 4 dz, a + f (b - a) along x, y, z in f64); a
 *                               corner without colour contributes the default colour; out_rgb f32[n,3], out_count
 *                               u8[n] = coloured corners.  image_w > 0: the points are image rows of image_w pixels
 *                               (shapes the 8x8-pixel wave tiles only), 0: a plain list. */
size_t mslam_tsdf_color_bytes(uint64_t capacity);
int mslam_tsdf_color_init(void* color, size_t color_bytes, uint64_t capacity, void* stream);
int mslam_tsdf_integrate_color(void* table, uint64_t capacity, void* color, const float* points_world,
                               const double* conf, const float* rgb, const float* cam_origin, int n_points,
                               double voxel_size, double trunc, double step_scale, void* stream);
int mslam_tsdf_color_rehash(void* old_table, uint64_t old_capacity, const void* old_color, void* new_table,
                            uint64_t new_capacity, void* new_color, void* stream);
int mslam_tsdf_color_dump(void* table, uint64_t capacity, const void* color, const int64_t* keys, int n, uint64_t* sums,
                          void* stream);
int mslam_tsdf_color_load(void* table, uint64_t capacity, void* color, const int64_t* keys, const uint64_t* sums, int n,
                          void* stream);
int mslam_tsdf_color_sample(void* table, uint64_t capacity, const void* color, const float* points, int n, int image_w,
                            double voxel_size, double default_r, double default_g, double default_b, float* out_rgb,
                            uint8_t* out_count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Render quality (NOT a reference interface): PSNR and SSIM of image pairs in one pass (csrc/image_metrics.hip,
 * DESIGN.md "Render quality"; the definition is tests/imgmetrics_numpy.py).
 *   a, b f32[n,h,w,c] (c in 1..4, data range 1), mask u8[n,h,w] (torch.bool storage) or NULL = all pixels.
 *   window  f64[11]: the normalised Gaussian taps (sigma 1.5), computed once by the caller.
 *   sums    f64[n,2]: the squared error over masked-in pixels and channels; S over valid window centres and channels.
 *   counts  i64[n,2]: n_pixels (masked-in); n_windows (centres whose 11x11 window lies in the image and is masked-in).
 *   ssim_map f32[n,h,w] or NULL: the channel mean of S at valid centres, NaN elsewhere.
 * A MSLAM_IMAGE_METRICS_TILE_H x _TILE_W tile of centres per 256-thread workgroup; the workspace holds one partial per
 * workgroup and quantity, which a second launch adds in block order: no atomics, bit-identical results from call to
 * call and for any position of an image in the batch.  h or w below 11 is legal (n_windows = 0). */
#define MSLAM_IMAGE_METRICS_TILE_H 16
#define MSLAM_IMAGE_METRICS_TILE_W 32
size_t mslam_image_metrics_workspace_bytes(int n, int h, int w, int c);
int mslam_image_metrics(const float* a, const float* b, const uint8_t* mask, int n, int h, int w, int c,
                        const double* window, double* sums, int64_t* counts, float* ssim_map, void* workspace,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * MASt3R two-view forward. Replaces the three model methods the SLAM front/back-end call
 * (mast3r_slam/mast3r_utils.py:34-40,57-64,74): model._encode_image, model._decoder,
 * model._downstream_head (thirdparty/mast3r/dust3r/dust3r/model.py:127-139,171-196;
 * mast3r/catmlp_dpt_head.py:71-96).  bf16 MFMA operands, fp32 accumulate / residual / softmax.
 *
 * create: cfg9 = {enc_dim, enc_depth, enc_heads, dec_dim, dec_depth, dec_heads, patch, desc_dim,
 * dpt_feature_dim}; weight_ptrs = DEVICE pointers in the canonical order documented in
 * mast3r_slam/mast3r_model.py::canonical_weights (matrices bf16 [out,in] with conv kernels
 * re-laid-out tap-major, biases / LayerNorm / last 1x1 conv fp32), weight_numels their element
 * counts (validated).  The model keeps the pointers; the caller keeps the tensors alive.
 * SYNCHRONISES the stream once (RoPE table upload).
 * ------------------------------------------------------------------------------------------ */
int mslam_mast3r_create(void** handle_out, const int* cfg9_host, void* const* weight_ptrs_host,
                        const long long* weight_numels_host, int n_weights, void* stream);
int mslam_mast3r_destroy(void* handle);
size_t mslam_mast3r_workspace_bytes(void* handle, int batch, int H, int W);

/* _encode_image: img f32[B,3,H,W] (ImgNorm range) -> feat f32[B, (H/16)(W/16), enc_dim]
 * (enc_norm output).  pos is implicit: token n = (y = n / (W/16), x = n % (W/16)). */
int mslam_mast3r_encode(void* handle, const float* img, int batch, int H, int W, float* feat_out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* _decoder + both _downstream_head calls of mast3r_utils.decoder (mast3r_utils.py:34-40):
 * feat1, feat2 f32[B,N,enc_dim] -> for side s in {1,2}: X f32[B,H,W,3] (pts3d), C f32[B,H,W]
 * (conf), D f32[B,H,W,desc_dim] (desc), Q f32[B,H,W] (desc_conf).  dec_last1/2 (may be NULL):
 * f32[B,N,dec_dim] = dec_norm'ed last decoder tokens (for tests). */
int mslam_mast3r_decode(void* handle, const float* feat1, const float* feat2, int batch, int H, int W,
                        float* X1, float* C1, float* D1, float* Q1, float* X2, float* C2, float* D2,
                        float* Q2, float* dec_last1, float* dec_last2, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Frame-to-keyframe tracking GN.  Replaces FrameTracker.opt_pose_ray_dist_sim3 /
 * opt_pose_calib_sim3 + solve (mast3r_slam/tracker.py:208-318; geometry.py:17-104;
 * nonlinear_optimizer.py:5-33): <= max_iters Gauss-Newton iterations on the relative Sim3
 * T_CkCf (f32[8] device, updated IN PLACE), residuals between keyframe points Xk f32[n,3] and
 * T.Xf[idx_f2k] (Xf f32[n,3], idx i64[n]), weights sqrt(Qk) (f32[n]) gated by valid (u8[n]).
 * use_calib: pixel + log-depth residual with K f32[3,3] (device).  No host sync: convergence
 * (rel. cost decrease < rel_error or |tau| < delta_norm) is a device flag.  status_out (device,
 * 32 bytes, may be NULL) <- {i32 done, i32 iters, i32 chol_fail, f32 old_cost, f32 last_cost,
 * f32 last_delta_norm, -, -}; chol_fail mirrors the exception path of tracker.py:72-93.
 * The loop state lives in `workspace`: iterations [first_iter, max_iters) are enqueued, first_iter == 0 resets the
 * state, so a caller may enqueue a first chunk, read the status and continue only when `done` is still 0.
 * ------------------------------------------------------------------------------------------ */
size_t mslam_track_workspace_bytes(int n_points);
int mslam_track_pose(int use_calib, float* T_rel, const float* Xf, const float* Xk, const int64_t* idx_f2k,
                     const float* Qk, const uint8_t* valid, int n_points, const float* K, int width,
                     int height, float sigma_a, float sigma_b, float huber, int pixel_border, float z_eps,
                     int first_iter, int max_iters, float rel_error, float delta_norm, void* status_out, void* workspace,
                     size_t workspace_bytes, void* stream);

/* The tensor expressions of FrameTracker.track around the pose loop (mast3r_slam/tracker.py:44-75: Qk, the validity
 * masks, match_frac; :147-177: the keyframe rule's two fractions and the keyframe's pointmap fused with the frame's view
 * of it, frame.py:41-105 'weighted_pointmap'; lietorch inv / mul / act at tracker.py:150,232) as three launches.  Each
 * value is produced by the same single IEEE operations, in the same order, as the op-by-op tensor form.
 * mslam_track_prepare: for keyframe pixel k with j = idx_f2k[k]:
 *   Qk[k] = sqrt(Qff[j] * Qkf[k]);  Cf = Cf_sum[j] * inv_nf;  Ck_avg[k] = Ck_sum[k] * inv_nk   (C / N of a Frame)
 *   valid_opt[k] = valid_match[k] & Cf > C_conf & Ck > C_conf & Qk > Q_conf;  valid_kf[k] = valid_match[k] & Qk > Q_conf
 *   T_rel = T_WCk^-1 * T_WCf (f32[8] each, unit quaternions as lietorch keeps them)
 *   workspace (16-byte aligned) <- per-block counts of valid_opt / valid_kf + one byte flag per frame pixel that some
 *   valid match points at (the verdict kernel counts them: the number of distinct idx_f2k[k] with valid_match[k]).
 * mslam_track_verdict: verdict6 <- {#valid_opt / n, iterations, chol_fail, #valid_kf / n, #distinct / n, done} with the
 *   solver status of mslam_track_pose (status_out) - the six scalars FrameTracker reads per frame.
 * mslam_track_fuse: T_WCf = T_WCk * T_rel;  X_new = ((C X_canon) + (Ckf (T_rel . Xkf))) / (C + Ckf);  C_new = C + Ckf. */
size_t mslam_track_prepare_workspace_bytes(int n_points);
int mslam_track_prepare(const int64_t* idx_f2k, const uint8_t* valid_match, const float* Qff, const float* Qkf,
                        const float* Cf_sum, float inv_nf, const float* Ck_sum, float inv_nk, float C_conf, float Q_conf,
                        int n_points, const float* T_WCk, const float* T_WCf, float* Qk, float* Ck_avg,
                        uint8_t* valid_opt, uint8_t* valid_kf, float* T_rel, void* workspace, size_t workspace_bytes,
                        void* stream);
int mslam_track_verdict(const void* prepare_workspace, const void* status, int n_points, float* verdict6, void* stream);
int mslam_track_fuse(const float* T_WCk, const float* T_rel, const float* Xkf, const float* Ckf, const float* X_canon,
                     const float* C, int n_points, float* T_WCf, float* X_new, float* C_new, void* stream);

/* ------------------------------------------------------------------------------------------
 * Building blocks of the MASt3R forward, exported for kernel-level parity tests and roofline
 * measurement (they have no counterpart in the reference's API: it calls cuBLAS/cuDNN through
 * torch, blocks.py:88-109, dpt_block.py:33-68).
 * ------------------------------------------------------------------------------------------ */
/* out[M,N] = act(A[M,K] . W[N,K]^T + bias) (+ residual f32[M,N]); A, W bf16; act 0 none, 1 GELU(erf),
 * 2 ReLU; out f32 or bf16.  K % 8 == 0. */
int mslam_gemm_bf16(const void* A, const void* W, const float* bias, const void* residual_f32, void* out,
                    int M, int N, int K, int act, int out_is_bf16, void* stream);
/* Tuning hook: force the tile configuration (codes in csrc/gemm.hip: 642 ... 2256; 0 = back to the built-in choice)
 * for every plain GEMM of exactly this shape (M < 0: the implicit-conv GEMM of shape |M| x N x K), process-wide.  tools/insitu_tune.py uses it to time whole network
 * stages under alternative tilings; results do not depend on the tiling (same K order per output element). */
int mslam_gemm_tile_override(int M, int N, int K, int cfg);
/* Measurement hook (bench.py `roofline`): between begin and end every launch of the plain GEMM of exactly this
 * shape - from any entry point, on any stream - is bracketed by two HIP events recorded on the stream it is
 * launched on (at most max_samples launches).  end() waits for the recorded events and returns the average and
 * minimum launch duration in microseconds (host doubles / int). */
int mslam_gemm_profile_begin(int M, int N, int K, int max_samples);
int mslam_gemm_profile_end(double* avg_us, double* min_us, int* samples);
/* NHWC bf16 conv (ks 1|3, stride 1|2, pad ks/2), W bf16 [Cout, ks*ks*Cin] tap-major; optional ReLU on
 * the input, act on the output, bf16 residual added after act. */
int mslam_conv2d_nhwc_bf16(const void* in, const void* W, const float* bias, const void* residual_bf16,
                           void* out_bf16, int B, int H, int Wd, int Cin, int Cout, int ks, int stride,
                           int relu_in, int act, void* stream);
/* O[B,Nq,H*64] = softmax(Q K^T) V ; Q,K bf16 [B,H,N,64] (Q pre-scaled by 1/8), VT bf16 [B,H,64,Nk]. */
int mslam_attention_bf16(const void* Q, const void* K, const void* VT, void* O, int batch, int heads,
                         int nq, int nk, void* stream);
/* The same product (Attention.forward / CrossAttention.forward, dust3r/croco/models/blocks.py:95-112,149-169) under a
 * forced work decomposition: `split` key splits x `qg` query groups of 32 rows per block, where mslam_attention_bf16
 * picks both from the shape.  For kernel tests and tools/attn_tune.py: the result depends on `split` only, every qg
 * gives the same bits.  A (split, qg) pair that the library does not hold returns MSLAM_EINVAL. */
int mslam_attention_bf16_cfg(const void* Q, const void* K, const void* VT, void* O, int batch, int heads,
                             int nq, int nk, int split, int qg, void* stream);
/* torch.nn.LayerNorm over the last dim (D <= 2048): x f32[rows,D] -> bf16 and/or f32 outputs. */
int mslam_layernorm_f32(const float* x, const float* w, const float* b, void* out_bf16, float* out_f32,
                        int rows, int D, float eps, void* stream);
/* The glue between those blocks.  Every entry below builds its launch with the very helper the forward uses (strides of
 * a grouped launch, choice between two forms of a kernel), so a test of the entry is a test of the forward's launch. */
/* HOST arrays cos, sin f32[len][16] <- cos / sin(p * 100^(-2i/32)), p < len, i < 16: the RoPE2D tables mslam_mast3r_create
 * uploads (len 1024). */
int mslam_rope_tables(float* cos_out, float* sin_out, int len);
/* Attention projection: x = A[M,K] . W^T + bias, W [n_sections*heads*64, K] holding sections sec_base ... (0 q, 1 k, 2 v).
 * q, k <- RoPE2D(x) (q also * q_scale) as bf16 [B,heads,ntok,64]; vt <- x transposed per head, bf16 [B,heads,64,kv_ntok];
 * token n of an image sits at (n / tok_w, n % tok_w); rows are whole images of ntok (q) / kv_ntok (k, v) tokens, both
 * divisible by 4.  W1 != NULL: a second problem (W1, bias1) on rows [M, 2M) of A, its outputs M*heads*64 elements behind
 * the first one's.  rope_cos / rope_sin: DEVICE copies of mslam_rope_tables(rope_len).  Outputs of sections the launch does
 * not hold are not touched (and may be NULL). */
int mslam_gemm_attn_bf16(const void* A, const void* W0, const float* bias0, const void* W1, const float* bias1, void* q,
                         void* k, void* vt, int M, int K, int n_sections, int sec_base, int heads, int ntok, int kv_ntok,
                         int tok_w, const float* rope_cos, const float* rope_sin, int rope_len, float q_scale,
                         void* stream);
/* Both sides of a decoder layer in one launch: out[s] = act(A[s] . Ws^T + bias_s) (+ residual[s]), s = 0, 1, with A, the
 * residual and out stacked as [2M, .].  out f32: optional f32 residual, which may be out itself (the residual stream);
 * out bf16: no residual. */
int mslam_gemm_grouped_bf16(const void* A, const void* W0, const float* bias0, const void* W1, const float* bias1,
                            const float* residual_f32, void* out, int M, int N, int K, int act, int out_is_bf16,
                            void* stream);
/* ConvTranspose2d with kernel == stride s on NHWC bf16: W bf16 [Cout*s*s, Cin] with row co*s*s + i*s + j, bias f32 [Cout];
 * out[b, y*s+i, x*s+j, co] bf16 [B, H*s, W*s, Cout].  Cin % 8 == 0. */
int mslam_conv_transpose_nhwc_bf16(const void* in, const void* W, const float* bias, void* out_bf16, int B, int H, int Wd,
                                   int Cin, int Cout, int s, void* stream);
/* mslam_conv2d_nhwc_bf16 with two optional bf16 residuals, both added after act (the residual unit of the DPT fusion
 * blocks: conv2(...) + x + the other path). */
int mslam_conv2d_res2_nhwc_bf16(const void* in, const void* W, const float* bias, const void* residual1_bf16,
                                const void* residual2_bf16, void* out_bf16, int B, int H, int Wd, int Cin, int Cout, int ks,
                                int stride, int relu_in, int act, void* stream);
/* LayerNorm of the two stacked decoder sides x f32 [2M, D], side s with its own affine pair: out_self[row] bf16 <-
 * self_s(x[row]).  With the mem pairs (all of mem0_w ... out_mem non-NULL; all NULL otherwise) also the norm_y each side
 * applies to the OTHER side's tokens: out_mem rows [0, M) <- mem0(x[M + r]), rows [M, 2M) <- mem1(x[r]). */
int mslam_layernorm_group_bf16(const float* x, const float* self0_w, const float* self0_b, const float* self1_w,
                               const float* self1_b, const float* mem0_w, const float* mem0_b, const float* mem1_w,
                               const float* mem1_b, void* out_self, void* out_mem, int M, int D, float eps, void* stream);
/* Bilinear x2, align_corners=True, NHWC bf16 [B,H,W,C] -> [B,2H,2W,C].  C % 8 == 0. */
int mslam_upsample2x_nhwc_bf16(const void* in, void* out, int B, int H, int Wd, int C, void* stream);
/* Tail of a head: l = w4[4,fc] . feat[pixel] + b4; X f32[B,H,W,3] <- l[0:3] * expm1(d)/d, d = |l[0:3]|; C <- 1 + exp(l[3]);
 * local features lf f32 [B*(H/P)*(W/P), lf_ld], channel c of pixel (y, x) at [token][c*P*P + (y%P)*P + x%P]:
 * D f32[B,H,W,desc_dim] <- unit vector of channels [0, desc_dim), Q <- exp(channel desc_dim).  feat bf16 [B,H,W,fc],
 * fc % 8 == 0, desc_dim <= 31, P divides H and W.  force_generic != 0: the per-pixel form also where the patch form
 * (P 16, fc 128, desc_dim 24) would run. */
int mslam_head_post(const void* feat_bf16, int fc, const float* w4, const float* b4, const float* lf, int lf_ld,
                    int desc_dim, int P, int B, int H, int Wd, float* X, float* C, float* D, float* Q, int force_generic,
                    void* stream);
/* img f32 [B,3,H,W] -> patches bf16 [B*(H/P)*(W/P), 3*P*P], column c*P*P + ky*P + kx (Conv2d weight order). */
int mslam_patchify_bf16(const float* img, void* patches_bf16, int B, int H, int Wd, int P, void* stream);
/* out bf16 [rows, ca+cb] <- cat(a [rows,ca], b [rows,cb]) along the columns. */
int mslam_concat2_bf16(const void* a, int ca, const void* b, int cb, void* out, long long rows, void* stream);
/* y bf16[n] <- x f32[n], round to nearest even. */
int mslam_cast_f32_bf16(const float* x, void* y_bf16, long long n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Local dense-block TSDF (camera-side half of the "dual TSDF"): replaces the python loops of
 * TSDFRefiner._build_tsdf_robust (mast3r_slam/tsdf_refine.py:837-940) and
 * _extract_surface_safe + _sample_tsdf_trilinear (:942-1064).  Grid layout [nz,ny,nx] f32, dims
 * (<= 64 per axis) computed by the caller as clamp(ceil(roi/voxel_size), max=max_grid_dim) (:844-846).
 * build: X_world f32[n,3] = T_WC.act(X_canon), C f32[n], origin/xyz_min/xyz_max f32[3] (device);
 * sequential float32 running-average semantics are preserved by per-voxel ordered replay.
 * raycast: sel_pix i64[n_sel] = pixel indices to march (the reference draws <= 100 with randperm);
 * surf f32[n_sel,3] <- surface point (or the original point), hit u8[n_sel].
 * ------------------------------------------------------------------------------------------ */
size_t mslam_tsdf_local_workspace_bytes(int n_points);
int mslam_tsdf_local_build(const float* X_world, const float* C, const float* origin, const float* xyz_min,
                           const float* xyz_max, int n_points, int nx, int ny, int nz, double voxel_size,
                           double trunc, float min_confidence, float* tsdf, float* weights, void* workspace,
                           size_t workspace_bytes, void* stream);
int mslam_tsdf_local_raycast(const float* tsdf, int nx, int ny, int nz, const float* xyz_min,
                             const float* xyz_max, const float* X_original, const int64_t* sel_pix, int n_sel,
                             int n_samples, float max_displacement, float* surf, uint8_t* hit, void* stream);

/* ------------------------------------------------------------------------------------------
 * Quality service patch statistics: replaces the torch reshape + nanmedian pipeline of
 * mast3r_slam/quality_core.py.  reduce_grid (:15-29) / u_from_CQ (:45-52) / r_from_scalar (:54-55) /
 * valid_grid (:57-59): one value per ps x ps patch of an h x w map, out f32[(h/ps)*(w/ps)].
 *   mode 0: nanmedian of x over valid pixels (valid u8[h*w] or NULL), empty patch -> 0
 *   mode 1: mean (valid NULL) / nanmean over valid pixels
 *   mode 2: median of U = 1 - sqrt(clamp(C/(c_thr+1e-8)) * clamp(Q/(q_thr+1e-8))), x = C, y = Q
 * classify (:66-117): robust z-scores of r and u over the n-patch grid, class ids int64[n], normalised priority f32[n].
 * ------------------------------------------------------------------------------------------ */
int mslam_quality_reduce_grid(const float* x, const float* y, const uint8_t* valid, int h, int w, int ps, int mode,
                              double c_thr, double q_thr, float* out, void* stream);
int mslam_quality_classify(const float* delta_cov, const float* r, const float* u, int n, float thr_zr, float thr_zu,
                           float thr_dc, int64_t* cls, float* pri, void* stream);

/* ------------------------------------------------------------------------------------------
 * Synthetic-data source (NOT a reference interface): the procedural box room of mast3r_slam/synthetic.py rendered
 * for `batch` view pairs in one kernel, in the layout of the MASt3R heads' outputs (X f32[b,h,w,3], C f32[b,h,w],
 * D f32[b,h,w,24], Q f32[b,h,w]; side 1 = view i in frame i, side 2 = view j in frame i).  ki / kj: device f32[batch]
 * camera-path indices; Wm (3x24) and phase (24): HOST doubles of the descriptor field.  Stands in for a trained
 * network's output in runs without a checkpoint (mast3r_slam/synthetic_gpu.py, bench.py).
 * ------------------------------------------------------------------------------------------ */
int mslam_room_pair(const float* ki, const float* kj, int batch, int h, int w, int n_frames, double fx, double fy,
                    double cx, double cy, double noise, const double* Wm_3x24, const double* phase_24, float* X1,
                    float* C1, float* D1, float* Q1, float* X2, float* C2, float* D2, float* Q2, void* stream);

/* cv2.remap(img, mapx, mapy, cv2.INTER_LINEAR) of the calibrated dataset readers (mast3r_slam/dataloader.py:495-496,
 * Intrinsics.remap) for 8-bit images: src u8[src_h, src_w, channels], maps f32[dst_h, dst_w] (position in src of every
 * dst pixel), dst u8[dst_h, dst_w, channels]; OpenCV's published fixed-point bilinear (1/32-pixel positions, 2^15
 * weights, constant border 0).  Parity with the library unpinned (OpenCV is absent): see csrc/undistort.hip. */
int mslam_remap_bilinear_u8(const uint8_t* src, int src_h, int src_w, int channels, const float* mapx,
                            const float* mapy, uint8_t* dst, int dst_h, int dst_w, void* stream);

/* fp64 GEMM of the retrieval head (Whitener.forward, thirdparty/mast3r/mast3r/retrieval/model.py:62-77; the projector's
 * Linear layers, model.py:108-151) on the f64 matrix cores:  out f64[M,N] = (A[M,K] - centre[K]) . B + bias[N].
 * A is f32 or f64 row-major [M,K]; B is f32 or f64, [K,N] row-major (b_transposed = 0) or [N,K] row-major
 * (b_transposed = 1: an nn.Linear weight); centre f64[K] and bias f64[N] may be NULL. */
int mslam_gemm_f64(const void* A, int a_is_f32, const void* B, int b_is_f32, int b_transposed, const double* centre,
                   const double* bias, double* out, int M, int N, int K, void* stream);

/* ------------------------------------------------------------------------------------------
 * Retrieval database: ASMK with binarised residuals.  Replaces, for one image at a time,
 *   ASMKKernel.aggregate_image + hamming.binarize_and_pack_2D   (thirdparty/mast3r/asmk/asmk/kernel.py:28-42,
 *                                                                asmk/cython/hamming.pyx:93-127)
 *   IVF.search + ASMKKernel.similarity + functional.asmk_kernel (asmk/inverted_file.py:90-114, kernel.py:59-71,
 *                                                                functional.py:10-15; use_idf False, processor.py:85)
 * as mast3r_slam/retrieval_database.py:107-166 calls them.
 *
 * mslam_asmk_aggregate: des f32[n_des, dim]; centroids f32[n_centroids, dim]; assign i64[n_des, m_assign] (the output
 *   of quantize_custom); uniq_words i64[n_uniq] = sorted unique values of `assign`; sig_out u32[n_uniq, dim/32]:
 *   bit (31 - d%32) of word d/32 = (sum of residuals of dimension d > 0).  dim must be a multiple of 32.
 * mslam_asmk_search: the inverted file as flat arrays in insertion order - entry_word i32[n_entries], entry_sig
 *   u32[n_entries, sig_words], img_start i32[n_images + 1] (entries of image i are [img_start[i], img_start[i+1]), words
 *   ascending) - queried with q_words i32[n_q] (sorted, unique) / q_sig u32[n_q, sig_words];
 *   scores f64[n_images] = sum over shared words of sim^alpha [sim >= threshold] / sqrt(entries of the image), over
 *   sqrt(n_q); sim = 1 - 2 hamming / (32 sig_words).  Signatures 16-byte aligned when sig_words % 4 == 0.
 * ------------------------------------------------------------------------------------------ */
int mslam_asmk_aggregate(const float* des, const float* centroids, const int64_t* assign, const int64_t* uniq_words,
                         uint32_t* sig_out, int n_des, int m_assign, int dim, int n_uniq, int n_centroids, void* stream);
int mslam_asmk_search(const int32_t* entry_word, const uint32_t* entry_sig, const int32_t* img_start, int n_images,
                      const int32_t* q_words, const uint32_t* q_sig, int n_q, int sig_words, float similarity_threshold,
                      float alpha, double* scores, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSLAM_HIP_H */
