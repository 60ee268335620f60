// Point clouds: how many points lie within a radius of a point, and the density clusters (DBSCAN) of a cloud.
// Semantics in DESIGN.md "Cloud clusters"; tests/cloud_cluster_numpy.py states the same definitions in numpy.  The
// distance is f64 on the f32 inputs in one fixed order and the build has -ffp-contract=off.
//
// THE DEFINITION.  d2(i, j) is MdPoint::dist2, the sum cloud_distance uses: (dx dx + dy dy) + dz dz of the f64
// differences.  A difference and its negation have the same square, so d2(i, j) and d2(j, i) are the same bits.
// "Within" is d2 <= eps2, eps2 an f64 the caller hands over as it is.
//   count   count[q] = the valid points of the cloud within eps2 of query q; 0 for a query with a non-finite
//           coordinate.  For the cloud in itself a point counts itself and its duplicates.  Not capped.
//   core    (the caller's) core[i] = valid[i] && count[i] >= min_points.
//   link    a cluster is a connected component of the graph on the core points with an edge where d2 <= eps2; its
//           root is its smallest point index.  Row q stands for point self[q].  A core row i unites (i, j) for every
//           core j < i within eps2 - the pair with j > i is row j's, by the symmetry of d2 - in the union-find
//           `parent` of union_find.h.  A non-core row unites nothing, so a path through a non-core point joins
//           nothing, and keeps its anchor: the core point smallest under the total order (d2, index) among those
//           within eps2.  anchor / anchor_dist2 of a row: (its own index, 0) for a core row, (the anchor, its d2) for
//           a border row, (-1, +inf) for noise, for an invalid point and for an entry of `self` outside [0, N).
//   finish  flatten: parent[v] = find(v) in a launch of its own, then labels: label_root[i] = root[anchor[i]] or -1,
//           is_cluster_root[v] = core[v] && root[v] == v.  The ranking of the roots and the sizes are the caller's
//           integer work (torch.cumsum, one host read); no output offset comes from a counter at one address.
//
// WHY THE CONSTANT BOUND IS EXACT.  Both walks are md_walk<MdPoint, kIndexed> of mesh_tri.h with a policy whose
// bound() is the constant eps2, so the skip test reads  lb2 > eps2 (1 + 2^-20) + 2^-27 S^2 .  By the invariant at the
// head of mesh_tri.h a point of a tile lies in the tile's box exactly (f32 values in f64), so its d2 to the lane's
// point is at least the box's lb2 up to the roundings of the two sums, which the factor and the S^2 term cover many
// times over: every point of a skipped tile (or group, whose box holds its tiles' boxes) has d2 > eps2 strictly.  It
// is then neither counted, nor united with, nor an anchor candidate - and unlike the k-th best of cloud_knn.hip the
// bound never moves, so what is skipped does not depend on the order of the visit either.  A lane without a valid
// point takes the bound -inf in its policy: nothing is within it, and md_walk never lets such a lane keep a tile in.
// Hence the same bytes in the three forms (order NULL: the plain scan; tiles; tiles and groups).
//
// THE UNION-FIND is cc_find / cc_unite of union_find.h, shared with mesh_components.hip, whose head has the invariant
// parent[v] <= v and what follows from it: every find descends, every unite retries onto a smaller pair, nothing
// spins or waits, and when the link launch has ended every tree's root is its component's smallest index whatever
// order the atomics landed in.  `parent` is touched only through the atomics; `core` was written by an earlier launch
// and is read plainly.  The unite loops are divergent and sit inside md_offer_tile's loop over the slots of a staged
// tile, whose trip count and LDS addresses are wave-uniform: a lane that unites holds the others of its wave at that
// iteration's end, where they reconverge, and md_offer_tile uses no cross-lane operation; the walk's next
// __syncthreads_and comes after the whole loop.  No lane waits for another INSIDE the loop, so no wave can hold a
// barrier up for ever.
//
// THE CACHED ROOT.  A core lane keeps `root`, a value cc_find(self) returned at some time, and skips the unite when
// cc_find(j) is that very index: both points then hang below it, connections are never undone, so the pair is united
// already.  It is refreshed after each unite.  In a dense neighbourhood nearly every pair after the first is of that
// kind, and the skip saves the second find and the compare.  Measured against a build that unites every pair: 20 ms
// against 52 ms for the link of a 2 M-point cloud with 600 neighbours per point (DESIGN.md "Cloud clusters").
#include "cloud_point.h"
#include "union_find.h"

namespace mslam {

// What a lane of the count keeps (the policy md_walk asks for): eps2 (-inf for a lane without a query) and the count
struct ClCount {
  double eps2;
  int count;
  __device__ __forceinline__ double bound() const { return eps2; }
  template <bool kIndexed>
  __device__ __forceinline__ void offer(double d, double, int) {
    count += d <= eps2 ? 1 : 0;
  }
};

// What a lane of the link keeps: its point `self`, whether that is a core point, the cached root (core) or the best
// anchor so far (not core)
struct ClLink {
  double eps2;
  const uint8_t* __restrict__ core;
  int32_t* parent;
  int self, root;
  bool is_core;
  double best;
  int best_j;
  __device__ __forceinline__ double bound() const { return eps2; }
  template <bool kIndexed>
  __device__ __forceinline__ void offer(double d, double tag, int) {
    if (!(d <= eps2)) return;
    const int j = (int)tag - 1;                      // MdPoint::load tags a valid slot with 1 + its index, j in [0, N)
    if (!core[j]) return;
    if (is_core) {
      if (j < self) {
        if (cc_find(parent, j) != root) {          // else: united already (THE CACHED ROOT)
          cc_unite(parent, self, j);
          root = cc_find(parent, self);
        }
      }
    } else if (d < best || (d == best && j < best_j)) {
      best = d, best_j = j;
    }
  }
};

template <bool kIndexed>
__global__ __launch_bounds__(kMdBlock) void cl_count_kernel(const float* __restrict__ queries, int n,
                                                            const float* __restrict__ points, int num_points,
                                                            double eps2, const int32_t* __restrict__ order,
                                                            const double* __restrict__ box,
                                                            const double* __restrict__ gbox,
                                                            int32_t* __restrict__ skipped,
                                                            int32_t* __restrict__ count) {
  __shared__ double s_pts[kMdTile * MdPoint::kDoubles];
  const int tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * kMdBlock + tid;
  const bool in_range = i < (size_t)n;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  if (in_range) qx = queries[3 * i], qy = queries[3 * i + 1], qz = queries[3 * i + 2];
  const bool has = in_range && cd_finite(qx, qy, qz);
  const MdPoint::Src src = {points, num_points};
  const int ntiles = (num_points + kMdTile - 1) / kMdTile;
  ClCount acc = {has ? eps2 : -INFINITY, 0};
  const int n_skipped = md_walk<MdPoint, kIndexed>((double)qx, (double)qy, (double)qz, has, src, kIndexed, box, gbox,
                                                   order, s_pts, ntiles, -1, acc);
  if (in_range) count[i] = acc.count;
  if (skipped && (tid & (kWave - 1)) == 0) skipped[4 * (size_t)blockIdx.x + tid / kWave] = n_skipped;
}

template <bool kIndexed>
__global__ __launch_bounds__(kMdBlock) void cl_link_kernel(const float* __restrict__ points, int num_points,
                                                           const int32_t* __restrict__ self, int n, double eps2,
                                                           const uint8_t* __restrict__ core,
                                                           const int32_t* __restrict__ order,
                                                           const double* __restrict__ box,
                                                           const double* __restrict__ gbox,
                                                           int32_t* __restrict__ skipped, int32_t* parent,
                                                           int32_t* __restrict__ anchor,
                                                           double* __restrict__ anchor_dist2) {
  __shared__ double s_pts[kMdTile * MdPoint::kDoubles];
  const int tid = threadIdx.x;
  const size_t row = (size_t)blockIdx.x * kMdBlock + tid;
  const bool in_range = row < (size_t)n;
  int v = -1;
  if (in_range) {
    v = self ? self[row] : (int)row;
    if ((unsigned)v >= (unsigned)num_points) v = -1;           // skipped, never followed
  }
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  if (v >= 0) qx = points[3 * (size_t)v], qy = points[3 * (size_t)v + 1], qz = points[3 * (size_t)v + 2];
  const bool has = v >= 0 && cd_finite(qx, qy, qz);
  const bool is_core = has && core[v] != 0;
  const MdPoint::Src src = {points, num_points};
  const int ntiles = (num_points + kMdTile - 1) / kMdTile;
  ClLink acc = {has ? eps2 : -INFINITY, core, parent, v, v, is_core, INFINITY, -1};
  const int n_skipped = md_walk<MdPoint, kIndexed>((double)qx, (double)qy, (double)qz, has, src, kIndexed, box, gbox,
                                                   order, s_pts, ntiles, -1, acc);
  if (in_range) {
    anchor[row] = is_core ? v : (has ? acc.best_j : -1);
    anchor_dist2[row] = is_core ? 0.0 : (has ? acc.best : INFINITY);
  }
  if (skipped && (tid & (kWave - 1)) == 0) skipped[4 * (size_t)blockIdx.x + tid / kWave] = n_skipped;
}

__global__ __launch_bounds__(256) void cl_init_kernel(int n, int32_t* __restrict__ parent) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v < n) parent[v] = v;
}

__global__ __launch_bounds__(256) void cl_flatten_kernel(int n, int32_t* parent) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  __hip_atomic_store(parent + v, cc_find(parent, v), CC_RELAXED);
}

__global__ __launch_bounds__(256) void cl_labels_kernel(const int32_t* __restrict__ root,
                                                        const uint8_t* __restrict__ core,
                                                        const int32_t* __restrict__ anchor, int n,
                                                        int32_t* __restrict__ label_root,
                                                        uint8_t* __restrict__ is_cluster_root) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int a = anchor[i];
  label_root[i] = (unsigned)a < (unsigned)n ? root[a] : -1;
  is_cluster_root[i] = core[i] && root[i] == i ? 1 : 0;
}

}  // namespace mslam

using namespace mslam;

extern "C" int mslam_cloud_radius_count(const float* queries, int n, const float* points, int num_points, double eps2,
                                        const int32_t* order, const void* index, size_t index_bytes, int levels,
                                        int32_t* skip_counts, int32_t* count, void* stream) {
  MSLAM_REQUIRE(n >= 0 && num_points >= 0, "cloud_radius_count: negative size");
  MSLAM_REQUIRE(eps2 >= 0.0, "cloud_radius_count: eps2 must be >= 0, got %g", eps2);
  MdIndexArg ix;
  if (int rc = md_index_arg("cloud_radius_count", num_points, order, index, index_bytes, levels, &ix)) return rc;
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(queries && count, "cloud_radius_count: null pointer");
  MSLAM_REQUIRE(num_points == 0 || points, "cloud_radius_count: null pointer");
  const auto kernel = ix.order ? cl_count_kernel<true> : cl_count_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(blocks_for(n, kMdBlock)), dim3(kMdBlock), 0, (hipStream_t)stream, queries, n, points,
                     num_points, eps2, ix.order, ix.box, ix.gbox, skip_counts, count);
  MSLAM_LAUNCH_CHECK("cloud_radius_count");
  return MSLAM_OK;
}

extern "C" int mslam_cloud_cluster_init(int num_points, int32_t* parent, void* stream) {
  MSLAM_REQUIRE(num_points >= 0, "cloud_cluster_init: negative size");
  if (num_points == 0) return MSLAM_OK;
  MSLAM_REQUIRE(parent, "cloud_cluster_init: null pointer");
  hipLaunchKernelGGL(cl_init_kernel, dim3(blocks_for(num_points, 256)), dim3(256), 0, (hipStream_t)stream, num_points,
                     parent);
  MSLAM_LAUNCH_CHECK("cloud_cluster_init");
  return MSLAM_OK;
}

extern "C" int mslam_cloud_cluster_link(const float* points, int num_points, const int32_t* self, int n, double eps2,
                                        const uint8_t* core, const int32_t* order, const void* index,
                                        size_t index_bytes, int levels, int32_t* skip_counts, int32_t* parent,
                                        int32_t* anchor, double* anchor_dist2, void* stream) {
  MSLAM_REQUIRE(n >= 0 && num_points >= 0, "cloud_cluster_link: negative size");
  MSLAM_REQUIRE(eps2 >= 0.0, "cloud_cluster_link: eps2 must be >= 0, got %g", eps2);
  MdIndexArg ix;
  if (int rc = md_index_arg("cloud_cluster_link", num_points, order, index, index_bytes, levels, &ix)) return rc;
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(anchor && anchor_dist2, "cloud_cluster_link: null pointer");
  MSLAM_REQUIRE(num_points == 0 || (points && core && parent), "cloud_cluster_link: null pointer");
  const auto kernel = ix.order ? cl_link_kernel<true> : cl_link_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(blocks_for(n, kMdBlock)), dim3(kMdBlock), 0, (hipStream_t)stream, points, num_points,
                     self, n, eps2, core, ix.order, ix.box, ix.gbox, skip_counts, parent, anchor, anchor_dist2);
  MSLAM_LAUNCH_CHECK("cloud_cluster_link");
  return MSLAM_OK;
}

extern "C" int mslam_cloud_cluster_flatten(int num_points, int32_t* parent, void* stream) {
  MSLAM_REQUIRE(num_points >= 0, "cloud_cluster_flatten: negative size");
  if (num_points == 0) return MSLAM_OK;
  MSLAM_REQUIRE(parent, "cloud_cluster_flatten: null pointer");
  hipLaunchKernelGGL(cl_flatten_kernel, dim3(blocks_for(num_points, 256)), dim3(256), 0, (hipStream_t)stream,
                     num_points, parent);
  MSLAM_LAUNCH_CHECK("cloud_cluster_flatten");
  return MSLAM_OK;
}

extern "C" int mslam_cloud_cluster_labels(const int32_t* root, const uint8_t* core, const int32_t* anchor,
                                          int num_points, int32_t* label_root, uint8_t* is_cluster_root,
                                          void* stream) {
  MSLAM_REQUIRE(num_points >= 0, "cloud_cluster_labels: negative size");
  if (num_points == 0) return MSLAM_OK;
  MSLAM_REQUIRE(root && core && anchor && label_root && is_cluster_root, "cloud_cluster_labels: null pointer");
  hipLaunchKernelGGL(cl_labels_kernel, dim3(blocks_for(num_points, 256)), dim3(256), 0, (hipStream_t)stream, root,
                     core, anchor, num_points, label_root, is_cluster_root);
  MSLAM_LAUNCH_CHECK("cloud_cluster_labels");
  return MSLAM_OK;
}
