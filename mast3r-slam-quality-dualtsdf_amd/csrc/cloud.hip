// Point clouds: a cloud index, the exact nearest neighbour of a point in a cloud, and the voxel downsample.  Semantics
// in DESIGN.md "Point clouds"; tests/cloud_numpy.py states the same definitions, operation by operation, in numpy.
// Everything is f64 on the f32 inputs in one fixed order and the build has -ffp-contract=off, so a * b + c below is two
// roundings, as in numpy.
//
// A point is VALID when its three coordinates are finite.  An invalid point is never anyone's nearest neighbour and is
// never fused into a voxel; a query with a non-finite coordinate has no neighbour (+inf, -1).
//
//   index     the caller sorts the Morton keys of the valid points (mslam_mesh_index_point_keys over the box of the valid
//             points, INT64_MAX for an invalid one) -> order i32[N]; md_build_index<MdPoint> of mesh_tri.h writes the f64
//             boxes of the tiles of 128 consecutive points IN `order` and of the groups of 32 tiles above them.  The
//             points are never copied or permuted.
//   distance  md_scan<MdPoint, .> of mesh_tri.h, the scan the mesh tools run over triangles: one query per thread, 256
//             per block, the tiles staged through LDS as f64, its skip test and its tie rule.  The invariant there holds
//             here in its simplest form: a point of a tile lies IN the tile's box exactly (f32 values in f64), so its
//             squared distance is at least the box's lb2 up to the roundings of the two sums, far inside the slack
//             (1 + 2^-20) and 2^-27 S^2 of the test.  A skipped tile therefore holds only points strictly farther than
//             a real point: neither the minimum nor a tie, and the output is that of the plain ascending scan, lowest
//             ORIGINAL index on ties, bit for bit.  A lane without a query idles through the tiles the block scans.
//   voxels    cd_voxel_key_kernel: world_to_key of tsdf_table.h per point.  The caller sorts the keys (stable), flags the
//             segment heads and lists them; cd_voxel_reduce_kernel then walks one voxel per thread in sorted order, which
//             within a voxel is original index order.  A voxel that holds a large share of the cloud serialises.
// No atomics, no waiting between blocks, every loop bounded by a tile or point count.
#include "cloud_point.h"
#include "tsdf_table.h"

namespace mslam {

// The nearest valid point of the cloud to each query.  A query with a non-finite coordinate is a lane without a point
// (`has` false) to md_scan.  kIndexed: the tiles follow `order`, they are culled by `box` and, when given, `gbox`, every
// lane takes its starting bound from the block's home tile, and ties go to the lowest original index; otherwise the
// plain ascending scan, where none of the three is read.
template <bool kIndexed>
__global__ __launch_bounds__(kMdBlock) void cd_distance_kernel(const float* __restrict__ queries, int n,
                                                               const float* __restrict__ points, int num_points,
                                                               const int32_t* __restrict__ order,
                                                               const double* __restrict__ box,
                                                               const double* __restrict__ gbox,
                                                               int32_t* __restrict__ skipped,
                                                               double* __restrict__ dist2,
                                                               int32_t* __restrict__ nearest) {
  __shared__ double s_pts[kMdTile * MdPoint::kDoubles];
  __shared__ int s_home;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const size_t i0 = (size_t)blockIdx.x * kMdBlock, i = i0 + tid;
  const bool in_range = i < (size_t)n;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  if (in_range) qx = queries[3 * i], qy = queries[3 * i + 1], qz = queries[3 * i + 2];
  const bool has = in_range && cd_finite(qx, qy, qz);
  const MdNearest r = md_scan<MdPoint, kIndexed>((double)qx, (double)qy, (double)qz, has, (double)queries[3 * i0],
                                                 (double)queries[3 * i0 + 1], (double)queries[3 * i0 + 2],
                                                 {points, num_points}, kIndexed, box, s_pts, &s_home, INFINITY, true,
                                                 order, gbox);
  if (in_range) {
    dist2[i] = has ? r.dist2 : INFINITY;
    nearest[i] = has ? r.face : -1;
  }
  if (skipped && lane == 0) skipped[4 * (size_t)blockIdx.x + wave] = r.skipped;
}

__global__ __launch_bounds__(256) void cd_voxel_key_kernel(const float* __restrict__ points, int n, float voxel_size,
                                                           int64_t* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
  uint64_t key = 0;
  keys[i] = cd_finite(x, y, z) && world_to_key(x, y, z, voxel_size, key) ? (int64_t)key : INT64_MAX;
}

// One voxel per thread: the members are the sorted slots from starts[v] while the key stays the same.  perm[slot] is the
// member's original index, range-checked before it is followed.
__global__ __launch_bounds__(256) void cd_voxel_reduce_kernel(const float* __restrict__ points,
                                                              const uint8_t* __restrict__ colors, int n,
                                                              const int64_t* __restrict__ sorted_keys,
                                                              const int64_t* __restrict__ perm,
                                                              const int64_t* __restrict__ starts, int num_voxels,
                                                              float* __restrict__ centroid, int32_t* __restrict__ count,
                                                              int32_t* __restrict__ first,
                                                              uint8_t* __restrict__ color) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= num_voxels) return;
  const int64_t s = starts[v];
  double sum[3] = {0.0, 0.0, 0.0};
  uint64_t csum[3] = {0, 0, 0};
  int cnt = 0, lowest = INT32_MAX;
  if (s >= 0 && s < (int64_t)n) {
    const int64_t key = sorted_keys[s];
    for (int64_t k = s; k < (int64_t)n && sorted_keys[k] == key; k++) {
      const int64_t j = perm[k];
      if ((uint64_t)j >= (uint64_t)n) continue;
#pragma unroll
      for (int d = 0; d < 3; d++) sum[d] += (double)points[3 * (size_t)j + d];
      if (colors) {
#pragma unroll
        for (int d = 0; d < 3; d++) csum[d] += colors[3 * (size_t)j + d];
      }
      cnt++;
      lowest = min(lowest, (int)j);
    }
  }
#pragma unroll
  for (int d = 0; d < 3; d++) centroid[3 * (size_t)v + d] = cnt ? (float)(sum[d] / (double)cnt) : 0.0f;
  count[v] = cnt;
  first[v] = cnt ? lowest : -1;
  if (color) {
#pragma unroll
    for (int d = 0; d < 3; d++)
      color[3 * (size_t)v + d] = cnt ? (uint8_t)((2 * csum[d] + (uint64_t)cnt) / (2 * (uint64_t)cnt)) : 0;
  }
}

}  // namespace mslam

using namespace mslam;

extern "C" size_t mslam_cloud_index_bytes(int num_points) { return num_points > 0 ? md_index_bytes(num_points) : 0; }

extern "C" int mslam_cloud_index_boxes(const float* points, int num_points, const int32_t* order, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  MSLAM_REQUIRE(num_points >= 0, "cloud_index_boxes: negative size");
  if (num_points == 0) return MSLAM_OK;
  MSLAM_REQUIRE(points && order && workspace, "cloud_index_boxes: null pointer");
  return md_build_index<MdPoint>({points, num_points}, order, workspace, workspace_bytes, "cloud_index_boxes",
                                 (hipStream_t)stream);
}

extern "C" int mslam_cloud_distance(const float* queries, int n, const float* points, int num_points,
                                    const int32_t* order, const void* index, size_t index_bytes, int levels,
                                    int32_t* skip_counts, double* dist2, int32_t* nearest, void* stream) {
  MSLAM_REQUIRE(n >= 0 && num_points >= 0, "cloud_distance: negative size");
  if (int rc = md_levels_arg("cloud_distance", levels)) return rc;
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(queries && dist2 && nearest, "cloud_distance: null pointer");
  MSLAM_REQUIRE(num_points == 0 || points, "cloud_distance: null pointer");
  MdIndexArg ix;
  if (int rc = md_index_arg("cloud_distance", num_points, order, index, index_bytes, levels, &ix)) return rc;
  hipLaunchKernelGGL(ix.order ? cd_distance_kernel<true> : cd_distance_kernel<false>, dim3(blocks_for(n, kMdBlock)),
                     dim3(kMdBlock), 0, (hipStream_t)stream, queries, n, points, num_points, ix.order, ix.box, ix.gbox,
                     skip_counts, dist2, nearest);
  MSLAM_LAUNCH_CHECK("cloud_distance");
  return MSLAM_OK;
}

extern "C" int mslam_cloud_voxel_keys(const float* points, int num_points, double voxel_size, int64_t* keys,
                                      void* stream) {
  MSLAM_REQUIRE(num_points >= 0, "cloud_voxel_keys: negative size");
  MSLAM_REQUIRE((float)voxel_size > 0.0f && (float)voxel_size < INFINITY,
                "cloud_voxel_keys: the voxel size must be positive and finite in float32");
  if (num_points == 0) return MSLAM_OK;
  MSLAM_REQUIRE(points && keys, "cloud_voxel_keys: null pointer");
  hipLaunchKernelGGL(cd_voxel_key_kernel, dim3(blocks_for(num_points, 256)), dim3(256), 0, (hipStream_t)stream, points,
                     num_points, (float)voxel_size, keys);
  MSLAM_LAUNCH_CHECK("cloud_voxel_keys");
  return MSLAM_OK;
}

extern "C" int mslam_cloud_voxel_reduce(const float* points, const uint8_t* colors, int num_points,
                                        const int64_t* sorted_keys, const int64_t* perm, const int64_t* starts,
                                        int num_voxels, float* centroid, int32_t* count, int32_t* first, uint8_t* color,
                                        void* stream) {
  MSLAM_REQUIRE(num_points >= 0 && num_voxels >= 0, "cloud_voxel_reduce: negative size");
  MSLAM_REQUIRE(num_voxels <= num_points, "cloud_voxel_reduce: more voxels than points");
  if (num_voxels == 0) return MSLAM_OK;
  MSLAM_REQUIRE(!colors == !color, "cloud_voxel_reduce: colors and color go together");
  MSLAM_REQUIRE(points && sorted_keys && perm && starts && centroid && count && first,
                "cloud_voxel_reduce: null pointer");
  hipLaunchKernelGGL(cd_voxel_reduce_kernel, dim3(blocks_for(num_voxels, 256)), dim3(256), 0, (hipStream_t)stream,
                     points, colors, num_points, sorted_keys, perm, starts, num_voxels, centroid, count, first, color);
  MSLAM_LAUNCH_CHECK("cloud_voxel_reduce");
  return MSLAM_OK;
}
