// What a point cloud is to the scans of mesh_tri.h: the validity rule and the tile trait MdPoint, shared by cloud.hip
// (index, nearest neighbour, voxels) and cloud_knn.hip (k nearest neighbours, normals).
#pragma once
#include "mesh_tri.h"

namespace mslam {

__device__ __forceinline__ bool cd_finite(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// What a tile of a cloud holds (the trait md_scan, md_box_kernel and md_build_index of mesh_tri.h ask for): a slot is
// x, y, z and the tag, 0 for an invalid point, else 1 + the original index (exact in a double).
struct MdPoint {
  struct Src {
    const float* points;
    int n;
  };
  static constexpr int kDoubles = 4;
  static __host__ __device__ __forceinline__ int count(const Src s) { return s.n; }
  // Point j as p[0..2] f64 and p[3] = 1 + j; all zeros for j >= n or an invalid point
  static __device__ __forceinline__ bool load(const Src s, int j, double* p) {
    p[0] = p[1] = p[2] = p[3] = 0.0;
    if (j >= s.n) return false;
    const float x = s.points[3 * (size_t)j], y = s.points[3 * (size_t)j + 1], z = s.points[3 * (size_t)j + 2];
    if (!cd_finite(x, y, z)) return false;
    p[0] = (double)x, p[1] = (double)y, p[2] = (double)z, p[3] = (double)j + 1.0;
    return true;
  }
  static __device__ __forceinline__ double dist2(double px, double py, double pz, const double* q) {
    const double dx = px - q[0], dy = py - q[1], dz = pz - q[2];
    return md_dot(dx, dy, dz, dx, dy, dz);
  }
};

}  // namespace mslam
