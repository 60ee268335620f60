// Mesh index: Morton-ordered tiles, so that the culled face scans of mesh_tri.h and mesh_raycast.hip prune whatever
// order the caller's faces are in.  Semantics in DESIGN.md "Mesh index"; tests/meshindex_numpy.py states the same
// definitions, operation by operation, in numpy.  Everything is f64 on the f32 inputs in one fixed order and the build
// has -ffp-contract=off.
//
//   keys     one thread per face: the 63-bit Morton code of its centroid ((a + b) + c) / 3, each axis quantised to 21
//            bits over the box of the mesh's vertices (`bounds`, formed by the caller); INT64_MAX for an invalid face
//            (md_load_tri's rule).  The same kernel, without faces, keys points: that is how queries are sorted.
//   (caller)   a stable sort of the keys -> order i32[F].  Stable: the index is the same bits on every build.
//   boxes    the f64 boxes of the tiles of 128 consecutive faces IN `order`, every entry of `order` range-checked before
//            it is followed, then the boxes of the groups of 32 tiles above them (md_build_index of mesh_tri.h).
// The faces are never copied or permuted: the scans stage tile t through order[128 t + k].  No atomics; nothing is
// written but the keys and the boxes.
#include "mesh_tri.h"

namespace mslam {

constexpr int kMiBits = 21;                            // per axis; tests/meshindex_numpy.py states it too

// bits 0..20 of x spread to every third bit
__device__ __forceinline__ uint64_t mi_spread(uint64_t x) {
  x &= 0x1fffffull;
  x = (x | (x << 32)) & 0x1f00000000ffffull;
  x = (x | (x << 16)) & 0x1f0000ff0000ffull;
  x = (x | (x << 8)) & 0x100f00f00f00f00full;
  x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
  x = (x | (x << 2)) & 0x1249249249249249ull;
  return x;
}

// The Morton code of the point c in the box bounds = lo.xyz, hi.xyz: per axis floor((c - lo) / (hi - lo) * 2^21) clamped
// to [0, 2^21) with fmax / fmin, so a NaN (a flat axis, a non-finite coordinate) is cell 0; x highest.
__device__ __forceinline__ int64_t mi_morton(const double* c, const float* __restrict__ bounds) {
  uint64_t key = 0;
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const double lo = (double)bounds[d], hi = (double)bounds[3 + d];
    const double u = (c[d] - lo) / (hi - lo) * (double)(1 << kMiBits);
    const double q = fmin(fmax(floor(u), 0.0), (double)((1 << kMiBits) - 1));
    key |= mi_spread((uint64_t)q) << (2 - d);
  }
  return (int64_t)key;
}

__global__ __launch_bounds__(256) void mi_keys_kernel(const float* __restrict__ vert, int nv,
                                                      const int32_t* __restrict__ faces, int nf,
                                                      const float* __restrict__ bounds, int64_t* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= (faces ? nf : nv)) return;
  double c[3];
  if (faces) {
    double t[kMdTriDoubles];
    if (!md_load_tri(vert, faces, i, nf, nv, t)) {
      keys[i] = INT64_MAX;
      return;
    }
#pragma unroll
    for (int d = 0; d < 3; d++) c[d] = ((t[d] + t[3 + d]) + t[6 + d]) / 3.0;
  } else {
#pragma unroll
    for (int d = 0; d < 3; d++) c[d] = (double)vert[3 * (size_t)i + d];
  }
  keys[i] = mi_morton(c, bounds);
}

}  // namespace mslam

using namespace mslam;

extern "C" size_t mslam_mesh_index_bytes(int num_faces) { return num_faces > 0 ? md_index_bytes(num_faces) : 0; }

extern "C" int mslam_mesh_index_keys(const float* vertices, int num_vertices, const int32_t* faces, int num_faces,
                                     const float* bounds, int64_t* keys, void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_index_keys: negative size");
  if (num_faces == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && keys && bounds && (vertices || num_vertices == 0), "mesh_index_keys: null pointer");
  hipLaunchKernelGGL(mi_keys_kernel, dim3(blocks_for(num_faces, 256)), dim3(256), 0, (hipStream_t)stream, vertices,
                     num_vertices, faces, num_faces, bounds, keys);
  MSLAM_LAUNCH_CHECK("mesh_index_keys");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_index_point_keys(const float* points, int n, const float* bounds, int64_t* keys,
                                           void* stream) {
  MSLAM_REQUIRE(n >= 0, "mesh_index_point_keys: negative size");
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(points && keys && bounds, "mesh_index_point_keys: null pointer");
  hipLaunchKernelGGL(mi_keys_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, points, n,
                     (const int32_t*)nullptr, 0, bounds, keys);
  MSLAM_LAUNCH_CHECK("mesh_index_point_keys");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_index_boxes(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                                      const int32_t* order, void* workspace, size_t workspace_bytes, void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_index_boxes: negative size");
  if (num_faces == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && order && workspace && (vertices || num_vertices == 0), "mesh_index_boxes: null pointer");
  return md_build_index<MdTri>({vertices, faces, num_faces, num_vertices}, order, workspace, workspace_bytes,
                               "mesh_index_boxes", (hipStream_t)stream);
}
