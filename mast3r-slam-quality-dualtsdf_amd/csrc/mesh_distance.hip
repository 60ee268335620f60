// Mesh quality: face areas, an area-weighted stratified surface sampler and the exact point-to-triangle-mesh distance.
// Semantics in DESIGN.md "Mesh quality"; tests/meshdist_numpy.py states the same definitions, operation by operation,
// in numpy.  Everything is f64 on the f32 inputs and the build has -ffp-contract=off, so a * b + c below is two
// roundings, as in numpy.
//
// A face is VALID when its three indices lie in [0, V) and the cross product (b - a) x (c - a) is not exactly zero.
// An invalid face has area 0, is never sampled and is never the nearest face.
//
// The distance is md_scan of mesh_tri.h, the culled nearest-face scan that mesh_align.hip calls too; the invariant that
// makes its culling exact is in that header.  Here every lane starts without a bound and takes one from the block's
// home tile.  mslam_mesh_distance_indexed is the same scan over the tiles of a mesh index (mesh_index.hip).
#include "mesh_tri.h"

namespace mslam {

__global__ __launch_bounds__(256) void md_area_kernel(const float* __restrict__ vert,
                                                      const int32_t* __restrict__ faces, int nf, int nv,
                                                      double* __restrict__ area) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  double t[kMdTriDoubles], n2;
  md_load_tri(vert, faces, f, nf, nv, t, &n2);
  area[f] = 0.5 * sqrt(n2);
}

// splitmix64 of seed + (i + 1) * golden ratio: stateless, the same bits on every call
__device__ __forceinline__ uint64_t md_hash(uint64_t seed, uint64_t i) {
  uint64_t z = seed + (i + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void md_sample_kernel(const float* __restrict__ vert,
                                                        const int32_t* __restrict__ faces, int nf, int nv,
                                                        const double* __restrict__ cdf, double total, int n,
                                                        uint64_t seed, float* __restrict__ points,
                                                        int32_t* __restrict__ face) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double u = ((double)i + 0.5) / (double)n * total;
  int lo = 0, hi = nf;                        // first face with cdf[f] > u
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (cdf[mid] > u) hi = mid; else lo = mid + 1;
  }
  int f = lo < nf - 1 ? lo : nf - 1;
  double t[kMdTriDoubles];
  while (!md_load_tri(vert, faces, f, nf, nv, t) && f > 0) f--;     // back to the last face with an area
  const uint64_t z = md_hash(seed, (uint64_t)i);
  double r1 = (double)(z >> 40) * 0x1p-24, r2 = (double)((z >> 16) & 0xFFFFFFull) * 0x1p-24;
  if (r1 + r2 > 1.0) {
    r1 = 1.0 - r1;
    r2 = 1.0 - r2;
  }
#pragma unroll
  for (int d = 0; d < 3; d++)
    points[3 * (size_t)i + d] = (float)((t[d] + r1 * (t[3 + d] - t[d])) + r2 * (t[6 + d] - t[d]));
  face[i] = f;
}

// skipped, when given: per wave, how many tiles the culled scan did not scan -> skipped[4 * block + wave] (the timing
// tool's figure; each wave owns its word).  kIndexed: the tiles follow `order`, `gbox` (may be null) holds the group
// boxes (mesh_tri.h); without it neither is read.
template <bool kIndexed>
__global__ __launch_bounds__(kMdBlock) void md_distance_kernel(const float* __restrict__ points, int n,
                                                               const float* __restrict__ vert,
                                                               const int32_t* __restrict__ faces, int nf, int nv,
                                                               int cull, const double* __restrict__ box,
                                                               const int32_t* __restrict__ order,
                                                               const double* __restrict__ gbox,
                                                               int32_t* __restrict__ skipped,
                                                               double* __restrict__ dist2,
                                                               int32_t* __restrict__ nearest) {
  __shared__ double s_tri[kMdTile * kMdTriDoubles];
  __shared__ int s_home;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const size_t i0 = (size_t)blockIdx.x * kMdBlock, i = i0 + tid;
  const bool has = i < (size_t)n;
  double px = 0.0, py = 0.0, pz = 0.0;
  if (has) px = (double)points[3 * i], py = (double)points[3 * i + 1], pz = (double)points[3 * i + 2];
  const MdNearest r =
      md_scan<MdTri, kIndexed>(px, py, pz, has, (double)points[3 * i0], (double)points[3 * i0 + 1],
                               (double)points[3 * i0 + 2], {vert, faces, nf, nv}, cull, box, s_tri, &s_home, INFINITY, true,
                               order, gbox);
  if (has) {
    dist2[i] = r.dist2;
    nearest[i] = r.face;
  }
  if (skipped && lane == 0) skipped[4 * (size_t)blockIdx.x + wave] = r.skipped;
}

}  // namespace mslam

using namespace mslam;

extern "C" int mslam_mesh_face_areas(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                                     double* area, void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_face_areas: negative size");
  if (num_faces == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && area && (vertices || num_vertices == 0), "mesh_face_areas: null pointer");
  hipLaunchKernelGGL(md_area_kernel, dim3(blocks_for(num_faces, 256)), dim3(256), 0, (hipStream_t)stream, vertices,
                     faces, num_faces, num_vertices, area);
  MSLAM_LAUNCH_CHECK("mesh_face_areas");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_sample(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                                 const double* cdf, double total, int n, uint64_t seed, float* points, int32_t* face,
                                 void* stream) {
  MSLAM_REQUIRE(num_faces > 0 && num_vertices > 0 && n >= 0, "mesh_sample: bad size");
  MSLAM_REQUIRE(total > 0.0 && total < INFINITY, "mesh_sample: the total area must be positive and finite");
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(vertices && faces && cdf && points && face, "mesh_sample: null pointer");
  hipLaunchKernelGGL(md_sample_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, vertices, faces,
                     num_faces, num_vertices, cdf, total, n, seed, points, face);
  MSLAM_LAUNCH_CHECK("mesh_sample");
  return MSLAM_OK;
}

extern "C" size_t mslam_mesh_distance_workspace_bytes(int num_faces) {
  return num_faces > 0 ? md_box_bytes(num_faces) : 0;
}

// Both distance queries after their argument checks.  Plain: `skip` 1 or 2 builds the boxes at the head of the
// workspace and culls by them, 2 also counts behind them.  `indexed`: the tiles follow `order`, the boxes are the
// index's, its groups are used at `levels` 2, and `skip_counts` (may be null) receives the per-wave counts.
static int md_distance_impl(const char* what, bool indexed, const float* points, int n, const float* vertices,
                            const int32_t* faces, int num_faces, int num_vertices, int skip, void* workspace,
                            size_t workspace_bytes, const int32_t* order, const void* index, size_t index_bytes,
                            int levels, int32_t* skip_counts, double* dist2, int32_t* nearest, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int cull = num_faces > 0 && (indexed || skip);
  MdIndexArg ix = {nullptr, (const double*)workspace, nullptr};
  if (indexed) {
    if (int rc = md_index_arg(what, num_faces, order, index, index_bytes, levels, &ix)) return rc;
  } else if (cull) {
    const size_t box_bytes = md_box_bytes(num_faces), count_bytes = skip == 2 ? md_count_bytes(n) : 0;
    if (workspace_bytes < box_bytes + count_bytes)
      return md_too_small(what, "workspace", workspace_bytes, box_bytes + count_bytes);
    md_launch_boxes<MdTri>({vertices, faces, num_faces, num_vertices}, nullptr, (double*)workspace, s);
    if (count_bytes) skip_counts = (int32_t*)((char*)workspace + box_bytes);
    if (num_faces <= kMdTile) {                  // one tile: it is scanned whatever its box says, so scan it once
      if (count_bytes) {
        int rc = check_hip(hipMemsetAsync(skip_counts, 0, count_bytes, s), "mesh_distance memset");
        if (rc) return rc;
      }
      cull = 0, skip_counts = nullptr;
    }
  }
  hipLaunchKernelGGL(indexed ? md_distance_kernel<true> : md_distance_kernel<false>, dim3(blocks_for(n, kMdBlock)),
                     dim3(kMdBlock), 0, s, points, n, vertices, faces, num_faces, num_vertices, cull, ix.box, ix.order,
                     ix.gbox, skip_counts, dist2, nearest);
  return md_launched(what);
}

extern "C" int mslam_mesh_distance(const float* points, int n, const float* vertices, const int32_t* faces,
                                   int num_faces, int num_vertices, int skip, void* workspace, size_t workspace_bytes,
                                   double* dist2, int32_t* nearest, void* stream) {
  MSLAM_REQUIRE(n >= 0 && num_faces >= 0 && num_vertices >= 0, "mesh_distance: negative size");
  MSLAM_REQUIRE(skip >= 0 && skip <= 2, "mesh_distance: skip must be 0, 1 or 2");
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(points && dist2 && nearest, "mesh_distance: null pointer");
  MSLAM_REQUIRE(num_faces == 0 || (faces && (vertices || num_vertices == 0)), "mesh_distance: null pointer");
  MSLAM_REQUIRE(!skip || num_faces == 0 || workspace, "mesh_distance: the culled scan needs a workspace");
  return md_distance_impl("mesh_distance", false, points, n, vertices, faces, num_faces, num_vertices, skip,
                          workspace, workspace_bytes, nullptr, nullptr, 0, 0, nullptr, dist2, nearest, stream);
}

extern "C" int mslam_mesh_distance_indexed(const float* points, int n, const float* vertices, const int32_t* faces,
                                           int num_faces, int num_vertices, const int32_t* order, const void* index,
                                           size_t index_bytes, int levels, int32_t* skip_counts, double* dist2,
                                           int32_t* nearest, void* stream) {
  MSLAM_REQUIRE(n >= 0 && num_faces >= 0 && num_vertices >= 0, "mesh_distance_indexed: negative size");
  if (int rc = md_levels_arg("mesh_distance_indexed", levels)) return rc;
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(points && dist2 && nearest, "mesh_distance_indexed: null pointer");
  MSLAM_REQUIRE(num_faces == 0 || (faces && order && index && (vertices || num_vertices == 0)),
                "mesh_distance_indexed: null pointer");
  return md_distance_impl("mesh_distance_indexed", true, points, n, vertices, faces, num_faces, num_vertices, 0,
                          nullptr, 0, order, index, index_bytes, levels, skip_counts, dist2, nearest, stream);
}
