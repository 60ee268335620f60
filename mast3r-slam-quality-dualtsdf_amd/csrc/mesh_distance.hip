// Mesh quality: face areas, an area-weighted stratified surface sampler and the exact point-to-triangle-mesh distance.
// Semantics in DESIGN.md "Mesh quality"; tests/meshdist_numpy.py states the same definitions, operation by operation,
// in numpy.  Everything is f64 on the f32 inputs and the build has -ffp-contract=off, so a * b + c below is two
// roundings, as in numpy.
//
// A face is VALID when its three indices lie in [0, V) and the cross product (b - a) x (c - a) is not exactly zero.
// An invalid face has area 0, is never sampled and is never the nearest face.
//
// THE INVARIANT that makes culling exact.  md_dist2(p, f) is |p - q|^2 for a computed point q of face f: a vertex
// itself, a + v (b - a) with a computed 0 <= v <= 1 (both ends of an edge region's division are ordered, and rounding
// is monotone), or a point of the face's plane.  A tile's box holds every vertex of its valid faces exactly (f32
// values in f64), so it holds each face, and q lies within eps of the box, eps a small multiple of the rounding unit
// times the largest coordinate S in play: |p - q| >= lb - eps, where lb is the distance from p to the box.  In the
// interior region an in-plane error of q adds to the distance from the plane, and a foot point wrongly taken for
// interior lies outside the face by no more than the same in-plane error.  The scan keeps
// best = min over scanned faces, and with culling also ub = min over the faces of one tile scanned first (any tile:
// ub is the value of a real face, so the final minimum is <= ub).  A tile is skipped only when, for every point of
// the wave (scan) or block (staging),
//     lb2 > min(best, ub) * (1 + 2^-20) + 2^-27 * S^2 .
// lb2 itself carries 4 roundings (relative 2^-51, inside the 2^-20), and 2^-27 S^2 >= 2 lb eps for eps = 2^-30 S, a
// closest-point error four million times the rounding unit: the slack is there for sliver triangles, and it costs
// nothing, because a tile worth skipping is centimetres away and 2^-27 S^2 is (1e-4 S)^2.  So every face of a skipped
// tile has md_dist2 > min(best, ub) >= the final minimum: it is neither the minimum nor a tie, and the output is the
// one of the plain ascending scan with its strict `<`, bit for bit.  tests/test_mesh_metrics_gpu.py is the judge.
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

// skip: 0 plain scan; 1 culled scan; 2 culled scan that also writes, per wave, how many tiles it did not scan to
// skipped[4 * block + wave] (the timing tool's figure; each wave owns its word).
__global__ __launch_bounds__(kMdBlock) void md_distance_kernel(const float* __restrict__ points, int n,
                                                               const float* __restrict__ vert,
                                                               const int32_t* __restrict__ faces, int nf, int nv,
                                                               int skip, const double* __restrict__ box,
                                                               int32_t* __restrict__ skipped,
                                                               double* __restrict__ dist2,
                                                               int32_t* __restrict__ nearest) {
  __shared__ double s_tri[kMdTile * kMdTriDoubles];
  __shared__ int s_home;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const size_t i = (size_t)blockIdx.x * kMdBlock + tid;
  const bool has = i < (size_t)n;
  const int ntiles = (nf + kMdTile - 1) / kMdTile;
  double px = 0.0, py = 0.0, pz = 0.0;
  if (has) px = (double)points[3 * i], py = (double)points[3 * i + 1], pz = (double)points[3 * i + 2];
  double best = INFINITY, ub = INFINITY;
  int best_f = -1, n_skipped = 0;

  if (skip) {
    // the tile whose box is nearest to the block's first point gives ub; which tile it is changes no output
    if (wave == 0) {
      const size_t i0 = (size_t)blockIdx.x * kMdBlock;
      const double qx = (double)points[3 * i0], qy = (double)points[3 * i0 + 1], qz = (double)points[3 * i0 + 2];
      double m = INFINITY, s2;
      int mt = -1;
      for (int t = lane; t < ntiles; t += kWave) {
        const double lb2 = md_box_lb2(qx, qy, qz, box + 6 * (size_t)t, &s2);
        if (lb2 < m) m = lb2, mt = t;
      }
      for (int off = 32; off > 0; off >>= 1) {
        const double om = __shfl_down(m, off, kWave);
        const int ot = __shfl_down(mt, off, kWave);
        if (ot >= 0 && (mt < 0 || om < m || (om == m && ot < mt))) m = om, mt = ot;
      }
      if (lane == 0) s_home = mt;
    }
    __syncthreads();
    const int home = s_home;
    if (home >= 0) {
      if (tid < kMdTile)
        md_load_tri(vert, faces, home * kMdTile + tid, nf, nv, s_tri + tid * kMdTriDoubles);
      __syncthreads();
      const int cnt = min(kMdTile, nf - home * kMdTile);
      for (int k = 0; k < cnt; k++) {
        const double* t = s_tri + k * kMdTriDoubles;
        if (t[9] != 0.0) ub = fmin(ub, md_dist2(px, py, pz, t));     // fmin: a NaN distance never becomes the bound
      }
    }
  }

  for (int tile = 0; tile < ntiles; tile++) {
    bool lane_skips = !has;
    if (skip && has) {
      double s2;
      const double lb2 = md_box_lb2(px, py, pz, box + 6 * (size_t)tile, &s2);
      lane_skips = lb2 > fmin(best, ub) * (1.0 + 0x1p-20) + 0x1p-27 * s2;
    }
    const bool wave_skips = skip && __all(lane_skips);
    // also the barrier between the last tile's reads and this tile's staging
    if (__syncthreads_and(skip && lane_skips)) {
      n_skipped++;
      continue;
    }
    if (tid < kMdTile) md_load_tri(vert, faces, tile * kMdTile + tid, nf, nv, s_tri + tid * kMdTriDoubles);
    __syncthreads();
    if (wave_skips) {
      n_skipped++;
      continue;
    }
    const int cnt = min(kMdTile, nf - tile * kMdTile);
    for (int k = 0; k < cnt; k++) {
      const double* t = s_tri + k * kMdTriDoubles;       // one address for the whole wave: an LDS broadcast
      if (t[9] != 0.0) {
        const double d = md_dist2(px, py, pz, t);
        if (d < best) best = d, best_f = tile * kMdTile + k;
      }
    }
  }
  if (has) {
    dist2[i] = best;
    nearest[i] = best_f;
  }
  if (skip == 2 && lane == 0) skipped[4 * (size_t)blockIdx.x + wave] = n_skipped;
}

static unsigned md_blocks(int n, int per) { return (unsigned)(((int64_t)n + per - 1) / per); }
static size_t md_box_bytes(int nf) { return (size_t)md_blocks(nf, kMdTile) * 6 * sizeof(double); }

}  // namespace mslam

using namespace mslam;

extern "C" int mslam_mesh_face_areas(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                                     double* area, void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_face_areas: negative size");
  if (num_faces == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && area && (vertices || num_vertices == 0), "mesh_face_areas: null pointer");
  hipLaunchKernelGGL(md_area_kernel, dim3(md_blocks(num_faces, 256)), dim3(256), 0, (hipStream_t)stream, vertices,
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
  hipLaunchKernelGGL(md_sample_kernel, dim3(md_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, vertices, faces,
                     num_faces, num_vertices, cdf, total, n, seed, points, face);
  MSLAM_LAUNCH_CHECK("mesh_sample");
  return MSLAM_OK;
}

extern "C" size_t mslam_mesh_distance_workspace_bytes(int num_faces) {
  return num_faces > 0 ? md_box_bytes(num_faces) : 0;
}

extern "C" int mslam_mesh_distance(const float* points, int n, const float* vertices, const int32_t* faces,
                                   int num_faces, int num_vertices, int skip, void* workspace, size_t workspace_bytes,
                                   double* dist2, int32_t* nearest, void* stream) {
  MSLAM_REQUIRE(n >= 0 && num_faces >= 0 && num_vertices >= 0, "mesh_distance: negative size");
  MSLAM_REQUIRE(skip >= 0 && skip <= 2, "mesh_distance: skip must be 0, 1 or 2");
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(points && dist2 && nearest, "mesh_distance: null pointer");
  MSLAM_REQUIRE(num_faces == 0 || (faces && (vertices || num_vertices == 0)), "mesh_distance: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const unsigned nblocks = md_blocks(n, kMdBlock);
  if (num_faces == 0) skip = 0;
  const size_t box_bytes = md_box_bytes(num_faces);
  if (skip) {
    const size_t count_bytes = skip == 2 ? (size_t)nblocks * 4 * sizeof(int32_t) : 0;
    MSLAM_REQUIRE(workspace, "mesh_distance: the culled scan needs a workspace");
    if (workspace_bytes < box_bytes + count_bytes) {
      set_error("mesh_distance: workspace of %zu bytes, %zu needed", workspace_bytes, box_bytes + count_bytes);
      return MSLAM_ENOMEM;
    }
    hipLaunchKernelGGL(md_box_kernel, dim3(md_blocks(num_faces, kMdTile)), dim3(kWave), 0, s, vertices, faces,
                       num_faces, num_vertices, (double*)workspace);
    if (num_faces <= kMdTile) {                  // one tile: it is scanned whatever its box says, so scan it once
      if (count_bytes) {
        int rc = check_hip(hipMemsetAsync((char*)workspace + box_bytes, 0, count_bytes, s), "mesh_distance memset");
        if (rc) return rc;
      }
      skip = 0;
    }
  }
  hipLaunchKernelGGL(md_distance_kernel, dim3(nblocks), dim3(kMdBlock), 0, s, points, n, vertices, faces, num_faces,
                     num_vertices, skip, (const double*)workspace,
                     skip == 2 ? (int32_t*)((char*)workspace + box_bytes) : nullptr, dist2, nearest);
  MSLAM_LAUNCH_CHECK("mesh_distance");
  return MSLAM_OK;
}
