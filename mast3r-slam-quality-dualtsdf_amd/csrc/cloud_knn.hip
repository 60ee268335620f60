// Point clouds: the k nearest neighbours of a point in a cloud, and normals from them.  Semantics in DESIGN.md "Point
// clouds"; tests/cloud_knn_numpy.py states the same definitions, operation by operation, in numpy.  Everything is f64
// on the f32 inputs in one fixed order and the build has -ffp-contract=off, so a * b + c below is two roundings.
//
// THE DEFINITION.  Row i of kn_kernel's output holds the k smallest valid points of the cloud under the TOTAL ORDER
// (dist2, original index), ascending: dist2 is MdPoint::dist2, the sum cloud_distance uses.  With `exclude` the point
// whose index is exclude[i] is left out of row i (by index: a duplicate of it at another index stays, at distance 0).
// Slots beyond the points that qualify hold (+inf, -1), and so does the whole row of a query with a non-finite
// coordinate.  k = 1 without exclude is cloud_distance's output, bit for bit.
//
// THE LIST.  Each lane keeps a sorted list of kCap (dist2, index) pairs in registers, kCap in {8, 16, 32} a template
// parameter and the runtime k <= kCap.  Only the last k slots are live: the first kCap - k hold (-inf, -1), below every
// candidate, and never move, so the list's last entry is the lane's k-th best - (+inf, -1) while fewer than k points
// have been met - at a constant register index whatever k is.  A candidate is offered only when it beats that entry
// under the total order; kn_offer is then one fully unrolled compare-and-shift pass, every index a constant, so nothing
// is indexed at run time and nothing goes to scratch (the resource table is in DESIGN.md).
//
// WHY CULLING STAYS EXACT.  The invariant of mesh_tri.h, read with the k-th best in the place of the best: md_walk
// compares a box with the policy's bound(), and KnList's is the list's last entry.  A point of a tile lies in the
// tile's box exactly, so its dist2 is at least the box's lb2 up to the roundings of the two sums.  A tile (or a group
// of 32) is skipped only when every lane with a query has
//     lb2 > kth (1 + 2^-20) + 2^-27 S^2 ,
// kth = +inf while the lane's list is not full.  Every point of a skipped tile is then strictly beyond the lane's
// current k-th best, which only shrinks: the point is neither in the final list nor tied with its last entry.
//
// THE HOME TILE.  The set of the k smallest under a total order, and their order, do not depend on the order of the
// visit.  So with an index the block first scans its home tile - the tile whose box is nearest to the block's first
// query, md_home_tile - as an ordinary tile, which fills the lists with near points, and hands it to the walk as
// `done`: the walk passes over that tile when it reaches it, so every point is still offered at most once.  Which tile
// it is changes no output bit.  There is no separate upper bound: the list's last entry is the bound.
//
// THE WALK is md_walk<MdPoint, kIndexed> of mesh_tri.h, md_scan's walk over a policy object: one query per thread,
// 256 per block, tiles of 128 points staged through LDS as f64 by md_stage<MdPoint, .>, one __syncthreads_and per tile
// that is also the barrier before the next staging; a lane without a query idles through the barriers and never keeps
// a tile in.  The policy object is KnList below.  MdPoint::load tags every valid slot with 1 + its
// original index, so the plain scan (order NULL: the tiles of the input order, nothing culled) applies the same total
// order and there is one kernel body.  An `order` entry outside [0, N) is skipped (md_slot); a point that `order` does
// not name is not seen, and `order` is taken to name no point twice.
// No atomics, no waiting between blocks, every loop bounded by a tile count or k.
//
// NORMALS.  kn_normals_kernel, one thread per point: centroid and covariance of the point's neighbour row in list
// order, the eigenvectors by cyclic Jacobi (kn_jacobi3 of jacobi3.h), the column of the smallest eigenvalue, its sign
// from a viewpoint or the largest component.
#include "cloud_point.h"
#include "jacobi3.h"

namespace mslam {

constexpr int kKnMaxK = MSLAM_CLOUD_KNN_MAX_K;      // the largest list a lane keeps in registers
constexpr int kKnMoments = MSLAM_CLOUD_NORMALS_MOMENTS;

__device__ __forceinline__ bool kn_less(double d, int i, double e, int j) { return d < e || (d == e && i < j); }

// (c, ci), which beats the list's last entry, into its place; the last entry drops out
template <int kCap>
__device__ __forceinline__ void kn_offer(double (&ld)[kCap], int (&li)[kCap], double c, int ci) {
  bool below_this = true;                            // c < entry j, j the slot being written
#pragma unroll
  for (int j = kCap - 1; j >= 1; j--) {
    const bool below_prev = kn_less(c, ci, ld[j - 1], li[j - 1]);
    ld[j] = below_prev ? ld[j - 1] : (below_this ? c : ld[j]);
    li[j] = below_prev ? li[j - 1] : (below_this ? ci : li[j]);
    below_this = below_prev;
  }
  if (below_this) ld[0] = c, li[0] = ci;
}

// What a lane keeps (the policy md_walk of mesh_tri.h asks for): the sorted list, and `ex`, the original index left out
// (-1: none).  kn_kernel builds the list in place, scans with it and stores from it.
template <int kCap>
struct KnList {
  int ex;
  double ld[kCap];
  int li[kCap];
  __device__ __forceinline__ double bound() const { return ld[kCap - 1]; }
  template <bool kIndexed>
  __device__ __forceinline__ void offer(double d, double tag, int) {
    const int f = (int)tag - 1;
    if (f != ex && kn_less(d, f, ld[kCap - 1], li[kCap - 1])) kn_offer<kCap>(ld, li, d, f);
  }
};

template <int kCap, bool kIndexed>
__global__ __launch_bounds__(kMdBlock) void kn_kernel(const float* __restrict__ queries, int n,
                                                      const float* __restrict__ points, int num_points, int k,
                                                      const int32_t* __restrict__ exclude,
                                                      const int32_t* __restrict__ order,
                                                      const double* __restrict__ box, const double* __restrict__ gbox,
                                                      int32_t* __restrict__ skipped, double* __restrict__ dist2,
                                                      int32_t* __restrict__ neighbors) {
  __shared__ double s_pts[kMdTile * MdPoint::kDoubles];
  __shared__ int s_home;
  const int tid = threadIdx.x;
  const size_t i0 = (size_t)blockIdx.x * kMdBlock, i = i0 + tid;
  const bool in_range = i < (size_t)n;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  if (in_range) qx = queries[3 * i], qy = queries[3 * i + 1], qz = queries[3 * i + 2];
  const bool has = in_range && cd_finite(qx, qy, qz);
  const double px = (double)qx, py = (double)qy, pz = (double)qz;
  const MdPoint::Src src = {points, num_points};
  const int ntiles = (num_points + kMdTile - 1) / kMdTile;

  // a lane without a query keeps (-inf, -1) throughout: nothing beats it, so the lane never inserts
  KnList<kCap> list;
  list.ex = in_range && exclude ? exclude[i] : -1;
#pragma unroll
  for (int s = 0; s < kCap; s++) list.ld[s] = has && s >= kCap - k ? INFINITY : -INFINITY, list.li[s] = -1;
  int home = -1;

  if (kIndexed && __syncthreads_or(has)) {
    home = md_home_tile((double)queries[3 * i0], (double)queries[3 * i0 + 1], (double)queries[3 * i0 + 2], box,
                        ntiles, &s_home);
    if (home >= 0) {
      const int cnt = min(kMdTile, num_points - home * kMdTile);          // before the staging branch, as in md_scan
      if (tid < kMdTile) md_stage<MdPoint, kIndexed>(src, order, home, tid, s_pts);
      __syncthreads();
      md_offer_tile<MdPoint, kIndexed>(s_pts, home, cnt, px, py, pz, list);
    }
  }
  const int n_skipped =
      md_walk<MdPoint, kIndexed>(px, py, pz, has, src, kIndexed, box, gbox, order, s_pts, ntiles, home, list);

  if (in_range) {
#pragma unroll
    for (int s = 0; s < kCap; s++) {
      const int slot = s - (kCap - k);
      if (slot >= 0) {
        dist2[i * (size_t)k + slot] = has ? list.ld[s] : INFINITY;
        neighbors[i * (size_t)k + slot] = has ? list.li[s] : -1;
      }
    }
  }
  if (skipped && (tid & (kWave - 1)) == 0) skipped[4 * (size_t)blockIdx.x + tid / kWave] = n_skipped;
}

// One point per thread.  moments (may be null): f64[N,15] - the centroid, the covariance xx xy xz yy yz zz (zeros for
// a point without a neighbour), the three diagonal entries after the sweeps and the oriented normal before its rounding
// to f32 - what the tests compare with the statement.
__global__ __launch_bounds__(256) void kn_normals_kernel(const float* __restrict__ points, int n,
                                                         const int32_t* __restrict__ neighbors, int k,
                                                         const float* __restrict__ viewpoints, int viewpoint_stride,
                                                         float* __restrict__ normals, float* __restrict__ curvature,
                                                         int32_t* __restrict__ count, double* __restrict__ moments) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n) return;
  const float fx = points[3 * i], fy = points[3 * i + 1], fz = points[3 * i + 2];
  const bool valid = cd_finite(fx, fy, fz);
  const int32_t* row = neighbors + i * (size_t)k;
  int m = 0;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  if (valid) {
    for (int s = 0; s < k; s++) {
      const int j = row[s];
      if ((unsigned)j >= (unsigned)n) continue;
      sx += (double)points[3 * (size_t)j], sy += (double)points[3 * (size_t)j + 1];
      sz += (double)points[3 * (size_t)j + 2];
      m++;
    }
  }
  const double dm = (double)m;
  double cx = 0.0, cy = 0.0, cz = 0.0, xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
  if (m > 0) {
    cx = sx / dm, cy = sy / dm, cz = sz / dm;
    for (int s = 0; s < k; s++) {
      const int j = row[s];
      if ((unsigned)j >= (unsigned)n) continue;
      const double rx = (double)points[3 * (size_t)j] - cx, ry = (double)points[3 * (size_t)j + 1] - cy;
      const double rz = (double)points[3 * (size_t)j + 2] - cz;
      xx += rx * rx, xy += rx * ry, xz += rx * rz, yy += ry * ry, yz += ry * rz, zz += rz * rz;
    }
    xx = xx / dm, xy = xy / dm, xz = xz / dm, yy = yy / dm, yz = yz / dm, zz = zz / dm;
  }
  double* mom = moments ? moments + kKnMoments * i : nullptr;
  if (mom) {
    mom[0] = cx, mom[1] = cy, mom[2] = cz;
    mom[3] = xx, mom[4] = xy, mom[5] = xz, mom[6] = yy, mom[7] = yz, mom[8] = zz;
  }

  double A[3][3] = {{xx, xy, xz}, {xy, yy, yz}, {xz, yz, zz}};
  double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  kn_jacobi3(A, V);
  const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
  int lo = 0;
  double lmin = l0;
  if (l1 < lmin) lo = 1, lmin = l1;
  if (l2 < lmin) lo = 2, lmin = l2;
  const double lmax = fmax(fmax(l0, l1), l2);
  const double lmid = fmax(fmin(l0, l1), fmin(fmax(l0, l1), l2));
  const bool degenerate = m < 3 || lmid <= 0x1p-40 * lmax;
  double nx = lo == 0 ? V[0][0] : lo == 1 ? V[0][1] : V[0][2];
  double ny = lo == 0 ? V[1][0] : lo == 1 ? V[1][1] : V[1][2];
  double nz = lo == 0 ? V[2][0] : lo == 1 ? V[2][1] : V[2][2];
  double n2 = 0.0;
  n2 += nx * nx, n2 += ny * ny, n2 += nz * nz;
  const double inv = 1.0 / sqrt(n2);
  nx = nx * inv, ny = ny * inv, nz = nz * inv;
  bool flip;
  if (viewpoints) {
    const float* v = viewpoints + (size_t)viewpoint_stride * i;
    const double dx = (double)v[0] - (double)fx, dy = (double)v[1] - (double)fy, dz = (double)v[2] - (double)fz;
    flip = (nx * dx + ny * dy) + nz * dz < 0.0;
  } else {
    double big = nx;
    if (fabs(ny) > fabs(big)) big = ny;
    if (fabs(nz) > fabs(big)) big = nz;
    flip = big < 0.0;
  }
  if (flip) nx = -nx, ny = -ny, nz = -nz;
  if (mom) {
    mom[9] = l0, mom[10] = l1, mom[11] = l2;
    mom[12] = degenerate ? 0.0 : nx, mom[13] = degenerate ? 0.0 : ny, mom[14] = degenerate ? 0.0 : nz;
  }
  normals[3 * i] = degenerate ? 0.0f : (float)nx;
  normals[3 * i + 1] = degenerate ? 0.0f : (float)ny;
  normals[3 * i + 2] = degenerate ? 0.0f : (float)nz;
  curvature[i] = degenerate ? NAN : (float)(fmax(lmin, 0.0) / ((l0 + l1) + l2));
  count[i] = m;
}

}  // namespace mslam

using namespace mslam;

extern "C" int mslam_cloud_knn(const float* queries, int n, const float* points, int num_points, int k,
                               const int32_t* exclude, const int32_t* order, const void* index, size_t index_bytes,
                               int levels, int32_t* skip_counts, double* dist2, int32_t* neighbors, void* stream) {
  MSLAM_REQUIRE(n >= 0 && num_points >= 0, "cloud_knn: negative size");
  MSLAM_REQUIRE(k >= 1 && k <= kKnMaxK, "cloud_knn: k must be in [1, %d], got %d", kKnMaxK, k);
  if (int rc = md_levels_arg("cloud_knn", levels)) return rc;
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(queries && dist2 && neighbors, "cloud_knn: null pointer");
  MSLAM_REQUIRE(num_points == 0 || points, "cloud_knn: null pointer");
  MdIndexArg ix;
  if (int rc = md_index_arg("cloud_knn", num_points, order, index, index_bytes, levels, &ix)) return rc;
  // the smallest capacity that holds k, plain or indexed
  static const decltype(&kn_kernel<8, false>) kernels[3][2] = {{kn_kernel<8, false>, kn_kernel<8, true>},
                                                                 {kn_kernel<16, false>, kn_kernel<16, true>},
                                                                 {kn_kernel<32, false>, kn_kernel<32, true>}};
  const auto kernel = kernels[k <= 8 ? 0 : k <= 16 ? 1 : 2][ix.order != nullptr];
  hipLaunchKernelGGL(kernel, dim3(blocks_for(n, kMdBlock)), dim3(kMdBlock), 0, (hipStream_t)stream, queries, n, points,
                     num_points, k, exclude, ix.order, ix.box, ix.gbox, skip_counts, dist2, neighbors);
  MSLAM_LAUNCH_CHECK("cloud_knn");
  return MSLAM_OK;
}

extern "C" int mslam_cloud_normals(const float* points, int num_points, const int32_t* neighbors, int k,
                                   const float* viewpoints, int viewpoint_stride, float* normals, float* curvature,
                                   int32_t* count, double* moments, void* stream) {
  MSLAM_REQUIRE(num_points >= 0, "cloud_normals: negative size");
  MSLAM_REQUIRE(k >= 1 && k <= kKnMaxK, "cloud_normals: k must be in [1, %d], got %d", kKnMaxK, k);
  MSLAM_REQUIRE(!viewpoints || viewpoint_stride == 0 || viewpoint_stride == 3,
                "cloud_normals: viewpoint_stride must be 0 (one for all) or 3 (one per point)");
  if (num_points == 0) return MSLAM_OK;
  MSLAM_REQUIRE(points && neighbors && normals && curvature && count, "cloud_normals: null pointer");
  hipLaunchKernelGGL(kn_normals_kernel, dim3(blocks_for(num_points, 256)), dim3(256), 0, (hipStream_t)stream, points,
                     num_points, neighbors, k, viewpoints, viewpoint_stride, normals, curvature, count, moments);
  MSLAM_LAUNCH_CHECK("cloud_normals");
  return MSLAM_OK;
}
