// What the two ICP steps share (mesh_align.hip: point-to-mesh with the closed-form solve; icp_plane.hip: point-to-plane
// with the Gauss-Newton solve): the rotation of the state's quaternion, the action of the state on a point, and the
// block reduce in the fixed order both document (f64, uncontracted), and the argument checks of their entry points.
#pragma once
#include "mesh_tri.h"

// The checks every step's entry point shares, on its own parameters src, n, trim, workspace, state, nearest, moved,
// dist2 and log_row; sizes_ok: its sizes are >= 0
#define MA_REQUIRE_STEP(what, sizes_ok)                                                \
  MSLAM_REQUIRE(sizes_ok, what ": negative size");                                     \
  MSLAM_REQUIRE(trim >= 0.0, what ": trim must be >= 0 (+inf keeps every pair)");      \
  MSLAM_REQUIRE(state && log_row, what ": null pointer");                              \
  MSLAM_REQUIRE(n == 0 || (src && nearest && moved && dist2 && workspace), what ": null pointer")

namespace mslam {

// row-major rotation of the unit quaternion q = (x, y, z, w)
__host__ __device__ __forceinline__ void ma_quat_to_mat(const double* q, double* R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - z * w);       R[2] = 2.0 * (x * z + y * w);
  R[3] = 2.0 * (x * y + z * w);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - x * w);
  R[6] = 2.0 * (x * z - y * w);       R[7] = 2.0 * (y * z + x * w);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// y = s * (R p) + t
__host__ __device__ __forceinline__ void ma_act(const double* R, const double* t, double s, const double* p, double* y) {
#pragma unroll
  for (int d = 0; d < 3; d++) y[d] = s * ((R[3 * d] * p[0] + R[3 * d + 1] * p[1]) + R[3 * d + 2] * p[2]) + t[d];
}

// Block sum of the kSums values v in a fixed order -> partial[kSums * block + k]: a shuffle tree in the wave, then the
// four waves in wave order.  s_part: 4 * kSums doubles of LDS.  A block of kMdBlock threads.
template <int kSums>
__device__ __forceinline__ void ma_block_reduce(double* v, double* s_part, double* __restrict__ partial) {
  static_assert(kSums <= kMdBlock, "one thread per sum writes the block's partial");
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
#pragma unroll
  for (int k = 0; k < kSums; k++) {
    const double x = wave_sum(v[k]);
    if (lane == 0) s_part[wave * kSums + k] = x;
  }
  __syncthreads();
  if (tid < kSums)
    partial[kSums * (size_t)blockIdx.x + tid] =
        ((s_part[tid] + s_part[kSums + tid]) + s_part[2 * kSums + tid]) + s_part[3 * kSums + tid];
}

}  // namespace mslam
