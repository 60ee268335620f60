// Point clouds: which planes a cloud consists of, by sequential RANSAC.  Semantics in DESIGN.md "Cloud planes";
// tests/cloud_planes_numpy.py states the same definitions in numpy, operation by operation.  All arithmetic on
// coordinates is f64 on the f32 inputs, one multiply or add at a time (the build has -ffp-contract=off); the counts are
// integers, summed with integer atomics, and the sums of the refit are reduced in one fixed order.  No float atomics.
//
// THE ROUND.  One round finds one plane, a call enqueues up to max_planes rounds and the host reads nothing back in
// between: M, planes_found, `done` and the chosen hypothesis live in `state` (i32[MSLAM_CLOUD_PLANES_STATE]), the
// current plane, its origin, the sums of its supporters and the candidate of the refit in `fit`
// (f64[MSLAM_CLOUD_PLANES_FIT]).  Every kernel of a round but the compaction returns at once when `done` is set.
//   remaining  pl_flag_kernel, pl_scan_kernel, pl_compact_kernel: the valid points without a label, ascending, by a
//              stable scan (block counts, one block scans them, ranks by ballot).  M < max(3, min_points) sets done.
//   draw       pl_draw_kernel: hypothesis h takes rem[draw(seed, r, h, j)], j = 0, 1, 2, draw SplitMix64's finaliser
//              three times over, mod M.  A void hypothesis (two equal draws, or a length that is not finite and > 0) is
//              four NaNs: no residual of it compares <= tol, so it counts 0.
//   count      pl_count_kernel, the hot one: H x M plane tests (below).
//   select     pl_select_kernel: one wave, the largest count and the lowest h on ties; below min_points sets done.
//   refit      pl_sums_kernel + pl_fit_kernel, 1 + iterations times: the eleven sums over the supporters of the plane
//              in turn (ma_block_reduce per block of 256 list rows, then one block adds the blocks t, t + 256, ... per
//              thread and reduces again), covariance, kn_jacobi3, a candidate; the candidate replaces the plane unless
//              the fit is degenerate or it has fewer supporters, which ends the refit (state[kStopped]).
//   label      pl_label_kernel gives the supporters the label planes_found; pl_commit_kernel orients the plane, writes
//              its row and increments planes_found.
//
// THE COUNT.  The hypotheses of the round lie in LDS, four doubles each (32 KB at the maximum of 1024), and are read as
// wave-wide broadcasts.  A lane holds kPlPerLane points of the remaining list in registers as doubles (their normals
// too under the gate) and walks the hypotheses; per hypothesis the wave takes a ballot per point, adds the popcounts
// (wave-uniform) and one lane adds the total to the block's integer count in LDS.  A block strides over the list in
// chunks of 256 kPlPerLane rows - the grid goes over the remaining list, never over N - and at its end adds each
// non-zero count to the global count with one integer atomic per (block, hypothesis).  A row past M, a point index
// outside [0, N) and, under the gate, a normal that is zero or not finite are loaded as NaN: no comparison with a NaN
// holds, so they never count, without a flag in the loop.  Integer sums do not depend on their order: the same bits
// whatever the grid.  The grid is capped at kPlMaxBlocks; with 36 KB of LDS four blocks fit a CU.  Nobody has measured
// these choices against others; tools/cloud_planes_time.py times the kernel as it is.
#include "cloud_point.h"
#include "jacobi3.h"
#include "mesh_align.h"

namespace mslam {

constexpr int kPlM = 0, kPlFound = 1, kPlDone = 2, kPlBestH = 3, kPlBestCount = 4, kPlStopped = 5;   // state
constexpr int kPlPlane = 0, kPlOrigin = 4, kPlSums = 8, kPlCand = 19, kPlTotal = 23;                   // fit
constexpr int kPlNumSums = MSLAM_CLOUD_PLANES_SUMS;
constexpr int kPlPerLane = 4;
constexpr int kPlChunk = kMdBlock * kPlPerLane;
constexpr int kPlMaxBlocks = 1024;
constexpr int kPlScanBlock = 1024;
static_assert(kPlTotal + kPlNumSums <= MSLAM_CLOUD_PLANES_FIT, "fit holds the plane, origin, sums, candidate, total");
static_assert(kPlNumSums == 11 && MSLAM_CLOUD_PLANES_ROW == 13, "the layouts tests/cloud_planes_numpy.py states");

__device__ __forceinline__ uint64_t pl_mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the list's length: never beyond the buffer the caller named
__device__ __forceinline__ int pl_len(const int32_t* state, int num_remaining) {
  const int m = state[kPlM];
  return m < 0 ? 0 : (m < num_remaining ? m : num_remaining);
}

// Point v of the cloud as doubles; NaN for an index outside [0, N)
__device__ __forceinline__ void pl_point(const float* __restrict__ points, int num_points, int v, double* p) {
  if ((unsigned)v < (unsigned)num_points) {
    p[0] = (double)points[3 * (size_t)v], p[1] = (double)points[3 * (size_t)v + 1], p[2] = (double)points[3 * (size_t)v + 2];
  } else {
    p[0] = p[1] = p[2] = NAN;
  }
}

// The normal of point v as doubles; NaN when it is zero or not finite, or v outside [0, N)
__device__ __forceinline__ void pl_normal(const float* __restrict__ normals, int num_points, int v, double* m) {
  m[0] = m[1] = m[2] = NAN;
  if ((unsigned)v >= (unsigned)num_points) return;
  const float x = normals[3 * (size_t)v], y = normals[3 * (size_t)v + 1], z = normals[3 * (size_t)v + 2];
  if (cd_finite(x, y, z) && (x != 0.0f || y != 0.0f || z != 0.0f)) m[0] = (double)x, m[1] = (double)y, m[2] = (double)z;
}

__device__ __forceinline__ double pl_residual(const double* n, const double* p) {
  return ((n[0] * p[0] + n[1] * p[1]) + n[2] * p[2]) + n[3];
}

template <bool kGate>
__device__ __forceinline__ bool pl_supports(const double* n, const double* p, const double* m, double tol, double cosa) {
  bool s = fabs(pl_residual(n, p)) <= tol;
  if (kGate) s = s && fabs((n[0] * m[0] + n[1] * m[1]) + n[2] * m[2]) >= cosa;
  return s;
}

// ---- remaining -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pl_flag(const float* __restrict__ points, const int32_t* __restrict__ labels, int n,
                                        int64_t i) {
  if (i >= n) return false;
  return labels[i] < 0 && cd_finite(points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]);
}

__global__ __launch_bounds__(kMdBlock) void pl_flag_kernel(const float* __restrict__ points,
                                                           const int32_t* __restrict__ labels, int n,
                                                           const int32_t* __restrict__ state,
                                                           int32_t* __restrict__ block_count) {
  if (state[kPlDone]) return;
  __shared__ int s_wave[4];
  const int tid = threadIdx.x;
  const uint64_t b = __ballot(pl_flag(points, labels, n, (int64_t)blockIdx.x * kMdBlock + tid));
  if ((tid & (kWave - 1)) == 0) s_wave[tid / kWave] = __popcll(b);
  __syncthreads();
  if (tid == 0) block_count[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

// One block: block_count[b] becomes the number of list rows in front of block b; M and done into the state
__global__ __launch_bounds__(kPlScanBlock) void pl_scan_kernel(int nblocks, int min_points, int32_t* block_count,
                                                               int32_t* state) {
  if (state[kPlDone]) return;
  __shared__ int s_wave[kPlScanBlock / kWave];
  __shared__ int s_base;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int start = 0; start < nblocks; start += kPlScanBlock) {
    const int b = start + tid;
    const int own = b < nblocks ? block_count[b] : 0;
    int incl = own;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int up = __shfl_up(incl, off, kWave);
      if (lane >= off) incl += up;
    }
    if (lane == kWave - 1) s_wave[wave] = incl;
    __syncthreads();
    int before = s_base;
    for (int w = 0; w < wave; w++) before += s_wave[w];
    if (b < nblocks) block_count[b] = before + incl - own;
    __syncthreads();
    if (tid == kPlScanBlock - 1) s_base = before + incl;
    __syncthreads();
  }
  if (tid == 0) {
    const int m = s_base;
    state[kPlM] = m;
    if (m < (min_points > 3 ? min_points : 3)) state[kPlDone] = 1;
  }
}

__global__ __launch_bounds__(kMdBlock) void pl_compact_kernel(const float* __restrict__ points,
                                                              const int32_t* __restrict__ labels, int n,
                                                              const int32_t* __restrict__ state,
                                                              const int32_t* __restrict__ block_offset,
                                                              int32_t* __restrict__ remaining) {
  // done from the scan of this very round: the list is written all the same, it is only never read
  __shared__ int s_wave[4];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t i = (int64_t)blockIdx.x * kMdBlock + tid;
  const bool f = pl_flag(points, labels, n, i);
  const uint64_t b = __ballot(f);
  if (lane == 0) s_wave[wave] = __popcll(b);
  __syncthreads();
  if (!f) return;
  int rank = block_offset[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; w++) rank += s_wave[w];
  if ((unsigned)rank < (unsigned)n) remaining[rank] = (int)i; // offsets a caller's stale state left behind: never past the list
}

// ---- draw ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pl_draw_kernel(const float* __restrict__ points, int num_points,
                                                      const int32_t* __restrict__ remaining, int num_remaining,
                                                      const int32_t* __restrict__ state, uint64_t seed, int round,
                                                      int num_hyp, double* __restrict__ hyp,
                                                      int32_t* __restrict__ triples) {
  if (state[kPlDone]) return;
  const int h = blockIdx.x * 256 + threadIdx.x;
  if (h >= num_hyp) return;
  const uint64_t m = (uint64_t)pl_len(state, num_remaining);
  double out[4] = {NAN, NAN, NAN, NAN};
  int v[3] = {-1, -1, -1};
  if (m > 0) {
    const uint64_t key = pl_mix(pl_mix(seed) ^ (((uint64_t)(uint32_t)round << 32) | (uint64_t)(uint32_t)h));
    uint64_t pos[3];
    double p[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      pos[j] = pl_mix(key ^ (uint64_t)j) % m;
      v[j] = remaining[pos[j]];
      pl_point(points, num_points, v[j], p[j]);
    }
    const double ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
    const double bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
    double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    nx = nx / len, ny = ny / len, nz = nz / len;
    const double d = -((nx * p[0][0] + ny * p[0][1]) + nz * p[0][2]);
    const bool distinct = pos[0] != pos[1] && pos[0] != pos[2] && pos[1] != pos[2];
    if (distinct && isfinite(len) && len > 0.0) out[0] = nx, out[1] = ny, out[2] = nz, out[3] = d;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) hyp[4 * (size_t)h + k] = out[k];
#pragma unroll
  for (int j = 0; j < 3; j++) triples[3 * (size_t)h + j] = v[j];
}

// ---- count -----------------------------------------------------------------------------------------------------------
template <bool kGate>
__global__ __launch_bounds__(kMdBlock) void pl_count_kernel(const float* __restrict__ points,
                                                            const float* __restrict__ normals, int num_points,
                                                            const int32_t* __restrict__ remaining, int num_remaining,
                                                            const int32_t* __restrict__ state,
                                                            const double* __restrict__ hyp, int num_hyp, double tol,
                                                            double cosa, int32_t* count) {
  if (state[kPlDone]) return;
  __shared__ double s_hyp[4 * MSLAM_CLOUD_PLANES_MAX_HYPOTHESES];
  __shared__ int s_count[MSLAM_CLOUD_PLANES_MAX_HYPOTHESES];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int m = pl_len(state, num_remaining);
  if ((int64_t)blockIdx.x * kPlChunk >= m) return;            // block-uniform: before any barrier
  for (int k = tid; k < 4 * num_hyp; k += kMdBlock) s_hyp[k] = hyp[k];
  for (int h = tid; h < num_hyp; h += kMdBlock) s_count[h] = 0;
  __syncthreads();
  for (int64_t base = (int64_t)blockIdx.x * kPlChunk; base < m; base += (int64_t)gridDim.x * kPlChunk) {
    double p[kPlPerLane][3], nm[kPlPerLane][3];
#pragma unroll
    for (int s = 0; s < kPlPerLane; s++) {
      const int64_t row = base + s * kMdBlock + tid;           // a wave's rows are consecutive
      const int v = row < m ? remaining[row] : -1;
      pl_point(points, num_points, v, p[s]);
      if (kGate) pl_normal(normals, num_points, v, nm[s]);
    }
    for (int h = 0; h < num_hyp; h++) {
      const double n[4] = {s_hyp[4 * h], s_hyp[4 * h + 1], s_hyp[4 * h + 2], s_hyp[4 * h + 3]};
      int total = 0;
#pragma unroll
      for (int s = 0; s < kPlPerLane; s++) total += __popcll(__ballot(pl_supports<kGate>(n, p[s], nm[s], tol, cosa)));
      if (lane == 0 && total) atomicAdd(&s_count[h], total);
    }
  }
  __syncthreads();
  for (int h = tid; h < num_hyp; h += kMdBlock)
    if (s_count[h]) atomicAdd(&count[h], s_count[h]);
}

// ---- select ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void pl_select_kernel(const int32_t* __restrict__ count, int num_hyp, int min_points,
                                                          const float* __restrict__ points, int num_points,
                                                          const double* __restrict__ hyp,
                                                          const int32_t* __restrict__ triples, int32_t* state,
                                                          double* __restrict__ fit) {
  if (state[kPlDone]) return;
  const int lane = threadIdx.x;
  int best = -1, best_h = 0x7fffffff;
  for (int h = lane; h < num_hyp; h += kWave) {
    const int c = count[h];
    if (c > best) best = c, best_h = h;                        // ascending h: the first maximum stays
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int c = __shfl_down(best, off, kWave), h = __shfl_down(best_h, off, kWave);
    if (c > best || (c == best && h < best_h)) best = c, best_h = h;
  }
  if (lane != 0) return;
  state[kPlBestH] = best_h;
  state[kPlBestCount] = best;
  state[kPlStopped] = 0;
  if (best < min_points || best < 1) {
    state[kPlDone] = 1;
    return;
  }
  double origin[3];
  pl_point(points, num_points, triples[3 * (size_t)best_h], origin);
#pragma unroll
  for (int k = 0; k < 4; k++) fit[kPlPlane + k] = hyp[4 * (size_t)best_h + k];
#pragma unroll
  for (int k = 0; k < 3; k++) fit[kPlOrigin + k] = origin[k];
}

// ---- refit -----------------------------------------------------------------------------------------------------------
// The eleven sums over the supporters of the plane at fit[slot] among the list rows of this block -> partial
template <bool kGate>
__global__ __launch_bounds__(kMdBlock) void pl_sums_kernel(const float* __restrict__ points,
                                                           const float* __restrict__ normals, int num_points,
                                                           const int32_t* __restrict__ remaining, int num_remaining,
                                                           const int32_t* __restrict__ state,
                                                           const double* __restrict__ fit, int slot, double tol,
                                                           double cosa, double* __restrict__ partial) {
  if (state[kPlDone] || state[kPlStopped]) return;
  __shared__ double s_part[4 * kPlNumSums];
  const int m = pl_len(state, num_remaining);
  if ((int64_t)blockIdx.x * kMdBlock >= m) return;            // block-uniform
  const int64_t row = (int64_t)blockIdx.x * kMdBlock + threadIdx.x;
  const int v = row < m ? remaining[row] : -1;
  double p[3], nm[3] = {0.0, 0.0, 0.0};
  pl_point(points, num_points, v, p);
  if (kGate) pl_normal(normals, num_points, v, nm);
  const double n[4] = {fit[slot], fit[slot + 1], fit[slot + 2], fit[slot + 3]};
  double s[kPlNumSums];
#pragma unroll
  for (int k = 0; k < kPlNumSums; k++) s[k] = 0.0;
  if (pl_supports<kGate>(n, p, nm, tol, cosa)) {
    const double r = pl_residual(n, p);
    const double qx = p[0] - fit[kPlOrigin], qy = p[1] - fit[kPlOrigin + 1], qz = p[2] - fit[kPlOrigin + 2];
    s[0] = 1.0, s[1] = qx, s[2] = qy, s[3] = qz;
    s[4] = qx * qx, s[5] = qx * qy, s[6] = qx * qz, s[7] = qy * qy, s[8] = qy * qz, s[9] = qz * qz;
    s[10] = r * r;
  }
  ma_block_reduce<kPlNumSums>(s, s_part, partial);
}

// mean = sum q / c and the covariance sum q q^T / c - mean mean^T of the sums S
__device__ __forceinline__ void pl_covariance(const double* S, double* mean, double (&A)[3][3]) {
  const double c = S[0];
  mean[0] = S[1] / c, mean[1] = S[2] / c, mean[2] = S[3] / c;
  const double xx = S[4] / c, xy = S[5] / c, xz = S[6] / c, yy = S[7] / c, yz = S[8] / c, zz = S[9] / c;
  A[0][0] = xx - mean[0] * mean[0], A[0][1] = xy - mean[0] * mean[1], A[0][2] = xz - mean[0] * mean[2];
  A[1][0] = A[0][1], A[1][1] = yy - mean[1] * mean[1], A[1][2] = yz - mean[1] * mean[2];
  A[2][0] = A[0][2], A[2][1] = A[1][2], A[2][2] = zz - mean[2] * mean[2];
}

__device__ __forceinline__ void pl_identity(double (&V)[3][3]) {
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) V[a][b] = a == b ? 1.0 : 0.0;
}

// A candidate from the sums S about `origin`; false when the fit is degenerate
__device__ bool pl_fit_plane(const double* S, const double* origin, double* cand) {
  if (!(S[0] >= 3.0)) return false;
  double mean[3], A[3][3], V[3][3];
  pl_covariance(S, mean, A);
  pl_identity(V);
  kn_jacobi3(A, V);
  const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
  int lo = 0;
  double lmin = l0;
  if (l1 < lmin) lo = 1, lmin = l1;
  if (l2 < lmin) lo = 2, lmin = l2;
  const double lmax = fmax(fmax(l0, l1), l2);
  const double lmid = fmax(fmin(l0, l1), fmin(fmax(l0, l1), l2));
  if (lmid <= 0x1p-40 * lmax) return false;
  double vx = lo == 0 ? V[0][0] : (lo == 1 ? V[0][1] : V[0][2]);
  double vy = lo == 0 ? V[1][0] : (lo == 1 ? V[1][1] : V[1][2]);
  double vz = lo == 0 ? V[2][0] : (lo == 1 ? V[2][1] : V[2][2]);
  const double inv = 1.0 / sqrt((vx * vx + vy * vy) + vz * vz);
  vx = vx * inv, vy = vy * inv, vz = vz * inv;
  const double cx = origin[0] + mean[0], cy = origin[1] + mean[1], cz = origin[2] + mean[2];
  cand[0] = vx, cand[1] = vy, cand[2] = vz;
  cand[3] = -((vx * cx + vy * cy) + vz * cz);
  return true;
}

// One block.  The blocks' partials in a fixed order, then the step of the refit: phase 0 has the sums of the plane,
// phase >= 1 those of the candidate; `last`: no further candidate is wanted
__global__ __launch_bounds__(kMdBlock) void pl_fit_kernel(const double* __restrict__ partial, int num_remaining,
                                                          int phase, int last, int32_t* state, double* fit) {
  if (state[kPlDone] || state[kPlStopped]) return;
  __shared__ double s_part[4 * kPlNumSums];
  const int tid = threadIdx.x;
  const int nblocks = (pl_len(state, num_remaining) + kMdBlock - 1) / kMdBlock;
  double s[kPlNumSums];
#pragma unroll
  for (int k = 0; k < kPlNumSums; k++) s[k] = 0.0;
  for (int b = tid; b < nblocks; b += kMdBlock) {
#pragma unroll
    for (int k = 0; k < kPlNumSums; k++) s[k] = s[k] + partial[kPlNumSums * (size_t)b + k];
  }
  ma_block_reduce<kPlNumSums>(s, s_part, fit + kPlTotal);   // blockIdx.x is 0
  __syncthreads();
  if (tid != 0) return;
  const double* total = fit + kPlTotal;
  if (phase > 0 && !(total[0] >= fit[kPlSums])) {              // fewer supporters: the plane stays
    state[kPlStopped] = 1;
    return;
  }
  if (phase > 0) {
#pragma unroll
    for (int k = 0; k < 4; k++) fit[kPlPlane + k] = fit[kPlCand + k];
  }
  for (int k = 0; k < kPlNumSums; k++) fit[kPlSums + k] = total[k];
  if (last) return;
  double cand[4];
  if (!pl_fit_plane(fit + kPlSums, fit + kPlOrigin, cand)) {
    state[kPlStopped] = 1;
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) fit[kPlCand + k] = cand[k];
}

// ---- label -----------------------------------------------------------------------------------------------------------
template <bool kGate>
__global__ __launch_bounds__(kMdBlock) void pl_label_kernel(const float* __restrict__ points,
                                                            const float* __restrict__ normals, int num_points,
                                                            const int32_t* __restrict__ remaining, int num_remaining,
                                                            const int32_t* __restrict__ state,
                                                            const double* __restrict__ fit, double tol, double cosa,
                                                            int max_planes, int32_t* __restrict__ labels) {
  if (state[kPlDone] || state[kPlFound] >= max_planes) return;
  const int64_t row = (int64_t)blockIdx.x * kMdBlock + threadIdx.x;
  if (row >= pl_len(state, num_remaining)) return;
  const int v = remaining[row];
  if ((unsigned)v >= (unsigned)num_points) return;
  double p[3], nm[3] = {0.0, 0.0, 0.0};
  pl_point(points, num_points, v, p);
  if (kGate) pl_normal(normals, num_points, v, nm);
  const double n[4] = {fit[kPlPlane], fit[kPlPlane + 1], fit[kPlPlane + 2], fit[kPlPlane + 3]};
  if (pl_supports<kGate>(n, p, nm, tol, cosa)) labels[v] = state[kPlFound];
}

__global__ void pl_commit_kernel(const float* __restrict__ viewpoint, const double* __restrict__ fit, int max_planes,
                                 int32_t* state, double* __restrict__ planes) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (state[kPlDone] || state[kPlFound] >= max_planes) return;
  double n[4] = {fit[kPlPlane], fit[kPlPlane + 1], fit[kPlPlane + 2], fit[kPlPlane + 3]};
  bool flip;
  if (viewpoint) {
    const double v[3] = {(double)viewpoint[0], (double)viewpoint[1], (double)viewpoint[2]};
    flip = pl_residual(n, v) < 0.0;
  } else {
    double big = n[0];
    if (fabs(n[1]) > fabs(big)) big = n[1];
    if (fabs(n[2]) > fabs(big)) big = n[2];
    flip = big < 0.0;
  }
  double mean[3], A[3][3], V[3][3];
  pl_covariance(fit + kPlSums, mean, A);
  pl_identity(V);
  kn_jacobi3(A, V);
  double* row = planes + MSLAM_CLOUD_PLANES_ROW * (size_t)state[kPlFound];
#pragma unroll
  for (int k = 0; k < 4; k++) row[k] = flip ? -n[k] : n[k];
  row[4] = fit[kPlSums], row[5] = fit[kPlSums + 10];
#pragma unroll
  for (int k = 0; k < 3; k++) row[6 + k] = fit[kPlOrigin + k] + mean[k];
  row[9] = A[0][0], row[10] = A[1][1], row[11] = A[2][2];
  row[12] = sqrt(row[5] / row[4]);
  state[kPlFound] = state[kPlFound] + 1;
}

// ---- the stages' launches, shared by the entry points of the stages and by the whole call ---------------------------
struct PlArgs {
  const float* points;
  const float* normals;
  int n;
  double tol, cosa;
  hipStream_t stream;
};

static int pl_remaining(const PlArgs& a, const int32_t* labels, int min_points, int32_t* block_offset, int32_t* rem,
                        int32_t* state) {
  const unsigned nb = blocks_for(a.n, kMdBlock);
  hipLaunchKernelGGL(pl_flag_kernel, dim3(nb), dim3(kMdBlock), 0, a.stream, a.points, labels, a.n, state, block_offset);
  hipLaunchKernelGGL(pl_scan_kernel, dim3(1), dim3(kPlScanBlock), 0, a.stream, (int)nb, min_points, block_offset, state);
  hipLaunchKernelGGL(pl_compact_kernel, dim3(nb), dim3(kMdBlock), 0, a.stream, a.points, labels, a.n, state,
                     block_offset, rem);
  MSLAM_LAUNCH_CHECK("cloud_planes_remaining");
  return MSLAM_OK;
}

static int pl_draw(const PlArgs& a, const int32_t* rem, int num_rem, const int32_t* state, uint64_t seed, int round,
                   int num_hyp, double* hyp, int32_t* triples) {
  hipLaunchKernelGGL(pl_draw_kernel, dim3(blocks_for(num_hyp, 256)), dim3(256), 0, a.stream, a.points, a.n, rem,
                     num_rem, state, seed, round, num_hyp, hyp, triples);
  MSLAM_LAUNCH_CHECK("cloud_planes_draw");
  return MSLAM_OK;
}

static int pl_count(const PlArgs& a, const int32_t* rem, int num_rem, const int32_t* state, const double* hyp,
                    int num_hyp, int32_t* count) {
  if (int rc = check_hip(hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)num_hyp, a.stream), "cloud_planes_count"))
    return rc;
  if (num_rem == 0) return MSLAM_OK;
  unsigned nb = blocks_for(num_rem, kPlChunk);
  if (nb > (unsigned)kPlMaxBlocks) nb = kPlMaxBlocks;
  const auto kernel = a.normals ? pl_count_kernel<true> : pl_count_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(nb), dim3(kMdBlock), 0, a.stream, a.points, a.normals, a.n, rem, num_rem, state, hyp,
                     num_hyp, a.tol, a.cosa, count);
  MSLAM_LAUNCH_CHECK("cloud_planes_count");
  return MSLAM_OK;
}

static int pl_select(const PlArgs& a, const int32_t* count, int num_hyp, int min_points, const double* hyp,
                     const int32_t* triples, int32_t* state, double* fit) {
  hipLaunchKernelGGL(pl_select_kernel, dim3(1), dim3(kWave), 0, a.stream, count, num_hyp, min_points, a.points, a.n, hyp,
                     triples, state, fit);
  MSLAM_LAUNCH_CHECK("cloud_planes_select");
  return MSLAM_OK;
}

static int pl_refit(const PlArgs& a, const int32_t* rem, int num_rem, int iterations, double* partial, int32_t* state,
                    double* fit) {
  if (num_rem == 0) return MSLAM_OK;
  const auto sums = a.normals ? pl_sums_kernel<true> : pl_sums_kernel<false>;
  for (int phase = 0; phase <= iterations; phase++) {
    hipLaunchKernelGGL(sums, dim3(blocks_for(num_rem, kMdBlock)), dim3(kMdBlock), 0, a.stream, a.points, a.normals, a.n,
                       rem, num_rem, state, fit, phase == 0 ? kPlPlane : kPlCand, a.tol, a.cosa, partial);
    hipLaunchKernelGGL(pl_fit_kernel, dim3(1), dim3(kMdBlock), 0, a.stream, partial, num_rem, phase,
                       phase == iterations ? 1 : 0, state, fit);
  }
  MSLAM_LAUNCH_CHECK("cloud_planes_refit");
  return MSLAM_OK;
}

static int pl_label(const PlArgs& a, const int32_t* rem, int num_rem, const float* viewpoint, const double* fit,
                    int max_planes, int32_t* state, int32_t* labels, double* planes) {
  if (num_rem == 0) return MSLAM_OK;
  const auto kernel = a.normals ? pl_label_kernel<true> : pl_label_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(blocks_for(num_rem, kMdBlock)), dim3(kMdBlock), 0, a.stream, a.points, a.normals, a.n,
                     rem, num_rem, state, fit, a.tol, a.cosa, max_planes, labels);
  hipLaunchKernelGGL(pl_commit_kernel, dim3(1), dim3(kWave), 0, a.stream, viewpoint, fit, max_planes, state, planes);
  MSLAM_LAUNCH_CHECK("cloud_planes_label");
  return MSLAM_OK;
}

// the layout of the whole call's workspace
struct PlWorkspace {
  size_t block_offset, rem, hyp, triples, count, partial, fit, bytes;
  PlWorkspace(int n, int num_hyp) {
    const size_t nb = blocks_for(n, kMdBlock);
    size_t at = 0;
    const auto take = [&at](size_t bytes) {
      const size_t here = at;
      at += (bytes + 15) / 16 * 16;
      return here;
    };
    fit = take(sizeof(double) * MSLAM_CLOUD_PLANES_FIT);
    hyp = take(sizeof(double) * 4 * (size_t)num_hyp);
    partial = take(sizeof(double) * kPlNumSums * nb);
    block_offset = take(sizeof(int32_t) * nb);
    rem = take(sizeof(int32_t) * (size_t)n);
    triples = take(sizeof(int32_t) * 3 * (size_t)num_hyp);
    count = take(sizeof(int32_t) * (size_t)num_hyp);
    bytes = at;
  }
};

}  // namespace mslam

using namespace mslam;

#define PL_ALIGNED(p, a) ((uintptr_t)(p) % (a) == 0)
// The checks the entry points share, on their own parameters
#define PL_REQUIRE_CLOUD(what)                                                                  \
  MSLAM_REQUIRE(num_points >= 0, what ": negative size");                                      \
  MSLAM_REQUIRE(num_points == 0 || points, what ": null pointer");                             \
  MSLAM_REQUIRE(PL_ALIGNED(points, 4) && PL_ALIGNED(normals, 4), what ": misaligned pointer")
#define PL_REQUIRE_LIST(what)                                                                   \
  MSLAM_REQUIRE(num_remaining >= 0 && num_remaining <= num_points, what ": num_remaining must be in [0, num_points]"); \
  MSLAM_REQUIRE(state && (num_remaining == 0 || remaining), what ": null pointer");            \
  MSLAM_REQUIRE(PL_ALIGNED(state, 4) && PL_ALIGNED(remaining, 4), what ": misaligned pointer")
#define PL_REQUIRE_HYP(what)                                                                    \
  MSLAM_REQUIRE(num_hypotheses >= 1 && num_hypotheses <= MSLAM_CLOUD_PLANES_MAX_HYPOTHESES,    \
                what ": num_hypotheses must be in [1, %d], got %d", MSLAM_CLOUD_PLANES_MAX_HYPOTHESES, num_hypotheses)
#define PL_REQUIRE_TOL(what)                                                                    \
  MSLAM_REQUIRE(tol > 0.0 && tol < INFINITY, what ": tol must be finite and > 0, got %g", tol); \
  MSLAM_REQUIRE(!normals || (cos_angle >= 0.0 && cos_angle <= 1.0), what ": cos_angle must be in [0, 1], got %g", cos_angle)

extern "C" int mslam_cloud_planes_remaining(const float* points, int num_points, const int32_t* labels, int min_points,
                                            int32_t* block_offsets, int32_t* remaining, int32_t* state, void* stream) {
  const float* normals = nullptr;
  PL_REQUIRE_CLOUD("cloud_planes_remaining");
  MSLAM_REQUIRE(state && PL_ALIGNED(state, 4), "cloud_planes_remaining: null or misaligned state");
  MSLAM_REQUIRE(num_points == 0 || (labels && block_offsets && remaining), "cloud_planes_remaining: null pointer");
  MSLAM_REQUIRE(PL_ALIGNED(labels, 4) && PL_ALIGNED(block_offsets, 4) && PL_ALIGNED(remaining, 4),
                "cloud_planes_remaining: misaligned pointer");
  const PlArgs a = {points, nullptr, num_points, 0.0, 0.0, (hipStream_t)stream};
  return pl_remaining(a, labels, min_points, block_offsets, remaining, state);
}

extern "C" int mslam_cloud_planes_draw(const float* points, int num_points, const int32_t* remaining, int num_remaining,
                                       const int32_t* state, uint64_t seed, int round, int num_hypotheses,
                                       double* hypotheses, int32_t* triples, void* stream) {
  const float* normals = nullptr;
  PL_REQUIRE_CLOUD("cloud_planes_draw");
  PL_REQUIRE_LIST("cloud_planes_draw");
  PL_REQUIRE_HYP("cloud_planes_draw");
  MSLAM_REQUIRE(round >= 0, "cloud_planes_draw: negative round");
  MSLAM_REQUIRE(hypotheses && triples, "cloud_planes_draw: null pointer");
  MSLAM_REQUIRE(PL_ALIGNED(hypotheses, 8) && PL_ALIGNED(triples, 4), "cloud_planes_draw: misaligned pointer");
  const PlArgs a = {points, nullptr, num_points, 0.0, 0.0, (hipStream_t)stream};
  return pl_draw(a, remaining, num_remaining, state, seed, round, num_hypotheses, hypotheses, triples);
}

extern "C" int mslam_cloud_planes_count(const float* points, const float* normals, int num_points,
                                        const int32_t* remaining, int num_remaining, const int32_t* state,
                                        const double* hypotheses, int num_hypotheses, double tol, double cos_angle,
                                        int32_t* count, void* stream) {
  PL_REQUIRE_CLOUD("cloud_planes_count");
  PL_REQUIRE_LIST("cloud_planes_count");
  PL_REQUIRE_HYP("cloud_planes_count");
  PL_REQUIRE_TOL("cloud_planes_count");
  MSLAM_REQUIRE(hypotheses && count, "cloud_planes_count: null pointer");
  MSLAM_REQUIRE(PL_ALIGNED(hypotheses, 8) && PL_ALIGNED(count, 4), "cloud_planes_count: misaligned pointer");
  const PlArgs a = {points, normals, num_points, tol, cos_angle, (hipStream_t)stream};
  return pl_count(a, remaining, num_remaining, state, hypotheses, num_hypotheses, count);
}

extern "C" int mslam_cloud_planes_select(const int32_t* count, int num_hypotheses, int min_points, const float* points,
                                         int num_points, const double* hypotheses, const int32_t* triples,
                                         int32_t* state, double* fit, void* stream) {
  const float* normals = nullptr;
  PL_REQUIRE_CLOUD("cloud_planes_select");
  PL_REQUIRE_HYP("cloud_planes_select");
  MSLAM_REQUIRE(count && hypotheses && triples && state && fit, "cloud_planes_select: null pointer");
  MSLAM_REQUIRE(PL_ALIGNED(count, 4) && PL_ALIGNED(hypotheses, 8) && PL_ALIGNED(triples, 4) && PL_ALIGNED(state, 4) &&
                    PL_ALIGNED(fit, 8), "cloud_planes_select: misaligned pointer");
  const PlArgs a = {points, nullptr, num_points, 0.0, 0.0, (hipStream_t)stream};
  return pl_select(a, count, num_hypotheses, min_points, hypotheses, triples, state, fit);
}

extern "C" int mslam_cloud_planes_refit(const float* points, const float* normals, int num_points,
                                        const int32_t* remaining, int num_remaining, double tol, double cos_angle,
                                        int iterations, double* partial, int32_t* state, double* fit, void* stream) {
  PL_REQUIRE_CLOUD("cloud_planes_refit");
  PL_REQUIRE_LIST("cloud_planes_refit");
  PL_REQUIRE_TOL("cloud_planes_refit");
  MSLAM_REQUIRE(iterations >= 0 && iterations <= 64, "cloud_planes_refit: iterations must be in [0, 64]");
  MSLAM_REQUIRE(fit && (num_remaining == 0 || partial), "cloud_planes_refit: null pointer");
  MSLAM_REQUIRE(PL_ALIGNED(fit, 8) && PL_ALIGNED(partial, 8), "cloud_planes_refit: misaligned pointer");
  const PlArgs a = {points, normals, num_points, tol, cos_angle, (hipStream_t)stream};
  return pl_refit(a, remaining, num_remaining, iterations, partial, state, fit);
}

extern "C" int mslam_cloud_planes_label(const float* points, const float* normals, int num_points,
                                        const int32_t* remaining, int num_remaining, double tol, double cos_angle,
                                        const float* viewpoint, const double* fit, int max_planes, int32_t* state,
                                        int32_t* labels, double* planes, void* stream) {
  PL_REQUIRE_CLOUD("cloud_planes_label");
  PL_REQUIRE_LIST("cloud_planes_label");
  PL_REQUIRE_TOL("cloud_planes_label");
  MSLAM_REQUIRE(max_planes >= 1 && max_planes <= MSLAM_CLOUD_PLANES_MAX_PLANES,
                "cloud_planes_label: max_planes must be in [1, %d], got %d", MSLAM_CLOUD_PLANES_MAX_PLANES, max_planes);
  MSLAM_REQUIRE(fit && planes && (num_remaining == 0 || labels), "cloud_planes_label: null pointer");
  MSLAM_REQUIRE(PL_ALIGNED(fit, 8) && PL_ALIGNED(planes, 8) && PL_ALIGNED(labels, 4) && PL_ALIGNED(viewpoint, 4),
                "cloud_planes_label: misaligned pointer");
  const PlArgs a = {points, normals, num_points, tol, cos_angle, (hipStream_t)stream};
  return pl_label(a, remaining, num_remaining, viewpoint, fit, max_planes, state, labels, planes);
}

extern "C" size_t mslam_cloud_planes_workspace_bytes(int num_points, int num_hypotheses) {
  if (num_points < 0 || num_hypotheses < 1 || num_hypotheses > MSLAM_CLOUD_PLANES_MAX_HYPOTHESES) return 0;
  return PlWorkspace(num_points, num_hypotheses).bytes;
}

extern "C" int mslam_cloud_planes(const float* points, const float* normals, int num_points, double tol,
                                  double cos_angle, int max_planes, int min_points, int num_hypotheses,
                                  int refit_iterations, uint64_t seed, const float* viewpoint, void* workspace,
                                  size_t workspace_bytes, int32_t* labels, double* planes, int32_t* state,
                                  void* stream) {
  PL_REQUIRE_CLOUD("cloud_planes");
  PL_REQUIRE_HYP("cloud_planes");
  PL_REQUIRE_TOL("cloud_planes");
  MSLAM_REQUIRE(max_planes >= 1 && max_planes <= MSLAM_CLOUD_PLANES_MAX_PLANES,
                "cloud_planes: max_planes must be in [1, %d], got %d", MSLAM_CLOUD_PLANES_MAX_PLANES, max_planes);
  MSLAM_REQUIRE(min_points >= 1, "cloud_planes: min_points must be >= 1, got %d", min_points);
  MSLAM_REQUIRE(refit_iterations >= 0 && refit_iterations <= 64, "cloud_planes: refit_iterations must be in [0, 64]");
  const PlWorkspace ws(num_points, num_hypotheses);
  MSLAM_REQUIRE(workspace, "cloud_planes: null pointer");
  if (workspace_bytes < ws.bytes) return md_too_small("cloud_planes", "workspace", workspace_bytes, ws.bytes);
  MSLAM_REQUIRE(planes && state && (num_points == 0 || labels), "cloud_planes: null pointer");
  MSLAM_REQUIRE(PL_ALIGNED(workspace, 16) && PL_ALIGNED(labels, 4) && PL_ALIGNED(planes, 8) && PL_ALIGNED(state, 4) &&
                    PL_ALIGNED(viewpoint, 4), "cloud_planes: misaligned pointer");
  const hipStream_t st = (hipStream_t)stream;
  char* w = (char*)workspace;
  double *fit = (double*)(w + ws.fit), *hyp = (double*)(w + ws.hyp), *partial = (double*)(w + ws.partial);
  int32_t *block_offset = (int32_t*)(w + ws.block_offset), *rem = (int32_t*)(w + ws.rem);
  int32_t *triples = (int32_t*)(w + ws.triples), *count = (int32_t*)(w + ws.count);
  if (int rc = check_hip(hipMemsetAsync(state, 0, sizeof(int32_t) * MSLAM_CLOUD_PLANES_STATE, st), "cloud_planes"))
    return rc;
  if (int rc = check_hip(hipMemsetAsync(fit, 0, sizeof(double) * MSLAM_CLOUD_PLANES_FIT, st), "cloud_planes")) return rc;
  if (num_points == 0) return MSLAM_OK;
  if (int rc = check_hip(hipMemsetAsync(labels, 0xFF, sizeof(int32_t) * (size_t)num_points, st), "cloud_planes"))
    return rc;
  const PlArgs a = {points, normals, num_points, tol, cos_angle, st};
  for (int round = 0; round < max_planes; round++) {
    if (int rc = pl_remaining(a, labels, min_points, block_offset, rem, state)) return rc;
    if (int rc = pl_draw(a, rem, num_points, state, seed, round, num_hypotheses, hyp, triples)) return rc;
    if (int rc = pl_count(a, rem, num_points, state, hyp, num_hypotheses, count)) return rc;
    if (int rc = pl_select(a, count, num_hypotheses, min_points, hyp, triples, state, fit)) return rc;
    if (int rc = pl_refit(a, rem, num_points, refit_iterations, partial, state, fit)) return rc;
    if (int rc = pl_label(a, rem, num_points, viewpoint, fit, max_planes, state, labels, planes)) return rc;
  }
  return MSLAM_OK;
}
