// Mesh alignment: the closed-form similarity (Sim3) between corresponding points and trimmed point-to-mesh ICP.
// Semantics in DESIGN.md "Mesh alignment"; tests/meshalign_numpy.py states the same definitions in numpy.  All arithmetic
// is f64 on the f32 inputs without contraction.  No atomics: every sum is reduced in a fixed order (a shuffle tree in
// the wave, the four waves of a block in wave order, the block partials ascending per lane of one wave, then a shuffle
// tree), so the same inputs give the same bits.
//
// The state is a device block of MSLAM_MESH_ALIGN_STATE_BYTES: f64 Sim3 [t(3), q(xyzw), s] in lietorch layout and an
// int32 status (MSLAM_MESH_ALIGN_OK / _DEGENERATE).  One ICP iteration is ma_step_kernel (transform, match, closest
// point, moments) followed by ma_solve_kernel (Horn's quaternion solve for the TOTAL transform from the original
// points: T_{k+1} replaces T_k, nothing is composed).
//
// The match is md_scan of mesh_tri.h, the culled nearest-face scan that md_distance_kernel calls too, on
// q_i = (float)(T_k p_i).  The boxes are computed once per alignment (mslam_mesh_align_init), and lane i's bound starts
// from md_dist2(q_i, face nearest_prev[i]) when that face exists and is valid, so a block stages its home tile only
// when one of its lanes has no such face.  The _indexed entries run the same step over the tiles of a mesh index
// (mesh_index.hip); the warm start is by original face index and does not change.
#include "mesh_align.h"

namespace mslam {

constexpr int kMaSums = 19;        // count, sum w, sum w p (3), sum w c (3), sum w p c^T (9), sum w |p|^2, sum w dist2
constexpr int kMaLog = MSLAM_MESH_ALIGN_LOG_DOUBLES;
static_assert(MSLAM_MESH_ALIGN_STATE_BYTES == 9 * sizeof(double), "eight doubles, then the status in a slot of its own");
static_assert(kMaLog >= 4 + kMaSums, "a log row holds four figures and the sums");

// The moment terms of one pair about the origins op (source side) and oc (target side), weight w; `in` false: zeros.
__device__ __forceinline__ void ma_terms(bool in, double w, const double* p, const double* c, const double* op,
                                         const double* oc, double d2, double* v) {
#pragma unroll
  for (int k = 0; k < kMaSums; k++) v[k] = 0.0;
  if (!in) return;
  const double a[3] = {p[0] - op[0], p[1] - op[1], p[2] - op[2]};
  const double b[3] = {c[0] - oc[0], c[1] - oc[1], c[2] - oc[2]};
  v[0] = 1.0;
  v[1] = w;
#pragma unroll
  for (int d = 0; d < 3; d++) {
    v[2 + d] = w * a[d];
    v[5 + d] = w * b[d];
#pragma unroll
    for (int e = 0; e < 3; e++) v[8 + 3 * d + e] = w * (a[d] * b[e]);
  }
  v[17] = w * md_dot(a[0], a[1], a[2], a[0], a[1], a[2]);
  v[18] = w * d2;
}

// count: also write, per wave, how many tiles it did not scan to skipped[4 * block + wave] (the timing tool's figure).
// kIndexed: the tiles follow `order`, `gbox` holds the group boxes (mesh_tri.h); without it neither is read.
template <bool kIndexed>
__global__ __launch_bounds__(kMdBlock) void ma_step_kernel(const float* __restrict__ src, int n,
                                                           const float* __restrict__ vert,
                                                           const int32_t* __restrict__ faces, int nf, int nv,
                                                           const double* __restrict__ state, int cull,
                                                           const double* __restrict__ box,
                                                           const int32_t* __restrict__ order,
                                                           const double* __restrict__ gbox, double trim2,
                                                           int32_t* __restrict__ skipped, int32_t* __restrict__ nearest,
                                                           float* __restrict__ moved, double* __restrict__ dist2,
                                                           double* __restrict__ closest,
                                                           double* __restrict__ partial) {
  __shared__ double s_tri[kMdTile * kMdTriDoubles];
  __shared__ double s_part[4 * kMaSums];
  __shared__ int s_home;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const size_t i0 = (size_t)blockIdx.x * kMdBlock, i = i0 + tid;
  const bool has = i < (size_t)n;

  // 1. the transform, rounded to f32 once; y0: the block's first point
  double R[9], tt[3], p[3] = {0.0, 0.0, 0.0}, op[3], oc[3], y[3], p0[3], y0[3];
  ma_quat_to_mat(state + 3, R);
  const double s = state[7];
#pragma unroll
  for (int d = 0; d < 3; d++) tt[d] = state[d], op[d] = (double)src[d], p0[d] = (double)src[3 * i0 + d];
  ma_act(R, tt, s, op, oc);
  ma_act(R, tt, s, p0, y0);
  if (has) {
#pragma unroll
    for (int d = 0; d < 3; d++) p[d] = (double)src[3 * i + d];
  }
  ma_act(R, tt, s, p, y);
  const float qf[3] = {(float)y[0], (float)y[1], (float)y[2]};
  const double px = (double)qf[0], py = (double)qf[1], pz = (double)qf[2];

  // 2. the nearest face; the bound starts from last iteration's face where there is one
  double ub = INFINITY;
  bool warm = false;
  if (cull && has) {
    const int wf = nearest[i];
    double t[kMdTriDoubles];
    if ((unsigned)wf < (unsigned)nf && md_load_tri(vert, faces, wf, nf, nv, t)) {
      ub = fmin(ub, md_dist2(px, py, pz, t));                        // fmin: a NaN distance never becomes the bound
      warm = true;
    }
  }
  const MdNearest r = md_scan<MdTri, kIndexed>(px, py, pz, has, (double)(float)y0[0], (double)(float)y0[1],
                                               (double)(float)y0[2], {vert, faces, nf, nv}, cull, box, s_tri, &s_home, ub,
                                               !warm, order, gbox);
  const double best = r.dist2;
  const int best_f = r.face;

  // 3. the closest point on the nearest face, and whether the pair counts
  double c[3] = {NAN, NAN, NAN};
  if (has && best_f >= 0) {
    double t[kMdTriDoubles];
    md_load_tri(vert, faces, best_f, nf, nv, t);
    md_closest(px, py, pz, t, c);
  }
  const bool inlier = has && best_f >= 0 && best <= trim2;
  if (has) {
#pragma unroll
    for (int d = 0; d < 3; d++) {
      moved[3 * i + d] = qf[d];
      if (closest) closest[3 * i + d] = c[d];
    }
    dist2[i] = best;
    nearest[i] = best_f;
  }
  if (skipped && lane == 0) skipped[4 * (size_t)blockIdx.x + wave] = r.skipped;

  // 4., 5. the moments about (p_0, T_k p_0), reduced in a fixed order
  double v[kMaSums];
  ma_terms(inlier, 1.0, p, c, op, oc, best, v);
  ma_block_reduce<kMaSums>(v, s_part, partial);
}

// Explicit pairs src[i] -> dst[i] with optional weights >= 0 (a pair of weight 0 does not count); the moments about
// (src[0], dst[0]); dist2 is |dst - src|^2, the residual under the identity.
__global__ __launch_bounds__(kMdBlock) void ma_pairs_kernel(const float* __restrict__ src,
                                                            const float* __restrict__ dst,
                                                            const float* __restrict__ weights, int n,
                                                            double* __restrict__ partial) {
  __shared__ double s_part[4 * kMaSums];
  const size_t i = (size_t)blockIdx.x * kMdBlock + threadIdx.x;
  const bool has = i < (size_t)n;
  double p[3] = {0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0}, op[3], oc[3], w = 0.0;
#pragma unroll
  for (int d = 0; d < 3; d++) op[d] = (double)src[d], oc[d] = (double)dst[d];
  if (has) {
#pragma unroll
    for (int d = 0; d < 3; d++) p[d] = (double)src[3 * i + d], c[d] = (double)dst[3 * i + d];
    w = weights ? (double)weights[i] : 1.0;
  }
  const double rx = c[0] - p[0], ry = c[1] - p[1], rz = c[2] - p[2];
  double v[kMaSums];
  ma_terms(has && w > 0.0, w, p, c, op, oc, md_dot(rx, ry, rz, rx, ry, rz), v);
  ma_block_reduce<kMaSums>(v, s_part, partial);
}

// Largest eigenvalue's unit eigenvector of the symmetric 4x4 A (destroyed) by cyclic Jacobi; one thread.
__host__ __device__ inline void ma_jacobi4(double A[4][4], double* evec) {
  double V[4][4];
  for (int a = 0; a < 4; a++)
    for (int b = 0; b < 4; b++) V[a][b] = a == b ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 32; sweep++) {
    double off = 0.0, diag = 0.0;
    for (int a = 0; a < 4; a++)
      for (int b = 0; b < 4; b++) (a == b ? diag : off) += A[a][b] * A[a][b];
    if (!(off > 0x1p-104 * diag)) break;                         // off-diagonal norm below 2^-52 of the diagonal's
    for (int p = 0; p < 3; p++) {
      for (int q = p + 1; q < 4; q++) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
        for (int k = 0; k < 4; k++) {                              // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = cs * akp - sn * akq;
          A[k][q] = sn * akp + cs * akq;
        }
        for (int k = 0; k < 4; k++) {                              // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = cs * apk - sn * aqk;
          A[q][k] = sn * apk + cs * aqk;
        }
        for (int k = 0; k < 4; k++) {                              // V <- V J
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = cs * vkp - sn * vkq;
          V[k][q] = sn * vkp + cs * vkq;
        }
      }
    }
  }
  int m = 0;
  for (int a = 1; a < 4; a++)
    if (A[a][a] > A[m][m]) m = a;
  double n2 = 0.0;
  for (int a = 0; a < 4; a++) n2 += V[a][m] * V[a][m];
  const double inv = 1.0 / sqrt(n2);
  for (int a = 0; a < 4; a++) evec[a] = V[a][m] * inv;
}

// The weighted Umeyama problem from the sums (about the origins op, oc): Horn's quaternion for the rotation,
// s = tr(R M) / sum w |p - pm|^2 (1 without with_scale), t = cm - s R pm, for the TOTAL transform from the original
// points -> T[8].  false (T untouched): fewer than 3 pairs, no source spread, or no positive finite scale.
__host__ __device__ inline bool ma_solve(const double* sum, const double* op, const double* oc, int with_scale,
                                         double* T) {
  const double count = sum[0], W = sum[1];
  if (!(count >= 3.0 && W > 0.0)) return false;
  double pm[3], cm[3], S[3][3], R[9];
  for (int d = 0; d < 3; d++) pm[d] = sum[2 + d] / W, cm[d] = sum[5 + d] / W;
  for (int d = 0; d < 3; d++)
    for (int e = 0; e < 3; e++) S[d][e] = sum[8 + 3 * d + e] - W * (pm[d] * cm[e]);       // sum w (p - pm)(c - cm)^T
  const double spread = sum[17] - W * ((pm[0] * pm[0] + pm[1] * pm[1]) + pm[2] * pm[2]);
  double big = 0.0;
  for (int d = 0; d < 3; d++)
    for (int e = 0; e < 3; e++) big = fmax(big, fabs(S[d][e]));
  if (!(spread > 0.0 && big < INFINITY)) return false;
  const double k = big > 0.0 ? 1.0 / big : 1.0;                     // Horn's matrix of S / max|S|, in (w, x, y, z) order
  const double xx = S[0][0] * k, xy = S[0][1] * k, xz = S[0][2] * k, yx = S[1][0] * k, yy = S[1][1] * k,
               yz = S[1][2] * k, zx = S[2][0] * k, zy = S[2][1] * k, zz = S[2][2] * k;
  double N[4][4] = {{(xx + yy) + zz, yz - zy, zx - xz, xy - yx},
                    {yz - zy, (xx - yy) - zz, xy + yx, zx + xz},
                    {zx - xz, xy + yx, (yy - xx) - zz, yz + zy},
                    {xy - yx, zx + xz, yz + zy, (zz - xx) - yy}};
  double e[4];
  ma_jacobi4(N, e);
  if (e[0] < 0.0) e[0] = -e[0], e[1] = -e[1], e[2] = -e[2], e[3] = -e[3];
  const double q[4] = {e[1], e[2], e[3], e[0]};
  ma_quat_to_mat(q, R);
  double tr = 0.0;                                                   // sum w (R (p - pm)) . (c - cm)
  for (int d = 0; d < 3; d++)
    for (int f = 0; f < 3; f++) tr += R[3 * d + f] * S[f][d];
  const double sc = with_scale ? tr / spread : 1.0;
  if (!(sc > 0.0 && sc < INFINITY)) return false;
  double pbar[3], rp[3];
  const double zero[3] = {0.0, 0.0, 0.0};
  for (int d = 0; d < 3; d++) pbar[d] = op[d] + pm[d];
  ma_act(R, zero, sc, pbar, rp);
  for (int d = 0; d < 3; d++) T[d] = (oc[d] + cm[d]) - rp[d];
  for (int d = 0; d < 4; d++) T[3 + d] = q[d];
  T[7] = sc;
  return true;
}

// One wave.  The origins the partials were formed about are src[0] and either T_k src[0] (dst == nullptr) or dst[0].
// Sums the partials, solves, writes the state (unless degenerate) and the log row
// [inliers, rmse at T_k, scale after the solve, status, the kMaSums sums].
__global__ __launch_bounds__(kWave) void ma_solve_kernel(const double* __restrict__ partial, int nblocks,
                                                         const float* __restrict__ src,
                                                         const float* __restrict__ dst, int n, int with_scale,
                                                         double* __restrict__ state, double* __restrict__ log_row) {
  const int lane = threadIdx.x;
  double sum[kMaSums];
#pragma unroll
  for (int k = 0; k < kMaSums; k++) {
    double x = 0.0;
    for (int b = lane; b < nblocks; b += kWave) x += partial[kMaSums * (size_t)b + k];
    sum[k] = wave_sum(x);
  }
  if (lane != 0) return;
  int status = MSLAM_MESH_ALIGN_DEGENERATE;
  if (n > 0) {
    double R[9], tt[3], op[3], oc[3], T[8];
#pragma unroll
    for (int d = 0; d < 3; d++) tt[d] = state[d], op[d] = (double)src[d];
    if (dst) {
#pragma unroll
      for (int d = 0; d < 3; d++) oc[d] = (double)dst[d];
    } else {
      ma_quat_to_mat(state + 3, R);
      ma_act(R, tt, state[7], op, oc);
    }
    if (ma_solve(sum, op, oc, with_scale, T)) {
      for (int k = 0; k < 8; k++) state[k] = T[k];
      status = MSLAM_MESH_ALIGN_OK;
    }
  }
  *(int32_t*)(state + 8) = status;
  log_row[0] = sum[0];
  log_row[1] = sum[1] > 0.0 ? sqrt(sum[18] / sum[1]) : INFINITY;
  log_row[2] = state[7];
  log_row[3] = (double)status;
#pragma unroll
  for (int k = 0; k < kMaSums; k++) log_row[4 + k] = sum[k];
  for (int k = 4 + kMaSums; k < kMaLog; k++) log_row[k] = 0.0;
}

// T0 f32[8] (or nullptr: the identity) -> the state, its quaternion normalised in f64
__global__ void ma_init_kernel(const float* __restrict__ T0, double* __restrict__ state) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double T[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0};
  if (T0) {
    for (int k = 0; k < 8; k++) T[k] = (double)T0[k];
    const double inv = 1.0 / sqrt((T[3] * T[3] + T[4] * T[4]) + (T[5] * T[5] + T[6] * T[6]));
    for (int k = 3; k < 7; k++) T[k] *= inv;
  }
  for (int k = 0; k < 8; k++) state[k] = T[k];
  int32_t* w = (int32_t*)(state + 8);
  w[0] = MSLAM_MESH_ALIGN_OK;
  w[1] = 0;
}

__global__ void ma_read_kernel(const double* __restrict__ state, double* __restrict__ T64, float* __restrict__ T32,
                               int32_t* __restrict__ status) {
  const int k = threadIdx.x;
  if (k < 8) {
    if (T64) T64[k] = state[k];
    if (T32) T32[k] = (float)state[k];
  }
  if (k == 0 && status) *status = *(const int32_t*)(state + 8);
}

static size_t ma_partial_bytes(int n) { return (size_t)blocks_for(n, kMdBlock) * kMaSums * sizeof(double); }

}  // namespace mslam

using namespace mslam;

extern "C" size_t mslam_mesh_align_workspace_bytes(int n, int num_faces, int count_skips) {
  if (n < 0 || num_faces < 0) return 0;
  return md_box_bytes(num_faces) + ma_partial_bytes(n) + (count_skips ? md_count_bytes(n) : 0);
}

extern "C" int mslam_mesh_align_init(const float* T0, const float* vertices, const int32_t* faces, int num_faces,
                                     int num_vertices, void* workspace, size_t workspace_bytes, void* state,
                                     void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_align_init: negative size");
  MSLAM_REQUIRE(state, "mesh_align_init: null pointer");
  MSLAM_REQUIRE(num_faces == 0 || (faces && workspace && (vertices || num_vertices == 0)),
                "mesh_align_init: null pointer");
  if (workspace_bytes < md_box_bytes(num_faces))
    return md_too_small("mesh_align_init", "workspace", workspace_bytes, md_box_bytes(num_faces));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ma_init_kernel, dim3(1), dim3(kWave), 0, s, T0, (double*)state);
  if (num_faces > 0) md_launch_boxes<MdTri>({vertices, faces, num_faces, num_vertices}, nullptr, (double*)workspace, s);
  MSLAM_LAUNCH_CHECK("mesh_align_init");
  return MSLAM_OK;
}

// One ICP iteration; `order` null: the boxes lie at the head of the workspace (mslam_mesh_align_init), otherwise they
// are a mesh index's and the workspace starts with the partials.
static int ma_step(const char* what, const float* src, int n, const float* vertices, const int32_t* faces,
                   int num_faces, int num_vertices, const int32_t* order, const void* index, size_t index_bytes,
                   double trim, int with_scale, int count_skips, void* workspace, size_t workspace_bytes, void* state,
                   int32_t* nearest, float* moved, double* dist2, double* closest, double* log_row, void* stream) {
  const bool indexed = order != nullptr;
  const size_t box_bytes = indexed ? 0 : md_box_bytes(num_faces), part_bytes = ma_partial_bytes(n);
  const size_t need = box_bytes + part_bytes + (count_skips ? md_count_bytes(n) : 0);
  if (workspace_bytes < need) return md_too_small(what, "workspace", workspace_bytes, need);
  MdIndexArg ix;
  if (int rc = md_index_arg(what, num_faces, order, index, index_bytes, 2, &ix)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const unsigned nblocks = blocks_for(n, kMdBlock);
  double* partial = (double*)((char*)workspace + box_bytes);
  int32_t* skipped = count_skips ? (int32_t*)((char*)workspace + box_bytes + part_bytes) : nullptr;
  if (n > 0 && indexed)
    hipLaunchKernelGGL(ma_step_kernel<true>, dim3(nblocks), dim3(kMdBlock), 0, s, src, n, vertices, faces, num_faces,
                       num_vertices, (const double*)state, num_faces > 0 ? 1 : 0, ix.box, order, ix.gbox, trim * trim,
                       skipped, nearest, moved, dist2, closest, partial);
  else if (n > 0)
    hipLaunchKernelGGL(ma_step_kernel<false>, dim3(nblocks), dim3(kMdBlock), 0, s, src, n, vertices, faces, num_faces,
                       num_vertices, (const double*)state, num_faces > kMdTile ? 1 : 0, (const double*)workspace,
                       (const int32_t*)nullptr, (const double*)nullptr, trim * trim, skipped, nearest, moved, dist2,
                       closest, partial);
  hipLaunchKernelGGL(ma_solve_kernel, dim3(1), dim3(kWave), 0, s, (const double*)partial, (int)nblocks, src,
                     (const float*)nullptr, n, with_scale, (double*)state, log_row);
  return md_launched(what);
}

extern "C" int mslam_mesh_align_step(const float* src, int n, const float* vertices, const int32_t* faces,
                                     int num_faces, int num_vertices, double trim, int with_scale, int count_skips,
                                     void* workspace, size_t workspace_bytes, void* state, int32_t* nearest,
                                     float* moved, double* dist2, double* closest, double* log_row, void* stream) {
  MA_REQUIRE_STEP("mesh_align_step", n >= 0 && num_faces >= 0 && num_vertices >= 0);
  MSLAM_REQUIRE(num_faces == 0 || (faces && workspace && (vertices || num_vertices == 0)),
                "mesh_align_step: null pointer");
  return ma_step("mesh_align_step", src, n, vertices, faces, num_faces, num_vertices, nullptr, nullptr, 0, trim,
                 with_scale, count_skips, workspace, workspace_bytes, state, nearest, moved, dist2, closest, log_row,
                 stream);
}

extern "C" int mslam_mesh_align_init_indexed(const float* T0, void* state, void* stream) {
  MSLAM_REQUIRE(state, "mesh_align_init_indexed: null pointer");
  hipLaunchKernelGGL(ma_init_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, T0, (double*)state);
  MSLAM_LAUNCH_CHECK("mesh_align_init_indexed");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_align_step_indexed(const float* src, int n, const float* vertices, const int32_t* faces,
                                             int num_faces, int num_vertices, const int32_t* order, const void* index,
                                             size_t index_bytes, double trim, int with_scale, int count_skips,
                                             void* workspace, size_t workspace_bytes, void* state, int32_t* nearest,
                                             float* moved, double* dist2, double* closest, double* log_row,
                                             void* stream) {
  MA_REQUIRE_STEP("mesh_align_step_indexed", n >= 0 && num_faces >= 0 && num_vertices >= 0);
  MSLAM_REQUIRE(order, "mesh_align_step_indexed: null pointer");
  MSLAM_REQUIRE(num_faces == 0 || (faces && index && (vertices || num_vertices == 0)),
                "mesh_align_step_indexed: null pointer");
  return ma_step("mesh_align_step_indexed", src, n, vertices, faces, num_faces, num_vertices, order, index,
                 index_bytes, trim, with_scale, count_skips, workspace, workspace_bytes, state, nearest, moved, dist2,
                 closest, log_row, stream);
}

extern "C" int mslam_mesh_align_fit_pairs(const float* src, const float* dst, const float* weights, int n,
                                          int with_scale, void* workspace, size_t workspace_bytes, void* state,
                                          double* log_row, void* stream) {
  MSLAM_REQUIRE(n >= 0, "mesh_align_fit_pairs: negative size");
  MSLAM_REQUIRE(state && log_row, "mesh_align_fit_pairs: null pointer");
  MSLAM_REQUIRE(n == 0 || (src && dst && workspace), "mesh_align_fit_pairs: null pointer");
  const size_t need = ma_partial_bytes(n);
  if (workspace_bytes < need) return md_too_small("mesh_align_fit_pairs", "workspace", workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const unsigned nblocks = blocks_for(n, kMdBlock);
  hipLaunchKernelGGL(ma_init_kernel, dim3(1), dim3(kWave), 0, s, (const float*)nullptr, (double*)state);
  if (n > 0)
    hipLaunchKernelGGL(ma_pairs_kernel, dim3(nblocks), dim3(kMdBlock), 0, s, src, dst, weights, n,
                       (double*)workspace);
  hipLaunchKernelGGL(ma_solve_kernel, dim3(1), dim3(kWave), 0, s, (const double*)workspace, (int)nblocks, src, dst, n,
                     with_scale, (double*)state, log_row);
  MSLAM_LAUNCH_CHECK("mesh_align_fit_pairs");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_align_read(const void* state, double* T64, float* T32, int32_t* status, void* stream) {
  MSLAM_REQUIRE(state, "mesh_align_read: null pointer");
  hipLaunchKernelGGL(ma_read_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, (const double*)state, T64, T32,
                     status);
  MSLAM_LAUNCH_CHECK("mesh_align_read");
  return MSLAM_OK;
}
