// Point-to-plane ICP for clouds and meshes: one fused step per iteration and a Gauss-Newton solve on Sim3.  Semantics in
// DESIGN.md "Point-to-plane ICP"; tests/icp_plane_numpy.py states the same definitions, operation by operation, in
// numpy.  All arithmetic is f64 on the f32 inputs without contraction.  No atomics: every sum is reduced in the fixed
// order of mesh_align.hip (a shuffle tree in the wave, the four waves of a block in wave order, the block partials
// ascending per lane of one wave, then a shuffle tree), so the same inputs give the same bits.
//
// The state block, its init and its read are mesh_align.hip's (mslam_mesh_align_init*, mslam_mesh_align_read).  One
// iteration is ip_step_kernel followed by ip_solve_kernel.
//
//   pair      q_i = (float)(T_k p_i), used in f64 from there on.  Its nearest primitive comes from md_scan of mesh_tri.h
//             exactly as cd_distance_kernel (MdPoint) and ma_step_kernel (MdTri, warm-started from last iteration's face)
//             call it.  c_i: the nearest point itself, or md_closest on the nearest face.  n_i: the given f32 normal of
//             the nearest point as it is, or ((b - a) x (c - a)) / its length of the nearest face.  Its sign is free.
//   inlier    a neighbour, dist2 <= trim^2, and a finite non-zero n_i - with point_weight > 0 a pair without a normal
//             stays and contributes its point rows alone.
//   rows      about o = q_0: a = q - o, e = q - c.  Plane: r = n . e, J = [n, a x n, n . a] in the order (tau, omega,
//             sigma).  Point, weight alpha = point_weight, per axis d: r_d = e_d, J_d = [u_d, a x u_d, a_d].
//   sums      kIpSums = 39: count, sum w, sum r^2, sum dist2, g = sum J^T r (7), H = sum J^T J (upper triangle row by
//             row, 28).
//   solve     H scaled to unit diagonal, Cholesky, H xi = -g; with_scale = 0 drops sigma.  Degenerate (state untouched):
//             fewer inliers than unknowns, a zero or non-finite diagonal entry, a pivot of the scaled matrix <= 2^-40, a
//             non-finite xi or scale.
//   update    x -> o + e^sigma R(omega) (x - o) + tau composed onto T_k.
#include "cloud_point.h"
#include "jacobi3.h"
#include "mesh_align.h"

namespace mslam {

constexpr int kIpSums = MSLAM_ICP_PLANE_SUMS;
constexpr int kIpLog = MSLAM_ICP_PLANE_LOG_DOUBLES;
constexpr int kIpG = 4, kIpH = 11;                  // where g and H begin among the sums
static_assert(kIpSums == 4 + 7 + 28, "count, sum w, sum r^2, sum dist2, g, the upper triangle of H");
static_assert(kIpLog == 6 + kIpSums, "a log row holds six figures and the sums");

// The moved first sample, the origin of the rows: T src[0] rounded to f32
__device__ __forceinline__ void ip_origin(const double* R, const double* t, double s, const float* __restrict__ src,
                                          double* o) {
  const double p0[3] = {(double)src[0], (double)src[1], (double)src[2]};
  double y[3];
  ma_act(R, t, s, p0, y);
#pragma unroll
  for (int d = 0; d < 3; d++) o[d] = (double)(float)y[d];
}

// The closest point c and the normal nrm of primitive `best` to q.  MdPoint: the point and its given normal.
__device__ __forceinline__ void ip_target(const MdPoint::Src tgt, const float* __restrict__ normals, int best,
                                          const double* q, double* c, double* nrm) {
#pragma unroll
  for (int d = 0; d < 3; d++) {
    c[d] = (double)tgt.points[3 * (size_t)best + d];
    nrm[d] = (double)normals[3 * (size_t)best + d];
  }
}

// MdTri: md_closest on the face and its plane's unit normal, ((b - a) x (c - a)) divided by its length
__device__ __forceinline__ void ip_target(const MdTri::Src tgt, const float* __restrict__, int best, const double* q,
                                          double* c, double* nrm) {
  double t[kMdTriDoubles];
  md_load_tri(tgt.vert, tgt.faces, best, tgt.nf, tgt.nv, t);
  md_closest(q[0], q[1], q[2], t, c);
  const double abx = t[3] - t[0], aby = t[4] - t[1], abz = t[5] - t[2];
  const double acx = t[6] - t[0], acy = t[7] - t[1], acz = t[8] - t[2];
  const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
  const double len = sqrt(md_dot(nx, ny, nz, nx, ny, nz));
  nrm[0] = nx / len, nrm[1] = ny / len, nrm[2] = nz / len;
}

// The lane's starting bound.  MdTri: last iteration's face when it exists and is valid (ma_step_kernel's warm start)
__device__ __forceinline__ bool ip_warm(const MdTri::Src tgt, int cull, bool has, const int32_t* __restrict__ nearest,
                                        size_t i, const double* q, double* ub) {
  if (!(cull && has)) return false;
  const int wf = nearest[i];
  double t[kMdTriDoubles];
  if ((unsigned)wf < (unsigned)tgt.nf && md_load_tri(tgt.vert, tgt.faces, wf, tgt.nf, tgt.nv, t)) {
    *ub = fmin(*ub, md_dist2(q[0], q[1], q[2], t));                  // fmin: a NaN distance never becomes the bound
    return true;
  }
  return false;
}

// MdPoint: none, as cd_distance_kernel
__device__ __forceinline__ bool ip_warm(const MdPoint::Src, int, bool, const int32_t* __restrict__, size_t,
                                        const double*, double*) {
  return false;
}

// Whether the moved sample can have a neighbour at all.  MdPoint: its coordinates are finite (cd_distance_kernel's rule);
// MdTri: always, a NaN distance never beats the best (ma_step_kernel's rule)
__device__ __forceinline__ bool ip_query_ok(const MdPoint::Src, const float* qf) { return cd_finite(qf[0], qf[1], qf[2]); }
__device__ __forceinline__ bool ip_query_ok(const MdTri::Src, const float*) { return true; }

// H[j][k], j <= k, among the sums: the upper triangle row by row
__host__ __device__ constexpr int ip_h(int j, int k) { return kIpH + 7 * j - j * (j - 1) / 2 + (k - j); }

// The terms of one pair -> v[kIpSums]; `in` false: zeros.  nrm: zeros for a pair without a normal.
__device__ __forceinline__ void ip_terms(bool in, const double* q, const double* c, const double* nrm, const double* o,
                                         double alpha, double d2, double* v) {
#pragma unroll
  for (int k = 0; k < kIpSums; k++) v[k] = 0.0;
  if (!in) return;
  const double a[3] = {q[0] - o[0], q[1] - o[1], q[2] - o[2]};
  const double e[3] = {q[0] - c[0], q[1] - c[1], q[2] - c[2]};
  const double r = (nrm[0] * e[0] + nrm[1] * e[1]) + nrm[2] * e[2];
  const double J[7] = {nrm[0], nrm[1], nrm[2], a[1] * nrm[2] - a[2] * nrm[1], a[2] * nrm[0] - a[0] * nrm[2],
                       a[0] * nrm[1] - a[1] * nrm[0], (nrm[0] * a[0] + nrm[1] * a[1]) + nrm[2] * a[2]};
  // the point rows: [u_d, a x u_d, a_d]
  const double P[3][7] = {{1.0, 0.0, 0.0, 0.0, a[2], -a[1], a[0]},
                          {0.0, 1.0, 0.0, -a[2], 0.0, a[0], a[1]},
                          {0.0, 0.0, 1.0, a[1], -a[0], 0.0, a[2]}};
  v[0] = 1.0;
  v[1] = 1.0;
  v[2] = r * r;
  v[3] = d2;
#pragma unroll
  for (int j = 0; j < 7; j++) {
    v[kIpG + j] = J[j] * r + alpha * ((P[0][j] * e[0] + P[1][j] * e[1]) + P[2][j] * e[2]);
#pragma unroll
    for (int k = j; k < 7; k++)
      v[ip_h(j, k)] = J[j] * J[k] + alpha * ((P[0][j] * P[0][k] + P[1][j] * P[1][k]) + P[2][j] * P[2][k]);
  }
}

// One sample per thread.  kIndexed: the tiles follow `order`, `gbox` (may be null: tiles alone) holds the group boxes
// (mesh_tri.h); without it neither is read.  normals: MdPoint alone.
template <class Prim, bool kIndexed>
__global__ __launch_bounds__(kMdBlock) void ip_step_kernel(const float* __restrict__ src, int n,
                                                           const typename Prim::Src tgt,
                                                           const float* __restrict__ normals,
                                                           const double* __restrict__ state, int cull,
                                                           const double* __restrict__ box,
                                                           const int32_t* __restrict__ order,
                                                           const double* __restrict__ gbox, double trim2, double alpha,
                                                           int32_t* __restrict__ nearest, float* __restrict__ moved,
                                                           double* __restrict__ dist2, double* __restrict__ closest,
                                                           double* __restrict__ partial) {
  __shared__ double s_tile[kMdTile * Prim::kDoubles];
  __shared__ double s_part[4 * kIpSums];
  __shared__ int s_home;
  const int tid = threadIdx.x;
  const size_t i0 = (size_t)blockIdx.x * kMdBlock, i = i0 + tid;
  const bool in_range = i < (size_t)n;

  // 1. the transform, rounded to f32 once; y0: the block's first point; o: the moved first sample
  double R[9], tt[3], p[3] = {0.0, 0.0, 0.0}, p0[3], y[3], y0[3], o[3];
  ma_quat_to_mat(state + 3, R);
  const double s = state[7];
#pragma unroll
  for (int d = 0; d < 3; d++) tt[d] = state[d], p0[d] = (double)src[3 * i0 + d];
  ip_origin(R, tt, s, src, o);
  ma_act(R, tt, s, p0, y0);
  if (in_range) {
#pragma unroll
    for (int d = 0; d < 3; d++) p[d] = (double)src[3 * i + d];
  }
  ma_act(R, tt, s, p, y);
  const float qf[3] = {(float)y[0], (float)y[1], (float)y[2]};
  const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
  const bool has = in_range && ip_query_ok(tgt, qf);

  // 2. the nearest primitive
  double ub = INFINITY;
  const bool warm = ip_warm(tgt, cull, has, nearest, i, q, &ub);
  const MdNearest r = md_scan<Prim, kIndexed>(q[0], q[1], q[2], has, (double)(float)y0[0], (double)(float)y0[1],
                                              (double)(float)y0[2], tgt, cull, box, s_tile, &s_home, ub, !warm, order,
                                              gbox);
  const double best = has ? r.dist2 : INFINITY;
  const int best_f = has ? r.face : -1;

  // 3. the closest point, the normal, and whether the pair counts
  double c[3] = {NAN, NAN, NAN}, nrm[3] = {0.0, 0.0, 0.0};
  if (best_f >= 0) ip_target(tgt, normals, best_f, q, c, nrm);
  const bool with_normal = isfinite(nrm[0]) && isfinite(nrm[1]) && isfinite(nrm[2]) &&
                           (nrm[0] != 0.0 || nrm[1] != 0.0 || nrm[2] != 0.0);
  if (!with_normal) nrm[0] = nrm[1] = nrm[2] = 0.0;
  const bool inlier = best_f >= 0 && best <= trim2 && (with_normal || alpha > 0.0);
  if (in_range) {
#pragma unroll
    for (int d = 0; d < 3; d++) {
      moved[3 * i + d] = qf[d];
      if (closest) closest[3 * i + d] = c[d];
    }
    dist2[i] = best;
    nearest[i] = best_f;
  }

  // 4. the terms about o, formed only now so that they do not live across the scan, reduced in a fixed order
  double v[kIpSums];
  ip_terms(inlier, q, c, nrm, o, alpha, best, v);
  ma_block_reduce<kIpSums>(v, s_part, partial);
}

// One lane: xi[nu] of H xi = -g from the sums, H scaled to unit diagonal, by Cholesky.  false: degenerate.  Every loop
// has constant bounds and is unrolled, so H and L are registers.
template <int nu>
__device__ __forceinline__ bool ip_solve(const double* sum, double* xi) {
  if (!(sum[0] >= (double)nu)) return false;
  double sc[nu], L[nu][nu], yv[nu];
#pragma unroll
  for (int j = 0; j < nu; j++) {
    const double d = sum[ip_h(j, j)];
    if (!(d > 0.0 && d < INFINITY)) return false;
    sc[j] = 1.0 / sqrt(d);
  }
#pragma unroll
  for (int j = 0; j < nu; j++) {
    double pv = (sum[ip_h(j, j)] * sc[j]) * sc[j];
#pragma unroll
    for (int k = 0; k < j; k++) pv -= L[j][k] * L[j][k];
    if (!(pv > 0x1p-40)) return false;                       // NaN fails too
    const double l = sqrt(pv);
    L[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < nu; i++) {
      double x = (sum[ip_h(j, i)] * sc[i]) * sc[j];
#pragma unroll
      for (int k = 0; k < j; k++) x -= L[i][k] * L[j][k];
      L[i][j] = x / l;
    }
  }
#pragma unroll
  for (int j = 0; j < nu; j++) {                             // L y = -(g scaled)
    double x = -(sum[kIpG + j] * sc[j]);
#pragma unroll
    for (int k = 0; k < j; k++) x -= L[j][k] * yv[k];
    yv[j] = x / L[j][j];
  }
#pragma unroll
  for (int j = nu - 1; j >= 0; j--) {                        // L^T z = y; xi holds z, unscaled, until the loop below
    double x = yv[j];
#pragma unroll
    for (int k = j + 1; k < nu; k++) x -= L[k][j] * xi[k];
    xi[j] = x / L[j][j];
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < nu; j++) {
    xi[j] = xi[j] * sc[j];
    ok = ok && isfinite(xi[j]);
  }
  return ok;
}

// T <- D o T for D: x -> o + e^sigma R(omega) (x - o) + tau.  false (T untouched): no positive finite scale.
__device__ inline bool ip_update(const double* xi, int with_scale, const double* o, double* T) {
  const double wx = xi[3], wy = xi[4], wz = xi[5];
  const double th2 = (wx * wx + wy * wy) + wz * wz;
  double A, B, hs, cw;                                       // sin th / th, (1 - cos th) / th^2, sin(th/2) / th, cos(th/2)
  if (th2 < 0x1p-26) {                                       // the series, whose next terms are below 2^-52 of the first
    A = 1.0 - th2 / 6.0;
    B = 0.5 - th2 / 24.0;
    hs = 0.5 - th2 / 48.0;
    cw = 1.0 - th2 / 8.0;
  } else {
    const double th = sqrt(th2), sh = sin(0.5 * th);
    A = sin(th) / th;
    B = (2.0 * (sh * sh)) / th2;
    hs = sh / th;
    cw = cos(0.5 * th);
  }
  const double Rd[9] = {1.0 + B * (wx * wx - th2), B * (wx * wy) - A * wz,    B * (wx * wz) + A * wy,
                        B * (wx * wy) + A * wz,    1.0 + B * (wy * wy - th2), B * (wy * wz) - A * wx,
                        B * (wx * wz) - A * wy,    B * (wy * wz) + A * wx,    1.0 + B * (wz * wz - th2)};
  const double es = with_scale ? exp(xi[6]) : 1.0;
  const double sn = es * T[7];
  if (!(sn > 0.0 && sn < INFINITY)) return false;
  const double dx = wx * hs, dy = wy * hs, dz = wz * hs, dw = cw;
  const double qx = T[3], qy = T[4], qz = T[5], qw = T[6];
  const double nx = ((dw * qx + dx * qw) + dy * qz) - dz * qy;
  const double ny = ((dw * qy - dx * qz) + dy * qw) + dz * qx;
  const double nz = ((dw * qz + dx * qy) - dy * qx) + dz * qw;
  const double nw = ((dw * qw - dx * qx) - dy * qy) - dz * qz;
  const double inv = 1.0 / sqrt((nx * nx + ny * ny) + (nz * nz + nw * nw));
  const double b[3] = {T[0] - o[0], T[1] - o[1], T[2] - o[2]};
  for (int d = 0; d < 3; d++)
    T[d] = (o[d] + es * ((Rd[3 * d] * b[0] + Rd[3 * d + 1] * b[1]) + Rd[3 * d + 2] * b[2])) + xi[d];
  T[3] = nx * inv, T[4] = ny * inv, T[5] = nz * inv, T[6] = nw * inv;
  T[7] = with_scale ? sn : T[7];
  return true;
}

// One wave.  Sums the partials, solves, updates the state (unless degenerate) and writes the log row
// [inliers, rms of the minimised residual, scale after the solve, status, point rmse, normal_spread, the kIpSums sums].
__global__ __launch_bounds__(kWave) void ip_solve_kernel(const double* __restrict__ partial, int nblocks,
                                                         const float* __restrict__ src, int n, int with_scale,
                                                         double alpha, double* __restrict__ state,
                                                         double* __restrict__ log_row) {
  const int lane = threadIdx.x;
  double sum[kIpSums];
#pragma unroll
  for (int k = 0; k < kIpSums; k++) {
    double x = 0.0;
    for (int b = lane; b < nblocks; b += kWave) x += partial[kIpSums * (size_t)b + k];
    sum[k] = wave_sum(x);
  }
  if (lane != 0) return;
  int status = MSLAM_MESH_ALIGN_DEGENERATE;
  if (n > 0) {
    double R[9], T[8], o[3], xi[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < 8; k++) T[k] = state[k];
    ma_quat_to_mat(T + 3, R);
    ip_origin(R, T, T[7], src, o);
    if ((with_scale ? ip_solve<7>(sum, xi) : ip_solve<6>(sum, xi)) && ip_update(xi, with_scale, o, T)) {
      for (int k = 0; k < 8; k++) state[k] = T[k];
      status = MSLAM_MESH_ALIGN_OK;
    }
  }
  *(int32_t*)(state + 8) = status;
  // the smallest eigenvalue of the translation block over sum w: how well the normals (and the point rows) span space
  double A[3][3] = {{sum[ip_h(0, 0)], sum[ip_h(0, 1)], sum[ip_h(0, 2)]},
                    {sum[ip_h(0, 1)], sum[ip_h(1, 1)], sum[ip_h(1, 2)]},
                    {sum[ip_h(0, 2)], sum[ip_h(1, 2)], sum[ip_h(2, 2)]}};
  double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  kn_jacobi3(A, V);
  const double lmin = fmin(fmin(A[0][0], A[1][1]), A[2][2]);
  const double W = sum[1];
  log_row[0] = sum[0];
  log_row[1] = W > 0.0 ? sqrt((sum[2] + alpha * sum[3]) / W) : INFINITY;
  log_row[2] = state[7];
  log_row[3] = (double)status;
  log_row[4] = W > 0.0 ? sqrt(sum[3] / W) : INFINITY;
  log_row[5] = W > 0.0 ? fmax(lmin, 0.0) / W : 0.0;
#pragma unroll
  for (int k = 0; k < kIpSums; k++) log_row[6 + k] = sum[k];
}

static size_t ip_partial_bytes(int n) { return (size_t)blocks_for(n, kMdBlock) * kIpSums * sizeof(double); }

// One iteration over the target `tgt`; box / gbox null: not read (cull 0, or tiles alone).
template <class Prim>
static int ip_step(const char* what, const float* src, int n, const typename Prim::Src tgt, const float* normals,
                   int cull, const double* box, const int32_t* order, const double* gbox, double trim,
                   double point_weight, int with_scale, double* partial, void* state, int32_t* nearest, float* moved,
                   double* dist2, double* closest, double* log_row, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const unsigned nblocks = blocks_for(n, kMdBlock);
  const auto kernel = order ? ip_step_kernel<Prim, true> : ip_step_kernel<Prim, false>;
  if (n > 0)
    hipLaunchKernelGGL(kernel, dim3(nblocks), dim3(kMdBlock), 0, s, src, n, tgt, normals, (const double*)state, cull,
                       box, order, gbox, trim * trim, point_weight, nearest, moved, dist2, closest, partial);
  hipLaunchKernelGGL(ip_solve_kernel, dim3(1), dim3(kWave), 0, s, (const double*)partial, (int)nblocks, src, n,
                     with_scale, point_weight, (double*)state, log_row);
  return md_launched(what);
}

}  // namespace mslam

using namespace mslam;

// the checks every step shares: mesh_align.h's, and the weight
#define IP_REQUIRE_STEP(what, sizes_ok) \
  MA_REQUIRE_STEP(what, sizes_ok);      \
  MSLAM_REQUIRE(point_weight >= 0.0 && point_weight < INFINITY, what ": point_weight must be finite and >= 0")

extern "C" size_t mslam_icp_plane_workspace_bytes(int n, int num_faces) {
  if (n < 0 || num_faces < 0) return 0;
  return md_box_bytes(num_faces) + ip_partial_bytes(n);
}

extern "C" int mslam_icp_plane_step_cloud(const float* src, int n, const float* points, const float* normals,
                                          int num_points, const int32_t* order, const void* index, size_t index_bytes,
                                          int levels, double trim, double point_weight, int with_scale,
                                          void* workspace, size_t workspace_bytes, void* state, int32_t* nearest,
                                          float* moved, double* dist2, double* closest, double* log_row,
                                          void* stream) {
  IP_REQUIRE_STEP("icp_plane_step_cloud", n >= 0 && num_points >= 0);
  if (int rc = md_levels_arg("icp_plane_step_cloud", levels)) return rc;
  MSLAM_REQUIRE(num_points == 0 || (points && normals), "icp_plane_step_cloud: null pointer");
  if (workspace_bytes < ip_partial_bytes(n))
    return md_too_small("icp_plane_step_cloud", "workspace", workspace_bytes, ip_partial_bytes(n));
  MdIndexArg ix;
  if (int rc = md_index_arg("icp_plane_step_cloud", num_points, order, index, index_bytes, levels, &ix)) return rc;
  return ip_step<MdPoint>("icp_plane_step_cloud", src, n, {points, num_points}, normals, ix.order ? 1 : 0, ix.box,
                          ix.order, ix.gbox, trim, point_weight, with_scale, (double*)workspace, state, nearest, moved,
                          dist2, closest, log_row, stream);
}

extern "C" int mslam_icp_plane_step_mesh(const float* src, int n, const float* vertices, const int32_t* faces,
                                         int num_faces, int num_vertices, double trim, double point_weight,
                                         int with_scale, void* workspace, size_t workspace_bytes, void* state,
                                         int32_t* nearest, float* moved, double* dist2, double* closest,
                                         double* log_row, void* stream) {
  IP_REQUIRE_STEP("icp_plane_step_mesh", n >= 0 && num_faces >= 0 && num_vertices >= 0);
  MSLAM_REQUIRE(num_faces == 0 || (faces && workspace && (vertices || num_vertices == 0)),
                "icp_plane_step_mesh: null pointer");
  const size_t need = md_box_bytes(num_faces) + ip_partial_bytes(n);
  if (workspace_bytes < need) return md_too_small("icp_plane_step_mesh", "workspace", workspace_bytes, need);
  return ip_step<MdTri>("icp_plane_step_mesh", src, n, {vertices, faces, num_faces, num_vertices}, nullptr,
                        num_faces > kMdTile ? 1 : 0, (const double*)workspace, nullptr, nullptr, trim, point_weight,
                        with_scale, (double*)((char*)workspace + md_box_bytes(num_faces)), state, nearest, moved, dist2,
                        closest, log_row, stream);
}

extern "C" int mslam_icp_plane_step_mesh_indexed(const float* src, int n, const float* vertices, const int32_t* faces,
                                                 int num_faces, int num_vertices, const int32_t* order,
                                                 const void* index, size_t index_bytes, double trim,
                                                 double point_weight, int with_scale, void* workspace,
                                                 size_t workspace_bytes, void* state, int32_t* nearest, float* moved,
                                                 double* dist2, double* closest, double* log_row, void* stream) {
  IP_REQUIRE_STEP("icp_plane_step_mesh_indexed", n >= 0 && num_faces >= 0 && num_vertices >= 0);
  MSLAM_REQUIRE(order, "icp_plane_step_mesh_indexed: null pointer");
  MSLAM_REQUIRE(num_faces == 0 || (faces && index && (vertices || num_vertices == 0)),
                "icp_plane_step_mesh_indexed: null pointer");
  if (workspace_bytes < ip_partial_bytes(n))
    return md_too_small("icp_plane_step_mesh_indexed", "workspace", workspace_bytes, ip_partial_bytes(n));
  MdIndexArg ix;
  if (int rc = md_index_arg("icp_plane_step_mesh_indexed", num_faces, order, index, index_bytes, 2, &ix)) return rc;
  // `order` itself, also over no faces: it selects the indexed kernel
  return ip_step<MdTri>("icp_plane_step_mesh_indexed", src, n, {vertices, faces, num_faces, num_vertices}, nullptr,
                        num_faces > 0 ? 1 : 0, ix.box, order, ix.gbox, trim, point_weight, with_scale,
                        (double*)workspace, state, nearest, moved, dist2, closest, log_row, stream);
}
