// Taubin lambda|mu smoothing of a welded triangle mesh, and vertex normals from the winding.  Semantics in DESIGN.md
// "Mesh smoothing"; tests/smooth_numpy.py states the same definitions, operation by operation, in numpy.  The state is
// f64, the build has -ffp-contract=off, so x + f * (S / n - x) below is four roundings, as in numpy.
//
//   edges    one thread per face: the six directed edge keys a * V + b of a counting face (indices in [0, V), pairwise
//            different), INT64_MAX in all six slots of any other face.
//   (caller)   sorts the keys; unique_consecutive with counts gives nbr = key % V, mult = the count (the number of
//            counting faces on that edge) and, by searchsorted, row_start: the neighbours of v, each once, ascending.
//   step     one thread per vertex, one Jacobi step x_out = x_in + f * (S / n - x_in): walks its row once and forms the
//            sum over all neighbours and the sum over the neighbours behind a boundary edge (mult == 1) side by side,
//            both in ascending neighbour index, then picks by the boundary mode.  A row has any length.
//   faces    one thread per face: the three (vertex, face) pair keys v * F + f of a counting face, INT64_MAX otherwise.
//   (caller)   sorts the pairs; searchsorted gives pair_start.
//   normals  one thread per vertex: the sum of (b - a) x (c - a) over its pairs' faces in ascending face index,
//            normalised; zero when the sum is zero or not finite; the input normal without a counting face.
// No atomics, and no thread reads what another writes within a launch: every sum has one fixed order, so the same input
// gives the same bits.  Every index read from memory is checked against its array before it is followed; an element
// that fails is skipped.
#include <math.h>

#include "mesh_topo.h"

namespace mslam {

constexpr int64_t kSmNone = INT64_MAX;

__global__ __launch_bounds__(256) void sm_edges_kernel(const int32_t* __restrict__ faces, int nf, int nv,
                                                       int64_t* __restrict__ keys) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
  const bool ok = tp_counts(a, b, c, nv);
  int64_t* k = keys + 6 * (size_t)f;
  k[0] = ok ? (int64_t)a * nv + b : kSmNone;
  k[1] = ok ? (int64_t)b * nv + a : kSmNone;
  k[2] = ok ? (int64_t)b * nv + c : kSmNone;
  k[3] = ok ? (int64_t)c * nv + b : kSmNone;
  k[4] = ok ? (int64_t)c * nv + a : kSmNone;
  k[5] = ok ? (int64_t)a * nv + c : kSmNone;
}

__global__ __launch_bounds__(256) void sm_faces_kernel(const int32_t* __restrict__ faces, int nf, int nv,
                                                       int64_t* __restrict__ pairs) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
  const bool ok = tp_counts(a, b, c, nv);
  pairs[3 * (size_t)f] = ok ? (int64_t)a * nf + f : kSmNone;
  pairs[3 * (size_t)f + 1] = ok ? (int64_t)b * nf + f : kSmNone;
  pairs[3 * (size_t)f + 2] = ok ? (int64_t)c * nf + f : kSmNone;
}

// STRIDE doubles per vertex: 3 packed, or 4 (x, y, z, 0) so that a neighbour is one aligned 32-byte read.
template <int STRIDE>
__device__ __forceinline__ void sm_load(const double* __restrict__ x, int64_t v, double (&p)[3]) {
  if (STRIDE == 4) {
    const double4 q = *reinterpret_cast<const double4*>(x + 4 * v);
    p[0] = q.x, p[1] = q.y, p[2] = q.z;
  } else {
    p[0] = x[3 * v], p[1] = x[3 * v + 1], p[2] = x[3 * v + 2];
  }
}

template <int STRIDE>
__global__ __launch_bounds__(256) void sm_step_kernel(const double* __restrict__ x_in, double* __restrict__ x_out,
                                                      const int64_t* __restrict__ row_start,
                                                      const int32_t* __restrict__ nbr, const int32_t* __restrict__ mult,
                                                      int nv, int64_t ne, double factor, int mode,
                                                      uint8_t* __restrict__ vclass) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const int64_t j0 = max(row_start[v], (int64_t)0), j1 = min(row_start[v + 1], ne);
  double sa[3] = {0.0, 0.0, 0.0}, sb[3] = {0.0, 0.0, 0.0};
  int na = 0, nb = 0;
  for (int64_t j = j0; j < j1; j++) {                 // ascending neighbour index: the keys were sorted
    const int u = nbr[j];
    if ((unsigned)u >= (unsigned)nv) continue;
    const bool rim = mult[j] == 1;
    double p[3];
    sm_load<STRIDE>(x_in, u, p);
#pragma unroll
    for (int d = 0; d < 3; d++) {
      sa[d] += p[d];
      if (rim) sb[d] += p[d];
    }
    na++;
    nb += rim ? 1 : 0;
  }
  double x[3];
  sm_load<STRIDE>(x_in, v, x);
  const bool isolated = na == 0, boundary = nb > 0;
  const bool along = boundary && mode == MSLAM_MESH_SMOOTH_CURVE;
  const bool moves = !isolated && !(boundary && mode == MSLAM_MESH_SMOOTH_FIXED);
  const double n = (double)(along ? nb : na);
  double r[3];
#pragma unroll
  for (int d = 0; d < 3; d++) r[d] = moves ? x[d] + factor * ((along ? sb[d] : sa[d]) / n - x[d]) : x[d];
  if (STRIDE == 4) {
    *reinterpret_cast<double4*>(x_out + 4 * v) = make_double4(r[0], r[1], r[2], 0.0);
  } else {
    x_out[3 * v] = r[0], x_out[3 * v + 1] = r[1], x_out[3 * v + 2] = r[2];
  }
  if (vclass) vclass[v] = isolated ? MSLAM_MESH_SMOOTH_ISOLATED : boundary ? MSLAM_MESH_SMOOTH_BOUNDARY
                                                                           : MSLAM_MESH_SMOOTH_INTERIOR;
}

__global__ __launch_bounds__(256) void sm_normals_kernel(const float* __restrict__ vert,
                                                         const int32_t* __restrict__ faces, int nf, int nv,
                                                         const int64_t* __restrict__ pairs,
                                                         const int64_t* __restrict__ pstart,
                                                         const float* __restrict__ nrm_in, float* __restrict__ nrm) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const int64_t j0 = max(pstart[v], (int64_t)0), j1 = min(pstart[v + 1], 3 * (int64_t)nf);
  double s[3] = {0.0, 0.0, 0.0};
  int n = 0;
  for (int64_t j = j0; j < j1; j++) {                 // ascending face index
    const int64_t f = pairs[j] - v * nf;
    if ((uint64_t)f >= (uint64_t)nf) continue;
    const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
    if (!tp_counts(ia, ib, ic, nv)) continue;
    double a[3], b[3], c[3], e1[3], e2[3], fn[3];
    tp_point(vert, ia, a), tp_point(vert, ib, b), tp_point(vert, ic, c);
    tp_sub(b, a, e1), tp_sub(c, a, e2);
    tp_cross(e1, e2, fn);
#pragma unroll
    for (int d = 0; d < 3; d++) s[d] += fn[d];
    n++;
  }
  const double ln = sqrt(tp_dot(s, s));
  const bool unit = ln > 0.0 && ln < (double)INFINITY;      // false when the sum is zero, infinite or NaN
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const size_t o = 3 * (size_t)v + d;
    nrm[o] = n == 0 ? (nrm_in ? nrm_in[o] : 0.0f) : unit ? (float)(s[d] / ln) : 0.0f;
  }
}

}  // namespace mslam

using namespace mslam;

extern "C" int mslam_mesh_smooth_edges(const int32_t* faces, int num_faces, int num_vertices, int64_t* keys,
                                       void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_smooth_edges: negative size");
  MSLAM_REQUIRE((int64_t)num_faces * 3 < ((int64_t)1 << 31), "mesh_smooth_edges: too many faces");
  if (num_faces == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && keys, "mesh_smooth_edges: null pointer");
  hipLaunchKernelGGL(sm_edges_kernel, dim3(blocks_for(num_faces, 256)), dim3(256), 0, (hipStream_t)stream, faces,
                     num_faces, num_vertices, keys);
  MSLAM_LAUNCH_CHECK("mesh_smooth_edges");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_smooth_step(const double* x_in, double* x_out, int stride, const int64_t* row_start,
                                      const int32_t* nbr, const int32_t* mult, int num_vertices, int64_t num_edges,
                                      double factor, int boundary_mode, uint8_t* vclass, void* stream) {
  MSLAM_REQUIRE(num_vertices >= 0 && num_edges >= 0, "mesh_smooth_step: negative size");
  MSLAM_REQUIRE(stride == 3 || stride == 4, "mesh_smooth_step: stride must be 3 or 4 doubles");
  MSLAM_REQUIRE(boundary_mode == MSLAM_MESH_SMOOTH_FIXED || boundary_mode == MSLAM_MESH_SMOOTH_CURVE ||
                    boundary_mode == MSLAM_MESH_SMOOTH_FREE,
                "mesh_smooth_step: unknown boundary mode");
  MSLAM_REQUIRE(isfinite(factor), "mesh_smooth_step: factor must be finite");
  if (num_vertices == 0) return MSLAM_OK;
  MSLAM_REQUIRE(x_in && x_out && x_in != x_out && row_start, "mesh_smooth_step: null pointer or x_out == x_in");
  MSLAM_REQUIRE(num_edges == 0 || (nbr && mult), "mesh_smooth_step: null pointer");
  MSLAM_REQUIRE(stride == 3 || ((uintptr_t)x_in % 32 == 0 && (uintptr_t)x_out % 32 == 0),
                "mesh_smooth_step: a stride of 4 needs 32-byte aligned states");
  const dim3 grid(blocks_for(num_vertices, 256)), block(256);
  if (stride == 4) {
    hipLaunchKernelGGL(sm_step_kernel<4>, grid, block, 0, (hipStream_t)stream, x_in, x_out, row_start, nbr, mult,
                       num_vertices, num_edges, factor, boundary_mode, vclass);
  } else {
    hipLaunchKernelGGL(sm_step_kernel<3>, grid, block, 0, (hipStream_t)stream, x_in, x_out, row_start, nbr, mult,
                       num_vertices, num_edges, factor, boundary_mode, vclass);
  }
  MSLAM_LAUNCH_CHECK("mesh_smooth_step");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_vertex_faces(const int32_t* faces, int num_faces, int num_vertices, int64_t* pairs,
                                       void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_vertex_faces: negative size");
  MSLAM_REQUIRE((int64_t)num_faces * 3 < ((int64_t)1 << 31), "mesh_vertex_faces: too many faces");
  if (num_faces == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && pairs, "mesh_vertex_faces: null pointer");
  hipLaunchKernelGGL(sm_faces_kernel, dim3(blocks_for(num_faces, 256)), dim3(256), 0, (hipStream_t)stream, faces,
                     num_faces, num_vertices, pairs);
  MSLAM_LAUNCH_CHECK("mesh_vertex_faces");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_vertex_normals(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                                         const int64_t* sorted_pairs, const int64_t* pair_start,
                                         const float* normals_in, float* normals, void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_vertex_normals: negative size");
  MSLAM_REQUIRE((int64_t)num_faces * 3 < ((int64_t)1 << 31), "mesh_vertex_normals: too many faces");
  if (num_vertices == 0) return MSLAM_OK;
  MSLAM_REQUIRE(vertices && pair_start && normals && normals != normals_in, "mesh_vertex_normals: null pointer");
  MSLAM_REQUIRE(num_faces == 0 || (faces && sorted_pairs), "mesh_vertex_normals: null pointer");
  hipLaunchKernelGGL(sm_normals_kernel, dim3(blocks_for(num_vertices, 256)), dim3(256), 0, (hipStream_t)stream,
                     vertices, faces, num_faces, num_vertices, sorted_pairs, pair_start, normals_in, normals);
  MSLAM_LAUNCH_CHECK("mesh_vertex_normals");
  return MSLAM_OK;
}
