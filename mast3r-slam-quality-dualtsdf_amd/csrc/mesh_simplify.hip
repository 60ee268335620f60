// Mesh simplification by vertex clustering on a uniform grid with quadric placement (Lindstrom, "Out-of-core
// simplification of large polygonal models").  Semantics in DESIGN.md "Mesh simplification"; tests/simplify_numpy.py
// states the same definitions, operation by operation, in numpy.  Everything is f64 on the f32 inputs and the build has
// -ffp-contract=off, so a * b + c below is two roundings, as in numpy.
//
//   keys    one thread per vertex: the packed key of its cell floor(p / c) (21 bits per axis, lexicographic x, y, z).
//   (caller)  stable sort of the keys; head flags and a cumsum number the clusters 0..C-1 in key order and give every
//           vertex its cluster; the first sorted position of every cluster (vstart).
//   faces   one thread per face: its three clusters, the rotated triple (-1 when the face collapses), the sort key(s) of
//           the triple, and one (cluster, face) pair key cluster * F + face per distinct cluster of the face.
//   (caller)  sorts the pair keys (-> pstart, the first pair of every cluster) and the triple keys (-> the face order).
//   solve   one thread per cluster: walks its vertex run in ascending vertex index (mean, normal, colour), its pair run
//           in ascending face index (the plane quadric), diagonalises the quadric and writes position, normal, colour.
//   mark    one thread per sorted face: the triple in sorted order, keep = live and unlike its predecessor, and a 1 at
//           every cluster a kept face references.
//   (caller)  exclusive scans of the flags (torch.cumsum), one host read of the output sizes; mslam_mesh_cc_emit then
//           gathers the referenced clusters and rewrites the faces.
// No floating-point atomics, no output offset from a counter at a single address, and no thread reads what another
// writes within a launch: every sum has one fixed order, so the same input gives the same bits.  Every index read from
// memory is checked against its array before it is followed; an element that fails is skipped.
#include <math.h>

#include "mesh_topo.h"

namespace mslam {

constexpr int64_t kMsBias = 1 << 20;                  // the voxel hash's key range per axis: [-2^20, 2^20)
constexpr int64_t kMsNone = INT64_MAX;
constexpr int kMsSweeps = 8;                          // cyclic Jacobi on a 3 x 3: converged to rounding after 5
constexpr double kMsEigRel = 1.0e-3;                  // directions with lambda <= this * lambda_max keep the mean

__global__ __launch_bounds__(256) void ms_keys_kernel(const float* __restrict__ vert, int nv, double cell,
                                                      int64_t* __restrict__ keys) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  int64_t key = 0;
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const double q = floor((double)vert[3 * (size_t)v + d] / cell);
    const bool in = q >= (double)-kMsBias && q < (double)kMsBias;      // false for NaN
    ok = ok && in;
    key = (key << 21) | (in ? (int64_t)q + kMsBias : 0);
  }
  keys[v] = ok ? key : kMsNone;
}

__global__ __launch_bounds__(256) void ms_faces_kernel(const int32_t* __restrict__ faces, int nf, int nv,
                                                       const int32_t* __restrict__ cluster, int nc, int packed,
                                                       int32_t* __restrict__ tri, int64_t* __restrict__ key_hi,
                                                       int64_t* __restrict__ key_lo, int64_t* __restrict__ pairs) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
  int ca = -1, cb = -1, cc = -1;
  if (tp_in_range(a, b, c, nv)) {
    ca = cluster[a], cb = cluster[b], cc = cluster[c];
  }
  const bool ok = (unsigned)ca < (unsigned)nc && (unsigned)cb < (unsigned)nc && (unsigned)cc < (unsigned)nc;
  const bool live = ok && ca != cb && cb != cc && ca != cc;
  pairs[3 * (size_t)f] = ok ? (int64_t)ca * nf + f : kMsNone;
  pairs[3 * (size_t)f + 1] = ok && cb != ca ? (int64_t)cb * nf + f : kMsNone;
  pairs[3 * (size_t)f + 2] = ok && cc != ca && cc != cb ? (int64_t)cc * nf + f : kMsNone;
  int t0 = ca, t1 = cb, t2 = cc;                      // rotated so that the smallest id is first: orientation kept
  if (cb < ca && cb < cc) {
    t0 = cb, t1 = cc, t2 = ca;
  } else if (cc < ca && cc < cb) {
    t0 = cc, t1 = ca, t2 = cb;
  }
  tri[3 * (size_t)f] = live ? t0 : -1;
  tri[3 * (size_t)f + 1] = live ? t1 : -1;
  tri[3 * (size_t)f + 2] = live ? t2 : -1;
  if (packed) {
    key_lo[f] = live ? ((int64_t)t0 * nc + t1) * nc + t2 : kMsNone;
  } else {
    key_lo[f] = live ? (int64_t)t1 * nc + t2 : kMsNone;
    key_hi[f] = live ? (int64_t)t0 : kMsNone;
  }
}

// One Jacobi rotation that zeroes a[P][Q]; the columns of v collect the rotations.
template <int P, int Q>
__device__ __forceinline__ void ms_rotate(double (&a)[3][3], double (&v)[3][3]) {
  constexpr int R = 3 - P - Q;
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const double arp = a[R][P], arq = a[R][Q];
  a[P][P] = a[P][P] - t * apq;
  a[Q][Q] = a[Q][Q] + t * apq;
  a[P][Q] = a[Q][P] = 0.0;
  a[R][P] = a[P][R] = c * arp - s * arq;
  a[R][Q] = a[Q][R] = s * arp + c * arq;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double vp = v[k][P], vq = v[k][Q];
    v[k][P] = c * vp - s * vq;
    v[k][Q] = s * vp + c * vq;
  }
}

__global__ __launch_bounds__(64) void ms_solve_kernel(
    const float* __restrict__ vert, const float* __restrict__ nrm, const float* __restrict__ col,
    const int32_t* __restrict__ faces, int nf, int nv, double cell, const int64_t* __restrict__ sorted_keys,
    const int64_t* __restrict__ vorder, const int64_t* __restrict__ vstart, const int64_t* __restrict__ pairs,
    const int64_t* __restrict__ pstart, int nc, int quadric, float* __restrict__ out_pos, float* __restrict__ out_nrm,
    float* __restrict__ out_col, int32_t* __restrict__ out_fallback) {
  const int cl = blockIdx.x * 64 + threadIdx.x;
  if (cl >= nc) return;
  const size_t o = 3 * (size_t)cl;
  const int64_t i0 = max(vstart[cl], (int64_t)0), i1 = min(vstart[cl + 1], (int64_t)nv);
  double x0[3] = {0.0, 0.0, 0.0}, s[3] = {0.0, 0.0, 0.0}, sn[3] = {0.0, 0.0, 0.0}, sc[3] = {0.0, 0.0, 0.0};
  int n = 0;
  if (i0 < i1) {
    const int64_t key = sorted_keys[i0];
#pragma unroll
    for (int d = 0; d < 3; d++)
      x0[d] = ((double)(((key >> (21 * (2 - d))) & 0x1FFFFF) - kMsBias) + 0.5) * cell;
  }
  for (int64_t i = i0; i < i1; i++) {                 // ascending vertex index: the sort was stable
    const int64_t v = vorder[i];
    if ((uint64_t)v >= (uint64_t)nv) continue;
#pragma unroll
    for (int d = 0; d < 3; d++) {
      s[d] += (double)vert[3 * v + d] - x0[d];
      sn[d] += (double)nrm[3 * v + d];
      if (col) sc[d] += (double)col[3 * v + d];
    }
    n++;
  }
  if (n == 0) {                                       // not a cluster: only on inconsistent input
#pragma unroll
    for (int d = 0; d < 3; d++) {
      out_pos[o + d] = 0.0f, out_nrm[o + d] = 0.0f;
      if (col) out_col[o + d] = 0.0f;
    }
    if (out_fallback) out_fallback[cl] = 1;
    return;
  }
  double m[3], x[3];
#pragma unroll
  for (int d = 0; d < 3; d++) x[d] = m[d] = s[d] / (double)n;
  bool fallback = true;
  if (quadric) {
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};      // xx, xy, xz, yy, yz, zz
    const int64_t j0 = max(pstart[cl], (int64_t)0), j1 = min(pstart[cl + 1], 3 * (int64_t)nf);
    for (int64_t j = j0; j < j1; j++) {               // ascending face index
      const int64_t f = pairs[j] - (int64_t)cl * nf;
      if ((uint64_t)f >= (uint64_t)nf) continue;
      const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
      if (!tp_in_range(ia, ib, ic, nv)) continue;
      double a[3], pb[3], pc[3], e1[3], e2[3], nn[3];
      tp_point(vert, ia, a), tp_point(vert, ib, pb), tp_point(vert, ic, pc);
      tp_sub(pb, a, e1), tp_sub(pc, a, e2);
      tp_cross(e1, e2, nn);
      const double nx = nn[0], ny = nn[1], nz = nn[2];
      if (nx == 0.0 && ny == 0.0 && nz == 0.0) continue;       // mslam_mesh_face_areas' validity rule
      const double ln = sqrt(nx * nx + ny * ny + nz * nz), w = 0.5 * ln;
      const double u[3] = {nx / ln, ny / ln, nz / ln};
      const double wu[3] = {w * u[0], w * u[1], w * u[2]};
      const double dd = -(u[0] * (a[0] - x0[0]) + u[1] * (a[1] - x0[1]) + u[2] * (a[2] - x0[2]));
      A[0] += wu[0] * u[0], A[1] += wu[0] * u[1], A[2] += wu[0] * u[2];
      A[3] += wu[1] * u[1], A[4] += wu[1] * u[2], A[5] += wu[2] * u[2];
      b[0] += wu[0] * dd, b[1] += wu[1] * dd, b[2] += wu[2] * dd;
    }
    double q[3][3] = {{A[0], A[1], A[2]}, {A[1], A[3], A[4]}, {A[2], A[4], A[5]}};
    double r[3], e[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
    for (int d = 0; d < 3; d++) r[d] = -b[d] - (q[d][0] * m[0] + q[d][1] * m[1] + q[d][2] * m[2]);
    for (int sweep = 0; sweep < kMsSweeps; sweep++) {
      ms_rotate<0, 1>(q, e);
      ms_rotate<0, 2>(q, e);
      ms_rotate<1, 2>(q, e);
    }
    const double lmax = fmax(fmax(q[0][0], q[1][1]), q[2][2]);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      if (q[i][i] > kMsEigRel * lmax) {               // false for NaN
        const double g = (e[0][i] * r[0] + e[1][i] * r[1] + e[2][i] * r[2]) / q[i][i];
#pragma unroll
        for (int d = 0; d < 3; d++) x[d] += e[d][i] * g;
      }
    }
    fallback = !(lmax > 0.0);
#pragma unroll
    for (int d = 0; d < 3; d++) fallback = fallback || !(fabs(x[d]) <= 0.5 * cell);      // also when x is not finite
    if (fallback) {
#pragma unroll
      for (int d = 0; d < 3; d++) x[d] = m[d];
    }
  }
  const double ln = sqrt(sn[0] * sn[0] + sn[1] * sn[1] + sn[2] * sn[2]);
#pragma unroll
  for (int d = 0; d < 3; d++) {
    out_pos[o + d] = (float)(x0[d] + x[d]);
    out_nrm[o + d] = ln > 0.0 ? (float)(sn[d] / ln) : 0.0f;
    if (col) out_col[o + d] = (float)(sc[d] / (double)n);
  }
  if (out_fallback) out_fallback[cl] = fallback ? 1 : 0;
}

__global__ __launch_bounds__(256) void ms_mark_kernel(const int32_t* __restrict__ tri,
                                                      const int64_t* __restrict__ order, int nf, int nc,
                                                      int32_t* __restrict__ sorted_tri,
                                                      int32_t* __restrict__ keep_face, int32_t* referenced) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nf) return;
  int t[3] = {-1, -1, -1}, p[3] = {-1, -1, -1};
  const int64_t f = order[j];
  if ((uint64_t)f < (uint64_t)nf) {
#pragma unroll
    for (int d = 0; d < 3; d++) t[d] = tri[3 * f + d];
  }
  if (j > 0) {
    const int64_t g = order[j - 1];
    if ((uint64_t)g < (uint64_t)nf) {
#pragma unroll
      for (int d = 0; d < 3; d++) p[d] = tri[3 * g + d];
    }
  }
  const bool live = (unsigned)t[0] < (unsigned)nc && (unsigned)t[1] < (unsigned)nc && (unsigned)t[2] < (unsigned)nc;
  const bool keep = live && !(t[0] == p[0] && t[1] == p[1] && t[2] == p[2]);
#pragma unroll
  for (int d = 0; d < 3; d++) {
    sorted_tri[3 * (size_t)j + d] = live ? t[d] : 0;
    if (keep) referenced[t[d]] = 1;                   // the same value from every writer
  }
  keep_face[j] = keep ? 1 : 0;
}

}  // namespace mslam

using namespace mslam;

extern "C" int mslam_mesh_simplify_keys(const float* vertices, int num_vertices, double cell_size, int64_t* keys,
                                        void* stream) {
  MSLAM_REQUIRE(num_vertices >= 0, "mesh_simplify_keys: negative size");
  MSLAM_REQUIRE(cell_size > 0.0 && isfinite(cell_size), "mesh_simplify_keys: cell_size must be finite and positive");
  if (num_vertices == 0) return MSLAM_OK;
  MSLAM_REQUIRE(vertices && keys, "mesh_simplify_keys: null pointer");
  hipLaunchKernelGGL(ms_keys_kernel, dim3(blocks_for(num_vertices, 256)), dim3(256), 0, (hipStream_t)stream, vertices,
                     num_vertices, cell_size, keys);
  MSLAM_LAUNCH_CHECK("mesh_simplify_keys");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_simplify_faces(const int32_t* faces, int num_faces, int num_vertices, const int32_t* cluster,
                                         int num_clusters, int packed, int32_t* tri, int64_t* key_hi, int64_t* key_lo,
                                         int64_t* pairs, void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0 && num_clusters >= 0, "mesh_simplify_faces: negative size");
  MSLAM_REQUIRE((int64_t)num_faces * 3 < ((int64_t)1 << 31), "mesh_simplify_faces: too many faces");
  MSLAM_REQUIRE((double)num_clusters * (double)num_faces < 4.0e18, "mesh_simplify_faces: pair keys overflow");
  MSLAM_REQUIRE(!packed || (double)num_clusters * (double)num_clusters * (double)num_clusters < 4.0e18,
                "mesh_simplify_faces: packed triple keys overflow");
  if (num_faces == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && tri && key_lo && pairs && (cluster || num_vertices == 0) && (key_hi || packed),
                "mesh_simplify_faces: null pointer");
  hipLaunchKernelGGL(ms_faces_kernel, dim3(blocks_for(num_faces, 256)), dim3(256), 0, (hipStream_t)stream, faces,
                     num_faces, num_vertices, cluster, num_clusters, packed, tri, key_hi, key_lo, pairs);
  MSLAM_LAUNCH_CHECK("mesh_simplify_faces");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_simplify_solve(const float* vertices, const float* normals, const float* colors,
                                         const int32_t* faces, int num_faces, int num_vertices, double cell_size,
                                         const int64_t* sorted_keys, const int64_t* vertex_order,
                                         const int64_t* vertex_start, const int64_t* sorted_pairs,
                                         const int64_t* pair_start, int num_clusters, int quadric, float* out_vertices,
                                         float* out_normals, float* out_colors, int32_t* out_fallback, void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0 && num_clusters >= 0, "mesh_simplify_solve: negative size");
  MSLAM_REQUIRE(num_clusters <= num_vertices, "mesh_simplify_solve: more clusters than vertices");
  MSLAM_REQUIRE(cell_size > 0.0 && isfinite(cell_size), "mesh_simplify_solve: cell_size must be finite and positive");
  MSLAM_REQUIRE((int64_t)num_faces * 3 < ((int64_t)1 << 31), "mesh_simplify_solve: too many faces");
  if (num_clusters == 0) return MSLAM_OK;
  MSLAM_REQUIRE(vertices && normals && sorted_keys && vertex_order && vertex_start && out_vertices && out_normals,
                "mesh_simplify_solve: null pointer");
  MSLAM_REQUIRE((colors == nullptr) == (out_colors == nullptr), "mesh_simplify_solve: colours need an input and an output");
  MSLAM_REQUIRE(!quadric || num_faces == 0 || (faces && sorted_pairs && pair_start), "mesh_simplify_solve: null pointer");
  hipLaunchKernelGGL(ms_solve_kernel, dim3(blocks_for(num_clusters, 64)), dim3(64), 0, (hipStream_t)stream, vertices,
                     normals, colors, faces, num_faces, num_vertices, cell_size, sorted_keys, vertex_order,
                     vertex_start, sorted_pairs, pair_start, num_clusters, quadric && num_faces > 0 ? 1 : 0,
                     out_vertices, out_normals, out_colors, out_fallback);
  MSLAM_LAUNCH_CHECK("mesh_simplify_solve");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_simplify_mark(const int32_t* tri, const int64_t* face_order, int num_faces, int num_clusters,
                                        int32_t* sorted_tri, int32_t* keep_face, int32_t* referenced, void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_clusters >= 0, "mesh_simplify_mark: negative size");
  if (num_faces == 0) return MSLAM_OK;
  MSLAM_REQUIRE(tri && face_order && sorted_tri && keep_face && (referenced || num_clusters == 0),
                "mesh_simplify_mark: null pointer");
  hipLaunchKernelGGL(ms_mark_kernel, dim3(blocks_for(num_faces, 256)), dim3(256), 0, (hipStream_t)stream, tri,
                     face_order, num_faces, num_clusters, sorted_tri, keep_face, referenced);
  MSLAM_LAUNCH_CHECK("mesh_simplify_mark");
  return MSLAM_OK;
}
