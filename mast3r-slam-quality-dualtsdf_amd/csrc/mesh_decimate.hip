// Mesh decimation: round-based half-edge collapse with plane quadrics (Garland & Heckbert).  Semantics in DESIGN.md
// "Mesh decimation"; tests/decimate_numpy.py states the same definitions, operation by operation, in numpy.  The state
// is f64, the build has -ffp-contract=off, so every product and sum below is rounded on its own, in the order written.
//
//   state       one thread per vertex: the plane quadric (10 doubles) and the area of its counting faces, summed in
//               ascending face index over the (vertex, face) pairs of mslam_mesh_vertex_faces.
//   (caller)      every round: the neighbour table (mslam_mesh_smooth_edges, sort, unique) and the pairs of the
//               current faces.
//   candidates  one thread per vertex u: removable?  then, per neighbour v ascending, the cost of u -> v, the error
//               gate, the link condition (a merge of the two sorted rows) and the flip test over the faces of u; keeps
//               the lowest (cost, v).  Writes best, cost, the sort key (hash32(u, round), u) and the vertex class.
//   (caller)      ranks the candidates by (cost, key) with two stable sorts.
//   spread      one thread per vertex: the minimum of a rank over the closed neighbourhood.  Twice: a candidate whose
//               rank comes back is the lowest within two hops and is selected.
//   apply       one thread per face: every corner that is a selected u becomes best[u], in place; one thread per
//               selected u: state[best[u]] += state[u], parent[u] = best[u].  Selected vertices are three hops apart,
//               so no two threads touch one row and no row that is read is written (DESIGN.md has the argument).
//   finish      one thread per face: keep_face, and referenced = 1 at the corners of a counting face; one thread per
//               vertex: the end of its parent chain.  The caller scans the flags and calls mslam_mesh_cc_emit.
// No atomics.  Every index read from memory is checked against its array before it is followed; an element that fails
// is skipped.
#include <math.h>

#include "mesh_topo.h"

namespace mslam {

constexpr int kDmState = MSLAM_MESH_DECIMATE_STATE;       // doubles per vertex: 10 quadric entries, then the area

// the finaliser of MurmurHash3 over u and the round: tests/decimate_numpy.py hash32
__device__ __forceinline__ uint32_t dm_hash32(uint32_t u, uint32_t round) {
  uint32_t x = u * 0x9E3779B1u + round * 0x85EBCA77u;
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// (b - a) x (c - a)
__device__ __forceinline__ void dm_cross(const double (&a)[3], const double (&b)[3], const double (&c)[3],
                                         double (&n)[3]) {
  double e1[3], e2[3];
  tp_sub(b, a, e1), tp_sub(c, a, e2);
  tp_cross(e1, e2, n);
}

__global__ __launch_bounds__(256) void dm_state_kernel(const float* __restrict__ vert,
                                                       const int32_t* __restrict__ faces, int nf, int nv,
                                                       const int64_t* __restrict__ pairs,
                                                       const int64_t* __restrict__ pstart, double* __restrict__ state) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const int64_t j0 = max(pstart[v], (int64_t)0), j1 = min(pstart[v + 1], 3 * (int64_t)nf);
  double s[kDmState];
#pragma unroll
  for (int k = 0; k < kDmState; k++) s[k] = 0.0;
  for (int64_t j = j0; j < j1; j++) {                 // ascending face index
    const int64_t f = pairs[j] - v * nf;
    if ((uint64_t)f >= (uint64_t)nf) continue;
    const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
    if (!tp_counts(ia, ib, ic, nv)) continue;
    double a[3], b[3], c[3], n[3];
    tp_point(vert, ia, a), tp_point(vert, ib, b), tp_point(vert, ic, c);
    dm_cross(a, b, c, n);
    const double ln = sqrt(tp_dot(n, n));
    if (!(ln > 0.0 && ln < (double)INFINITY)) continue;
    const double kx = n[0] / ln, ky = n[1] / ln, kz = n[2] / ln, area = 0.5 * ln;
    const double g[4] = {kx, ky, kz, -((kx * a[0] + ky * a[1]) + kz * a[2])};
    int k = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const double w = area * g[i];
#pragma unroll
      for (int jj = i; jj < 4; jj++) s[k] += w * g[jj], k++;
    }
    s[10] += area;
  }
#pragma unroll
  for (int k = 0; k < kDmState; k++) state[kDmState * v + k] = s[k];
}

__global__ __launch_bounds__(256) void dm_candidates_kernel(
    const float* __restrict__ vert, const int32_t* __restrict__ faces, int nf, int nv,
    const int64_t* __restrict__ row_start, const int32_t* __restrict__ nbr, const int32_t* __restrict__ mult, int64_t ne,
    const int64_t* __restrict__ pairs, const int64_t* __restrict__ pstart, const double* __restrict__ state, double gate,
    uint32_t round, int32_t* __restrict__ best, double* __restrict__ cost, int64_t* __restrict__ key,
    uint8_t* __restrict__ vclass) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= nv) return;
  const int64_t j0 = max(row_start[u], (int64_t)0), j1 = max(min(row_start[u + 1], ne), j0);
  const int64_t p0 = max(pstart[u], (int64_t)0), p1 = max(min(pstart[u + 1], 3 * (int64_t)nf), p0);
  int odd = 0, rim = 0;
  for (int64_t j = j0; j < j1; j++) {
    const int m = mult[j];
    odd += m != 2 ? 1 : 0;
    rim += m == 1 ? 1 : 0;
  }
  const bool removable = j1 > j0 && odd == 0 && p1 - p0 == j1 - j0;
  if (vclass) {
    vclass[u] = j1 == j0 ? MSLAM_MESH_DECIMATE_ISOLATED : rim > 0 ? MSLAM_MESH_DECIMATE_BOUNDARY
                         : removable ? MSLAM_MESH_DECIMATE_REMOVABLE : MSLAM_MESH_DECIMATE_OTHER;
  }
  int bestv = -1;
  double bestc = (double)INFINITY;
  if (removable) {
    double su[kDmState];
#pragma unroll
    for (int k = 0; k < kDmState; k++) su[k] = state[kDmState * u + k];
    for (int64_t j = j0; j < j1; j++) {               // ascending v: a tie in cost keeps the lower v
      const int v = nbr[j];
      if ((unsigned)v >= (unsigned)nv) continue;
      double q[kDmState], h[3];
#pragma unroll
      for (int k = 0; k < kDmState; k++) q[k] = su[k] + state[kDmState * (int64_t)v + k];
      tp_point(vert, v, h);
      const double x = h[0], y = h[1], z = h[2];
      const double r0 = ((q[0] * x + q[1] * y) + q[2] * z) + q[3];
      const double r1 = ((q[1] * x + q[4] * y) + q[5] * z) + q[6];
      const double r2 = ((q[2] * x + q[5] * y) + q[7] * z) + q[8];
      const double r3 = ((q[3] * x + q[6] * y) + q[8] * z) + q[9];
      const double c = ((r0 * x + r1 * y) + r2 * z) + r3;
      const double cv = c > 0.0 ? c : 0.0;
      if (!(cv < bestc)) continue;
      if (gate >= 0.0 && !(cv <= gate * q[10])) continue;
      // link: exactly two vertices in both rows, each sorted ascending, neither a closed fan of three faces or fewer
      const int64_t k0 = max(row_start[v], (int64_t)0), k1 = min(row_start[v + 1], ne);
      int common = 0;
      bool thin = false;
      for (int64_t i = j0, k = k0; i < j1 && k < k1;) {
        const int a = nbr[i], b = nbr[k];
        if (a == b) {
          common++;
          if ((unsigned)a < (unsigned)nv) {
            const int64_t deg = row_start[a + 1] - row_start[a];
            thin |= deg <= 3 && pstart[a + 1] - pstart[a] == deg;
          }
        }
        i += a <= b ? 1 : 0;
        k += b <= a ? 1 : 0;
      }
      if (common != 2 || thin) continue;
      // flip: every face of u that does not hold v keeps its side and its area
      bool ok = true;
      for (int64_t i = p0; i < p1 && ok; i++) {
        const int64_t f = pairs[i] - u * nf;
        if ((uint64_t)f >= (uint64_t)nf) continue;
        const int t[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
        if (!tp_counts(t[0], t[1], t[2], nv)) continue;
        if (t[0] == v || t[1] == v || t[2] == v) continue;
        double p[3][3], w[3][3], o[3], n[3];
#pragma unroll
        for (int d = 0; d < 3; d++) {
          tp_point(vert, t[d], p[d]);
#pragma unroll
          for (int e = 0; e < 3; e++) w[d][e] = t[d] == (int)u ? h[e] : p[d][e];
        }
        dm_cross(p[0], p[1], p[2], o);
        dm_cross(w[0], w[1], w[2], n);
        ok = tp_dot(n, o) > 0.0;
      }
      if (!ok) continue;
      bestc = cv, bestv = v;
    }
  }
  best[u] = bestv;
  cost[u] = bestc;
  key[u] = bestv >= 0 ? (int64_t)(((uint64_t)dm_hash32((uint32_t)u, round) << 31) | (uint64_t)u) : INT64_MAX;
}

__global__ __launch_bounds__(256) void dm_spread_kernel(const int32_t* __restrict__ in,
                                                        const int64_t* __restrict__ row_start,
                                                        const int32_t* __restrict__ nbr, int nv, int64_t ne,
                                                        int32_t* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const int64_t j0 = max(row_start[v], (int64_t)0), j1 = min(row_start[v + 1], ne);
  int32_t m = in[v];
  for (int64_t j = j0; j < j1; j++) {
    const int w = nbr[j];
    if ((unsigned)w < (unsigned)nv) m = min(m, in[w]);
  }
  out[v] = m;
}

__global__ __launch_bounds__(256) void dm_apply_faces_kernel(int32_t* __restrict__ faces, int nf, int nv,
                                                             const uint8_t* __restrict__ selected,
                                                             const int32_t* __restrict__ best) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const int a = faces[3 * (size_t)f + d];
    if ((unsigned)a >= (unsigned)nv || !selected[a]) continue;
    const int v = best[a];
    if ((unsigned)v < (unsigned)nv) faces[3 * (size_t)f + d] = v;
  }
}

__global__ __launch_bounds__(256) void dm_apply_state_kernel(int nv, const uint8_t* __restrict__ selected,
                                                             const int32_t* __restrict__ best,
                                                             double* __restrict__ state, int32_t* __restrict__ parent) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= nv || !selected[u]) return;
  const int v = best[u];
  if ((unsigned)v >= (unsigned)nv || v == (int)u) return;
#pragma unroll
  for (int k = 0; k < kDmState; k++) state[kDmState * (int64_t)v + k] += state[kDmState * u + k];
  parent[u] = v;
}

__global__ __launch_bounds__(256) void dm_finish_kernel(const int32_t* __restrict__ faces, int nf, int nv,
                                                        const int32_t* __restrict__ parent, int max_steps,
                                                        int32_t* __restrict__ keep_face,
                                                        int32_t* __restrict__ referenced, int32_t* __restrict__ end) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nf) {
    const int a = faces[3 * (size_t)i], b = faces[3 * (size_t)i + 1], c = faces[3 * (size_t)i + 2];
    const bool ok = tp_counts(a, b, c, nv);
    keep_face[i] = ok ? 1 : 0;
    if (ok) referenced[a] = 1, referenced[b] = 1, referenced[c] = 1;      // every writer writes the same value
  }
  if (i < nv) {
    int w = i;
    for (int s = 0; s < max_steps; s++) {             // a chain grows by at most one link per round
      const int p = parent[w];
      if ((unsigned)p >= (unsigned)nv || p == w) break;
      w = p;
    }
    end[i] = w;
  }
}

}  // namespace mslam

using namespace mslam;

extern "C" int mslam_mesh_decimate_state(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                                         const int64_t* sorted_pairs, const int64_t* pair_start, double* state,
                                         void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_decimate_state: negative size");
  MSLAM_REQUIRE((int64_t)num_faces * 3 < ((int64_t)1 << 31), "mesh_decimate_state: too many faces");
  if (num_vertices == 0) return MSLAM_OK;
  MSLAM_REQUIRE(vertices && pair_start && state, "mesh_decimate_state: null pointer");
  MSLAM_REQUIRE(num_faces == 0 || (faces && sorted_pairs), "mesh_decimate_state: null pointer");
  hipLaunchKernelGGL(dm_state_kernel, dim3(blocks_for(num_vertices, 256)), dim3(256), 0, (hipStream_t)stream, vertices,
                     faces, num_faces, num_vertices, sorted_pairs, pair_start, state);
  MSLAM_LAUNCH_CHECK("mesh_decimate_state");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_decimate_candidates(const float* vertices, const int32_t* faces, int num_faces,
                                              int num_vertices, const int64_t* row_start, const int32_t* nbr,
                                              const int32_t* mult, int64_t num_edges, const int64_t* sorted_pairs,
                                              const int64_t* pair_start, const double* state, double gate, int round,
                                              int32_t* best, double* cost, int64_t* key, uint8_t* vclass,
                                              void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0 && num_edges >= 0 && round >= 0,
                "mesh_decimate_candidates: negative size");
  MSLAM_REQUIRE((int64_t)num_faces * 3 < ((int64_t)1 << 31), "mesh_decimate_candidates: too many faces");
  MSLAM_REQUIRE(!isnan(gate), "mesh_decimate_candidates: the gate is NaN");
  if (num_vertices == 0) return MSLAM_OK;
  MSLAM_REQUIRE(vertices && row_start && pair_start && state && best && cost && key,
                "mesh_decimate_candidates: null pointer");
  MSLAM_REQUIRE(num_edges == 0 || (nbr && mult), "mesh_decimate_candidates: null pointer");
  MSLAM_REQUIRE(num_faces == 0 || (faces && sorted_pairs), "mesh_decimate_candidates: null pointer");
  hipLaunchKernelGGL(dm_candidates_kernel, dim3(blocks_for(num_vertices, 256)), dim3(256), 0, (hipStream_t)stream,
                     vertices, faces, num_faces, num_vertices, row_start, nbr, mult, num_edges, sorted_pairs, pair_start,
                     state, gate, (uint32_t)round, best, cost, key, vclass);
  MSLAM_LAUNCH_CHECK("mesh_decimate_candidates");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_decimate_spread(const int32_t* rank_in, const int64_t* row_start, const int32_t* nbr,
                                          int num_vertices, int64_t num_edges, int32_t* rank_out, void* stream) {
  MSLAM_REQUIRE(num_vertices >= 0 && num_edges >= 0, "mesh_decimate_spread: negative size");
  if (num_vertices == 0) return MSLAM_OK;
  MSLAM_REQUIRE(rank_in && row_start && rank_out && rank_in != rank_out,
                "mesh_decimate_spread: null pointer or rank_out == rank_in");
  MSLAM_REQUIRE(num_edges == 0 || nbr, "mesh_decimate_spread: null pointer");
  hipLaunchKernelGGL(dm_spread_kernel, dim3(blocks_for(num_vertices, 256)), dim3(256), 0, (hipStream_t)stream, rank_in,
                     row_start, nbr, num_vertices, num_edges, rank_out);
  MSLAM_LAUNCH_CHECK("mesh_decimate_spread");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_decimate_apply(int32_t* faces, int num_faces, int num_vertices, const uint8_t* selected,
                                         const int32_t* best, double* state, int32_t* parent, void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_decimate_apply: negative size");
  MSLAM_REQUIRE((int64_t)num_faces * 3 < ((int64_t)1 << 31), "mesh_decimate_apply: too many faces");
  if (num_vertices == 0) return MSLAM_OK;
  MSLAM_REQUIRE(selected && best && state && parent, "mesh_decimate_apply: null pointer");
  MSLAM_REQUIRE(num_faces == 0 || faces, "mesh_decimate_apply: null pointer");
  if (num_faces > 0) {
    hipLaunchKernelGGL(dm_apply_faces_kernel, dim3(blocks_for(num_faces, 256)), dim3(256), 0, (hipStream_t)stream,
                       faces, num_faces, num_vertices, selected, best);
    MSLAM_LAUNCH_CHECK("mesh_decimate_apply faces");
  }
  hipLaunchKernelGGL(dm_apply_state_kernel, dim3(blocks_for(num_vertices, 256)), dim3(256), 0, (hipStream_t)stream,
                     num_vertices, selected, best, state, parent);
  MSLAM_LAUNCH_CHECK("mesh_decimate_apply state");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_decimate_finish(const int32_t* faces, int num_faces, int num_vertices, const int32_t* parent,
                                          int max_steps, int32_t* keep_face, int32_t* referenced, int32_t* end,
                                          void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0 && max_steps >= 0, "mesh_decimate_finish: negative size");
  MSLAM_REQUIRE((int64_t)num_faces * 3 < ((int64_t)1 << 31), "mesh_decimate_finish: too many faces");
  const int n = num_vertices > num_faces ? num_vertices : num_faces;
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(num_vertices == 0 || (parent && referenced && end), "mesh_decimate_finish: null pointer");
  MSLAM_REQUIRE(num_faces == 0 || (faces && keep_face), "mesh_decimate_finish: null pointer");
  hipLaunchKernelGGL(dm_finish_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, faces, num_faces,
                     num_vertices, parent, max_steps, keep_face, referenced, end);
  MSLAM_LAUNCH_CHECK("mesh_decimate_finish");
  return MSLAM_OK;
}
